// sap_rows.h -- the per-lane arithmetic of GM17's R1CS -> SAP maps (include/ginger_hip_sap.h), free of HIP: the shape of the
// SAP instance of an R1CS one, one lane of the witness rows (gm17/r1cs_to_sap.rs:125-189, :206-232) and one row of
// instance_map_with_evaluation's result (:37-94).  r1cs.hip's kernels are these functions behind a thread index, and the CPU
// tests run the same text over the host executor's products (tests/host_shim/sap_shim.cpp, sap_check.cpp under the host
// sanitizers).  DESIGN.md section 16a.
//
// Forms.  Every vector here is rows of 24 words in the ABI's Montgomery form (x 2^768), canonical (below the modulus).  Sums,
// differences and small multiples are the same limbs in any Montgomery form, so they are formed on the unpacked ABI limbs
// without a product; only the square of a constraint (and of an input) goes through the internal form: one product in, the
// square, one product out, and one more for into_repr where a scalar destination is given.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fp29.h"

namespace gh {

// The SAP instance of an R1CS instance of ni inputs (the constant one included), na aux variables and nc constraints.
struct SapShape {
    uint64_t ni = 0, nc = 0, nv = 0;             // nv = ni + na
    uint64_t N = 0;                              // the SAP domain, a power of two >= domain_arg()
    GH_HD uint64_t domain_arg() const { return 2 * nc + 2 * (ni - 1) + 1; }       // r1cs_to_sap.rs:18-21, :151-155
    GH_HD uint64_t sap_nv() const { return 2 * (ni - 1) + (nv - ni) + nc; }       // :30-31
    GH_HD uint64_t full_rows() const { return sap_nv() + 1; }                     // z || e || f
    GH_HD uint64_t aux_rows() const { return sap_nv() - (ni - 1); }               // full[ni ..]
    GH_HD uint64_t rows_lanes() const { return nc + ni + (N - domain_arg()); }    // sap_rows_lane: one per constraint, per input, per padding row
};

GH_HD void sap_store_zero(uint32_t* dst) {
    GH_UNROLL for (int k = 0; k < 24; k++) dst[k] = 0;
}

// x, y, w: unpacked ABI rows.  -> s = x + y, d = x - y, sq = (x - y)^2, c = 4 w + sq, all in the ABI's form; with want_repr,
// repr = into_repr of the square, the integer itself (a flag and a reference: a nullable pointer would put repr on the stack).
template <class P> GH_HD void sap_pair(const Fp& x, const Fp& y, const Fp& w, Fp& s, Fp& d, Fp& sq, Fp& c, bool want_repr, Fp& repr) {
    s = fp_add<P>(x, y);
    d = fp_sub<P>(x, y);
    const Fp e = fp_sqr<P>(fp_mul<P>(d, fp_const<P>(P::CIN)));              // internal form
    sq = fp_mul<P>(e, fp_const<P>(P::COUT));
    c = fp_add<P>(fp_dbl<P>(fp_dbl<P>(w)), sq);
    if (want_repr) {
        Fp one = fp_zero();
        one.l[0] = 1;
        repr = fp_mul<P>(e, one);
    }
}

// Lane t < sh.rows_lanes() of the witness rows.  az, bz, cz: the three products (nc rows each), z: the assignment (nv rows);
// a, c: N rows each; scalars (nullable): sap_nv rows, into_repr of full[1 ..]; aux (nullable): aux_rows() rows, the same of
// full[ni ..]; full (nullable): full_rows() Montgomery rows.  This lane writes the rows of e and f only: the rows of z in
// scalars / aux / full are the conversion's (r1cs_convert_kernel) or the caller's copy.
//   t < nc:               constraint t: a[2t], a[2t + 1], c[2t], c[2t + 1], e_t
//   t = nc:               a[2 nc] = c[2 nc] = one
//   nc < t < nc + ni:     input i = t - nc: rows 2 nc + 2 i - 1 and 2 nc + 2 i of both, f_i
//   the rest:             one zero row of both, from row domain_arg() on
template <class P>
GH_HD void sap_rows_lane(const SapShape& sh, uint64_t t, const uint32_t* az, const uint32_t* bz, const uint32_t* cz, const uint32_t* z,
                         uint32_t* a, uint32_t* c, uint32_t* scalars, uint32_t* aux, uint32_t* full) {
    const uint64_t nc = sh.nc, ni = sh.ni;
    if (t > nc + ni - 1 || t == nc) {
        const uint64_t row = t == nc ? 2 * nc : sh.domain_arg() + (t - nc - ni);
        if (t == nc) {
            const Fp one = fp_const<P>(P::COUT);                             // 2^768 mod p: one in the ABI's form
            fp_pack(a + row * 24, one);
            fp_pack(c + row * 24, one);
        } else {
            sap_store_zero(a + row * 24);
            sap_store_zero(c + row * 24);
        }
        return;
    }
    // a constraint (x, y, w) = (Az, Bz, Cz) or an input (z_i, one, z_i): the same four rows and one new variable
    const bool input = t > nc;
    const uint64_t i = input ? t - nc : t;
    const uint64_t row0 = input ? 2 * nc + 2 * i - 1 : 2 * i;               // the row of the sum
    const uint64_t var = input ? sh.nv + nc + i - 1 : sh.nv + i;            // index of the new variable in full
    const Fp x = fp_unpack((input ? z : az) + i * 24);
    const Fp y = input ? fp_const<P>(P::COUT) : fp_unpack(bz + i * 24);
    const Fp w = input ? x : fp_unpack(cz + i * 24);
    Fp s, d, sq, cc, repr = fp_zero();
    sap_pair<P>(x, y, w, s, d, sq, cc, scalars || aux, repr);
    fp_pack(a + row0 * 24, s);
    fp_pack(a + (row0 + 1) * 24, d);
    fp_pack(c + row0 * 24, cc);
    fp_pack(c + (row0 + 1) * 24, sq);
    if (full) fp_pack(full + var * 24, sq);
    if (scalars) fp_pack(scalars + (var - 1) * 24, repr);
    if (aux) fp_pack(aux + (var - ni) * 24, repr);
}

// Row j < sh.full_rows() of the instance map.  at_p = A^T p, bt_m = B^T m, ct_q = C^T q (nv rows each) for p_i = u[2i] +
// u[2i + 1], m_i = u[2i] - u[2i + 1], q_i = u[2i]; u: N rows; a, c: full_rows() rows.  Row 0 sums the ni - 1 input pairs
// in this one lane's loop.
template <class P>
GH_HD void sap_instance_row(const SapShape& sh, uint64_t j, const uint32_t* at_p, const uint32_t* bt_m, const uint32_t* ct_q, const uint32_t* u,
                            uint32_t* a, uint32_t* c) {
    const uint64_t nc = sh.nc, ni = sh.ni, nv = sh.nv;
    const uint32_t* ui = u + 2 * nc * 24;                                   // the rows of the inputs: one, then (odd, even) pairs
    if (j >= nv) {                                                          // an extra variable: it does not occur in A (:68, :85-91)
        const uint64_t i = j - nv;
        const uint32_t* pair = i < nc ? u + 2 * i * 24 : ui + (2 * (i - nc + 1) - 1) * 24;
        sap_store_zero(a + j * 24);
        fp_pack(c + j * 24, fp_add<P>(fp_unpack(pair), fp_unpack(pair + 24)));
        return;
    }
    Fp av = fp_add<P>(fp_unpack(at_p + j * 24), fp_unpack(bt_m + j * 24));
    Fp cv = fp_dbl<P>(fp_dbl<P>(fp_unpack(ct_q + j * 24)));
    if (j == 0) {
        const Fp one_row = fp_unpack(ui);
        av = fp_add<P>(av, one_row);
        cv = fp_add<P>(cv, one_row);
        for (uint64_t i = 1; i < ni; i++)
            av = fp_add<P>(av, fp_sub<P>(fp_unpack(ui + (2 * i - 1) * 24), fp_unpack(ui + 2 * i * 24)));
    } else if (j < ni) {
        const Fp odd = fp_unpack(ui + (2 * j - 1) * 24);
        av = fp_add<P>(av, fp_add<P>(odd, fp_unpack(ui + 2 * j * 24)));
        cv = fp_add<P>(cv, fp_dbl<P>(fp_dbl<P>(odd)));
    }
    fp_pack(a + j * 24, av);
    fp_pack(c + j * 24, cv);
}

// p, m, q of constraint i in the internal form, the input vectors of the three transposed products: one conversion per element
template <class P> GH_HD void sap_split(const uint32_t* u, uint64_t i, Fp& p, Fp& m, Fp& q) {
    q = fp_from_abi<P>(u + 2 * i * 24);
    const Fp o = fp_from_abi<P>(u + (2 * i + 1) * 24);
    p = fp_add<P>(q, o);
    m = fp_sub<P>(q, o);
}

}  // namespace gh
