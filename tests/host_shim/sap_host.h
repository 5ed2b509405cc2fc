// What tests/host_shim/sap_shim.cpp and sap_check.cpp share: the SAP maps of include/ginger_hip_sap.h on the host -- the three
// products by r1cs_plan.h's host executor, then ginger-lib_amd/csrc/sap_rows.h's lanes in a loop, in the order r1cs.hip
// launches them.  Test infrastructure.
#pragma once
#include "../../ginger-lib_amd/csrc/r1cs_plan.h"
#include "../../ginger-lib_amd/csrc/sap_rows.h"
#include "../../include/ginger_hip_r1cs.h"

namespace sap_host {

using namespace gh;

inline const uint32_t* w32(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }
inline uint32_t* w32(uint64_t* p) { return reinterpret_cast<uint32_t*>(p); }

// false where the SAP domain exceeds the field's 2-adicity
template <class P> bool shape(uint64_t ni, uint64_t na, uint64_t nc, SapShape& sh, uint32_t* log_n) {
    sh.ni = ni;
    sh.nc = nc;
    sh.nv = ni + na;
    if (!r1cs_domain<P>(sh.domain_arg(), log_n)) return false;
    sh.N = (uint64_t)1 << *log_n;
    return true;
}

// y = M x (transpose: M^T x) through the level builder and the host executor; y: rows of the output orientation
template <class P>
void product(const SapShape& sh, const gh_r1cs_matrix_t& m, uint32_t S, bool transpose, const uint64_t* x, std::vector<uint64_t>& y) {
    std::vector<Fp> dict;
    std::vector<uint32_t> code;
    uint32_t counts[R1CS_CLASSES];
    r1cs_classify<P>(m.coeff_values, m.num_coeffs, dict, code, counts);
    R1csPlan plan;
    if (transpose) {
        std::vector<uint64_t> t_ptr;
        std::vector<uint32_t> t_col, t_coeff;
        r1cs_transpose(sh.nc, sh.nv, m.row_ptr, m.col, m.coeff_id, t_ptr, t_col, t_coeff);
        r1cs_build_plan(sh.nv, sh.nc, t_ptr.data(), t_col.data(), t_coeff.data(), code, S, plan);
    } else {
        r1cs_build_plan(sh.nc, sh.nv, m.row_ptr, m.col, m.coeff_id, code, S, plan);
    }
    y.assign(12 * (size_t)(transpose ? sh.nv : sh.nc) + 12, ~(uint64_t)0);
    r1cs_plan_run<P>(plan, dict, x, y.data());
}

// gh_sap_rows(_dev): a, c: N rows; scalars, aux, full: nullable
template <class P>
void rows(const SapShape& sh, const gh_r1cs_matrix_t* m, uint32_t S, const uint64_t* z, uint64_t* a, uint64_t* c, uint64_t* scalars, uint64_t* aux,
          uint64_t* full) {
    std::vector<uint64_t> prod[3];
    for (int k = 0; k < 3; k++) product<P>(sh, m[k], S, false, z, prod[k]);
    // what the conversion of the assignment leaves in the scalar destinations, and the caller's copy into full
    Fp one = fp_zero();
    one.l[0] = 1;
    for (uint64_t i = 0; i < sh.nv; i++) {
        uint32_t repr[24];
        fp_pack(repr, fp_mul<P>(fp_from_abi<P>(w32(z + 12 * i)), one));
        if (scalars && i) memcpy(scalars + 12 * (i - 1), repr, 96);
        if (aux && i >= sh.ni) memcpy(aux + 12 * (i - sh.ni), repr, 96);
        if (full) memcpy(full + 12 * i, z + 12 * i, 96);
    }
    for (uint64_t t = 0; t < sh.rows_lanes(); t++)
        sap_rows_lane<P>(sh, t, w32(prod[0].data()), w32(prod[1].data()), w32(prod[2].data()), w32(z), w32(a), w32(c), scalars ? w32(scalars) : nullptr,
                         aux ? w32(aux) : nullptr, full ? w32(full) : nullptr);
}

// gh_sap_instance_map(_dev): u: N rows; a, c: full_rows() rows
template <class P> void instance_map(const SapShape& sh, const gh_r1cs_matrix_t* m, uint32_t S, const uint64_t* u, uint64_t* a, uint64_t* c) {
    std::vector<uint64_t> x[3], prod[3];
    for (int k = 0; k < 3; k++) x[k].assign(12 * (size_t)sh.nc + 12, 0);
    for (uint64_t i = 0; i < sh.nc; i++) {
        Fp p, mm, q;
        sap_split<P>(w32(u), i, p, mm, q);
        fp_to_abi<P>(w32(&x[0][12 * i]), p);              // the executor converts its input vector itself
        fp_to_abi<P>(w32(&x[1][12 * i]), mm);
        fp_to_abi<P>(w32(&x[2][12 * i]), q);
    }
    for (int k = 0; k < 3; k++) product<P>(sh, m[k], S, true, x[k].data(), prod[k]);
    for (uint64_t j = 0; j < sh.full_rows(); j++)
        sap_instance_row<P>(sh, j, w32(prod[0].data()), w32(prod[1].data()), w32(prod[2].data()), w32(u), w32(a), w32(c));
}

}  // namespace sap_host
