// A stand-alone program over ginger-lib_amd/csrc/sap_rows.h: small random systems -- among them one input and no constraint
// (a domain of one row: no padding row is left), one input and one constraint, no aux variable, many inputs -- go through the
// host form of the SAP rows and of the instance map (sap_host.h) into buffers of exactly the documented sizes that held 0xFF,
// and every row is compared with the definition evaluated term by term in the internal form.  Meant to be built with the host
// sanitizers and run once on its own (no GPU, nothing loaded into another process):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_shim/sap_check.cpp -o sap_check
// Exit status 0 and "ok" on success.  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include "sap_host.h"

using namespace gh;
using sap_host::w32;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
// a random element in the ABI's form: random limbs below 2^752 are below both moduli
static void random_row(uint64_t* w) {
    for (int i = 0; i < 12; i++) w[i] = rnd();
    w[11] &= ((uint64_t)1 << 48) - 1;
}
template <class P> static Fp of_abi(const uint64_t* w) { return fp_from_abi<P>(w32(w)); }
template <class P> static bool row_is(const uint64_t* got, const Fp& want) {
    uint64_t w[12];
    fp_to_abi<P>(w32(w), want);
    return memcmp(w, got, 96) == 0;
}
template <class P> static bool repr_is(const uint64_t* got, const Fp& want) {
    Fp one = fp_zero();
    one.l[0] = 1;
    uint32_t w[24];
    fp_pack(w, fp_mul<P>(want, one));
    return memcmp(w, got, 96) == 0;
}
static bool all_ff(const uint64_t* row) {
    for (int k = 0; k < 12; k++)
        if (row[k] != ~(uint64_t)0) return false;
    return true;
}

struct Csr {
    std::vector<uint64_t> row_ptr, values;
    std::vector<uint32_t> col, cid;
    gh_r1cs_matrix_t view() const { return gh_r1cs_matrix_t{row_ptr.data(), col.data(), cid.data(), values.data(), values.size() / 12}; }
};

template <class P> static Csr random_matrix(uint64_t nc, uint64_t nv) {
    Csr m;
    const uint32_t ND = 5;
    m.values.resize(12 * ND);
    const Fp one = fp_one<P>();
    fp_to_abi<P>(w32(&m.values[0]), one);
    fp_to_abi<P>(w32(&m.values[12]), fp_neg<P>(one));
    fp_to_abi<P>(w32(&m.values[24]), fp_add<P>(one, fp_dbl<P>(one)));
    random_row(&m.values[36]);
    random_row(&m.values[48]);
    m.row_ptr.assign(nc + 1, 0);
    for (uint64_t r = 0; r < nc; r++) {
        const uint32_t t = r % 4 == 3 ? 0 : 1 + (uint32_t)(rnd() % 6);
        for (uint32_t j = 0; j < t; j++) {
            m.col.push_back((uint32_t)(rnd() % nv));
            m.cid.push_back((uint32_t)(rnd() % ND));
        }
        m.row_ptr[r + 1] = m.col.size();
    }
    return m;
}

template <class P> static std::vector<Fp> naive(const Csr& m, uint64_t rows, uint64_t cols, const std::vector<Fp>& x, bool transpose) {
    std::vector<Fp> y(transpose ? cols : rows, fp_zero());
    for (uint64_t r = 0; r < rows; r++)
        for (uint64_t j = m.row_ptr[r]; j < m.row_ptr[r + 1]; j++) {
            const Fp cf = of_abi<P>(&m.values[12 * (size_t)m.cid[j]]);
            if (transpose) y[m.col[j]] = fp_add<P>(y[m.col[j]], fp_mul<P>(x[r], cf));
            else y[r] = fp_add<P>(y[r], fp_mul<P>(x[m.col[j]], cf));
        }
    return y;
}

template <class P> static Fp times4(const Fp& v) { return fp_dbl<P>(fp_dbl<P>(v)); }

template <class P> static void one_system(uint64_t ni, uint64_t na, uint64_t nc, uint32_t S, uint64_t want_N) {
    SapShape sh;
    uint32_t log_n = 0;
    CHECK(sap_host::shape<P>(ni, na, nc, sh, &log_n));
    CHECK(sh.N == want_N && sh.N >= sh.domain_arg() && sh.full_rows() == sh.nv + nc + ni - 1 && sh.rows_lanes() == sh.N - nc - ni + 1);
    const uint64_t nv = sh.nv, N = sh.N;
    const Csr ms[3] = {random_matrix<P>(nc, nv), random_matrix<P>(nc, nv), random_matrix<P>(nc, nv)};
    const gh_r1cs_matrix_t m[3] = {ms[0].view(), ms[1].view(), ms[2].view()};
    const Fp one = fp_one<P>();

    // ---- the rows
    std::vector<uint64_t> z(12 * nv);
    for (uint64_t i = 0; i < nv; i++) random_row(&z[12 * i]);
    fp_to_abi<P>(w32(&z[0]), one);
    std::vector<Fp> zi(nv);
    for (uint64_t i = 0; i < nv; i++) zi[i] = of_abi<P>(&z[12 * i]);
    const std::vector<Fp> az = naive<P>(ms[0], nc, nv, zi, false), bz = naive<P>(ms[1], nc, nv, zi, false), cz = naive<P>(ms[2], nc, nv, zi, false);
    for (int with_scalars = 0; with_scalars < 2; with_scalars++) {
        std::vector<uint64_t> a(12 * N, ~(uint64_t)0), c(12 * N, ~(uint64_t)0), scal(12 * sh.sap_nv(), ~(uint64_t)0), aux(12 * sh.aux_rows(), ~(uint64_t)0),
            full(12 * sh.full_rows(), ~(uint64_t)0);
        sap_host::rows<P>(sh, m, S, z.data(), a.data(), c.data(), with_scalars ? scal.data() : nullptr, with_scalars ? aux.data() : nullptr,
                          with_scalars ? nullptr : full.data());
        std::vector<Fp> want_full(zi);
        for (uint64_t i = 0; i < nc; i++) {
            const Fp d = fp_sub<P>(az[i], bz[i]), e = fp_sqr<P>(d);
            want_full.push_back(e);
            CHECK(row_is<P>(&a[12 * 2 * i], fp_add<P>(az[i], bz[i])) && row_is<P>(&a[12 * (2 * i + 1)], d));
            CHECK(row_is<P>(&c[12 * 2 * i], fp_add<P>(times4<P>(cz[i]), e)) && row_is<P>(&c[12 * (2 * i + 1)], e));
        }
        CHECK(row_is<P>(&a[12 * 2 * nc], one) && row_is<P>(&c[12 * 2 * nc], one));
        for (uint64_t i = 1; i < ni; i++) {
            const Fp d = fp_sub<P>(zi[i], one), f = fp_sqr<P>(d);
            want_full.push_back(f);
            const uint64_t r0 = 2 * nc + 2 * i - 1;
            CHECK(row_is<P>(&a[12 * r0], fp_add<P>(zi[i], one)) && row_is<P>(&a[12 * (r0 + 1)], d));
            CHECK(row_is<P>(&c[12 * r0], fp_add<P>(times4<P>(zi[i]), f)) && row_is<P>(&c[12 * (r0 + 1)], f));
        }
        CHECK(want_full.size() == sh.full_rows());
        for (uint64_t r = sh.domain_arg(); r < N; r++)
            for (int k = 0; k < 12; k++) CHECK(a[12 * r + k] == 0 && c[12 * r + k] == 0);
        for (uint64_t k = 0; k < sh.full_rows(); k++) {
            if (with_scalars) {
                if (k) CHECK(repr_is<P>(&scal[12 * (k - 1)], want_full[k]));
                if (k >= ni) CHECK(repr_is<P>(&aux[12 * (k - ni)], want_full[k]));
                CHECK(all_ff(&full[12 * k]));
            } else {
                CHECK(row_is<P>(&full[12 * k], want_full[k]));
            }
        }
        if (!with_scalars)
            for (uint64_t k = 0; k < sh.sap_nv(); k++) CHECK(all_ff(&scal[12 * k]));
    }

    // ---- the instance map
    std::vector<uint64_t> u(12 * N);
    for (uint64_t i = 0; i < N; i++) random_row(&u[12 * i]);
    std::vector<Fp> ui(N), p(nc), mm(nc), q(nc);
    for (uint64_t i = 0; i < N; i++) ui[i] = of_abi<P>(&u[12 * i]);
    for (uint64_t i = 0; i < nc; i++) {
        p[i] = fp_add<P>(ui[2 * i], ui[2 * i + 1]);
        mm[i] = fp_sub<P>(ui[2 * i], ui[2 * i + 1]);
        q[i] = ui[2 * i];
    }
    const std::vector<Fp> at_p = naive<P>(ms[0], nc, nv, p, true), bt_m = naive<P>(ms[1], nc, nv, mm, true), ct_q = naive<P>(ms[2], nc, nv, q, true);
    std::vector<Fp> wa(sh.full_rows(), fp_zero()), wc(sh.full_rows(), fp_zero());
    for (uint64_t j = 0; j < nv; j++) {
        wa[j] = fp_add<P>(at_p[j], bt_m[j]);
        wc[j] = times4<P>(ct_q[j]);
    }
    for (uint64_t i = 0; i < nc; i++) wc[nv + i] = p[i];
    wa[0] = fp_add<P>(wa[0], ui[2 * nc]);
    wc[0] = fp_add<P>(wc[0], ui[2 * nc]);
    for (uint64_t i = 1; i < ni; i++) {
        const Fp odd = ui[2 * nc + 2 * i - 1], even = ui[2 * nc + 2 * i];
        wa[0] = fp_add<P>(wa[0], fp_sub<P>(odd, even));
        wa[i] = fp_add<P>(wa[i], fp_add<P>(odd, even));
        wc[i] = fp_add<P>(wc[i], times4<P>(odd));
        wc[nv + nc - 1 + i] = fp_add<P>(odd, even);
    }
    std::vector<uint64_t> a(12 * sh.full_rows(), ~(uint64_t)0), c(12 * sh.full_rows(), ~(uint64_t)0);
    sap_host::instance_map<P>(sh, m, S, u.data(), a.data(), c.data());
    for (uint64_t j = 0; j < sh.full_rows(); j++) CHECK(row_is<P>(&a[12 * j], wa[j]) && row_is<P>(&c[12 * j], wc[j]));
}

int main() {
    SapShape sh;
    uint32_t lg = 0;
    CHECK(sap_host::shape<P4>(3, 0, (1 << 13) - 3, sh, &lg) && lg == 14);        // 2^14 - 1: MNT6-753 Fr has 2-adicity 15
    CHECK(!sap_host::shape<P4>(3, 0, (1 << 13) - 2, sh, &lg));                   // 2^14 + 1
    one_system<P6>(1, 0, 0, 4, 1);       // z = (one): the domain is the row of ones, no padding row
    one_system<P4>(1, 0, 0, 4, 1);
    one_system<P6>(1, 0, 1, 4, 4);       // one constraint over the constant alone, one padding row
    one_system<P4>(1, 2, 1, 2, 4);
    one_system<P6>(2, 0, 0, 4, 4);       // inputs without constraints or aux variables
    one_system<P4>(3, 4, 29, 4, 64);     // 63: one padding row
    one_system<P6>(3, 4, 30, 2, 128);    // 65: the domain doubles
    one_system<P6>(40, 3, 7, 32, 128);   // more inputs than constraints
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
