// A stand-alone program over ginger-lib_amd/csrc/r1cs_plan.h: random sparse matrices with empty, short and very long rows,
// repeated indices and every class of coefficient are validated, transposed, scheduled at several segment lengths and run by
// the host executor; the results are compared with sums the program forms term by term.  Meant to be built with the host
// sanitizers and run once on its own (no GPU, nothing loaded into another process):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_shim/r1cs_check.cpp -o r1cs_check
// Exit status 0 and "ok" on success.  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include "../../ginger-lib_amd/csrc/r1cs_plan.h"

using namespace gh;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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
template <class P> static void abi_of(uint64_t* w, const Fp& v) { fp_to_abi<P>(reinterpret_cast<uint32_t*>(w), v); }
template <class P> static Fp of_abi(const uint64_t* w) { return fp_from_abi<P>(reinterpret_cast<const uint32_t*>(w)); }

template <class P> static void one_matrix(uint32_t rows, uint32_t cols, uint32_t long_row_terms) {
    // dictionary: 0, 1, -1, 2, -2, 15, -15, 16 and random values
    const uint32_t ND = 12;
    std::vector<uint64_t> values(12 * ND);
    std::vector<Fp> dv(ND);
    Fp k = fp_zero();
    const Fp one = fp_one<P>();
    Fp mult[17];
    for (int i = 0; i <= 16; i++) { mult[i] = k; k = fp_add<P>(k, one); }
    const Fp fixed[8] = {mult[0], mult[1], fp_neg<P>(mult[1]), mult[2], fp_neg<P>(mult[2]), mult[15], fp_neg<P>(mult[15]), mult[16]};
    for (uint32_t i = 0; i < ND; i++) {
        if (i < 8) abi_of<P>(&values[12 * i], fixed[i]);
        else random_row(&values[12 * i]);
        CHECK(r1cs_below<P>(&values[12 * i]));
        dv[i] = of_abi<P>(&values[12 * i]);
    }
    // rows: empty every fifth, one long row, the rest 1 .. 6 terms with a repeated index now and then
    std::vector<uint64_t> row_ptr(rows + 1, 0);
    std::vector<uint32_t> col, cid;
    for (uint32_t r = 0; r < rows; r++) {
        uint32_t t = r % 5 == 4 ? 0 : 1 + (uint32_t)(rnd() % 6);
        if (r == rows / 2) t = long_row_terms;
        for (uint32_t j = 0; j < t; j++) {
            col.push_back(j % 7 == 3 && !col.empty() ? col.back() : (uint32_t)(rnd() % cols));
            cid.push_back((uint32_t)(rnd() % ND));
        }
        row_ptr[r + 1] = col.size();
    }
    CHECK(r1cs_check_csr(rows, cols, row_ptr.data(), col.data(), cid.data(), ND) == nullptr);
    std::vector<uint64_t> x(12 * (size_t)cols), u(12 * (size_t)rows);
    for (uint32_t i = 0; i < cols; i++) random_row(&x[12 * (size_t)i]);
    for (uint32_t i = 0; i < rows; i++) random_row(&u[12 * (size_t)i]);
    if (cols > 2) { abi_of<P>(&x[0], fp_zero()); abi_of<P>(&x[12], one); abi_of<P>(&x[24], fp_neg<P>(one)); }
    // naive sums
    std::vector<Fp> want(rows, fp_zero()), want_t(cols, fp_zero());
    for (uint32_t r = 0; r < rows; r++)
        for (uint64_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
            want[r] = fp_add<P>(want[r], fp_mul<P>(of_abi<P>(&x[12 * (size_t)col[j]]), dv[cid[j]]));
            want_t[col[j]] = fp_add<P>(want_t[col[j]], fp_mul<P>(of_abi<P>(&u[12 * (size_t)r]), dv[cid[j]]));
        }
    std::vector<Fp> dict;
    std::vector<uint32_t> code;
    uint32_t counts[R1CS_CLASSES];
    r1cs_classify<P>(values.data(), ND, dict, code, counts);
    CHECK(counts[R1CS_ZERO] == 1 && counts[R1CS_ONE] == 1 && counts[R1CS_MINUS_ONE] == 1 && counts[R1CS_SMALL] == 2 &&
          counts[R1CS_MINUS_SMALL] == 2 && counts[R1CS_GENERAL] == 5);
    std::vector<uint64_t> t_ptr;
    std::vector<uint32_t> t_col, t_cid;
    r1cs_transpose(rows, cols, row_ptr.data(), col.data(), cid.data(), t_ptr, t_col, t_cid);
    CHECK(r1cs_check_csr(cols, rows, t_ptr.data(), t_col.data(), t_cid.data(), ND) == nullptr);
    for (uint32_t c = 0; c < cols; c++)
        for (uint64_t j = t_ptr[c]; j + 1 < t_ptr[c + 1]; j++) CHECK(t_col[j] <= t_col[j + 1]);      // stable in row order
    const uint32_t segs[] = {2, 3, 4, 32};
    for (uint32_t S : segs) {
        R1csPlan plan;
        r1cs_build_plan(rows, cols, row_ptr.data(), col.data(), cid.data(), code, S, plan);
        CHECK(plan.levels.size() == r1cs_row_levels(plan.longest, S));
        std::vector<uint64_t> y(12 * (size_t)rows, ~(uint64_t)0);
        r1cs_plan_run<P>(plan, dict, x.data(), y.data());
        for (uint32_t r = 0; r < rows; r++) {
            uint64_t w[12];
            abi_of<P>(w, want[r]);
            CHECK(memcmp(w, &y[12 * (size_t)r], 96) == 0);
        }
        r1cs_build_plan(cols, rows, t_ptr.data(), t_col.data(), t_cid.data(), code, S, plan);
        std::vector<uint64_t> yt(12 * (size_t)cols, ~(uint64_t)0);
        r1cs_plan_run<P>(plan, dict, u.data(), yt.data());
        for (uint32_t c = 0; c < cols; c++) {
            uint64_t w[12];
            abi_of<P>(w, want_t[c]);
            CHECK(memcmp(w, &yt[12 * (size_t)c], 96) == 0);
        }
    }
}

static void refusals() {
    const uint64_t ok_ptr[3] = {0, 1, 2}, bad0[3] = {1, 1, 2}, mono[3] = {0, 2, 1};
    const uint32_t col[2] = {0, 4}, cid[2] = {0, 1}, big_col[2] = {0, 5}, big_id[2] = {2, 0};
    CHECK(r1cs_check_csr(2, 5, ok_ptr, col, cid, 2) == nullptr);
    CHECK(r1cs_check_csr(2, 5, nullptr, col, cid, 2) != nullptr);
    CHECK(r1cs_check_csr(2, 5, bad0, col, cid, 2) != nullptr);
    CHECK(r1cs_check_csr(2, 5, mono, col, cid, 2) != nullptr);
    CHECK(r1cs_check_csr(2, 5, ok_ptr, nullptr, cid, 2) != nullptr);
    CHECK(r1cs_check_csr(2, 5, ok_ptr, col, nullptr, 2) != nullptr);
    CHECK(r1cs_check_csr(2, 5, ok_ptr, big_col, cid, 2) != nullptr);
    CHECK(r1cs_check_csr(2, 5, ok_ptr, col, big_id, 2) != nullptr);
    const uint64_t none[1] = {0};
    CHECK(r1cs_check_csr(0, 5, none, nullptr, nullptr, 0) == nullptr);
    CHECK(!r1cs_below<P4>(r1cs_modulus<P4>()) && !r1cs_below<P6>(r1cs_modulus<P6>()));
    uint32_t lg = 0;
    CHECK(r1cs_domain<P6>(((uint64_t)1 << 20), &lg) && lg == 20);
    CHECK(r1cs_domain<P6>(((uint64_t)1 << 20) + 1, &lg) && lg == 21);
    CHECK(r1cs_domain<P4>(((uint64_t)1 << 14), &lg) && lg == 14);
    CHECK(!r1cs_domain<P4>(((uint64_t)1 << 14) + 1, &lg));
    CHECK(r1cs_row_levels(0, 4) == 1 && r1cs_row_levels(4, 4) == 1 && r1cs_row_levels(5, 4) == 2 && r1cs_row_levels(16, 4) == 2 &&
          r1cs_row_levels(17, 4) == 3 && r1cs_row_levels((uint64_t)1 << 20, 32) == 4);
}

int main() {
    refusals();
    one_matrix<P6>(70, 23, 65);
    one_matrix<P4>(70, 23, 65);
    one_matrix<P6>(1, 1, 1100);          // one row whose column repeats 1100 times; transposed: one long row as well
    one_matrix<P4>(131, 64, 17);
    one_matrix<P6>(5, 200, 0);           // mostly unused variables: empty rows of the transposed matrix
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
