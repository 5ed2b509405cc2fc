// poly_check.cpp -- the lane bodies of the polynomial unit (ginger-lib_amd/csrc/poly_kernels.h) over the host executor
// (poly_host.h), as a program of its own for the host sanitizers: every buffer is a heap allocation of exactly the rows the
// ABI promises, so a lane that reads or writes one row too far is an AddressSanitizer report.  The shapes are the bounds: empty
// vectors, one row, lengths around a run, a segment and a chunk, and the two-pass forms.  The results are checked against each
// other (evaluate against the remainder of the division, the division against the multiplication); the values themselves are
// the CPU tests' business (tests/test_poly_host.py).  Prints "ok".
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_shim/poly_check.cpp -o poly_check
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include "poly_host.h"

using namespace poly_host;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
// exactly `rows` rows on the heap (one byte where there are none, never touched)
struct Rows {
    std::unique_ptr<uint32_t[]> p;
    uint64_t rows;
    explicit Rows(uint64_t r) : p(new uint32_t[r ? r * 24 : 1]), rows(r) { memset(p.get(), 0xff, (r ? r * 24 : 1) * 4); }
    uint32_t* get() { return p.get(); }
};
template <class P> void fill(Rows& v) {          // values below 2^752: canonical in both fields
    for (uint64_t i = 0; i < v.rows; i++) {
        for (int w = 0; w < 24; w++) v.get()[i * 24 + w] = (uint32_t)rnd();
        v.get()[i * 24 + 23] &= 0xffff;
        if (i % 7 == 3) memset(v.get() + i * 24, 0, 96);
    }
}
static void fail(const char* what, uint64_t a, uint64_t b) {
    printf("FAILED %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    exit(1);
}

template <class P> void run_field() {
    PolyTuning small;
    small.run_len = small.direct_max = small.seg_max = 4;
    const PolyTuning tunings[2] = {small, PolyTuning()};
    const uint64_t sizes[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 1025};
    Rows z(3), one(1);
    fill<P>(z);
    memset(z.get(), 0, 96);                                                   // z_0 = 0
    for (const PolyTuning& t : tunings)
        for (uint64_t n : sizes) {
            Rows c(n), ev(3), q(n ? n - 1 : 0), rem(1), back(n);
            fill<P>(c);
            evaluate<P>(c.get(), n, z.get(), 3, t, ev.get());
            for (int p = 0; p < 3; p++) {
                evaluate<P>(c.get(), n, z.get() + 24 * p, 1, t, one.get());      // the grouped level against one point at a time
                if (memcmp(one.get(), ev.get() + 24 * p, 96)) fail("evaluate group", n, p);
                divide_linear<P>(c.get(), n, z.get() + 24 * p, t, q.get(), rem.get());
                if (memcmp(rem.get(), ev.get() + 24 * p, 96)) fail("remainder", n, p);
            }
            for (uint32_t log_n : {0u, 1u, 2u, 6u}) {
                const uint64_t N = (uint64_t)1 << log_n;
                Rows prod(n + N), dq(n), dr(N), vq(n > N ? n - N : 0), vr(N);
                mul_vanishing<P>(c.get(), n, log_n, prod.get());
                divide_vanishing<P>(prod.get(), n + N, log_n, t, dq.get(), dr.get());     // (c v) / v = (c, 0)
                if (n && memcmp(dq.get(), c.get(), n * 96)) fail("divide(mul)", n, N);
                if (reduce(dr.get(), N, true) != N) fail("divide(mul) remainder", n, N);
                divide_vanishing<P>(c.get(), n, log_n, t, vq.get(), vr.get());
            }
            Rows sum(n > 5 ? n : 5), five(5);
            fill<P>(five);
            for (int op = 0; op < 4; op++) axpy<P>(op, c.get(), n, five.get(), op == POLY_NEG ? 0 : 5, z.get() + 24, sum.get());
            if (reduce(c.get(), n, false) > n || reduce(c.get(), n, true) > n) fail("reduce", n, 0);
        }
    Rows big(5000), bq(4999), br(1);
    fill<P>(big);
    divide_vanishing<P>(big.get(), 5000, 0, small, bq.get(), br.get());          // N = 1: the two-pass form, six levels
    Rows g(1), dom(64), coeffs(2);
    fill<P>(g);
    fill<P>(coeffs);
    const uint64_t exps[2] = {0, 67};
    for (uint32_t log_n : {0u, 1u, 6u}) {
        elements<P>(g.get(), log_n, dom.get());
        sparse<P>(g.get(), exps, coeffs.get(), 2, log_n, dom.get());
    }
    for (uint64_t n = 0; n <= 70; n++)
        if (fold_cover(n, small) || fold_cover(n, PolyTuning()) || scan_cover(n, 1, 4, 4) || scan_cover(n, 4, 4, 4) || scan_cover(n, 1, 32, 32))
            fail("plan", n, 0);
}

int main() {
    run_field<P6>();
    run_field<P4>();
    printf("ok\n");
    return 0;
}
