// A stand-alone program over ginger-lib_amd/csrc/gm17_sum.h: the GH_HD group additions of the GM17 verifier on their degenerate
// cases, for G1 and G2 of both engines, with the group laws as the check.  Built with the host sanitizers and run once on its
// own (no GPU, nothing loaded into another process) by tests/test_gm17_verify_host.py test_sanitized_standalone_check, through
// tests/shim_build.py sanitized_check:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_shim/gm17_sum_check.cpp -o gm17_sum_check
// Exit status 0 and "ok" on success.  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include "../../ginger-lib_amd/csrc/gm17_sum.h"

using namespace gh;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

template <class G> static bool same(const Gm17Point<typename G::F::T>& a, const Gm17Point<typename G::F::T>& b) {
    typedef typename G::F F;
    if (a.inf || b.inf) return a.inf && b.inf && F::is_zero(a.x) && F::is_zero(a.y) && F::is_zero(b.x) && F::is_zero(b.y);
    return F::eq(a.x, b.x) && F::eq(a.y, b.y);
}

template <class G> static bool on_curve(const Gm17Point<typename G::F::T>& p, const typename G::F::T& b) {
    typedef typename G::F F;
    if (p.inf) return true;
    return F::eq(F::sqr(p.y), F::add(F::add(F::mul(F::sqr(p.x), p.x), F::mul(G::a(), p.x)), b));
}

template <class G> static void cases(const Gm17Point<typename G::F::T>& g, const typename G::F::T& b) {
    typedef typename G::F F;
    typedef Gm17Point<typename F::T> Pt;
    const Pt inf{F::zero(), F::zero(), true};
    CHECK(on_curve<G>(g, b));
    const Pt g2 = gm17_add<G>(g, g);                                  // a doubling
    CHECK(!g2.inf && on_curve<G>(g2, b) && !same<G>(g2, g));
    const Pt g3 = gm17_add<G>(g2, g), g3b = gm17_add<G>(g, g2);       // distinct points, both orders
    CHECK(!g3.inf && on_curve<G>(g3, b) && same<G>(g3, g3b));
    const Pt g4 = gm17_add<G>(g2, g2), g4b = gm17_add<G>(g3, g);      // (2 + 2) G = (3 + 1) G
    CHECK(same<G>(g4, g4b));
    CHECK(same<G>(gm17_add<G>(g, gm17_neg<G>(g)), inf));              // opposite points
    CHECK(same<G>(gm17_add<G>(gm17_neg<G>(g3), g3), inf));
    CHECK(same<G>(gm17_add<G>(g3, gm17_neg<G>(g)), g2));              // 3 G - G = 2 G
    CHECK(same<G>(gm17_add<G>(inf, g), g));                           // either operand at infinity
    CHECK(same<G>(gm17_add<G>(g, inf), g));
    CHECK(same<G>(gm17_add<G>(inf, inf), inf));
    CHECK(same<G>(gm17_neg<G>(inf), inf));
    const Pt two{g.x, F::zero(), false};                              // y = 0 (not on the curve): the tangent is vertical
    CHECK(same<G>(gm17_add<G>(two, two), inf));
    const Pt junk{g.y, g.x, true};                                    // the coordinates of a point at infinity are not used
    CHECK(same<G>(gm17_add<G>(junk, g), g));
    CHECK(same<G>(gm17_add<G>(junk, junk), inf));
}

static Fp w4(const uint64_t* w) { return fp_from_abi<P4>((const uint32_t*)w); }
static Fp w6(const uint64_t* w) { return fp_from_abi<P6>((const uint32_t*)w); }

int main() {
    {
        static const uint64_t x[12] = GH_MNT4753_G1_GX0_M_64, y[12] = GH_MNT4753_G1_GY0_M_64, b[12] = GH_MNT4753_G1_B0_M_64;
        cases<Gm17G1<Mnt4Pairing>>(Gm17Point<Fp>{w4(x), w4(y), false}, w4(b));
    }
    {
        static const uint64_t x[12] = GH_MNT6753_G1_GX0_M_64, y[12] = GH_MNT6753_G1_GY0_M_64, b[12] = GH_MNT6753_G1_B0_M_64;
        cases<Gm17G1<Mnt6Pairing>>(Gm17Point<Fp>{w6(x), w6(y), false}, w6(b));
    }
    {
        static const uint64_t x0[12] = GH_MNT4753_G2_GX0_M_64, x1[12] = GH_MNT4753_G2_GX1_M_64, y0[12] = GH_MNT4753_G2_GY0_M_64,
                              y1[12] = GH_MNT4753_G2_GY1_M_64, b0[12] = GH_MNT4753_G2_B0_M_64, b1[12] = GH_MNT4753_G2_B1_M_64;
        cases<Gm17G2<Mnt4Pairing>>(Gm17Point<Fp2T>{Fp2T{w4(x0), w4(x1)}, Fp2T{w4(y0), w4(y1)}, false}, Fp2T{w4(b0), w4(b1)});
    }
    {
        static const uint64_t x0[12] = GH_MNT6753_G2_GX0_M_64, x1[12] = GH_MNT6753_G2_GX1_M_64, x2[12] = GH_MNT6753_G2_GX2_M_64,
                              y0[12] = GH_MNT6753_G2_GY0_M_64, y1[12] = GH_MNT6753_G2_GY1_M_64, y2[12] = GH_MNT6753_G2_GY2_M_64,
                              b0[12] = GH_MNT6753_G2_B0_M_64, b1[12] = GH_MNT6753_G2_B1_M_64, b2[12] = GH_MNT6753_G2_B2_M_64;
        cases<Gm17G2<Mnt6Pairing>>(Gm17Point<Fp3T>{Fp3T{w6(x0), w6(x1), w6(x2)}, Fp3T{w6(y0), w6(y1), w6(y2)}, false},
                                   Fp3T{w6(b0), w6(b1), w6(b2)});
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
