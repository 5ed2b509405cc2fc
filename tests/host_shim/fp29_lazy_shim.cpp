// Host build (g++) of the lazy G1 bucket arithmetic of fp29.h / ec29.h (fp_mul27, fp_sqr27, fp_mul2s27, the lazy differences,
// xyzz_madd_lazy with its init and exit conversions), exported for ctypes: tests/test_fp29_lazy_host.py checks it against Python
// integers and, limb for limb, against the generated assembly in the simulator.  Elements cross this interface as their 26 raw
// limbs (the top limb may be wide).  With -DFP29_LAZY_MAIN the file is a stand-alone program (the sanitizer run of the same
// test): it drives every function with operands at the bounds the kernel uses and a chain of 60 updates per prime against
// the fully reduced xyzz_madd.  Test infrastructure only; not part of the product library.
#include <stdio.h>
#include <string.h>
#include "../../ginger-lib_amd/csrc/ec29.h"

using namespace gh;

static Fp ld(const uint32_t* w) {
    Fp r;
    for (int i = 0; i < NL; i++) r.l[i] = w[i];
    return r;
}
static void st(uint32_t* w, const Fp& a) {
    for (int i = 0; i < NL; i++) w[i] = a.l[i];
}

template <class P> static void lazy_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
    Fp r = fp_zero();
    switch (op) {
        case 0: r = fp_mul27<P>(ld(a), ld(b)); break;
        case 1: r = fp_sqr27<P>(ld(a)); break;
        case 2: r = fp_mul2s27<P>(ld(a), ld(b), ld(c), ld(d)); break;
        case 3: r = fp_lazy_sub<P, 3>(ld(a), ld(b)); break;
        case 4: r = fp_lazy_sub<P, 1>(ld(a), ld(b)); break;
        case 5: r = fp_lazy_x3<P>(ld(a), ld(b), ld(c)); break;
        case 6: r = fp_neg_lazy<P>(ld(a)); break;
        case 7: r.l[0] = fp_is_zero_or_p<P>(ld(a)) ? 1u : 0u; break;
        case 8: r = fp_lazy_one<P>(); break;
    }
    st(out, r);
}

// n table rows (x[26] y[26]) with their signs through xyzz_madd_lazy from an empty sum; out: the 78 words the kernel stores,
// state: X, V, ZZ, ZZZ (26 words each) and sigma.  Returns how often `same` was reported (such an entry is skipped).
template <class P> static int lazy_chain(int n, const uint32_t* rows, const uint8_t* neg, uint32_t* out, uint32_t* state) {
    XyzzLazy s = xyzz_lazy_zero();
    int sames = 0;
    for (int j = 0; j < n; j++) {
        bool same;
        xyzz_madd_lazy<P>(s, ld(rows + 2 * NL * j), ld(rows + 2 * NL * j + NL), neg[j] != 0, same);
        sames += same ? 1 : 0;
    }
    Fp x, y, z;
    xyzz_lazy_to_proj<P>(s, x, y, z);
    st(out, x);
    st(out + NL, y);
    st(out + 2 * NL, z);
    st(state, s.x);
    st(state + NL, s.v);
    st(state + 2 * NL, s.zz);
    st(state + 3 * NL, s.zzz);
    state[4 * NL] = s.sneg;
    return sames;
}

extern "C" {
void t_lazy_op(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
    if (field == 4) lazy_op<P4>(op, a, b, c, d, out); else lazy_op<P6>(op, a, b, c, d, out);
}
uint64_t t_lazy_split(int field) { return field == 4 ? Dual27Split<P4>::MASK : Dual27Split<P6>::MASK; }
int t_lazy_chain(int field, int n, const uint32_t* rows, const uint8_t* neg, uint32_t* out, uint32_t* state) {
    return field == 4 ? lazy_chain<P4>(n, rows, neg, out, state) : lazy_chain<P6>(n, rows, neg, out, state);
}
}

#ifdef FP29_LAZY_MAIN
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 32);
}
template <class P> static Fp rnd_fp() {      // below p: the top limb stays under p's
    Fp r;
    for (int i = 0; i < NL - 1; i++) r.l[i] = rnd32() & LM;
    r.l[NL - 1] = rnd32() % P::P[NL - 1];
    return r;
}
// every limb at 2^29 - 1, the top limb that of k p + 2^733
template <class P> static Fp at_bound(int k) {
    Fp r;
    for (int i = 0; i < NL - 1; i++) r.l[i] = LM;
    r.l[NL - 1] = (uint32_t)(((uint64_t)k * P::P[NL - 1]) + (uint64_t)k + 256u);
    return r;
}
template <class P> static bool almost_reduced(const Fp& a) {
    for (int i = 0; i < NL - 1; i++) if (a.l[i] > LM) return false;
    return a.l[NL - 1] <= P::P[NL - 1] + 257u;
}
template <class C, class P> static int check(const char* name) {
    typedef typename C::F F;
    int bad = 0;
    // the widest operands of the update: 9 p by almost reduced, the 9 p square, the lazy dual product, the differences
    const Fp ar = at_bound<P>(1), x5 = at_bound<P>(5), p9 = at_bound<P>(9), w3 = at_bound<P>(3), t7 = at_bound<P>(7);
    bad += !almost_reduced<P>(fp_mul27<P>(p9, ar));
    bad += !almost_reduced<P>(fp_sqr27<P>(p9));
    bad += !almost_reduced<P>(fp_mul2s27<P>(w3, t7, ar, ar));
    bad += !almost_reduced<P>(fp_mul27<P>(fp_lazy_sub<P, 3>(ar, fp_zero()), ar));
    bad += !almost_reduced<P>(fp_mul27<P>(fp_lazy_sub<P, 3>(fp_zero(), x5), ar));
    bad += !almost_reduced<P>(fp_mul27<P>(fp_lazy_x3<P>(ar, fp_zero(), fp_zero()), ar));
    bad += !almost_reduced<P>(fp_mul27<P>(fp_lazy_x3<P>(fp_zero(), ar, ar), ar));
    bad += !fp_is_zero_or_p<P>(fp_const<P>(P::P)) || !fp_is_zero_or_p<P>(fp_zero()) || fp_is_zero_or_p<P>(fp_one<P>());
    bad += !fp_is_zero_or_p<P>(fp_sqr27<P>(fp_lazy_sub<P, 3>(ar, ar)));          // P = 8 p squares to p
    // 60 updates: the lazy sum and the fully reduced one are the same projective point after every entry
    XyzzLazy s = xyzz_lazy_zero();
    Xyzz<C> r = xyzz_zero<C>();
    for (int j = 0; j < 60; j++) {
        const Fp qx = rnd_fp<P>(), qy = rnd_fp<P>();
        const bool neg = rnd32() & 1;
        bool same_l, same_r;
        xyzz_madd_lazy<P>(s, qx, qy, neg, same_l);
        r = xyzz_madd<C>(r, Aff<C>{qx, neg ? fp_neg<P>(qy) : qy}, same_r);
        Fp x, y, z;
        xyzz_lazy_to_proj<P>(s, x, y, z);
        const Proj<C> e = xyzz_to_proj<C>(r);
        bad += same_l != same_r;
        bad += !fp_eq(fp_mul<P>(x, e.z), fp_mul<P>(e.x, z)) || !fp_eq(fp_mul<P>(y, e.z), fp_mul<P>(e.y, z));
        bad += fp_is_zero(z) != fp_is_zero(e.z);
        for (int i = 0; i < NL; i++) bad += x.l[i] > LM || y.l[i] > LM || z.l[i] > LM;
    }
    // q == sum is reported, q == -sum gives infinity, and the sum restarts from it
    {
        const Fp c = fp_lazy_one<P>();
        const Fp qx = rnd_fp<P>(), qy = rnd_fp<P>();
        XyzzLazy t = xyzz_lazy_zero();
        bool same;
        xyzz_madd_lazy<P>(t, qx, qy, false, same);
        bad += same || !fp_eq(t.zz, c);
        xyzz_madd_lazy<P>(t, qx, qy, false, same);
        bad += !same;
        xyzz_madd_lazy<P>(t, qx, qy, true, same);
        bad += same || !xyzz_lazy_is_zero<P>(t);
        Fp x, y, z;
        xyzz_lazy_to_proj<P>(t, x, y, z);
        bad += !fp_is_zero(x) || !fp_eq(y, fp_one<P>()) || !fp_is_zero(z);
        xyzz_madd_lazy<P>(t, qx, qy, true, same);
        bad += same || xyzz_lazy_is_zero<P>(t);
    }
    printf("%s: %s\n", name, bad ? "FAILED" : "ok");
    return bad;
}
int main() {
    int bad = check<Mnt4G1, P4>("mnt4753") + check<Mnt6G1, P6>("mnt6753");
    return bad ? 1 : 0;
}
#endif
