// A stand-alone program over ginger-lib_amd/csrc/sqrt29.h: the GH_HD square roots, the signed-digit subgroup chain and the
// rows of compress / decompress on their edge inputs, with the field and group laws as the check.  Meant to be built with the
// host sanitizers and run once on its own (no GPU, nothing loaded into another process):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_shim/points_check.cpp -o points_check
// Exit status 0 and "ok" on success.  Test infrastructure.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../ginger-lib_amd/csrc/sqrt29.h"

using namespace gh;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static const uint32_t E4[] = GH_P4_SQRT_E32, E6[] = GH_P6_SQRT_E32, E63[] = GH_P6Q3_SQRT_E32;
static const int8_t R4[] = GH_MNT4_R_NAF, R6[] = GH_MNT6_R_NAF;

template <class P> static Fp small(uint32_t v) {
    uint32_t w[24] = {v};
    return fp_from_canon_words<P>(w);
}

// Fq: zero, one, p - 1, the non-residue z = g^t (order 2^S), z^2 (a square that takes every correction round), an element whose
// t-th power is one (no correction round), small squares
template <class P> static void fq_cases(const uint32_t* e) {
    typedef F1<P, false> F;
    const Fp z = SqrtFq<P>::z(), one = F::one();
    FpRoot r = fq_sqrt_call<P>(fp_zero(), e);
    CHECK(r.ok && fp_is_zero(r.v));
    r = fq_sqrt_call<P>(one, e);
    CHECK(r.ok && F::eq(F::sqr(r.v), one));
    r = fq_sqrt_call<P>(z, e);
    CHECK(!r.ok);
    const Fp z2 = F::sqr(z);
    r = fq_sqrt_call<P>(z2, e);
    CHECK(r.ok && F::eq(F::sqr(r.v), z2));
    Fp u = small<P>(3);                                              // 3^(2^S): its order divides t
    for (int i = 0; i < SqrtFq<P>::S; i++) u = F::sqr(u);
    r = fq_sqrt_call<P>(u, e);
    CHECK(r.ok && F::eq(F::sqr(r.v), u));
    const Fp m1 = F::neg(one);                                       // p - 1: a square iff S > 1, and it is
    r = fq_sqrt_call<P>(m1, e);
    CHECK(r.ok && F::eq(F::sqr(r.v), m1));
    for (uint32_t v = 2; v < 12; v++) {
        const Fp a = small<P>(v), sq = F::sqr(a);
        r = fq_sqrt_call<P>(sq, e);
        CHECK(r.ok && F::eq(F::sqr(r.v), sq));
        r = fq_sqrt_call<P>(F::mul(sq, z), e);                       // a square times a non-residue
        CHECK(!r.ok);
    }
    CHECK(F::eq(fp_dbl<P>(SqrtFq<P>::half()), one));
}

static void fq2_cases() {
    typedef F2<P4, 13, false> F;
    bool ok;
    const Fp z = SqrtFq<P4>::z();
    Fp2T r = fq2_sqrt(F::zero(), E4, ok);
    CHECK(ok && F::is_zero(r));
    r = fq2_sqrt(F::one(), E4, ok);
    CHECK(ok && F::eq(F::sqr(r), F::one()));
    const Fp2T res{fp_sqr<P4>(small<P4>(7)), fp_zero()};             // c1 = 0, c0 a residue
    r = fq2_sqrt(res, E4, ok);
    CHECK(ok && F::eq(F::sqr(r), res) && fp_is_zero(r.c1));
    r = fq2_sqrt(Fp2T{z, fp_zero()}, E4, ok);                        // c1 = 0, c0 a non-residue: the reference's None
    CHECK(!ok);
    int found = 0, none = 0;
    for (uint32_t v = 1; v < 12; v++) {
        const Fp2T a{small<P4>(v), small<P4>(v + 5)}, sq = F::sqr(a);
        r = fq2_sqrt(sq, E4, ok);
        CHECK(ok && F::eq(F::sqr(r), sq));
        r = fq2_sqrt(a, E4, ok);                                     // whatever a is: a root only if it squares back
        if (ok) { CHECK(F::eq(F::sqr(r), a)); found++; } else none++;
    }
    CHECK(found + none == 11);
}

static void fq3_cases() {
    typedef F3<P6, 11, false> F;
    bool ok;
    Fp3T r = fq3_sqrt(F::zero(), E63, ok);
    CHECK(ok && F::is_zero(r));
    r = fq3_sqrt(F::one(), E63, ok);
    CHECK(ok && F::eq(F::sqr(r), F::one()));
    const uint32_t z0[NL] = GH_P6Q3_SQRT_Z0_I29, z1[NL] = GH_P6Q3_SQRT_Z1_I29, z2[NL] = GH_P6Q3_SQRT_Z2_I29;
    const Fp3T z{fp_const<P6>(z0), fp_const<P6>(z1), fp_const<P6>(z2)};
    r = fq3_sqrt(z, E63, ok);
    CHECK(!ok);
    const Fp3T zz = F::sqr(z);
    r = fq3_sqrt(zz, E63, ok);                                       // every correction round
    CHECK(ok && F::eq(F::sqr(r), zz));
    for (uint32_t v = 1; v < 4; v++) {
        const Fp3T a{small<P6>(v), small<P6>(v + 2), small<P6>(3 * v)}, sq = F::sqr(a);
        r = fq3_sqrt(sq, E63, ok);
        CHECK(ok && F::eq(F::sqr(r), sq));
        r = fq3_sqrt(F::mul(sq, z), E63, ok);
        CHECK(!ok);
    }
}

// the generator: a member; compress -> decompress gives it back with either sign of y; the rows that must fail do
template <class C> static void curve_cases(const Aff<C>& g, const uint32_t* e, const int8_t* rnaf) {
    typedef typename C::FC F;
    constexpr int D = F::DEG;
    const typename F::T b = PointCurve<C>::b();
    CHECK(aff_on_curve<C>(g, b) && aff_is_member<C>(g, b, rnaf));
    CHECK(r_times_is_zero<C>(g, rnaf));
    const Aff<C> off{g.x, F::add(g.y, F::one())};
    CHECK(!aff_is_member<C>(off, b, rnaf));
    for (int s = 0; s < 2; s++) {
        const Aff<C> p = s ? aff_neg<C>(g) : g;
        uint32_t xw[24 * D];
        const uint8_t fl = compress_row<C>(p, false, xw);
        CHECK((fl & ~PT_FLAG_PARITY) == 0);
        Aff<C> q;
        bool inf;
        CHECK(decompress_row<C>(xw, fl, b, e, rnaf, q, inf) == PT_OK && !inf && F::eq(q.x, p.x) && F::eq(q.y, p.y));
        CHECK(decompress_row<C>(xw, fl | 4, b, e, rnaf, q, inf) == PT_INVALID_FLAGS);
        CHECK(decompress_row<C>(xw, fl | PT_FLAG_INFINITY, b, e, rnaf, q, inf) == PT_INVALID_FLAGS && F::is_zero(q.x) && F::is_zero(q.y) && !inf);
        xw[23] |= 0x80000000u;                                       // far above the modulus
        CHECK(decompress_row<C>(xw, fl, b, e, rnaf, q, inf) == PT_INVALID_FIELD_ELEMENT);
    }
    uint32_t zw[24 * D];
    memset(zw, 0, sizeof zw);
    Aff<C> q;
    bool inf;
    CHECK(decompress_row<C>(zw, PT_FLAG_INFINITY, b, e, rnaf, q, inf) == PT_OK && inf && F::is_zero(q.x) && F::eq(q.y, F::one()));
    CHECK(decompress_row<C>(zw, PT_FLAG_INFINITY | PT_FLAG_PARITY, b, e, rnaf, q, inf) == PT_INVALID_FLAGS);
    CHECK(compress_row<C>(g, true, zw) == PT_FLAG_INFINITY);
    for (int w = 0; w < 24 * D; w++) CHECK(zw[w] == 0);
    uint32_t pw[24];                                                 // the modulus itself: not below it; one less: below
    Fp pm;
    for (int i = 0; i < NL; i++) pm.l[i] = C::PF::P[i];
    fp_pack(pw, pm);
    CHECK(!fp_words_below_p<typename C::PF>(pw));
    pw[0] -= 1;
    CHECK(fp_words_below_p<typename C::PF>(pw));
}

static Fp w4(const uint64_t* w) { return fp_from_abi<P4>((const uint32_t*)w); }
static Fp w6(const uint64_t* w) { return fp_from_abi<P6>((const uint32_t*)w); }

int main() {
    fq_cases<P4>(E4);
    fq_cases<P6>(E6);
    fq2_cases();
    fq3_cases();
    {
        static const uint64_t x[12] = GH_MNT4753_G1_GX0_M_64, y[12] = GH_MNT4753_G1_GY0_M_64;
        curve_cases<Mnt4G1>(Aff<Mnt4G1>{w4(x), w4(y)}, E4, R4);
    }
    {
        static const uint64_t x[12] = GH_MNT6753_G1_GX0_M_64, y[12] = GH_MNT6753_G1_GY0_M_64;
        curve_cases<Mnt6G1>(Aff<Mnt6G1>{w6(x), w6(y)}, E6, R6);
    }
    {
        static const uint64_t x0[12] = GH_MNT4753_G2_GX0_M_64, x1[12] = GH_MNT4753_G2_GX1_M_64, y0[12] = GH_MNT4753_G2_GY0_M_64,
                              y1[12] = GH_MNT4753_G2_GY1_M_64;
        curve_cases<Mnt4G2>(Aff<Mnt4G2>{Fp2T{w4(x0), w4(x1)}, Fp2T{w4(y0), w4(y1)}}, E4, R4);
    }
    {
        static const uint64_t x0[12] = GH_MNT6753_G2_GX0_M_64, x1[12] = GH_MNT6753_G2_GX1_M_64, x2[12] = GH_MNT6753_G2_GX2_M_64,
                              y0[12] = GH_MNT6753_G2_GY0_M_64, y1[12] = GH_MNT6753_G2_GY1_M_64, y2[12] = GH_MNT6753_G2_GY2_M_64;
        curve_cases<Mnt6G2>(Aff<Mnt6G2>{Fp3T{w6(x0), w6(x1), w6(x2)}, Fp3T{w6(y0), w6(y1), w6(y2)}}, E63, R6);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
