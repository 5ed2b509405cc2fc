// Host build (g++) of ginger-lib_amd/csrc/sqrt29.h for tests/test_points_host.py: the square roots, the subgroup chain and
// one row of compress / decompress, the same text the kernels of points.hip run.  Test infrastructure.
//
// Field elements cross this interface as canonical integers (12 LE u64 per Fq coefficient); points as the ABI's Montgomery
// x || y.  field: 0 = MNT4-753 Fq, 1 = MNT6-753 Fq, 2 = Fq2 over MNT4-753 Fq, 3 = Fq3 over MNT6-753 Fq.  curve: gh_curve_t.
#include <stdint.h>
#include "../../ginger-lib_amd/csrc/sqrt29.h"

using namespace gh;

namespace {

const uint32_t E4[] = GH_P4_SQRT_E32, E6[] = GH_P6_SQRT_E32, E63[] = GH_P6Q3_SQRT_E32;
const int8_t R4[] = GH_MNT4_R_NAF, R6[] = GH_MNT6_R_NAF;
static_assert(sizeof(E4) == 4 * SQRT_E_WORDS_P4 && sizeof(E6) == 4 * SQRT_E_WORDS_P6 && sizeof(E63) == 4 * SQRT_E_WORDS_P6Q3, "exponent words");
static_assert(sizeof(R4) == GH_MNT4_R_DIGITS && sizeof(R6) == GH_MNT6_R_DIGITS, "digit strings");

template <class C> struct Consts;
template <> struct Consts<Mnt4G1> { static const uint32_t* e() { return E4; } static const int8_t* r() { return R4; } };
template <> struct Consts<Mnt4G2> { static const uint32_t* e() { return E4; } static const int8_t* r() { return R4; } };
template <> struct Consts<Mnt6G1> { static const uint32_t* e() { return E6; } static const int8_t* r() { return R6; } };
template <> struct Consts<Mnt6G2> { static const uint32_t* e() { return E63; } static const int8_t* r() { return R6; } };

template <class C> Aff<C> load(const uint64_t* xy) {
    typedef typename C::FC F;
    const uint32_t* w = (const uint32_t*)xy;
    return Aff<C>{F::from_abi(w), F::from_abi(w + 24 * F::DEG)};
}

template <class C> int decompress(const uint64_t* x, uint8_t flags, uint64_t* out_xy, uint8_t* out_inf) {
    typedef typename C::FC F;
    Aff<C> p;
    bool inf;
    const int st = decompress_row<C>((const uint32_t*)x, flags, PointCurve<C>::b(), Consts<C>::e(), Consts<C>::r(), p, inf);
    F::to_abi((uint32_t*)out_xy, p.x);
    F::to_abi((uint32_t*)out_xy + 24 * F::DEG, p.y);
    *out_inf = inf;
    return st;
}
template <class C> int compress(const uint64_t* xy, uint8_t inf, uint64_t* out_x) { return compress_row<C>(load<C>(xy), inf != 0, (uint32_t*)out_x); }
template <class C> int member(const uint64_t* xy, uint8_t inf) {
    return inf || aff_is_member<C>(load<C>(xy), PointCurve<C>::b(), Consts<C>::r());
}

#define DISPATCH(curve, fn, ...)                                                                                        \
    ((curve) == 0 ? fn<Mnt4G1>(__VA_ARGS__) : (curve) == 1 ? fn<Mnt4G2>(__VA_ARGS__) : (curve) == 2 ? fn<Mnt6G1>(__VA_ARGS__) \
                                                             : fn<Mnt6G2>(__VA_ARGS__))

}  // namespace

extern "C" {

// out = a root of a (canonical coefficients), returns whether one exists as the reference sees it; out is unspecified if not
int pts_sqrt(int field, const uint64_t* a, uint64_t* out) {
    const uint32_t* w = (const uint32_t*)a;
    uint32_t* o = (uint32_t*)out;
    bool ok = false;
    switch (field) {
        case 0: {
            const FpRoot r = fq_sqrt_call<P4>(fp_from_canon_words<P4>(w), E4);
            fp_to_canon_words<P4>(o, r.v);
            return r.ok;
        }
        case 1: {
            const FpRoot r = fq_sqrt_call<P6>(fp_from_canon_words<P6>(w), E6);
            fp_to_canon_words<P6>(o, r.v);
            return r.ok;
        }
        case 2: {
            const Fp2T r = fq2_sqrt(Fp2T{fp_from_canon_words<P4>(w), fp_from_canon_words<P4>(w + 24)}, E4, ok);
            fp_to_canon_words<P4>(o, r.c0);
            fp_to_canon_words<P4>(o + 24, r.c1);
            return ok;
        }
        default: {
            const Fp3T r = fq3_sqrt(Fp3T{fp_from_canon_words<P6>(w), fp_from_canon_words<P6>(w + 24), fp_from_canon_words<P6>(w + 48)}, E63, ok);
            fp_to_canon_words<P6>(o, r.c0);
            fp_to_canon_words<P6>(o + 24, r.c1);
            fp_to_canon_words<P6>(o + 48, r.c2);
            return ok;
        }
    }
}
int pts_decompress(int curve, const uint64_t* x, uint8_t flags, uint64_t* out_xy, uint8_t* out_inf) { return DISPATCH(curve, decompress, x, flags, out_xy, out_inf); }
int pts_compress(int curve, const uint64_t* xy, uint8_t inf, uint64_t* out_x) { return DISPATCH(curve, compress, xy, inf, out_x); }
int pts_member(int curve, const uint64_t* xy, uint8_t inf) { return DISPATCH(curve, member, xy, inf); }

}  // extern "C"
