// A stand-alone program over ginger-lib_amd/csrc/unit_host.h: the argument checks and their messages, the modulus comparison at
// its edges, the generator checks of the hash handles and PhaseTimer::copy_out.  It calls no HIP API and needs no device: the
// paths it drives are the ones that return before a unit touches the card.  Built with the host sanitizers and run once on its
// own (nothing loaded into another process) by tests/test_shim_build.py test_unit_host_check_runs_clean_under_the_sanitizers,
// through tests/shim_build.py sanitized_check:
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host_shim/unit_host_check.cpp -o unit_host_check
// Exit status 0 and "ok" on success.  Test infrastructure.
#include <stdio.h>
#include <string>
#include <vector>
#include "../../ginger-lib_amd/csrc/unit_host.h"

// what unit_host.h expects of the library's context (ginger_hip.hip in the product)
namespace gh_rt {
Ctx g;
std::string g_err;
}  // namespace gh_rt

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

// p - 1, p, p + 1 of a modulus whose lowest word is neither 0 nor all ones (both are odd primes of 753 bits)
template <class P> static void modulus_edges() {
    const uint64_t* p = modulus64<P>();
    uint64_t x[3][12];
    for (int k = 0; k < 3; k++) memcpy(x[k], p, 96);
    x[0][0] -= 1;
    x[2][0] += 1;
    CHECK(below<P>(x[0]) && !below<P>(x[1]) && !below<P>(x[2]));
    uint64_t zero[12] = {}, top[12];
    memcpy(top, p, 96);
    top[11] += 1;                                             // differs in the most significant word only
    CHECK(below<P>(zero) && !below<P>(top));
    top[11] -= 2;
    top[0] = ~(uint64_t)0;
    CHECK(below<P>(top));
    // all_below: every row counts, none for count 0
    CHECK(all_below<P>(&x[0][0], 1) && !all_below<P>(&x[0][0], 2) && !all_below<P>(&x[0][0], 3) && all_below<P>(&x[1][0], 0));
}

static void messages() {
    CHECK(null_arg() == GH_E_BAD_ARG && g_err == "null argument");
    CHECK(too_large() == GH_E_BAD_ARG && g_err == "input too large");
    CHECK(unknown_field() == GH_E_BAD_ARG && g_err == "unknown field id");
    g_err.clear();
    CHECK(field_ok(GH_MNT4753_FR) == GH_OK && field_ok(GH_MNT6753_FR) == GH_OK && g_err.empty());
    // (an id outside the enumeration cannot be formed here: the sanitizer refuses the load; tests/test_abi_errors.py passes them)
    CHECK(is_g1(GH_MNT4753_G1) && is_g1(GH_MNT6753_G1) && !is_g1(GH_MNT4753_G2) && !is_g1(GH_MNT6753_G2));
    size_t r = 0;
    CHECK(!mul_overflows(3, 5, &r) && r == 15 && mul_overflows(SIZE_MAX, 2, &r) && !mul_overflows(SIZE_MAX, 1, &r));
    CHECK(blocks(0, 64) == 0 && blocks(1, 64) == 1 && blocks(64, 64) == 1 && blocks(65, 64) == 2);
    CHECK(GH_FIELD_DISPATCH(GH_MNT4753_FR, modulus64) == modulus64<P6>() && GH_FIELD_DISPATCH(GH_MNT6753_FR, modulus64) == modulus64<P4>());
}

// the generator of each G1 curve passes; a row off the curve, a row not below the modulus and the infinity flag are told apart
template <class C> static void generators(gh_curve_t curve) {
    uint64_t xyz[36];
    generator_xyz<C>(xyz);
    std::vector<uint64_t> xy(48);
    memcpy(&xy[0], xyz, 192);
    memcpy(&xy[24], xyz, 192);
    CHECK(on_curve_host<C>(xyz));
    CHECK(check_generators(curve, "", xy.data(), nullptr, 2) == GH_OK);
    xy[24] ^= 1;                                              // second row: x off by one bit
    CHECK(check_generators(curve, "", xy.data(), nullptr, 2) == GH_E_BAD_ARG && g_err == "a generator is not on the curve");
    CHECK(check_generators(curve, "gen_xy: ", xy.data(), nullptr, 2) == GH_E_BAD_ARG && g_err == "gen_xy: a generator is not on the curve");
    const uint8_t inf[2] = {0, 1};
    CHECK(check_generators(curve, "", xy.data(), inf, 2) == GH_OK);              // a row flagged at infinity is not read as a point
    CHECK(check_generators(curve, "", xy.data(), nullptr, 1) == GH_OK && check_generators(curve, "", xy.data(), nullptr, 0) == GH_OK);
    memcpy(&xy[36], modulus64<typename Scheme<C>::PF>(), 96);                    // second row: y == p, flagged or not
    CHECK(check_generators(curve, "rand_xy: ", xy.data(), inf, 2) == GH_E_BAD_ARG &&
          g_err == "rand_xy: a generator coordinate is not below the modulus");
    std::vector<uint64_t> kept;
    std::vector<uint8_t> flags;
    const uint8_t raw[2] = {0, 7};
    keep(kept, flags, xy.data(), raw, 2);
    CHECK(kept == xy && flags.size() == 2 && flags[0] == 0 && flags[1] == 1);
    keep(kept, flags, xy.data(), nullptr, 1);
    CHECK(kept.size() == 24 && flags.size() == 1 && flags[0] == 0);
    CHECK(data_below<C>(xyz, 3) && scalar_below<C>(xyz, 0));
}

// copy_out: the argument check, the count it returns and what it leaves untouched
static void copy_out() {
    PhaseTimer tm{3};
    tm.ms = {1.5f, 0.f, 2.5f};
    tm.total_ms = 4.f;
    float out[5] = {-1, -1, -1, -1, -1}, total = -1;
    CHECK(tm.copy_out(nullptr, 1, &total) == GH_E_BAD_ARG && g_err == "null argument" && total == -1);
    CHECK(tm.copy_out(out, -1, &total) == GH_E_BAD_ARG && total == -1);
    CHECK(tm.copy_out(nullptr, -1, nullptr) == GH_E_BAD_ARG);
    CHECK(tm.copy_out(nullptr, 0, &total) == 0 && total == 4.f);                 // max_phases 0: only the total
    CHECK(tm.copy_out(out, 0, nullptr) == 0 && out[0] == -1);
    CHECK(tm.copy_out(out, 2, nullptr) == 2 && out[0] == 1.5f && out[1] == 0.f && out[2] == -1);
    CHECK(tm.copy_out(out, 3, &total) == 3 && out[2] == 2.5f && out[3] == -1);
    CHECK(tm.copy_out(out, 5, &total) == 3 && out[3] == -1 && out[4] == -1);     // above the count: the count
    PhaseTimer none;                                          // a unit whose phase count is set by its first call
    total = -1;
    CHECK(none.copy_out(out, 5, &total) == 0 && total == 0.f);
    CHECK(none.copy_out(nullptr, 0, nullptr) == 0);
}

int main() {
    modulus_edges<P4>();
    modulus_edges<P6>();
    messages();
    generators<Mnt4G1>(GH_MNT4753_G1);
    generators<Mnt6G1>(GH_MNT6753_G1);
    copy_out();
    printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
