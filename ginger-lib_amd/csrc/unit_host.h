// unit_host.h -- the host layer under every device unit: launch arithmetic, the argument checks and
// their messages, what a unit knows of a G1 curve on the host, pooled buffers and copies on g.stream, and the phase timer
// behind every *_last_timing.  Host code only, no kernel.  Everything sits in an anonymous namespace: every unit that includes
// this header gets its own instances, its own timers included.
#pragma once
#include <string.h>
#include <algorithm>
#include <chrono>
#include "runtime.h"
#include "ec29.h"
#include "modulus.h"

namespace {

using namespace gh;
using gh_rt::g;
using gh_rt::g_err;

inline unsigned blocks(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }
inline bool mul_overflows(size_t a, size_t b, size_t* r) { return __builtin_mul_overflow(a, b, r); }

// ---- the argument checks: count rows of 12 words below P's modulus (below<P>: modulus.h), and the messages every unit shares
template <class P> bool all_below(const uint64_t* x, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (!below<P>(x + 12 * i)) return false;
    return true;
}
template <class P> Fp from_abi12(const uint64_t* v12) { return fp_from_abi<P>(reinterpret_cast<const uint32_t*>(v12)); }   // an ABI row -> internal
inline int null_arg() { g_err = "null argument"; return GH_E_BAD_ARG; }
inline int too_large() { g_err = "input too large"; return GH_E_BAD_ARG; }
inline int unknown_field() { g_err = "unknown field id"; return GH_E_BAD_ARG; }
inline int field_ok(gh_field_t f) { return f == GH_MNT4753_FR || f == GH_MNT6753_FR ? GH_OK : unknown_field(); }   // then GH_FIELD_DISPATCH

// ---- the G1 curves.  C the group, PF its base (= data) field, PS its scalar field; field: the hash's field id
template <class C> struct Scheme;
template <> struct Scheme<Mnt6G1> { typedef P6 PF; typedef P4 PS; static constexpr gh_field_t field = GH_MNT4753_FR; };
template <> struct Scheme<Mnt4G1> { typedef P4 PF; typedef P6 PS; static constexpr gh_field_t field = GH_MNT6753_FR; };
inline bool is_g1(gh_curve_t c) { return c == GH_MNT6753_G1 || c == GH_MNT4753_G1; }
template <class C> bool data_below(const uint64_t* x, size_t count) { return all_below<typename Scheme<C>::PF>(x, count); }
template <class C> bool scalar_below(const uint64_t* x, size_t count) { return all_below<typename Scheme<C>::PS>(x, count); }

template <class C> Fp curve_b() {
    static const uint64_t b4[12] = GH_MNT4753_G1_B0_M_64, b6[12] = GH_MNT6753_G1_B0_M_64;
    return fp_from_abi<typename Scheme<C>::PF>((const uint32_t*)(std::is_same<C, Mnt6G1>::value ? b6 : b4));
}
// y^2 == x^3 + a x + b on the host
template <class C> bool on_curve_host(const uint64_t* xy) {
    typedef typename Scheme<C>::PF PF;
    typedef F1<PF, true> F;
    const Fp x = fp_from_abi<PF>((const uint32_t*)xy), y = fp_from_abi<PF>((const uint32_t*)(xy + 12));
    const Fp rhs = F::add(F::add(F::mul(F::sqr(x), x), C::mul_by_a(x)), curve_b<C>());
    return F::eq(F::sqr(y), rhs);
}
template <class C> void generator_xyz(uint64_t* g_xyz) {
    const bool m6 = std::is_same<C, Mnt6G1>::value;
    static const uint64_t gx4[12] = GH_MNT4753_G1_GX0_M_64, gy4[12] = GH_MNT4753_G1_GY0_M_64, one4[12] = GH_P4_R_64;
    static const uint64_t gx6[12] = GH_MNT6753_G1_GX0_M_64, gy6[12] = GH_MNT6753_G1_GY0_M_64, one6[12] = GH_P6_R_64;
    memcpy(g_xyz, m6 ? gx6 : gx4, 96);
    memcpy(g_xyz + 12, m6 ? gy6 : gy4, 96);
    memcpy(g_xyz + 24, m6 ? one6 : one4, 96);
}

// The generators of a hash handle (gh_bh_create, gh_pedersen_create), x || y rows of `count`: below the modulus, and on the curve
// unless flagged at infinity; `prefix` opens the message ("" or the argument's name and a colon)
inline int check_generators(gh_curve_t curve, const char* prefix, const uint64_t* xy, const uint8_t* inf, size_t count) {
    if (!GH_G1_DISPATCH(curve, data_below, xy, 2 * count)) {
        g_err = std::string(prefix) + "a generator coordinate is not below the modulus";
        return GH_E_BAD_ARG;
    }
    for (size_t i = 0; i < count; i++)
        if (!(inf && inf[i]) && !GH_G1_DISPATCH(curve, on_curve_host, xy + 24 * i)) {
            g_err = std::string(prefix) + "a generator is not on the curve";
            return GH_E_BAD_ARG;
        }
    return GH_OK;
}
// the handle's host copy of them, the infinity bytes as 0 / 1
inline void keep(std::vector<uint64_t>& xy, std::vector<uint8_t>& flags, const uint64_t* src, const uint8_t* inf, size_t count) {
    xy.assign(src, src + 24 * count);
    flags.assign(count, 0);
    if (inf)
        for (size_t i = 0; i < count; i++) flags[i] = inf[i] != 0;
}

// ---- pooled device buffers and copies on g.stream.  A unit's entry points hold api_mutex() and synchronise before they return,
// so the units that share a prefix of the pool never hold a buffer at once.  An entry point of the "vb_" units keeps a Trim:
// when it returns, every "vb_" buffer above SLAB_KEEP_BYTES is released, and Poseidon's slab by the same rule.
template <class T> int dbuf(const char* name, size_t count, T** out, size_t min_bytes = 64) {
    return gh_rt::pool_get(name, std::max(count * sizeof(T), min_bytes), (void**)out);
}
template <class T> int up(T* d, const T* h, size_t count) {
    if (count) HIPCHK(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, g.stream));
    return GH_OK;
}
template <class T> int down(T* h, const T* d, size_t count) {
    if (count) HIPCHK(hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, g.stream));
    return GH_OK;
}
struct Trim {
    ~Trim() {
        gh_rt::pool_trim("vb_", gh_rt::SLAB_KEEP_BYTES);
        gh_rt::poseidon_trim_slab();
    }
};

// ---- A unit's phase timer and the record its *_last_timing reports.  The timer owns its events: they are created when a
// call first needs them and destroyed by a g.at_shutdown hook that also resets the object, so a timer works again after
// gh_shutdown and gh_init.  Every event is recorded on g.stream.  Three uses, all starting with begin():
//   consecutive phases   mark() before the first phase and after each; finish() waits for the last event: ms[i] = the time
//                        between events i and i + 1, total_ms = the wall clock since begin()
//   labelled intervals   mark(phase) after each launch; finish(n_phases), after the caller has waited for the stream: the
//                        interval that ends at an event counts towards that event's phase, total_ms = the sum of the intervals
//   one bracket          mark() on either side; wait() for the second event where the caller does not wait for the stream;
//                        bracket(&t) reads the time, single(phase) makes it the record's only phase and its total
struct PhaseTimer {
    std::vector<float> ms;                         // the record: one entry per phase
    float total_ms = 0;
    explicit PhaseTimer(int n_phases = 0) : ms((size_t)n_phases, 0.f) {}

    PhaseTimer& begin() {
        used = 0;
        t0 = std::chrono::steady_clock::now();
        return *this;
    }
    int mark(int phase = 0) {
        if (used == ev.size()) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            ev.push_back(e);
            label.push_back(0);
            if (!registered) {
                registered = true;
                g.at_shutdown.push_back([this] {
                    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
                    ev.clear();
                    label.clear();
                    used = 0;
                    registered = false;
                });
            }
        }
        HIPCHK(hipEventRecord(ev[used], g.stream));
        label[used++] = phase;
        return GH_OK;
    }
    int finish() {
        HIPCHK(hipEventSynchronize(ev[used - 1]));
        std::fill(ms.begin(), ms.end(), 0.f);
        for (size_t i = 1; i < used && i <= ms.size(); i++) HIPCHK(hipEventElapsedTime(&ms[i - 1], ev[i - 1], ev[i]));
        total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return GH_OK;
    }
    int finish(int n_phases) {
        ms.assign((size_t)n_phases, 0.f);
        total_ms = 0;
        for (size_t k = 1; k < used; k++) {
            float d = 0;
            HIPCHK(hipEventElapsedTime(&d, ev[k - 1], ev[k]));
            ms[(size_t)label[k]] += d;
            total_ms += d;
        }
        return GH_OK;
    }
    int wait() {
        HIPCHK(hipEventSynchronize(ev[1]));
        return GH_OK;
    }
    int bracket(float* t) {
        HIPCHK(hipEventElapsedTime(t, ev[0], ev[1]));
        return GH_OK;
    }
    int single(int phase) {
        std::fill(ms.begin(), ms.end(), 0.f);
        if (int rc = bracket(&ms[(size_t)phase])) return rc;
        total_ms = ms[(size_t)phase];
        return GH_OK;
    }
    // the body of a *_last_timing: the count of phases written, or an error
    int copy_out(float* phase_ms, int max_phases, float* total) const {
        if ((!phase_ms && max_phases > 0) || max_phases < 0) return null_arg();
        const int cnt = std::min(max_phases, (int)ms.size());
        for (int i = 0; i < cnt; i++) phase_ms[i] = ms[(size_t)i];
        if (total) *total = total_ms;
        return cnt;
    }

private:
    std::vector<hipEvent_t> ev;                    // grown on demand
    std::vector<int> label;                        // phase of the interval that ENDS at event k
    size_t used = 0;
    bool registered = false;
    std::chrono::steady_clock::time_point t0;
};

}  // namespace
