// pairing.hip -- the C ABI of include/ginger_hip_pairing.h and include/ginger_hip_gm17.h, and the two validating verifiers of
// include/ginger_hip_points.h: the entry points take the lock, find
// the engine's PairingOps and call them.  The kernels and the host steps are the templates of pairing_impl.h and
// gm17_verify_impl.h; this unit instantiates them for MNT4-753, pairing_mnt6753.hip for MNT6-753.  DESIGN.md sections 14, 14b.
#include "pairing_impl.h"
#include "gm17_verify_impl.h"
GH_DEFINE_PAIRING_OPS(gh::Mnt4Pairing, pairing_ops_mnt4753)

namespace {

int g_last_engine = GH_PAIRING_MNT4753;            // whose timing record gh_pairing_last_timing reports
int g_last_gm17_engine = GH_PAIRING_MNT4753;       // the same for gh_gm17_last_timing

const gh_rt::PairingOps* ops_of_engine(int engine) {
    switch (engine) {
        case GH_PAIRING_MNT4753: return gh_rt::pairing_ops_mnt4753();
        case GH_PAIRING_MNT6753: return gh_rt::pairing_ops_mnt6753();
    }
    g_err = "unknown pairing engine";
    return nullptr;
}
int checked_handle(gh_groth16_vk* h) {
    if (!h || h->magic != gh_groth16_vk::MAGIC) { g_err = "not a Groth16 verifying key"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}
int checked_handle(gh_gm17_vk* h) {
    if (!h || h->magic != gh_gm17_vk::MAGIC) { g_err = "not a GM17 verifying key"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}

// what the verify entry points begin with: the lock, the Trim, the handle check and the PairingOps of the key's engine, which
// `last` records for the scheme's last_timing; then call(ops)
template <class H, class F> int with_key(H* h, int& last, F call) {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    const gh_rt::PairingOps* ops = ops_of_engine(h->engine);
    if (!ops) return GH_E_BAD_HANDLE;
    last = h->engine;
    return call(ops);
}
template <class H> int vk_free(H* h) {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    if (!h) return GH_OK;
    if (int rc = checked_handle(h)) return rc;
    delete h;
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_pairing_product(int engine, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
                       size_t k, uint64_t* out_gt) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    const PairingOps* ops = ops_of_engine(engine);
    if (!ops) return GH_E_BAD_ARG;
    g_last_engine = engine;
    return ops->product(g1_xy, g1_inf, g2_xy, g2_inf, n, k, out_gt);
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_vk_create(int engine, const uint64_t* alpha_g1_beta_g2, const uint64_t* gamma_g2_xy, const uint64_t* delta_g2_xy,
                         const uint64_t* gamma_abc_g1_xy, size_t n_abc, gh_groth16_vk_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!out) return null_arg();
    *out = nullptr;
    const PairingOps* ops = ops_of_engine(engine);
    if (!ops) return GH_E_BAD_ARG;
    return ops->vk_create(engine, alpha_g1_beta_g2, gamma_g2_xy, delta_g2_xy, gamma_abc_g1_xy, n_abc, out);
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_vk_free(gh_groth16_vk_t h) try {
    return vk_free(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_verify(gh_groth16_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                      const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) try {
    return with_key(h, g_last_engine, [&](const PairingOps* ops) {
        return ops->verify(h, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status);
    });
} catch (...) { return gh_rt::api_exception(); }

int gh_pairing_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return ops_of_engine(g_last_engine)->last_timing(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

// ---- include/ginger_hip_points.h: the verifiers that validate their proof points first (the rest of that header: points.hip)
int gh_groth16_verify_checked(gh_groth16_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                              const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status,
                              uint8_t* out_point_status) try {
    return with_key(h, g_last_engine, [&](const PairingOps* ops) {
        return ops->verify_validated(h, 0, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status, out_point_status);
    });
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_verify_compressed(gh_groth16_vk_t h, const uint64_t* a_x, const uint8_t* a_flags, const uint64_t* b_x, const uint8_t* b_flags,
                                 const uint64_t* c_x, const uint8_t* c_flags, const uint64_t* inputs, size_t n, size_t n_inputs,
                                 uint8_t* out_status, uint8_t* out_point_status) try {
    return with_key(h, g_last_engine, [&](const PairingOps* ops) {
        return ops->verify_validated(h, 1, a_x, a_flags, b_x, b_flags, c_x, c_flags, inputs, n, n_inputs, out_status, out_point_status);
    });
} catch (...) { return gh_rt::api_exception(); }

// ---- include/ginger_hip_gm17.h
int gh_gm17_vk_create(int engine, const uint64_t* g_alpha_g1_xy, const uint64_t* h_beta_g2_xy, const uint64_t* g_gamma_g1_xy,
                      const uint64_t* h_gamma_g2_xy, const uint64_t* h_g2_xy, const uint64_t* query_g1_xy, size_t n_query, gh_gm17_vk_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!out) return null_arg();
    *out = nullptr;
    const PairingOps* ops = ops_of_engine(engine);
    if (!ops) return GH_E_BAD_ARG;
    return ops->gm17_vk_create(engine, g_alpha_g1_xy, h_beta_g2_xy, g_gamma_g1_xy, h_gamma_g2_xy, h_g2_xy, query_g1_xy, n_query, out);
} catch (...) { return gh_rt::api_exception(); }

int gh_gm17_vk_free(gh_gm17_vk_t h) try {
    return vk_free(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_gm17_verify(gh_gm17_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                   const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) try {
    return with_key(h, g_last_gm17_engine, [&](const PairingOps* ops) {
        return ops->gm17_verify(h, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status);
    });
} catch (...) { return gh_rt::api_exception(); }

int gh_gm17_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return ops_of_engine(g_last_gm17_engine)->gm17_last_timing(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
