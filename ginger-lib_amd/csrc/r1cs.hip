// r1cs.hip -- the C ABI of include/ginger_hip_r1cs.h: the three constraint matrices of an R1CS instance resident on the
// device, in both orientations, and the sparse products over them.  The schedule of a product is designed on the host
// (r1cs_plan.h: validation, dictionary classes, transposition, level builder -- all of it host-tested); here are the handle
// that keeps its arrays on the device, the kernels that execute it and the reference-shaped calls above the products: the QAP
// maps of Groth16 and, over the same handle and launch helpers, the SAP maps of GM17 (include/ginger_hip_sap.h, sap_rows.h).
// DESIGN.md sections 16 and 16a.
//
// One product: the input vector is converted once to the internal 26 x 29-bit form (r1cs_convert_kernel), level 0 gathers it
// (one lane per segment, r1cs_term per term), the levels above sum partials; the lane that closes a row writes the ABI row.
// Every index a kernel reads was checked on the host when the handle was built (r1cs_check_csr) or was made by the level
// builder; the vectors' lengths are the handle's.
#include <algorithm>
#include <memory>
#include "unit_host.h"
#include "r1cs_plan.h"
#include "sap_rows.h"
#include "../../include/ginger_hip_sap.h"

namespace {

using gh_rt::DevMem;

constexpr int BLOCK = 128;

// ---------------------------------------------------------------------------------------------------- kernels
// xs[i] = x[i] in internal form; scalars (nullable): row i - 1 = the integer x[i] itself (into_repr), i >= 1; aux (nullable):
// the same integer a second time, row i - aux_first, i >= aux_first (the SAP prover's second copy of the aux part)
template <class P>
__global__ void __launch_bounds__(BLOCK)
r1cs_convert_kernel(const uint32_t* __restrict__ x, size_t n, Fp* __restrict__ xs, uint32_t* __restrict__ scalars, uint32_t* __restrict__ aux,
                    size_t aux_first) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const Fp v = fp_from_abi<P>(x + i * 24);
    xs[i] = v;
    const bool to_aux = aux && i >= aux_first;
    if ((scalars && i) || to_aux) {
        Fp one = fp_zero();
        one.l[0] = 1;
        const Fp repr = fp_mul<P>(v, one);
        if (scalars && i) fp_pack(scalars + (i - 1) * 24, repr);
        if (to_aux) fp_pack(aux + (i - aux_first) * 24, repr);
    }
}

// One lane per segment of a level.  GATHER (level 0): the terms are src / code over `in` = the converted input vector;
// otherwise `in` is the partial vector of the level below and every term has coefficient one.
template <class P, bool GATHER>
__global__ void __launch_bounds__(BLOCK)
r1cs_level_kernel(const R1csSeg* __restrict__ segs, uint32_t n_segs, const uint32_t* __restrict__ src, const uint32_t* __restrict__ code,
                  const Fp* __restrict__ in, const Fp* __restrict__ dict, Fp* __restrict__ partials, uint32_t* __restrict__ y) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_segs) return;
    const R1csSeg s = segs[i];
    Fp acc = fp_zero();
#pragma unroll 1
    for (uint32_t j = s.first; j < s.first + s.count; j++) {
        if constexpr (GATHER) r1cs_term<P>(acc, in[src[j]], code[j], dict);
        else acc = fp_add<P>(acc, in[j]);
    }
    if (s.out & R1CS_FINAL) fp_to_abi<P>(y + (size_t)(s.out & ~R1CS_FINAL) * 24, acc);
    else partials[s.out] = acc;
}

// rows [nc, N) of evaluate's three outputs: a[nc] = one, a[nc + i] = z_i for 0 < i < ni, everything else zero
template <class P>
__global__ void __launch_bounds__(BLOCK)
r1cs_tail_kernel(const uint32_t* __restrict__ z, size_t nc, size_t ni, size_t N, uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                 uint32_t* __restrict__ c) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= (N - nc) * 3) return;
    const size_t r = t / 3, m = t % 3;
    uint32_t* dst = (m == 0 ? a : m == 1 ? b : c) + (nc + r) * 24;
    uint32_t w[24];
#pragma unroll
    for (int k = 0; k < 24; k++) w[k] = 0;
    if (m == 0 && r < ni) {
        if (r == 0) fp_pack(w, fp_const<P>(P::COUT));          // 2^768 mod p: one in the ABI's form
        else {
#pragma unroll
            for (int k = 0; k < 24; k++) w[k] = z[r * 24 + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 24; k++) dst[k] = w[k];
}

// a[i] += u[nc + i], i < ni (instance_map_with_evaluation :36-38; both rows in the ABI's form, the sum needs no product)
template <class P>
__global__ void __launch_bounds__(BLOCK)
r1cs_add_inputs_kernel(const uint32_t* __restrict__ u, size_t nc, size_t ni, uint32_t* __restrict__ a) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ni) return;
    fp_pack(a + i * 24, fp_add<P>(fp_unpack(a + i * 24), fp_unpack(u + (nc + i) * 24)));
}

// ---- GM17's R1CS -> SAP maps (include/ginger_hip_sap.h): the lanes are sap_rows.h's, which the CPU tests run on the host
// witness rows: one lane per constraint, then one per input (the row of ones first), then one per padding row
template <class P>
__global__ void __launch_bounds__(BLOCK)
sap_rows_kernel(SapShape sh, const uint32_t* __restrict__ az, const uint32_t* __restrict__ bz, const uint32_t* __restrict__ cz,
                const uint32_t* __restrict__ z, uint32_t* __restrict__ a, uint32_t* __restrict__ c, uint32_t* __restrict__ scalars,
                uint32_t* __restrict__ aux, uint32_t* __restrict__ full) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < sh.rows_lanes()) sap_rows_lane<P>(sh, t, az, bz, cz, z, a, c, scalars, aux, full);
}

// u -> p, m, q in the internal form, the inputs of the three transposed products: xs[i], xs[nc + i], xs[2 nc + i]
template <class P>
__global__ void __launch_bounds__(BLOCK)
sap_split_kernel(const uint32_t* __restrict__ u, uint64_t nc, Fp* __restrict__ xs) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nc) return;
    Fp p, m, q;
    sap_split<P>(u, i, p, m, q);
    xs[i] = p;
    xs[nc + i] = m;
    xs[2 * nc + i] = q;
}

// one lane per row of the instance map's a and c
template <class P>
__global__ void __launch_bounds__(BLOCK)
sap_instance_finish_kernel(SapShape sh, const uint32_t* __restrict__ at_p, const uint32_t* __restrict__ bt_m, const uint32_t* __restrict__ ct_q,
                           const uint32_t* __restrict__ u, uint32_t* __restrict__ a, uint32_t* __restrict__ c) {
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < sh.full_rows()) sap_instance_row<P>(sh, j, at_p, bt_m, ct_q, u, a, c);
}

// ---------------------------------------------------------------------------------------------------- the handle
struct DevLevel {
    DevMem segs;
    uint32_t n_segs = 0, n_partials = 0;
    size_t partial_off = 0;                        // of this level's partials inside the call's partial scratch
};
struct DevPlan {
    DevMem src, code;
    std::vector<DevLevel> levels;
    uint32_t rows = 0, n_src = 0, longest = 0;
    uint64_t nnz = 0;
};

}  // namespace

struct gh_r1cs {
    static constexpr uint32_t MAGIC = 0x67685231u;
    uint32_t magic = MAGIC;
    gh_field_t field;
    size_t ni = 0, na = 0, nc = 0;
    uint32_t log_n = 0, segment = 0;
    DevPlan plan[3][2];
    DevMem dict[3];                                // each matrix's dictionary, internal form
    uint32_t class_counts[R1CS_CLASSES] = {};
    size_t device_bytes = 0, max_partials = 0;
    int max_levels = 0;
    ~gh_r1cs() { magic = 0; }
};

namespace {

gh_r1cs* checked(gh_r1cs_t h) {
    if (!h || h->magic != gh_r1cs::MAGIC) { g_err = "not an R1CS handle"; return nullptr; }
    return h;
}

// one event after every launch, told apart by phase once the stream has been waited for (unit_host.h: labelled intervals)
PhaseTimer g_tm;

// ---- upload
int upload_plan(const R1csPlan& p, DevPlan& d, size_t& bytes) {
    d.rows = p.rows;
    d.n_src = p.n_src;
    d.longest = p.longest;
    d.nnz = p.src.size();
    int rc;
    if (d.nnz) {
        if ((rc = d.src.alloc(d.nnz * 4)) || (rc = d.code.alloc(d.nnz * 4))) return rc;
        HIPCHK(hipMemcpy(d.src.get(), p.src.data(), d.nnz * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.code.get(), p.code.data(), d.nnz * 4, hipMemcpyHostToDevice));
        bytes += d.nnz * 8;
    }
    size_t off = 0;
    d.levels.resize(p.levels.size());
    for (size_t l = 0; l < p.levels.size(); l++) {
        DevLevel& dl = d.levels[l];
        dl.n_segs = (uint32_t)p.levels[l].segs.size();
        dl.n_partials = p.levels[l].n_partials;
        dl.partial_off = off;
        off += dl.n_partials;
        const size_t b = (size_t)dl.n_segs * sizeof(R1csSeg);
        if ((rc = dl.segs.alloc(b))) return rc;
        HIPCHK(hipMemcpy(dl.segs.get(), p.levels[l].segs.data(), b, hipMemcpyHostToDevice));
        bytes += b;
    }
    return GH_OK;
}

// the checks of gh_r1cs_upload that need the field
template <class P> const char* check_values(size_t ni, size_t nc, const gh_r1cs_matrix_t* m, uint32_t* log_n, bool* domain_ok) {
    for (int k = 0; k < 3; k++) {
        if (m[k].num_coeffs && !m[k].coeff_values) return "null coeff_values";
        if (m[k].num_coeffs >> 29) return "a dictionary holds 2^29 entries or more";
        for (size_t i = 0; i < m[k].num_coeffs; i++)
            if (!below<P>(m[k].coeff_values + 12 * i)) return "a dictionary value is not below the modulus";
    }
    *domain_ok = r1cs_domain<P>((uint64_t)nc + ni, log_n);
    return nullptr;
}

template <class P> int build(gh_r1cs* h, const gh_r1cs_matrix_t* m) {
    const uint64_t nv = h->ni + h->na;
    std::vector<uint64_t> t_ptr;
    std::vector<uint32_t> t_col, t_coeff, dict_code;
    std::vector<Fp> dict;
    R1csPlan plan;
    int rc;
    for (int k = 0; k < 3; k++) {
        uint32_t counts[R1CS_CLASSES];
        r1cs_classify<P>(m[k].coeff_values, m[k].num_coeffs, dict, dict_code, counts);
        for (uint32_t c = 0; c < R1CS_CLASSES; c++) h->class_counts[c] += counts[c];
        const size_t db = std::max<size_t>(dict.size(), 1) * sizeof(Fp);
        if ((rc = h->dict[k].alloc(db))) return rc;
        if (!dict.empty()) HIPCHK(hipMemcpy(h->dict[k].get(), dict.data(), dict.size() * sizeof(Fp), hipMemcpyHostToDevice));
        h->device_bytes += db;
        for (int tr = 0; tr < 2; tr++) {
            if (tr == 0) r1cs_build_plan(h->nc, nv, m[k].row_ptr, m[k].col, m[k].coeff_id, dict_code, h->segment, plan);
            else {
                r1cs_transpose(h->nc, nv, m[k].row_ptr, m[k].col, m[k].coeff_id, t_ptr, t_col, t_coeff);
                r1cs_build_plan(nv, h->nc, t_ptr.data(), t_col.data(), t_coeff.data(), dict_code, h->segment, plan);
            }
            if ((rc = upload_plan(plan, h->plan[k][tr], h->device_bytes))) return rc;
            h->max_partials = std::max(h->max_partials, plan.total_partials());
            h->max_levels = std::max(h->max_levels, (int)plan.levels.size());
        }
    }
    return GH_OK;
}

// ---- the launches, all on g.stream without a wait
struct Scratch {
    Fp* xs = nullptr;
    Fp* part = nullptr;
};
// xs_rows: the converted input vector(s) of the call; 0 = one vector of either orientation
int get_scratch(const gh_r1cs* h, Scratch& s, size_t xs_rows = 0) {
    const size_t n = std::max<size_t>(std::max(std::max(h->ni + h->na, h->nc), xs_rows), 1);
    int rc;
    if ((rc = gh_rt::pool_get("r1cs_x", n * sizeof(Fp), (void**)&s.xs))) return rc;
    return gh_rt::pool_get("r1cs_part", std::max<size_t>(h->max_partials, 1) * sizeof(Fp), (void**)&s.part);
}

template <class P> int convert(const void* d_x, size_t n, const Scratch& s, void* d_scalars, void* d_aux = nullptr, size_t aux_first = 0) {
    if (!n) return g_tm.mark(0);
    GH_LAUNCH((r1cs_convert_kernel<P>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_x, n, s.xs, (uint32_t*)d_scalars,
              (uint32_t*)d_aux, aux_first);
    return g_tm.mark(0);
}

// y = M x over the converted vector in s.xs
template <class P> int product(const gh_r1cs* h, int which, int tr, const Scratch& s, void* d_y) {
    const DevPlan& p = h->plan[which][tr];
    const Fp* dict = h->dict[which].as<Fp>();
    for (size_t l = 0; l < p.levels.size(); l++) {
        const DevLevel& lv = p.levels[l];
        if (lv.n_segs) {
            Fp* out = s.part + lv.partial_off;
            if (l == 0)
                GH_LAUNCH((r1cs_level_kernel<P, true>), dim3(blocks(lv.n_segs, BLOCK)), dim3(BLOCK), 0, g.stream, lv.segs.as<R1csSeg>(), lv.n_segs,
                          p.src.as<uint32_t>(), p.code.as<uint32_t>(), (const Fp*)s.xs, dict, out, (uint32_t*)d_y);
            else
                GH_LAUNCH((r1cs_level_kernel<P, false>), dim3(blocks(lv.n_segs, BLOCK)), dim3(BLOCK), 0, g.stream, lv.segs.as<R1csSeg>(), lv.n_segs,
                          (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const Fp*)(s.part + p.levels[l - 1].partial_off), dict, out,
                          (uint32_t*)d_y);
        }
        if (int rc = g_tm.mark(1 + (int)l)) return rc;
    }
    HIPCHK(hipGetLastError());
    return GH_OK;
}

int finish(const gh_r1cs* h) {
    HIPCHK(hipStreamSynchronize(g.stream));
    return g_tm.finish(h->max_levels + 2);
}

template <class P> int matvec(const gh_r1cs* h, int which, int tr, const void* d_x, void* d_y) {
    Scratch s;
    int rc;
    if ((rc = get_scratch(h, s)) || (rc = g_tm.begin().mark(0))) return rc;
    if ((rc = convert<P>(d_x, h->plan[which][tr].n_src, s, nullptr)) || (rc = product<P>(h, which, tr, s, d_y))) return rc;
    return finish(h);
}

// the evaluation of :105-119, :141-151, no wait
template <class P> int evaluate_launch(const gh_r1cs* h, const void* d_z, void* d_a, void* d_b, void* d_c, void* d_scalars) {
    Scratch s;
    int rc;
    if ((rc = get_scratch(h, s)) || (rc = g_tm.begin().mark(0))) return rc;
    if ((rc = convert<P>(d_z, h->ni + h->na, s, d_scalars))) return rc;
    void* out[3] = {d_a, d_b, d_c};
    for (int k = 0; k < 3; k++)
        if ((rc = product<P>(h, k, 0, s, out[k]))) return rc;
    const size_t N = (size_t)1 << h->log_n;
    GH_LAUNCH((r1cs_tail_kernel<P>), dim3(blocks((N - h->nc) * 3, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_z, h->nc, h->ni, N, (uint32_t*)d_a,
              (uint32_t*)d_b, (uint32_t*)d_c);
    HIPCHK(hipGetLastError());
    return g_tm.mark(h->max_levels + 1);
}

template <class P> int instance_map_launch(const gh_r1cs* h, const void* d_u, void* d_a, void* d_b, void* d_c) {
    Scratch s;
    int rc;
    if ((rc = get_scratch(h, s)) || (rc = g_tm.begin().mark(0))) return rc;
    if ((rc = convert<P>(d_u, h->nc, s, nullptr))) return rc;
    void* out[3] = {d_a, d_b, d_c};
    for (int k = 0; k < 3; k++)
        if ((rc = product<P>(h, k, 1, s, out[k]))) return rc;
    GH_LAUNCH((r1cs_add_inputs_kernel<P>), dim3(blocks(h->ni, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_u, h->nc, h->ni, (uint32_t*)d_a);
    HIPCHK(hipGetLastError());
    return g_tm.mark(h->max_levels + 1);
}

// ---- GM17's R1CS -> SAP maps: the same conversion, products and marks, then one SAP kernel
// the shape, or GH_E_UNSUPPORTED where EvaluationDomain::new(2 nc + 2 (ni - 1) + 1) would be None; no device call
template <class P> int sap_shape_of(const gh_r1cs* h, SapShape* sh, uint32_t* log_n) {
    sh->ni = h->ni;
    sh->nc = h->nc;
    sh->nv = h->ni + h->na;
    if (!r1cs_domain<P>(sh->domain_arg(), log_n)) { g_err = "the SAP domain exceeds the field's 2-adicity"; return GH_E_UNSUPPORTED; }
    sh->N = (uint64_t)1 << *log_n;
    return GH_OK;
}
int sap_shape(const gh_r1cs* h, SapShape* sh, uint32_t* log_n) {
    return h->field == GH_MNT4753_FR ? sap_shape_of<P6>(h, sh, log_n) : sap_shape_of<P4>(h, sh, log_n);
}

// the three product vectors of a SAP call, in the ABI's form: rows of the longer orientation each
int get_sap_products(const gh_r1cs* h, uint32_t* out[3]) {
    const size_t rows = std::max<size_t>(std::max(h->ni + h->na, h->nc), 1);
    uint32_t* base;
    if (int rc = gh_rt::pool_get("sap_prod", 3 * rows * 96, (void**)&base)) return rc;
    for (int k = 0; k < 3; k++) out[k] = base + (size_t)k * rows * 24;
    return GH_OK;
}

// r1cs_to_sap.rs:125-189, :206-232, no wait.  d_full: null, or full_rows() rows whose first nv the caller has filled.
template <class P>
int sap_rows_launch(const gh_r1cs* h, const SapShape& sh, const void* d_z, void* d_a, void* d_c, void* d_scalars, void* d_aux, void* d_full) {
    Scratch s;
    uint32_t* prod[3];
    int rc;
    if ((rc = get_scratch(h, s)) || (rc = get_sap_products(h, prod)) || (rc = g_tm.begin().mark(0))) return rc;
    if ((rc = convert<P>(d_z, sh.nv, s, d_scalars, d_aux, sh.ni))) return rc;
    for (int k = 0; k < 3; k++)
        if ((rc = product<P>(h, k, 0, s, prod[k]))) return rc;
    GH_LAUNCH((sap_rows_kernel<P>), dim3(blocks(sh.rows_lanes(), BLOCK)), dim3(BLOCK), 0, g.stream, sh, (const uint32_t*)prod[0], (const uint32_t*)prod[1],
              (const uint32_t*)prod[2], (const uint32_t*)d_z, (uint32_t*)d_a, (uint32_t*)d_c, (uint32_t*)d_scalars, (uint32_t*)d_aux, (uint32_t*)d_full);
    HIPCHK(hipGetLastError());
    return g_tm.mark(h->max_levels + 1);
}

// r1cs_to_sap.rs:37-94, no wait: p, m, q side by side in the conversion scratch, one transposed product over each
template <class P> int sap_instance_launch(const gh_r1cs* h, const SapShape& sh, const void* d_u, void* d_a, void* d_c) {
    Scratch s;
    uint32_t* prod[3];
    int rc;
    if ((rc = get_scratch(h, s, 3 * sh.nc)) || (rc = get_sap_products(h, prod)) || (rc = g_tm.begin().mark(0))) return rc;
    if (sh.nc) GH_LAUNCH((sap_split_kernel<P>), dim3(blocks(sh.nc, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_u, sh.nc, s.xs);
    if ((rc = g_tm.mark(0))) return rc;
    for (int k = 0; k < 3; k++) {
        Scratch sk = s;
        sk.xs = s.xs + (size_t)k * sh.nc;
        if ((rc = product<P>(h, k, 1, sk, prod[k]))) return rc;
    }
    GH_LAUNCH((sap_instance_finish_kernel<P>), dim3(blocks(sh.full_rows(), BLOCK)), dim3(BLOCK), 0, g.stream, sh, (const uint32_t*)prod[0],
              (const uint32_t*)prod[1], (const uint32_t*)prod[2], (const uint32_t*)d_u, (uint32_t*)d_a, (uint32_t*)d_c);
    HIPCHK(hipGetLastError());
    return g_tm.mark(h->max_levels + 1);
}

int to_device(void* d, const void* hsrc, size_t bytes) { return up((uint8_t*)d, (const uint8_t*)hsrc, bytes); }
int to_host(void* hdst, const void* d, size_t bytes) { return down((uint8_t*)hdst, (const uint8_t*)d, bytes); }

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_r1cs_upload(gh_field_t field, size_t num_inputs, size_t num_aux, size_t num_constraints, const gh_r1cs_matrix_t* m,
                   uint32_t segment_terms, gh_r1cs_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!m || !out) return null_arg();
    *out = nullptr;
    if (int rc = field_ok(field)) return rc;
    if (num_inputs == 0) { g_err = "num_inputs is 0: variable 0 is the constant one"; return GH_E_BAD_ARG; }
    if (segment_terms == 1) { g_err = "segment_terms must be 0 or at least 2"; return GH_E_BAD_ARG; }
    size_t nv;
    if (__builtin_add_overflow(num_inputs, num_aux, &nv) || nv >= R1CS_FINAL || num_constraints >= R1CS_FINAL) {
        g_err = "2^31 variables or constraints or more";
        return GH_E_BAD_ARG;
    }
    for (int k = 0; k < 3; k++)
        if (const char* why = r1cs_check_csr(num_constraints, nv, m[k].row_ptr, m[k].col, m[k].coeff_id, m[k].num_coeffs)) {
            g_err = why;
            return GH_E_BAD_ARG;
        }
    uint32_t log_n = 0;
    bool domain_ok = false;
    if (const char* why = GH_FIELD_DISPATCH(field, check_values, num_inputs, num_constraints, m, &log_n, &domain_ok)) {
        g_err = why;
        return GH_E_BAD_ARG;
    }
    if (!domain_ok) { g_err = "the QAP domain exceeds the field's 2-adicity"; return GH_E_UNSUPPORTED; }
    if (int rc = ensure_init()) return rc;
    std::unique_ptr<gh_r1cs> h(new gh_r1cs);
    h->field = field;
    h->ni = num_inputs;
    h->na = num_aux;
    h->nc = num_constraints;
    h->log_n = log_n;
    h->segment = segment_terms ? segment_terms : R1CS_DEFAULT_SEGMENT;
    if (int rc = GH_FIELD_DISPATCH(field, build, h.get(), m)) return rc;
    *out = h.release();
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_free(gh_r1cs_t handle) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!handle) return GH_OK;
    gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (g.ready) HIPCHK(hipStreamSynchronize(g.stream));
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_info(gh_r1cs_t handle, gh_r1cs_info_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!out) return null_arg();
    memset(out, 0, sizeof *out);
    out->num_inputs = h->ni;
    out->num_aux = h->na;
    out->num_constraints = h->nc;
    out->log_n = h->log_n;
    out->segment_terms = h->segment;
    for (int k = 0; k < 3; k++)
        for (int tr = 0; tr < 2; tr++) {
            out->nnz[k][tr] = h->plan[k][tr].nnz;
            out->longest_row[k][tr] = h->plan[k][tr].longest;
            out->levels[k][tr] = (uint32_t)h->plan[k][tr].levels.size();
        }
    for (uint32_t c = 0; c < R1CS_CLASSES; c++) out->class_counts[c] = h->class_counts[c];
    out->device_bytes = h->device_bytes;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_matvec_dev(gh_r1cs_t handle, int which, int transpose, const void* d_x, void* d_y) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (which < 0 || which > 2) { g_err = "which must be 0 (A), 1 (B) or 2 (C)"; return GH_E_BAD_ARG; }
    const DevPlan& p = h->plan[which][transpose ? 1 : 0];
    if ((p.n_src && !d_x) || (p.rows && !d_y)) return null_arg();
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(h->field, matvec, h, which, transpose ? 1 : 0, d_x, d_y);
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_evaluate_dev(gh_r1cs_t handle, const void* d_assignment, void* d_a, void* d_b, void* d_c) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!d_assignment || !d_a || !d_b || !d_c) return null_arg();
    if (int rc = ensure_init()) return rc;
    if (int rc = GH_FIELD_DISPATCH(h->field, evaluate_launch, h, d_assignment, d_a, d_b, d_c, nullptr)) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_evaluate(gh_r1cs_t handle, const uint64_t* assignment, uint64_t* a, uint64_t* b, uint64_t* c) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!assignment || !a || !b || !c) return null_arg();
    if (int rc = ensure_init()) return rc;
    const size_t zb = (h->ni + h->na) * 96, ob = ((size_t)1 << h->log_n) * 96;
    DevMem dz, da, db, dc;
    int rc;
    if ((rc = dz.alloc(zb)) || (rc = da.alloc(ob)) || (rc = db.alloc(ob)) || (rc = dc.alloc(ob)) || (rc = to_device(dz.get(), assignment, zb))) return rc;
    if ((rc = GH_FIELD_DISPATCH(h->field, evaluate_launch, h, dz.get(), da.get(), db.get(), dc.get(), nullptr))) return rc;
    if ((rc = to_host(a, da.get(), ob)) || (rc = to_host(b, db.get(), ob)) || (rc = to_host(c, dc.get(), ob))) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_witness_map_dev(gh_r1cs_t handle, const void* d_assignment, const uint64_t* d1, const uint64_t* d2, const uint64_t* d3,
                            void* d_h, void* d_scalars) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!d_assignment || !d1 || !d2 || !d3 || !d_h) return null_arg();
    if (int rc = ensure_init()) return rc;
    const size_t ob = ((size_t)1 << h->log_n) * 96;
    void *da, *db, *dc;
    int rc;
    if ((rc = pool_get("r1cs_a", ob, &da)) || (rc = pool_get("r1cs_b", ob, &db)) || (rc = pool_get("r1cs_c", ob, &dc))) return rc;
    if ((rc = GH_FIELD_DISPATCH(h->field, evaluate_launch, h, d_assignment, da, db, dc, d_scalars))) return rc;
    if ((rc = witness_map(h->field, da, db, dc, h->log_n, d1, d2, d3, d_h))) return rc;      // waits for the stream at its end
    return g_tm.finish(h->max_levels + 2);
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_instance_map_dev(gh_r1cs_t handle, const void* d_u, void* d_a, void* d_b, void* d_c) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!d_u || !d_a || !d_b || !d_c) return null_arg();
    if (int rc = ensure_init()) return rc;
    if (int rc = GH_FIELD_DISPATCH(h->field, instance_map_launch, h, d_u, d_a, d_b, d_c)) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_instance_map(gh_r1cs_t handle, const uint64_t* u, uint64_t* a, uint64_t* b, uint64_t* c) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!u || !a || !b || !c) return null_arg();
    if (int rc = ensure_init()) return rc;
    const size_t ub = ((size_t)1 << h->log_n) * 96, ob = (h->ni + h->na) * 96;
    DevMem du, da, db, dc;
    int rc;
    if ((rc = du.alloc(ub)) || (rc = da.alloc(ob)) || (rc = db.alloc(ob)) || (rc = dc.alloc(ob)) || (rc = to_device(du.get(), u, ub))) return rc;
    if ((rc = GH_FIELD_DISPATCH(h->field, instance_map_launch, h, du.get(), da.get(), db.get(), dc.get()))) return rc;
    if ((rc = to_host(a, da.get(), ob)) || (rc = to_host(b, db.get(), ob)) || (rc = to_host(c, dc.get(), ob))) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_r1cs_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

// ---- include/ginger_hip_sap.h
int gh_sap_info(gh_r1cs_t handle, gh_sap_info_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!out) return null_arg();
    SapShape sh;
    uint32_t log_n;
    if (int rc = sap_shape(h, &sh, &log_n)) return rc;
    memset(out, 0, sizeof *out);
    out->sap_log_n = log_n;
    out->sap_num_variables = sh.sap_nv();
    const size_t longer = std::max<size_t>(std::max<size_t>(sh.nv, sh.nc), 1);
    out->scratch_bytes = std::max<size_t>(longer, 3 * sh.nc) * sizeof(Fp) + std::max<size_t>(h->max_partials, 1) * sizeof(Fp) + 3 * longer * 96 +
                         2 * sh.N * 96;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_sap_rows_dev(gh_r1cs_t handle, const void* d_assignment, void* d_a, void* d_c, void* d_scalars, void* d_aux_scalars) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!d_assignment || !d_a || !d_c) return null_arg();
    SapShape sh;
    uint32_t log_n;
    if (int rc = sap_shape(h, &sh, &log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    if (int rc = GH_FIELD_DISPATCH(h->field, sap_rows_launch, h, sh, d_assignment, d_a, d_c, d_scalars, d_aux_scalars, nullptr)) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_sap_rows(gh_r1cs_t handle, const uint64_t* assignment, uint64_t* a, uint64_t* c, uint64_t* full) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!assignment || !a || !c || !full) return null_arg();
    SapShape sh;
    uint32_t log_n;
    if (int rc = sap_shape(h, &sh, &log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t zb = sh.nv * 96, ob = sh.N * 96, fb = sh.full_rows() * 96;
    DevMem dz, da, dc, df;
    int rc;
    if ((rc = dz.alloc(zb)) || (rc = da.alloc(ob)) || (rc = dc.alloc(ob)) || (rc = df.alloc(fb))) return rc;
    if ((rc = to_device(dz.get(), assignment, zb)) || (rc = to_device(df.get(), assignment, zb))) return rc;      // full = z || e || f
    if ((rc = GH_FIELD_DISPATCH(h->field, sap_rows_launch, h, sh, dz.get(), da.get(), dc.get(), nullptr, nullptr, df.get()))) return rc;
    if ((rc = to_host(a, da.get(), ob)) || (rc = to_host(c, dc.get(), ob)) || (rc = to_host(full, df.get(), fb))) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_sap_r1cs_witness_map_dev(gh_r1cs_t handle, const void* d_assignment, const uint64_t* d1, const uint64_t* d2, void* d_h, void* d_scalars,
                                void* d_aux_scalars) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!d_assignment || !d1 || !d2 || !d_h) return null_arg();
    SapShape sh;
    uint32_t log_n;
    if (int rc = sap_shape(h, &sh, &log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    void *da, *dc;
    int rc;
    if ((rc = pool_get("sap_a", sh.N * 96, &da)) || (rc = pool_get("sap_c", sh.N * 96, &dc))) return rc;
    if ((rc = GH_FIELD_DISPATCH(h->field, sap_rows_launch, h, sh, d_assignment, da, dc, d_scalars, d_aux_scalars, nullptr))) return rc;
    if ((rc = sap_witness_map(h->field, da, dc, log_n, d1, d2, d_h))) return rc;                  // waits for the stream at its end
    return g_tm.finish(h->max_levels + 2);
} catch (...) { return gh_rt::api_exception(); }

int gh_sap_instance_map_dev(gh_r1cs_t handle, const void* d_u, void* d_a, void* d_c) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!d_u || !d_a || !d_c) return null_arg();
    SapShape sh;
    uint32_t log_n;
    if (int rc = sap_shape(h, &sh, &log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    if (int rc = GH_FIELD_DISPATCH(h->field, sap_instance_launch, h, sh, d_u, d_a, d_c)) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_sap_instance_map(gh_r1cs_t handle, const uint64_t* u, uint64_t* a, uint64_t* c) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const gh_r1cs* h = checked(handle);
    if (!h) return GH_E_BAD_HANDLE;
    if (!u || !a || !c) return null_arg();
    SapShape sh;
    uint32_t log_n;
    if (int rc = sap_shape(h, &sh, &log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t ub = sh.N * 96, ob = sh.full_rows() * 96;
    DevMem du, da, dc;
    int rc;
    if ((rc = du.alloc(ub)) || (rc = da.alloc(ob)) || (rc = dc.alloc(ob)) || (rc = to_device(du.get(), u, ub))) return rc;
    if ((rc = GH_FIELD_DISPATCH(h->field, sap_instance_launch, h, sh, du.get(), da.get(), dc.get()))) return rc;
    if ((rc = to_host(a, da.get(), ob)) || (rc = to_host(c, dc.get(), ob))) return rc;
    return finish(h);
} catch (...) { return gh_rt::api_exception(); }

int gh_sap_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
