// C ABI of the GMM-VB data-pass engine (see include/gmmvb.h for the contract and the reference
// call sites each entry point replaces).
// This unit: workspace life cycle, parameters and drift hints, pass counters and the policy exchange of row shards, row
// preparation.  gmmvb_estep is capi_estep.hip, gmmvb_mstep capi_mstep.hip, the read-outs capi_readout.hip.
#include "capi_internal.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace gmmvb {
int fail(int code, const char* what, hipError_t e) {
    g_err = what;
    if (e != hipSuccess) {
        g_err += ": ";
        g_err += hipGetErrorString(e);
    }
    return code;
}
}  // namespace gmmvb

namespace {
// the sizes workspace_plan.h needs from the kernels' translation units, for K components of D features
KernelSizes kernel_sizes(int K, int D) {
    KernelSizes ks;
    ks.max_tiles = kMaxTiles;
    ks.t1_splits = GMMVB_T1_SPLITS;
    ks.sel_rows = kSelRows;
    ks.lse_rows = kLseRows;
    ks.scan_parts = kScanParts;
    ks.rec_slots = kRecSlots;
    ks.generic_rows = generic_rows(D);
    if (D > 32 * kMaxTiles) return ks;
    const int T = feature_tiles(D, kMaxTiles);
    ks.mstep_components_per_wg = mstep_components_per_wg(T, false);
    ks.slab_len = slab_len(T);
    ks.estep_image_doubles = estep_image_doubles(T);
    ks.estep_tri_image_doubles = estep_tri_image_doubles();
    ks.estep_bound_blocks = estep_bound_blocks(T);
    ks.estep_i8_image_bytes = estep_i8_image_bytes(D, 0);
    ks.estep_i8_bound_image_bytes = estep_i8_image_bytes(D, 1);
    ks.estep_i8_digit_row_bytes = estep_i8_digit_row_bytes(D);
    ks.proj_image_len = proj_image_len(K, D);
    ks.proj_const_len = proj_const_len(K);
    return ks;
}

// where the workspace keeps the pointer of each buffer of workspace_plan.h: the field of the same name
struct Slots {
    void** at[kBufCount];
#define GMMVB_X(name) (void**)&ws->name,
    explicit Slots(gmmvb_workspace* ws) : at{GMMVB_WORKSPACE_BUFFERS(GMMVB_X)} {}
#undef GMMVB_X
};

struct HipAllocator {
    hipError_t err = hipSuccess;
    void* get(int64_t bytes, bool pinned) {
        void* p = nullptr;
        err = pinned ? hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) : hipMalloc(&p, (size_t)bytes);
        return err == hipSuccess ? p : nullptr;
    }
    bool zero(void* p, int64_t bytes, bool pinned) {
        if (pinned) std::memset(p, 0, (size_t)bytes);
        else err = hipMemset(p, 0, (size_t)bytes);
        return err == hipSuccess;
    }
    void release(void* p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
};

// the events, and what the kernels need set before their first launch
hipError_t init_workspace(gmmvb_workspace* ws) {
    hipError_t e = hipEventCreateWithFlags(&ws->ctr_ev, hipEventDisableTiming);
    if (ws->generic) {
        const int lds = (int)((size_t)ws->D * generic_rows(ws->D) * sizeof(double));
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)estep_generic_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)estep_generic_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        return e;
    }
    // the policy table at this shape, and the events its calibration records around the workspace's own first bulk passes
    ws->pt.init(ws->T, estep_bound_blocks(ws->T) ? (ws->D + 31) / 32 : 0);
    for (int i = 0; i < 6 && e == hipSuccess && ws->prune != 0; ++i) e = hipEventCreate(&ws->cal_ev[i]);
    return e;
}
}  // namespace

extern "C" {

int gmmvb_abi_version(void) { return GMMVB_ABI_VERSION; }
const char* gmmvb_last_error(void) { return g_err.c_str(); }

int64_t gmmvb_stats_len(int K, int D) {
    if (K < 1 || D < 1) return -1;
    return (int64_t)K * (2 + (int64_t)D + (int64_t)D * D);
}

static int create_workspace(int K, int D, int x_dtype, int64_t max_rows, gmmvb_workspace* first, gmmvb_workspace** out) {
    if (!out) return fail(GMMVB_EINVAL, "out is null");
    *out = nullptr;
    if (K < 1 || D < 1 || max_rows < 1) return fail(GMMVB_EINVAL, "K, D and max_rows must be positive");
    if (x_dtype != GMMVB_F32 && x_dtype != GMMVB_F64) return fail(GMMVB_EINVAL, "x_dtype must be GMMVB_F32 or GMMVB_F64");
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "hipGetDevice", e);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "hipGetDeviceProperties", e);

    gmmvb_workspace* ws = new (std::nothrow) gmmvb_workspace();
    gmmvb_scratch* group = first ? first->scratch : new (std::nothrow) gmmvb_scratch();
    if (!ws || !group) {
        delete ws;
        if (!first) delete group;
        return fail(GMMVB_ENOMEM, "host allocation failed");
    }
    ws->scratch = group;
    ++group->refs;
    const KernelSizes ks = kernel_sizes(K, D);
    const WorkspaceShape shape = make_shape(K, D, x_dtype, max_rows, prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256,
                                            WorkspaceOptions::read(std::getenv), ks);
    static_cast<WorkspaceShape&>(*ws) = shape;
    if (!first) group->npad = shape.npad;
    ws->buffers = buffer_plan(shape, ks, group->npad);      // (not inside somebody's timed iteration: lists and records too)
    HipAllocator hip;
    if (const BufferSpec* failed = allocate_all(ws->buffers, Slots(ws).at, group, hip, &ws->bytes)) {
        gmmvb_workspace_destroy(ws);
        return fail(failed->code, failed->what, hip.err);
    }
    e = init_workspace(ws);
    if (e != hipSuccess) {
        gmmvb_workspace_destroy(ws);
        return fail(GMMVB_EHIP, "workspace initialisation", e);
    }
    *out = ws;
    return GMMVB_OK;
}

int gmmvb_workspace_create(int K, int D, int x_dtype, int64_t max_rows, gmmvb_workspace** out) {
    return create_workspace(K, D, x_dtype, max_rows, nullptr, out);
}

int gmmvb_workspace_create_tile(gmmvb_workspace* first, int64_t max_rows, gmmvb_workspace** out) {
    if (!out) return fail(GMMVB_EINVAL, "out is null");
    *out = nullptr;
    if (!first || !first->scratch) return fail(GMMVB_EINVAL, "null argument");
    if (first->generic || first->hmm != nullptr)
        return fail(GMMVB_EUNSUPPORTED, "tile groups: mixture workspaces with c_degree <= 256 only (the HMM's time axis does not tile)");
    if (max_rows < 1 || max_rows > first->max_rows)
        return fail(GMMVB_EINVAL, "a further tile must not be larger than the group's first workspace");
    return create_workspace(first->K, first->D, first->x_dtype, max_rows, first, out);
}

int gmmvb_workspace_destroy(gmmvb_workspace* ws) {
    if (!ws) return GMMVB_OK;
    gmmvb_scratch* group = ws->scratch;
    if (group && group->owner == ws) group->owner = nullptr;
    HipAllocator hip;
    if (free_all(ws->buffers, Slots(ws).at, group, hip)) delete group;
    if (ws->pol_host) (void)hipHostFree(ws->pol_host);      // (gmmvb_set_shard)
    auto drop = [](hipEvent_t e) {
        if (e) (void)hipEventDestroy(e);
    };
    drop(ws->pol_ev);
    drop(ws->ctr_ev);
    for (hipEvent_t e : ws->ev) drop(e);
    for (hipEvent_t e : ws->span_ev) drop(e);
    for (hipEvent_t e : ws->cal_ev) drop(e);
    if (ws->hmm) hmm_state_destroy(ws->hmm);
    delete ws;
    return GMMVB_OK;
}

int64_t gmmvb_workspace_bytes(const gmmvb_workspace* ws) { return ws ? ws->bytes : -1; }

const char* gmmvb_last_launch_info(const gmmvb_workspace* ws) { return ws ? ws->info : ""; }

int gmmvb_pass_counts(const gmmvb_workspace* ws, int64_t* out /*[8]*/) {
    if (!ws || !out) return fail(GMMVB_EINVAL, "null argument");
    for (int i = 0; i < 8; ++i) out[i] = ws->passes[i];
    return GMMVB_OK;
}

int gmmvb_profile_enable(gmmvb_workspace* ws, int on) {
    if (!ws) return fail(GMMVB_EINVAL, "null argument");
    if (on && !ws->ev[0]) {
        for (auto& e : ws->ev) {
            hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return fail(GMMVB_EHIP, "hipEventCreate", rc);
        }
        for (auto& e : ws->span_ev) {
            hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return fail(GMMVB_EHIP, "hipEventCreate", rc);
        }
    }
    ws->prof = on != 0;
    ws->prof_light = on == 2;
    ws->span_open = false;
    ws->ev_e = ws->ev_m = false;
    ws->n_spans = 0;
    return GMMVB_OK;
}

const char* gmmvb_profile_span_name(int slot) { return (slot >= 0 && slot < kSpanSlots) ? kSpanNames[slot] : ""; }

int gmmvb_profile_spans(gmmvb_workspace* ws, float* ms /*[8]*/, int* launches /*[8]*/) {
    if (!ws || !ms || !launches) return fail(GMMVB_EINVAL, "null argument");
    for (int i = 0; i < kSpanSlots; ++i) {
        ms[i] = 0.0f;
        launches[i] = 0;
    }
    for (int i = 0; i < ws->n_spans; ++i) {
        float t = 0.0f;
        hipError_t rc = hipEventSynchronize(ws->span_ev[2 * i + 1]);
        if (rc == hipSuccess) rc = hipEventElapsedTime(&t, ws->span_ev[2 * i], ws->span_ev[2 * i + 1]);
        if (rc != hipSuccess) return fail(GMMVB_EHIP, "event timing (span)", rc);
        ms[ws->span_slot[i]] += t;
        ++launches[ws->span_slot[i]];
    }
    return GMMVB_OK;
}

int gmmvb_profile_last_ms(gmmvb_workspace* ws, float* estep_ms, float* mstep_ms) {
    if (!ws || !estep_ms || !mstep_ms) return fail(GMMVB_EINVAL, "null argument");
    *estep_ms = *mstep_ms = -1.0f;
    if (ws->ev_e) {
        hipError_t rc = hipEventSynchronize(ws->ev[1]);
        if (rc == hipSuccess) rc = hipEventElapsedTime(estep_ms, ws->ev[0], ws->ev[1]);
        if (rc != hipSuccess) return fail(GMMVB_EHIP, "event timing (estep)", rc);
    }
    if (ws->ev_m) {
        hipError_t rc = hipEventSynchronize(ws->ev[3]);
        if (rc == hipSuccess) rc = hipEventElapsedTime(mstep_ms, ws->ev[2], ws->ev[3]);
        if (rc != hipSuccess) return fail(GMMVB_EHIP, "event timing (mstep)", rc);
    }
    return GMMVB_OK;
}

int gmmvb_set_pivot(gmmvb_workspace* ws, const double* pivot_dev, void* stream) {
    if (!ws || !pivot_dev) return fail(GMMVB_EINVAL, "null argument");
    hipError_t e = hipMemcpyAsync(ws->pivot, pivot_dev, (size_t)ws->D * sizeof(double), hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "hipMemcpyAsync(pivot)", e);
    ws->xc_src = nullptr;      // the centred copy (if any) is stale now
    ws->xq_src = nullptr;      // ... and so are the digit planes
    ++ws->pivot_gen;
    drop_settled_rows(ws);
    return GMMVB_OK;
}

int gmmvb_wants_drift(const gmmvb_workspace* ws, int64_t n_rows) {
    if (!ws || ws->prune == 0 || ws->estep_variant != kEstepLds8 || ws->hmm != nullptr || !ws->rec_k) return 0;
    if (ws->opt_carry_off) return 0;
    if (ws->sharded) n_rows = ws->shard_rows / ws->shard_ranks;        // the same answer on every rank
    return (ws->prune == 2 || n_rows * (int64_t)ws->K >= (int64_t(1) << 23)) ? 1 : 0;
}

namespace {
// drift[0..K) = gamma, [K..2K) = delta, [2K..3K) = c of the parameters the records belong to, [3K..4K) = Gamma - one launch
// instead of four device-to-device copies (each a dispatch of its own on the iteration's critical path)
__global__ void set_drift_kernel(const double* __restrict__ gamma, const double* __restrict__ delta, const double* __restrict__ big_gamma,
                                 const double* __restrict__ cvec, int K, double* __restrict__ drift) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    drift[k] = gamma[k];
    drift[K + k] = delta[k];
    drift[2 * K + k] = cvec[k];
    drift[3 * K + k] = big_gamma[k];
}
}  // namespace

int gmmvb_set_drift(gmmvb_workspace* ws, const double* gamma_dev, const double* delta_dev, const double* big_gamma_dev,
                    double typical_gamma, void* stream) {
    if (!ws || !gamma_dev || !delta_dev || !big_gamma_dev) return fail(GMMVB_EINVAL, "null argument");
    ws->typical_gamma = typical_gamma;
    hipStream_t st = (hipStream_t)stream;
    // (with the constants of the parameters the records belong to: the next gmmvb_set_params overwrites cvec)
    hipLaunchKernelGGL(set_drift_kernel, dim3((unsigned)((ws->K + 255) / 256)), dim3(256), 0, st, gamma_dev, delta_dev, big_gamma_dev,
                       ws->cvec, ws->K, ws->drift);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GMMVB_EHIP, "set_drift_kernel", e);
    ws->have_drift = ws->have_params && ws->params_used;     // else: not the parameters the records belong to
    return GMMVB_OK;
}

// test / diagnostic read-out of one row's candidate record (blocking): out[0..7] slot components (-1 empty), out[8..15]
// slot distances, out[16] B, out[17] exact bits, out[18] selected bits, out[19] flags, out[20] khat, out[21] lse,
// out[22..25] the row's mask words
int gmmvb_debug_record(gmmvb_workspace* ws, int64_t row, double* out /*[26] host*/) {
    if (!ws || !out || !ws->rec_k || row < 0 || row >= ws->npad) return fail(GMMVB_EINVAL, "bad argument");
    hipError_t e = hipDeviceSynchronize();
    auto get = [&e](void* dst, const void* src, size_t n) {
        if (e == hipSuccess) e = hipMemcpy(dst, src, n, hipMemcpyDeviceToHost);
    };
    for (int j = 0; j < kRecSlots; ++j) {
        unsigned short k = 0;
        float d = 0.0f;
        get(&k, ws->rec_k + (int64_t)j * ws->npad + row, sizeof(k));
        get(&d, ws->rec_d + (int64_t)j * ws->npad + row, sizeof(d));
        out[j] = k == kRecEmpty ? -1.0 : (double)k;
        out[8 + j] = d;
    }
    float B = 0.0f;
    unsigned char ex = 0, sel = 0, fl = 0;
    int kh = 0;
    get(&B, ws->rec_B + row, sizeof(B));
    get(&ex, ws->rec_exact + row, 1);
    get(&sel, ws->rec_sel + row, 1);
    get(&fl, ws->rec_flags + row, 1);
    get(&kh, ws->khat + row, sizeof(kh));
    get(out + 21, ws->lse + row, sizeof(double));
    out[16] = B;
    out[17] = ex;
    out[18] = sel;
    out[19] = fl;
    out[20] = kh;
    for (int w = 0; w < 4; ++w) {
        unsigned long long m = 0;
        if (w < (ws->K + 63) / 64) get(&m, ws->masks + (int64_t)w * ws->npad + row, sizeof(m));
        out[22 + w] = (double)m;
    }
    if (e != hipSuccess) return fail(GMMVB_EHIP, "reading a record back", e);
    return GMMVB_OK;
}

int64_t gmmvb_regroup_count(const gmmvb_workspace* ws) { return ws ? ws->sorts : -1; }

// test / diagnostic: the proof round's kernel over (row, k) for EVERY row of the prepared matrix
namespace {
__global__ void debug_all_rows_kernel(int* __restrict__ list, int* __restrict__ counts, int K, int k, int64_t n_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) list[i] = (int)i;
    if (i < K) counts[i] = (int)(i == k ? n_rows : 0);
}
}  // namespace

int gmmvb_debug_proof(gmmvb_workspace* ws, int k, int64_t n_rows, float* ub_dev, double* lb_dev, void* stream) {
    if (!ws || !ub_dev || !lb_dev || k < 0 || k >= ws->K) return fail(GMMVB_EINVAL, "bad argument");
    if (!ws->xq || !ws->img_i8b || ws->xq_src == nullptr || ws->xq_rows != n_rows || ws->xq_gen != ws->img_gen || !ws->have_params)
        return fail(GMMVB_ESTATE, "no digit planes for these rows: gmmvb_set_pivot, gmmvb_prepare_rows, gmmvb_set_params first");
    claim_scratch(ws);
    hipStream_t st = (hipStream_t)stream;
    ws->tmeta_valid = false;                                       // (the bound array is written behind the sweeps' back)
    drop_settled_rows(ws);
    const unsigned grid = (unsigned)((std::max<int64_t>(n_rows, ws->K) + 255) / 256);
    hipLaunchKernelGGL(debug_all_rows_kernel, dim3(grid), dim3(256), 0, st, ws->lists + (int64_t)k * ws->npad, ws->counts, ws->K, k,
                       n_rows);
    hipLaunchKernelGGL(gather_plan_kernel, dim3(1), dim3(64), 0, st, ws->counts, ws->K, estep_i8_pairs_per_chunk(), ws->plan);
    hipError_t e = launch_estep_i8_proof(ws->D, ws->num_cu, st, ws->xq, ws->xqe, ws->img_i8b, ws->cvec, ws->K, ws->lists, ws->npad,
                                         ws->counts, ws->plan, ws->ub32, ws->lnrho, ws->npad);
    if (e == hipSuccess) e = hipMemcpyAsync(ub_dev, ws->ub32 + (int64_t)k * ws->npad, (size_t)n_rows * sizeof(float),
                                            hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(lb_dev, ws->lnrho + (int64_t)k * ws->npad, (size_t)n_rows * sizeof(double),
                                            hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "proof kernel (diagnostic)", e);
    // whatever the workspace held of an E-step is gone
    ws->e_state = 0;
    ws->lost_estep = false;
    ws->bounds_rows = 0;
    ws->rec_valid = ws->dense_valid = ws->rec_live = false;
    ws->active_lists = ws->blk_fresh = false;
    ws->lag.valid = false;
    return GMMVB_OK;
}

int gmmvb_forget(gmmvb_workspace* ws) {
    if (!ws) return fail(GMMVB_EINVAL, "null argument");
    ws->forget = true;
    ws->have_drift = false;
    drop_settled_rows(ws);
    return GMMVB_OK;
}

int gmmvb_set_params(gmmvb_workspace* ws, const double* c_dev, const double* m_dev, const double* u_dev,
                     void* stream) {
    if (!ws || !c_dev || !m_dev || !u_dev) return fail(GMMVB_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (ws->generic) {
        e = hipMemcpyAsync(ws->cvec, c_dev, (size_t)ws->K * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "hipMemcpyAsync(c)", e);
        e = hipMemcpyAsync(ws->gen_m, m_dev, (size_t)ws->K * ws->D * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(ws->gen_u, u_dev, (size_t)ws->K * ws->D * ws->D * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "hipMemcpyAsync(m, u)", e);
        ws->have_params = true;
        ws->params_used = false;
        return GMMVB_OK;
    }
    // (c and the int8 images' pivot ride along: the digits are taken about the pivot in force now; the int8 kernels read that
    // copy, not ws->pivot)
    if (ws->wide) {
        // 128 < D <= 256: a component's triangle does not fit in LDS, and there are no int8 images at that width
        if (ws->pivot_i8) return fail(GMMVB_EUNSUPPORTED, "gmmvb_set_params: int8 images past D = 128");
        hipLaunchKernelGGL(pack_params_kernel, dim3(ws->K), dim3(256), 0, st, u_dev, m_dev, ws->K, ws->D, ws->T, ws->img_len, ws->img,
                           c_dev, ws->cvec, nullptr, nullptr);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(GMMVB_EHIP, "pack_params_kernel", e);
    } else {
        // one launch: the f64 image and every int8 image the workspace has (pack_images_kernel)
        e = launch_pack_images(u_dev, m_dev, c_dev, ws->pivot, ws->K, ws->D, ws->T, ws->img_len, ws->img, ws->cvec, ws->pivot_i8,
                               ws->pivot_i8 ? ws->img_i8 : nullptr, ws->pivot_i8 ? ws->img_i8b : nullptr, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "pack_images_kernel", e);
        if (ws->pivot_i8) ws->img_gen = ws->pivot_gen;
    }
    if (ws->tri) {
        e = launch_pack_tri16(u_dev, m_dev, ws->K, ws->D, ws->tri, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "pack_tri16_kernel", e);
    }
    // The stateless sweep's table for these parameters (project.h), when a sweep can follow: regrouped rows, their tiles'
    // references, digit planes about the pivot in force, and a drift hint (the settled rows' own bound is still carried).
    ws->proj_table = false;
    if (ws->gimg && ws->opt_project != 0 && ws->sorted && ws->tile_ref_valid && ws->have_drift && ws->xq_gen == ws->pivot_gen &&
        !ws->opt_carry_off) {
        e = launch_proj_table(u_dev, m_dev, c_dev, ws->pivot, ws->K, ws->D, ws->gimg, ws->gconst, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "proj_table_kernel", e);
        ws->proj_table = true;
    }
    ws->have_params = true;
    ws->params_used = false;
    return GMMVB_OK;
}

// Counters of the last E-step, blocking: waits for the copy that the E-step enqueued (gmmvb_last_sparsity, and the
// M-step right after a dense E-step, where the host has been waiting for the dense kernel anyway).
int fetch_counters(gmmvb_workspace* ws) {
    if (ws->ctr_pending) {
        hipError_t e = hipEventSynchronize(ws->ctr_ev);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "waiting for the E-step counters", e);
        ws->lag.act = ws->ctr_host[0];
        if (ws->pend_mode == 0) {              // dense pass: every pair evaluated, no records involved
            ws->lag.eval = (double)ws->pend_rows * ws->K;
            ws->lag.over = 0.0;
            ws->lag.settled = 0.0;
            ws->lag.listed = ws->lag.accum = ws->lag.act;
            ws->lag.exits = 0.0;
            ws->lag.cols = -1.0;
            ws->lag.left = -1.0;
            ws->lag_quiet = ws->lag_skipped = -1.0;
            ws->lag.proof = 0.0;
            ws->lag.moved = 0.0;
        } else {
            ws->lag.proof = ws->ctr_host[7];
            ws->lag.exits = (ws->exit_host && ws->gather_exit) ? (double)ws->exit_host[0] : 0.0;
            ws->lag.cols = (ws->exit_host && ws->pend_lazy) ? (double)ws->exit_host[1] : -1.0;
            ws->lag.left = (ws->exit_host && ws->pend_proj) ? (double)ws->exit_host[2] : -1.0;
            ws->lag_quiet = (ws->exit_host && ws->pend_quiet) ? (double)(ws->exit_host[3] & 0xFFFFFFFFull) : -1.0;
            ws->lag_skipped = (ws->exit_host && ws->pend_quiet) ? (double)(ws->exit_host[3] >> 32) : -1.0;
            ws->lag.settled = ws->ctr_host[4];
            ws->lag.listed = ws->ctr_host[5];
            ws->lag.accum = ws->ctr_host[6];                               // a bound pass / sweep also evaluated every row's (previous) best component
            ws->lag.eval = ws->ctr_host[1] + ((ws->pend_mode == 1 || ws->pend_mode == 3) ? ws->pend_round0 : 0.0);
            ws->lag.over = ws->ctr_host[2];
            // rows whose best component changed: after a regrouping they no longer sit with their component's rows.
            // (the first pass after a regrouping compares with the bound kernel's guess, not with a previous best)
            ws->lag.moved = ws->ctr_host[3];
            if (!ws->sharded && ws->sorted && !ws->pend_first_sorted) ws->moved_since_sort += ws->lag.moved;
        }
        ws->lag.rows = (double)ws->pend_rows;
        ws->lag.mode = ws->pend_mode;
        ws->lag.valid = true;
        ws->ctr_pending = false;
    }
    return GMMVB_OK;
}

// The same without waiting: takes the counters over if their copy has completed (the driver synchronises once per
// VB iteration, so by the next E-step it always has).
void poll_counters(gmmvb_workspace* ws) {
    if (ws->ctr_pending && hipEventQuery(ws->ctr_ev) == hipSuccess) (void)fetch_counters(ws);
}

// ---- row-sharded jobs: one policy for all ranks ------------------------------------------------------------------------
// The choice of pass (dense / bound / sweep / records, regrouping, bound level, settling) is driven by counters of the
// previous pass.  With the rows sharded over ranks each rank would see its own counters and the ranks would drift apart:
// a 40-ms bound pass on one rank while the others sweep in 8 ms stalls everybody at the iteration's all-reduce.  So the
// counters travel with the statistics block: gmmvb_policy_export writes them (GMMVB_POLICY_LEN doubles) where the caller's
// all-reduce picks them up, gmmvb_policy_import hands the sums back, and a sharded workspace (gmmvb_set_shard) decides
// from those sums only - every rank the same way.
namespace {
__global__ void policy_export_kernel(const double* __restrict__ ctr, const unsigned long long* __restrict__ exits, int mode,
                                     double rows, int K, double round0, int counted, int use_exits, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool dense = mode == 0;
    const double act = counted ? ctr[0] : 0.0;
    out[0] = act;
    out[1] = dense ? rows * K : ctr[1] + ((mode == 1 || mode == 3) ? round0 : 0.0);
    out[2] = dense ? 0.0 : ctr[2];
    out[3] = dense ? 0.0 : ctr[3];
    out[4] = dense ? 0.0 : ctr[4];
    out[5] = dense ? act : ctr[5];
    out[6] = dense ? act : ctr[6];
    out[7] = dense ? 0.0 : ctr[7];
    out[8] = (dense || !use_exits || !exits) ? 0.0 : (double)*exits;
    out[9] = rows;
    out[10] = 1.0;                      // ranks
    out[11] = counted ? 1.0 : 0.0;      // ranks whose pass counted its pairs
    out[12] = (double)mode;             // kind of the pass these counters describe (the same on every rank: sum / ranks)
    for (int i = 13; i < GMMVB_POLICY_LEN; ++i) out[i] = 0.0;
}
}  // namespace

int gmmvb_set_shard(gmmvb_workspace* ws, int64_t global_rows, int n_ranks) {
    if (!ws || global_rows < 1 || n_ranks < 1) return fail(GMMVB_EINVAL, "bad argument");
    ws->sharded = n_ranks > 1;
    ws->shard_rows = global_rows;
    ws->shard_ranks = n_ranks;
    ws->pol.valid = false;
    if (ws->sharded && !ws->pol_host) {
        hipError_t e = hipHostMalloc((void**)&ws->pol_host, GMMVB_POLICY_LEN * sizeof(double), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ws->pol_ev, hipEventDisableTiming);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "policy buffers", e);
    }
    return GMMVB_OK;
}

int gmmvb_policy_export(gmmvb_workspace* ws, double* out_dev, void* stream) {
    if (!ws || !out_dev) return fail(GMMVB_EINVAL, "null argument");
    if (ws->e_state != 1) return fail(GMMVB_ESTATE, "no E-step output in the workspace");
    hipLaunchKernelGGL(policy_export_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ws->ctr, ws->exit_ctr, ws->prev_pass,
                       (double)ws->e_rows, ws->K, ws->pend_round0, ws->exp_counted ? 1 : 0, ws->gather_exit ? 1 : 0, out_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GMMVB_EHIP, "policy export", e);
    return GMMVB_OK;
}

int gmmvb_policy_import(gmmvb_workspace* ws, const double* in_dev, void* stream) {
    if (!ws || !in_dev) return fail(GMMVB_EINVAL, "null argument");
    if (!ws->sharded) return GMMVB_OK;          // a single process decides from its own counters
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(ws->pol_host, in_dev, GMMVB_POLICY_LEN * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(ws->pol_ev, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "policy import", e);
    ws->pol_pending = true;
    ws->pol_mode = ws->prev_pass;
    ws->pol_first_sorted = ws->pend_first_sorted;
    return GMMVB_OK;
}

// The imported counters, waited for: the copy was enqueued before the caller's per-iteration host sync, so this returns
// at once - and every rank must see them (a rank that decided without them would part ways with the others).
int take_policy(gmmvb_workspace* ws) {
    if (!ws->pol_pending) return GMMVB_OK;
    hipError_t e = hipEventSynchronize(ws->pol_ev);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "waiting for the imported counters", e);
    const double* h = ws->pol_host;
    gmmvb_pass_counters& p = ws->pol;
    p.act = h[0];
    p.eval = h[1];
    p.over = h[2];
    p.moved = h[3];
    p.settled = h[4];
    p.listed = h[5];
    p.accum = h[6];
    p.proof = h[7];
    p.exits = h[8];
    p.rows = h[9];
    p.ranks = h[10];
    // the kind of the pass the counters were taken in travels with them: a row-tiled pass imports the same job-wide tail
    // before every tile, when this workspace's last pass is already the previous TILE of the current iteration
    p.mode = h[10] >= 1.0 ? (int)(h[12] / h[10] + 0.5) : ws->pol_mode;
    p.valid = h[10] >= 1.0 && h[11] == h[10];
    if (p.valid && ws->sorted && !ws->pol_first_sorted) ws->moved_since_sort += p.moved;
    ws->pol_pending = false;
    return GMMVB_OK;
}

int gmmvb_last_sparsity(gmmvb_workspace* ws, void* stream, double* active_pairs, double* evaluated_pairs) {
    (void)stream;
    if (!ws || !active_pairs || !evaluated_pairs) return fail(GMMVB_EINVAL, "null argument");
    if (ws->e_state != 1 && !ws->lost_estep) return fail(GMMVB_ESTATE, "no E-step output in the workspace");
    int rc = fetch_counters(ws);
    if (rc) return rc;
    *evaluated_pairs = ws->lag.mode == 0 ? (double)ws->e_rows * ws->K : ws->lag.eval;
    *active_pairs = (ws->sparse && ws->act_rows == ws->e_rows) ? ws->lag.act : -1.0;   // GMMVB_MSTEP_SPARSE=0: not counted
    return GMMVB_OK;
}

int gmmvb_last_work(gmmvb_workspace* ws, double* out) {
    if (!ws || !out) return fail(GMMVB_EINVAL, "null argument");
    if (ws->e_state != 1 && !ws->lost_estep) return fail(GMMVB_ESTATE, "no E-step output in the workspace");
    int rc = fetch_counters(ws);
    if (rc) return rc;
    const bool counted = ws->sparse && ws->act_rows == ws->e_rows;
    out[0] = counted ? ws->lag.act : -1.0;
    out[1] = ws->lag.mode == 0 ? (double)ws->e_rows * ws->K : ws->lag.eval;
    out[2] = counted ? ws->lag.accum : -1.0;
    out[3] = ws->lag.mode == 0 ? 0.0 : ws->lag.settled;
    out[4] = ws->lag.mode == 0 ? 0.0 : ws->lag.exits;
    out[5] = ws->lag.mode == 0 ? 0.0 : ws->lag.proof;
    out[6] = ws->lag.mode == 3 ? ws->lag.cols : -1.0;
    out[7] = ws->lag.mode == 3 ? ws->lag.left : -1.0;
    return GMMVB_OK;
}

int gmmvb_policy_calibrate(gmmvb_workspace* ws, int on) {
    if (!ws) return fail(GMMVB_EINVAL, "null argument");
    ws->opt_calibrate = on != 0;
    if (!on) {                        // back to the scaled literals
        ws->pt.init(ws->T, estep_bound_blocks(ws->T) ? (ws->D + 31) / 32 : 0);
        for (double& p : ws->cal_pairs) p = 0.0;
    }
    return GMMVB_OK;
}

int gmmvb_policy_table(gmmvb_workspace* ws, double* out /*[GMMVB_POLICY_TABLE_LEN], host*/) {
    if (!ws || !out) return fail(GMMVB_EINVAL, "null argument");
    cal_poll(ws);
    const gmmvb::PolicyTable& t = ws->pt;
    const double v[GMMVB_POLICY_TABLE_LEN] = {t.dense_e_ns, t.dense_m_ns, t.bound_ns, t.exact_ns, t.proof_ns, t.list_m_ns,
                                              t.lit_dense_e, t.lit_dense_m, t.lit_bound, t.prune_below(), t.dense_again_above(),
                                              t.list_m_below(), (double)(t.measured & 7), (double)((t.measured >> 3) & 7),
                                              ws->opt_calibrate ? 1.0 : 0.0, 0.0};
    for (int i = 0; i < GMMVB_POLICY_TABLE_LEN; ++i) out[i] = v[i];
    return GMMVB_OK;
}

int check_x(const gmmvb_workspace* ws, const void* x_dev, int64_t ldx, int64_t n_rows, bool* vec) {
    if (!ws || !x_dev) return fail(GMMVB_EINVAL, "null argument");
    if (n_rows < 1 || n_rows > ws->max_rows) return fail(GMMVB_EINVAL, "n_rows must be in [1, max_rows]");
    if (ldx < ws->D) return fail(GMMVB_EINVAL, "ldx must be >= D");
    const int64_t esz = ws->x_dtype == GMMVB_F64 ? 8 : 4;
    // vector loads: whole 16-feature blocks, 4-element (E) and T-element (M) vectors naturally aligned
    const int64_t valign = esz * (ws->T > 4 ? ws->T : 4);
    *vec = (ws->D % 16 == 0) && ((uintptr_t)x_dev % valign == 0) && ((ldx * esz) % valign == 0);
    return GMMVB_OK;
}

int gmmvb_prepare_rows(gmmvb_workspace* ws, const void* x_dev, int64_t ldx, int64_t n_rows, void* stream) {
    bool vec = false;
    int rc = check_x(ws, x_dev, ldx, n_rows, &vec);
    if (rc) return rc;
    claim_scratch(ws);                 // (the centred copy is written below)
    ws->bounds_rows = 0;               // (new) sample matrix: nothing of an earlier E-step may be carried over
    drop_settled_rows(ws);
    ws->sorted = false;                // ... and the internal row order is the caller's again
    ws->tile_ref_valid = false;
    ws->rec_valid = false;
    ws->dense_valid = false;
    ws->lag.valid = false;
    if (!ws->xc) return GMMVB_OK;      // disabled: the M-step reads x directly
    const int Dp = 16 * ws->T;
    const int64_t pad_rows = round_up(n_rows, 64) + 64;
    const int64_t total = pad_rows * Dp;
    const unsigned grid = (unsigned)((total + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (ws->x_dtype == GMMVB_F64)
        hipLaunchKernelGGL(center_rows_kernel<double>, dim3(grid), dim3(256), 0, st, (const double*)x_dev, ldx, n_rows,
                           pad_rows, ws->D, Dp, ws->pivot, ws->xc);
    else
        hipLaunchKernelGGL(center_rows_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x_dev, ldx, n_rows,
                           pad_rows, ws->D, Dp, ws->pivot, ws->xc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GMMVB_EHIP, "center_rows launch", e);
    ws->xc_src = x_dev;
    ws->xc_rows = n_rows;
    ws->xc_ldx = ldx;
    ws->xc_stale = false;
    if (ws->xq) {              // the int8 digit planes of the proof round, about the same pivot
        e = launch_x_digits(x_dev, ws->x_dtype == GMMVB_F64, ldx, n_rows, ws->D, ws->pivot, ws->xq, ws->xqe, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "x_digits launch", e);
        ws->xq_src = x_dev;
        ws->xq_rows = n_rows;
        ws->xq_ldx = ldx;
        ws->xq_gen = ws->pivot_gen;
    }
    return GMMVB_OK;
}

// The centred copy in the workspace's internal row order (after a regrouping; see regroup_rows)
hipError_t recenter_rows(gmmvb_workspace* ws, int64_t n_rows, hipStream_t st) {
    const int Dp = 16 * ws->T;
    const int64_t pad_rows = round_up(n_rows, 64) + 64;
    const unsigned cg = (unsigned)((pad_rows * Dp + 255) / 256);
    // regrouped rows: the workspace's permuted copy; else (the copy was lost to another tile of the group) the caller's matrix
    const void* src = ws->sorted ? ws->xp : ws->xc_src;
    const int64_t ld = ws->sorted ? (int64_t)ws->D : ws->xc_ldx;
    if (ws->x_dtype == GMMVB_F64)
        hipLaunchKernelGGL(center_rows_kernel<double>, dim3(cg), dim3(256), 0, st, (const double*)src, ld, n_rows,
                           pad_rows, ws->D, Dp, ws->pivot, ws->xc);
    else
        hipLaunchKernelGGL(center_rows_kernel<float>, dim3(cg), dim3(256), 0, st, (const float*)src, ld, n_rows,
                           pad_rows, ws->D, Dp, ws->pivot, ws->xc);
    ws->xc_stale = false;
    return hipGetLastError();
}


}  // extern "C"
