// include/ctfit.h: argument checks, the layout of the two scratch buffers, and the launches of ctfit_kernels.h.
#include "../../include/ctfit.h"
#include "ctfit_kernels.h"
#include "ctree_shape.h"

namespace ctfit {
using namespace entry;
using namespace ctree_shape;
ENTRY_SAME_CODES(CTFIT);
static_assert(CTFIT_TILE == kTile && CTFIT_SEQ_STAGE == kSeqStage && CTFIT_SERIAL_RUN == kSerialRun,
              "ctfit.h and ctfit_kernels.h disagree");
static thread_local Err g_err = {""};

static int check_shape(const char* who, int k, int D, Shape* sh) {
    const int rc = shape_of(k, D, sh);
    if (rc == CTFIT_EINVAL) return g_err.fail(rc, "%s: k and D must be >= 1", who);
    if (rc == CTFIT_EUNSUPPORTED)
        return g_err.fail(rc, "%s: k > %d or k^(D+1) > %d is not supported", who, CTREE_MAX_K, CTREE_MAX_SLOTS);
    return CTFIT_OK;
}

static bool lds_path(const Shape& sh) { return sh.bins <= CTREE_LDS_BINS; }

// work: [ count slabs | lnW, all levels | counts of levels 0..D-1 | head counts of levels 0..D-1 | has-heads flags | lead ]
struct Work {
    int64_t* slabs;
    double* lnw;
    int64_t* cl;
    u64* hcnt;
    uint8_t* flag;
    double* lead;
    int64_t len, zero_len;            // 8-byte slots in all; of them hcnt and flag, which ctfit_count zeroes
};
static Work work_of(const Shape& sh, int k, void* work) {
    Work w;
    int64_t at = 0;
    int64_t* base = (int64_t*)work;
    w.slabs = base + at, at += (int64_t)ctree::kMaxSlabs * (lds_path(sh) ? 1 + sh.bins : 1);
    w.lnw = (double*)(base + at), at += sh.nodes;
    w.cl = base + at, at += sh.upper * k;
    w.hcnt = (u64*)(base + at), at += sh.upper * k;
    w.flag = (uint8_t*)(base + at), at += (sh.upper + 7) / 8;
    w.zero_len = sh.upper * k + (sh.upper + 7) / 8;
    w.lead = (double*)(base + at), at += sh.upper;
    w.len = at;
    return w;
}

// head: [ buckets, then their scan: 2H | long runs: count, nodes | tile sums of the scan ]
struct Head {
    u64 *scan, *long_list, *tile_sum;
    int64_t long_cap, tiles, len;
};
static Head head_of(int64_t H, void* head) {
    Head h;
    u64* base = (u64*)head;
    h.scan = base;
    h.long_list = base + 2 * H;
    h.long_cap = H / kSerialRun + 1;
    h.tile_sum = h.long_list + 1 + h.long_cap;
    h.tiles = (2 * H + kScanTile - 1) / kScanTile;
    h.len = 2 * H + 1 + h.long_cap + h.tiles;
    return h;
}

static Offsets offsets_of(const Shape& sh, int D) {
    Offsets lv;
    for (int d = 0; d <= kMaxD + 1; ++d) lv.off[d] = sh.off[d <= D ? d : D];
    return lv;
}

static int elem_size(int d) { return d == CTFIT_U8 ? 1 : d == CTFIT_I32 ? 4 : 8; }

// What ctfit_count and ctfit_rank check alike.
static int check_sample(const char* who, int dtype, const void* x, int64_t n, const void* seq_off, const void* hoff, int64_t S,
                        int64_t H) {
    if (dtype < CTFIT_U8 || dtype > CTFIT_I64) return g_err.fail(CTFIT_EINVAL, "%s: dtype must be CTFIT_U8, CTFIT_I32 or CTFIT_I64", who);
    if (n < 1 || S < 1 || H < 1) return g_err.fail(CTFIT_EINVAL, "%s: n, S and H must be >= 1", who);
    if (n >= ((int64_t)1 << 31) || S >= ((int64_t)1 << 31)) return g_err.fail(CTFIT_EUNSUPPORTED, "%s: n and S must be below 2^31", who);
    if (H > n) return g_err.fail(CTFIT_EINVAL, "%s: more heads than positions", who);
    if (!x || !seq_off || !hoff) return g_err.fail(CTFIT_EINVAL, "%s: null pointer", who);
    if (misaligned(x, elem_size(dtype))) return g_err.fail(CTFIT_EINVAL, "%s: x_dev must be aligned to its element size", who);
    if (any_misaligned(8, seq_off, hoff)) return g_err.fail(CTFIT_EINVAL, "%s: misaligned pointer", who);
    return CTFIT_OK;
}

struct Sample {
    const void* x;
    int64_t n;
    const int64_t *seq_off, *hoff;
    int64_t S, H;
    int k, D;
};

template <typename T>
static int launch_count(const Sample& a, const Shape& sh, const Work& w, int64_t* out, u64* keys, hipStream_t st) {
    int64_t span;
    int slabs = slab_span(a.n, ctree::kMaxSlabs, ctree::kMinSpan, &span);
    span = (span + kTile - 1) / kTile * kTile;              // whole tiles, so that every tile but the last is full
    slabs = (int)((a.n + span - 1) / span);
    const Offsets lv = offsets_of(sh, a.D);
    const bool ldsh = lds_path(sh);
    if (ldsh) {
        hipLaunchKernelGGL((count_kernel<T, true>), dim3(slabs), dim3(kThreads), sizeof(u64) * (size_t)sh.bins, st, (const T*)a.x,
                           a.n, span, a.seq_off, a.hoff, a.S, a.H, a.k, a.D, lv, sh.bins, (u64*)nullptr, w.slabs, keys, keys + a.H,
                           w.hcnt, w.flag);
    } else {
        const hipError_t e = hipMemsetAsync(out + 2, 0, sizeof(int64_t) * (size_t)sh.bins, st);
        if (e != hipSuccess) return g_err.hip(CTFIT_EHIP, "ctfit_count: hipMemsetAsync", e);
        hipLaunchKernelGGL((count_kernel<T, false>), dim3(slabs), dim3(kThreads), 0, st, (const T*)a.x, a.n, span, a.seq_off,
                           a.hoff, a.S, a.H, a.k, a.D, lv, sh.bins, (u64*)(out + 2), w.slabs, keys, keys + a.H, w.hcnt, w.flag);
    }
    if (int rc = g_err.launched("ctfit count_kernel launch")) return rc;
    const int64_t slab_len = ldsh ? 1 + sh.bins : 1;
    hipLaunchKernelGGL(ctree::count_combine_kernel, dim3(grid_of(slab_len, kThreads)), dim3(kThreads), 0, st,
                       (const int64_t*)w.slabs, slabs, slab_len, a.n, out);
    return g_err.launched("ctfit count_combine_kernel launch");
}

template <typename T>
static int launch_rank(const Sample& a, const Shape& sh, const Work& w, const u64* keys, u64* bucket, hipStream_t st) {
    hipLaunchKernelGGL((rank_kernel<T>), dim3(grid_of(a.n, kTile)), dim3(kThreads), 0, st, (const T*)a.x, a.n, a.seq_off, a.hoff,
                       a.S, a.H, a.k, a.D, offsets_of(sh, a.D), keys, keys + a.H, (const uint8_t*)w.flag, bucket);
    return g_err.launched("ctfit rank_kernel launch");
}
}  // namespace ctfit

using namespace ctfit;

extern "C" {

int ctfit_abi_version(void) { return CTFIT_ABI_VERSION; }
const char* ctfit_last_error(void) { return g_err.msg; }

int64_t ctfit_work_len(int k, int D) {
    Shape sh;
    if (shape_of(k, D, &sh) != CTFIT_OK) return -1;
    return work_of(sh, k, nullptr).len;
}

int64_t ctfit_head_len(int64_t H) {
    if (H < 1 || H >= ((int64_t)1 << 31)) return -1;
    return head_of(H, nullptr).len;
}

int ctfit_count(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, const void* hoff_dev, int64_t S, int64_t H,
                int k, int D, void* out_dev, void* keys_dev, void* work_dev, void* stream) {
    Shape sh;
    if (int rc = check_shape("ctfit_count", k, D, &sh)) return rc;
    if (int rc = check_sample("ctfit_count", dtype, x_dev, n, seq_off_dev, hoff_dev, S, H)) return rc;
    if (!out_dev || !keys_dev || !work_dev) return g_err.fail(CTFIT_EINVAL, "ctfit_count: null pointer");
    if (any_misaligned(8, out_dev, keys_dev, work_dev)) return g_err.fail(CTFIT_EINVAL, "ctfit_count: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const Work w = work_of(sh, k, work_dev);
    hipError_t e = hipMemsetAsync(w.hcnt, 0, sizeof(int64_t) * (size_t)w.zero_len, st);
    // a slot that no head claims sorts behind every node and matches none
    if (e == hipSuccess) e = hipMemsetAsync(keys_dev, 0x7f, sizeof(u64) * 2 * (size_t)H, st);
    if (e != hipSuccess) return g_err.hip(CTFIT_EHIP, "ctfit_count: hipMemsetAsync", e);
    const Sample a = {x_dev, n, (const int64_t*)seq_off_dev, (const int64_t*)hoff_dev, S, H, k, D};
    int64_t* out = (int64_t*)out_dev;
    u64* keys = (u64*)keys_dev;
    if (dtype == CTFIT_U8) return launch_count<uint8_t>(a, sh, w, out, keys, st);
    if (dtype == CTFIT_I32) return launch_count<int32_t>(a, sh, w, out, keys, st);
    return launch_count<int64_t>(a, sh, w, out, keys, st);
}

int ctfit_rank(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, const void* hoff_dev, int64_t S, int64_t H,
               int k, int D, const void* keys_sorted_dev, const void* beta_dev, const void* exists_dev,
               const void* hn_beta_dev, void* head_dev, void* work_dev, void* stream) {
    Shape sh;
    if (int rc = check_shape("ctfit_rank", k, D, &sh)) return rc;
    if (int rc = check_sample("ctfit_rank", dtype, x_dev, n, seq_off_dev, hoff_dev, S, H)) return rc;
    if (!keys_sorted_dev || !beta_dev || !exists_dev || !hn_beta_dev || !head_dev || !work_dev)
        return g_err.fail(CTFIT_EINVAL, "ctfit_rank: null pointer");
    if (any_misaligned(8, keys_sorted_dev, beta_dev, hn_beta_dev, (const void*)head_dev, (const void*)work_dev))
        return g_err.fail(CTFIT_EINVAL, "ctfit_rank: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const Work w = work_of(sh, k, work_dev);
    const Head h = head_of(H, head_dev);
    const hipError_t e = hipMemsetAsync(h.scan, 0, sizeof(u64) * (2 * (size_t)H + 1), st);      // the buckets and long_list[0]
    if (e != hipSuccess) return g_err.hip(CTFIT_EHIP, "ctfit_rank: hipMemsetAsync", e);
    const Sample a = {x_dev, n, (const int64_t*)seq_off_dev, (const int64_t*)hoff_dev, S, H, k, D};
    const u64* keys = (const u64*)keys_sorted_dev;
    int rc = dtype == CTFIT_U8    ? launch_rank<uint8_t>(a, sh, w, keys, h.scan, st)
             : dtype == CTFIT_I32 ? launch_rank<int32_t>(a, sh, w, keys, h.scan, st)
                                  : launch_rank<int64_t>(a, sh, w, keys, h.scan, st);
    if (rc) return rc;
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)h.tiles), dim3(kThreads), 0, st, (const u64*)h.scan, 2 * H, h.tile_sum);
    if ((rc = g_err.launched("ctfit scan_sums_kernel launch"))) return rc;
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kThreads), 0, st, h.tile_sum, h.tiles);
    if ((rc = g_err.launched("ctfit scan_tiles_kernel launch"))) return rc;
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)h.tiles), dim3(kThreads), 0, st, h.scan, 2 * H, (const u64*)h.tile_sum);
    if ((rc = g_err.launched("ctfit scan_apply_kernel launch"))) return rc;
    const LeadArgs p = {keys, keys + H, h.scan, H, k, (const double*)beta_dev, (const uint8_t*)exists_dev,
                        (const double*)hn_beta_dev};
    hipLaunchKernelGGL(lead_short_kernel, dim3(grid_of(sh.upper, kThreads)), dim3(kThreads), 0, st, p, sh.upper,
                       (const uint8_t*)w.flag, w.lead, h.long_list, h.long_cap);
    if ((rc = g_err.launched("ctfit lead_short_kernel launch"))) return rc;
    const int64_t grid = h.long_cap < kLongGrid ? h.long_cap : kLongGrid;
    hipLaunchKernelGGL(lead_long_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, p, sh.upper, w.lead, (const u64*)h.long_list,
                       h.long_cap);
    return g_err.launched("ctfit lead_long_kernel launch");
}

int ctfit_sweep(int k, int D, const void* cnt_dev, void* beta_dev, void* g_dev, void* exists_dev, double hn_g,
                const void* hn_beta_dev, void* work_dev, void* stream) {
    Shape sh;
    if (int rc = check_shape("ctfit_sweep", k, D, &sh)) return rc;
    if (!cnt_dev || !beta_dev || !g_dev || !exists_dev || !hn_beta_dev || !work_dev)
        return g_err.fail(CTFIT_EINVAL, "ctfit_sweep: null pointer");
    if (!(hn_g >= 0.0 && hn_g <= 1.0)) return g_err.fail(CTFIT_EINVAL, "ctfit_sweep: hn_g must be in [0, 1]");
    if (any_misaligned(8, cnt_dev, (const void*)beta_dev, (const void*)g_dev, hn_beta_dev, (const void*)work_dev))
        return g_err.fail(CTFIT_EINVAL, "ctfit_sweep: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const Work w = work_of(sh, k, work_dev);
    double* beta = (double*)beta_dev;
    double* g = (double*)g_dev;
    uint8_t* ex = (uint8_t*)exists_dev;
    const double* hb = (const double*)hn_beta_dev;
    hipLaunchKernelGGL(ctree::sweep_deepest_kernel, dim3(grid_of(sh.pw[D], kThreads)), dim3(kThreads), 0, st, k, sh.pw[D],
                       (const int64_t*)cnt_dev, beta + sh.off[D] * k, g + sh.off[D], ex + sh.off[D], hb, w.lnw + sh.off[D]);
    if (int rc = g_err.launched("ctfit sweep_deepest_kernel launch")) return rc;
    for (int d = D - 1; d >= 0; --d) {
        const int64_t* child = d + 1 == D ? (const int64_t*)cnt_dev : w.cl + sh.off[d + 1] * k;
        hipLaunchKernelGGL(sweep_level_lead_kernel, dim3(grid_of(sh.pw[d], kThreads)), dim3(kThreads), 0, st, k, sh.pw[d], child,
                           (const int64_t*)w.hcnt + sh.off[d] * k, (const double*)(w.lead + sh.off[d]), w.cl + sh.off[d] * k,
                           (const double*)(w.lnw + sh.off[d + 1]), w.lnw + sh.off[d], beta + sh.off[d] * k, g + sh.off[d],
                           ex + sh.off[d], hn_g, hb);
        if (int rc = g_err.launched("ctfit sweep_level_lead_kernel launch")) return rc;
    }
    return CTFIT_OK;
}

}  // extern "C"
