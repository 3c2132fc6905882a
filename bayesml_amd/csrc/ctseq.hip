// include/ctseq.h: argument checks, the layout of the scratch, and the launches of ctseq_kernels.h, one group per level.
#include "../../include/ctseq.h"
#include "ctseq_kernels.h"
#include "ctree_shape.h"

namespace ctseq {
using namespace entry;
using ctree_shape::Shape;           // the pass works on ctree.h's tables: their layout and limit
using ctree_shape::shape_of;
ENTRY_SAME_CODES(CTSEQ);
static thread_local Err g_err = {""};

// The scratch, in 8-byte slots from its start.  int32 arrays take half a slot per entry.
struct Layout {
    int64_t rows;                                       // binary64 [m][k], only with want_rows
    int64_t perm, key;                                  // (D + 1) x int32 [m] each: perm_d and key_d of every level
    int64_t tmp, tkey, segst, ca;                       // int32 [m]
    int64_t q, own, delta, gvis, sumb0, g0s;            // binary64 [m]
    int64_t hist, agg_sum, agg_flag, carry, sym;        // (k+1) x tiles int32; tiles; tiles int32; tiles; uint8 [m+D]
    int64_t total, half_m;
};

static Layout layout_of(int k, int D, int64_t m, bool want_rows) {
    Layout l;
    const int64_t h = (m + 1) / 2, tiles = (m + kTile - 1) / kTile;
    int64_t at = 0;
    auto take = [&at](int64_t slots) { const int64_t here = at; at += slots; return here; };
    l.half_m = h;
    l.rows = take(want_rows ? m * k : 0);               // first, so that the caller can find the rows of the last pass
    l.perm = take(h * (D + 1));
    l.key = take(h * (D + 1));
    l.tmp = take(h);
    l.tkey = take(h);
    l.segst = take(h);
    l.ca = take(h);
    l.q = take(m);
    l.own = take(m);
    l.delta = take(m);
    l.gvis = take(m);
    l.sumb0 = take(m);
    l.g0s = take(m);
    l.hist = take(((int64_t)(k + 1) * tiles + 1) / 2);
    l.agg_sum = take(tiles);
    l.agg_flag = take((tiles + 1) / 2);
    l.carry = take(tiles);
    l.sym = take((m + D + 7) / 8);
    l.total = at;
    return l;
}

static int elem_size(int d) { return d == CTSEQ_U8 ? 1 : d == CTSEQ_I32 ? 4 : 8; }

// Stable partition of src (msrc positions) by the level's digit or by the symbol; `hist` is scratch.
template <bool BY_SYM>
static int partition(hipStream_t st, const int* perm, const uint32_t* key, int msrc, int64_t begin, int d, int k, int D,
                     const uint8_t* sym, int* hist, uint32_t pw_prev, int* operm, uint32_t* okey) {
    const int tiles = (int)grid_of(msrc, kTile);
    hipLaunchKernelGGL((part_hist_kernel<BY_SYM>), dim3(tiles), dim3(kTile), 0, st, perm, msrc, begin, d, k, D, sym, tiles,
                       hist);
    if (int rc = g_err.launched("part_hist_kernel launch")) return rc;
    hipLaunchKernelGGL(scan_int_kernel, dim3(1), dim3(kScanThreads), 0, st, hist, (int64_t)(k + 1) * tiles);
    if (int rc = g_err.launched("scan_int_kernel launch")) return rc;
    hipLaunchKernelGGL((part_scatter_kernel<BY_SYM>), dim3(tiles), dim3(kTile), 0, st, perm, key, msrc, begin, d, k, D, sym,
                       tiles, (const int*)hist, pw_prev, operm, okey);
    return g_err.launched("part_scatter_kernel launch");
}
}  // namespace ctseq

using namespace ctseq;

extern "C" {

int ctseq_abi_version(void) { return CTSEQ_ABI_VERSION; }
const char* ctseq_last_error(void) { return g_err.msg; }

int64_t ctseq_work_len(int k, int D, int64_t m, int want_rows) {
    Shape sh;
    if (shape_of(k, D, &sh) != CTSEQ_OK || m < 1 || m >= ((int64_t)1 << 31)) return -1;
    return layout_of(k, D, m, want_rows != 0).total;
}

int ctseq_pass(int dtype, const void* x_dev, int64_t n, int64_t begin, int64_t m, int k, int D, void* beta_dev, void* g_dev,
               void* exists_dev, void* leaf_dev, double hn_g, const void* hn_beta_dev, void* rows_dev, void* argmax_dev,
               void* nats_dev, void* work_dev, void* stream) {
    Shape sh;
    const int src = shape_of(k, D, &sh);
    if (src == CTSEQ_EINVAL) return g_err.fail(src, "ctseq_pass: k and D must be >= 1");
    if (src == CTSEQ_EUNSUPPORTED)
        return g_err.fail(src, "ctseq_pass: k > %d or k^(D+1) > %d is not supported", CTREE_MAX_K, CTREE_MAX_SLOTS);
    if (dtype < CTSEQ_U8 || dtype > CTSEQ_I64)
        return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: dtype must be CTSEQ_U8, CTSEQ_I32 or CTSEQ_I64");
    if (n < 1 || m < 1 || begin < 0) return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: n and m must be >= 1 and begin >= 0");
    if (m >= ((int64_t)1 << 31)) return g_err.fail(CTSEQ_EUNSUPPORTED, "ctseq_pass: m must be below 2^31");
    if (begin > n - m) return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: begin + m must not exceed n");
    if (!x_dev || !beta_dev || !g_dev || !exists_dev || !leaf_dev || !hn_beta_dev || !work_dev)
        return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: null pointer");
    if (!(hn_g >= 0.0 && hn_g <= 1.0)) return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: hn_g must be in [0, 1]");
    if (misaligned(x_dev, elem_size(dtype)))
        return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: x_dev must be aligned to its element size");
    if (any_misaligned(8, beta_dev, g_dev, hn_beta_dev, rows_dev, argmax_dev, nats_dev, work_dev))
        return g_err.fail(CTSEQ_EINVAL, "ctseq_pass: misaligned pointer");

    hipStream_t st = (hipStream_t)stream;
    const bool rows_wanted = rows_dev || argmax_dev;
    const Layout lay = layout_of(k, D, m, rows_wanted && !rows_dev);
    int64_t* w = (int64_t*)work_dev;
    const int mi = (int)m;
    auto perm_of = [&](int d) { return (int*)(w + lay.perm + lay.half_m * d); };
    auto key_of = [&](int d) { return (uint32_t*)(w + lay.key + lay.half_m * d); };
    int* tmp = (int*)(w + lay.tmp);
    uint32_t* tkey = (uint32_t*)(w + lay.tkey);
    int* segst = (int*)(w + lay.segst);
    int* ca = (int*)(w + lay.ca);
    double *q = (double*)(w + lay.q), *own = (double*)(w + lay.own), *delta = (double*)(w + lay.delta);
    double *gvis = (double*)(w + lay.gvis), *sumb0 = (double*)(w + lay.sumb0), *g0s = (double*)(w + lay.g0s);
    int* hist = (int*)(w + lay.hist);
    double *agg_sum = (double*)(w + lay.agg_sum), *carry = (double*)(w + lay.carry);
    int* agg_flag = (int*)(w + lay.agg_flag);
    uint8_t* sym = (uint8_t*)(w + lay.sym);
    double* rows = rows_dev ? (double*)rows_dev : (double*)(w + lay.rows);
    double* beta = (double*)beta_dev;
    double* g = (double*)g_dev;
    uint8_t *ex = (uint8_t*)exists_dev, *leaf = (uint8_t*)leaf_dev;
    const double* hb = (const double*)hn_beta_dev;

    // positions of the chunk that reach level d: those with begin + il >= d
    auto reach = [&](int d) {
        const int64_t cut = d - begin;
        return (int)(m - (cut < 0 ? 0 : cut > m ? m : cut));
    };

    const int64_t len = m + D;
    if (dtype == CTSEQ_U8)
        hipLaunchKernelGGL((load_symbols_kernel<uint8_t>), dim3(grid_of(len, kTile)), dim3(kTile), 0, st, (const uint8_t*)x_dev,
                           n, begin, len, k, D, sym);
    else if (dtype == CTSEQ_I32)
        hipLaunchKernelGGL((load_symbols_kernel<int32_t>), dim3(grid_of(len, kTile)), dim3(kTile), 0, st, (const int32_t*)x_dev,
                           n, begin, len, k, D, sym);
    else
        hipLaunchKernelGGL((load_symbols_kernel<int64_t>), dim3(grid_of(len, kTile)), dim3(kTile), 0, st, (const int64_t*)x_dev,
                           n, begin, len, k, D, sym);
    if (int rc = g_err.launched("load_symbols_kernel launch")) return rc;

    // the order of every level, top-down
    hipLaunchKernelGGL(init_level0_kernel, dim3(grid_of(m, kTile)), dim3(kTile), 0, st, mi, perm_of(0), key_of(0));
    if (int rc = g_err.launched("init_level0_kernel launch")) return rc;
    int deepest = 0;
    for (int d = 1; d <= D && reach(d) > 0; ++d) {
        if (int rc = partition<false>(st, perm_of(d - 1), key_of(d - 1), reach(d - 1), begin, d, k, D, sym, hist,
                                      (uint32_t)sh.pw[d - 1], perm_of(d), key_of(d)))
            return rc;
        deepest = d;
    }

    // predictions and updates, bottom-up
    for (int d = deepest; d >= 0; --d) {
        const int md = reach(d);
        const unsigned tiles = grid_of(md, kTile);
        const int* perm = perm_of(d);
        const uint32_t* key = key_of(d);
        const uint32_t pw = (uint32_t)sh.pw[d];
        double* beta_l = beta + sh.off[d] * k;
        double* g_l = g + sh.off[d];
        uint8_t *ex_l = ex + sh.off[d], *leaf_l = leaf + sh.off[d];

        if (int rc = partition<true>(st, perm, key, md, begin, d, k, D, sym, hist, 0u, tmp, tkey)) return rc;
        hipLaunchKernelGGL(seg_head_kernel, dim3(tiles), dim3(kTile), 0, st, key, md, d, k, D, pw, (const double*)beta_l,
                           (const double*)g_l, (const uint8_t*)ex_l, hn_g, hb, segst, sumb0, g0s);
        if (int rc = g_err.launched("seg_head_kernel launch")) return rc;
        hipLaunchKernelGGL(sym_rank_kernel, dim3(tiles), dim3(kTile), 0, st, (const int*)tmp, (const uint32_t*)tkey, md, ca);
        if (int rc = g_err.launched("sym_rank_kernel launch")) return rc;
        hipLaunchKernelGGL(own_delta_kernel, dim3(tiles), dim3(kTile), 0, st, perm, key, (const int*)segst, (const int*)ca,
                           (const double*)sumb0, md, begin, d, k, D, pw, (const uint8_t*)sym, (const double*)beta_l,
                           (const uint8_t*)ex_l, hb, (const double*)q, own, delta, agg_sum, agg_flag);
        if (int rc = g_err.launched("own_delta_kernel launch")) return rc;
        hipLaunchKernelGGL(carry_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const double*)agg_sum, (const int*)agg_flag,
                           (int)tiles, carry);
        if (int rc = g_err.launched("carry_scan_kernel launch")) return rc;
        hipLaunchKernelGGL(mix_kernel, dim3(tiles), dim3(kTile), 0, st, perm, key, (const int*)segst, (const double*)g0s,
                           (const double*)own, (const double*)delta, (const double*)carry, md, begin, d, D, pw, g_l, q, gvis);
        if (int rc = g_err.launched("mix_kernel launch")) return rc;
        if (rows_wanted) {
            int W = 64;
            while (W / 2 >= k) W /= 2;
            const int64_t threads = (int64_t)grid_of(md, kRowBlock) * W;
            hipLaunchKernelGGL(rows_level_kernel, dim3(grid_of(threads, kTile)), dim3(kTile), 0, st, perm, key,
                               (const int*)segst, (const double*)sumb0, (const double*)gvis, (const int*)tmp,
                               (const uint32_t*)tkey, md, begin, d, k, D, pw, (const uint8_t*)sym, (const double*)beta_l,
                               (const uint8_t*)ex_l, hb, W, rows);
            if (int rc = g_err.launched("rows_level_kernel launch")) return rc;
        }
        hipLaunchKernelGGL(create_nodes_kernel, dim3(tiles), dim3(kTile), 0, st, key, (const int*)segst, md, d, k, D, pw,
                           beta_l, ex_l, leaf_l, hb);
        if (int rc = g_err.launched("create_nodes_kernel launch")) return rc;
        hipLaunchKernelGGL(add_counts_kernel, dim3(tiles), dim3(kTile), 0, st, (const uint32_t*)tkey, md, k, pw, beta_l);
        if (int rc = g_err.launched("add_counts_kernel launch")) return rc;
    }

    if (nats_dev) {
        hipLaunchKernelGGL(nats_kernel, dim3(grid_of(m, kTile)), dim3(kTile), 0, st, (const double*)q, mi, (double*)nats_dev);
        if (int rc = g_err.launched("nats_kernel launch")) return rc;
    }
    if (argmax_dev) {
        hipLaunchKernelGGL(argmax_kernel, dim3(grid_of(m, kTile)), dim3(kTile), 0, st, (const double*)rows, mi, k,
                           (int64_t*)argmax_dev);
        if (int rc = g_err.launched("argmax_kernel launch")) return rc;
    }
    return CTSEQ_OK;
}

}  // extern "C"
