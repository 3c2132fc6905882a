// include/ctsp.h: argument checks, key widths and capacity planning in plain C++, and the launches of ctsp_kernels.h.
#include "../../include/ctsp.h"
#include "ctsp_kernels.h"
#include "ctree_shape.h"

namespace ctsp {
using namespace entry;
using ctree_shape::slab_span;
using ctree_shape::subtree_pow;
ENTRY_SAME_CODES(CTSP);
static thread_local Err g_err = {""};

static int symbol_bits(int k) {
    int b = 1;
    while ((1 << b) < k) ++b;
    return b;
}

// 0 = fine, CTSP_EINVAL / CTSP_EUNSUPPORTED otherwise (no message set); *b = bits per symbol.
static int shape_of(int k, int D, int* b) {
    if (k < 1 || D < 1) return CTSP_EINVAL;
    if (k > CTSP_MAX_K) return CTSP_EUNSUPPORTED;
    *b = symbol_bits(k);
    if ((int64_t)*b * D > CTSP_MAX_KEY_BITS) return CTSP_EUNSUPPORTED;
    return CTSP_OK;
}

static int check_shape(const char* who, int k, int D, int* b) {
    const int rc = shape_of(k, D, b);
    if (rc == CTSP_EINVAL) return g_err.fail(rc, "%s: k and D must be >= 1", who);
    if (rc == CTSP_EUNSUPPORTED)
        return g_err.fail(rc, "%s: k > %d or ceil(log2 k) * D > %d is not supported", who, CTSP_MAX_K, CTSP_MAX_KEY_BITS);
    return CTSP_OK;
}

// off[0] = 0 and every level's capacity a power of two >= 2, at most 2^30 (the grids of one lane per (slot, symbol))
static int check_offsets(const char* who, const int64_t* off, int D) {
    if (!off) return g_err.fail(CTSP_EINVAL, "%s: null pointer", who);
    if (off[0] != 0) return g_err.fail(CTSP_EINVAL, "%s: off[0] must be 0", who);
    for (int d = 0; d <= D; ++d) {
        const int64_t cap = off[d + 1] - off[d];
        if (cap < 2 || (cap & (cap - 1)) != 0 || cap > ((int64_t)1 << 30))
            return g_err.fail(CTSP_EINVAL, "%s: the capacity of level %d must be a power of two in 2..2^30", who, d);
    }
    return CTSP_OK;
}

// min(n, k^level), without overflow
static int64_t new_nodes_bound(int k, int level, int64_t n) {
    if (k == 1) return n < 1 ? n : 1;
    int64_t p = 1;
    for (int d = 0; d < level; ++d) {
        p *= k;
        if (p >= n) return n;
    }
    return p < n ? p : n;
}

// k^level capped at 2^62
static int64_t level_size(int k, int level) {
    int64_t p = 1;
    for (int d = 0; d < level; ++d) {
        if (p > ((int64_t)1 << 62) / k) return (int64_t)1 << 62;
        p *= k;
    }
    return p;
}

static int elem_size(int d) { return d == CTSP_U8 ? 1 : d == CTSP_I32 ? 4 : 8; }

template <typename T>
static int launch_count(const void* x_dev, int64_t n, int k, int b, int D, const int64_t* off, u64* key, u64* cnt,
                        int64_t* status, hipStream_t st) {
    int64_t span;
    const int S = slab_span(n, kMaxSlabs, kMinSpan, &span);
    hipLaunchKernelGGL((count_kernel<T>), dim3(S), dim3(kThreads), 0, st, (const T*)x_dev, n, span, k, b, D, key + off[D],
                       off[D + 1] - off[D], cnt + off[D] * k, status);
    return g_err.launched("ctsp count_kernel launch");
}
}  // namespace ctsp

using namespace ctsp;

extern "C" {

int ctsp_abi_version(void) { return CTSP_ABI_VERSION; }
const char* ctsp_last_error(void) { return g_err.msg; }

int ctsp_symbol_bits(int k) { return k < 1 || k > CTSP_MAX_K ? -1 : symbol_bits(k); }

int ctsp_key_bits(int k, int D) {
    int b;
    return shape_of(k, D, &b) == CTSP_OK ? b * D : -1;
}

int64_t ctsp_capacity(int k, int D, int level, int64_t present, int64_t n, int64_t floor_cap) {
    int b;
    if (shape_of(k, D, &b) != CTSP_OK || level < 0 || level > D || present < 0 || n < 0 || floor_cap < 0) return -1;
    if (present > ((int64_t)1 << 38) || n > ((int64_t)1 << 38) || floor_cap > ((int64_t)1 << 40)) return -1;
    int64_t need = present + new_nodes_bound(k, level, n);
    const int64_t all = level_size(k, level);
    if (need > all) need = all;
    int64_t cap = 2;
    while (cap < 2 * need || cap < floor_cap) cap *= 2;
    return cap;
}

int64_t ctsp_slot_bytes(int k) { return k < 1 || k > CTSP_MAX_K ? -1 : 8 + 8 * (int64_t)k + 8 + 1 + 1 + 8 * (int64_t)k + 8; }

int ctsp_count(int dtype, const void* x_dev, int64_t n, int k, int D, const int64_t* off, void* key_dev, void* cnt_dev,
               void* lnw_dev, void* status_dev, void* stream) {
    int b;
    if (int rc = check_shape("ctsp_count", k, D, &b)) return rc;
    if (dtype < CTSP_U8 || dtype > CTSP_I64)
        return g_err.fail(CTSP_EINVAL, "ctsp_count: dtype must be CTSP_U8, CTSP_I32 or CTSP_I64");
    if (n < 1) return g_err.fail(CTSP_EINVAL, "ctsp_count: n must be >= 1");
    if (!x_dev || !key_dev || !cnt_dev || !lnw_dev || !status_dev) return g_err.fail(CTSP_EINVAL, "ctsp_count: null pointer");
    if (int rc = check_offsets("ctsp_count", off, D)) return rc;
    if (misaligned(x_dev, elem_size(dtype)))
        return g_err.fail(CTSP_EINVAL, "ctsp_count: x_dev must be aligned to its element size");
    if (any_misaligned(8, key_dev, cnt_dev, lnw_dev, status_dev))
        return g_err.fail(CTSP_EINVAL, "ctsp_count: key_dev, cnt_dev, lnw_dev and status_dev must be aligned to 8 bytes");
    hipStream_t st = (hipStream_t)stream;
    const size_t slots = (size_t)off[D + 1];
    hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int64_t) * CTSP_STATUS_LEN, st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt_dev, 0, sizeof(int64_t) * slots * (size_t)k, st);
    if (e == hipSuccess) e = hipMemsetAsync(lnw_dev, 0, sizeof(double) * slots, st);
    if (e != hipSuccess) return g_err.hip(CTSP_EHIP, "ctsp_count: hipMemsetAsync", e);
    u64* key = (u64*)key_dev;
    u64* cnt = (u64*)cnt_dev;
    int64_t* status = (int64_t*)status_dev;
    if (dtype == CTSP_U8) return launch_count<uint8_t>(x_dev, n, k, b, D, off, key, cnt, status, st);
    if (dtype == CTSP_I32) return launch_count<int32_t>(x_dev, n, k, b, D, off, key, cnt, status, st);
    return launch_count<int64_t>(x_dev, n, k, b, D, off, key, cnt, status, st);
}

int ctsp_levelup(int k, int D, const int64_t* off, void* key_dev, void* cnt_dev, const void* head_dev, int n_head,
                 void* status_dev, void* stream) {
    int b;
    if (int rc = check_shape("ctsp_levelup", k, D, &b)) return rc;
    if (n_head < 0 || n_head > D) return g_err.fail(CTSP_EINVAL, "ctsp_levelup: n_head must be in 0..D");
    if (!key_dev || !cnt_dev || !status_dev || (n_head > 0 && !head_dev))
        return g_err.fail(CTSP_EINVAL, "ctsp_levelup: null pointer");
    if (int rc = check_offsets("ctsp_levelup", off, D)) return rc;
    if (any_misaligned(8, key_dev, cnt_dev, status_dev) || misaligned(head_dev, 4))
        return g_err.fail(CTSP_EINVAL, "ctsp_levelup: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    u64* key = (u64*)key_dev;
    u64* cnt = (u64*)cnt_dev;
    for (int d = D - 1; d >= 0; --d) {
        const int64_t cap_c = off[d + 2] - off[d + 1], cap = off[d + 1] - off[d];
        hipLaunchKernelGGL(levelup_kernel, dim3(grid_of(cap_c * k, kThreads)), dim3(kThreads), 0, st, k, b, D, d, b * (D - d),
                           (const u64*)(key + off[d + 1]), cap_c, (const u64*)(cnt + off[d + 1] * k), key + off[d], cap,
                           cnt + off[d] * k, (const int32_t*)head_dev, n_head, (int64_t*)status_dev);
        if (int rc = g_err.launched("ctsp levelup_kernel launch")) return rc;
    }
    return CTSP_OK;
}

int ctsp_sweep(int k, int D, const int64_t* off, const void* key_dev, const void* cnt_dev, void* lnw_dev, void* beta_dev,
               void* g_dev, void* exists_dev, void* leaf_dev, const void* head_dev, int n_head, double hn_g,
               const void* hn_beta_dev, void* stream) {
    int b;
    if (int rc = check_shape("ctsp_sweep", k, D, &b)) return rc;
    if (n_head < 0 || n_head > D) return g_err.fail(CTSP_EINVAL, "ctsp_sweep: n_head must be in 0..D");
    if (!key_dev || !cnt_dev || !lnw_dev || !beta_dev || !g_dev || !exists_dev || !leaf_dev || !hn_beta_dev ||
        (n_head > 0 && !head_dev))
        return g_err.fail(CTSP_EINVAL, "ctsp_sweep: null pointer");
    if (!(hn_g >= 0.0 && hn_g <= 1.0)) return g_err.fail(CTSP_EINVAL, "ctsp_sweep: hn_g must be in [0, 1]");
    if (int rc = check_offsets("ctsp_sweep", off, D)) return rc;
    if (any_misaligned(8, key_dev, cnt_dev, lnw_dev, beta_dev, g_dev, hn_beta_dev) || misaligned(head_dev, 4))
        return g_err.fail(CTSP_EINVAL, "ctsp_sweep: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const u64* key = (const u64*)key_dev;
    const int64_t* cnt = (const int64_t*)cnt_dev;
    double* lnw = (double*)lnw_dev;
    double* beta = (double*)beta_dev;
    double* g = (double*)g_dev;
    uint8_t* ex = (uint8_t*)exists_dev;
    uint8_t* lf = (uint8_t*)leaf_dev;
    for (int d = D; d >= 0; --d) {
        const int dc = d < D ? d + 1 : d;          // (level d + 1's tables are not read at d = D)
        const int64_t cap = off[d + 1] - off[d];
        hipLaunchKernelGGL(sweep_kernel, dim3(grid_of(cap, kThreads)), dim3(kThreads), 0, st, k, b, D, d, b * (D - d),
                           key + off[d], cap, cnt + off[d] * k, lnw + off[d], beta + off[d] * k, g + off[d], ex + off[d],
                           lf + off[d], key + off[dc], off[dc + 1] - off[dc], (const double*)(lnw + off[dc]), hn_g,
                           (const double*)hn_beta_dev, (const int32_t*)head_dev, n_head);
        if (int rc = g_err.launched("ctsp sweep_kernel launch")) return rc;
    }
    return CTSP_OK;
}

int ctsp_map(int k, int D, const int64_t* off, const void* key_dev, const void* g_dev, const void* exists_dev, double hn_g,
             void* val_dev, void* map_leaf_dev, void* stream) {
    int b;
    if (int rc = check_shape("ctsp_map", k, D, &b)) return rc;
    if (!key_dev || !g_dev || !exists_dev || !val_dev || !map_leaf_dev) return g_err.fail(CTSP_EINVAL, "ctsp_map: null pointer");
    if (!(hn_g >= 0.0 && hn_g <= 1.0)) return g_err.fail(CTSP_EINVAL, "ctsp_map: hn_g must be in [0, 1]");
    if (int rc = check_offsets("ctsp_map", off, D)) return rc;
    if (any_misaligned(8, key_dev, g_dev, val_dev)) return g_err.fail(CTSP_EINVAL, "ctsp_map: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const u64* key = (const u64*)key_dev;
    const double* g = (const double*)g_dev;
    const uint8_t* ex = (const uint8_t*)exists_dev;
    double* val = (double*)val_dev;
    uint8_t* ml = (uint8_t*)map_leaf_dev;
    for (int d = D; d >= 0; --d) {
        const int dc = d < D ? d + 1 : d;
        const int64_t cap = off[d + 1] - off[d];
        const double pw_here = d < D ? subtree_pow(hn_g, k, D, d) : 1.0;
        hipLaunchKernelGGL(map_kernel, dim3(grid_of(cap, kThreads)), dim3(kThreads), 0, st, k, b, D, d, b * (D - d),
                           key + off[d], cap, g + off[d], ex + off[d], key + off[dc], off[dc + 1] - off[dc], ex + off[dc],
                           (const double*)(val + off[dc]), pw_here, val + off[d], ml + off[d]);
        if (int rc = g_err.launched("ctsp map_kernel launch")) return rc;
    }
    return CTSP_OK;
}

int ctsp_find(int k, int D, const int64_t* off, void* key_dev, int64_t nq, const void* q_level_dev, const void* q_key_dev,
              int insert, void* slot_dev, void* status_dev, void* stream) {
    int b;
    if (int rc = check_shape("ctsp_find", k, D, &b)) return rc;
    if (nq < 1) return g_err.fail(CTSP_EINVAL, "ctsp_find: nq must be >= 1");
    if (!key_dev || !q_level_dev || !q_key_dev || !slot_dev || !status_dev)
        return g_err.fail(CTSP_EINVAL, "ctsp_find: null pointer");
    if (int rc = check_offsets("ctsp_find", off, D)) return rc;
    if (any_misaligned(8, key_dev, q_key_dev, slot_dev, status_dev) || misaligned(q_level_dev, 4))
        return g_err.fail(CTSP_EINVAL, "ctsp_find: misaligned pointer");
    Offsets lv;
    for (int d = 0; d <= D + 1; ++d) lv.off[d] = off[d];
    for (int d = D + 2; d <= kMaxLevels; ++d) lv.off[d] = off[D + 1];
    hipLaunchKernelGGL(find_kernel, dim3(grid_of(nq, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, b, D, lv,
                       (u64*)key_dev, nq, (const int32_t*)q_level_dev, (const u64*)q_key_dev, insert, (int64_t*)slot_dev,
                       (int64_t*)status_dev);
    return g_err.launched("ctsp find_kernel launch");
}

int ctsp_rehash(int k, int D, const int64_t* off_old, const void* key_old_dev, const void* beta_old_dev,
                const void* g_old_dev, const void* exists_old_dev, const void* leaf_old_dev, const int64_t* off_new,
                void* key_new_dev, void* beta_new_dev, void* g_new_dev, void* exists_new_dev, void* leaf_new_dev,
                void* status_dev, void* stream) {
    int b;
    if (int rc = check_shape("ctsp_rehash", k, D, &b)) return rc;
    if (!key_old_dev || !beta_old_dev || !g_old_dev || !exists_old_dev || !leaf_old_dev || !key_new_dev || !beta_new_dev ||
        !g_new_dev || !exists_new_dev || !leaf_new_dev || !status_dev)
        return g_err.fail(CTSP_EINVAL, "ctsp_rehash: null pointer");
    if (int rc = check_offsets("ctsp_rehash", off_old, D)) return rc;
    if (int rc = check_offsets("ctsp_rehash", off_new, D)) return rc;
    if (any_misaligned(8, key_old_dev, beta_old_dev, g_old_dev, key_new_dev, beta_new_dev, g_new_dev, status_dev))
        return g_err.fail(CTSP_EINVAL, "ctsp_rehash: misaligned pointer");
    if (key_old_dev == key_new_dev) return g_err.fail(CTSP_EINVAL, "ctsp_rehash: the old and the new tables must differ");
    hipStream_t st = (hipStream_t)stream;
    for (int d = 0; d <= D; ++d) {
        const int64_t oo = off_old[d], on = off_new[d], cap_o = off_old[d + 1] - oo, cap_n = off_new[d + 1] - on;
        hipLaunchKernelGGL(rehash_kernel, dim3(grid_of(cap_o, kThreads)), dim3(kThreads), 0, st, k, (const u64*)key_old_dev + oo,
                           cap_o, (const double*)beta_old_dev + oo * k, (const double*)g_old_dev + oo,
                           (const uint8_t*)exists_old_dev + oo, (const uint8_t*)leaf_old_dev + oo, (u64*)key_new_dev + on, cap_n,
                           (double*)beta_new_dev + on * k, (double*)g_new_dev + on, (uint8_t*)exists_new_dev + on,
                           (uint8_t*)leaf_new_dev + on, (int64_t*)status_dev);
        if (int rc = g_err.launched("ctsp rehash_kernel launch")) return rc;
    }
    return CTSP_OK;
}

}  // extern "C"
