// Instantiations of the int8-digit E-step for T32 = ceil(D/32) in 1..4, x in {f32, f64}: the 6-digit E-step and the
// 3-digit bound pass of the pruned E-step.
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include "aux_kernels.h"
#include "estep_i8.h"
#include "launch.h"

namespace gmmvb {

int estep_i8_image_bytes(int D, int bound) { return i8_img_bytes(bound ? kBoundDigits : kDigits, i8_blocks(D)); }
int estep_i8_rows_per_wg() { return 8 * 32; }

// Every image of a parameter hand-over in one launch (gmmvb_set_params, D <= 128): blockIdx.x = component, blockIdx.y =
// image kind - 0: the f64 image, c -> cvec and the pivot copy; then one per int8 image the workspace has (the 6-digit one
// first).  Before: a launch per image, back to back at the head of every iteration, each walking the rows of u in global
// memory with one thread per row (loads strided by D doubles across the lanes).  Now a workgroup stages the lower triangle
// of u_k once with coalesced row reads - [D][ld] doubles, ld odd (129 at D = 128): a thread per row walks its row without
// bank conflicts - and the row scans, the tile loop and the digit loop all read that copy.  The scans keep their order of
// operations, so the images are the same bits as before.
// The int8 workgroups take the pivot from its source: the copy in pivot_dst is being written by workgroup (0, 0) of the same
// launch.
constexpr int kPackThreads = 512;
__global__ __launch_bounds__(kPackThreads) void pack_images_kernel(const double* __restrict__ u, const double* __restrict__ m,
                                                                    const double* __restrict__ c_src, const double* __restrict__ pivot_src,
                                                                    int K, int D, int T, int img_len, double* __restrict__ img,
                                                                    double* __restrict__ c_dst, double* __restrict__ pivot_dst,
                                                                    int T32, unsigned char* __restrict__ img6, int img6_bytes,
                                                                    unsigned char* __restrict__ img3, int img3_bytes) {
    extern __shared__ double us[];          // [D][ld] lower triangle of u_k | mv [D]
    __shared__ double row_scale[128], row_max[128], row_beta[128];
    __shared__ int row_bad[128];
    const int k = blockIdx.x, kind = blockIdx.y;
    const int ld = D | 1;
    double* mv = us + D * ld;
    const double* uk = u + (int64_t)k * D * D;
    for (int e = threadIdx.x; e < D * D; e += kPackThreads) {
        const int i = e / D, j = e - i * D;
        if (j <= i) us[i * ld + j] = uk[e];
    }
    for (int i = threadIdx.x; i < D; i += kPackThreads) {
        const double mi = m[(int64_t)k * D + i];
        mv[i] = kind == 0 ? mi : mi - pivot_src[i];
    }
    __syncthreads();
    if (kind == 0) {
        if (threadIdx.x == 0) c_dst[k] = c_src[k];
        if (pivot_dst && k == 0)
            for (int f = threadIdx.x; f < D; f += kPackThreads) pivot_dst[f] = pivot_src[f];
        pack_f64_image(us, ld, mv, D, T, img_len, img + (int64_t)k * img_len);
    } else if (kind == 1 && img6) {
        pack_i8_image<kDigits>(us, ld, mv, D, T32, img6_bytes, img6 + (int64_t)k * img6_bytes, row_scale, row_max, row_beta, row_bad);
    } else {
        pack_i8_image<kBoundDigits>(us, ld, mv, D, T32, img3_bytes, img3 + (int64_t)k * img3_bytes, row_scale, row_max, row_beta,
                                    row_bad);
    }
}

hipError_t launch_pack_images(const double* u, const double* m, const double* c_src, const double* pivot_src, int K, int D, int T,
                              int img_len, double* img, double* cvec, double* pivot_dst, unsigned char* img6, unsigned char* img3,
                              hipStream_t st) {
    if (D > 128 || ((img6 || img3) && !pivot_dst)) return hipErrorInvalidValue;
    // more than 64 KB of dynamic LDS has to be asked for, once per device
    static std::mutex mu;
    static bool asked[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (dev < 0 || dev >= 64 || !asked[dev]) {
            e = hipFuncSetAttribute((const void*)pack_images_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((128 * 129 + 128) * sizeof(double)));
            if (e != hipSuccess) return e;
            if (dev >= 0 && dev < 64) asked[dev] = true;
        }
    }
    const int t32 = i8_blocks(D);
    const size_t lds = ((size_t)D * (D | 1) + D) * sizeof(double);
    const unsigned kinds = 1u + (img6 ? 1u : 0u) + (img3 ? 1u : 0u);
    hipLaunchKernelGGL(pack_images_kernel, dim3(K, kinds), dim3(kPackThreads), lds, st, u, m, c_src, pivot_src, K, D, T, img_len, img,
                       cvec, pivot_dst, t32, img6, i8_img_bytes(kDigits, t32), img3, i8_img_bytes(kBoundDigits, t32));
    return hipGetLastError();
}

template <int ND, bool BOUND, int T32, int TB, typename XT, bool VEC>
static hipError_t go(int grid, hipStream_t st, const EstepI8Args& a) {
    hipLaunchKernelGGL((estep_i8<ND, BOUND, T32, TB, XT, VEC, 8>), dim3(grid), dim3(512), 0, st,
                       static_cast<const XT*>(a.x), a.ldx, a.n_rows, a.D, a.img, a.pivot, a.cvec, a.K, a.lnrho, a.npad, a.khat, a.ub);
    return hipGetLastError();
}

template <int ND, bool BOUND, int T32, int TB>
static hipError_t pick_x(int x_is_f64, bool vec, int grid, hipStream_t st, const EstepI8Args& a) {
    if (x_is_f64) return vec ? go<ND, BOUND, T32, TB, double, true>(grid, st, a) : go<ND, BOUND, T32, TB, double, false>(grid, st, a);
    return vec ? go<ND, BOUND, T32, TB, float, true>(grid, st, a) : go<ND, BOUND, T32, TB, float, false>(grid, st, a);
}

hipError_t launch_estep_i8(int x_is_f64, bool vec, int grid, hipStream_t st, const EstepI8Args& a, const char** name) {
    static const char* names[] = {"", "estep_i8<T32=1>", "estep_i8<T32=2>", "estep_i8<T32=3>", "estep_i8<T32=4>"};
    const int t32 = i8_blocks(a.D);
    *name = names[t32 <= 4 ? t32 : 0];
    switch (t32) {
        case 1: return pick_x<kDigits, false, 1, 1>(x_is_f64, vec, grid, st, a);
        case 2: return pick_x<kDigits, false, 2, 2>(x_is_f64, vec, grid, st, a);
        case 3: return pick_x<kDigits, false, 3, 3>(x_is_f64, vec, grid, st, a);
        case 4: return pick_x<kDigits, false, 4, 4>(x_is_f64, vec, grid, st, a);
    }
    return hipErrorInvalidValue;
}

// tb = output blocks the bound pass evaluates, 1 .. ceil(D / 32)
hipError_t launch_estep_i8_bound(int x_is_f64, bool vec, int tb, int grid, hipStream_t st, const EstepI8Args& a,
                                 const char** name) {
    static const char* names[5][5] = {
        {"", "", "", "", ""},
        {"", "estep_i8_bound<T32=1,blocks=1>", "", "", ""},
        {"", "estep_i8_bound<T32=2,blocks=1>", "estep_i8_bound<T32=2,blocks=2>", "", ""},
        {"", "estep_i8_bound<T32=3,blocks=1>", "estep_i8_bound<T32=3,blocks=2>", "estep_i8_bound<T32=3,blocks=3>", ""},
        {"", "estep_i8_bound<T32=4,blocks=1>", "estep_i8_bound<T32=4,blocks=2>", "estep_i8_bound<T32=4,blocks=3>",
         "estep_i8_bound<T32=4,blocks=4>"}};
    const int t32 = i8_blocks(a.D);
    if (t32 < 1 || t32 > 4 || tb < 1 || tb > t32) return hipErrorInvalidValue;
    *name = names[t32][tb];
#define BC(T, B) \
    if (t32 == T && tb == B) return pick_x<kBoundDigits, true, T, B>(x_is_f64, vec, grid, st, a);
    BC(1, 1) BC(2, 1) BC(2, 2) BC(3, 1) BC(3, 2) BC(3, 3) BC(4, 1) BC(4, 2) BC(4, 3) BC(4, 4)
#undef BC
    return hipErrorInvalidValue;
}

// sample digits in HBM; two-sided bounds of listed pairs over them (the proof round): all ceil(D / 32) blocks, three digits
int64_t estep_i8_digit_row_bytes(int D) { return i8_digit_row_bytes(i8_blocks(D)); }

hipError_t launch_x_digits(const void* x, int x_is_f64, int64_t ldx, int64_t n_rows, int D, const double* pivot,
                           unsigned char* xq, signed char* xqe, hipStream_t st) {
    const int t32 = i8_blocks(D);
    if (t32 < 1 || t32 > 4) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n_rows + 31) / 32);
    if (x_is_f64)
        hipLaunchKernelGGL(x_digits_kernel<double>, dim3(grid), dim3(256), 0, st, static_cast<const double*>(x), ldx, n_rows, D,
                           t32, pivot, xq, xqe);
    else
        hipLaunchKernelGGL(x_digits_kernel<float>, dim3(grid), dim3(256), 0, st, static_cast<const float*>(x), ldx, n_rows, D,
                           t32, pivot, xq, xqe);
    return hipGetLastError();
}

int estep_i8_pairs_per_chunk() { return i8_pairs_per_chunk(); }

hipError_t launch_estep_i8_proof(int D, int grid, hipStream_t st, const unsigned char* xq, const signed char* xqe,
                                 const unsigned char* img, const double* cvec, int K, const int* lists, int64_t cap,
                                 const int* counts, const int* plan, float* ub, double* lb, int64_t npad) {
    if (K > 256) return hipErrorInvalidValue;
    grid *= 2;      // two workgroups per CU (108 registers: four waves per SIMD): 1.21 -> 1.10 ms per step at the benchmark shape;
                    // the kernel streams 385 B of digit planes per pair at 3.4 TB/s, three or four per CU change nothing
#define PC(T)                                                                                                              \
    case T:                                                                                                                \
        hipLaunchKernelGGL((estep_i8_proof<T>), dim3(grid), dim3(512), 0, st, xq, xqe, img, cvec, K, lists, cap, counts,   \
                           plan, ub, lb, npad);                                                                            \
        return hipGetLastError();
    switch (i8_blocks(D)) {
        PC(1) PC(2) PC(3) PC(4)
    }
#undef PC
    return hipErrorInvalidValue;
}


// The proof round over row superblocks (estep_i8.h, estep_i8_proof_blocked).  `work` holds the item table: per superblock
// totals and bases, per (superblock, component) item counts, then the items themselves - at most pairs / 256 + one per
// (superblock, component).  The caller hands over a buffer that is free during the E-step (the M-step's slabs).
int64_t estep_i8_proof_work_bytes(int K, int64_t n_rows) {
    const int64_t nblk = (n_rows + 255) / 256;
    const int64_t n_super = (nblk * 256 + kProofSuperRows - 1) / kProofSuperRows;
    const int64_t head = ((2 * n_super + kProofXcds + 3) / 4 * 4 + (n_super * (K + 1) + 3) / 4 * 4) * (int64_t)sizeof(int);
    const int64_t items = n_rows * (int64_t)K / kProofItem + n_super * K + 1;
    return head + items * (int64_t)sizeof(i4v);
}

hipError_t launch_estep_i8_proof_blocked(int D, int num_cu, hipStream_t st, const unsigned char* xq, const signed char* xqe,
                                         const unsigned char* img, const double* cvec, int K, const int* lists, int64_t cap,
                                         const int* counts, const int* blk_base, int nblk, void* work, float* ub, double* lb,
                                         int64_t npad) {
    if (K > 256 || nblk < 1 || !work || ((uintptr_t)work & 15)) return hipErrorInvalidValue;
    const int n_super = (int)(((int64_t)nblk * 256 + kProofSuperRows - 1) / kProofSuperRows);
    int* tot = static_cast<int*>(work);
    int* xb = tot + n_super;
    int* xtot = xb + n_super;
    int* cum = tot + (2 * (int64_t)n_super + kProofXcds + 3) / 4 * 4;
    i4v* items = reinterpret_cast<i4v*>(cum + ((int64_t)n_super * (K + 1) + 3) / 4 * 4);
    hipLaunchKernelGGL(proof_units_kernel, dim3(n_super), dim3(256), 0, st, blk_base, counts, K, nblk, cum, tot);
    hipLaunchKernelGGL(proof_order_kernel, dim3(kProofXcds), dim3(1024), 0, st, tot, n_super, xb, xtot);
    hipLaunchKernelGGL(proof_items_kernel, dim3(n_super), dim3(256), 0, st, blk_base, counts, K, nblk, cum, xb, xtot, items);
    // as many workgroups as are resident at once (182 - 222 registers past one feature block of 32: one per CU) - the items
    // are dealt out interleaved, and a workgroup that starts late would go through the superblocks a second time
    const int per_cu = i8_blocks(D) == 1 ? 2 : 1;
    const int grid = kProofXcds * ((per_cu * num_cu + kProofXcds - 1) / kProofXcds);
#define PB(T)                                                                                                              \
    case T:                                                                                                                \
        hipLaunchKernelGGL((estep_i8_proof_blocked<T>), dim3(grid), dim3(512), 0, st, xq, xqe, img, cvec, K, lists, cap,   \
                           items, xtot, ub, lb, npad);                                                                     \
        return hipGetLastError();
    switch (i8_blocks(D)) {
        PB(1) PB(2) PB(3) PB(4)
    }
#undef PB
    return hipErrorInvalidValue;
}

}  // namespace gmmvb
