// include/mvnseq.h: the argument checks and the eight launches of a pass (mvnseq_kernels.h); the schedule is regseq's.
#include "../../include/mvnseq.h"
#include "regvb_internal.h"
#include "mvnseq_kernels.h"

namespace mvnseq {
ENTRY_SAME_CODES(MVNSEQ);
static_assert(MVNSEQ_BLOCK == kBlock && MVNSEQ_MAX_DEGREE == REGVB_MAX_DEGREE, "mvnseq.h and the kernels disagree");
static_assert((int)MVNSEQ_F32 == (int)REGVB_F32 && (int)MVNSEQ_F64 == (int)REGVB_F64, "mvnseq.h repeats regvb.h's codes");
static thread_local entry::Err g_err = {""};

using regseq::block_count;
using regseq::block_start;

// work:  [ table (nb + 1 int64) | colsum [nb][PD] | scale [nb][B] | mean_rel [nb][B][D] | slabs [nb][gram_slab_len(T)] |
//          states [nb][state_len(D)] ]
struct Layout {
    int64_t colsum, scale, means, slabs, states, total;
};
static Layout layout_of(int D, int64_t nb) {
    Layout l;
    l.colsum = nb + 1;
    l.scale = l.colsum + nb * padded(D);
    l.means = l.scale + nb * kBlock;
    l.slabs = l.means + nb * kBlock * D;
    l.states = l.slabs + nb * regvb::gram_slab_len(regvb::even_tiles(D));
    l.total = l.states + nb * state_len(D);
    return l;
}

// the block whose first row is `row` in the schedule of n rows (row = n: the block count), or -1
static int64_t block_at(int64_t n, int64_t row) {
    if (row == n) return block_count(n);
    if (row < 0 || row > n) return -1;
    int64_t b;
    if (row < kBlock - 1) {
        b = 0;
        while (((int64_t)1 << b) - 1 < row) ++b;
    } else {
        b = regseq::kLog2Block + (row - (kBlock - 1)) / kBlock;
    }
    return block_start(n, b) == row ? b : -1;
}

struct PassArgs {
    int D;
    int64_t ldx, n_rows;
    const double* start;
    double* carry;
    double* p_m;
    int64_t ld_pm;
    RowOutputs out;
    double* work;
    hipStream_t st;
};

template <typename XT>
static int launch_pass(const XT* x, const PassArgs& a, int64_t b0, int64_t nb) {
    const int D = a.D, T = regvb::even_tiles(D);
    const Layout l = layout_of(D, nb);
    int64_t* table = (int64_t*)a.work;
    double* colsum = a.work + l.colsum;
    double* scale = a.work + l.scale;
    double* means = a.work + l.means;
    double* slabs = a.work + l.slabs;
    double* states = a.work + l.states;
    const unsigned grid = (unsigned)nb;
    const int cols = D <= 64 ? 64 : (D <= 128 ? 128 : 256);        // a thread per column
    hipLaunchKernelGGL(regseq::block_table_kernel, dim3(entry::grid_of(nb + 1, 256)), dim3(256), 0, a.st, a.n_rows, b0, nb, table);
    if (int rc = g_err.launched("block_table_kernel launch")) return rc;
    hipLaunchKernelGGL((block_colsum_kernel<XT>), dim3(grid), dim3(cols), 0, a.st, x, a.ldx, D, table, colsum);
    if (int rc = g_err.launched("block_colsum_kernel launch")) return rc;
    hipLaunchKernelGGL(colsum_scan_kernel, dim3(entry::grid_of(D, 64)), dim3(64), 0, a.st, nb, D, a.carry, colsum);
    if (int rc = g_err.launched("colsum_scan_kernel launch")) return rc;
    hipLaunchKernelGGL((block_means_kernel<XT>), dim3(grid), dim3(cols), 0, a.st, x, a.ldx, D, table, a.start, colsum, means,
                       scale, a.p_m, a.ld_pm);
    if (int rc = g_err.launched("block_means_kernel launch")) return rc;
    const CentredRows<XT> src = {x, a.ldx, D, means, scale, block_start(a.n_rows, b0)};
    regvb::for_tiles(T, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        hipLaunchKernelGGL((regseq::block_gram_kernel<TT, CentredRows<XT>>), dim3(grid), dim3(32 * TT), 0, a.st, src, table, slabs);
    });
    if (int rc = g_err.launched("block_gram_kernel launch")) return rc;
    hipLaunchKernelGGL(gram_scan_kernel, dim3(entry::grid_of((int64_t)D * D + 1, 64)), dim3(64), 0, a.st, slabs, table, nb, T, D,
                       a.carry, states);
    if (int rc = g_err.launched("gram_scan_kernel launch")) return rc;
    hipLaunchKernelGGL(block_start_kernel, dim3(grid), dim3(1024), 0, a.st, a.start, D, states);
    if (int rc = g_err.launched("block_start_kernel launch")) return rc;
    hipLaunchKernelGGL((block_innovations_kernel<CentredRows<XT>>), dim3(grid), dim3(256), 0, a.st, src, table, states, a.start,
                       D, a.out);
    return g_err.launched("block_innovations_kernel launch");
}
}  // namespace mvnseq

using namespace mvnseq;

extern "C" {

int mvnseq_abi_version(void) { return MVNSEQ_ABI_VERSION; }
const char* mvnseq_last_error(void) { return g_err.msg; }

int mvnseq_block(int D) { return D < 1 || D > MVNSEQ_MAX_DEGREE ? -1 : kBlock; }

int64_t mvnseq_block_count(int64_t n) { return n < 1 ? -1 : block_count(n); }

int64_t mvnseq_block_start(int64_t n, int64_t b) {
    if (n < 1 || b < 0 || b > block_count(n)) return -1;
    return block_start(n, b);
}

int64_t mvnseq_work_len(int D, int64_t blocks) {
    if (D < 1 || D > MVNSEQ_MAX_DEGREE || blocks < 1 || blocks > ((int64_t)1 << 31) - 1) return -1;
    return layout_of(D, blocks).total;
}

int mvnseq_pass(int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, int64_t row_begin, int64_t row_count,
                const double* start_dev, double* carry_dev, double* p_m_dev, int64_t ld_pm, double* logdet_dev,
                double* quad_dev, double* nats_dev, double* work_dev, void* stream) {
    const char* who = "mvnseq_pass";
    if (D < 1 || D > MVNSEQ_MAX_DEGREE) return g_err.fail(MVNSEQ_EINVAL, "%s: D must be in 1..256", who);
    if (x_dtype != MVNSEQ_F32 && x_dtype != MVNSEQ_F64)
        return g_err.fail(MVNSEQ_EINVAL, "%s: x_dtype must be MVNSEQ_F32 or MVNSEQ_F64", who);
    if (n_rows < 1) return g_err.fail(MVNSEQ_EINVAL, "%s: n_rows must be >= 1", who);
    if (ldx < D) return g_err.fail(MVNSEQ_EINVAL, "%s: ldx must be >= D", who);
    if (p_m_dev && ld_pm < D) return g_err.fail(MVNSEQ_EINVAL, "%s: ld_pm must be >= D", who);
    if (row_count < 1) return g_err.fail(MVNSEQ_EINVAL, "%s: row_count must be >= 1", who);
    const int64_t first = block_at(n_rows, row_begin);
    const int64_t last = row_begin + row_count > row_begin ? block_at(n_rows, row_begin + row_count) : -1;
    if (first < 0 || last < 0)
        return g_err.fail(MVNSEQ_EINVAL, "%s: the rows [%lld, %lld) are not whole blocks of the schedule of %lld rows", who,
                          (long long)row_begin, (long long)(row_begin + row_count), (long long)n_rows);
    if (!x_dev || !start_dev || !carry_dev || !work_dev) return g_err.fail(MVNSEQ_EINVAL, "%s: null pointer", who);
    if (entry::misaligned(x_dev, x_dtype == MVNSEQ_F32 ? 4 : 8))
        return g_err.fail(MVNSEQ_EINVAL, "%s: x must be aligned to its element size", who);
    if (entry::any_misaligned(8, start_dev, carry_dev, work_dev, p_m_dev, logdet_dev, quad_dev, nats_dev))
        return g_err.fail(MVNSEQ_EINVAL, "%s: the double arrays must be 8-byte aligned", who);
    const PassArgs a = {D, ldx, n_rows, start_dev, carry_dev, p_m_dev, ld_pm, {logdet_dev, quad_dev, nats_dev}, work_dev,
                        (hipStream_t)stream};
    if (x_dtype == MVNSEQ_F32) return launch_pass((const float*)x_dev, a, first, last - first);
    return launch_pass((const double*)x_dev, a, first, last - first);
}

}  // extern "C"
