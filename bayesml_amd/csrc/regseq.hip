// include/regseq.h: the schedule, the argument checks and the five launches of a pass (regseq_kernels.h).
#include "../../include/regseq.h"
#include "regvb_internal.h"
#include "regseq_kernels.h"

namespace regseq {
ENTRY_SAME_CODES(REGSEQ);
static_assert(REGSEQ_BLOCK == kBlock && REGSEQ_MAX_DEGREE == REGVB_MAX_DEGREE, "regseq.h and the kernels disagree");
static_assert((int)REGSEQ_F32 == (int)REGVB_F32 && (int)REGSEQ_F64 == (int)REGVB_F64 &&
                  (int)REGSEQ_PAD_ZEROS == (int)REGVB_PAD_ZEROS, "regseq.h repeats regvb.h's codes");
static thread_local entry::Err g_err = {""};

// work:  [ table (nb + 1 int64) | slabs [nb][gram_slab_len(T)] | states [nb][state_len(D)] ]
struct Layout {
    int64_t slabs, states, total;
};
static Layout layout_of(int D, int64_t nb) {
    Layout l;
    l.slabs = nb + 1;
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
        b = kLog2Block + (row - (kBlock - 1)) / kBlock;
    }
    return block_start(n, b) == row ? b : -1;
}

struct PassArgs {
    int D;
    int64_t n_rows, row_begin, row_count;
    const double* start;
    double* carry;
    RowOutputs out;
    double* work;
    hipStream_t st;
};

// everything about a pass that does not depend on the row source; b0, nb: the block range
static int check_pass(const char* who, const PassArgs& a, int64_t* b0, int64_t* nb) {
    if (a.row_count < 1) return g_err.fail(REGSEQ_EINVAL, "%s: row_count must be >= 1", who);
    const int64_t first = block_at(a.n_rows, a.row_begin);
    const int64_t last = a.row_begin + a.row_count > a.row_begin ? block_at(a.n_rows, a.row_begin + a.row_count) : -1;
    if (first < 0 || last < 0)
        return g_err.fail(REGSEQ_EINVAL, "%s: the rows [%lld, %lld) are not whole blocks of the schedule of %lld rows", who,
                          (long long)a.row_begin, (long long)(a.row_begin + a.row_count), (long long)a.n_rows);
    if (!a.start || !a.carry || !a.work) return g_err.fail(REGSEQ_EINVAL, "%s: null pointer", who);
    if (entry::any_misaligned(8, a.start, a.carry, a.work, a.out.p_m, a.out.p_lambda, a.out.p_nu, a.out.nats))
        return g_err.fail(REGSEQ_EINVAL, "%s: the double arrays must be 8-byte aligned", who);
    *b0 = first;
    *nb = last - first;
    return REGSEQ_OK;
}

template <typename SRC>
static int launch_pass(const SRC& src, const PassArgs& a, int64_t b0, int64_t nb) {
    const int D = a.D, T = regvb::even_tiles(D);
    const Layout l = layout_of(D, nb);
    int64_t* table = (int64_t*)a.work;
    double* slabs = a.work + l.slabs;
    double* states = a.work + l.states;
    hipLaunchKernelGGL(block_table_kernel, dim3(entry::grid_of(nb + 1, 256)), dim3(256), 0, a.st, a.n_rows, b0, nb, table);
    if (int rc = g_err.launched("block_table_kernel launch")) return rc;
    regvb::for_tiles(T, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        hipLaunchKernelGGL((block_gram_kernel<TT, SRC>), dim3((unsigned)nb), dim3(32 * TT), 0, a.st, src, table, slabs);
    });
    if (int rc = g_err.launched("block_gram_kernel launch")) return rc;
    const int64_t len = (int64_t)D * D + D + 2;
    hipLaunchKernelGGL(block_scan_kernel, dim3(entry::grid_of(len, 64)), dim3(64), 0, a.st, slabs, nb, T, D, a.carry, states);
    if (int rc = g_err.launched("block_scan_kernel launch")) return rc;
    hipLaunchKernelGGL(block_start_kernel, dim3((unsigned)nb), dim3(1024), 0, a.st, a.start, D, states);
    if (int rc = g_err.launched("block_start_kernel launch")) return rc;
    hipLaunchKernelGGL((block_innovations_kernel<SRC>), dim3((unsigned)nb), dim3(256), 0, a.st, src, table, states, a.start,
                       D, a.out);
    return g_err.launched("block_innovations_kernel launch");
}
}  // namespace regseq

using namespace regseq;

extern "C" {

int regseq_abi_version(void) { return REGSEQ_ABI_VERSION; }
const char* regseq_last_error(void) { return g_err.msg; }

int regseq_block(int D) { return D < 1 || D > REGSEQ_MAX_DEGREE ? -1 : kBlock; }

int64_t regseq_block_count(int64_t n) { return n < 1 ? -1 : block_count(n); }

int64_t regseq_block_start(int64_t n, int64_t b) {
    if (n < 1 || b < 0 || b > block_count(n)) return -1;
    return block_start(n, b);
}

int64_t regseq_work_len(int D, int64_t blocks) {
    if (D < 1 || D > REGSEQ_MAX_DEGREE || blocks < 1 || blocks > ((int64_t)1 << 31) - 1) return -1;
    return layout_of(D, blocks).total;
}

int regseq_pass(int D, int x_dtype, const void* x_dev, int64_t ldx, int y_dtype, const void* y_dev, int64_t n_rows,
                int64_t row_begin, int64_t row_count, const double* start_dev, double* carry_dev, double* p_m_dev,
                double* p_lambda_dev, double* p_nu_dev, double* nats_dev, double* work_dev, void* stream) {
    const char* who = "regseq_pass";
    if (D < 1) return g_err.fail(REGSEQ_EINVAL, "%s: D must be >= 1", who);
    if (D > REGSEQ_MAX_DEGREE) return g_err.fail(REGSEQ_EUNSUPPORTED, "%s: D > 256 is not supported", who);
    if (x_dtype != REGSEQ_F32 && x_dtype != REGSEQ_F64)
        return g_err.fail(REGSEQ_EINVAL, "%s: x_dtype must be REGSEQ_F32 or REGSEQ_F64", who);
    if (y_dtype != REGSEQ_F32 && y_dtype != REGSEQ_F64)
        return g_err.fail(REGSEQ_EINVAL, "%s: y_dtype must be REGSEQ_F32 or REGSEQ_F64", who);
    if (n_rows < 1) return g_err.fail(REGSEQ_EINVAL, "%s: n_rows must be >= 1", who);
    if (ldx < D) return g_err.fail(REGSEQ_EINVAL, "%s: ldx must be >= D", who);
    if (!x_dev || !y_dev) return g_err.fail(REGSEQ_EINVAL, "%s: null pointer", who);
    if (entry::misaligned(x_dev, x_dtype == REGSEQ_F32 ? 4 : 8) || entry::misaligned(y_dev, y_dtype == REGSEQ_F32 ? 4 : 8))
        return g_err.fail(REGSEQ_EINVAL, "%s: x and y must be aligned to their element size", who);
    const PassArgs a = {D, n_rows, row_begin, row_count, start_dev, carry_dev, {p_m_dev, p_lambda_dev, p_nu_dev, nats_dev},
                        work_dev, (hipStream_t)stream};
    int64_t b0, nb;
    if (int rc = check_pass(who, a, &b0, &nb)) return rc;
    const float* xf = (const float*)x_dev;
    const double* xd = (const double*)x_dev;
    const float* yf = (const float*)y_dev;
    const double* yd = (const double*)y_dev;
    using regvb::MatrixRows;
    if (x_dtype == REGSEQ_F32 && y_dtype == REGSEQ_F32) return launch_pass(MatrixRows<float, float>{xf, ldx, yf, D}, a, b0, nb);
    if (x_dtype == REGSEQ_F32) return launch_pass(MatrixRows<float, double>{xf, ldx, yd, D}, a, b0, nb);
    if (y_dtype == REGSEQ_F32) return launch_pass(MatrixRows<double, float>{xd, ldx, yf, D}, a, b0, nb);
    return launch_pass(MatrixRows<double, double>{xd, ldx, yd, D}, a, b0, nb);
}

int regseq_pass_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding, int64_t row_begin,
                       int64_t row_count, const double* start_dev, double* carry_dev, double* p_m_dev,
                       double* p_lambda_dev, double* p_nu_dev, double* nats_dev, double* work_dev, void* stream) {
    const char* who = "regseq_pass_window";
    if (p < 0) return g_err.fail(REGSEQ_EINVAL, "%s: p must be >= 0", who);
    if (p + 1 > REGSEQ_MAX_DEGREE) return g_err.fail(REGSEQ_EUNSUPPORTED, "%s: p + 1 > 256 is not supported", who);
    if (x_dtype != REGSEQ_F32 && x_dtype != REGSEQ_F64)
        return g_err.fail(REGSEQ_EINVAL, "%s: x_dtype must be REGSEQ_F32 or REGSEQ_F64", who);
    if (padding != REGSEQ_PAD_NONE && padding != REGSEQ_PAD_ZEROS)
        return g_err.fail(REGSEQ_EINVAL, "%s: padding must be REGSEQ_PAD_NONE or REGSEQ_PAD_ZEROS", who);
    if (length <= p) return g_err.fail(REGSEQ_EINVAL, "%s: length must be > p", who);
    if (!series_dev) return g_err.fail(REGSEQ_EINVAL, "%s: null pointer", who);
    if (entry::misaligned(series_dev, x_dtype == REGSEQ_F32 ? 4 : 8))
        return g_err.fail(REGSEQ_EINVAL, "%s: the series must be aligned to its element size", who);
    const int64_t t0 = padding == REGSEQ_PAD_ZEROS ? 0 : p;
    const PassArgs a = {p + 1, length - t0, row_begin, row_count, start_dev, carry_dev,
                        {p_m_dev, p_lambda_dev, p_nu_dev, nats_dev}, work_dev, (hipStream_t)stream};
    int64_t b0, nb;
    if (int rc = check_pass(who, a, &b0, &nb)) return rc;
    using regvb::WindowRows;
    if (x_dtype == REGSEQ_F32) return launch_pass(WindowRows<float>{(const float*)series_dev, p, t0}, a, b0, nb);
    return launch_pass(WindowRows<double>{(const double*)series_dev, p, t0}, a, b0, nb);
}

}  // extern "C"
