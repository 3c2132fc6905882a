// The per-row stage of hmmpred.hip, for the translation units that share it (hmmpred.hip itself and hmmbatch.hip): its
// kernels are instantiated once, in hmmpred.o.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hmmpred {

// ln e [K][npad] of the n_rows >= 1 rows of x (emission_kernel up to D = 128, emission_plain_kernel above), then rho'
// [n_rows][Kp] in lane order and m [n_rows] of it (hmm_prep_kernel up to 64 states, hmm_prep_generic_kernel above).  Enqueues
// only.  Returns an hmmpred_status; on failure the message is hmmpred_last_error()'s.
int emit_rows(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* pivot_dev,
              const double* img_dev, const double* c_dev, const double* nu_dev, double* lne, int64_t npad, double* rho,
              double* m, hipStream_t st);

}  // namespace hmmpred
