// Index arithmetic of the packed lower triangle of tile pairs.  No HIP header: policy.h and pass_plan.h read it from a plain
// host compiler as well (tests/pass_plan_cases.cpp).
#pragma once

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace gmmvb {

__host__ __device__ constexpr int tri_pairs(int t) { return t * (t + 1) / 2; }
// index of the tile pair (hi, lo) with lo <= hi in the packed lower triangle
__host__ __device__ constexpr int pair_index(int hi, int lo) { return hi * (hi + 1) / 2 + lo; }

}  // namespace gmmvb
