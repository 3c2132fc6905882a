// What the two translation units of include/regvb.h share: the thread-local error slot and the tile dispatch.
#pragma once
#include "../../include/regvb.h"
#include "entry.h"
#include "regvb_kernels.h"

namespace regvb {
extern thread_local entry::Err g_err;      // behind regvb_last_error() (regvb_stats.hip)

// f(std::integral_constant<int, T>) for the even tile count T = even_tiles(D), D <= 256
template <typename F>
inline void for_tiles(int T, F&& f) {
    switch (T) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 10: f(std::integral_constant<int, 10>{}); break;
        case 12: f(std::integral_constant<int, 12>{}); break;
        case 14: f(std::integral_constant<int, 14>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}
}  // namespace regvb
