// What the translation units of the four small C ABIs (regvb.h, expfam.h, ctree.h, mtree.h) share on the host: the status
// codes, the error slot behind a family's *_last_error(), and the grid and alignment arithmetic of their argument checks.
// Host only; the kernel headers do not include it.  (The gmmvb_* core reports through its workspace: capi_internal.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

namespace entry {

// The codes every family's status enum repeats under its own prefix.
enum { kOk = 0, kInvalid = 1, kUnsupported = 2, kHipError = 3 };
#define ENTRY_SAME_CODES(PFX)                                                                                  \
    static_assert(PFX##_OK == entry::kOk && PFX##_EINVAL == entry::kInvalid &&                                 \
                      PFX##_EUNSUPPORTED == entry::kUnsupported && PFX##_EHIP == entry::kHipError,             \
                  #PFX "_* status codes are not entry.h's")

// A family's last message.  Each family owns one `static thread_local` instance, so a failure in one family never shows in
// another's *_last_error() and every thread reads its own.  The calls return `code`, to be returned as they stand.
struct Err {
    char msg[256];

    __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        return code;
    }
    int hip(int code, const char* what, hipError_t e) { return fail(code, "%s: %s", what, hipGetErrorString(e)); }
    // after a kernel launch
    int launched(const char* what) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? kOk : hip(kHipError, what, e);
    }
};

inline unsigned grid_of(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// true for a non-null pointer that is not a multiple of `bytes`
inline bool misaligned(const void* p, size_t bytes) { return (uintptr_t)p % bytes != 0; }
template <typename... P>
inline bool any_misaligned(size_t bytes, const P*... p) {
    return (misaligned(p, bytes) || ...);
}

}  // namespace entry
