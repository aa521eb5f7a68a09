// The host variants' plain path (rt_query.cpp, rt_aov.cpp, rt_denoise.cpp), one copy: device buffers for the
// call, copies in, the device variant on the context's stream, copies out, synchronise, free.  What differs
// between the entry points stays with them: the byte counts, which buffers copy which way, the texts of
// rt_last_error, and what follows a success.  No performance claim.
#pragma once

#include <string>

#include "rt_ctx.hpp"

namespace rtamd {

// Staged: the call's device buffers, bytes[i] each (0: none).
template <int kN>
struct Staged {
    void* d[kN] = {};
    template <class T>
    T* as(int i) const { return static_cast<T*>(d[i]); }
    void release() {
        for (void*& p : d)
            if (p) { (void)hipFree(p); p = nullptr; }
    }
    int alloc(rt_ctx* c, const size_t (&bytes)[kN], const char* who) {
        for (int i = 0; i < kN; ++i) {
            if (!bytes[i]) continue;
            const hipError_t e = hipMalloc(&d[i], bytes[i]);
            if (e != hipSuccess) {
                d[i] = nullptr;
                release();
                (void)hipGetLastError();
                return e == hipErrorOutOfMemory ? fail(c, RT_E_NOMEM, std::string(who) + ": the device buffers do not fit")
                                                : hip_fail(c, e, who);
            }
        }
        return RT_OK;
    }
};

// The entry point's name (a failed allocation) and what rt_last_error says of a failed copy / synchronise.
struct StagedTexts {
    const char *who, *copy, *sync;
};

// Allocates, copies in (in[i]: the host source of buffer i, null: none), run(s) -> status, copies out (out[i]:
// the host destination, null: none; only if everything before succeeded), synchronises (also after a failure,
// before anything is freed) and frees: on every path.  The first error in that order is the one reported.
template <int kN, class Run>
int run_staged(rt_ctx* c, const size_t (&bytes)[kN], const void* const (&in)[kN], void* const (&out)[kN], const StagedTexts& t,
               Run&& run) {
    Staged<kN> s;
    if (const int rc = s.alloc(c, bytes, t.who); rc != RT_OK) return rc;
    hipError_t e = hipSuccess;
    for (int i = 0; i < kN && e == hipSuccess; ++i)
        if (s.d[i] && in[i]) e = hipMemcpyAsync(s.d[i], in[i], bytes[i], hipMemcpyHostToDevice, c->stream);
    int rc = RT_OK;
    if (e == hipSuccess) rc = run(s);
    for (int i = 0; i < kN && rc == RT_OK && e == hipSuccess; ++i)
        if (s.d[i] && out[i]) e = hipMemcpyAsync(out[i], s.d[i], bytes[i], hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also before the buffers are freed after a failure
    s.release();
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return hip_fail(c, e, t.copy);
    if (es != hipSuccess) return hip_fail(c, es, t.sync);
    return RT_OK;
}

}  // namespace rtamd
