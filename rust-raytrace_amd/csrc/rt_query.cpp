// C ABI: ray queries (include/raytrace_amd.h, "ray queries").  Here are the argument checks of rt_query_nearest /
// rt_query_occluded and their device variants, the refusals that leave the context's statistics alone, and the host
// variants' plain allocate / copy in / render / copy out / free (the render itself is rt_render.cpp's, render_query;
// the kernels wf_query.hip's).
#include <cstdio>

#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

// What every entry point refuses before anything of the context changes.
int check_call(rt_ctx* c, bool occlusion, bool device, const double* rays, uint32_t n, uint32_t channels,
               const rt_hit_buffers* bufs, const uint8_t* occluded, uint32_t flags) {
    QueryArgs a;
    a.occlusion = occlusion; a.device = device;
    a.rays = rays; a.n = n; a.channels = channels; a.flags = flags;
    a.has_bufs = bufs != nullptr;
    if (bufs) { a.ptrs[0] = bufs->t; a.ptrs[1] = bufs->object; a.ptrs[2] = bufs->normal; }
    a.occluded = occluded;
    const char* why = nullptr;
    if (const int rc = plan_query_args(a, &why); rc != RT_OK) return fail(c, rc, why);
    if (!c->has_scene) return fail(c, RT_E_NOSCENE, "no scene uploaded");
    return RT_OK;
}

// Only the selected buffers are read from the caller's struct (none of an empty batch).
QueryOut selected(uint32_t n, uint32_t channels, const rt_hit_buffers* b) {
    QueryOut out{};
    if (n == 0) return out;
    if (channels & RT_HIT_T) out.t = b->t;
    if (channels & RT_HIT_OBJECT) out.object = b->object;
    if (channels & RT_HIT_NORMAL) out.normal = b->normal;
    return out;
}

int nearest_device(rt_ctx* c, const double* d_rays, uint32_t n, uint32_t channels, const rt_hit_buffers* dev, uint32_t flags,
                   void* stream) {
    if (const int rc = check_call(c, false, true, d_rays, n, channels, dev, nullptr, flags); rc != RT_OK) return rc;
    QueryCall q;
    q.rays = d_rays; q.n = n; q.channels = channels; q.flags = flags;
    q.out = selected(n, channels, dev);
    return render_query(c, q, stream);
}

int occluded_device(rt_ctx* c, const double* d_rays, const double* d_r2, uint32_t n, uint8_t* d_occluded, uint32_t flags,
                    void* stream) {
    if (const int rc = check_call(c, true, true, d_rays, n, 0, nullptr, d_occluded, flags); rc != RT_OK) return rc;
    QueryCall q;
    q.occlusion = true;
    q.rays = d_rays; q.r2 = d_r2; q.ranged = d_r2 != nullptr; q.n = n; q.flags = flags;
    q.occluded = d_occluded;
    return render_query(c, q, stream);
}

// The host variants, the plain way: device buffers for the rays, the ranges and the selected outputs, one copy in,
// the render on the context's stream, one copy per output, free.  No performance claim.
// Staged: the call's device buffers (rays, ranges or t, object, normal, occluded), bytes[i] each (0: none).
struct Staged {
    static constexpr int kN = 5;
    void* d[kN] = {};
    void release() {
        for (void*& p : d)
            if (p) { (void)hipFree(p); p = nullptr; }
    }
    int alloc(rt_ctx* c, const size_t bytes[kN], const char* who) {
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

// Copies in (in[i]: the host source of buffer i, null: none), the render, copies out (out[i]: the host destination,
// null: none), synchronise, free: on every path.
int run_host(rt_ctx* c, Staged& s, const size_t bytes[Staged::kN], const void* const in[Staged::kN], void* const out[Staged::kN],
             const QueryCall& q, rt_stats* stats, const char* who) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < Staged::kN && e == hipSuccess; ++i)
        if (s.d[i] && in[i]) e = hipMemcpyAsync(s.d[i], in[i], bytes[i], hipMemcpyHostToDevice, c->stream);
    int rc = RT_OK;
    if (e == hipSuccess) rc = render_query(c, q, nullptr);
    for (int i = 0; i < Staged::kN && rc == RT_OK && e == hipSuccess; ++i)
        if (s.d[i] && out[i]) e = hipMemcpyAsync(out[i], s.d[i], bytes[i], hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also before the buffers are freed after a failure
    s.release();
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return hip_fail(c, e, who);
    if (es != hipSuccess) return hip_fail(c, es, who);
    if (stats) return rt_ctx_stats(c, stats);
    return check_join_error(c);
}

int nearest_host(rt_ctx* c, const double* rays, uint32_t n, uint32_t channels, const rt_hit_buffers* host, uint32_t flags,
                 rt_stats* stats) {
    if (const int rc = check_call(c, false, false, rays, n, channels, host, nullptr, flags); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const QueryOut sel = selected(n, channels, host);
    const size_t N = n;
    const size_t bytes[Staged::kN] = {N * 48, sel.t ? N * 8 : 0, sel.object ? N * 4 : 0, sel.normal ? N * 24 : 0, 0};
    const void* const in[Staged::kN] = {rays, nullptr, nullptr, nullptr, nullptr};
    void* const out[Staged::kN] = {nullptr, sel.t, sel.object, sel.normal, nullptr};
    Staged s;
    if (const int rc = s.alloc(c, bytes, "rt_query_nearest"); rc != RT_OK) return rc;
    QueryCall q;
    q.rays = static_cast<const double*>(s.d[0]); q.n = n; q.channels = channels; q.flags = flags;
    q.out = QueryOut{static_cast<double*>(s.d[1]), static_cast<int32_t*>(s.d[2]), static_cast<double*>(s.d[3])};
    return run_host(c, s, bytes, in, out, q, stats, "rt_query_nearest");
}

int occluded_host(rt_ctx* c, const double* rays, const double* r2, uint32_t n, uint8_t* occluded, uint32_t flags,
                  rt_stats* stats) {
    if (const int rc = check_call(c, true, false, rays, n, 0, nullptr, occluded, flags); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = n;
    const size_t bytes[Staged::kN] = {N * 48, r2 ? N * 8 : 0, 0, 0, N};
    const void* const in[Staged::kN] = {rays, r2, nullptr, nullptr, nullptr};
    void* const out[Staged::kN] = {nullptr, nullptr, nullptr, nullptr, n ? occluded : nullptr};
    Staged s;
    if (const int rc = s.alloc(c, bytes, "rt_query_occluded"); rc != RT_OK) return rc;
    QueryCall q;
    q.occlusion = true;
    q.rays = static_cast<const double*>(s.d[0]); q.r2 = static_cast<const double*>(s.d[1]); q.ranged = r2 != nullptr;
    q.n = n; q.flags = flags;
    q.occluded = static_cast<uint8_t*>(s.d[4]);
    return run_host(c, s, bytes, in, out, q, stats, "rt_query_occluded");
}

}  // namespace

extern "C" {

int rt_query_nearest(rt_ctx* c, const double* rays, uint32_t n, uint32_t channels, const rt_hit_buffers* host, uint32_t flags,
                     rt_stats* stats) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return nearest_host(c, rays, n, channels, host, flags, stats); });
}

int rt_query_occluded(rt_ctx* c, const double* rays, const double* r2, uint32_t n, uint8_t* occluded, uint32_t flags,
                      rt_stats* stats) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return occluded_host(c, rays, r2, n, occluded, flags, stats); });
}

int rt_query_nearest_device(rt_ctx* c, const double* d_rays, uint32_t n, uint32_t channels, const rt_hit_buffers* dev,
                            uint32_t flags, void* stream) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return nearest_device(c, d_rays, n, channels, dev, flags, stream); });
}

int rt_query_occluded_device(rt_ctx* c, const double* d_rays, const double* d_r2, uint32_t n, uint8_t* d_occluded,
                             uint32_t flags, void* stream) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return occluded_device(c, d_rays, d_r2, n, d_occluded, flags, stream); });
}

}  // extern "C"
