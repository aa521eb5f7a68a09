// C ABI: ray queries (include/raytrace_amd.h, "ray queries").  Here are the argument checks of rt_query_nearest /
// rt_query_occluded and their device variants, the refusals that leave the context's statistics alone, and the host
// variants' plain allocate / copy in / render / copy out / free (the render itself is rt_render.cpp's, render_query;
// the kernels wf_query.hip's).
#include <cstdio>

#include "host_staging.hpp"
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

// The host variants, the plain way (host_staging.hpp): device buffers for the rays, the ranges and the selected
// outputs, one copy in, the render on the context's stream, one copy per output, free.  After a render that
// succeeded: the statistics, if asked for, else what a device-side join may have to report.
int after_render(rt_ctx* c, int rc, rt_stats* stats) {
    if (rc != RT_OK) return rc;
    if (stats) return rt_ctx_stats(c, stats);
    return check_join_error(c);
}

int nearest_host(rt_ctx* c, const double* rays, uint32_t n, uint32_t channels, const rt_hit_buffers* host, uint32_t flags,
                 rt_stats* stats) {
    if (const int rc = check_call(c, false, false, rays, n, channels, host, nullptr, flags); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const QueryOut sel = selected(n, channels, host);
    const size_t N = n;
    const size_t bytes[4] = {N * 48, sel.t ? N * 8 : 0, sel.object ? N * 4 : 0, sel.normal ? N * 24 : 0};
    const void* const in[4] = {rays, nullptr, nullptr, nullptr};
    void* const out[4] = {nullptr, sel.t, sel.object, sel.normal};
    const char* const who = "rt_query_nearest";
    return after_render(c, run_staged(c, bytes, in, out, StagedTexts{who, who, who}, [&](const Staged<4>& s) {
        QueryCall q;
        q.rays = s.as<const double>(0); q.n = n; q.channels = channels; q.flags = flags;
        q.out = QueryOut{s.as<double>(1), s.as<int32_t>(2), s.as<double>(3)};
        return render_query(c, q, nullptr);
    }), stats);
}

int occluded_host(rt_ctx* c, const double* rays, const double* r2, uint32_t n, uint8_t* occluded, uint32_t flags,
                  rt_stats* stats) {
    if (const int rc = check_call(c, true, false, rays, n, 0, nullptr, occluded, flags); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = n;
    const size_t bytes[3] = {N * 48, r2 ? N * 8 : 0, N};
    const void* const in[3] = {rays, r2, nullptr};
    void* const out[3] = {nullptr, nullptr, n ? occluded : nullptr};
    const char* const who = "rt_query_occluded";
    return after_render(c, run_staged(c, bytes, in, out, StagedTexts{who, who, who}, [&](const Staged<3>& s) {
        QueryCall q;
        q.occlusion = true;
        q.rays = s.as<const double>(0); q.r2 = s.as<const double>(1); q.ranged = r2 != nullptr; q.n = n; q.flags = flags;
        q.occluded = s.as<uint8_t>(2);
        return render_query(c, q, nullptr);
    }), stats);
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
