// C ABI: first-hit feature buffers (include/raytrace_amd.h, "first-hit feature buffers").  Here are the
// argument checks of rt_render_aov / rt_render_aov_device, the refusals that leave the context's statistics
// alone, and the host variant's plain allocate / render / copy / free (the render itself is rt_render.cpp's,
// render_aov; the kernel wf_aov.hip's).
#include <cstdio>

#include "host_staging.hpp"
#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

// Elements per pixel of channel i (depth, normal, albedo, coverage, object); all 4-byte elements.
constexpr uint32_t kElems[5] = {1, 3, 3, 1, 1};

// What both entry points refuse before anything of the context changes.
int check_call(rt_ctx* c, const rt_render_opts* o, uint32_t channels, const rt_aov_buffers* bufs) {
    if (!o || !bufs) return fail(c, RT_E_INVALID, "rt_render_aov: null argument");
    const void* const ptrs[5] = {bufs->depth, bufs->normal, bufs->albedo, bufs->coverage, bufs->object};
    const char* why = nullptr;
    if (const int rc = plan_aov_args(channels, ptrs, &why); rc != RT_OK) return fail(c, rc, why);
    if (!c->has_scene) return fail(c, RT_E_NOSCENE, "no scene uploaded");
    if (c->dsc.cam_dof)
        return fail(c, RT_E_UNSUPPORTED, "rt_render_aov: a DepthOfFieldCamera's rays go through cos and sin: no bit-exact first hits");
    return RT_OK;
}

// Only the selected buffers are read from the caller's struct.
AovOut selected(uint32_t channels, const rt_aov_buffers* b) {
    AovOut out{};
    if (channels & RT_AOV_DEPTH) out.depth = b->depth;
    if (channels & RT_AOV_NORMAL) out.normal = b->normal;
    if (channels & RT_AOV_ALBEDO) out.albedo = b->albedo;
    if (channels & RT_AOV_COVERAGE) out.coverage = b->coverage;
    if (channels & RT_AOV_OBJECT) out.object = b->object;
    return out;
}

int aov_device(rt_ctx* c, const rt_render_opts* o, uint32_t channels, const rt_aov_buffers* dev, void* stream) {
    if (const int rc = check_call(c, o, channels, dev); rc != RT_OK) return rc;
    return render_aov(c, o, selected(channels, dev), channels, stream);
}

// The host variant, the plain way: device buffers for the selected channels, the render on the context's
// stream, one copy per channel, free (host_staging.hpp).
int aov_host(rt_ctx* c, const rt_render_opts* o, uint32_t channels, const rt_aov_buffers* host, rt_stats* stats) {
    if (const int rc = check_call(c, o, channels, host); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t npix = static_cast<uint64_t>(o->tile_w) * o->tile_h;
    // (an empty tile has no buffers: the render checks the geometry and launches nothing)
    size_t bytes[5];
    for (int i = 0; i < 5; ++i) bytes[i] = (channels >> i) & 1u ? npix * kElems[i] * 4 : 0;
    const void* const in[5] = {};
    void* const dst[5] = {host->depth, host->normal, host->albedo, host->coverage, host->object};
    const StagedTexts texts{"rt_render_aov", "rt_render_aov: copy to the host", "rt_render_aov: synchronize"};
    const int rc = run_staged(c, bytes, in, dst, texts, [&](const Staged<5>& s) {
        const AovOut out{s.as<float>(0), s.as<float>(1), s.as<float>(2), s.as<float>(3), s.as<int32_t>(4)};
        return render_aov(c, o, out, channels, nullptr);
    });
    if (rc != RT_OK) return rc;
    if (stats) return rt_ctx_stats(c, stats);
    return check_join_error(c);
}

}  // namespace

extern "C" {

int rt_render_aov(rt_ctx* c, const rt_render_opts* o, uint32_t channels, const rt_aov_buffers* host, rt_stats* stats) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return aov_host(c, o, channels, host, stats); });
}

int rt_render_aov_device(rt_ctx* c, const rt_render_opts* o, uint32_t channels, const rt_aov_buffers* dev, void* stream) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return aov_device(c, o, channels, dev, stream); });
}

}  // extern "C"
