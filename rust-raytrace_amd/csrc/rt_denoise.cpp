// C ABI: the denoiser (include/raytrace_amd.h, "denoiser").  Here are the argument checks of rt_denoise /
// rt_denoise_device (render_plan.hpp, plan_denoise_args), the context's scratch, the passes the planner lists
// (plan_denoise; the kernels are wf_denoise.hip's) and the host variant's plain allocate / copy / run / copy / free.
// A denoise is not a render: it needs no scene and touches neither the counters nor the last render's statistics.
#include <cstdio>

#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

int check_call(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* in, const void* out_rgb, const void* out_bgr) {
    const char* why = nullptr;
    if (const int rc = plan_denoise_args(p, in, out_rgb, out_bgr, &why); rc != RT_OK) return fail(c, rc, why);
    return RT_OK;
}

// The scratch of a w x h call, kept for the next one.  It is freed (to grow) only once the denoise that last used it
// has finished.
int ensure_scratch(rt_ctx* c, const DenoisePlan& d) {
    if (!c->dn_done) HIP_TRY(c, hipEventCreateWithFlags(&c->dn_done, hipEventDisableTiming));
    if (d.scratch_bytes <= c->dn_cap) return RT_OK;
    if (c->dn_pending) HIP_TRY(c, hipEventSynchronize(c->dn_done));
    c->dn_pending = false;
    if (c->d_dn) (void)hipFree(c->d_dn);
    c->d_dn = nullptr;
    c->dn_cap = 0;
    const hipError_t e = hipMalloc(&c->d_dn, d.scratch_bytes);
    if (e != hipSuccess) {
        c->d_dn = nullptr;
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? fail(c, RT_E_NOMEM, "rt_denoise: the scratch images do not fit") : hip_fail(c, e, "rt_denoise");
    }
    c->dn_cap = d.scratch_bytes;
    return RT_OK;
}

int denoise_device(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* in, float* out_rgb, uint8_t* out_bgr,
                   void* stream) {
    if (const int rc = check_call(c, p, in, out_rgb, out_bgr); rc != RT_OK) return rc;
    // (the kernels index pixels with int coordinates; an image beyond that has no scratch either way)
    if (p->width > (1u << 30) || p->height > (1u << 30)) return fail(c, RT_E_NOMEM, "rt_denoise: the scratch images do not fit");
    HIP_TRY(c, hipSetDevice(c->device));
    const DenoisePlan d = plan_denoise(*p);
    if (const int rc = ensure_scratch(c, d); rc != RT_OK) return rc;
    const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (c->dn_pending) HIP_TRY(c, hipStreamWaitEvent(st, c->dn_done, 0));
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: denoise %ux%u iters %u flags 0x%x variant %u\n", p->width, p->height, p->iterations, p->flags,
                     d.variant);
    unsigned char* base = static_cast<unsigned char*>(c->d_dn);
    DnRec* img[2] = {reinterpret_cast<DnRec*>(base), reinterpret_cast<DnRec*>(base + d.image_bytes)};
    DnRec* guide = reinterpret_cast<DnRec*>(base + 2 * d.image_bytes);
    const DnFilter f{p->width, p->height, p->flags, p->normal_squarings, p->sigma_color, p->sigma_depth};
    const bool by_n = p->flags & RT_DN_NORMAL, by_z = p->flags & RT_DN_DEPTH, demod = p->flags & RT_DN_DEMODULATE;
    const float* albedo = demod ? in->albedo : nullptr;
    HIP_TRY(c, launch_denoise_pack(f, in->rgb, by_n ? in->normal : nullptr, by_z ? in->depth : nullptr, albedo, img[0], guide, st));
    const uint32_t pitch = p->bgr_pitch ? p->bgr_pitch : 3 * p->width;
    for (uint32_t i = 0; i < d.passes; ++i) {
        const DnRec* src = img[i & 1u];
        if (i + 1 < d.passes) HIP_TRY(c, launch_denoise_pass(f, d.step[i], d.lds[i], src, guide, img[(i + 1) & 1u], d.grid_x, d.grid_y, st));
        else HIP_TRY(c, launch_denoise_last(f, d.step[i], d.lds[i], src, guide, albedo, out_rgb, out_bgr, pitch, d.grid_x, d.grid_y, st));
    }
    HIP_TRY(c, hipEventRecord(c->dn_done, st));
    c->dn_pending = true;
    return RT_OK;
}

// The host variant, the plain way: device buffers for the inputs the flags select and for the outputs asked for, the
// filter on the context's stream, the copies back, free.  The BGR rows go through a tight device image, so that the
// caller's padding bytes are never written.  No performance claim.
int denoise_host(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* host, float* out_rgb, uint8_t* out_bgr) {
    if (const int rc = check_call(c, p, host, out_rgb, out_bgr); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = static_cast<size_t>(p->width) * p->height;
    const bool use[4] = {true, (p->flags & RT_DN_NORMAL) != 0, (p->flags & RT_DN_DEPTH) != 0, (p->flags & RT_DN_DEMODULATE) != 0};
    const float* const src[4] = {host->rgb, host->normal, host->depth, host->albedo};
    const size_t bytes[6] = {npix * 12, npix * 12, npix * 4, npix * 12, out_rgb ? npix * 12 : 0, out_bgr ? npix * 3 : 0};
    void* d[6] = {};
    auto release = [&] {
        for (void* q : d)
            if (q) (void)hipFree(q);
    };
    for (int i = 0; i < 6; ++i) {
        if ((i < 4 && !use[i]) || bytes[i] == 0) continue;
        const hipError_t e = hipMalloc(&d[i], bytes[i]);
        if (e != hipSuccess) {
            d[i] = nullptr;
            release();
            (void)hipGetLastError();
            return e == hipErrorOutOfMemory ? fail(c, RT_E_NOMEM, "rt_denoise: the device buffers do not fit") : hip_fail(c, e, "rt_denoise");
        }
    }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i)
        if (d[i]) e = hipMemcpyAsync(d[i], src[i], bytes[i], hipMemcpyHostToDevice, c->stream);
    int rc = RT_OK;
    if (e == hipSuccess) {
        rt_denoise_params q = *p;
        q.bgr_pitch = 0;
        const rt_denoise_inputs dev{static_cast<const float*>(d[0]), static_cast<const float*>(d[1]), static_cast<const float*>(d[2]),
                                    static_cast<const float*>(d[3])};
        rc = denoise_device(c, &q, &dev, static_cast<float*>(d[4]), static_cast<uint8_t*>(d[5]), nullptr);
    }
    if (rc == RT_OK && e == hipSuccess && d[4]) e = hipMemcpyAsync(out_rgb, d[4], bytes[4], hipMemcpyDeviceToHost, c->stream);
    if (rc == RT_OK && e == hipSuccess && d[5]) {
        const size_t pitch = p->bgr_pitch ? p->bgr_pitch : 3 * static_cast<size_t>(p->width);
        e = hipMemcpy2DAsync(out_bgr, pitch, d[5], 3 * static_cast<size_t>(p->width), 3 * static_cast<size_t>(p->width), p->height,
                             hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // also before the buffers are freed after a failure
    release();
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return hip_fail(c, e, "rt_denoise: copy");
    if (es != hipSuccess) return hip_fail(c, es, "rt_denoise: synchronize");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* host, float* out_rgb, uint8_t* out_bgr) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return denoise_host(c, p, host, out_rgb, out_bgr); });
}

int rt_denoise_device(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* dev, float* d_out_rgb, uint8_t* d_out_bgr,
                      void* stream) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return denoise_device(c, p, dev, d_out_rgb, d_out_bgr, stream); });
}

}  // extern "C"
