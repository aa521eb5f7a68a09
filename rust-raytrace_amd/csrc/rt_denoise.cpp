// C ABI: the denoiser (include/raytrace_amd.h, "denoiser").  Here are the argument checks of rt_denoise /
// rt_denoise_device (render_plan.hpp, plan_denoise_args), the context's scratch, the passes the planner lists
// (plan_denoise; the kernels are wf_denoise.hip's) and the host variant's plain allocate / copy / run / copy / free.
// rt_denoise_var / rt_denoise_var_device (the variance-guided filter) are the same body with an rt_denoise_variance
// beside the other structs: plan_denoise_var_args, the same scratch and event, the kernels' kVar forms.
// A denoise is not a render: it needs no scene and touches neither the counters nor the last render's statistics.
#include <cstdio>

#include "host_staging.hpp"
#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

// var_call: rt_denoise_var's checks (var may then be null: refused in its turn).
int check_call(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* in, bool var_call, const rt_denoise_variance* var,
               const void* out_rgb, const void* out_bgr) {
    const char* why = nullptr;
    const int rc = var_call ? plan_denoise_var_args(p, in, var, out_rgb, out_bgr, &why) : plan_denoise_args(p, in, out_rgb, out_bgr, &why);
    return rc != RT_OK ? fail(c, rc, why) : RT_OK;
}

// The scratch of a w x h call, kept for the next one.  It is freed (to grow) only once the denoise that last used it
// has finished.
int ensure_scratch(rt_ctx* c, const DenoisePlan& d, const char* who, const char* no_room) {
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
        return e == hipErrorOutOfMemory ? fail(c, RT_E_NOMEM, no_room) : hip_fail(c, e, who);
    }
    c->dn_cap = d.scratch_bytes;
    return RT_OK;
}

int denoise_device(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* in, bool var_call, const rt_denoise_variance* var,
                   float* out_rgb, uint8_t* out_bgr, void* stream) {
    if (const int rc = check_call(c, p, in, var_call, var, out_rgb, out_bgr); rc != RT_OK) return rc;
    // (the kernels index pixels with int coordinates; an image beyond that has no scratch either way)
    const char* who = var_call ? "rt_denoise_var" : "rt_denoise";
    const char* no_room = var_call ? "rt_denoise_var: the scratch images do not fit" : "rt_denoise: the scratch images do not fit";
    if (p->width > (1u << 30) || p->height > (1u << 30)) return fail(c, RT_E_NOMEM, no_room);
    HIP_TRY(c, hipSetDevice(c->device));
    const DenoisePlan d = plan_denoise(*p);
    if (const int rc = ensure_scratch(c, d, who, no_room); rc != RT_OK) return rc;
    const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (c->dn_pending) HIP_TRY(c, hipStreamWaitEvent(st, c->dn_done, 0));
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: denoise%s %ux%u iters %u flags 0x%x variant %u\n", var_call ? "-var" : "", p->width, p->height,
                     p->iterations, p->flags, d.variant);
    unsigned char* base = static_cast<unsigned char*>(c->d_dn);
    DnRec* img[2] = {reinterpret_cast<DnRec*>(base), reinterpret_cast<DnRec*>(base + d.image_bytes)};
    DnRec* guide = reinterpret_cast<DnRec*>(base + 2 * d.image_bytes);
    const DnFilter f{p->width, p->height, p->flags, p->normal_squarings, p->sigma_color, p->sigma_depth};
    const bool by_n = p->flags & RT_DN_NORMAL, by_z = p->flags & RT_DN_DEPTH, demod = p->flags & RT_DN_DEMODULATE;
    const float* albedo = demod ? in->albedo : nullptr;
    const DnVar dv = var_call ? DnVar{var->sigma_variance, var->variance_floor, var->out_variance} : DnVar{};
    const DnVar* pv = var_call ? &dv : nullptr;
    HIP_TRY(c, launch_denoise_pack(f, in->rgb, by_n ? in->normal : nullptr, by_z ? in->depth : nullptr, albedo, img[0], guide, st,
                                   var_call ? var->variance : nullptr));
    const uint32_t pitch = p->bgr_pitch ? p->bgr_pitch : 3 * p->width;
    for (uint32_t i = 0; i < d.passes; ++i) {
        const DnRec* src = img[i & 1u];
        if (i + 1 < d.passes) HIP_TRY(c, launch_denoise_pass(f, d.step[i], d.lds[i], src, guide, img[(i + 1) & 1u], d.grid_x, d.grid_y, st, pv));
        else HIP_TRY(c, launch_denoise_last(f, d.step[i], d.lds[i], src, guide, albedo, out_rgb, out_bgr, pitch, d.grid_x, d.grid_y, st, pv));
    }
    HIP_TRY(c, hipEventRecord(c->dn_done, st));
    c->dn_pending = true;
    return RT_OK;
}

// The host variant, the plain way: device buffers for the inputs the flags select and for the outputs asked for, the
// filter on the context's stream, the copies back, free.  The BGR rows go through a tight device image, so that the
// caller's padding bytes are never written: that copy is pitched, and follows the filter here (host_staging.hpp has
// the rest).
// rt_denoise_var stages two more: the variance image in, the filtered variance out (rt_denoise leaves the two slots
// empty: no allocation, no copy).
int denoise_host(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* host, bool var_call, const rt_denoise_variance* var,
                 float* out_rgb, uint8_t* out_bgr) {
    if (const int rc = check_call(c, p, host, var_call, var, out_rgb, out_bgr); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = static_cast<size_t>(p->width) * p->height, row = 3 * static_cast<size_t>(p->width);
    float* const out_var = var_call ? var->out_variance : nullptr;
    const size_t bytes[8] = {npix * 12, p->flags & RT_DN_NORMAL ? npix * 12 : 0, p->flags & RT_DN_DEPTH ? npix * 4 : 0,
                             p->flags & RT_DN_DEMODULATE ? npix * 12 : 0, out_rgb ? npix * 12 : 0, out_bgr ? npix * 3 : 0,
                             var_call ? npix * 12 : 0, out_var ? npix * 4 : 0};
    const void* const in[8] = {host->rgb, host->normal, host->depth, host->albedo, nullptr, nullptr,
                               var_call ? var->variance : nullptr, nullptr};
    void* const out[8] = {nullptr, nullptr, nullptr, nullptr, out_rgb, nullptr, nullptr, out_var};
    const StagedTexts texts = var_call ? StagedTexts{"rt_denoise_var", "rt_denoise_var: copy", "rt_denoise_var: synchronize"}
                                       : StagedTexts{"rt_denoise", "rt_denoise: copy", "rt_denoise: synchronize"};
    return run_staged(c, bytes, in, out, texts, [&](const Staged<8>& s) -> int {
        rt_denoise_params q = *p;
        q.bgr_pitch = 0;
        const rt_denoise_inputs dev{s.as<const float>(0), s.as<const float>(1), s.as<const float>(2), s.as<const float>(3)};
        rt_denoise_variance dvar{};
        if (var_call) dvar = rt_denoise_variance{s.as<const float>(6), s.as<float>(7), var->sigma_variance, var->variance_floor};
        if (const int rc = denoise_device(c, &q, &dev, var_call, &dvar, s.as<float>(4), s.as<uint8_t>(5), nullptr); rc != RT_OK) return rc;
        if (!s.d[5]) return RT_OK;
        const hipError_t e = hipMemcpy2DAsync(out_bgr, p->bgr_pitch ? p->bgr_pitch : row, s.d[5], row, row, p->height,
                                              hipMemcpyDeviceToHost, c->stream);
        return e == hipSuccess ? RT_OK : hip_fail(c, e, texts.copy);
    });
}

}  // namespace

extern "C" {

int rt_denoise(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* host, float* out_rgb, uint8_t* out_bgr) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return denoise_host(c, p, host, false, nullptr, out_rgb, out_bgr); });
}

int rt_denoise_device(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* dev, float* d_out_rgb, uint8_t* d_out_bgr,
                      void* stream) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return denoise_device(c, p, dev, false, nullptr, d_out_rgb, d_out_bgr, stream); });
}

int rt_denoise_var(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* host, const rt_denoise_variance* host_var,
                   float* out_rgb, uint8_t* out_bgr) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return denoise_host(c, p, host, true, host_var, out_rgb, out_bgr); });
}

int rt_denoise_var_device(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_inputs* dev, const rt_denoise_variance* dev_var,
                          float* d_out_rgb, uint8_t* d_out_bgr, void* stream) {
    if (!c) return RT_E_INVALID;
    return guarded(c, [&] { return denoise_device(c, p, dev, true, dev_var, d_out_rgb, d_out_bgr, stream); });
}

}  // extern "C"
