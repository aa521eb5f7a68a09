// C ABI: progressive rendering (include/raytrace_amd.h, "progressive rendering").  An rt_accum is the
// f64 running sum of every pixel of one tile, kept on the device between rt_render_accumulate calls
// (main.rs:47-56 split over calls); here are its creation and binding, the argument checks of the
// accumulate call (the render itself is rt_render.cpp's, render_accumulate), the resolves, and
// download / upload.  The checkpoint file is host_checkpoint.cpp's.
#include <algorithm>
#include <cstdio>

#include "host_staging.hpp"
#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

// The calls that touch the sums: a live context that is the accumulator's own, and the scene it is bound to.
int usable(rt_ctx* c, rt_accum* a, const char* what) {
    if (!a->ctx) return fail(c, RT_E_INVALID, std::string(what) + ": the accumulator's context was destroyed");
    if (a->ctx != c) return fail(c, RT_E_INVALID, std::string(what) + ": the accumulator belongs to another context");
    if (!c->has_scene) return fail(c, RT_E_NOSCENE, "no scene uploaded");
    if (a->scene_gen != c->scene_gen)
        return fail(c, RT_E_INVALID, std::string(what) + ": another scene was uploaded since the accumulator was bound (rt_accum_reset)");
    return RT_OK;
}

// Stream st is about to touch the sums: after the context's pending render (which may write them) and, for a
// writer, after a pending device resolve (which reads them on some caller's stream).
int order_on(rt_ctx* c, rt_accum* a, hipStream_t st, bool writer) {
    if (c->render_pending && st != c->done_stream) HIP_TRY(c, hipStreamWaitEvent(st, c->render_done, 0));
    if (writer && a->read_pending) {
        HIP_TRY(c, hipStreamWaitEvent(st, a->read_done, 0));
        a->read_pending = false;
    }
    return RT_OK;
}

// The resolve kernel over the whole tile on st.  pad_end: bytes of a BGR row written (pixels, then zeros).
int launch_resolve(rt_ctx* c, rt_accum* a, uint32_t pitch, uint32_t pad_end, float* d_rgb, uint8_t* d_bgr, hipStream_t st) {
    FrameParams fp{};
    fp.tile_w = a->o.tile_w; fp.tile_h = a->o.tile_h;
    fp.row0 = 0; fp.rows = a->o.tile_h;
    fp.bgr_pitch = pitch;
    fp.pad_end = pad_end;
    fp.out_rgb = d_rgb;
    fp.out_bgr = d_bgr;
    fp.aa_acc = a->d_sums;
    fp.aa_spp = a->samples;
    LaunchMarks m;
    m.pool = &c->tev; m.used = &c->t_used; m.out = &c->tint;
    if (a->timed) HIP_TRY(c, m.begin(st));
    HIP_TRY(c, launch_accum_resolve(fp, 4u * static_cast<uint32_t>(c->n_cu), st));
    if (a->timed) HIP_TRY(c, m.mark(st, kKfCompose));
    return RT_OK;
}

int check_pitch(rt_ctx* c, const rt_accum* a, uint32_t bgr_pitch, uint32_t& pitch) {
    pitch = bgr_pitch ? bgr_pitch : 3 * a->o.tile_w;
    if (pitch < 3 * a->o.tile_w) return fail(c, RT_E_INVALID, "bgr_pitch < 3*tile_w");
    if (a->samples == 0) return fail(c, RT_E_INVALID, "the accumulator holds no samples");
    return RT_OK;
}

int accum_create(rt_ctx* c, const rt_render_opts* o, bool moments, rt_accum** out) {
    if (!c->has_scene) return fail(c, RT_E_NOSCENE, "no scene uploaded");
    // the options' own checks, as a render makes them (render_accumulate with no samples renders nothing)
    rt_render_opts b = *o;
    b.spp = 1; b.flags = 0; b.algo = RT_ALGO_AUTO; b.bgr_pitch = 0; b._pad = 0;
    if (const int rc = render_accumulate(c, &b, nullptr, 0, 0, nullptr); rc != RT_OK) return rc;
    b.spp = 0;
    b.band = b.band ? b.band : 1;
    b.band_stride = b.band_stride ? b.band_stride : 1;
    HIP_TRY(c, hipSetDevice(c->device));
    rt_accum* a = new rt_accum;
    a->ctx = c;
    a->o = b;
    a->scene_gen = c->scene_gen;
    a->npix = static_cast<uint64_t>(o->tile_w) * o->tile_h;
    a->moments = moments;
    // the sums and, with moments, the plane of the sums of squares after them: one allocation, made here, so
    // that a reserved accumulate allocates nothing
    uint64_t doubles = 0;
    if (!plan_accum_doubles(a->npix, moments, &doubles)) {      // (two 32-bit sides can pass 2^64 / 48)
        delete a;
        return fail(c, RT_E_NOMEM, "the accumulator's sums do not fit");
    }
    hipError_t e = hipEventCreateWithFlags(&a->read_done, hipEventDisableTiming);
    if (e == hipSuccess && a->npix) e = hipMalloc(reinterpret_cast<void**>(&a->d_sums), doubles * sizeof(double));
    if (e == hipSuccess && moments) e = hipMalloc(reinterpret_cast<void**>(&a->d_above), sizeof(unsigned long long));
    if (e == hipSuccess && moments) e = hipHostMalloc(reinterpret_cast<void**>(&a->h_above), sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
        if (a->d_sums) (void)hipFree(a->d_sums);
        if (a->d_above) (void)hipFree(a->d_above);
        if (a->read_done) (void)hipEventDestroy(a->read_done);
        delete a;
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? fail(c, RT_E_NOMEM, "the accumulator's sums do not fit") : hip_fail(c, e, "rt_accum_create");
    }
    c->accums.push_back(a);
    *out = a;
    return RT_OK;
}

int accumulate(rt_ctx* c, rt_accum* a, uint32_t n, int32_t algo, uint32_t flags, void* stream) {
    if (const int rc = usable(c, a, "rt_render_accumulate"); rc != RT_OK) return rc;
    rt_render_opts o = a->o;
    o.spp = 1;                      // (not read: the call's samples are n)
    o.algo = algo;
    o.flags = flags;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (n && a->read_pending) {
        HIP_TRY(c, hipStreamWaitEvent(st, a->read_done, 0));
        a->read_pending = false;
    }
    if (const int rc = render_accumulate(c, &o, a->d_sums, a->samples, n, stream, a->moments); rc != RT_OK) return rc;
    if (n) {
        a->samples += n;
        a->timed = (flags & RT_TIME_KERNELS) != 0;
    }
    return RT_OK;
}

int resolve_device(rt_ctx* c, rt_accum* a, uint32_t bgr_pitch, void* d_rgb, void* d_bgr, void* stream) {
    if (const int rc = usable(c, a, "rt_accum_resolve"); rc != RT_OK) return rc;
    uint32_t pitch;
    if (const int rc = check_pitch(c, a, bgr_pitch, pitch); rc != RT_OK) return rc;
    if (a->npix == 0 || (!d_rgb && !d_bgr)) return RT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (const int rc = order_on(c, a, st, false); rc != RT_OK) return rc;
    if (const int rc = launch_resolve(c, a, pitch, 3 * a->o.tile_w, static_cast<float*>(d_rgb), static_cast<uint8_t*>(d_bgr), st);
        rc != RT_OK)
        return rc;
    HIP_TRY(c, hipEventRecord(a->read_done, st));
    a->read_pending = true;
    return RT_OK;
}

int resolve_host(rt_ctx* c, rt_accum* a, uint32_t bgr_pitch, float* out_rgb, uint8_t* out_bgr) {
    if (const int rc = usable(c, a, "rt_accum_resolve_host"); rc != RT_OK) return rc;
    uint32_t pitch;
    if (const int rc = check_pitch(c, a, bgr_pitch, pitch); rc != RT_OK) return rc;
    if (a->npix == 0 || (!out_rgb && !out_bgr)) return RT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rgb_bytes = out_rgb ? a->npix * 3 * sizeof(float) : 0;
    const size_t bgr_bytes = out_bgr ? static_cast<size_t>(pitch) * a->o.tile_h : 0;
    // the context's device frame (rt_render's): its earlier copies are done when rt_render returns
    if (const int rc = ensure_host_frame(c, rgb_bytes, bgr_bytes); rc != RT_OK) return rc;
    if (const int rc = order_on(c, a, c->stream, false); rc != RT_OK) return rc;
    // the frame's rows are copied whole: their padding is written as zero (main.rs:42)
    if (const int rc = launch_resolve(c, a, pitch, pitch, out_rgb ? c->d_rgb : nullptr, out_bgr ? c->d_bgr : nullptr, c->stream);
        rc != RT_OK)
        return rc;
    if (out_rgb) HIP_TRY(c, hipMemcpyAsync(out_rgb, c->d_rgb, rgb_bytes, hipMemcpyDeviceToHost, c->stream));
    if (out_bgr) HIP_TRY(c, hipMemcpyAsync(out_bgr, c->d_bgr, bgr_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return check_join_error(c);
}

int download(rt_ctx* c, rt_accum* a, double* sums, size_t cap, uint32_t* samples) {
    if (const int rc = usable(c, a, "rt_accum_download"); rc != RT_OK) return rc;
    if (cap < 3 * a->npix || (!sums && a->npix)) return fail(c, RT_E_INVALID, "rt_accum_download: fewer than 3 * tile_w * tile_h doubles");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = order_on(c, a, c->stream, false); rc != RT_OK) return rc;
    if (a->npix && a->samples)
        HIP_TRY(c, hipMemcpyAsync(sums, a->d_sums, a->npix * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // no samples: the device memory holds nothing defined; the sums of no samples are BLACK (main.rs:47)
    if (a->samples == 0) std::fill(sums, sums + 3 * a->npix, 0.0);
    if (samples) *samples = a->samples;
    return check_join_error(c);
}

int upload(rt_ctx* c, rt_accum* a, const double* sums, size_t n, uint32_t samples) {
    if (const int rc = usable(c, a, "rt_accum_upload"); rc != RT_OK) return rc;
    const char* refusal = nullptr;
    if (const int rc = plan_accum_call(AccumCall::upload, a->moments, &refusal); rc != RT_OK) return fail(c, rc, refusal);
    if (n != 3 * a->npix || (!sums && n)) return fail(c, RT_E_INVALID, "rt_accum_upload: not 3 * tile_w * tile_h doubles");
    if (samples > kAccumMaxSamples) return fail(c, RT_E_INVALID, "rt_accum_upload: samples above 2^31");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = order_on(c, a, c->stream, true); rc != RT_OK) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(a->d_sums, sums, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    a->samples = samples;
    // later renders on other streams are ordered after this copy: it has completed
    return RT_OK;
}

// rt_accum_download_moments: the squares' plane (of no samples: zeros, as the sums').
int download_moments(rt_ctx* c, rt_accum* a, double* squares, size_t cap) {
    if (const int rc = usable(c, a, "rt_accum_download_moments"); rc != RT_OK) return rc;
    const char* refusal = nullptr;
    if (const int rc = plan_accum_call(AccumCall::download_moments, a->moments, &refusal); rc != RT_OK) return fail(c, rc, refusal);
    if (cap < 3 * a->npix || (!squares && a->npix))
        return fail(c, RT_E_INVALID, "rt_accum_download_moments: fewer than 3 * tile_w * tile_h doubles");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = order_on(c, a, c->stream, false); rc != RT_OK) return rc;
    if (a->npix && a->samples)
        HIP_TRY(c, hipMemcpyAsync(squares, a->d_sums + 3 * a->npix, a->npix * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a->samples == 0) std::fill(squares, squares + 3 * a->npix, 0.0);
    return check_join_error(c);
}

// rt_accum_upload_moments: sums, squares and count together, so neither plane is ever stale.
int upload_moments(rt_ctx* c, rt_accum* a, const double* sums, const double* squares, size_t n, uint32_t samples) {
    if (const int rc = usable(c, a, "rt_accum_upload_moments"); rc != RT_OK) return rc;
    const char* refusal = nullptr;
    if (const int rc = plan_accum_call(AccumCall::upload_moments, a->moments, &refusal); rc != RT_OK) return fail(c, rc, refusal);
    if (n != 3 * a->npix || ((!sums || !squares) && n))
        return fail(c, RT_E_INVALID, "rt_accum_upload_moments: not 3 * tile_w * tile_h doubles of each");
    if (samples > kAccumMaxSamples) return fail(c, RT_E_INVALID, "rt_accum_upload_moments: samples above 2^31");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = order_on(c, a, c->stream, true); rc != RT_OK) return rc;
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(a->d_sums, sums, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(a->d_sums + n, squares, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    a->samples = samples;
    return RT_OK;
}

// The checks of both noise calls; nothing has changed when one refuses.
int check_noise(rt_ctx* c, rt_accum* a, double floor, double threshold, const char* what) {
    if (const int rc = usable(c, a, what); rc != RT_OK) return rc;
    const char* refusal = nullptr;
    if (const int rc = plan_noise(a->moments, a->samples, floor, threshold, &refusal); rc != RT_OK)
        return fail(c, rc, std::string(what) + ": " + refusal);
    return RT_OK;
}

// accum_noise over the whole tile on st, ordered as a resolve is (a reader of the sums); the count comes back
// once st has run it.
int noise_device(rt_ctx* c, rt_accum* a, double floor, double threshold, float* d_var, float* d_err, uint64_t* above, hipStream_t st) {
    if (a->npix == 0) {
        *above = 0;
        return RT_OK;
    }
    if (const int rc = order_on(c, a, st, false); rc != RT_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(a->d_above, 0, sizeof(unsigned long long), st));
    FrameParams fp{};
    fp.tile_w = a->o.tile_w; fp.tile_h = a->o.tile_h;
    fp.row0 = 0; fp.rows = a->o.tile_h;
    fp.aa_acc = a->d_sums;
    fp.aa_spp = a->samples;
    LaunchMarks m;
    m.pool = &c->tev; m.used = &c->t_used; m.out = &c->tint;
    if (a->timed) HIP_TRY(c, m.begin(st));
    HIP_TRY(c, launch_accum_noise(fp, 4u * static_cast<uint32_t>(c->n_cu), floor, threshold, d_var, d_err, a->d_above, st));
    if (a->timed) HIP_TRY(c, m.mark(st, kKfCompose));
    // the count lands in the accumulator's own page-locked word: nothing queued points into this frame
    HIP_TRY(c, hipMemcpyAsync(a->h_above, a->d_above, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(a->read_done, st));
    a->read_pending = true;
    HIP_TRY(c, hipStreamSynchronize(st));
    *above = *a->h_above;
    return RT_OK;
}

int noise(rt_ctx* c, rt_accum* a, double floor, double threshold, void* d_var, void* d_err, uint64_t* above, void* stream) {
    if (const int rc = check_noise(c, a, floor, threshold, "rt_accum_noise"); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return noise_device(c, a, floor, threshold, static_cast<float*>(d_var), static_cast<float*>(d_err), above, st);
}

int noise_host(rt_ctx* c, rt_accum* a, double floor, double threshold, float* variance, float* error, uint64_t* above) {
    if (const int rc = check_noise(c, a, floor, threshold, "rt_accum_noise_host"); rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes[2] = {variance ? a->npix * 3 * sizeof(float) : 0, error ? a->npix * sizeof(float) : 0};
    const void* const in[2] = {nullptr, nullptr};
    void* const out[2] = {variance, error};
    uint64_t n = 0;
    const StagedTexts texts{"rt_accum_noise_host", "rt_accum_noise_host: copy", "rt_accum_noise_host: synchronise"};
    const int rc = run_staged<2>(c, bytes, in, out, texts, [&](const Staged<2>& s) {
        return noise_device(c, a, floor, threshold, s.as<float>(0), s.as<float>(1), &n, c->stream);
    });
    if (rc != RT_OK) return rc;
    *above = n;
    return check_join_error(c);
}

// The accumulator's device resources, once nothing on the device uses them.
void release(rt_accum* a) {
    rt_ctx* c = a->ctx;
    (void)hipSetDevice(c->device);
    if (c->render_pending) (void)hipEventSynchronize(c->render_done);
    if (a->read_pending) (void)hipEventSynchronize(a->read_done);
    if (a->d_sums) (void)hipFree(a->d_sums);
    if (a->d_above) (void)hipFree(a->d_above);
    if (a->h_above) (void)hipHostFree(a->h_above);
    if (a->read_done) (void)hipEventDestroy(a->read_done);
    a->d_sums = nullptr;
    a->d_above = nullptr;
    a->h_above = nullptr;
    a->read_done = nullptr;
    a->read_pending = false;
    a->ctx = nullptr;
}

}  // namespace

namespace rtamd {

void orphan_accums(rt_ctx* c) {
    for (rt_accum* a : c->accums) release(a);
    c->accums.clear();
}

}  // namespace rtamd

extern "C" {

int rt_accum_create(rt_ctx* c, const rt_render_opts* o, rt_accum** out) {
    if (!c || !o || !out) return RT_E_INVALID;
    *out = nullptr;
    return guarded(c, [&] { return accum_create(c, o, false, out); });
}

int rt_accum_create_moments(rt_ctx* c, const rt_render_opts* o, rt_accum** out) {
    if (!c || !o || !out) return RT_E_INVALID;
    *out = nullptr;
    return guarded(c, [&] { return accum_create(c, o, true, out); });
}

int rt_accum_has_moments(const rt_accum* a, int32_t* flag) {
    if (!a || !flag) return RT_E_INVALID;
    *flag = a->moments ? 1 : 0;
    return RT_OK;
}

void rt_accum_destroy(rt_accum* a) {
    if (!a) return;
    if (rt_ctx* c = a->ctx) {
        c->accums.erase(std::remove(c->accums.begin(), c->accums.end(), a), c->accums.end());
        release(a);
    }
    delete a;
}

int rt_accum_samples(const rt_accum* a, uint32_t* samples) {
    if (!a || !samples) return RT_E_INVALID;
    *samples = a->samples;
    return RT_OK;
}

int rt_accum_reset(rt_accum* a) {
    if (!a) return RT_E_INVALID;
    if (!a->ctx) return fail(nullptr, RT_E_INVALID, "rt_accum_reset: the accumulator's context was destroyed");
    if (!a->ctx->has_scene) return fail(a->ctx, RT_E_NOSCENE, "no scene uploaded");
    a->samples = 0;
    a->scene_gen = a->ctx->scene_gen;
    return RT_OK;
}

int rt_render_accumulate(rt_ctx* c, rt_accum* a, uint32_t n, int32_t algo, uint32_t flags, void* stream) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return accumulate(c, a, n, algo, flags, stream); });
}

int rt_accum_resolve(rt_ctx* c, rt_accum* a, uint32_t bgr_pitch, void* d_rgb, void* d_bgr, void* stream) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return resolve_device(c, a, bgr_pitch, d_rgb, d_bgr, stream); });
}

int rt_accum_resolve_host(rt_ctx* c, rt_accum* a, uint32_t bgr_pitch, float* out_rgb, uint8_t* out_bgr) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return resolve_host(c, a, bgr_pitch, out_rgb, out_bgr); });
}

int rt_accum_download(rt_ctx* c, rt_accum* a, double* sums, size_t cap_doubles, uint32_t* samples) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return download(c, a, sums, cap_doubles, samples); });
}

int rt_accum_upload(rt_ctx* c, rt_accum* a, const double* sums, size_t n_doubles, uint32_t samples) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return upload(c, a, sums, n_doubles, samples); });
}

int rt_accum_download_moments(rt_ctx* c, rt_accum* a, double* squares, size_t cap_doubles) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return download_moments(c, a, squares, cap_doubles); });
}

int rt_accum_upload_moments(rt_ctx* c, rt_accum* a, const double* sums, const double* squares, size_t n_doubles, uint32_t samples) {
    if (!c || !a) return RT_E_INVALID;
    return guarded(c, [&] { return upload_moments(c, a, sums, squares, n_doubles, samples); });
}

int rt_accum_noise(rt_ctx* c, rt_accum* a, double floor, double threshold, void* d_variance, void* d_error, uint64_t* above,
                   void* stream) {
    if (!c || !a || !above) return RT_E_INVALID;
    return guarded(c, [&] { return noise(c, a, floor, threshold, d_variance, d_error, above, stream); });
}

int rt_accum_noise_host(rt_ctx* c, rt_accum* a, double floor, double threshold, float* variance, float* error, uint64_t* above) {
    if (!c || !a || !above) return RT_E_INVALID;
    return guarded(c, [&] { return noise_host(c, a, floor, threshold, variance, error, above); });
}

}  // extern "C"
