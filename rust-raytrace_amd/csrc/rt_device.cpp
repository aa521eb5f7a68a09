// C ABI: device contexts (create / destroy), their tuning keys and the arithmetic probes.
// See include/raytrace_amd.h for the contract and the reference interfaces these replace;
// rt_ctx.hpp names the files that hold the rest of the context's entry points.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

// Upload n records of `in_d` doubles (and `in_i` ints, 0: none), run `launch` on the device copies, download
// the records' `out_i` ints and `out_d` doubles.  One allocation, the doubles first (8-byte aligned).
template <class Launch>
int run_record_probe(rt_ctx* c, uint32_t n, const double* in_d, size_t n_in_d, const int32_t* in_i, size_t n_in_i,
                     int32_t* out_i, size_t n_out_i, double* out_d, size_t n_out_d, Launch&& launch) {
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t N = n;
    const size_t o_od = 8 * n_in_d * N, o_ii = o_od + 8 * n_out_d * N, o_oi = o_ii + 4 * n_in_i * N;
    uint8_t* d = nullptr;
    HIP_TRY(c, hipMalloc(&d, o_oi + 4 * n_out_i * N));
    auto body = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(d, in_d, o_od, hipMemcpyHostToDevice, c->stream));
        if (n_in_i) HIP_TRY(c, hipMemcpyAsync(d + o_ii, in_i, 4 * n_in_i * N, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch(reinterpret_cast<const double*>(d), reinterpret_cast<const int32_t*>(d + o_ii),
                          reinterpret_cast<int32_t*>(d + o_oi), reinterpret_cast<double*>(d + o_od)));
        HIP_TRY(c, hipMemcpyAsync(out_i, d + o_oi, 4 * n_out_i * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(out_d, d + o_od, 8 * n_out_d * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return RT_OK;
    };
    const int rc = body();
    (void)hipFree(d);
    return rc;
}

}  // namespace

extern "C" {

int rt_device_count(int* n) {
    if (!n) return RT_E_INVALID;
    *n = 0;
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) { *n = 0; return RT_OK; }
    *n = k;
    return RT_OK;
}

int rt_ctx_create(int device, rt_ctx** out) {
    if (!out) return RT_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(nullptr, RT_E_NODEVICE, "no HIP device " + std::to_string(device));
    auto* c = new (std::nothrow) rt_ctx();
    if (!c) return RT_E_NOMEM;
    c->device = device;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu < 1)
        c->n_cu = 256;
    auto cleanup = [&](int rc) { rt_ctx_destroy(c); return rc; };
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(nullptr, RT_E_HIP, "hipSetDevice failed"));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->render_done) != hipSuccess ||
        hipMalloc(&c->d_counters, kCounterWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->d_srgb, 255 * sizeof(double)) != hipSuccess ||
        hipMemcpy(c->d_srgb, srgb_average_table(), 255 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        upload_srgb_table(srgb_average_table()) != hipSuccess)
        return cleanup(fail(nullptr, RT_E_HIP, "context initialisation failed"));
    // the kernels' code objects load at their first launch: here, not in the first render
    if (warm_streams(c, {c->stream}) != RT_OK) return cleanup(fail(nullptr, RT_E_HIP, "context warm-up failed"));
    *out = c;
    return RT_OK;
}

void rt_ctx_destroy(rt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->render_pending) (void)hipEventSynchronize(c->render_done);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->tally.on = false;                   // nobody can read it any more: drop_lanes has nothing to settle
    orphan_accums(c);                      // accumulators still alive lose their sums; rt_accum_destroy stays valid
    if (c->d_blob) (void)hipFree(c->d_blob);
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->d_srgb) (void)hipFree(c->d_srgb);
    if (c->d_path) (void)hipFree(c->d_path);
    if (c->d_rgb) (void)hipFree(c->d_rgb);
    if (c->d_bgr) (void)hipFree(c->d_bgr);
    if (c->dn_pending) (void)hipEventSynchronize(c->dn_done);   // a denoise on a caller's stream still reads the scratch
    if (c->d_dn) (void)hipFree(c->d_dn);
    if (c->dn_done) (void)hipEventDestroy(c->dn_done);
    drop_lanes(c);
    for (hipEvent_t e : c->tev) (void)hipEventDestroy(e);
    if (c->render_done) (void)hipEventDestroy(c->render_done);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (int i = 0; i < kRing; ++i) {
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
        if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
    }
    for (hipEvent_t e : c->band_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->sp_ev) if (e) (void)hipEventDestroy(e);
    if (c->sp_cam) (void)hipEventDestroy(c->sp_cam);
    if (c->sp_ready) (void)hipEventDestroy(c->sp_ready);
    if (c->cp_done) (void)hipEventDestroy(c->cp_done);
    if (c->d_sp) (void)hipFree(c->d_sp);
    if (c->sdma_state == 1) {
        for (hsa_signal_t sg : c->sdma_sig)
            if (sg.handle) (void)hsa_signal_destroy(sg);
        (void)hsa_shut_down();             // balances sdma_setup's hsa_init
    }
    if (c->h_sp_meta) (void)hipHostFree(c->h_sp_meta);
    if (c->h_sp_pk) (void)hipHostFree(c->h_sp_pk);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->fork) (void)hipEventDestroy(c->fork);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* rt_last_error(const rt_ctx* c) { return c ? c->err.c_str() : thread_error(); }

int rt_div_a2_check(rt_ctx* c, const double* x, const double* a, uint32_t n, double* fast, double* slow) {
    if (!c || (n && (!x || !a || !fast || !slow))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return guarded(c, [&] {
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t bytes = static_cast<size_t>(n) * sizeof(double);
        double* d = nullptr;
        HIP_TRY(c, hipMalloc(&d, 4 * bytes));
        auto body = [&]() -> int {
            HIP_TRY(c, hipMemcpyAsync(d, x, bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d + n, a, bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, launch_div_a2_probe(d, d + n, n, d + 2 * static_cast<size_t>(n), d + 3 * static_cast<size_t>(n), c->stream));
            HIP_TRY(c, hipMemcpyAsync(fast, d + 2 * static_cast<size_t>(n), bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(slow, d + 3 * static_cast<size_t>(n), bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return RT_OK;
        };
        const int rc = body();
        (void)hipFree(d);
        return rc;
    });
}

int rt_cull_check(rt_ctx* c, uint32_t n, const double* rays, const float* boxes, const double* t, const int32_t* codes,
                  double reach, int32_t* out_i, float* out_f) {
    if (!c || (n && (!rays || !boxes || !t || !codes || !out_i || !out_f))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return guarded(c, [&] {
        HIP_TRY(c, hipSetDevice(c->device));
        // one allocation: [rays 48 n][t 8 n][boxes 24 n][codes 4 n][out_i 20 n][out_f 20 n]
        const size_t N = n;
        const size_t o_t = 48 * N, o_box = o_t + 8 * N, o_code = o_box + 24 * N, o_oi = o_code + 4 * N, o_of = o_oi + 20 * N;
        uint8_t* d = nullptr;
        HIP_TRY(c, hipMalloc(&d, o_of + 20 * N));
        auto body = [&]() -> int {
            HIP_TRY(c, hipMemcpyAsync(d, rays, 48 * N, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d + o_t, t, 8 * N, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d + o_box, boxes, 24 * N, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d + o_code, codes, 4 * N, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, launch_cull_probe(n, reinterpret_cast<const double*>(d), reinterpret_cast<const float*>(d + o_box),
                                         reinterpret_cast<const double*>(d + o_t), reinterpret_cast<const int32_t*>(d + o_code),
                                         static_cast<float>(reach), reinterpret_cast<int32_t*>(d + o_oi), reinterpret_cast<float*>(d + o_of),
                                         c->stream));
            HIP_TRY(c, hipMemcpyAsync(out_i, d + o_oi, 20 * N, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(out_f, d + o_of, 20 * N, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return RT_OK;
        };
        const int rc = body();
        (void)hipFree(d);
        return rc;
    });
}

int rt_isect_check(rt_ctx* c, uint32_t n, const double* records, int32_t* out_i, double* out_d) {
    if (!c || (n && (!records || !out_i || !out_d))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return guarded(c, [&] {
        // the device's sphere carries rr = radius * radius, formed as the upload forms it
        std::vector<double> in(records, records + 16 * static_cast<size_t>(n));
        for (size_t i = 0; i < n; ++i) in[16 * i + 9] = sphere_rr(in[16 * i + 9]);
        return run_record_probe(c, n, in.data(), 16, nullptr, 0, out_i, 3, out_d, 15,
                                [&](const double* di, const int32_t*, int32_t* oi, double* od) {
                                    return launch_isect_probe(n, di, oi, od, c->stream);
                                });
    });
}

int rt_shade_check(rt_ctx* c, uint32_t n, const double* records, const int32_t* kinds, int32_t* out_i, double* out_d) {
    if (!c || (n && (!records || !kinds || !out_i || !out_d))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return guarded(c, [&] {
        // 27 -> 29 doubles: the material's kd_sig and ks_sig (the upload's significance()) go in after ks
        std::vector<double> in(29 * static_cast<size_t>(n));
        for (size_t i = 0; i < n; ++i) {
            const double* q = records + 27 * i;
            double* o = in.data() + 29 * i;
            for (int k = 0; k < 15; ++k) o[k] = q[k];
            o[15] = significance(rt_color{q[9], q[10], q[11]});
            o[16] = significance(rt_color{q[12], q[13], q[14]});
            for (int k = 15; k < 27; ++k) o[k + 2] = q[k];
        }
        return run_record_probe(c, n, in.data(), 29, kinds, 2, out_i, 3, out_d, 20,
                                [&](const double* di, const int32_t* ii, int32_t* oi, double* od) {
                                    return launch_shade_probe(n, di, ii, oi, od, c->stream);
                                });
    });
}

int rt_sqrt_check(rt_ctx* c, const double* x, uint32_t n, double* fast, double* slow) {
    if (!c || (n && (!x || !fast || !slow))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return guarded(c, [&] {
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t bytes = static_cast<size_t>(n) * sizeof(double);
        double* d = nullptr;
        HIP_TRY(c, hipMalloc(&d, 3 * bytes));
        auto body = [&]() -> int {
            HIP_TRY(c, hipMemcpyAsync(d, x, bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, launch_sqrt_probe(d, n, d + n, d + 2 * static_cast<size_t>(n), c->stream));
            HIP_TRY(c, hipMemcpyAsync(fast, d + n, bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(slow, d + 2 * static_cast<size_t>(n), bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return RT_OK;
        };
        const int rc = body();
        (void)hipFree(d);
        return rc;
    });
}

int rt_ctx_set_tuning(rt_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return RT_E_INVALID;
    for (int i = 0; i < kTuneCount; ++i) {
        if (std::strcmp(key, kTune[i].name) != 0) continue;
        if (value < kTune[i].lo || value > kTune[i].hi)
            return fail(c, RT_E_INVALID, std::string("tuning ") + key + " out of range");
        // cu_mask and prio shape the lanes' streams, which are created once: rebuild
        // the lanes (after their work is done) so the next render uses the new value
        if ((i == kTuneCuMask || i == kTunePrio || i == kTuneAQueue) && value != c->tune[i] && !c->lanes.empty()) {
            if (hipSetDevice(c->device) != hipSuccess) return fail(c, RT_E_HIP, "hipSetDevice failed");
            if (c->render_pending) (void)hipEventSynchronize(c->render_done);
            drop_lanes(c);
        }
        c->tune[i] = value;
        return RT_OK;
    }
    return fail(c, RT_E_INVALID, std::string("unknown tuning key ") + key);
}

int rt_ctx_get_tuning(const rt_ctx* c, const char* key, int64_t* value) {
    if (!c || !key || !value) return RT_E_INVALID;
    for (int i = 0; i < kTuneCount; ++i)
        if (std::strcmp(key, kTune[i].name) == 0) { *value = c->tune[i]; return RT_OK; }
    return RT_E_INVALID;
}

const char* rt_tuning_key(int index) { return index >= 0 && index < kTuneCount ? kTune[index].name : nullptr; }

}  // extern "C"
