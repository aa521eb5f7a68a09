// The frame's two ends: pixel -> camera ray, colour -> output buffers, and the background
// (solid colour or skybox) of a ray that leaves the scene.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "trace_types.hpp"
#include "trace_rng.hpp"
#include "trace_prims.hpp"

namespace rtamd {

// Pixel -> camera ray (main.rs:50-53; camera.rs:78) of AA sample `sample`: the
// centre jitter, or the keyed draws of that sample (fp.jitter; the chain
// schedules trace sample 0, RT_ALGO_WAVEFRONT_AA sample fp.aa_pass per pass).
__device__ __forceinline__ Ray camera_ray(const DevScene& sc, const FrameParams& fp, uint32_t lx, uint32_t local_row,
                                          uint32_t sample) {
    const uint32_t x = fp.x0 + lx;
    const uint32_t y = fp.y0 + ((local_row / fp.band) * fp.band_stride + fp.band_phase) * fp.band + local_row % fp.band;
    double jx = 0.5, jy = 0.5;
    if (fp.jitter) {
        const uint64_t ka = key_child(key_pixel(fp.seed, x, y), sample);
        jx = key_f64(ka, 0);
        jy = key_f64(ka, 1);
    }
    const double px = ((static_cast<double>(x) + jx) - fp.hw) * fp.scale;
    const double py = ((static_cast<double>(y) + jy) - fp.hh) * fp.scale;
    const double* M = sc.cam_m;
    const double dx = M[0] * px + M[1] * py + M[2] * 1.0;
    const double dy = M[3] * px + M[4] * py + M[5] * 1.0;
    const double dz = M[6] * px + M[7] * py + M[8] * 1.0;
#if RT_DIVK
    const DivK l = div_k(sqrt_win(dx * dx + dy * dy + dz * dz));
    return Ray{sc.cam_pos[0], sc.cam_pos[1], sc.cam_pos[2], div_by(dx, l), div_by(dy, l), div_by(dz, l)};
#else
    const double l = sqrt(dx * dx + dy * dy + dz * dz);
    return Ray{sc.cam_pos[0], sc.cam_pos[1], sc.cam_pos[2], dx / l, dy / l, dz / l};
#endif
}

// Final colour of a pixel from its spp identical centre-jitter samples
// (raytrace.rs:271-275, main.rs:47-56): res = BLACK; res += (BLACK + c)/1 per
// sample; res / spp.
__device__ __forceinline__ Col average_samples(Col c, uint32_t spp) {
    c = Col{(0.0 + c.r) / 1.0, (0.0 + c.g) / 1.0, (0.0 + c.b) / 1.0};
    Col res{0.0, 0.0, 0.0};
    for (uint32_t k = 0; k < spp; ++k) res = Col{res.r + c.r, res.g + c.g, res.b + c.b};
    const double aa = static_cast<double>(spp);
    return Col{res.r / aa, res.g / aa, res.b / aa};
}

__device__ __forceinline__ void write_pixel(const FrameParams& fp, uint32_t lx, uint32_t out_row, Col res,
                                            const double* srgb = c_srgb_avg) {
    const size_t p = static_cast<size_t>(out_row) * fp.tile_w + lx;
    if (fp.out_rgb) {
        fp.out_rgb[3 * p + 0] = static_cast<float>(res.r);
        fp.out_rgb[3 * p + 1] = static_cast<float>(res.g);
        fp.out_rgb[3 * p + 2] = static_cast<float>(res.b);
    }
    if (fp.out_bgr) {
        uint8_t* q = fp.out_bgr + static_cast<size_t>(out_row) * fp.bgr_pitch + 3u * lx;
        q[0] = to_srgb(res.b, srgb);
        q[1] = to_srgb(res.g, srgb);
        q[2] = to_srgb(res.r, srgb);
        if (lx == fp.tile_w - 1)       // BMP row padding is zero (main.rs:42)
            for (uint32_t k = 3u * fp.tile_w; k < fp.pad_end; ++k)
                fp.out_bgr[static_cast<size_t>(out_row) * fp.bgr_pitch + k] = 0;
    }
}

// Texture::sample (texture.rs:46-58) of skybox face k: bilinear over
// Color::from_srgb texels (color.rs:611-613), coordinates clamped to [0, 1].
__device__ __forceinline__ double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }   // texture.rs:28-31

__device__ __forceinline__ Col texel(const DevScene& sc, const DevTexFace& f, uint32_t x, uint32_t y) {
    const uint8_t* p = sc.tex + f.off + 3ull * (x + static_cast<uint64_t>(y) * f.w);
    return Col{sc.srgb_values[p[0]], sc.srgb_values[p[1]], sc.srgb_values[p[2]]};
}

__device__ __forceinline__ Col tex_sample(const DevScene& sc, int k, double u, double v) {
    const DevTexFace f = sc.faces[k];
    const double x = clamp01(u) * static_cast<double>(f.w - 1);
    const double y = clamp01(v) * static_cast<double>(f.h - 1);
    const uint32_t x0 = x >= 0.0 ? static_cast<uint32_t>(x) : 0u;   // `as u32`: NaN -> 0
    const uint32_t y0 = y >= 0.0 ? static_cast<uint32_t>(y) : 0u;
    const uint32_t x1 = x0 >= f.w - 1 ? f.w - 1 : x0 + 1;
    const uint32_t y1 = y0 >= f.h - 1 ? f.h - 1 : y0 + 1;
    const double xx = x - static_cast<double>(x0), yy = y - static_cast<double>(y0);
    const Col a = texel(sc, f, x0, y0), b = texel(sc, f, x0, y1), c = texel(sc, f, x1, y0), d = texel(sc, f, x1, y1);
    const Col cx0{a.r * (1.0 - yy) + b.r * yy, a.g * (1.0 - yy) + b.g * yy, a.b * (1.0 - yy) + b.b * yy};
    const Col cx1{c.r * (1.0 - yy) + d.r * yy, c.g * (1.0 - yy) + d.g * yy, c.b * (1.0 - yy) + d.b * yy};
    return Col{cx0.r * (1.0 - xx) + cx1.r * xx, cx0.g * (1.0 - xx) + cx1.g * xx, cx0.b * (1.0 - xx) + cx1.b * xx};
}

// Background::color (raytrace.rs:228-256): the solid colour, or the skybox
// face the direction's dominant axis points at (x, then y, then z; no strict
// winner: BLACK).
__device__ __forceinline__ Col background(const DevScene& sc, const Ray& r) {
    if (!sc.skybox) return Col{sc.bg[0], sc.bg[1], sc.bg[2]};
    const double dx = r.dx, dy = r.dy, dz = r.dz;
    const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
    if (ax > az && ax > ay) {
        const double px = -dz / dx, py = -dy / ax;
        return tex_sample(sc, dx > 0.0 ? 0 : 1, px * 0.5 + 0.5, py * 0.5 + 0.5);
    }
    if (ay > ax && ay > az) {
        const double px = dx / ay, py = dz / dy;
        return tex_sample(sc, dy > 0.0 ? 2 : 3, px * 0.5 + 0.5, py * 0.5 + 0.5);
    }
    if (az > ax && az > ay) {
        const double px = dx / dz, py = -dy / az;
        return tex_sample(sc, dz > 0.0 ? 4 : 5, px * 0.5 + 0.5, py * 0.5 + 0.5);
    }
    return Col{0.0, 0.0, 0.0};
}

}  // namespace rtamd
