// The denoiser (include/raytrace_amd.h, rt_denoise_device): an edge-avoiding a-trous wavelet filter over a colour
// image, guided by the first-hit feature buffers.  The rule is the header's, operation by operation: f64 + - * / and
// comparisons in the order written there (-ffp-contract=off: nothing fused), one rounding to f32 between passes.
//   dn_pack      the caller's tight f32 images into 16-byte records: colour (demodulated) and guide (normal, depth),
//                so that a tap is two dwordx4 loads
//   dn_pass      one pass, one pixel per lane, a wave on 64 consecutive pixels of a row; kLds false: the taps are
//                read through L2 (direct form); kLds true (steps 1 and 2): the workgroup's 64 x 8 tile and a halo of
//                2 * step pixels are staged in LDS first.  Both forms run dn_filter on the same records: same bits.
//                kLast: the pass that remodulates and writes the caller's f32 and sRGB outputs row segment by row
//                segment (store_row_segment, the staged sRGB table: what wf_compose and accum_resolve do).
// kVar (rt_denoise_var_device, the header's "variance-guided" additions): the colour record's fourth float carries a
// scalar variance.  dn_pack forms it, a pass prefilters it over the 3 x 3 pixels around its own (always one pixel
// apart: inside the staged halo in the LDS form, eight more records through L2 in the direct form), divides every
// tap's weight once more and writes the variance of its weighted mean; the last pass stores it one dword per lane.
// The forms without kVar are the code they were.
// No walk stack, no private arrays: no scratch.
#define RT_UNIT wf_denoise      // reads the sRGB table: its own copy (trace_types.hpp)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "render_plan.hpp"
#include "wf_device.hpp"
#include "wf_launch.hpp"

namespace rtamd {
namespace {

constexpr uint32_t kDnThreads = kDnTileW * kDnTileH;
static_assert(kDnTileW == 64, "a wave is one 64-pixel row segment (store_row_segment)");
static_assert(sizeof(DnRec) == kDnRecordBytes, "one dwordx4 per record");
// the staged tile of the largest LDS step: (64 + 4 s) x (8 + 4 s) records
constexpr uint32_t kDnLdsRecs = (kDnTileW + 4 * kDnLdsMaxStep) * (kDnTileH + 4 * kDnLdsMaxStep);

__device__ __forceinline__ bool dn_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double dn_k(int a) { return a == 0 ? 0.375 : (a == 1 ? 0.25 : 0.0625); }   // K = {3/8, 1/4, 1/16}

// What only the kVar kernels are passed: nothing otherwise.
struct DnNoVar {};
template <bool kVar>
using DnVarArg = std::conditional_t<kVar, DnVar, DnNoVar>;
template <bool kVar>
using DnVarImage = std::conditional_t<kVar, const float*, DnNoVar>;

template <bool kVar>
__global__ __launch_bounds__(256) void dn_pack(DnFilter f, const float* rgb, const float* normal, const float* depth,
                                               const float* albedo, DnRec* colour, DnRec* guide, DnVarImage<kVar> variance) {
    const uint64_t npix = static_cast<uint64_t>(f.w) * f.h;
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= npix) return;
    float c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
    if (f.flags & RT_DN_DEMODULATE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = static_cast<double>(albedo[3 * p + k]);
            if (a > 0.0) c[k] = static_cast<float>(static_cast<double>(c[k]) / a);
        }
    }
    float var = 0.0f;
    if constexpr (kVar) {
        double u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u[k] = static_cast<double>(variance[3 * p + k]);
            if (f.flags & RT_DN_DEMODULATE) {
                const double a = static_cast<double>(albedo[3 * p + k]);
                if (a > 0.0) u[k] = u[k] / (a * a);
            }
            u[k] = u[k] > 0.0 ? u[k] : 0.0;
        }
        var = static_cast<float>((u[0] + u[1]) + u[2]);
    }
    colour[p] = DnRec{c[0], c[1], c[2], var};
    DnRec g{0.0f, 0.0f, 0.0f, 0.0f};
    if (f.flags & RT_DN_NORMAL) { g.x = normal[3 * p]; g.y = normal[3 * p + 1]; g.z = normal[3 * p + 2]; }
    if (f.flags & RT_DN_DEPTH) g.w = depth[p];
    guide[p] = g;
}

__device__ __forceinline__ double dn_g(int a) { return a == 0 ? 0.5 : 0.25; }                       // G = {1/2, 1/4}

// The pass's value of pixel (x, y) (inside the image).  fetch(qx, qy, c, g) gives the records of a pixel inside the image.
// kVar: svsv = sigma_variance * sigma_variance; xvar: the variance the pass leaves at the pixel.
template <bool kVar, class Fetch>
__device__ __forceinline__ Col dn_filter(const DnFilter& f, uint32_t s, int x, int y, const Fetch& fetch, double svsv,
                                         double vfloor, double& xvar) {
    const bool by_n = f.flags & RT_DN_NORMAL, by_z = f.flags & RT_DN_DEPTH, by_c = f.flags & RT_DN_COLOR;
    DnRec cp, gp;
    fetch(x, y, cp, gp);
    const double pr = cp.x, pg = cp.y, pb = cp.z;
    const double pnx = gp.x, pny = gp.y, pnz = gp.z, pz = gp.w;
    const double t = f.sigma_depth * static_cast<double>(s), tt = t * t;
    const double sc = f.sigma_color / static_cast<double>(s), scsc = sc * sc;
    const int w = static_cast<int>(f.w), h = static_cast<int>(f.h), st = static_cast<int>(s);
    double sr = 0.0, sg = 0.0, sb = 0.0, ws = 0.0;
    double den = 0.0, vs = 0.0;
    if constexpr (kVar) {
        double gs = 0.0, gw = 0.0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= h) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= w) continue;
                DnRec cq = cp, gq = gp;
                if (dx != 0 || dy != 0) fetch(qx, qy, cq, gq);
                const double gk = dn_g(dy < 0 ? -dy : dy) * dn_g(dx < 0 ? -dx : dx);
                gs = gs + gk * static_cast<double>(cq.w);
                gw = gw + gk;
            }
        }
        den = svsv * (gs / gw) + vfloor;
    }
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + st * dy;
        if (qy < 0 || qy >= h) continue;
        const double ky = dn_k(dy < 0 ? -dy : dy);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + st * dx;
            if (qx < 0 || qx >= w) continue;
            double wt = ky * dn_k(dx < 0 ? -dx : dx);
            DnRec cq = cp, gq = gp;
            if (dx != 0 || dy != 0) {
                fetch(qx, qy, cq, gq);
                if (by_n) {
                    double d = (pnx * static_cast<double>(gq.x) + pny * static_cast<double>(gq.y)) + pnz * static_cast<double>(gq.z);
                    d = d > 0.0 ? d : 0.0;
                    for (uint32_t k = 0; k < f.squarings; ++k) d = d * d;
                    wt = wt * d;
                }
                if (by_z) {
                    const double dz = pz - static_cast<double>(gq.w);
                    wt = wt / (1.0 + (dz * dz) / tt);
                }
                if (by_c) {
                    const double dr = pr - static_cast<double>(cq.x), dg = pg - static_cast<double>(cq.y),
                                 db = pb - static_cast<double>(cq.z);
                    const double e = (dr * dr + dg * dg) + db * db;
                    wt = wt / (1.0 + e / scsc);
                }
                // e written out again, on purpose: the compiler forms it once, and one block shared with RT_DN_COLOR's
                // (`if (by_c || kVar)`) moves registers in the kernels without kVar
                if constexpr (kVar) {
                    const double dr = pr - static_cast<double>(cq.x), dg = pg - static_cast<double>(cq.y),
                                 db = pb - static_cast<double>(cq.z);
                    const double e = (dr * dr + dg * dg) + db * db;
                    wt = wt / (1.0 + e / den);
                }
                if (!(wt > 0.0) || !(dn_finite(cq.x) && dn_finite(cq.y) && dn_finite(cq.z))) continue;
            }
            sr = sr + wt * static_cast<double>(cq.x);
            sg = sg + wt * static_cast<double>(cq.y);
            sb = sb + wt * static_cast<double>(cq.z);
            ws = ws + wt;
            if constexpr (kVar) vs = vs + (wt * wt) * static_cast<double>(cq.w);
        }
    }
    if constexpr (kVar) {
        const double xv = vs / (ws * ws);
        xvar = xv > 0.0 ? xv : 0.0;
    }
    return Col{sr / ws, sg / ws, sb / ws};
}

// Workgroup (bx, by): the tile of pixels [64 bx, 64 bx + 64) x [8 by, 8 by + 8); wave j its row j.
template <bool kLds, bool kLast, bool kVar>
__global__ __launch_bounds__(kDnThreads) void dn_pass(DnFilter f, uint32_t s, const DnRec* src, const DnRec* guide, DnRec* dst,
                                                      const float* albedo, float* out_rgb, uint8_t* out_bgr, uint32_t bgr_pitch,
                                                      DnVarArg<kVar> va) {
    __shared__ DnRec s_c[kLds ? kDnLdsRecs : 1], s_g[kLds ? kDnLdsRecs : 1];
    __shared__ float s_rgb[kLast ? kDnTileH : 1][192];
    __shared__ uint32_t s_bgr[kLast ? kDnTileH : 1][48];
    __shared__ double s_srgb[kLast ? 255 : 1];
    const bool guided = f.flags & (RT_DN_NORMAL | RT_DN_DEPTH);
    const int x0 = static_cast<int>(blockIdx.x * kDnTileW), y0 = static_cast<int>(blockIdx.y * kDnTileH);
    const int halo = 2 * static_cast<int>(s), tw = static_cast<int>(kDnTileW) + 2 * halo;
    if constexpr (kLast)
        for (uint32_t i = threadIdx.x; i < 255; i += kDnThreads) s_srgb[i] = c_srgb_avg[i];
    if constexpr (kLds) {
        // the tile and its halo; a record outside the image is never read (its tap is skipped), so it is not staged
        const int th = static_cast<int>(kDnTileH) + 2 * halo;
        for (int i = static_cast<int>(threadIdx.x); i < tw * th; i += static_cast<int>(kDnThreads)) {
            const int gx = x0 - halo + i % tw, gy = y0 - halo + i / tw;
            if (gx < 0 || gy < 0 || gx >= static_cast<int>(f.w) || gy >= static_cast<int>(f.h)) continue;
            const size_t q = static_cast<size_t>(gy) * f.w + static_cast<size_t>(gx);
            s_c[i] = src[q];
            if (guided) s_g[i] = guide[q];
        }
    }
    if constexpr (kLds || kLast) __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int x = x0 + static_cast<int>(lane), y = y0 + static_cast<int>(wave);
    if (y >= static_cast<int>(f.h)) return;                    // (wave-uniform; no barrier follows)
    const bool inside = x < static_cast<int>(f.w);
    Col v{0.0, 0.0, 0.0};
    double svsv = 0.0, vfloor = 0.0, xvar = 0.0;
    if constexpr (kVar) {
        svsv = va.sigma_variance * va.sigma_variance;
        vfloor = va.variance_floor;
    }
    if (inside) {
        if constexpr (kLds) {
            v = dn_filter<kVar>(f, s, x, y, [&](int qx, int qy, DnRec& c, DnRec& g) {
                const int i = (qy - y0 + halo) * tw + (qx - x0 + halo);
                c = s_c[i];
                if (guided) g = s_g[i];
            }, svsv, vfloor, xvar);
        } else {
            v = dn_filter<kVar>(f, s, x, y, [&](int qx, int qy, DnRec& c, DnRec& g) {
                const size_t q = static_cast<size_t>(qy) * f.w + static_cast<size_t>(qx);
                c = src[q];
                if (guided) g = guide[q];
            }, svsv, vfloor, xvar);
        }
    }
    const size_t p = static_cast<size_t>(y) * f.w + static_cast<size_t>(x);
    if constexpr (!kLast) {
        if (inside) dst[p] = DnRec{static_cast<float>(v.r), static_cast<float>(v.g), static_cast<float>(v.b), static_cast<float>(xvar)};
    } else {
        if constexpr (kVar)
            if (inside && va.out_variance) va.out_variance[p] = static_cast<float>(xvar);   // one dword per lane
        if (inside && (f.flags & RT_DN_DEMODULATE)) {
            const double ar = albedo[3 * p], ag = albedo[3 * p + 1], ab = albedo[3 * p + 2];
            if (ar > 0.0) v.r = v.r * ar;
            if (ag > 0.0) v.g = v.g * ag;
            if (ab > 0.0) v.b = v.b * ab;
        }
        FrameParams fp{};
        fp.tile_w = f.w;
        fp.bgr_pitch = bgr_pitch;
        fp.pad_end = 3 * f.w;                                  // a caller's rows: the padding is the caller's
        fp.out_rgb = out_rgb;
        fp.out_bgr = out_bgr;
        const uint32_t nv = min(kDnTileW, f.w - static_cast<uint32_t>(x0));
        store_row_segment(fp, s_rgb[wave], s_bgr[wave], bgr_dwords(fp), static_cast<uint32_t>(y), static_cast<uint32_t>(x0), nv,
                          static_cast<float>(v.r), static_cast<float>(v.g), static_cast<float>(v.b), inside ? pack_bgr(v, s_srgb) : 0u);
    }
}

template <bool kLast, bool kVar>
hipError_t launch_pass(const DnFilter& f, uint32_t step, bool lds, const DnRec* src, const DnRec* guide, DnRec* dst,
                       const float* albedo, float* out_rgb, uint8_t* out_bgr, uint32_t bgr_pitch, uint32_t grid_x, uint32_t grid_y,
                       hipStream_t s, DnVarArg<kVar> va) {
    if (lds && step > kDnLdsMaxStep) return hipErrorInvalidValue;
    const dim3 grid(grid_x, grid_y), block(kDnThreads);
    if (lds)
        hipLaunchKernelGGL((dn_pass<true, kLast, kVar>), grid, block, 0, s, f, step, src, guide, dst, albedo, out_rgb, out_bgr, bgr_pitch, va);
    else
        hipLaunchKernelGGL((dn_pass<false, kLast, kVar>), grid, block, 0, s, f, step, src, guide, dst, albedo, out_rgb, out_bgr, bgr_pitch, va);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_denoise_pack(const DnFilter& f, const float* rgb, const float* normal, const float* depth,
                               const float* albedo, DnRec* colour, DnRec* guide, hipStream_t s, const float* variance) {
    const uint64_t npix = static_cast<uint64_t>(f.w) * f.h;
    const dim3 grid(static_cast<uint32_t>((npix + 255) / 256)), block(256);
    if (variance) hipLaunchKernelGGL(dn_pack<true>, grid, block, 0, s, f, rgb, normal, depth, albedo, colour, guide, variance);
    else hipLaunchKernelGGL(dn_pack<false>, grid, block, 0, s, f, rgb, normal, depth, albedo, colour, guide, DnNoVar{});
    return hipGetLastError();
}

hipError_t launch_denoise_pass(const DnFilter& f, uint32_t step, bool lds, const DnRec* src, const DnRec* guide, DnRec* dst,
                               uint32_t grid_x, uint32_t grid_y, hipStream_t s, const DnVar* var) {
    if (var) return launch_pass<false, true>(f, step, lds, src, guide, dst, nullptr, nullptr, nullptr, 0, grid_x, grid_y, s, *var);
    return launch_pass<false, false>(f, step, lds, src, guide, dst, nullptr, nullptr, nullptr, 0, grid_x, grid_y, s, DnNoVar{});
}

hipError_t launch_denoise_last(const DnFilter& f, uint32_t step, bool lds, const DnRec* src, const DnRec* guide,
                               const float* albedo, float* out_rgb, uint8_t* out_bgr, uint32_t bgr_pitch, uint32_t grid_x,
                               uint32_t grid_y, hipStream_t s, const DnVar* var) {
    if (var) return launch_pass<true, true>(f, step, lds, src, guide, nullptr, albedo, out_rgb, out_bgr, bgr_pitch, grid_x, grid_y, s, *var);
    return launch_pass<true, false>(f, step, lds, src, guide, nullptr, albedo, out_rgb, out_bgr, bgr_pitch, grid_x, grid_y, s, DnNoVar{});
}

RT_UNIT_WARM(wf_denoise)
RT_UNIT_SRGB(wf_denoise)

}  // namespace rtamd
