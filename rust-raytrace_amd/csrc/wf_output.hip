// The kernels that write pixels and statistics outside the fold: the row-by-row compose and
// resolve passes, a skybox scene's camera misses, the sparse-copy kernels and the tally.
#define RT_UNIT wf_output       // reads the sRGB table: its own copy (trace_types.hpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "wf_device.hpp"
#include "wf_launch.hpp"

namespace rtamd {

namespace {

// wf_sky_pixels (the second sky pass of a skybox scene; the first is wf_sky_term,
// wf_fold.hip), after the camera pass without compose: every chunk pixel whose camera ray missed
// (csky) is finished here, in row order: the ray rebuilt from the FRAME coordinates (camera_ray:
// tile origin, bands, the pass's AA sample), the skybox sampled, and the pixel written as the
// average of its spp identical samples (main.rs:47-56) or, kAa, the sample added to its running sum.
template <bool kAa, bool kMom = false>
__global__ __launch_bounds__(kWfThreads) void wf_sky_pixels(DevScene sc, FrameParams fp, WfBufs b) {
    __shared__ double s_srgb[255];
    for (int i = threadIdx.x; i < 255; i += kWfThreads) s_srgb[i] = c_srgb_avg[i];
    __syncthreads();
    const uint64_t npix = static_cast<uint64_t>(fp.tile_w) * fp.rows;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * kWfThreads + threadIdx.x; p < npix;
         p += static_cast<uint64_t>(gridDim.x) * kWfThreads) {
        if (!b.csky()[p]) continue;
        const uint32_t lx = static_cast<uint32_t>(p % fp.tile_w), lrow = fp.row0 + static_cast<uint32_t>(p / fp.tile_w);
        const Col c = background(sc, camera_ray(sc, fp, lx, lrow, fp.aa_pass));
        if constexpr (kAa) aa_add<kMom>(fp, static_cast<uint32_t>(p), aa_sample(c));
        else write_pixel(fp, lx, lrow, average_samples(c, fp.spp), s_srgb);
    }
}

// The row-by-row kernels take the chunk's rows in 64-pixel segments, one segment per wave per
// turn, the grid striding over them: the body runs with the segment that starts at pixel x0 of
// chunk row lrow (both wave-uniform).  A loop macro like RT_FOR_CHUNKS (a helper taking the body
// as a lambda compiled wf_compose and wf_aa_compose to other code).
constexpr int kComposeWaves = kWfThreads / 64;
#define RT_FOR_ROW_SEGMENTS(fp, lrow, x0)                                                                         \
    for (uint64_t rt_sg = static_cast<uint64_t>(blockIdx.x) * kComposeWaves + (threadIdx.x >> 6),                 \
                  rt_segs = ((fp).tile_w + 63u) / 64u, rt_total = rt_segs * (fp).rows;                            \
         rt_sg < rt_total; rt_sg += static_cast<uint64_t>(gridDim.x) * kComposeWaves)                             \
        if (const uint32_t lrow = static_cast<uint32_t>(rt_sg / rt_segs), x0 = static_cast<uint32_t>(rt_sg % rt_segs) * 64u; true)

// The grid of a row-by-row kernel: at most `workgroups`, one wave per segment.
dim3 row_grid(const FrameParams& fp, uint32_t workgroups) {
    const uint64_t segs = static_cast<uint64_t>((fp.tile_w + 63u) / 64u) * fp.rows;
    return dim3(std::max(1u, static_cast<uint32_t>(std::min<uint64_t>(workgroups, (segs + kComposeWaves - 1) / kComposeWaves))));
}

// The frame of the chunk, row by row (WfBufs::compose): each wave writes 64
// consecutive pixels of one row -- their f32 RGB as 192 consecutive dwords and
// their sRGB BGR as 48 consecutive dwords (or bytes when the row pitch is not a
// multiple of 4), staged through LDS so every store instruction covers
// consecutive addresses -- from the pixel map (chain, background or ambient
// object) and the chains' colours in ccol.  The colours are the fold's /
// write_pixel's values: f32 of the averaged f64 colour and to_srgb of it.
// kSky (a skybox scene): a background pixel is not a constant: its camera ray is rebuilt from the
// frame coordinates (camera_ray) and the skybox sampled in its direction.
template <bool kSky>
__global__ __launch_bounds__(kWfThreads) void wf_compose(DevScene sc, FrameParams fp, WfBufs b) {
    __shared__ float s_rgb[kComposeWaves][192];
    __shared__ uint32_t s_bgr[kComposeWaves][48];
    __shared__ double s_srgb[255];
    for (int i = threadIdx.x; i < 255; i += kWfThreads) s_srgb[i] = c_srgb_avg[i];
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool dw = bgr_dwords(fp);
    RT_FOR_ROW_SEGMENTS(fp, lrow, x0) {
        const uint32_t nv = min(64u, fp.tile_w - x0);                 // pixels in this segment
        const uint32_t x = x0 + lane;
        float r = 0.0f, g = 0.0f, bl = 0.0f;
        uint32_t q = 0;
        if (lane < nv) {
            const uint32_t code = ldn(&b.pmap()[static_cast<size_t>(lrow) * fp.tile_w + x]);
            if (code == kPixBackground && kSky) {
                const Col res = average_samples(background(sc, camera_ray(sc, fp, x, fp.row0 + lrow, fp.aa_pass)), fp.spp);
                r = static_cast<float>(res.r); g = static_cast<float>(res.g); bl = static_cast<float>(res.b);
                q = pack_bgr(res, s_srgb);
            } else if (code == kPixBackground) {
                r = fp.bg_rgb[0]; g = fp.bg_rgb[1]; bl = fp.bg_rgb[2];
                q = fp.bg_bgr[0] | (static_cast<uint32_t>(fp.bg_bgr[1]) << 8) | (static_cast<uint32_t>(fp.bg_bgr[2]) << 16);
            } else if (code & kPixAmbient) {                           // (rare) the ambient colour of a camera hit
                const Col res = average_samples(end_colour(sc, static_cast<int32_t>(code & ~kPixAmbient)), fp.spp);
                r = static_cast<float>(res.r); g = static_cast<float>(res.g); bl = static_cast<float>(res.b);
                q = pack_bgr(res, s_srgb);
            } else {
                const U32x4 cc = ldn(reinterpret_cast<const U32x4*>(b.ccol()) + code);
                r = __uint_as_float(cc[0]); g = __uint_as_float(cc[1]); bl = __uint_as_float(cc[2]);
                q = cc[3];
            }
        }
        store_row_segment(fp, s_rgb[wave], s_bgr[wave], dw, lrow, x0, nv, r, g, bl, q);
    }
}

// RT_ALGO_WAVEFRONT_AA with the compose route: what wf_compose is to a frame, for one pass's
// running sums.  Row by row, 64 consecutive pixels per wave: the pass's sample colour of each
// pixel from the pixel map (the background's, an ambient end's, or the chain's, which the fold
// left in term[chain]) is added to the pixel's running sum (aa_add: coalesced).
template <bool kSky, bool kMom = false>
__global__ __launch_bounds__(kWfThreads) void wf_aa_compose(DevScene sc, FrameParams fp, WfBufs b) {
    const uint32_t lane = threadIdx.x & 63u;
    RT_FOR_ROW_SEGMENTS(fp, lrow, x0) {
        const uint32_t x = x0 + lane;
        if (x >= fp.tile_w) continue;
        const uint32_t p = lrow * fp.tile_w + x;
        const uint32_t code = ldn(&b.pmap()[p]);
        Col s;
        if (code == kPixBackground && kSky) s = aa_sample(background(sc, camera_ray(sc, fp, x, fp.row0 + lrow, fp.aa_pass)));
        else if (code == kPixBackground) s = Col{fp.aa_bg[0], fp.aa_bg[1], fp.aa_bg[2]};
        else if (code & kPixAmbient) s = aa_sample(end_colour(sc, static_cast<int32_t>(code & ~kPixAmbient)));
        else s = Col{ldn(&b.term(0)[code]), ldn(&b.term(1)[code]), ldn(&b.term(2)[code])};
        aa_add<kMom>(fp, p, s);
    }
}

// rt_accum_resolve, and RT_ALGO_WAVEFRONT_AA after the last pass of a chunk: main.rs:56 for a
// tile of running sums, whenever asked.  sums: the tile pixels'
// running sums (3 f64 per pixel, tile row-major) of `samples` samples each; a pixel is sum /
// (double)samples (NaN propagates), rounded once to f32 and quantised from the f64 value.  Row
// by row over rows [0, fp.rows), 64 consecutive pixels per wave, coalesced through
// store_row_segment as wf_compose writes a frame.  Reads the sums, never writes them.
__global__ __launch_bounds__(kWfThreads) void accum_resolve(FrameParams fp, const double* sums, uint32_t samples) {
    __shared__ float s_rgb[kComposeWaves][192];
    __shared__ uint32_t s_bgr[kComposeWaves][48];
    __shared__ double s_srgb[255];
    for (int i = threadIdx.x; i < 255; i += kWfThreads) s_srgb[i] = c_srgb_avg[i];
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool dw = bgr_dwords(fp);
    const double aa = static_cast<double>(samples);
    RT_FOR_ROW_SEGMENTS(fp, lrow, x0) {
        const uint32_t nv = min(64u, fp.tile_w - x0);
        float r = 0.0f, g = 0.0f, bl = 0.0f;
        uint32_t q = 0;
        if (lane < nv) {
            const double* a = sums + 3 * (static_cast<size_t>(lrow) * fp.tile_w + x0 + lane);
            const Col res{ldn(&a[0]) / aa, ldn(&a[1]) / aa, ldn(&a[2]) / aa};
            r = static_cast<float>(res.r); g = static_cast<float>(res.g); bl = static_cast<float>(res.b);
            q = pack_bgr(res, s_srgb);
        }
        store_row_segment(fp, s_rgb[wave], s_bgr[wave], dw, lrow, x0, nv, r, g, bl, q);
    }
}

// rt_accum_noise: the estimate of a moments accumulator.  sums: the tile's 3 f64 sums per
// pixel, then, as a plane of their own, its 3 f64 sums of squares per pixel; n = samples >= 2.  Per pixel and
// channel, every line one IEEE f64 operation (no fma): mean = S / N; d = Q - (S * mean); v = d < 0 ? 0 : d /
// (N * (N - 1)) (a NaN d stays NaN); err = sqrt((v_r + v_g) + v_b) / (floor + ((|mean_r| + |mean_g|) +
// |mean_b|)); above = !(err <= threshold).  Row by row, 64 consecutive pixels per wave as accum_resolve reads
// them; variance (3 f32 per pixel, staged through the wave's LDS slice: consecutive dwords) and error (1 f32 per
// pixel) may be null.  A wave counts its pixels above by ballot and adds its total once to *above, which the host
// zeroed on the stream.  Reads the sums and squares, never writes them.
__global__ __launch_bounds__(kWfThreads) void accum_noise(FrameParams fp, const double* sums, uint32_t samples, double err_floor,
                                                          double threshold, float* variance, float* error,
                                                          unsigned long long* above) {
    __shared__ float s_var[kComposeWaves][192];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const double* squares = sums + 3 * (static_cast<size_t>(fp.tile_w) * fp.tile_h);
    const double N = static_cast<double>(samples), den = __dmul_rn(N, N - 1.0);
    unsigned long long count = 0;
    RT_FOR_ROW_SEGMENTS(fp, lrow, x0) {
        const uint32_t nv = min(64u, fp.tile_w - x0);
        const size_t p0 = static_cast<size_t>(lrow) * fp.tile_w + x0;
        float vf[3] = {0.0f, 0.0f, 0.0f}, ef = 0.0f;
        bool over = false;
        if (lane < nv) {
            const double* a = sums + 3 * (p0 + lane);
            const double* q = squares + 3 * (p0 + lane);
            double v[3], mean[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double S = ldn(&a[k]), Q = ldn(&q[k]);
                mean[k] = S / N;
                const double d = __dsub_rn(Q, __dmul_rn(S, mean[k]));
                v[k] = d < 0.0 ? 0.0 : d / den;
                vf[k] = static_cast<float>(v[k]);
            }
            const double err = sqrt(__dadd_rn(__dadd_rn(v[0], v[1]), v[2])) /
                               __dadd_rn(err_floor, __dadd_rn(__dadd_rn(fabs(mean[0]), fabs(mean[1])), fabs(mean[2])));
            ef = static_cast<float>(err);
            over = !(err <= threshold);
        }
        count += static_cast<unsigned long long>(__popcll(__ballot(over)));
        if (variance) {
            float* s = s_var[wave];
            s[3 * lane] = vf[0]; s[3 * lane + 1] = vf[1]; s[3 * lane + 2] = vf[2];
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            float* dst = variance + 3 * p0;
#pragma unroll
            for (uint32_t j = 0; j < 3; ++j) {
                const uint32_t i = lane + 64u * j;
                if (i < 3 * nv) dst[i] = s[i];
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (error && lane < nv) error[p0 + lane] = ef;
    }
    if (lane == 0 && count) atomicAdd(above, count);
}

// Sparse host copies (rt_render, tuning sparse_out): after the
// camera pass every pixel that starts no chain is final, so the host copies the
// frame then, while the generations run; after the fold only the 16-pixel row
// segments that hold a chain pixel are packed, in row order, and copied.
// wf_chain_segs: one wave per chunk row: segbits (bit s of the row's words:
// segment s holds a chain pixel) and the row's segment count.
__global__ __launch_bounds__(256) void wf_chain_segs(FrameParams fp, WfBufs b, uint32_t* segbits, uint32_t* rowcnt) {
    const uint32_t row = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (row >= fp.rows) return;
    const uint32_t nseg = (fp.tile_w + kSegPx - 1) / kSegPx, words = (nseg + 31) / 32;
    const uint8_t* m = b.cmark() + static_cast<size_t>(row) * fp.tile_w;
    uint32_t cnt = 0;
    for (uint32_t s0 = 0; s0 < nseg; s0 += 64) {
        const uint32_t s = s0 + lane;
        bool any = false;
        if (s < nseg) {
            const uint32_t x1 = min(s * kSegPx + kSegPx, fp.tile_w);
            for (uint32_t x = s * kSegPx; x < x1; ++x) any |= m[x] != 0;
        }
        const unsigned long long bal = __ballot(any);
        cnt += static_cast<uint32_t>(__popcll(bal));
        if (lane == 0) segbits[static_cast<size_t>(row) * words + s0 / 32] = static_cast<uint32_t>(bal);
        if (lane == 32 && s0 / 32 + 1 < words) segbits[static_cast<size_t>(row) * words + s0 / 32 + 1] = static_cast<uint32_t>(bal >> 32);
    }
    if (lane == 0) rowcnt[row] = cnt;
}

// rowoff[r] = segments of rows < r (exclusive scan, rowoff[rows] = total); one workgroup.
__global__ __launch_bounds__(1024) void wf_row_scan(const uint32_t* rowcnt, uint32_t rows, uint32_t* rowoff) {
    __shared__ uint32_t s_wave[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t per = (rows + 1023u) / 1024u, a = t * per, e = min(a + per, rows);
    uint32_t sum = 0;
    for (uint32_t i = a; i < e; ++i) sum += rowcnt[i];
    uint32_t inc = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= static_cast<uint32_t>(off)) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (uint32_t w = 0; w < wave; ++w) run += s_wave[w];
    for (uint32_t i = a; i < e; ++i) { rowoff[i] = run; run += rowcnt[i]; }
    if (t == 1023) rowoff[rows] = run;
}

// After the fold: the flagged segments' BGR (48 B) and f32 RGB (192 B) in row
// order, segment i of the frame at pk_bgr + 48 i / pk_rgb + 48 i; one wave per row.
__global__ __launch_bounds__(256) void wf_chain_pack(FrameParams fp, const uint32_t* segbits, const uint32_t* rowoff,
                                                     uint8_t* pk_bgr, float* pk_rgb) {
    const uint32_t row = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (row >= fp.rows) return;
    const uint32_t nseg = (fp.tile_w + kSegPx - 1) / kSegPx, words = (nseg + 31) / 32;
    const size_t frow = fp.row0 + row;
    uint32_t base = rowoff[row];
    for (uint32_t s0 = 0; s0 < nseg; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t wd = s < nseg ? segbits[static_cast<size_t>(row) * words + s / 32] : 0u;
        const bool flag = (wd >> (s % 32)) & 1u;
        const unsigned long long bal = __ballot(flag);
        const uint32_t rank = base + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)));
        base += static_cast<uint32_t>(__popcll(bal));
        if (!flag) continue;
        const uint32_t x0 = s * kSegPx, n = min(kSegPx, fp.tile_w - x0);
        if (fp.out_bgr) {
            const uint8_t* src = fp.out_bgr + frow * fp.bgr_pitch + 3u * x0;
            uint8_t* dst = pk_bgr + static_cast<size_t>(rank) * (3 * kSegPx);
            if (n == kSegPx && fp.bgr_pitch % 4u == 0) {
                static_assert(kSegPx % 4 == 0, "segments of whole dwords");
                for (uint32_t k = 0; k < 3 * kSegPx / 4; ++k)
                    reinterpret_cast<uint32_t*>(dst)[k] = reinterpret_cast<const uint32_t*>(src)[k];
            } else {
                for (uint32_t k = 0; k < 3 * n; ++k) dst[k] = src[k];
            }
        }
        if (fp.out_rgb) {
            const float* src = fp.out_rgb + (frow * fp.tile_w + x0) * 3;
            float* dst = pk_rgb + static_cast<size_t>(rank) * (3 * kSegPx);
            for (uint32_t k = 0; k < 3 * n; ++k) dst[k] = src[k];
        }
    }
}

// Scene::intersect calls of this chunk: every pixel's camera ray, every later
// queue entry, and one shadow query per light per shade record; plus the
// per-generation queue sizes.  One workgroup; atomics because chunks on
// different streams may finish together.
__global__ __launch_bounds__(kWfThreads) void wf_tally(FrameParams fp, WfBufs b, int n_lights, int generations) {
    __shared__ unsigned long long s_sum[2 * kMaxGenerations];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // one wave per (generation, queue|records) pair, lanes striding the regions
    for (int item = wave; item < 2 * generations; item += kWfThreads / 64) {
        const int g = item >> 1;
        const uint32_t* src = (item & 1) ? b.rs() : b.rq();
        unsigned long long v = 0;
        if ((item & 1) || g > 0)
            for (uint32_t r = lane; r < b.G; r += 64) v += src[g * b.G + r];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) s_sum[(item & 1) ? kMaxGenerations + g : g] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long nearest = static_cast<unsigned long long>(fp.tile_w) * fp.rows, shadow = 0;
        for (int g = 0; g < generations; ++g) {
            nearest += s_sum[g];
            shadow += s_sum[kMaxGenerations + g] * n_lights;
        }
        atomicAdd(&b.totals[0], nearest * fp.spp);
        atomicAdd(&b.totals[1], shadow * fp.spp);
    }
    // (RT_ALGO_WAVEFRONT_AA: the queue sizes of the last pass of the last chunk only)
    if (fp.aa_acc && !(fp.aa_flags & kAaTallyGens)) return;
    for (int g = threadIdx.x; g < generations; g += kWfThreads) {
        atomicAdd(&b.gen_totals[kCntQ + g], s_sum[g]);
        atomicAdd(&b.gen_totals[kCntS + g], s_sum[kMaxGenerations + g]);
    }
}

}  // namespace

hipError_t launch_sky_pixels(const DevScene& sc, const FrameParams& fp, const WfBufs& b, hipStream_t s, LaunchMarks* m) {
    hipError_t e;
    if (m && (e = m->begin(s)) != hipSuccess) return e;
    const uint64_t npix = static_cast<uint64_t>(fp.tile_w) * fp.rows;
    const dim3 grid(std::max(1u, static_cast<uint32_t>(std::min<uint64_t>(4u * b.G, (npix + kWfThreads - 1) / kWfThreads))));
    (void)dispatch_bools(
        [&](auto kAa, auto kMom) {
            if constexpr (kMom() && !kAa()) {                  // (kMom: a moments accumulator's passes only)
                return hipErrorInvalidValue;
            } else {
                hipLaunchKernelGGL((wf_sky_pixels<kAa(), kMom()>), grid, dim3(kWfThreads), 0, s, sc, fp, b);
                return hipSuccess;
            }
        },
        fp.aa_acc != nullptr, aa_moments(fp));
    return m ? m->mark(s, kKfCompose) : hipGetLastError();
}

// The compose route's last step of a chunk (or, RT_ALGO_WAVEFRONT_AA, of a pass: the samples to
// the running sums), once every chain has its colour.
hipError_t launch_compose(const DevScene& sc, const FrameParams& fp, const WfBufs& b, hipStream_t s) {
    const dim3 grid = row_grid(fp, 4u * b.G);
    return dispatch_bools(
        [&](auto kAa, auto kSky, auto kMom) {
            if constexpr (kAa()) hipLaunchKernelGGL((wf_aa_compose<kSky(), kMom()>), grid, dim3(kWfThreads), 0, s, sc, fp, b);
            else hipLaunchKernelGGL(wf_compose<kSky()>, grid, dim3(kWfThreads), 0, s, sc, fp, b);
            return hipSuccess;
        },
        fp.aa_acc != nullptr, sc.skybox, aa_moments(fp));
}

hipError_t launch_accum_resolve(const FrameParams& fp, uint32_t workgroups, hipStream_t s) {
    if (fp.tile_w == 0 || fp.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_resolve, row_grid(fp, workgroups), dim3(kWfThreads), 0, s, fp, fp.aa_acc, fp.aa_spp);
    return hipGetLastError();
}

hipError_t launch_accum_noise(const FrameParams& fp, uint32_t workgroups, double err_floor, double threshold, float* variance,
                              float* error, unsigned long long* above, hipStream_t s) {
    if (fp.tile_w == 0 || fp.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_noise, row_grid(fp, workgroups), dim3(kWfThreads), 0, s, fp, fp.aa_acc, fp.aa_spp, err_floor, threshold,
                       variance, error, above);
    return hipGetLastError();
}

hipError_t launch_tally(const FrameParams& fp, const WfBufs& b, int n_lights, int generations, hipStream_t s) {
    hipLaunchKernelGGL(wf_tally, dim3(1), dim3(kWfThreads), 0, s, fp, b, n_lights, generations);
    return hipGetLastError();
}

hipError_t launch_chain_segs(const FrameParams& fp, const WfBufs& b, uint32_t* segbits, uint32_t* rowcnt, uint32_t* rowoff,
                             hipStream_t s) {
    const dim3 grid((fp.rows + 3u) / 4u);
    hipLaunchKernelGGL(wf_chain_segs, grid, dim3(256), 0, s, fp, b, segbits, rowcnt);
    hipLaunchKernelGGL(wf_row_scan, dim3(1), dim3(1024), 0, s, rowcnt, fp.rows, rowoff);
    return hipGetLastError();
}

hipError_t launch_chain_pack(const FrameParams& fp, const uint32_t* segbits, const uint32_t* rowoff, uint8_t* pk_bgr,
                             float* pk_rgb, hipStream_t s) {
    hipLaunchKernelGGL(wf_chain_pack, dim3((fp.rows + 3u) / 4u), dim3(256), 0, s, fp, segbits, rowoff, pk_bgr, pk_rgb);
    return hipGetLastError();
}

RT_UNIT_WARM(wf_output)
RT_UNIT_SRGB(wf_output)

}  // namespace rtamd
