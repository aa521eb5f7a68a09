// The fused tail of the wavefront schedule: one launch that takes every chain still running at
// generation T-1 through all its remaining bounces and folds it (wf_tail).
#define RT_UNIT wf_tail         // reads the sRGB table: its own copy (trace_types.hpp)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wf_chain.hpp"
#include "wf_launch.hpp"

namespace rtamd {

namespace {

// One chain of the fused tail from its shade record of generation T-1 on: the
// record's shadows and shading (wf_occlusion + wf_shade), then generation by
// generation what wf_nearest (finish_nearest), wf_occlusion and wf_shade do to
// it, in registers -- the same operations on the same operands, so the levels
// it writes are the per-generation kernels' bits.  Returns the chain's
// terminal colour and sets nlev (the generation it ended in) instead of writing
// them: the caller folds the chain right away.  cnt[0][k] / cnt[1][k]: this
// workgroup's shade records of generation k / rays queued for generation k.
template <bool kFresnel, bool kCount, bool kSky, bool kPack>
__device__ __forceinline__ Col tail_chain(const DevScene& sc, const FrameParams& fp, const WfBufs& b, const BvhView& v,
                                          int k, ShadeIn in, int& nlev, uint32_t (*cnt)[kMaxGenerations], Work& wn,
                                          Work& wsh) {
    const int k0 = k;
    for (;;) {
        in.mask = grid_shadow_mask<kCount>(sc, v, in.ptx, in.pty, in.ptz, in.prim, wsh);
        const ShadeOut so = shade_compute<kFresnel, false, kPack>(sc, b, k, in);        // level k if specular
        if (!so.specular) { nlev = k; return so.res; }
        const Ray r = reflect_ray(Ray{in.ptx, in.pty, in.ptz, in.dx, in.dy, in.dz}, in.ptx, in.pty, in.ptz, so.nx, so.ny,
                                  so.nz);                                   // raytrace.rs:58-64
        const double sig = (so.f * in.sig) * sc.mats[in.obj].ks_sig;
        ++k;
        if (k > k0 + 1) atomicAdd(&cnt[1][k], 1u);                         // (Q_T was counted by wf_nearest)
        const Hit h = nearest_any<kSrcBvhL8C, kCount>(sc, v, r, &wn);
        nlev = k;
        if (h.obj == INT32_MAX) {                                          // raytrace.rs:265, 228-256
            if constexpr (kSky) return background(sc, r);                  // (folded at once: sampled here)
            else return end_colour(sc, INT32_MAX);
        }
        const DevMaterial& m = sc.mats[h.obj];
        if (static_cast<uint32_t>(k) > fp.max_depth) return end_colour(sc, h.obj);    // raytrace.rs:33
        in.ptx = r.ox + r.dx * h.t; in.pty = r.oy + r.dy * h.t; in.ptz = r.oz + r.dz * h.t;   // ray.cast(t)
        double nx, ny, nz;
        hit_normal(sc, v.sph, h.prim, in.ptx, in.pty, in.ptz, nx, ny, nz);
        const Shading sh = shading_flags<kFresnel>(m, sig, nx * r.dx + ny * r.dy + nz * r.dz);
        if (!sh.diffuse && !sh.specular) return end_colour(sc, h.obj);
        atomicAdd(&cnt[0][k], 1u);
        in.dx = r.dx; in.dy = r.dy; in.dz = r.dz;
        in.sig = sig;
        in.obj = h.obj;
        in.prim = h.prim;
    }
}

// The fused tail (WfStreams::tail_fuse = T): for a small chunk (one rank's
// share of a frame), whose late generations are a chain of latency-bound
// launches, one launch takes every chain still running at generation T-1 from
// its shade record of T-1 through all its remaining bounces (tail_chain), one
// chain per work-item, and folds it onto its levels (fold_levels, as wf_fold)
// and writes its pixel: instead of a nearest-hit launch per generation >= T
// with its shadow and shading launches, and the frame-end fold.  The launch
// waits for the B streams (the levels of generations <= T-2 are written); the
// chains that ended by generation T-1 are folded meanwhile on a B stream
// (wf_fold over nlev <= T-1; the tail's chains keep nlev = kNlevRunning).  It
// lasts about as long as the slowest chain's remaining bounces, not the sum
// over generations of each generation's slowest walk plus a launch each.
// Needs the src-9 tree (whole tree + spheres in LDS) and a light-view grid for
// every light.  Chains in contiguous runs of cw per wave (tuning tail_width;
// auto: spread over about half of the waves; 48 per wave beat 16 / 24 / 32 /
// 64 on one rank's share of an 8-way C3 frame: the slowest chain of a wave
// against the lanes its finished chains leave idle), contiguous so that the
// record loads and level stores stay coalesced.  gridDim.x workgroups, all
// resident; workgroup w publishes its counts in region w and zeros in the
// other regions r = w (mod gridDim.x) of every generation >= T.
template <bool kFresnel, bool kCount, bool kAa = false, bool kSky = false, bool kPack = false, bool kMom = false>
__global__ __launch_bounds__(kWfThreads, 4) void wf_tail(DevScene sc, FrameParams fp, WfBufs b, int T, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t s_cnt[2][kMaxGenerations];
    __shared__ double s_srgb[255];
    const QueueLds ql = queue_lds(lds + staged_bytes<kSrcBvhL8C>(sc), b.G);
    for (int i = threadIdx.x; i < 2 * kMaxGenerations; i += kWfThreads) (&s_cnt[0][0])[i] = 0u;
    for (int i = threadIdx.x; i < 255; i += kWfThreads) s_srgb[i] = c_srgb_avg[i];
    region_scan(b.rs() + (T - 1) * b.G, b.G, ql.scan, ql.wave);   // generation T-1's records; ends with a barrier
    const uint32_t n = ql.scan[b.G];
    const int gens = static_cast<int>(fp.max_depth) + 2;
    const uint32_t nw = gridDim.x * (kWfThreads / 64);
    const uint32_t lane = threadIdx.x & 63u, slot = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
    const uint32_t cw = W > 0 ? static_cast<uint32_t>(W) : max(1u, min(64u, (2u * n + nw - 1) / nw));
    Work wn, wsh;
    const BvhView v = stage_lds<kSrcBvhL8C, true>(sc, lds);
    __syncthreads();
    const size_t rk = static_cast<size_t>(T - 1) * b.qcap;
    for (uint64_t base = static_cast<uint64_t>(slot) * cw; base < n; base += static_cast<uint64_t>(nw) * cw) {
        const uint64_t j = base + lane;
        if (lane >= cw || j >= n) continue;
        const size_t at = rk + region_entry(ql.scan, b.G, b.R, static_cast<uint32_t>(j));
        const ShadeIn in = shade_load(b, at, false);
        int nlev = 0;
        const Col term = tail_chain<kFresnel, kCount, kSky, kPack>(sc, fp, b, v, T - 1, in, nlev, s_cnt, wn, wsh);
        const Col folded = fold_levels<kFresnel, kPack>(sc, b, in.c, nlev, term);
        const Col res = kAa ? aa_sample(folded) : average_samples(folded, fp.spp);
        emit_chain<kAa, kMom>(fp, b, in.c, b.compose ? 0u : b.cpix()[in.c], res, s_srgb);
    }
    __syncthreads();
    for (uint32_t rg = blockIdx.x; rg < b.G; rg += gridDim.x) {
        const bool own = rg == blockIdx.x;
        for (int k = T + static_cast<int>(threadIdx.x); k < gens; k += kWfThreads) {
            b.rs()[k * b.G + rg] = own ? s_cnt[0][k] : 0u;
            b.rq()[(k + 1) * b.G + rg] = own ? s_cnt[1][k + 1] : 0u;
        }
    }
    flush_work<kCount>(b, 2, wn);
    flush_work<kCount>(b, 4, wsh);
}

}  // namespace

// (one source only: the tail walks kSrcBvhL8C's LDS layout, whatever the generations before it used)
hipError_t launch_tail(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int T, bool count, bool packed, int wgs,
                       int width, hipStream_t s) {
    const size_t lds = staged_bytes<kSrcBvhL8C>(sc) + queue_lds_bytes(b.G);
    return dispatch_bools(
        [&](auto kFresnel, auto kCount, auto kAa, auto kSky, auto kPack, auto kMom) {
            if constexpr (kMom() && !kAa()) {                  // (kMom: a moments accumulator's passes only)
                return hipErrorInvalidValue;
            } else {
                hipLaunchKernelGGL((wf_tail<kFresnel(), kCount(), kAa(), kSky(), kPack(), kMom()>), dim3(wgs), dim3(kWfThreads),
                                   lds, s, sc, fp, b, T, width);
                return hipSuccess;
            }
        },
        sc.has_fresnel, count, fp.aa_acc != nullptr, sc.skybox, packed, aa_moments(fp));
}

RT_UNIT_WARM(wf_tail)
RT_UNIT_SRGB(wf_tail)

}  // namespace rtamd
