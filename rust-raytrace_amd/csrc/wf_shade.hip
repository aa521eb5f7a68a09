// The shading kernels of the wavefront schedule: wf_occlusion (the shadow queries of a
// generation's shade records) and wf_shade (their Phong sums); launch_shading runs both.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wf_chain.hpp"
#include "wf_launch.hpp"

namespace rtamd {

namespace {

// The shadow queries of every shade record of generation k (raytrace.rs:39-49):
// one work-item per (record, light) pair -- the lights of one hit are
// independent queries -- setting bit l of the record's occlusion mask.
template <int kSrc, bool kCount>
__global__ __launch_bounds__(kWfThreads, Src<kSrc>::waves) void wf_occlusion(DevScene sc, FrameParams fp, WfBufs b, int k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const QueueLds ql = queue_lds(lds + staged_bytes<kSrc>(sc), b.G);
    region_scan(b.rs() + k * b.G, b.G, ql.scan, ql.wave);
    const uint32_t L = static_cast<uint32_t>(sc.n_lights);
    const uint32_t nrec = ql.scan[b.G], n = nrec * L;
    if (!wg_has_work(b, n)) return;
    const BvhView v = stage_lds<kSrc>(sc, lds);
    __syncthreads();
    Work w;
    const size_t rk = static_cast<size_t>(k) * b.qcap;
    // light-major: a wave traces 64 consecutive records toward ONE light (coherent).
    // Software pipelined: the next chunk's shade points are loaded (HBM) before this
    // chunk's queries run.  The grid sources take everything else a query needs before its
    // list walk from LDS, so the chunk's first wait on vector memory comes after the
    // own-sphere test and these loads have that long to arrive.
    const uint32_t W = b.G * (kWfThreads / 64), lane = threadIdx.x & 63u;
    // qi / nrec by a multiply with floor(2^32 / nrec) kept in a scalar register (the estimate
    // is at most 2 low: two corrections); entries stay 32-bit (entry < qcap <= capa, a u32)
    const uint32_t nrec_s = __builtin_amdgcn_readfirstlane(nrec);
    const uint32_t magic = __builtin_amdgcn_readfirstlane(
        nrec_s > 1u ? static_cast<uint32_t>((1ull << 32) / nrec_s) : 0xFFFFFFFFu);
    auto item_at = [&](uint32_t qi, uint32_t& l) {
        uint32_t q = __umulhi(qi, magic), rem = qi - q * nrec_s;
        if (rem >= nrec_s) { ++q; rem -= nrec_s; }
        if (rem >= nrec_s) { ++q; rem -= nrec_s; }
        l = q;
        return static_cast<uint32_t>(region_entry(ql.scan, b.G, b.R, rem));
    };
    // Source 15 (spheres through L2, in registers) has no room for the prefetched words at its 64
    // VGPRs: they were spilled, with a wait behind their loads.  It loads a chunk's points when
    // it starts the chunk.
    constexpr bool kAhead = kSrc != kSrcGridG;
    uint32_t rc = wave_slot(b, n), lc = 0;
    uint32_t atc = 0;
    double pc[3] = {0.0, 0.0, 0.0};
    int32_t hc = -1;
    if (kAhead && static_cast<uint64_t>(rc) * 64u + lane < n) {
        atc = item_at(rc * 64u + lane, lc);
        const size_t at = rk + atc;
        pc[0] = ldn_if<3>(&b.rf(0)[at]); pc[1] = ldn_if<3>(&b.rf(1)[at]); pc[2] = ldn_if<3>(&b.rf(2)[at]);
        hc = static_cast<int32_t>(b.ru(1)[at]);
    }
    // The first chunk needs these at once anyway.  Waiting for them here, before the loop, keeps
    // the loop's own waits exact: with loads pending on entry the compiler waits for the loop's
    // prefetch right behind its issue, on every chunk.
    asm volatile("" :: "v"(pc[0]), "v"(pc[1]), "v"(pc[2]), "v"(hc));
    for (; static_cast<uint64_t>(rc) * 64u < n; rc += W) {
        const uint64_t qn = static_cast<uint64_t>(kAhead ? rc + W : rc) * 64u + lane;
        uint32_t ln = 0;
        uint32_t atn = 0;
        double pn[3] = {0.0, 0.0, 0.0};
        int32_t hn = -1;
        if (qn < n) {
            atn = item_at(static_cast<uint32_t>(qn), ln);
            const size_t at = rk + atn;
            pn[0] = ldn_if<3>(&b.rf(0)[at]); pn[1] = ldn_if<3>(&b.rf(1)[at]); pn[2] = ldn_if<3>(&b.rf(2)[at]);
            hn = static_cast<int32_t>(b.ru(1)[at]);
        }
        if constexpr (!kAhead) { lc = ln; atc = atn; pc[0] = pn[0]; pc[1] = pn[1]; pc[2] = pn[2]; hc = hn; }
        const uint32_t qi = rc * 64u + lane;
        const uint32_t l = lc;
        const size_t at = rk + atc;
        const double ptx = pc[0], pty = pc[1], ptz = pc[2];
        const int32_t hint = hc;
        if constexpr (kAhead) { lc = ln; atc = atn; pc[0] = pn[0]; pc[1] = pn[1]; pc[2] = pn[2]; hc = hn; }
        if (qi >= n) continue;
        double lx, ly, lz, r2;
        // the sphere the point lies on is tested first (it shadows every light behind its surface)
        bool occluded;
        if constexpr (Src<kSrc>::grid) {        // the host checked: every light has a grid
            // light and grid header from LDS (stage_lds); the cell's offsets are requested first
            // and travel during the light direction, the planes and the own-sphere test
            const LdsGridHdr& g = v.ghdr[l];
            const GridReq q = lgrid_request(sc, g, ptx, pty, ptz);
            (void)light_dir(v.llights[l], ptx, pty, ptz, lx, ly, lz, r2);
            const Ray sray{ptx + lx * kEps, pty + ly * kEps, ptz + lz * kEps, lx, ly, lz};
            occluded = occluded_lgrid_lds<kCount>(sc, v, g, q, sray, r2, hint, &w);
        } else {
            const bool has_range = light_dir(sc.lights[l], ptx, pty, ptz, lx, ly, lz, r2);
            const Ray sray{ptx + lx * kEps, pty + ly * kEps, ptz + lz * kEps, lx, ly, lz};
            occluded = has_range && sc.lgrid && sc.lgrid[l].R > 0
                           ? occluded_lgrid<kCount>(sc, v, sc.lgrid[l], sray, r2, ptx, pty, ptz, hint, &w)
                           : occluded_any<kSrc, kCount>(sc, v, sray, has_range, r2, hint, &w);
        }
        if (occluded) atomicOr(&b.ru(3)[at], 1u << l);
    }
    flush_work<kCount>(b, 4, w);
}

// The Phong sum of every shade record of generation k.
template <bool kFresnel, bool kPack = false>
__global__ __launch_bounds__(kWfThreads, RT_SHADE_WAVES) void wf_shade(DevScene sc, FrameParams fp, WfBufs b, int k) {
    __shared__ uint32_t s_scan[kMaxRegions + 1];
    __shared__ uint32_t s_wave[kWfThreads / 64];
    region_scan(b.rs() + k * b.G, b.G, s_scan, s_wave);
    const uint32_t n = s_scan[b.G];
    const size_t rk = static_cast<size_t>(k) * b.qcap;
    // software pipelined: the next chunk's records are loaded (HBM) before this chunk is
    // shaded, so at the kernel's 4 waves per SIMD their latency hides behind the f64 math
    const uint32_t W = gridDim.x * (kWfThreads / 64), lane = threadIdx.x & 63u;
    const bool lit = sc.n_lights > 0;
    uint32_t rc = wave_slot(b, n);
    ShadeIn cur{};
    bool have = false;
    if (static_cast<uint64_t>(rc) * 64u + lane < n) {
        cur = shade_load(b, rk + region_entry(s_scan, b.G, b.R, rc * 64u + lane), lit);
        have = true;
    }
    for (; static_cast<uint64_t>(rc) * 64u < n; rc += W) {
        const uint64_t jn = static_cast<uint64_t>(rc + W) * 64u + lane;
        ShadeIn nxt{};
        const bool have_n = jn < n;
        if (have_n) nxt = shade_load(b, rk + region_entry(s_scan, b.G, b.R, static_cast<uint32_t>(jn)), lit);
        if (have) shade_compute<kFresnel, true, kPack>(sc, b, k, cur);
        cur = nxt;
        have = have_n;
    }
}

template <int kSrc>
hipError_t launch_occlusion_src(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, bool count, hipStream_t s) {
    const size_t lds = staged_bytes<kSrc>(sc) + queue_lds_bytes(b.G);
    return dispatch_bools(
        [&](auto kCount) {
            hipLaunchKernelGGL((wf_occlusion<kSrc, kCount()>), dim3(b.G), dim3(kWfThreads), lds, s, sc, fp, b, k);
            return hipSuccess;
        },
        count);
}

}  // namespace

// The shadow queries and the shading of generation k on b stream sb (after its
// nearest-hit launch).
hipError_t launch_shading(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, int src_occ, int grid_occ,
                          bool count, bool packed, hipStream_t sb, LaunchMarks* mb) {
    hipError_t e;
    if (sc.n_lights > 0) {
        if (mb && (e = mb->begin(sb)) != hipSuccess) return e;
        switch (grid_occ == 1 ? kSrcGridL : grid_occ == 2 ? kSrcGridG : src_occ) {
        case kSrcGridL: e = launch_occlusion_src<kSrcGridL>(sc, fp, b, k, count, sb); break;
        case kSrcGridG: e = launch_occlusion_src<kSrcGridG>(sc, fp, b, k, count, sb); break;
        case kSrcGlobal: e = launch_occlusion_src<kSrcGlobal>(sc, fp, b, k, count, sb); break;
        case kSrcLds: e = launch_occlusion_src<kSrcLds>(sc, fp, b, k, count, sb); break;
        case kSrcBvhG: e = launch_occlusion_src<kSrcBvhG>(sc, fp, b, k, count, sb); break;
        case kSrcBvhL8: e = launch_occlusion_src<kSrcBvhL8>(sc, fp, b, k, count, sb); break;
        case kSrcBvh4L: e = launch_occlusion_src<kSrcBvh4L>(sc, fp, b, k, count, sb); break;
        default: e = launch_occlusion_src<kSrcBvh4G>(sc, fp, b, k, count, sb); break;
        }
        if (e != hipSuccess) return e;
        if (mb && (e = mb->mark(sb, kKfOcclusion)) != hipSuccess) return e;
    }
    if (mb && (e = mb->begin(sb)) != hipSuccess) return e;
    e = dispatch_bools(
        [&](auto kFresnel, auto kPack) {
            hipLaunchKernelGGL((wf_shade<kFresnel(), kPack()>), dim3(b.G), dim3(kWfThreads), 0, sb, sc, fp, b, k);
            return hipSuccess;
        },
        sc.has_fresnel, packed);
    return mb ? mb->mark(sb, kKfShade) : e;
}

RT_UNIT_WARM(wf_shade)

}  // namespace rtamd
