// The fold of the wavefront schedule: wf_fold (every ended chain's levels onto its terminal, and
// its pixel) and, on a skybox scene, wf_sky_term before it.
#define RT_UNIT wf_fold         // reads the sRGB table: its own copy (trace_types.hpp)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wf_chain.hpp"
#include "wf_launch.hpp"

namespace rtamd {

namespace {

// One chain per work-item: the chains of the chunk are generation 0's shade
// records (chain c = record entry c), dealt densely over G workgroups through
// the region scan of generation 0's record counts, 64 consecutive chains to a
// wave (so levels and terminals are read in chain order, coalesced).  The
// launch is G workgroups whatever the queue capacity: one workgroup per 256
// entries of capacity (the first design) dispatched tens of thousands of
// mostly empty workgroups, ~80 us of dispatch for one rank's share of an
// 8-way C3 frame.  Chain c folds its levels onto its terminal and writes
// pixel cpix[c].  The quantisation table is staged in LDS: the binary search
// indexes it with a different entry per lane, which from __constant__ memory
// costs nine dependent vector loads per channel.
// Only chains of lo <= nlev <= hi: with the fused tail, the chains that ended
// by generation T-1 fold on a B stream while the tail runs (every level and
// terminal they need is written by then); the tail folds its own.
// RT_FOLD_THREADS-thread workgroups (256: at the fold's ~96 VGPRs five of them,
// 20 waves, fit a CU where one 1024-thread workgroup leaves 4 wave slots idle),
// dealt block-major over (kWfThreads / RT_FOLD_THREADS) x G workgroups.
template <bool kFresnel, bool kAa = false, bool kPack = false, bool kMom = false>
__global__ __launch_bounds__(RT_FOLD_THREADS, RT_FOLD_WAVES) void wf_fold(DevScene sc, FrameParams fp, WfBufs b, uint32_t lo,
                                                                          uint32_t hi) {
    constexpr int kT = RT_FOLD_THREADS;
    __shared__ double s_srgb[255];
    __shared__ uint32_t s_scan[kMaxRegions + 1];
    __shared__ uint32_t s_wave[kT / 64];
    for (int i = threadIdx.x; i < 255; i += kT) s_srgb[i] = c_srgb_avg[i];
    region_scan<kT>(b.rs(), b.G, s_scan, s_wave);         // generation 0's records = the chains (also publishes s_srgb)
    const uint32_t n = s_scan[b.G];
    // software pipelined: the next chunk's chain header (level count, pixel, terminal) is
    // loaded before this chain's levels are folded, one dependent round trip less per chain
    const uint32_t W = gridDim.x * (kT / 64), lane = threadIdx.x & 63u;
    struct Head {
        uint32_t c, nlev, p;
        Col term;
    };
    auto head = [&](uint64_t j) {
        Head hd{0u, kNlevRunning, 0u, Col{0.0, 0.0, 0.0}};
        if (j < n) {
            hd.c = static_cast<uint32_t>(region_entry(s_scan, b.G, b.R, static_cast<uint32_t>(j)));
            hd.nlev = b.nlev()[hd.c];
            hd.p = b.compose ? 0u : b.cpix()[hd.c];
            hd.term = Col{ldn_if<kNtFold>(&b.term(0)[hd.c]), ldn_if<kNtFold>(&b.term(1)[hd.c]),
                          ldn_if<kNtFold>(&b.term(2)[hd.c])};
        }
        return hd;
    };
    uint32_t rc = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    Head cur = head(static_cast<uint64_t>(rc) * 64u + lane);
    for (; static_cast<uint64_t>(rc) * 64u < n; rc += W) {
        const Head nxt = head(static_cast<uint64_t>(rc + W) * 64u + lane);
        if (cur.nlev >= lo && cur.nlev <= hi) {             // (kNlevRunning: not ended yet, or no chain)
            const Col folded = fold_levels<kFresnel, kPack>(sc, b, cur.c, static_cast<int>(cur.nlev), cur.term);
            const Col res = kAa ? aa_sample(folded) : average_samples(folded, fp.spp);
            emit_chain<kAa, kMom>(fp, b, cur.c, cur.p, res, s_srgb);
        }
        cur = nxt;
    }
}

// The first of the two sky passes of a skybox scene (both timed under
// RT_KF_COMPOSE; the other is wf_sky_pixels, wf_output.hip), so that no traversal kernel and no
// fold fetches a texel.
//
// wf_sky_term, before a fold: every chain that ended on a miss (nlev carries kNlevSky, term the
// missing ray's direction: set_sky_terminal) gets its terminal colour, the skybox in that direction
// (Background::color reads nothing else of the ray), and its plain level count.  Chains dealt as
// wf_fold deals them; a chain still running (kNlevRunning) or ended on a colour is left alone, so
// the pass may run before the early fold of the fused tail and again before the last one.
__global__ __launch_bounds__(RT_FOLD_THREADS) void wf_sky_term(DevScene sc, WfBufs b) {
    constexpr int kT = RT_FOLD_THREADS;
    __shared__ uint32_t s_scan[kMaxRegions + 1];
    __shared__ uint32_t s_wave[kT / 64];
    region_scan<kT>(b.rs(), b.G, s_scan, s_wave);
    const uint32_t n = s_scan[b.G];
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kT + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kT) {
        const uint32_t c = static_cast<uint32_t>(region_entry(s_scan, b.G, b.R, static_cast<uint32_t>(j)));
        const uint32_t nl = b.nlev()[c];
        if (nl == kNlevRunning || !(nl & kNlevSky)) continue;
        const Col col = background(sc, Ray{0.0, 0.0, 0.0, b.term(0)[c], b.term(1)[c], b.term(2)[c]});
        b.term(0)[c] = col.r; b.term(1)[c] = col.g; b.term(2)[c] = col.b;
        b.nlev()[c] = static_cast<uint8_t>(nl & ~kNlevSky);
    }
}

}  // namespace

hipError_t launch_fold(const DevScene& sc, const FrameParams& fp, const WfBufs& b, hipStream_t s, LaunchMarks* m,
                       uint32_t lo, uint32_t hi, bool packed) {
    hipError_t e;
    const dim3 grid(b.G * (kWfThreads / RT_FOLD_THREADS)), block(RT_FOLD_THREADS);
    if (sc.skybox) {                           // the terminals of the chains that ended on a miss
        if (m && (e = m->begin(s)) != hipSuccess) return e;
        hipLaunchKernelGGL(wf_sky_term, grid, block, 0, s, sc, b);
        if (m && (e = m->mark(s, kKfCompose)) != hipSuccess) return e;
    }
    if (m && (e = m->begin(s)) != hipSuccess) return e;
    // kAa (RT_ALGO_WAVEFRONT_AA): the sample's colour to the running sums
    (void)dispatch_bools(
        [&](auto kFresnel, auto kAa, auto kPack, auto kMom) {
            if constexpr (kMom() && !kAa()) {                  // (kMom: a moments accumulator's passes only)
                return hipErrorInvalidValue;
            } else {
                hipLaunchKernelGGL((wf_fold<kFresnel(), kAa(), kPack(), kMom()>), grid, block, 0, s, sc, fp, b, lo, hi);
                return hipSuccess;
            }
        },
        sc.has_fresnel, fp.aa_acc != nullptr, packed, aa_moments(fp));
    return m ? m->mark(s, kKfFold) : hipGetLastError();
}

RT_UNIT_WARM(wf_fold)
RT_UNIT_SRGB(wf_fold)

}  // namespace rtamd
