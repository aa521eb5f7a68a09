// Host-side sequencing of the wavefront schedule: one chunk through every generation on its
// lane's streams (launch_wavefront), the stream joins, and what concerns every code object of the
// kernel translation units (warm-up, the sRGB table, the RT_STAMP counters).  The kernels of the
// generations live in the family units (wf_nearest_*.hip, wf_shade.hip, wf_tail.hip, wf_fold.hip,
// wf_output.hip) and are reached through wf_launch.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "wf_device.hpp"
#include "wf_launch.hpp"

namespace rtamd {

// Stream a waits for the work issued so far on the b streams of mask (those that are
// not stream a itself): through events, or on the device (ws.dj_flags: launch_signal on
// each, one launch_join on a).
static hipError_t join_b(const WfStreams& ws, uint32_t mask) {
    hipError_t e;
    uint32_t m = 0;
    for (int i = 0; i < ws.nb; ++i)
        if (((mask >> i) & 1u) && ws.b[i] != ws.a) m |= 1u << i;
    if (!m) return hipSuccess;
    if (ws.dj_flags) {
        const uint64_t n = ++*ws.dj_next;
        for (int i = 0; i < ws.nb; ++i)
            if (((m >> i) & 1u) && (e = launch_signal(ws.dj_flags + i, n, ws.b[i])) != hipSuccess) return e;
        return launch_join(ws.dj_flags, m, n, ws.dj_err, ws.a);
    }
    for (int i = 0; i < ws.nb; ++i) {
        if (!((m >> i) & 1u)) continue;
        if ((e = hipEventRecord(ws.b_done[i], ws.b[i])) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(ws.a, ws.b_done[i], 0)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// wf_nearest of generation k: through the camera's view grid (generation 0, ws.cam 3 / 4: the
// spheres in LDS / through L2) or from sphere source src.
static hipError_t launch_nearest(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, int src, int cam,
                                 bool count, hipStream_t s) {
    if (k == 0 && cam == 3) return launch_nearest_src<kSrcCamGridL>(sc, fp, b, k, count, s);
    if (k == 0 && cam == 4) return launch_nearest_src<kSrcCamGridG>(sc, fp, b, k, count, s);
    switch (src) {
    case kSrcGlobal: return launch_nearest_src<kSrcGlobal>(sc, fp, b, k, count, s);
    case kSrcLds: return launch_nearest_src<kSrcLds>(sc, fp, b, k, count, s);
    case kSrcBvhL8: return launch_nearest_src<kSrcBvhL8>(sc, fp, b, k, count, s);
    case kSrcBvhL8C: return launch_nearest_src<kSrcBvhL8C>(sc, fp, b, k, count, s);
    case kSrcBvhPH: return launch_nearest_src<kSrcBvhPH>(sc, fp, b, k, count, s);
    case kSrcBvhPHC: return launch_nearest_src<kSrcBvhPHC>(sc, fp, b, k, count, s);
    case kSrcBvhP: return launch_nearest_src<kSrcBvhP>(sc, fp, b, k, count, s);
    case kSrcQ4: return launch_nearest_src<kSrcQ4>(sc, fp, b, k, count, s);
    case kSrcQ4P: return launch_nearest_src<kSrcQ4P>(sc, fp, b, k, count, s);
    default: return launch_nearest_src<kSrcBvhG>(sc, fp, b, k, count, s);
    }
}

// Generation k of a chunk: its nearest-hit launch on stream a, then its shadow and shading
// launches on a b stream; or, from generation ws.tail_fuse on, the fused tail.
static hipError_t launch_generation(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, int src, int src_occ,
                                    bool count, const WfStreams& ws) {
    hipError_t e;
    const bool packed = levels_packed(ws.tail_fuse);
    if (ws.tail_fuse > 0 && k >= ws.tail_fuse) {      // the fused tail: every generation >= T in one launch
        if (k > ws.tail_fuse) return hipSuccess;
        // the tail folds its chains: the levels of generations <= T-2 (the B streams) must be written
        if ((e = join_b(ws, (1u << ws.nb) - 1u)) != hipSuccess) return e;
        // the chains that ended by generation T-1, folded on a B stream while the tail runs
        if (ws.b[0] != ws.a) {
            if ((e = hipEventRecord(ws.near_done[k], ws.a)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(ws.b[0], ws.near_done[k], 0)) != hipSuccess) return e;
        }
        if ((e = launch_fold(sc, fp, b, ws.b[0], ws.b[0] != ws.a ? ws.mb[0] : ws.ma, 0u, static_cast<uint32_t>(k - 1),
                             packed)) != hipSuccess)
            return e;
        if (ws.ma && (e = ws.ma->begin(ws.a)) != hipSuccess) return e;
        if ((e = launch_tail(sc, fp, b, k, count, packed, ws.tail_wgs, ws.tail_width, ws.a)) != hipSuccess) return e;
        return ws.ma ? ws.ma->mark(ws.a, kKfTail) : hipGetLastError();
    }
    e = ws.ma ? ws.ma->begin(ws.a) : hipSuccess;
    if (e != hipSuccess) return e;
    if ((e = launch_nearest(sc, fp, b, k, src, ws.cam, count, ws.a)) != hipSuccess) return e;
    e = ws.ma ? ws.ma->mark(ws.a, k == 0 ? kKfCamera : kKfNearest) : hipSuccess;
    if (e != hipSuccess) return e;
    if (static_cast<uint32_t>(k) > fp.max_depth) return hipSuccess;    // no shade records past the cut-off
    // the fused tail shades the records of generation T-1 itself
    if (ws.tail_fuse > 0 && k >= ws.tail_fuse - 1) return hipSuccess;
    // shadows and shading of generation k: on a b stream once nearest_k is done
    // (generations alternate over the b streams, so consecutive ones overlap too)
    const int bi = k % ws.nb;
    const hipStream_t sb = ws.b[bi];
    if (sb != ws.a) {
        if ((e = hipEventRecord(ws.near_done[k], ws.a)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(sb, ws.near_done[k], 0)) != hipSuccess) return e;
    }
    return launch_shading(sc, fp, b, k, src_occ, ws.grid_occ, count, packed, sb, ws.mb[bi]);
}

// One chunk (fp.row0, fp.rows) through every generation.  src: the sphere
// source of the nearest-hit kernel (kSrc*), src_occ: of the shadow kernel;
// count: instrumented kernels; mark is recorded on stream a after generation
// mark_gen has been launched (chunk pipelining across lanes).  The nearest-hit
// chain runs on ws.a, the shadow + shading kernels of each generation on ws.b
// streams (each waiting for its generation's nearest-hit kernel); the fold
// waits for all of them.  Supported (src, src_occ) pairs: (0, 0), (1, 1),
// (2, 2), (7, 7), (7, 10), (9, 10), (2, 11), (5, 11), (6, 11), (8, 11), (25, 11),
// (26, 11); any other pair runs as (2, 11).
hipError_t launch_wavefront(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int src, int src_occ,
                            bool count, const WfStreams& ws, hipEvent_t mark, int mark_gen) {
    static constexpr int kPairs[][2] = {
        {kSrcGlobal, kSrcGlobal}, {kSrcLds, kSrcLds},      {kSrcBvhG, kSrcBvhG},    {kSrcBvhL8, kSrcBvhL8},
        {kSrcBvhL8, kSrcBvh4L},   {kSrcBvhL8C, kSrcBvh4L}, {kSrcBvhG, kSrcBvh4G},   {kSrcBvhPH, kSrcBvh4G},
        {kSrcBvhPHC, kSrcBvh4G},  {kSrcBvhP, kSrcBvh4G},   {kSrcQ4, kSrcBvh4G},     {kSrcQ4P, kSrcBvh4G}};
    const bool supported = std::any_of(std::begin(kPairs), std::end(kPairs),
                                       [&](const int (&p)[2]) { return p[0] == src && p[1] == src_occ; });
    if (!supported) { src = kSrcBvhG; src_occ = kSrcBvh4G; }
    const int gens = static_cast<int>(fp.max_depth) + 2;          // depths 0 .. max_depth+1
    for (int k = 0; k < gens; ++k) {
        hipError_t e;
        if ((e = launch_generation(sc, fp, b, k, src, src_occ, count, ws)) != hipSuccess) return e;
        // a skybox scene's camera misses (compose: wf_compose / wf_aa_compose write them)
        if (k == 0 && sc.skybox && !b.compose && (e = launch_sky_pixels(sc, fp, b, ws.a, ws.ma)) != hipSuccess) return e;
        if (k == 0 && ws.sp_s) {               // every pixel without a chain is final now
            if ((e = hipEventRecord(ws.sp_cam, ws.a)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(ws.sp_s, ws.sp_cam, 0)) != hipSuccess) return e;
            if ((e = launch_chain_segs(fp, b, ws.sp_bits, ws.sp_cnt, ws.sp_off, ws.sp_s)) != hipSuccess) return e;
            if ((e = hipEventRecord(ws.sp_ready, ws.sp_s)) != hipSuccess) return e;
        }
        if (mark && k == mark_gen) {
            e = hipEventRecord(mark, ws.a);
            if (e != hipSuccess) return e;
        }
    }
    hipError_t e;
    // the tally reads only the queue sizes: on stream a while the b streams finish the last shading
    // (or later, when statistics are asked for: ws.lazy_tally)
    if (!ws.lazy_tally) {
        if (ws.ma && (e = ws.ma->begin(ws.a)) != hipSuccess) return e;
        if ((e = launch_tally(fp, b, sc.n_lights, gens, ws.a)) != hipSuccess) return e;
        if (ws.ma && (e = ws.ma->mark(ws.a, kKfTally)) != hipSuccess) return e;
    }
    // the b streams' work joins stream a (with the fused tail only b[0]'s early fold is left: the
    // tail's launch already waited for every b stream, and none has had work since)
    if ((e = join_b(ws, ws.tail_fuse > 0 ? 1u : (1u << ws.nb) - 1u)) != hipSuccess) return e;
    // the chains not folded yet (all of them without the fused tail, which folded every chain:
    // its own as it ended them, the others on a B stream)
    if (ws.tail_fuse == 0 &&
        (e = launch_fold(sc, fp, b, ws.a, ws.ma, 0u, kNlevRunning - 1u, levels_packed(ws.tail_fuse))) != hipSuccess)
        return e;
    // the compose route: the frame, row by row, once every chain has its colour; or,
    // RT_ALGO_WAVEFRONT_AA, the pass's samples to the running sums (without compose the pass has
    // added them already)
    if (b.compose) {
        if (ws.ma && (e = ws.ma->begin(ws.a)) != hipSuccess) return e;
        if ((e = launch_compose(sc, fp, b, ws.a)) != hipSuccess) return e;
        if (ws.ma && (e = ws.ma->mark(ws.a, kKfCompose)) != hipSuccess) return e;
    }
    // RT_ALGO_WAVEFRONT_AA: after the chunk's last pass the resolve writes the chunk's rows
    if (fp.aa_acc && fp.aa_pass + 1 == fp.aa_spp) {
        if (ws.ma && (e = ws.ma->begin(ws.a)) != hipSuccess) return e;
        if ((e = launch_accum_resolve(fp, 4u * b.G, ws.a)) != hipSuccess) return e;
        if (ws.ma && (e = ws.ma->mark(ws.a, kKfCompose)) != hipSuccess) return e;
    }
    if (ws.sp_s) {                           // the chain pixels' segments, packed in row order
        if ((e = hipStreamWaitEvent(ws.a, ws.sp_ready, 0)) != hipSuccess) return e;
        if ((e = launch_chain_pack(fp, ws.sp_bits, ws.sp_off, ws.sp_bgr, ws.sp_rgb, ws.a)) != hipSuccess) return e;
    }
    // every row of the chunk is final now (the fold runs in chain order, not by rows)
    if (ws.fold_ev && (e = hipEventRecord(*ws.fold_ev, ws.a)) != hipSuccess) return e;
    return hipGetLastError();
}

// Device-side join of b streams into stream a (WfStreams::dj_flags): a b stream
// ends its share with wf_signal (one work-item stores the join's number into
// the stream's flag word once the kernels before it on that stream are done:
// in-order stream), and stream a runs wf_join, one wave whose lane i polls
// flag i until it reaches the number.  Instead of an event record on the b
// stream and a barrier packet on stream a: the cross-queue event wait measured
// ~50 us between the b stream's last kernel and stream a's next one, a kernel
// boundary on one queue ~8 us.  Flags only grow (one number per join, from
// the host), so they need no reset.  A join that has waited kJoinTimeout
// (100 MHz ticks) gives up and sets the error word (a page-locked host word,
// reported by the next rt_render or rt_ctx_stats): the stream goes on rather
// than hang the device.
constexpr uint64_t kJoinTimeout = 200000000ull;      // 2 s
__global__ __launch_bounds__(64) void wf_signal(uint64_t* flag, uint64_t n) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(64) void wf_join(uint64_t* flags, uint32_t mask, uint64_t n, uint64_t* err) {
    const uint32_t i = threadIdx.x;
    if (i < kDjFlags && ((mask >> i) & 1u)) {
        const uint64_t t0 = wall_clock64();
        while (__hip_atomic_load(&flags[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < n) {
            __builtin_amdgcn_s_sleep(1);
            if (wall_clock64() - t0 > kJoinTimeout) {       // err: a page-locked host word the host reads directly
                __hip_atomic_store(err, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
    }
}

hipError_t launch_signal(uint64_t* flag, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(wf_signal, dim3(1), dim3(64), 0, s, flag, n);
    return hipGetLastError();
}

hipError_t launch_join(uint64_t* flags, uint32_t mask, uint64_t n, uint64_t* err, hipStream_t s) {
    hipLaunchKernelGGL(wf_join, dim3(1), dim3(64), 0, s, flags, mask, n, err);
    return hipGetLastError();
}

// rt_ctx_reserve: one launch on a stream has the runtime set up the stream's hardware queue,
// including the queue's scratch, which it sizes at the first launch that needs private memory:
// kWarmScratch bytes per lane, at least what any wavefront kernel spills or stacks (DESIGN.md
// §3.4: 128-208 B).  A code object is loaded by its first launch, so launch_warmup also runs the
// empty kernel of every other kernel translation unit (RT_WARM_UNITS): no frame pays for a load.
constexpr uint32_t kWarmScratch = 256;
__global__ __launch_bounds__(kWfThreads) void wf_warm(uint32_t* sink, uint32_t salt) {
    volatile uint32_t priv[kWarmScratch / 4];       // volatile + a lane-dependent index: kept in scratch
    const uint32_t i = (threadIdx.x * 7u + salt) % (kWarmScratch / 4);
    priv[i] = salt;
    if (priv[(i + salt) % (kWarmScratch / 4)] == 0xfeedf00du && sink) sink[blockIdx.x] = salt;
}

hipError_t launch_warmup(uint32_t workgroups, hipStream_t s) {
    hipLaunchKernelGGL(wf_warm, dim3(std::max(1u, workgroups)), dim3(kWfThreads), 0, s, nullptr, 1u);
    hipError_t e = hipGetLastError();
#define RT_X(unit) if (e == hipSuccess) e = unit_warm_##unit(s);
    RT_WARM_UNITS(RT_X)
#undef RT_X
    return e;
}

hipError_t upload_srgb_table(const double* avg255) {
    hipError_t e = hipSuccess;
#define RT_X(unit) if (e == hipSuccess) e = unit_srgb_##unit(avg255);
    RT_SRGB_UNITS(RT_X)
#undef RT_X
    return e;
}

#if RT_STAMP
#define RT_X(unit) hipError_t unit_stamps_##unit(unsigned long long (*a)[12], unsigned long long (*b)[4], bool reset);
RT_NEAREST_UNITS(RT_X)
#undef RT_X
}  // namespace rtamd
extern "C" int rt_debug_stamps(unsigned long long* out, int n, int reset) {
    // out: 16 fields per generation, summed over the wf_nearest_*.hip units (one source runs per
    // render, so at most one unit's are not zero); field 12 is a maximum
    static unsigned long long a[rtamd::kMaxGenerations][12], b[rtamd::kMaxGenerations][4];
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    for (int i = 0; i < n && i < 16 * rtamd::kMaxGenerations; ++i) out[i] = 0;
#define RT_X(unit)                                                                                \
    if (rtamd::unit_stamps_##unit(a, b, reset != 0) != hipSuccess) return -3;                     \
    for (int i = 0; i < n && i < 16 * rtamd::kMaxGenerations; ++i) {                              \
        const unsigned long long v = (i % 16) < 12 ? a[i / 16][i % 16] : b[i / 16][i % 16 - 12]; \
        out[i] = i % 16 == 12 ? std::max(out[i], v) : out[i] + v;                                 \
    }
    RT_NEAREST_UNITS(RT_X)
#undef RT_X
    return 0;
}
namespace rtamd {
#endif

}  // namespace rtamd
