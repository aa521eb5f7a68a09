// The nearest-hit kernel of the wavefront schedule, wf_nearest, and its launcher
// launch_nearest_src<kSrc>.  The kernel's instantiations (24 per sphere source, 16 per camera-grid
// source) are most of the library's device code, so they are spread over several translation
// units that compile side by side: each wf_nearest_*.hip includes this header and instantiates
// the launcher for its group of sources (RT_NEAREST_UNIT).
#pragma once
#include "wf_device.hpp"
#include "wf_launch.hpp"

namespace rtamd {

// RT_STAMP=1 (diagnostic builds only, tools/stamp_probe.py): per generation,
// wf_nearest's wave-cycles by phase from s_memtime stamps taken after a full
// wait, [k][0] setup (region scan + LDS staging), [1] ray load + region entry,
// [2] traversal, [3] finish (records, rays, terminals), [4] chunks, [5] waves;
// the counting kernels add [6] the slowest lane's and [7] all lanes' node
// visits per chunk (divergence); [8..10] the traversal's descend / leaf / pop
// loops (wave-cycles), [12] the slowest wave's traversal cycles, [13..15] the
// waves' iterations of those three loops.  Read with rt_debug_stamps (this
// build only), which adds up the arrays of the wf_nearest_*.hip units (field 12: their maximum).
#ifndef RT_STAMP
#define RT_STAMP 0
#endif
#if RT_STAMP
// (fields 12.. in a second array: a [kMaxGenerations][16] array hits a gfx950
// backend error, "Operand has incorrect register class")
static __device__ unsigned long long g_stamp[kMaxGenerations][12];
static __device__ unsigned long long g_stamp2[kMaxGenerations][4];
#define RT_STAMP_AT(v)                                                            \
    do {                                                                          \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");              \
        v = __builtin_amdgcn_s_memtime();                                         \
    } while (0)
// unit_stamps_<unit>: this unit's arrays to the host, optionally zeroed afterwards
#define RT_UNIT_STAMPS(unit)                                                                                          \
    hipError_t unit_stamps_##unit(unsigned long long (*a)[12], unsigned long long (*b)[4], bool reset) {              \
        hipError_t e;                                                                                                 \
        if ((e = hipMemcpyFromSymbol(a, HIP_SYMBOL(g_stamp), sizeof g_stamp)) != hipSuccess) return e;                \
        if ((e = hipMemcpyFromSymbol(b, HIP_SYMBOL(g_stamp2), sizeof g_stamp2)) != hipSuccess) return e;              \
        if (!reset) return hipSuccess;                                                                                \
        static unsigned long long za[kMaxGenerations][12], zb[kMaxGenerations][4];                                    \
        if ((e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), za, sizeof za)) != hipSuccess) return e;                      \
        return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp2), zb, sizeof zb);                                                \
    }
#else
#define RT_STAMP_AT(v) ((void)0)
#define RT_UNIT_STAMPS(unit)
#endif

// What a wf_nearest_*.hip unit carries beside its instantiations.
#define RT_NEAREST_UNIT(unit) RT_UNIT_WARM(unit) RT_UNIT_SRGB(unit) RT_UNIT_STAMPS(unit)

namespace {

// What follows a nearest hit (all 64 lanes call it; `live` lanes carry a
// query): a miss or a cut-off ends the chain at once (terminal colour; a
// camera ray that ends writes its final pixel); a lit hit becomes a shade
// record of generation k, and a specular one also queues its reflection ray in
// Q_{k+1}.  counts[0..1]: this workgroup's LDS append counters (records, rays).
// Chains: a lit camera hit starts chain c = its record's entry (generation 0,
// pixel cpix[c]); its records, reflection rays, levels and terminal carry c
// (`p` is the pixel for kCam, the chain otherwise), so the levels and
// terminals of a generation are written in about the order of its records.
// kAa (kCam only): a camera ray that ends adds its sample's colour to the pixel's running sum.
// kSky (a skybox scene's instantiations): a miss is not a constant.  A later
// generation's leaves the ray's direction as the chain's terminal (set_sky_terminal); a camera
// ray's is noted in pmap (compose, as ever) or csky, and wf_compose / wf_aa_compose / wf_sky_pixels
// rebuild the ray and write the pixel or add its sample.
// kMom (kAa only): ... and its square to the running sum of squares (aa_add<true>).
template <bool kCam, bool kFresnel, bool kAa = false, bool kSky = false, bool kMom = false>
__device__ __forceinline__ void finish_nearest(const DevScene& sc, const FrameParams& fp, const WfBufs& b,
                                               const DevSphere* sph, int k, bool live, const Ray& r, double sig,
                                               uint32_t p, const Hit& h, uint32_t* counts, size_t obase, size_t rbase) {
    bool shade = false, refl = false;
    double ptx = 0.0, pty = 0.0, ptz = 0.0, nsig = 0.0;
    Ray rr{};
    // a chain that ends here without lighting: background (end_obj INT32_MAX) or the
    // object's ambient colour
    bool ends = false;
    int32_t end_obj = INT32_MAX;
    if (live) {
        if (h.obj == INT32_MAX) {                                           // raytrace.rs:265, 228-232
            if constexpr (kCam) {                                           // no levels: final now
                if (b.compose) stn(&b.pmap()[p], kPixBackground);
                else if constexpr (kSky) { /* csky below: wf_sky_pixels */ }
                else if constexpr (kAa) aa_add<kMom>(fp, p, Col{fp.aa_bg[0], fp.aa_bg[1], fp.aa_bg[2]});
                else write_background_pixel(fp, b, p);
            } else if constexpr (kSky) {
                set_sky_terminal(b, p, r, k);
            } else {
                ends = true;
            }
        } else {
            const DevMaterial& m = sc.mats[h.obj];
            if (static_cast<uint32_t>(k) > fp.max_depth) {                  // raytrace.rs:33 / 126
                ends = true;
                end_obj = h.obj;
            } else {
                ptx = r.ox + r.dx * h.t; pty = r.oy + r.dy * h.t; ptz = r.oz + r.dz * h.t;   // ray.cast(t)
                double nx, ny, nz;
                hit_normal(sc, sph, h.prim, ptx, pty, ptz, nx, ny, nz);
                const double nd = nx * r.dx + ny * r.dy + nz * r.dz;
                const Shading sh = shading_flags<kFresnel>(m, sig, nd);
                if (!sh.diffuse && !sh.specular) {
                    ends = true;
                    end_obj = h.obj;
                } else {
                    shade = true;
                    if (sh.specular) {                                      // raytrace.rs:58-64 / 159-164
                        if (nd > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
                        rr = reflect_ray(r, ptx, pty, ptz, nx, ny, nz);
                        nsig = (sh.f * sig) * m.ks_sig;
                        refl = true;
                    }
                }
            }
        }
    }
    if (ends) {
        if constexpr (kCam) {                              // no levels: the final pixel now
            if (b.compose) stn(&b.pmap()[p], kPixAmbient | static_cast<uint32_t>(end_obj));
            else if constexpr (kAa) aa_add<kMom>(fp, p, aa_sample(end_colour(sc, end_obj)));
            else write_pixel(fp, p % fp.tile_w, fp.row0 + p / fp.tile_w, average_samples(end_colour(sc, end_obj), fp.spp));
        } else {
            set_terminal(b, p, end_colour(sc, end_obj), k);
        }
    }
    if constexpr (kCam) {
        if (b.mark && live) stn(&b.cmark()[p], static_cast<uint8_t>(shade ? 1 : 0));
        if constexpr (kSky) {
            if (!b.compose && live) stn(&b.csky()[p], static_cast<uint8_t>(h.obj == INT32_MAX ? 1 : 0));
        }
    }
    const uint32_t slot = lds_append(&counts[0], shade);
    const uint32_t chain = kCam ? static_cast<uint32_t>(obase) + slot : p;   // (slot valid when shade)
    if (kCam && shade && b.compose) stn(&b.pmap()[p], chain);
    if (shade) {
        const size_t at = rbase + slot;
        stn(&b.rf(0)[at], ptx); stn(&b.rf(1)[at], pty); stn(&b.rf(2)[at], ptz);
        stn(&b.rf(3)[at], r.dx); stn(&b.rf(4)[at], r.dy); stn(&b.rf(5)[at], r.dz);
        stn(&b.rf(6)[at], sig);
        stn(&b.ru(0)[at], static_cast<uint32_t>(h.obj));
        stn(&b.ru(1)[at], static_cast<uint32_t>(h.prim));
        stn(&b.ru(2)[at], chain);
        stn(&b.ru(3)[at], 0u);
        if constexpr (kCam) {
            stn(&b.cpix()[chain], p);
            b.nlev()[chain] = kNlevRunning;                   // set_terminal gives the level count
        }
    }
    const uint32_t rslot = lds_append(&counts[1], refl);
    if (refl) {
        const int qn = (k + 1) & 1;
        const size_t at = obase + rslot;
        stn(&b.qf(qn, 0)[at], rr.ox); stn(&b.qf(qn, 1)[at], rr.oy); stn(&b.qf(qn, 2)[at], rr.oz);
        stn(&b.qf(qn, 3)[at], rr.dx); stn(&b.qf(qn, 4)[at], rr.dy); stn(&b.qf(qn, 5)[at], rr.dz);
        stn(&b.qf(qn, 6)[at], nsig);
        stn(&b.qpix(qn)[at], chain);
    }
}

// Scene::intersect for every ray of Q_k (generation 0: the camera rays of the
// chunk, computed here).  Outcomes that end the chain without lighting are
// resolved on the spot (miss -> background; depth cut-off or insignificant
// surface -> ambient, raytrace.rs:32-35); the rest become shade records of
// generation k in this workgroup's region, and a specular hit also appends
// its reflection ray (raytrace.rs:58-64) to Q_{k+1} right here: the next
// generation depends only on the hit, never on the shadow rays or the Phong
// sum, so those run on the other stream, off the critical path.
template <int kSrc, bool kCam, bool kCount, bool kFresnel, bool kAa = false, bool kSky = false, bool kMom = false>
__global__ __launch_bounds__(kWfThreads, Src<kSrc>::waves) void wf_nearest(DevScene sc, FrameParams fp, WfBufs b, int k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
#ifndef RT_NEAR_PRIO
#define RT_NEAR_PRIO 2
#endif
    // the nearest-hit chain is the frame's critical path: its waves win issue
    // arbitration over the shadow / shading waves sharing a SIMD
    if (RT_NEAR_PRIO) __builtin_amdgcn_s_setprio(RT_NEAR_PRIO);
    [[maybe_unused]] unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0, acc[6] = {0, 0, 0, 0, 0, 0};
    RT_STAMP_AT(st0);
    const QueueLds ql = queue_lds(lds + staged_bytes<kSrc>(sc), b.G);
    if (threadIdx.x < kQueueCounters) ql.count[threadIdx.x] = 0;
    uint32_t n;
    if constexpr (kCam) {
        n = b.slots;
    } else {
        region_scan(b.rq() + k * b.G, b.G, ql.scan, ql.wave);
        n = ql.scan[b.G];
    }
    if (!wg_has_work(b, n)) {                  // nothing dealt here: publish empty regions, free the CU
        if (threadIdx.x == 0) {
            b.rs()[k * b.G + blockIdx.x] = 0;
            b.rq()[(k + 1) * b.G + blockIdx.x] = 0;
        }
        return;
    }
    const BvhView v = stage_lds<kSrc, true>(sc, lds);
    __syncthreads();                                       // publishes the LDS staging and counters
    RT_STAMP_AT(st1);
    acc[0] = st1 - st0;
    Work w;
    const size_t obase = static_cast<size_t>(blockIdx.x) * b.R;
    const size_t rbase = static_cast<size_t>(k) * b.qcap + obase;
    RT_FOR_CHUNKS(b, n, j) {
        RT_STAMP_AT(st0);
        [[maybe_unused]] const uint32_t visits0 = w.boxes;
        Ray r{};
        double sig = 0.0;
        uint32_t p = 0;
        Hit h{};
        bool live = false;
        if (j < n) {
            if constexpr (kCam) {
                uint32_t lx, ly;
                if (slot_pixel(b, fp, j, lx, ly)) {
                    r = camera_ray(sc, fp, lx, fp.row0 + ly, fp.aa_pass);
                    sig = 1.0;                              // raytrace.rs:273 via main.rs:54
                    p = ly * fp.tile_w + lx;
                    live = true;
                }
            } else {
                const size_t at = region_entry(ql.scan, b.G, b.R, j);
                r = load_ray(b, k & 1, at);
                sig = ldn_if<kNtQ>(&b.qf(k & 1, 6)[at]);
                p = ldn_if<kNtQ>(&b.qpix(k & 1)[at]);
                live = true;
            }
        }
        RT_STAMP_AT(st1);
        if (live) h = nearest_any<kSrc, kCount>(sc, v, r, &w);
        RT_STAMP_AT(st2);
        finish_nearest<kCam, kFresnel, kAa, kSky, kMom>(sc, fp, b, v.sph, k, live, r, sig, p, h, ql.count, obase, rbase);
        RT_STAMP_AT(st3);
#if RT_STAMP
        acc[1] += st1 - st0; acc[2] += st2 - st1; acc[3] += st3 - st2; acc[4] += 1;
        if constexpr (kCount) {
            unsigned long long mx = (w.boxes - visits0) / 2, sm = mx;
            for (int off = 32; off > 0; off >>= 1) {
                mx = max(mx, static_cast<unsigned long long>(__shfl_xor(mx, off, 64)));
                sm += __shfl_xor(sm, off, 64);
            }
            if ((threadIdx.x & 63) == 0) { atomicAdd(&g_stamp[k][6], mx); atomicAdd(&g_stamp[k][7], sm); }
        }
#endif
    }
#if RT_STAMP
    for (int q = 0; q < 3; ++q)               // the wave's time in each loop = its longest-running lane's
        for (int off = 32; off > 0; off >>= 1)
            w.cyc[q] = max(w.cyc[q], static_cast<unsigned long long>(__shfl_xor(w.cyc[q], off, 64)));
    if ((threadIdx.x & 63) == 0) {
        for (int q = 0; q < 5; ++q) atomicAdd(&g_stamp[k][q], acc[q]);
        atomicAdd(&g_stamp[k][5], 1ull);
        for (int q = 0; q < 3; ++q) atomicAdd(&g_stamp[k][8 + q], w.cyc[q]);
        atomicMax(&g_stamp2[k][0], acc[2]);
    }
    for (int q = 0; q < 3; ++q) {
        unsigned long long ws = w.wsteps[q];
        for (int off = 32; off > 0; off >>= 1) ws += __shfl_xor(ws, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_stamp2[k][1 + q], ws);
    }
#endif
    __syncthreads();
    if (threadIdx.x == 0) {
        b.rs()[k * b.G + blockIdx.x] = ql.count[0];
        b.rq()[(k + 1) * b.G + blockIdx.x] = ql.count[1];
    }
    flush_work<kCount>(b, 2, w);
}

}  // namespace

// Generation 0 (kCam) computes the chunk's camera rays; the camera pass of RT_ALGO_WAVEFRONT_AA
// (fp.aa_acc) and a skybox scene (kSky) have instantiations of their own, the others are untouched.
template <int kSrc>
hipError_t launch_nearest_src(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, bool count, hipStream_t s) {
    const size_t lds = staged_bytes<kSrc>(sc) + queue_lds_bytes(b.G);
    const bool cam = k == 0;
    return dispatch_bools(
        [&](auto kCam, auto kCount, auto kFresnel, auto kAa, auto kSky, auto kMom) {
            // kAa exists only with kCam, kMom only with kAa, and a camera-grid source only as the camera pass
            if constexpr ((!kCam() && (kAa() || Src<kSrc>::cgrid)) || (kMom() && !kAa())) {
                return hipErrorInvalidValue;
            } else {
                hipLaunchKernelGGL((wf_nearest<kSrc, kCam(), kCount(), kFresnel(), kAa(), kSky(), kMom()>), dim3(b.G),
                                   dim3(kWfThreads), lds, s, sc, fp, b, k);
                return hipSuccess;
            }
        },
        cam, count, sc.has_fresnel, cam && fp.aa_acc, sc.skybox, cam && aa_moments(fp));
}

}  // namespace rtamd
