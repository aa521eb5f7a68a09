// Device code that more than one kernel family of the wavefront schedule uses: the queue and LDS
// infrastructure, the sphere sources, the level and terminal helpers and the row writers.  Included
// by the wf_*.hip translation units; everything is inlined into their kernels (internal linkage).
//
// The wavefront schedule (wf_*): one generation per recursion depth k.  Queue Q_k in HBM
// holds exactly the rays ray_color is called with at depth k; per
// generation:
//     wf_nearest    Scene::intersect for every ray of Q_k (scene.rs:247-249)
//                   and compaction of the hits that need light evaluation
//     wf_occlusion  the shadow queries of those hits (raytrace.rs:41-49)
//     wf_shade      the Phong sum (raytrace.rs:31-56), push of the level's
//                   local colour, compaction of the reflection rays into
//                   Q_{k+1} (raytrace.rs:58-64)
// then wf_fold evaluates `res + ks * ray_color(child)` inner-first from the
// per-pixel level stack (bit-exact, raytrace.rs:63) and writes f32 RGB +
// sRGB BGR.  Every lane of every launch holds a live ray: no divergence over
// path length, small kernels, high occupancy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "trace_common.hpp"

namespace rtamd {
namespace {

// Queues are BLOCK-PARTITIONED: a queue of generation k is G regions of R
// entries, region r written only by workgroup r of the producing kernel
// (appending through an LDS counter) and its size published in rq/rs[k*G+r].
// No global atomic sits on the data path: a single global queue counter
// serialises at ~88 atomics/us (MI355X_MICROARCH.md, "dequeue") and was the
// measured bottleneck of the first version.  Consumers read the queue DENSELY:
// each workgroup scans the G region sizes into LDS and maps item i to
// (region, offset) by binary search, so small tail queues still fill whole
// waves.  Every queue kernel runs exactly G workgroups of kWfThreads and
// grid-strides over its items, so workgroup b produces at most R outputs.

// Wave-aggregated append to an LDS counter: one LDS atomic per wave, lanes
// get consecutive slots in lane order.  All 64 lanes must call it.
__device__ __forceinline__ uint32_t lds_append(uint32_t* counter, bool want) {
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return 0xFFFFFFFFu;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll(static_cast<long long>(mask)) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, static_cast<uint32_t>(__popcll(mask)));
    base = __shfl(base, leader, 64);
    const uint32_t below = static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
    return want ? base + below : 0xFFFFFFFFu;
}

// Work dealing: a queue is consumed in 64-item chunks; chunk c goes to wave
// slot c mod W (W = G * 16 waves).  Slots are numbered workgroup-first
// (b.wg_major = 0: a small tail queue spreads over every workgroup) or
// workgroup-major (b.wg_major = 1: consecutive chunks fill one workgroup's
// waves, so the workgroups past the queue's end exit at once and free their
// CU for the kernels of the other stream).  Either way a workgroup takes at
// most 16 chunks per round of W, i.e. at most R items.  Loop condition and
// chunk are wave-uniform.
// A queue smaller than b.spread_below items is always dealt workgroup-first
// (its few chunks then occupy every CU instead of a few whole workgroups).
__device__ __forceinline__ bool deal_major(const WfBufs& b, uint32_t n) { return b.wg_major && n >= b.spread_below; }

__device__ __forceinline__ uint32_t wave_slot(const WfBufs& b, uint32_t n) {
    const uint32_t wave = threadIdx.x >> 6;
    return deal_major(b, n) ? blockIdx.x * (kWfThreads / 64) + wave : wave * b.G + blockIdx.x;
}

// Whether this workgroup's first chunk is below n (workgroup-uniform).
__device__ __forceinline__ bool wg_has_work(const WfBufs& b, uint32_t n, uint32_t width = 64) {
    const uint64_t first = deal_major(b, n) ? static_cast<uint64_t>(blockIdx.x) * (kWfThreads / 64) : blockIdx.x;
    return first * width < n;
}

#define RT_FOR_CHUNKS(b, n, j)                                                              \
    for (uint32_t rt_c = wave_slot(b, n), rt_w = (b).G * (kWfThreads / 64);                  \
         static_cast<uint64_t>(rt_c) * 64u < static_cast<uint64_t>(n); rt_c += rt_w)        \
        if (const uint32_t j = rt_c * 64u + (threadIdx.x & 63u); true)

// Exclusive scan of the G region sizes `counts` into s_scan[0..G]
// (s_scan[G] = queue size; G <= kMaxScan: the regions of up to kMaxScan / G
// consecutive generations, laid out one after the other).  s_wave: 16 words.
// Ends with a barrier.
template <int kT = kWfThreads>
__device__ void region_scan(const uint32_t* counts, uint32_t G, uint32_t* s_scan, uint32_t* s_wave) {
    const uint32_t per = (G + kT - 1) / kT;                         // 1 .. 4 (1024 threads), .. 16 (256)
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int kPer = (kMaxScan + kT - 1) / kT;
    uint32_t v[kPer] = {}, sum = 0;
    for (uint32_t e = 0; e < per; ++e) {
        const uint32_t i = t * per + e;
        v[e] = i < G ? counts[i] : 0u;
        sum += v[e];
    }
    uint32_t inc = sum;                                              // inclusive wave scan
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= static_cast<uint32_t>(off)) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (t == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < kT / 64; ++w) { const uint32_t x = s_wave[w]; s_wave[w] = acc; acc += x; }
    }
    __syncthreads();
    uint32_t run = s_wave[wave] + inc - sum;
    for (uint32_t e = 0; e < per; ++e) {
        const uint32_t i = t * per + e;
        if (i < G) s_scan[i] = run;
        run += v[e];
    }
    if (t == kT - 1) s_scan[G] = run;
    __syncthreads();
}

// Dense item i (< s_scan[G]) -> its entry index region * R + offset.
__device__ __forceinline__ size_t region_entry(const uint32_t* s_scan, uint32_t G, uint32_t R, uint32_t i) {
    uint32_t lo = 0, hi = G - 1;                  // largest r with s_scan[r] <= i
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (s_scan[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return static_cast<size_t>(lo) * R + (i - s_scan[lo]);
}

// Generation-0 slot j of the chunk (8x8 tiles, row-major) -> local pixel.
__device__ __forceinline__ bool slot_pixel(const WfBufs& b, const FrameParams& fp, uint32_t j, uint32_t& lx, uint32_t& ly) {
    const uint32_t tile = j >> 6, w = j & 63u;
    lx = (tile % b.tiles_x) * 8u + (w & 7u);
    ly = (tile / b.tiles_x) * 8u + (w >> 3);
    return lx < fp.tile_w && ly < fp.rows;
}

// Streaming accesses (queues, shade records, levels): each word is written once
// and read once by a later launch, so they bypass L2 allocation (nontemporal)
// and leave it to the BVH / sphere lines the traversals re-read.
#ifndef RT_NT
#define RT_NT 1
#endif
template <class T>
__device__ __forceinline__ T ldn(const T* p) {
#if RT_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
template <class T, class U>
__device__ __forceinline__ void stn(T* p, U v) {
#if RT_NT
    __builtin_nontemporal_store(static_cast<T>(v), p);
#else
    *p = static_cast<T>(v);
#endif
}

// RT_NT >= 2: also the shadow-list entries and the shade records' last read;
// RT_NT >= 3: also the shadow kernels' record reads.
template <int kLevel, class T>
__device__ __forceinline__ T ldn_if(const T* p) {
#if RT_NT
    if constexpr (RT_NT >= kLevel) return __builtin_nontemporal_load(p);
#endif
    return *p;
}
template <int kLevel, class T, class U>
__device__ __forceinline__ void stn_if(T* p, U v) {
#if RT_NT
    if constexpr (RT_NT >= kLevel) { __builtin_nontemporal_store(static_cast<T>(v), p); return; }
#endif
    *p = static_cast<T>(v);
}

// the fold's loads (RT_NT_FOLD=1: nontemporal; measured 346 -> 413 us per fold at C3, so plain)
#ifndef RT_NT_FOLD
#define RT_NT_FOLD 0
#endif
constexpr int kNtFold = RT_NT_FOLD ? 1 : 99;
// the queue loads of the nearest-hit kernel (RT_NT_QLOAD=0: plain loads)
#ifndef RT_NT_QLOAD
#define RT_NT_QLOAD 1
#endif
constexpr int kNtQ = RT_NT_QLOAD ? 1 : 99;

__device__ __forceinline__ Ray load_ray(const WfBufs& b, int q, size_t i) {
    return Ray{ldn_if<kNtQ>(&b.qf(q, 0)[i]), ldn_if<kNtQ>(&b.qf(q, 1)[i]), ldn_if<kNtQ>(&b.qf(q, 2)[i]),
               ldn_if<kNtQ>(&b.qf(q, 3)[i]), ldn_if<kNtQ>(&b.qf(q, 4)[i]), ldn_if<kNtQ>(&b.qf(q, 5)[i])};
}

// Occupancy / unrolling of the fold and shading kernels (A/B builds: EXTRA=-D...)
#ifndef RT_FOLD_UNROLL
#define RT_FOLD_UNROLL 4        // levels whose loads are issued together
#endif
#ifndef RT_FOLD_WAVES
#define RT_FOLD_WAVES 1         // wf_fold's launch bounds: min waves per SIMD (1: the compiler's choice, 96 VGPRs)
#endif
#ifndef RT_FOLD_THREADS
#define RT_FOLD_THREADS 256     // wf_fold's workgroup size
#endif
#ifndef RT_SHADE_WAVES
#define RT_SHADE_WAVES 1
#endif

// Sphere sources of the wavefront intersection kernels.
constexpr int kSrcGlobal = 0;       // brute force, sphere list through the caches
constexpr int kSrcLds = 1;          // brute force, sphere list staged in LDS per workgroup
constexpr int kSrcBvhG = 2;         // binary BVH from HBM/L2 (trees too deep for the 4-wide stack)
constexpr int kSrcBvhL8 = 7;        // binary BVH + spheres in LDS, 64 VGPRs: two 1024-thread workgroups per CU
constexpr int kSrcBvhL8C = 9;       // kSrcBvhL8 with compact 32-bit stack entries (small trees, depth <= kShortStack)
constexpr int kSrcBvh4L = 10;       // 4-wide BVH + spheres in LDS, 64 VGPRs (shadow queries without a light grid)
constexpr int kSrcBvh4G = 11;       // 4-wide BVH + spheres from HBM/L2, 64 VGPRs (idem)
// Trees too large for LDS: the breadth-first top of the binary tree (DevScene::pfx2
// nodes, chosen by the host) in LDS, the rest and the spheres from HBM/L2 (64 VGPRs).
constexpr int kSrcBvhP = 8;         // binary BVH, LDS prefix
constexpr int kSrcBvhPH = 5;        // binary BVH with binary16 bounds (DevBvhNodeH), LDS prefix of twice the nodes
constexpr int kSrcBvhPHC = 6;       // kSrcBvhPH with compact 32-bit stack entries (18-bit codes: <= 16383 spheres)
// Shadow kernel when every light is a point light with a light-view grid: no
// tree walk at all (so no traversal stack in scratch and no register spills),
// spheres from LDS or HBM/L2.
constexpr int kSrcGridL = 14;
constexpr int kSrcGridG = 15;
// Generation 0 only: camera rays through the camera's view grid (nearest_cgrid),
// spheres staged in LDS (22) or read through L2 (23).
constexpr int kSrcCamGridL = 22;
constexpr int kSrcCamGridG = 23;
// The quantised 4-wide tree (DevQNode4, nearest_q4), spheres from HBM/L2 (64 VGPRs): every
// node in LDS (25, trees of <= ~1500 nodes such as C4's) or the breadth-first top
// DevScene::pfxq nodes in LDS and the rest through L2 (26, C5); tuning qtree, off by default
constexpr int kSrcQ4 = 25;
constexpr int kSrcQ4P = 26;

template <int kSrc>
struct Src {
    static constexpr bool grid = kSrc == kSrcGridL || kSrc == kSrcGridG;
    static constexpr bool cgrid = kSrc == kSrcCamGridL || kSrc == kSrcCamGridG;
    static constexpr bool q4 = kSrc == kSrcQ4 || kSrc == kSrcQ4P;
    static constexpr bool bvh = kSrc >= kSrcBvhG && !grid && !cgrid && !q4;
    static constexpr bool wide = kSrc == kSrcBvh4L || kSrc == kSrcBvh4G;
    static constexpr bool half = kSrc == kSrcBvhPH || kSrc == kSrcBvhPHC;
    static constexpr int compact_bits = kSrc == kSrcBvhL8C ? 16 : kSrc == kSrcBvhPHC ? 18 : 0;
    static constexpr bool prefix = kSrc == kSrcBvhP || half;
    static constexpr bool all_lds = kSrc == kSrcBvhL8 || kSrc == kSrcBvhL8C || kSrc == kSrcBvh4L;
    static constexpr bool sph_lds = kSrc == kSrcLds || all_lds || kSrc == kSrcGridL || kSrc == kSrcCamGridL;
    static constexpr int nodes = all_lds ? 2 : half ? 3 : prefix ? 1 : 0;
    static constexpr int waves = kSrc >= kSrcBvhL8 || half ? 8 : 4;   // min waves per SIMD
};

// Nodes of the LDS prefix of a prefix source.
template <int kSrc>
__host__ __device__ inline int32_t prefix_nodes(const DevScene& sc) {
    if (kSrc == kSrcBvhP) return min(sc.n_bvh, sc.pfx2);
    if (Src<kSrc>::half) return min(sc.n_bvh, 2 * sc.pfx2);     // same LDS bytes, 32-B nodes
    if (kSrc == kSrcQ4P) return min(sc.n_q4, sc.pfxq);
    if (kSrc == kSrcQ4) return sc.n_q4;
    return 0;
}

// The scene constants a grid source stages behind its spheres (stage_grid_consts): one LdsGridHdr
// per light and the DevLight array (shadow grids), or the camera grid's one header; then the planes
// and their object ids when there are at most kStagedPlanes.  The shadow mask has 32 bits, so at
// most 32 * (240 + 104) B = 10.75 KB of headers and lights and 416 B of planes: with the planner's
// 64 KB (shadow) and 72 KB (camera) sphere limits and the queue words a workgroup stays below
// half a CU's 160 KB up to ~20 lights at G = 512, and far below the launch limit always.
template <int kSrc>
__host__ __device__ inline size_t grid_const_bytes(const DevScene& sc) {
    if (!Src<kSrc>::grid && !Src<kSrc>::cgrid) return 0;
    const size_t nh = Src<kSrc>::grid ? static_cast<size_t>(sc.n_lights) : 1;
    size_t bytes = nh * sizeof(LdsGridHdr) + (Src<kSrc>::grid ? nh * sizeof(DevLight) : 0);
    if (sc.n_planes <= kStagedPlanes) bytes += static_cast<size_t>(sc.n_planes) * (sizeof(DevPlane) + sizeof(int32_t));
    return bytes;
}

// LDS layout of the intersection kernels: [staged data][region scan, G + 1][wave sums, 16][counter].
template <int kSrc>
__host__ __device__ inline size_t staged_bytes(const DevScene& sc) {
    if (Src<kSrc>::grid || Src<kSrc>::cgrid) {
        const size_t per = kSrc == kSrcGridL ? sizeof(DevSphere) : kSrc == kSrcCamGridL ? sizeof(DevSphere) + sizeof(int32_t) : 0;
        const size_t sph = (static_cast<size_t>(sc.n_spheres) * per + 15) / 16 * 16;
        return (sph + grid_const_bytes<kSrc>(sc) + 15) / 16 * 16;
    }
    size_t bytes = 0;
    if (Src<kSrc>::q4) bytes = static_cast<size_t>(prefix_nodes<kSrc>(sc)) * sizeof(DevQNode4);
    if (kSrc == kSrcLds) bytes = static_cast<size_t>(sc.n_spheres) * sizeof(DevSphere);
    if (kSrc == kSrcBvhP) bytes = static_cast<size_t>(prefix_nodes<kSrc>(sc)) * sizeof(DevBvhNode);
    if (Src<kSrc>::half) bytes = static_cast<size_t>(prefix_nodes<kSrc>(sc)) * sizeof(DevBvhNodeH);
    if (Src<kSrc>::nodes == 2)
        bytes = Src<kSrc>::wide ? static_cast<size_t>(sc.n_bvh4) * kBvh4Planes * sizeof(DevBvh4Plane) : node_planes_bytes(sc.n_bvh);
    if (Src<kSrc>::bvh && Src<kSrc>::sph_lds) bytes += static_cast<size_t>(sc.n_spheres) * (sizeof(DevSphere) + sizeof(int32_t));
    return (bytes + 15) / 16 * 16;
}

// Stage a grid source's scene constants at `at` (16-byte aligned; grid_const_bytes): headers,
// lights, planes, plane ids, in that order.  Eight work-items per header: one per face (the
// face's five words gathered from DevLightGrid's per-field arrays) and one for the rest.
template <int kSrc>
__device__ __forceinline__ void stage_grid_consts(const DevScene& sc, unsigned char* at, BvhView& v) {
    constexpr int T = kWfThreads;
    const DevLightGrid* src = Src<kSrc>::grid ? sc.lgrid : sc.cgrid;
    const int nh = Src<kSrc>::grid ? sc.n_lights : 1;
    LdsGridHdr* hdr = reinterpret_cast<LdsGridHdr*>(at);
    if (src)
        for (int i = threadIdx.x; i < nh * 8; i += T) {
            const DevLightGrid& g = src[i >> 3];
            LdsGridHdr& h = hdr[i >> 3];
            const int f = i & 7;
            if (f < 6) {
                h.face[f] = LdsGridFace{g.fx0[f], g.fy0[f], g.fw[f], g.fh[f], g.off_base[f], {0u, 0u, 0u}};
            } else if (f == 6) {
                h.lx = g.lx; h.ly = g.ly; h.lz = g.lz;
                h.R = g.R; h.always_begin = g.always_begin; h.always_end = g.always_end;
            }
        }
    v.ghdr = hdr;
    at += static_cast<size_t>(nh) * sizeof(LdsGridHdr);
    if constexpr (Src<kSrc>::grid) {
        static_assert(sizeof(DevLight) % 8 == 0, "DevLight is copied as 8-byte words");
        uint64_t* ll = reinterpret_cast<uint64_t*>(at);
        const uint64_t* gl = reinterpret_cast<const uint64_t*>(sc.lights);
        const int nw = nh * static_cast<int>(sizeof(DevLight) / 8);
        for (int i = threadIdx.x; i < nw; i += T) ll[i] = gl[i];
        v.llights = reinterpret_cast<const DevLight*>(at);
        at += static_cast<size_t>(nh) * sizeof(DevLight);
    }
    if (sc.n_planes > 0 && sc.n_planes <= kStagedPlanes) {
        uint64_t* lp = reinterpret_cast<uint64_t*>(at);
        const uint64_t* gp = reinterpret_cast<const uint64_t*>(sc.planes);
        const int nw = sc.n_planes * static_cast<int>(sizeof(DevPlane) / 8);
        for (int i = threadIdx.x; i < nw; i += T) lp[i] = gp[i];
        int32_t* lo = reinterpret_cast<int32_t*>(lp + nw);
        for (int i = threadIdx.x; i < sc.n_planes; i += T) lo[i] = sc.plane_obj[i];
        v.lplanes = reinterpret_cast<const DevPlane*>(lp);
        v.lplane_obj = lo;
    }
}

// Stage what the source keeps in LDS (the whole tree and the spheres, or the
// top of the tree); returns the view the queries use.
// kNearest: the nearest-hit walk's byte-offset node encoding (stage_node_planes).
template <int kSrc, bool kNearest = false>
__device__ __forceinline__ BvhView stage_lds(const DevScene& sc, unsigned char* lds) {
    constexpr int T = kWfThreads;
    BvhView v = global_view(sc);
    size_t off = 0;
    if constexpr (Src<kSrc>::q4) {
        const int32_t nl = prefix_nodes<kSrc>(sc);
        uint4* ln = reinterpret_cast<uint4*>(lds);
        const uint4* gn = reinterpret_cast<const uint4*>(sc.q4);
        for (int i = threadIdx.x; i < 3 * nl; i += T) ln[i] = gn[i];
        v.q4l = reinterpret_cast<const DevQNode4*>(lds);
        v.nq = nl;
        return v;
    } else if constexpr (kSrc == kSrcBvhP) {
        DevBvhNode* ln = reinterpret_cast<DevBvhNode*>(lds);
        const int32_t nl = prefix_nodes<kSrc>(sc);
        for (int i = threadIdx.x; i < nl; i += T) ln[i] = sc.bvh[i];
        v.pnodes = ln;
        v.nl = nl;
        return v;
    } else if constexpr (Src<kSrc>::half) {
        DevBvhNodeH* ln = reinterpret_cast<DevBvhNodeH*>(lds);
        const int32_t nl = prefix_nodes<kSrc>(sc);
        for (int i = threadIdx.x; i < nl; i += T) ln[i] = sc.bvh_h[i];
        v.hpnodes = ln;
        v.hgnodes = sc.bvh_h;
        v.nl = nl;
        return v;
    } else if constexpr (kSrc == kSrcLds || kSrc == kSrcGridL) {
        DevSphere* ls = reinterpret_cast<DevSphere*>(lds);
        for (int i = threadIdx.x; i < sc.n_spheres; i += T) ls[i] = sc.spheres[i];
        v.sph = ls;
        if constexpr (kSrc == kSrcGridL)
            stage_grid_consts<kSrc>(sc, lds + (static_cast<size_t>(sc.n_spheres) * sizeof(DevSphere) + 15) / 16 * 16, v);
        return v;
    } else if constexpr (kSrc == kSrcCamGridL) {
        DevSphere* ls = reinterpret_cast<DevSphere*>(lds);
        int32_t* lo = reinterpret_cast<int32_t*>(ls + sc.n_spheres);
        for (int i = threadIdx.x; i < sc.n_spheres; i += T) { ls[i] = sc.spheres[i]; lo[i] = sc.sphere_obj[i]; }
        v.sph = ls;
        v.obj = lo;
        stage_grid_consts<kSrc>(sc, lds + (static_cast<size_t>(sc.n_spheres) * (sizeof(DevSphere) + sizeof(int32_t)) + 15) / 16 * 16, v);
        return v;
    } else if constexpr (kSrc == kSrcGridG || kSrc == kSrcCamGridG) {
        stage_grid_consts<kSrc>(sc, lds, v);
        return v;
    } else if constexpr (Src<kSrc>::nodes == 2 && Src<kSrc>::wide) {
        DevBvh4Plane* lp = reinterpret_cast<DevBvh4Plane*>(lds);
        const int n = kBvh4Planes * sc.n_bvh4;
        for (int i = threadIdx.x; i < n; i += T) lp[i] = sc.bvh4[i];
        v.p4 = lp;
        off = static_cast<size_t>(n) * sizeof(DevBvh4Plane);
    } else if constexpr (Src<kSrc>::nodes == 2) {
        v.lnodes = stage_node_planes<T, kNearest>(sc.bvh, sc.n_bvh, lds);
        v.nl = sc.n_bvh;
        off = node_planes_bytes(sc.n_bvh);
    }
    if constexpr (Src<kSrc>::bvh && Src<kSrc>::sph_lds) {
        DevSphere* ls = reinterpret_cast<DevSphere*>(lds + off);
        int32_t* lo = reinterpret_cast<int32_t*>(ls + sc.n_spheres);
        for (int i = threadIdx.x; i < sc.n_spheres; i += T) { ls[i] = sc.spheres[i]; lo[i] = sc.sphere_obj[i]; }
        v.sph = ls;
        v.obj = lo;
    }
    return v;
}

// register entries on top of the binary16 prefix walk's stack (src 5, 6): three (C4 49.80-49.86
// vs 50.07-50.09 ms with two, 50.41 with one, 50.36 with four; C5 equal within 0.5%)
#ifndef RT_HALF_REG
#define RT_HALF_REG 3
#endif
// register entries on top of the compact stack (the whole tree in LDS, src 9): one (C3 3.054 vs
// 3.116 ms, 8-way share 0.756 vs 0.765 ms on one box; two 3.168 vs 3.144 ms); A/B builds:
// EXTRA=-DRT_COMPACT_REG=n
#ifndef RT_COMPACT_REG
#define RT_COMPACT_REG 1
#endif
// Scene::intersect of one ray through the source's structure (scene.rs:247-249).
template <int kSrc, bool kCount>
__device__ __forceinline__ Hit nearest_any(const DevScene& sc, const BvhView& v, const Ray& r, Work* w) {
    if constexpr (Src<kSrc>::cgrid) return nearest_cgrid<kCount>(sc, v, r, w);       // stage_lds staged the header
    else if constexpr (Src<kSrc>::q4) return nearest_q4<kCount, kSrc == kSrcQ4>(sc, v, r, w);
    // two stack entries in registers when the tree is read through L2 below its LDS prefix
    // (C4 74.0 -> 71.4 ms); RT_COMPACT_REG on the compact stack with the whole tree in LDS (the
    // 64-bit stack: 3.66 -> 3.80 ms with 1-4 in round 2)
    else if constexpr (Src<kSrc>::bvh && Src<kSrc>::nodes == 2)
        return nearest_bvh_bl<kCount, 2, Src<kSrc>::compact_bits ? RT_COMPACT_REG : 0, Src<kSrc>::compact_bits>(sc, v, r, w);
    else if constexpr (Src<kSrc>::bvh && Src<kSrc>::half) return nearest_bvh_bl<kCount, 3, RT_HALF_REG, Src<kSrc>::compact_bits>(sc, v, r, w);
    else if constexpr (Src<kSrc>::bvh && Src<kSrc>::prefix) return nearest_bvh_bl<kCount, 1, 2>(sc, v, r, w);
    else if constexpr (Src<kSrc>::bvh) return nearest_bvh_bl<kCount, 0, 0>(sc, v, r, w);
    else return nearest_brute<kCount>(sc, v.sph, r, w);
}

template <int kSrc, bool kCount>
__device__ __forceinline__ bool occluded_any(const DevScene& sc, const BvhView& v, const Ray& r, bool has_range,
                                             double r2, int32_t hint, Work* w) {
    if constexpr (Src<kSrc>::wide) return occluded_bvh4<kCount>(sc, v, r, has_range, r2, hint, w);
    else if constexpr (Src<kSrc>::bvh) return occluded_bvh<kCount, Src<kSrc>::nodes, 0>(sc, v, r, has_range, r2, hint, w);
    else return occluded_brute<kCount>(sc, v.sph, r, has_range, r2, w);
}

// One global atomic per workgroup into totals[at], totals[at + 1]
// (instrumented kernels only; every thread of the workgroup must call it).
template <bool kCount>
__device__ __forceinline__ void flush_work(const WfBufs& b, int at, Work w) {
    if constexpr (kCount) {
        __shared__ unsigned long long s_w[2];
        if (threadIdx.x == 0) { s_w[0] = 0; s_w[1] = 0; }
        __syncthreads();
        unsigned long long bx = w.boxes, sp = w.spheres;
        for (int off = 32; off > 0; off >>= 1) {
            bx += __shfl_xor(bx, off, 64);
            sp += __shfl_xor(sp, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&s_w[0], bx);
            atomicAdd(&s_w[1], sp);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(&b.totals[at], s_w[0]);
            atomicAdd(&b.totals[at + 1], s_w[1]);
        }
    }
}

// A camera ray that misses everything: the pixel is the background averaged
// over samples, precomputed on the host (FrameParams::bg_*), written here (it
// starts no chain, so wf_fold never sees it).
__device__ __forceinline__ void write_background_pixel(const FrameParams& fp, const WfBufs& b, uint32_t p) {
    const uint32_t lx = p % fp.tile_w, row = fp.row0 + p / fp.tile_w;
    if (fp.out_rgb) {
        float* q = fp.out_rgb + (static_cast<size_t>(row) * fp.tile_w + lx) * 3;
        q[0] = fp.bg_rgb[0]; q[1] = fp.bg_rgb[1]; q[2] = fp.bg_rgb[2];
    }
    if (fp.out_bgr) {
        uint8_t* q = fp.out_bgr + static_cast<size_t>(row) * fp.bgr_pitch + 3u * lx;
        q[0] = fp.bg_bgr[0]; q[1] = fp.bg_bgr[1]; q[2] = fp.bg_bgr[2];
        if (lx == fp.tile_w - 1)       // BMP row padding is zero (main.rs:42)
            for (uint32_t k = 3u * fp.tile_w; k < fp.pad_end; ++k) fp.out_bgr[static_cast<size_t>(row) * fp.bgr_pitch + k] = 0;
    }
}

// The colour that ends a chain without lighting: the background (obj INT32_MAX,
// a miss) or the object's ambient colour (cut-off, insignificant surface).
__device__ __forceinline__ Col end_colour(const DevScene& sc, int32_t obj) {
    if (obj == INT32_MAX) return Col{sc.bg[0], sc.bg[1], sc.bg[2]};
    const DevMaterial& m = sc.mats[obj];
    return Col{m.amb[0], m.amb[1], m.amb[2]};
}

typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));

// The sRGB bytes of a colour as the frame stores a pixel: b | g << 8 | r << 16.
__device__ __forceinline__ uint32_t pack_bgr(Col c, const double* table) {
    return static_cast<uint32_t>(to_srgb(c.b, table)) | (static_cast<uint32_t>(to_srgb(c.g, table)) << 8) |
           (static_cast<uint32_t>(to_srgb(c.r, table)) << 16);
}

// RT_ALGO_WAVEFRONT_AA: one camera sample's colour as raytrace() returns it
// (raytrace.rs:271-275 with one camera sample: BLACK + c, divided by 1).
__device__ __forceinline__ Col aa_sample(Col c) { return Col{(0.0 + c.r) / 1.0, (0.0 + c.g) / 1.0, (0.0 + c.b) / 1.0}; }

// ... and main.rs:47-55's `res = res + raytrace(..)` for sample fp.aa_pass of chunk
// pixel p: pass 0 starts from BLACK (0.0 + s_0, nothing read), pass a adds s_a to
// the sum of samples 0 .. a-1.  A pixel has one writer per pass and the passes
// of a chunk follow each other on its lane's stream: plain loads and stores.
// kMom (a moments accumulator; instantiations of their own, so a plain accumulator and a
// one-shot antialiased render run the kernels they always ran): the running sums of squares in the plane after
// the tile's sums continue by the same rule, pass 0 stores 0.0 + s * s.
// One sample's step of a running sum of squares: q = s * s, then Q + q, two IEEE operations and never an fma.
__device__ __forceinline__ double sq_add(double Q, double s) { return __dadd_rn(Q, __dmul_rn(s, s)); }
template <bool kMom = false>
__device__ __forceinline__ void aa_add(const FrameParams& fp, uint32_t p, Col s) {
    double* q = fp.aa_acc + 3 * static_cast<size_t>(p);
    Col acc{0.0, 0.0, 0.0};
    if (fp.aa_pass) acc = Col{q[0], q[1], q[2]};
    q[0] = acc.r + s.r; q[1] = acc.g + s.g; q[2] = acc.b + s.b;
    if constexpr (kMom) {
        double* q2 = q + 3 * (static_cast<size_t>(fp.tile_w) * fp.tile_h);
        Col sq{0.0, 0.0, 0.0};
        if (fp.aa_pass) sq = Col{q2[0], q2[1], q2[2]};
        q2[0] = sq_add(sq.r, s.r); q2[1] = sq_add(sq.g, s.g); q2[2] = sq_add(sq.b, s.b);
    }
}

// The final colour of chain c (pixel p of the chunk): into ccol[c] for wf_compose
// (chain order: coalesced), or straight into the frame.  kAa (res: the sample's
// colour): into term[c] (the chain's terminal, folded by now) for wf_aa_compose,
// or added to pixel p's running sum.
template <bool kAa = false, bool kMom = false>
__device__ __forceinline__ void emit_chain(const FrameParams& fp, const WfBufs& b, uint32_t c, uint32_t p, Col res,
                                           const double* srgb) {
    if constexpr (kAa) {
        if (b.compose) { stn(&b.term(0)[c], res.r); stn(&b.term(1)[c], res.g); stn(&b.term(2)[c], res.b); }
        else aa_add<kMom>(fp, p, res);
    } else if (b.compose) {
        const uint32_t q = pack_bgr(res, srgb);
        const U32x4 v = {__float_as_uint(static_cast<float>(res.r)), __float_as_uint(static_cast<float>(res.g)),
                         __float_as_uint(static_cast<float>(res.b)), q};
        stn(reinterpret_cast<U32x4*>(b.ccol()) + c, v);
    } else {
        write_pixel(fp, p % fp.tile_w, fp.row0 + p / fp.tile_w, res, srgb);
    }
}

// A level entry (WfLevel at index at = k * capa + chain) moves as its two 16-B halves {r, g} and
// {b, f}: one lane writes, and later reads, one whole aligned 32-B sector.  f: the factor the fold
// multiplies by beside ks (the Schlick factor of a FresnelMaterial hit, else exactly 1.0).
typedef double F64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_level(const WfBufs& b, size_t at, Col res, double f) {
    F64x2* e = reinterpret_cast<F64x2*>(b.lev() + at);
    stn(e, F64x2{res.r, res.g});
    stn(e + 1, F64x2{res.b, f});
}
// kF false (a scene without FresnelMaterial: every f is 1.0): f is not fetched, 24 B of the sector.
template <bool kF>
__device__ __forceinline__ WfLevel load_level(const WfBufs& b, size_t at) {
    const F64x2* e = reinterpret_cast<const F64x2*>(b.lev() + at);
    const F64x2 lo = ldn_if<kNtFold>(e);
    if constexpr (kF) {
        const F64x2 hi = ldn_if<kNtFold>(e + 1);
        return WfLevel{lo[0], lo[1], hi[0], hi[1]};
    } else {
        return WfLevel{lo[0], lo[1], ldn_if<kNtFold>(&b.lev()[at].b), 1.0};
    }
}

// Chain c ends in generation k with colour col (wf_fold folds its k levels onto it).
__device__ __forceinline__ void set_terminal(const WfBufs& b, uint32_t c, Col col, int k) {
    stn(&b.term(0)[c], col.r); stn(&b.term(1)[c], col.g); stn(&b.term(2)[c], col.b);
    b.nlev()[c] = static_cast<uint8_t>(k);
}
// ... on a skybox scene by a miss of ray r: the skybox is sampled later (wf_sky_term, before the
// fold), so the traversal kernel carries no texel fetches; term holds the direction until then.
__device__ __forceinline__ void set_sky_terminal(const WfBufs& b, uint32_t c, const Ray& r, int k) {
    stn(&b.term(0)[c], r.dx); stn(&b.term(1)[c], r.dy); stn(&b.term(2)[c], r.dz);
    b.nlev()[c] = static_cast<uint8_t>(kNlevSky | static_cast<uint32_t>(k));
}

// LDS of a queue kernel after its staged data.
constexpr int kQueueCounters = 2;           // this workgroup's shade records and reflection rays

struct QueueLds {
    uint32_t* scan;     // G + 1
    uint32_t* wave;     // 16
    uint32_t* count;    // shade records, reflection rays appended by this workgroup
};

__device__ __forceinline__ QueueLds queue_lds(unsigned char* at, uint32_t G) {
    uint32_t* p = reinterpret_cast<uint32_t*>(at);
    return QueueLds{p, p + G + 1, p + G + 1 + kWfThreads / 64};
}

__host__ __device__ inline size_t queue_lds_bytes(uint32_t G) { return (G + 1 + kWfThreads / 64 + kQueueCounters) * 4u; }

// One wave's 64-pixel segment of a frame row (pixels [x0, x0 + nv) of chunk row lrow; lane's
// pixel: f32 r, g, bl and sRGB bytes q = b | g << 8 | r << 16): the f32 RGB as consecutive dwords
// and the BGR as consecutive dwords (dw) or bytes, staged through the wave's LDS slices so that
// every store instruction covers consecutive addresses; the row's zero padding after its last
// segment.  Wave-uniform arguments but r, g, bl, q.
__device__ __forceinline__ void store_row_segment(const FrameParams& fp, float* s_rgb, uint32_t* s_bgr, bool dw, uint32_t lrow,
                                                  uint32_t x0, uint32_t nv, float r, float g, float bl, uint32_t q) {
    const uint32_t lane = threadIdx.x & 63u, x = x0 + lane;
    const uint32_t orow = fp.row0 + lrow;
    if (fp.out_rgb) {
        s_rgb[3 * lane] = r; s_rgb[3 * lane + 1] = g; s_rgb[3 * lane + 2] = bl;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        float* dst = fp.out_rgb + (static_cast<size_t>(orow) * fp.tile_w + x0) * 3;
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            const uint32_t i = lane + 64u * j;
            if (i < 3 * nv) dst[i] = s_rgb[i];
        }
    }
    if (fp.out_bgr) {
        uint8_t* row = fp.out_bgr + static_cast<size_t>(orow) * fp.bgr_pitch;
        if (dw) {
            uint8_t* sb = reinterpret_cast<uint8_t*>(s_bgr);
            sb[3 * lane] = static_cast<uint8_t>(q); sb[3 * lane + 1] = static_cast<uint8_t>(q >> 8);
            sb[3 * lane + 2] = static_cast<uint8_t>(q >> 16);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            // dwords [0, ceil(3 nv / 4)) of the segment; bytes past 3 nv are row padding (zero)
            const uint32_t nd = (3 * nv + 3) / 4;
            if (lane < nd) {
                uint32_t v = s_bgr[lane];
                const uint32_t valid = 3 * nv - 4 * lane;                // bytes of this dword that are pixels
                if (valid < 4) v &= (1u << (8 * valid)) - 1u;
                reinterpret_cast<uint32_t*>(row + 3 * x0)[lane] = v;
            }
            __builtin_amdgcn_wave_barrier();
        } else if (lane < nv) {
            row[3 * x] = static_cast<uint8_t>(q); row[3 * x + 1] = static_cast<uint8_t>(q >> 8);
            row[3 * x + 2] = static_cast<uint8_t>(q >> 16);
        }
        if (x0 + nv == fp.tile_w)                                  // BMP row padding is zero (main.rs:42)
            for (uint32_t k = (dw ? (3 * fp.tile_w + 3) & ~3u : 3 * fp.tile_w) + lane; k < fp.pad_end; k += 64)
                row[k] = 0;
    }
    __builtin_amdgcn_wave_barrier();
}
// dword-aligned BGR rows whose last dword the render may write whole (pixels, then zero padding)
__device__ __forceinline__ bool bgr_dwords(const FrameParams& fp) {
    return ((fp.bgr_pitch | reinterpret_cast<uintptr_t>(fp.out_bgr)) & 3u) == 0 && ((3 * fp.tile_w + 3) & ~3u) <= fp.pad_end;
}

}  // namespace
}  // namespace rtamd
