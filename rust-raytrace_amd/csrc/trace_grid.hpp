// The light-view grids (point-light shadows) and the camera's view grid (generation 0), read
// through L2 or from staged scene constants.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "trace_types.hpp"
#include "trace_prims.hpp"
#include "trace_view.hpp"
#include "trace_bvh.hpp"

namespace rtamd {

// ---- point-light shadows through the light-view grid ---------------------
// The shadow query of occluded_bvh4 for a point light (has_range), with the
// spheres taken from the light's grid (host_lightgrid.cpp) instead of a tree:
// the always list, then the list of the cell that p's direction from the light
// falls in, in increasing box distance from the light, stopping at the first
// box farther than p (no blocker can be farther from the light than p is).
// Every sphere that could report a blocking hit is on those lists, and each is
// tested with the exact quadratic, so the any-hit answer is the linear scan's.
// A degenerate direction (p at the light, non-finite) tests every sphere.
template <bool kCount = false>
__device__ __forceinline__ bool occluded_lgrid(const DevScene& sc, const BvhView& v, const DevLightGrid& g,
                                               const Ray& r, double r2, double ptx, double pty, double ptz,
                                               int32_t hint, Work* w = nullptr) {
    bool plane_block = false;
    for (int i = 0; i < sc.n_planes; ++i) {
        double t;
        if (!plane_t(sc.planes[i], r, t)) continue;
        if (t != t) return false;                  // the NaN hit is the nearest: t*t < r2 fails (lit)
        plane_block |= t * t < r2;
    }
    if (plane_block) return true;
    if (sc.n_spheres == 0) return false;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    auto blocks = [&](int32_t k) {
        if constexpr (kCount) ++w->spheres;
        double t;
        return sphere_t(v.sph[k], r, sk, t) && t * t < r2;
    };
    if (hint >= 0 && blocks(hint)) return true;
    for (uint32_t e = g.always_begin; e < g.always_end; ++e)
        if (blocks(sc.lg_ent[e].sph)) return true;
    const float dx = static_cast<float>(ptx - g.lx), dy = static_cast<float>(pty - g.ly),
                dz = static_cast<float>(ptz - g.lz);
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const int fa = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float da = fa == 0 ? dx : fa == 1 ? dy : dz;
    const float db = fa == 0 ? dy : fa == 1 ? dz : dx;
    const float dc = fa == 0 ? dz : fa == 1 ? dx : dy;
    // ... and so does a shade point beyond the culling domain (the far-origin rule)
    if (!(fabsf(da) > 0.0f && fabsf(da) < 3.0e38f) || beyond_reach(static_cast<float>(ptx), static_cast<float>(pty), static_cast<float>(ptz), sc.cull_reach)) {
        for (int32_t k = 0; k < sc.n_spheres; ++k)
            if (blocks(k)) return true;
        return false;
    }
    const int f = 2 * fa + (da < 0.0f ? 1 : 0);
    const float inv = 1.0f / fabsf(da);
    const float R = static_cast<float>(g.R);
    const int ci = min(max(static_cast<int>(floorf((db * inv + 1.0f) * 0.5f * R)), 0), g.R - 1);
    const int cj = min(max(static_cast<int>(floorf((dc * inv + 1.0f) * 0.5f * R)), 0), g.R - 1);
    const int li = ci - g.fx0[f], lj = cj - g.fy0[f];
    if (li < 0 || lj < 0 || li >= g.fw[f] || lj >= g.fh[f]) return false;    // no sphere in this direction
    const uint32_t cell = g.off_base[f] + static_cast<uint32_t>(lj * g.fw[f] + li);
    const uint32_t e0 = sc.lg_off[cell], e1 = sc.lg_off[cell + 1];
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz) * 1.00001f + 1e-5f;     // >= |p - L|
    for (uint32_t e = e0; e < e1; ++e) {
        const DevLgEntry en = sc.lg_ent[e];
        if (en.near > dist) break;
        if (blocks(en.sph)) return true;
    }
    return false;
}

// ---- the two grid queries on staged scene constants ------------------------
// occluded_lgrid and nearest_cgrid for the kernels that keep the lights' grid headers, the
// lights and the planes in LDS (BvhView::ghdr; sources 14, 15, 22, 23): the same tests in the
// same order with the same stops, so answers and RT_COUNT_WORK counters are theirs.  Only the
// loads move.  The cell is computed first (f32 arithmetic on p - L, independent of every
// test) and its offset pair is requested before the planes and the hint sphere are tested; the
// always list (empty unless the light sits in a sphere's padded box) is read after them.  A
// list entry is one 8-byte load, and entry e + 1 is requested before entry e's sphere test
// starts (one ahead: the kernels run at the 64 registers of 8 waves per SIMD).  End of list: the
// look-ahead is guarded by e + 1 < e1, so nothing at or beyond a list's e1 is ever read and
// lg_ent / cg_ent carry no padding.  The kernels that stage nothing (the general shadow kernel
// of a scene with an ungridded light, the fused tail's grid_shadow_mask at its 128 registers)
// keep occluded_lgrid above, headers through L2.

typedef uint64_t __attribute__((may_alias, aligned(8))) GridEntryBits;
// One DevLgEntry as 64 bits: sph in the low word, near in the high word.
__device__ __forceinline__ uint64_t load_grid_entry(const DevLgEntry* ent, uint32_t e) {
    return *reinterpret_cast<const GridEntryBits*>(ent + e);
}
__device__ __forceinline__ int32_t entry_sph(uint64_t bits) { return static_cast<int32_t>(static_cast<uint32_t>(bits)); }
__device__ __forceinline__ float entry_near(uint64_t bits) { return __uint_as_float(static_cast<uint32_t>(bits >> 32)); }
// Keeps a requested load where it is written: without it the compiler sinks the load next to
// its first use, behind the sphere test it was meant to overlap.
__device__ __forceinline__ void keep_loads_here() { asm volatile("" ::: "memory"); }

// A grid query's request: the direction's cell (occluded_lgrid's arithmetic, operation for
// operation) and its offset pair, in flight when grid_request returns (nothing there waits for
// it).  Four registers for the caller to hold through the tests that come before the list.
constexpr uint32_t kGridNone = 0;      // no sphere in this direction
constexpr uint32_t kGridList = 1;      // the cell's list, entries [e0, e1)
constexpr uint32_t kGridWhole = 2;     // degenerate direction or beyond the culling domain: every sphere
struct GridReq {
    uint32_t kind;
    uint32_t e0, e1;
    float dist;            // shadow queries: the f32 bound >= |p - L| the list walk stops at
};
__device__ __forceinline__ GridReq grid_request(const LdsGridHdr& g, const uint32_t* off, float dx, float dy, float dz,
                                                bool beyond) {
    GridReq q{kGridNone, 0u, 0u, 0.0f};
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const int fa = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float da = fa == 0 ? dx : fa == 1 ? dy : dz;
    const float db = fa == 0 ? dy : fa == 1 ? dz : dx;
    const float dc = fa == 0 ? dz : fa == 1 ? dx : dy;
    if (!(fabsf(da) > 0.0f && fabsf(da) < 3.0e38f) || beyond) {
        q.kind = kGridWhole;
        return q;
    }
    const int f = 2 * fa + (da < 0.0f ? 1 : 0);
    const float inv = 1.0f / fabsf(da);
    const int gR = g.R;
    const float R = static_cast<float>(gR);
    const int ci = min(max(static_cast<int>(floorf((db * inv + 1.0f) * 0.5f * R)), 0), gR - 1);
    const int cj = min(max(static_cast<int>(floorf((dc * inv + 1.0f) * 0.5f * R)), 0), gR - 1);
    const LdsGridFace fc = g.face[f];
    const int li = ci - fc.fx0, lj = cj - fc.fy0;
    if (li < 0 || lj < 0 || li >= fc.fw || lj >= fc.fh) return q;
    const uint32_t cell = fc.off_base + static_cast<uint32_t>(lj * fc.fw + li);
    q.kind = kGridList;
    q.e0 = off[cell];
    q.e1 = off[cell + 1];
    keep_loads_here();
    return q;
}
// ... of the shadow query of shade point p toward the light of grid g
__device__ __forceinline__ GridReq lgrid_request(const DevScene& sc, const LdsGridHdr& g, double ptx, double pty, double ptz) {
    const float dx = static_cast<float>(ptx - g.lx), dy = static_cast<float>(pty - g.ly),
                dz = static_cast<float>(ptz - g.lz);
    GridReq q = grid_request(g, sc.lg_off, dx, dy, dz,
                             beyond_reach(static_cast<float>(ptx), static_cast<float>(pty), static_cast<float>(ptz), sc.cull_reach));
    q.dist = sqrtf(dx * dx + dy * dy + dz * dz) * 1.00001f + 1e-5f;     // >= |p - L|
    asm volatile("" : "+v"(q.dist));        // computed here: one live register, not dx, dy, dz
    return q;
}

// g: the light's staged header; q: lgrid_request for the same point and light, made by the
// caller before it computes the light direction, so that the offsets travel during that
// division chain too.
template <bool kCount = false>
__device__ __forceinline__ bool occluded_lgrid_lds(const DevScene& sc, const BvhView& v, const LdsGridHdr& g, const GridReq& q,
                                                   const Ray& r, double r2, int32_t hint, Work* w = nullptr) {
    bool plane_block = false;
    auto planes = [&](const DevPlane* P) {
        for (int i = 0; i < sc.n_planes; ++i) {
            double t;
            if (!plane_t(P[i], r, t)) continue;
            if (t != t) return 1;                    // the NaN hit is the nearest: t*t < r2 fails (lit)
            plane_block |= t * t < r2;
        }
        return 0;
    };
    if (v.lplanes ? planes(v.lplanes) : planes(sc.planes)) return false;
    if (plane_block) return true;
    if (sc.n_spheres == 0) return false;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    auto blocks = [&](int32_t k) {
        if constexpr (kCount) ++w->spheres;
        double t;
        return sphere_t(v.sph[k], r, sk, t) && t * t < r2;
    };
    if (hint >= 0 && blocks(hint)) return true;
    uint32_t ae = g.always_begin;
    const uint32_t ae1 = g.always_end;
    if (ae < ae1) {
        uint64_t nxt = load_grid_entry(sc.lg_ent, ae);
        do {
            const uint64_t cur = nxt;
            if (++ae < ae1) nxt = load_grid_entry(sc.lg_ent, ae);
            keep_loads_here();
            if (blocks(entry_sph(cur))) return true;
        } while (ae < ae1);
    }
    if (q.kind == kGridWhole) {
        for (int32_t k = 0; k < sc.n_spheres; ++k)
            if (blocks(k)) return true;
        return false;
    }
    const uint32_t e1 = q.e1;
    uint32_t e = q.e0;
    if (q.kind == kGridNone || e >= e1) return false;
    const float dist = q.dist;
    uint64_t nxt = load_grid_entry(sc.lg_ent, e);
    for (;;) {
        const uint64_t cur = nxt;
        if (++e < e1) nxt = load_grid_entry(sc.lg_ent, e);
        keep_loads_here();
        if (entry_near(cur) > dist) break;
        if (blocks(entry_sph(cur))) return true;
        if (e >= e1) break;
    }
    return false;
}

// ---- generation 0: the camera's view grid --------------------------------
// Scene::intersect for a camera ray (origin = the camera position) through the
// camera's view grid (host_lightgrid.cpp build_view_grid): the planes, the
// always list, then the ray direction's cell in increasing box distance from
// the camera, stopping at the first entry whose distance bound exceeds the
// current best t (t_limit margin).  A reported hit point lies in its sphere's
// padded box and in the ray direction from the camera, so its sphere is on
// that cell's list, and its distance from the camera (t |d|, |d| = 1 up to
// rounding) is at least the entry's bound: every sphere that could win or tie
// is tested with the exact quadratic, and the (t, object id) minimum is the
// linear scan's (scene.rs:247-249).  A degenerate direction
// tests every sphere.
// Every caller is a camera-grid source (22, 23), which stages the header.
template <bool kCount = false>
__device__ __forceinline__ Hit nearest_cgrid(const DevScene& sc, const BvhView& v, const Ray& r, Work* w = nullptr) {
    const LdsGridHdr& g = *v.ghdr;
    const GridReq q = grid_request(g, sc.cg_off, static_cast<float>(r.dx), static_cast<float>(r.dy), static_cast<float>(r.dz), false);
    Hit h = v.lplanes ? nearest_planes_at(v.lplanes, v.lplane_obj, sc.n_planes, r) : nearest_planes(sc, r);
    if (h.nan_t || sc.n_spheres == 0) return h;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    float lim = h.obj == INT32_MAX ? __builtin_inff() : t_limit(h.t);
    auto test = [&](int32_t k) {
        if constexpr (kCount) ++w->spheres;
        double t;
        if (sphere_t(v.sph[k], r, sk, t)) {
            const int32_t obj = v.obj[k];
            if (t < h.t || (t == h.t && obj < h.obj)) { h.t = t; h.obj = obj; h.prim = k; lim = t_limit(t); }
        }
    };
    uint32_t ae = g.always_begin;
    const uint32_t ae1 = g.always_end;
    if (ae < ae1) {
        uint64_t nxt = load_grid_entry(sc.cg_ent, ae);
        do {
            const uint64_t cur = nxt;
            if (++ae < ae1) nxt = load_grid_entry(sc.cg_ent, ae);
            keep_loads_here();
            test(entry_sph(cur));
        } while (ae < ae1);
    }
    if (q.kind == kGridWhole) {
        for (int32_t k = 0; k < sc.n_spheres; ++k) test(k);
        return h;
    }
    const uint32_t e1 = q.e1;
    uint32_t e = q.e0;
    if (q.kind == kGridNone || e >= e1) return h;    // no sphere box in this direction
    uint64_t nxt = load_grid_entry(sc.cg_ent, e);
    for (;;) {
        const uint64_t cur = nxt;
        if (++e < e1) nxt = load_grid_entry(sc.cg_ent, e);
        keep_loads_here();
        if (entry_near(cur) > lim) break;
        test(entry_sph(cur));
        if (e >= e1) break;
    }
    return h;
}

}  // namespace rtamd
