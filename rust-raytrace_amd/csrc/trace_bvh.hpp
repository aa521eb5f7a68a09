// The conservative f32 slab tests and the three walks of the binary tree.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_layout.hpp"
#include "trace_types.hpp"
#include "trace_prims.hpp"
#include "trace_view.hpp"

namespace rtamd {

// ------------------------------------------------------------------ BVH
//
// Culling must never skip a sphere the exact f64 test would report, or the
// result would differ from the reference's linear scan.  Boxes are padded and
// rounded outward on the host; here every slab interval is computed in f32
// from the f32-rounded ray and then widened by a relative kBoxTol, which
// covers the f32 rounding of origin, direction and slab arithmetic (each a few
// ulps, relative to the t values they perturb).  The slab test runs on the
// direction scaled by a power of two 2^-te that brings its largest component
// into [0.5, 1) whenever that component lies outside [2^-20, 2^20] (te = 0,
// no scaling, for the unit-length camera, reflection and point-light shadow
// rays): t' = t 2^te, exactly, and every t limit handed to the box tests is
// scaled the same way (t_limit(rb, t)).  Without it the f32 direction of a
// directional light's unnormalised shadow ray (-direction, raytrace.rs:41,
// scene.rs:131-139) or of a reflection off a plane whose normal is far from
// unit length over- or underflows, or has every component clamped (round 5:
// a light of magnitude 1e-35 culled occluders).  Direction components below
// 1e-20 of the scaled direction are clamped (no 0 * inf NaNs); such a ray
// moves < 1e-14 relative to its largest component along that axis over any
// relevant t, far below the box padding.  DESIGN.md "BVH exactness" has the
// argument in full.
constexpr float kBoxTol = 1e-5f;
constexpr int kBvhStack = 64;      // host builder bounds the depth (median splits past depth 40)
constexpr int kBvh4Stack = 64;     // 4-wide: the host checks the tree's worst case (bvh4_stack_need) against it

// f32 image of a ray for the slab tests: 1/d per axis and -o/d, so each slab
// bound is one FMA, fma(lo, 1/d, -o/d).  The FMA's rounding terms are of the
// same two kinds the tolerance argument covers: relative to t (rounding of
// 1/d and of the result) and a spatial 2^-24 |o| from rounding o/d.  te: the
// slab t values are t 2^te (see above).
struct RayBox {
    float ix, iy, iz, nox, noy, noz;
    int32_t te;
};

__device__ __forceinline__ float inv_dir(double d) {
    float f = static_cast<float>(d);
    if (!(fabsf(f) >= 1e-20f)) f = copysignf(1e-20f, f);
    return 1.0f / f;
}

#ifndef RT_DIR_SCALE
#define RT_DIR_SCALE 1      // (A/B builds only: 0 = the round-4 unscaled slab tests, not exact for such rays)
#endif
// reach: DevScene::cull_reach.  A ray that starts beyond it (device_layout.hpp, DESIGN.md §4 "the
// far-origin rule") gets the null image, 1/d = 0: every slab bound is fma(v, 0, -0) = 0, so every box
// test passes with entry t = 0 <= any t limit and the walk tests every sphere, as the linear scan does.
// Decided once per ray; the slab tests themselves are the same for every ray.
__device__ __forceinline__ RayBox make_raybox(const Ray& r, float reach) {
    const float ox = static_cast<float>(r.ox), oy = static_cast<float>(r.oy), oz = static_cast<float>(r.oz);
    const bool far = beyond_reach(ox, oy, oz, reach);
    const double m = fmax(fmax(fabs(r.dx), fabs(r.dy)), fabs(r.dz));
    // m = f 2^te with f in [0.5, 1) (v_frexp_exp_i32_f64); NaN and infinite directions keep
    // te = 0 (their t values are NaN anyway)
    const int32_t te = RT_DIR_SCALE && ((m > 0x1p20 && m < __builtin_huge_val()) || (m < 0x1p-20 && m > 0.0))
                           ? __builtin_amdgcn_frexp_exp(m) : 0;
    // (-o/d follows as -(o * 0) = 0 for an origin within the f32 range.  Beyond it, or NaN, the f32
    // image is not finite and the bounds of that axis are NaN: a NaN origin's sphere tests report
    // nothing, a finite f64 origin beyond 3.4e38 is outside what the slab tests support.  Selecting
    // -o/d as well measured 0.6% slower at C3)
    const float ix = far ? 0.0f : inv_dir(ldexp(r.dx, -te)), iy = far ? 0.0f : inv_dir(ldexp(r.dy, -te)),
                iz = far ? 0.0f : inv_dir(ldexp(r.dz, -te));
    return RayBox{ix, iy, iz, -(ox * ix), -(oy * iy), -(oz * iz), te};
}

// Slab bound t at coordinate v along the axis with (1/d, -o/d) = (i, no).
__device__ __forceinline__ float slab_t(float v, float i, float no) { return __builtin_fmaf(v, i, no); }

// Interval widening by the relative kBoxTol (one FMA with an |x| modifier), or as
// one multiply by these factors where the sign cases do not matter (RT_WIDEN_MUL).
#ifndef RT_WIDEN_MUL
#define RT_WIDEN_MUL 1
#endif
constexpr float kWidenLo = 1.0f - kBoxTol;
constexpr float kWidenHi = 1.0f + kBoxTol;
__device__ __forceinline__ float widen_lo(float t) { return __builtin_fmaf(-kBoxTol, fabsf(t), t); }
__device__ __forceinline__ float widen_hi(float t) { return __builtin_fmaf(kBoxTol, fabsf(t), t); }

// Conservative slab test; tlim = largest t still of interest.
__device__ __forceinline__ bool box_hit(const float* lo, const float* hi, const RayBox& rb, float tlim, float& tnear) {
    const float ax = slab_t(lo[0], rb.ix, rb.nox), bx = slab_t(hi[0], rb.ix, rb.nox);
    const float ay = slab_t(lo[1], rb.iy, rb.noy), by = slab_t(hi[1], rb.iy, rb.noy);
    const float az = slab_t(lo[2], rb.iz, rb.noz), bz = slab_t(hi[2], rb.iz, rb.noz);
    float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    tn = widen_lo(tn);
    tf = widen_hi(tf);
    tnear = tn;
    // tn <= tf && tf >= 0 && tn <= tlim, as one compare: every caller's tlim is
    // >= 0 (+inf or t_limit of a positive t), so max(tn, 0) <= min(tf, tlim)
    // states exactly the same three conditions (fewer compares and mask ANDs)
#ifndef RT_BOXFOLD
#define RT_BOXFOLD 1
#endif
    if (RT_BOXFOLD) return fmaxf(tn, 0.0f) <= fminf(tf, tlim);
    return tn <= tf && tf >= 0.0f && tn <= tlim;
}

// box_hit as the whole-LDS walk (nearest_bvh_bl, kNodes 2) runs it, on the box's NEAR bounds
// (lo on an axis with 1/d >= 0, near_is_lo, else hi) and FAR bounds: fma(v, 1/d, -o/d) is
// monotone in v for a fixed ray, so fma(near) = min(fma(lo), fma(hi)) exactly: box_hit's
// interval, without its six min/max.  rt_cull_check probes this function beside box_hit.
__device__ __forceinline__ bool near_is_lo(float inv) { return inv >= 0.0f; }
__device__ __forceinline__ bool box_hit_nf(float nx, float ny, float nz, float fx, float fy, float fz, const RayBox& rb,
                                           float tlim, float& tnear) {
    const float a = fmaxf(fmaxf(slab_t(nx, rb.ix, rb.nox), slab_t(ny, rb.iy, rb.noy)), slab_t(nz, rb.iz, rb.noz));
    const float b = fminf(fminf(slab_t(fx, rb.ix, rb.nox), slab_t(fy, rb.iy, rb.noy)), slab_t(fz, rb.iz, rb.noz));
#if RT_WIDEN_MUL
    // the relative widening as one multiply per bound (§4 item 2): t (1 - tol) for the
    // entry, f (1 + tol) for the exit.  Where the two forms differ (t or f < 0) the
    // compare below clamps t to 0 and a negative exit fails either way; +inf stays +inf
    tnear = a * kWidenLo;
    const float f = b * kWidenHi;
#else
    tnear = widen_lo(a);
    const float f = widen_hi(b);
#endif
    // box_hit's folded test max(t, 0) <= min(f, tlim) as two compares: tlim is never
    // NaN, and !(x > f) holds for a NaN f as min(f, tlim) = tlim does (no
    // canonicalisation of tlim per visit, no min)
    const float x = fmaxf(tnear, 0.0f);
    return x <= tlim && !(x > f);
}

// An f32 bound >= t (t >= 0 or +inf), for culling boxes that start beyond t.
__device__ __forceinline__ float t_limit(double t) {
    float f = static_cast<float>(t);
    if (static_cast<double>(f) < t) f = __uint_as_float(__float_as_uint(f) + 1u);   // next f32 up (t >= 0)
    return f + kBoxTol * f;
}
// ... in the scaled t of the ray's slab tests (t 2^te, exact; te = 0 for unit-length rays)
__device__ __forceinline__ float t_limit(const RayBox& rb, double t) { return t_limit(ldexp(t, rb.te)); }

// The private stack array must stay in scratch: an array small enough for the
// compiler to promote to registers is indexed per lane with divergent indices,
// which compiles to a waterfall loop over the wave's distinct indices (the
// 128-B compact stack measured 130x slower that way).  Passing its address to
// an empty asm statement makes it escape, so it is never promoted.  (Its 32-bit
// scratch offset, not the 64-bit generic pointer: the generic cast's null check
// hit an instruction-selection error in one kernel.)
template <class T>
__device__ __forceinline__ void rt_keep_in_scratch(T* p) {
    asm volatile("" : : "v"(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p))));
}

// Traversal stacks, declared as plain locals so the compiler keeps the stack
// pointer (and the register part) in registers.  The top kReg entries live in
// registers, shifted with v_mov on push/pop (constant indices after
// unrolling); deeper entries live in a private array (scratch, cached in
// L1/L2).  A pop refills the register part from scratch, so the load's
// latency overlaps the traversal work before the entry is needed; with
// kReg = 0 every pop waits for its scratch load.  The nearest query packs
// (node, entry t) into one 64-bit entry: one scratch access per push / pop.
// The host bounds the tree depth, so kBvhStack entries always suffice.
#define RT_STACK_DECL(kReg, E) RT_STACK_DECL_N(kReg, E, kBvhStack)
#define RT_STACK_DECL_N(kReg, E, kN)                                                   \
    E stk_m[kN];                                                                       \
    E stk_r[(kReg) > 0 ? (kReg) : 1];                                                  \
    int stk_n = 0;                                                                     \
    auto stk_push = [&](E v) {                                                         \
        if constexpr ((kReg) > 0) {                                                    \
            if (stk_n >= (kReg)) stk_m[stk_n - (kReg)] = stk_r[(kReg) - 1];            \
            _Pragma("unroll") for (int q = (kReg) - 1; q > 0; --q) stk_r[q] = stk_r[q - 1]; \
            stk_r[0] = v;                                                              \
        } else {                                                                       \
            stk_m[stk_n] = v;                                                          \
        }                                                                              \
        ++stk_n;                                                                       \
    };                                                                                 \
    auto stk_pop = [&]() -> E {                                                        \
        --stk_n;                                                                       \
        if constexpr ((kReg) > 0) {                                                    \
            const E v = stk_r[0];                                                      \
            _Pragma("unroll") for (int q = 0; q < (kReg) - 1; ++q) stk_r[q] = stk_r[q + 1]; \
            if (stk_n >= (kReg)) stk_r[(kReg) - 1] = stk_m[stk_n - (kReg)];            \
            return v;                                                                  \
        } else {                                                                       \
            return stk_m[stk_n];                                                       \
        }                                                                              \
    }

__device__ __forceinline__ uint64_t stk_entry(int32_t node, float t) {
    return (static_cast<uint64_t>(__float_as_uint(t)) << 32) | static_cast<uint32_t>(node);
}
__device__ __forceinline__ int32_t stk_node(uint64_t e) { return static_cast<int32_t>(static_cast<uint32_t>(e)); }
__device__ __forceinline__ float stk_t(uint64_t e) { return __uint_as_float(static_cast<uint32_t>(e >> 32)); }

// Compact 32-bit entries (host: every node index and leaf code fits kBits
// bits signed, depth <= kShortStack): the low kBits bits are the node / leaf
// code (sign-extended), the rest the entry t's top 32 - kBits bits (sign,
// exponent, 23 - kBits mantissa bits: 16 -> 7, 18 -> 5).  Dropping the low
// mantissa bits moves t toward zero: a non-negative t can only get smaller and
// a negative one stays negative, so `t <= tlim` (tlim > 0) culls a subset of
// what the exact t would: the same leaves that can hold the winner are
// visited, and the (t, object) winner does not depend on order.
constexpr int kShortStack = 32;
template <int kBits>
__device__ __forceinline__ uint32_t stk_entry_c(int32_t node, float t) {
    constexpr uint32_t kMask = (1u << kBits) - 1u;
    return (__float_as_uint(t) & ~kMask) | (static_cast<uint32_t>(node) & kMask);
}
template <int kBits>
__device__ __forceinline__ int32_t stk_node_c(uint32_t e) { return static_cast<int32_t>(e << (32 - kBits)) >> (32 - kBits); }
template <int kBits>
__device__ __forceinline__ float stk_t_c(uint32_t e) { return __uint_as_float(e & ~((1u << kBits) - 1u)); }

// Scene::intersect through the BVH.  Same winner as nearest_brute: candidates
// compete on (t, object id), independent of visiting order.
template <bool kCount = false, int kNodes = 0, int kReg = 0>
__device__ __forceinline__ Hit nearest_bvh(const DevScene& sc, const BvhView& v, const Ray& r, Work* w = nullptr) {
    Hit h = nearest_planes(sc, r);
    if (h.nan_t || sc.n_spheres == 0) return h;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    const RayBox rb = make_raybox(r, sc.cull_reach);
    float tlim = h.obj == INT32_MAX ? __builtin_inff() : t_limit(rb, h.t);
    RT_STACK_DECL(kReg, uint64_t);
    int32_t cur = sc.bvh_root;
    for (;;) {
        if (cur >= 0) {
            const DevBvhNode nd = fetch_node<kNodes>(v, cur);
            if constexpr (kCount) w->boxes += 2;
            float t0, t1;
            const bool h0 = box_hit(nd.lo0, nd.hi0, rb, tlim, t0);
            const bool h1 = box_hit(nd.lo1, nd.hi1, rb, tlim, t1);
            if (h0 && h1) {
                const bool first0 = t0 <= t1;
                stk_push(stk_entry(first0 ? nd.c1 : nd.c0, first0 ? t1 : t0));
                cur = first0 ? nd.c0 : nd.c1;
                continue;
            }
            if (h0) { cur = nd.c0; continue; }
            if (h1) { cur = nd.c1; continue; }
        } else {
            const int first = (~cur) >> 3, cnt = ((~cur) & 7) + 1;
            if constexpr (kCount) w->spheres += cnt;
            for (int k = first; k < first + cnt; ++k) {
                double t;
                if (sphere_t(v.sph[k], r, sk, t)) {
                    const int32_t obj = v.obj[k];
                    if (t < h.t || (t == h.t && obj < h.obj)) {
                        h.t = t; h.obj = obj; h.prim = k;
                        tlim = t_limit(rb, t);
                    }
                }
            }
        }
        // pop, skipping entries that the current best already rules out
        for (;;) {
            if (stk_n == 0) return h;
            const uint64_t e = stk_pop();
            cur = stk_node(e);
            if (stk_t(e) <= tlim) break;
        }
    }
}

// nearest_bvh with the inner-node step written branch-light:
// a wave descends inner nodes in one tight loop whose only divergent
// statement is the masked push of the far child, then tests its leaf, then
// pops past the entries the current best rules out.  Same visiting order,
// culling and result as nearest_bvh.
template <bool kCount = false, int kNodes = 0, int kReg = 0, int kCompactBits = 0>
__device__ __forceinline__ Hit nearest_bvh_bl(const DevScene& sc, const BvhView& v, const Ray& r, Work* w = nullptr) {
    Hit h = nearest_planes(sc, r);
    if (h.nan_t || sc.n_spheres == 0) return h;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    const RayBox rb = make_raybox(r, sc.cull_reach);
    float tlim = h.obj == INT32_MAX ? __builtin_inff() : t_limit(rb, h.t);
    // not a node and no leaf code: INT32_MIN (~cur would list 8 spheres at 2^28), or 0 for the
    // byte-offset nodes of the whole-LDS walk (node c is (c + 1) * 8)
    constexpr int32_t kNone = kNodes == 2 ? 0 : INT32_MIN;
    // kReg newest entries in registers (the LDS-prefix source), the rest in scratch;
    // kCompactBits > 0: 32-bit entries with that many code bits, kShortStack of them
    // (128 B of scratch per lane); 0: 64-bit (node, t) entries
    constexpr bool kCompact = kCompactBits > 0;
    using StkE = std::conditional_t<kCompact, uint32_t, uint64_t>;
    RT_STACK_DECL_N(kReg, StkE, (kCompact ? kShortStack : kBvhStack));
    if constexpr (kCompact) rt_keep_in_scratch(stk_m);
    auto mk_entry = [](int32_t node, float t) -> StkE {
        if constexpr (kCompact) return stk_entry_c<kCompactBits>(node, t); else return stk_entry(node, t);
    };
    auto e_node = [](StkE e) -> int32_t {
        if constexpr (kCompact) return stk_node_c<kCompactBits>(e); else return stk_node(e);
    };
    auto e_t = [](StkE e) -> float {
        if constexpr (kCompact) return stk_t_c<kCompactBits>(e); else return stk_t(e);
    };
    // whole tree in LDS (kNodes 2): nodes as byte offsets (stage_node_planes<., true>), 0 = none
    int32_t cur = kNodes == 2 ? node_byte_off(sc.bvh_root) : sc.bvh_root;
    [[maybe_unused]] unsigned long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    // whole tree in LDS: per axis the array of NEAR bound pairs (lo when 1/d >= 0,
    // else hi) and of FAR pairs.  fma(v, 1/d, -o/d) is monotone in v for a fixed
    // ray (1/d != 0), so fma(near) = min(fma(lo), fma(hi)) exactly: box_hit's
    // interval, without its six min/max per child.  Byte bases one pair before
    // node 0, so node byte offset (c + 1) * 8 addresses pair c.
    [[maybe_unused]] const char *nxa = nullptr, *fxa = nullptr, *nya = nullptr, *fya = nullptr, *nza = nullptr,
                                *fza = nullptr, *ca = nullptr;
    if constexpr (kNodes == 2) {
        const char* L = reinterpret_cast<const char*>(v.lnodes) - 8;
        const size_t n8 = static_cast<size_t>(v.nl) * 8;
        nxa = L + (near_is_lo(rb.ix) ? 0 : n8); fxa = L + (near_is_lo(rb.ix) ? n8 : 0);
        nya = L + 2 * n8 + (near_is_lo(rb.iy) ? 0 : n8); fya = L + 2 * n8 + (near_is_lo(rb.iy) ? n8 : 0);
        nza = L + 4 * n8 + (near_is_lo(rb.iz) ? 0 : n8); fza = L + 4 * n8 + (near_is_lo(rb.iz) ? n8 : 0);
        ca = L + 6 * n8;
    }
    for (;;) {
        RT_WSTAMP(q0);
        while (kNodes == 2 ? cur > 0 : cur >= 0) {
            RT_WSTEP(0);
            float t0, t1;
            bool h0, h1;
            int32_t c0, c1;
            if constexpr (kNodes == 2) {
                auto pair = [cur](const char* base) { return *reinterpret_cast<const float2*>(base + cur); };
                const float2 nx = pair(nxa), fx = pair(fxa), ny = pair(nya), fy = pair(fya), nz = pair(nza), fz = pair(fza);
                const int2 cc = *reinterpret_cast<const int2*>(ca + cur);
                h0 = box_hit_nf(nx.x, ny.x, nz.x, fx.x, fy.x, fz.x, rb, tlim, t0);
                h1 = box_hit_nf(nx.y, ny.y, nz.y, fx.y, fy.y, fz.y, rb, tlim, t1);
                c0 = cc.x;
                c1 = cc.y;
            } else {
                const DevBvhNode nd = fetch_node<kNodes>(v, cur);
                h0 = box_hit(nd.lo0, nd.hi0, rb, tlim, t0);
                h1 = box_hit(nd.lo1, nd.hi1, rb, tlim, t1);
                c0 = nd.c0;
                c1 = nd.c1;
            }
            if constexpr (kCount) w->boxes += 2;
            const bool first0 = t0 <= t1;
            if (h0 && h1) stk_push(mk_entry(first0 ? c1 : c0, first0 ? t1 : t0));
            cur = (h0 && (!h1 || first0)) ? c0 : (h1 ? c1 : kNone);
        }
        RT_WSTAMP(q1);
        if (cur != kNone) {
            const int first = (~cur) >> 3, cnt = ((~cur) & 7) + 1;
            if constexpr (kCount) w->spheres += cnt;
            for (int k = first; k < first + cnt; ++k) {
                RT_WSTEP(1);
                double t;
                if (sphere_t<kNodes == 3 ? (RT_BF_HALF != 0) : kNodes == 2 ? (RT_BF_LDS != 0) : (RT_ROOTS_BF != 0)>(v.sph[k], r, sk, t)) {
                    const int32_t obj = v.obj[k];
                    if (t < h.t || (t == h.t && obj < h.obj)) {
                        h.t = t; h.obj = obj; h.prim = k;
                        tlim = t_limit(rb, t);
                    }
                }
            }
        }
        RT_WSTAMP(q2);
        cur = kNone;
        while (stk_n > 0) {
            RT_WSTEP(2);
            const StkE e = stk_pop();
            if (e_t(e) <= tlim) { cur = e_node(e); break; }
        }
        RT_WSTAMP(q3);
#if RT_STAMP
        w->cyc[0] += q1 - q0; w->cyc[1] += q2 - q1; w->cyc[2] += q3 - q2;
#endif
        if (cur == kNone) return h;
    }
}

// The shadow query (see occluded_brute, trace_prims.hpp, for the any-hit equivalence).
template <bool kCount = false, int kNodes = 0, int kReg = 0>
__device__ __forceinline__ bool occluded_bvh(const DevScene& sc, const BvhView& v, const Ray& r, bool has_range,
                                             double r2, int32_t hint = -1, Work* w = nullptr) {
    bool plane_block = false;
    for (int i = 0; i < sc.n_planes; ++i) {
        double t;
        if (!plane_t(sc.planes[i], r, t)) continue;
        if (!has_range) return true;
        if (t != t) return false;
        plane_block |= t * t < r2;
    }
    if (plane_block) return true;
    if (sc.n_spheres == 0) return false;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    if (hint >= 0) {                     // see occluded_bvh4 (trace_bvh4.hpp)
        if constexpr (kCount) ++w->spheres;
        double t;
        if (sphere_t(v.sph[hint], r, sk, t) && (!has_range || t * t < r2)) return true;
    }
    const RayBox rb = make_raybox(r, sc.cull_reach);
    // t*t < r2 implies t < sqrt(r2) (up to rounding, covered by t_limit's margin)
    const float tlim = has_range ? t_limit(rb, sqrt(r2)) : __builtin_inff();
    RT_STACK_DECL(kReg, int32_t);
    int32_t cur = sc.bvh_root;
    for (;;) {
        if (cur >= 0) {
            const DevBvhNode nd = fetch_node<kNodes>(v, cur);
            if constexpr (kCount) w->boxes += 2;
            float t0, t1;
            const bool h0 = box_hit(nd.lo0, nd.hi0, rb, tlim, t0);
            const bool h1 = box_hit(nd.lo1, nd.hi1, rb, tlim, t1);
            if (h0 && h1) {
                const bool first0 = t0 <= t1;
                stk_push(first0 ? nd.c1 : nd.c0);
                cur = first0 ? nd.c0 : nd.c1;
                continue;
            }
            if (h0) { cur = nd.c0; continue; }
            if (h1) { cur = nd.c1; continue; }
        } else {
            const int first = (~cur) >> 3, cnt = ((~cur) & 7) + 1;
            if constexpr (kCount) w->spheres += cnt;
            for (int k = first; k < first + cnt; ++k) {
                double t;
                if (sphere_t(v.sph[k], r, sk, t) && (!has_range || t * t < r2)) return true;
            }
        }
        if (stk_n == 0) return false;
        cur = stk_pop();
    }
}

}  // namespace rtamd
