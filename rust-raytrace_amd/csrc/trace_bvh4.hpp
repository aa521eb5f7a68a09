// The 4-wide tree (shadow queries) and the quantised 4-wide tree (nearest hits).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "trace_types.hpp"
#include "trace_prims.hpp"
#include "trace_view.hpp"
#include "trace_bvh.hpp"

namespace rtamd {

// ---- 4-wide BVH --------------------------------------------------------
// One node visit tests the 4 child boxes (same conservative slab test); the
// shadow query takes the hit children in slot order.  Misses are marked by the child pointer (kBvh4Empty), never by t, so a box
// hit at t = +inf is still visited.
struct Node4Hits {
    float t[4];
    int32_t c[4];
};

__device__ __forceinline__ Node4Hits node4_test(const BvhView& v, int32_t node, const RayBox& rb, float tlim) {
    // axis by axis (as box_hit, same operations), so only two planes are live at a time
    const int32_t N = v.n4;
    const DevBvh4Plane* P = v.p4 + node;
    float tn[4], tf[4];
    {
        const DevBvh4Plane lo = P[0], hi = P[N];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = slab_t(lo.f[k], rb.ix, rb.nox), b = slab_t(hi.f[k], rb.ix, rb.nox);
            tn[k] = fminf(a, b);
            tf[k] = fmaxf(a, b);
        }
    }
    {
        const DevBvh4Plane lo = P[2 * N], hi = P[3 * N];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = slab_t(lo.f[k], rb.iy, rb.noy), b = slab_t(hi.f[k], rb.iy, rb.noy);
            tn[k] = fmaxf(tn[k], fminf(a, b));
            tf[k] = fminf(tf[k], fmaxf(a, b));
        }
    }
    {
        const DevBvh4Plane lo = P[4 * N], hi = P[5 * N];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = slab_t(lo.f[k], rb.iz, rb.noz), b = slab_t(hi.f[k], rb.iz, rb.noz);
            tn[k] = fmaxf(tn[k], fminf(a, b));
            tf[k] = fminf(tf[k], fmaxf(a, b));
        }
    }
    const DevBvh4Plane ch = P[6 * N];
    Node4Hits o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float n = widen_lo(tn[k]);
        const float f = widen_hi(tf[k]);
        const bool hit = n <= f && f >= 0.0f && n <= tlim && ch.i[k] != kBvh4Empty;
        o.t[k] = hit ? n : __builtin_inff();
        o.c[k] = hit ? ch.i[k] : kBvh4Empty;
    }
    return o;
}

// `hint`: a sphere (leaf-order index, or -1) tested before the traversal: the
// sphere the shadow ray starts on, which occludes it whenever the light is
// behind that surface.  Any-hit: testing one sphere early cannot change the
// answer (and the planes, with the NaN rule, are decided before it).
template <bool kCount = false>
__device__ __forceinline__ bool occluded_bvh4(const DevScene& sc, const BvhView& v, const Ray& r, bool has_range,
                                              double r2, int32_t hint, Work* w = nullptr) {
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
    if (hint >= 0) {
        if constexpr (kCount) ++w->spheres;
        double t;
        if (sphere_t(v.sph[hint], r, sk, t) && (!has_range || t * t < r2)) return true;
    }
    const RayBox rb = make_raybox(r, sc.cull_reach);
    const float tlim = has_range ? t_limit(rb, sqrt(r2)) : __builtin_inff();
    // pushes are unconditional stores at the stack top (junk when nothing is
    // pushed; the next push overwrites it): no branch per child
    int32_t stk_m[kBvh4Stack];
    int stk_n = 0;
    int32_t cur = sc.bvh4_root;
    for (;;) {
        if (cur >= 0) {
            // slot order (measured: near-to-far sorting costs more than it saves here)
            const Node4Hits n = node4_test(v, cur, rb, tlim);
            if constexpr (kCount) w->boxes += 4;
            int32_t next = kBvh4Empty;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool hk = n.c[k] != kBvh4Empty;
                if (hk && next != kBvh4Empty) stk_m[stk_n++] = next;
                next = hk ? n.c[k] : next;
            }
            if (next != kBvh4Empty) { cur = next; continue; }
        } else {
            const int first = (~cur) >> 3, cnt = ((~cur) & 7) + 1;
            if constexpr (kCount) w->spheres += cnt;
            for (int k = first; k < first + cnt; ++k) {
                double t;
                if (sphere_t(v.sph[k], r, sk, t) && (!has_range || t * t < r2)) return true;
            }
        }
        if (stk_n == 0) return false;
        cur = stk_m[--stk_n];
    }
}

// ---- quantised 4-wide tree (DevQNode4) -----------------------------------------
// Scene::intersect (scene.rs:247-249) through the 4-wide tree whose child boxes
// are 8-bit multiples of a per-node power-of-two step (host_bvh.cpp
// quantize_bvh4).  A bound decodes exactly: fma(q, s, m * s) = (m + q) * s is an
// f32 value (|m + q| < 2^24, s a power of two in the normal range), and it lies
// outside the f32 child box (rounded outward), so the slab test below is the
// f32 tree's test on a box that contains that one: it culls a subset of what
// the f32 test culls.  The nearest hit child is
// entered first, the other hit children pushed far-to-near (64-bit entries:
// the entry t and the node index, or kQ4LeafTag | first << 3 | count - 1);
// leaves get the exact f64 test and the winner is the lexicographic (t,
// object id) minimum over every tested sphere, as for the binary tree.
// kAll: every node in LDS (ds reads); else nodes [0, nq) from LDS and the rest
// through L2 by one flat load (the same 48-B layout on both sides).
constexpr uint32_t kQ4LeafTag = 0x80000000u;

__device__ __forceinline__ float q4_step(int32_t f) { return __uint_as_float((static_cast<uint32_t>(f) >> 24) << 23); }
__device__ __forceinline__ float q4_byte(uint32_t w, int k) { return static_cast<float>((w >> (8 * k)) & 0xFFu); }

template <bool kCount = false, bool kAll = true>
__device__ __forceinline__ Hit nearest_q4(const DevScene& sc, const BvhView& v, const Ray& r, Work* w = nullptr) {
    Hit h = nearest_planes(sc, r);
    if (h.nan_t || sc.n_spheres == 0) return h;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    const RayBox rb = make_raybox(r, sc.cull_reach);
    float tlim = h.obj == INT32_MAX ? __builtin_inff() : t_limit(rb, h.t);
    const bool fx = rb.ix < 0.0f, fy = rb.iy < 0.0f, fz = rb.iz < 0.0f;     // near slab bound = hi
    RT_STACK_DECL_N(0, uint64_t, kQ4Stack);
    rt_keep_in_scratch(stk_m);
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    uint32_t cur = 0;                                            // the root: inner node 0
    for (;;) {
        while (cur < kQ4LeafTag) {
            DevQNode4 nd;
            if constexpr (kAll) nd = v.q4l[cur];
            else nd = *(static_cast<int32_t>(cur) < v.nq ? v.q4l + cur : v.q4g + cur);
            const float sx = q4_step(nd.frame[0]), sy = q4_step(nd.frame[1]), sz = q4_step(nd.frame[2]);
            const float ox = static_cast<float>((nd.frame[0] << 8) >> 8) * sx;      // m * s, exact
            const float oy = static_cast<float>((nd.frame[1] << 8) >> 8) * sy;
            const float oz = static_cast<float>((nd.frame[2] << 8) >> 8) * sz;
            const uint32_t nxw = fx ? nd.hi[0] : nd.lo[0], fxw = fx ? nd.lo[0] : nd.hi[0];
            const uint32_t nyw = fy ? nd.hi[1] : nd.lo[1], fyw = fy ? nd.lo[1] : nd.hi[1];
            const uint32_t nzw = fz ? nd.hi[2] : nd.lo[2], fzw = fz ? nd.lo[2] : nd.hi[2];
            float t[4];
            uint32_t c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float tn = fmaxf(fmaxf(slab_t(__builtin_fmaf(q4_byte(nxw, k), sx, ox), rb.ix, rb.nox),
                                             slab_t(__builtin_fmaf(q4_byte(nyw, k), sy, oy), rb.iy, rb.noy)),
                                       slab_t(__builtin_fmaf(q4_byte(nzw, k), sz, oz), rb.iz, rb.noz));
                const float tf = fminf(fminf(slab_t(__builtin_fmaf(q4_byte(fxw, k), sx, ox), rb.ix, rb.nox),
                                             slab_t(__builtin_fmaf(q4_byte(fyw, k), sy, oy), rb.iy, rb.noy)),
                                       slab_t(__builtin_fmaf(q4_byte(fzw, k), sz, oz), rb.iz, rb.noz));
                const float n = widen_lo(tn);
                const uint32_t ref = nd.child[k];
                const bool hit = fmaxf(n, 0.0f) <= fminf(widen_hi(tf), tlim) && ref != kQ4Empty;
                t[k] = hit ? n : __builtin_inff();
                c[k] = !hit ? kNone
                       : ref < kQ4Leaf ? ref
                                       : kQ4LeafTag | ((nd.base + ((ref >> 3) & 0xFFFu)) << 3) | (ref & 7u);
            }
            if constexpr (kCount) w->boxes += 4;
            // near-to-far: misses (t = +inf, c = kNone) sort last
#define RT_Q4CAS(i, j)                                                              \
            {                                                                       \
                const bool sw = t[j] < t[i];                                        \
                const float ti = t[i]; const uint32_t ci = c[i];                    \
                t[i] = sw ? t[j] : ti; c[i] = sw ? c[j] : ci;                       \
                t[j] = sw ? ti : t[j]; c[j] = sw ? ci : c[j];                       \
            }
            RT_Q4CAS(0, 1) RT_Q4CAS(2, 3) RT_Q4CAS(0, 2) RT_Q4CAS(1, 3) RT_Q4CAS(1, 2)
#undef RT_Q4CAS
#pragma unroll
            for (int k = 3; k >= 1; --k)
                if (c[k] != kNone) stk_push(stk_entry(static_cast<int32_t>(c[k]), t[k]));
            cur = c[0];
        }
        if (cur != kNone) {
            const int first = static_cast<int>((cur & ~kQ4LeafTag) >> 3), cnt = static_cast<int>(cur & 7u) + 1;
            if constexpr (kCount) w->spheres += cnt;
            for (int k = first; k < first + cnt; ++k) {
                double tt;
                if (sphere_t(v.sph[k], r, sk, tt)) {
                    const int32_t obj = v.obj[k];
                    if (tt < h.t || (tt == h.t && obj < h.obj)) {
                        h.t = tt; h.obj = obj; h.prim = k;
                        tlim = t_limit(rb, tt);
                    }
                }
            }
        }
        cur = kNone;
        while (stk_n > 0) {
            const uint64_t e = stk_pop();
            if (stk_t(e) <= tlim) { cur = static_cast<uint32_t>(stk_node(e)); break; }
        }
        if (cur == kNone) return h;
    }
}

}  // namespace rtamd
