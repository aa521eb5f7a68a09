// The exact primitives: the division and square root as gfx950 computes them, the sphere and
// plane tests (shapes.rs), and the scans that test every object.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "trace_types.hpp"

namespace rtamd {

// The per-ray constants of shapes.rs:60-89's quadratic: a2 = 2.0*a and
// a4 = 4.0*a (the same f64 products the reference forms per test) and the
// reciprocal of a2 refined exactly as gfx950's f64 division refines its
// denominator (v_rcp_f64, then two Newton steps r += r*(1 - a2*r)).  `win` is
// the exponent window of numerators div_a2 may finish with that hoisted
// reciprocal (0: none, the ray's a2 is outside [2^-100, 2^101)).
struct SphK {
    double a2, a4, ra2;
    uint32_t win;
};

// Any denominator d (RT_DIVK: the normalisations' three divisions by one length): the same
// reciprocal and window, and div_by below the same three operations as div_a2 -- which is
// div_by with d = 2a, so rt_div_a2_check pins both.
struct DivK {
    double d, rd;
    uint32_t win;
};

__device__ __forceinline__ DivK div_k(double d) {
    DivK k;
    k.d = d;
    double r = __builtin_amdgcn_rcp(d);
    double e = fma(-d, r, 1.0);
    r = fma(r, e, r);
    e = fma(-d, r, 1.0);
    k.rd = fma(r, e, r);
    const uint32_t ed = (static_cast<uint32_t>(__double2hiint(d)) >> 20) & 0x7FFu;
    k.win = ed - 923u < 201u ? 1500u : 0u;
    return k;
}

__device__ __forceinline__ SphK sphere_k(double a) {
    const DivK d = div_k(2.0 * a);
    SphK k;
    k.a2 = d.d;
    k.a4 = 4.0 * a;
    k.ra2 = d.rd;
    k.win = d.win;
    return k;
}

// x / a2, correctly rounded.  The compiler's f64 division is v_div_scale (of
// numerator and denominator), that reciprocal, q0 = x*r, e = fma(-a2, q0, x),
// v_div_fmas = fma(e, r, q0), v_div_fixup.  With a2 in [2^-100, 2^101) and
// |x| in [2^-900, 2^600) (biased exponent 123..1622) div_scale scales neither
// operand (exponent gap < 768, no denormal quotient or reciprocal, x not tiny)
// and div_fixup returns q with sign(x), so the three operations below give the
// division's bits; any other x (0, denormal, huge, inf, NaN) takes the division.
__device__ __forceinline__ double div_by(double x, const DivK& k) {
    const uint32_t ex = (static_cast<uint32_t>(__double2hiint(x)) >> 20) & 0x7FFu;
    if (ex - 123u < k.win) {
        const double q0 = x * k.rd;
        const double e = fma(-k.d, q0, x);
        return fma(e, k.rd, q0);
    }
    return x / k.d;
}

__device__ __forceinline__ double div_a2(double x, const SphK& k) { return div_by(x, DivK{k.a2, k.ra2, k.win}); }

// sqrt(x) as gfx950's correctly rounded f64 square root computes it (the compiler's
// sequence: v_rsq_f64 refined by Goldschmidt / Newton steps), without the parts that
// do nothing for x in [2^-767, +inf): the sequence scales x by 2^256 when x < 2^-767
// (and its result by 2^-128), which is ldexp by 0 here, and returns x itself for +-0
// and +inf, which x is not.  So for those x the core below gives the sequence's bits
// (pinned on the device against sqrt(): rt_sqrt_check, tests/test_gpu_division.py);
// any other x (tiny, denormal, 0, inf, NaN, negative) takes sqrt().
#ifndef RT_WSQRT
#define RT_WSQRT 1
#endif
// RT_DIVK: the normalisations (hit normal, light direction, half vector, camera ray) as
// div_k / div_by and sqrt_win (round 6, same box: C3 2.790 vs 2.806 ms, 8-way share 0.655-0.658
// vs 0.658-0.662 ms, C4 49.05 vs 49.24 ms, C5 291.0 vs 294.9 ms; exact: the GPU suite is green)
#ifndef RT_DIVK
#define RT_DIVK 1
#endif
__device__ __forceinline__ double sqrt_win(double x) {
    if (RT_WSQRT && x >= 0x1p-767 && x < __builtin_huge_val()) {
        const double y = __builtin_amdgcn_rsq(x);
        double g = x * y, h = y * 0.5;
        const double r = fma(-h, g, 0.5);
        g = fma(g, r, g);
        h = fma(h, r, h);
        double d = fma(-g, g, x);
        g = fma(d, h, g);
        d = fma(-g, g, x);
        return fma(d, h, g);
    }
    return sqrt(x);
}

// shapes.rs:60-89, split in two: sphere_disc forms b and the discriminant (the
// miss path, every test), sphere_roots the rest for disc > 0: t1, or t2 when t1 <= 0.
__device__ __forceinline__ double sphere_disc(const DevSphere& s, const Ray& r, const SphK& k, double& b) {
    const double ocx = r.ox - s.cx, ocy = r.oy - s.cy, ocz = r.oz - s.cz;
    b = 2.0 * (r.dx * ocx + r.dy * ocy + r.dz * ocz);
    const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - s.rr;
    return b * b - k.a4 * cc;
}

// kBF: the branch-free form (both quotients straight-line) or the branchy one (a division only
// for a positive numerator, the second root only when the first is behind).  Round 6, same box:
// C3 2.912-2.917 vs 2.924-2.930 ms branch-free everywhere, but C5 305.3 vs 294.6 ms and C4 49.46 vs
// 49.27 ms; the binary16 walk of trees beyond LDS (RT_BF_HALF) takes the branchy form.
#ifndef RT_ROOTS_BF
#define RT_ROOTS_BF 1
#endif
#ifndef RT_BF_HALF
#define RT_BF_HALF 0
#endif
#ifndef RT_BF_LDS
#define RT_BF_LDS 1
#endif
template <bool kBF = (RT_ROOTS_BF != 0)>
__device__ __forceinline__ bool sphere_roots(double b, double disc, const SphK& k, double& t) {
    const double sq = sqrt_win(disc);
    if constexpr (kBF) {
    // both roots' quotients straight-line (div_a2's three operations, whose result for x <= 0 or NaN is
    // never > 0), the real division only for a positive numerator outside the window (rare)
    const double x1 = -b - sq, x2 = -b + sq;
    auto fast = [&](double x) {
        const double q0 = x * k.ra2;
        const double e = fma(-k.a2, q0, x);
        return fma(e, k.ra2, q0);
    };
    auto in_win = [&](double x) { return ((static_cast<uint32_t>(__double2hiint(x)) >> 20) & 0x7FFu) - 123u < k.win; };
    double t1 = fast(x1), t2 = fast(x2);
    const bool slow1 = x1 > 0.0 && !in_win(x1), slow2 = x2 > 0.0 && !in_win(x2);
    if (slow1 || slow2) {
        if (slow1) t1 = x1 / k.a2;
        if (slow2) t2 = x2 / k.a2;
    }
    const bool h1 = t1 > 0.0;
    t = h1 ? t1 : t2;
    return h1 || t2 > 0.0;
    } else {
    // a2 >= 0 (or NaN): x <= 0 or NaN gives x / a2 <= 0, -0 or NaN, never > 0, so the
    // division is skipped there (a root behind the origin)
    const double x1 = -b - sq;
    if (x1 > 0.0) {
        const double t1 = div_a2(x1, k);
        if (t1 > 0.0) { t = t1; return true; }
    }
    const double x2 = -b + sq;
    if (x2 > 0.0) {
        const double t2 = div_a2(x2, k);
        if (t2 > 0.0) { t = t2; return true; }
    }
    return false;
    }
}

// The exact quadratic; true + the t the reference returns, or false for None.
template <bool kBF = (RT_ROOTS_BF != 0)>
__device__ __forceinline__ bool sphere_t(const DevSphere& s, const Ray& r, const SphK& k, double& t) {
    double b;
    const double disc = sphere_disc(s, r, k, b);
    return disc > 0.0 && sphere_roots<kBF>(b, disc, k, t);
}

// shapes.rs:100-112: t = n.(p - o) / n.d ; None iff t <= 0 (a NaN t is a hit).
__device__ __forceinline__ bool plane_t(const DevPlane& p, const Ray& r, double& t) {
    const double ex = p.px - r.ox, ey = p.py - r.oy, ez = p.pz - r.oz;
    t = (p.nx * ex + p.ny * ey + p.nz * ez) / (p.nx * r.dx + p.ny * r.dy + p.nz * r.dz);
    return !(t <= 0.0);
}

// The nearest plane among P[0, n) with object ids O (always brute force: few, and they carry the
// NaN quirk).
__device__ __forceinline__ Hit nearest_planes_at(const DevPlane* P, const int32_t* O, int n, const Ray& r) {
    Hit h;
    h.t = __builtin_huge_val();
    h.obj = INT32_MAX;
    h.prim = 0;
    h.nan_t = false;
    for (int i = 0; i < n; ++i) {
        double t;
        if (!plane_t(P[i], r, t)) continue;
        const int32_t obj = O[i];
        if (t != t) {
            if (!h.nan_t) { h.nan_t = true; h.t = t; h.obj = obj; h.prim = ~i; }
        } else if (!h.nan_t && (t < h.t || (t == h.t && obj < h.obj))) {
            h.t = t; h.obj = obj; h.prim = ~i;
        }
    }
    return h;
}

// ... among the scene's own arrays.
__device__ __forceinline__ Hit nearest_planes(const DevScene& sc, const Ray& r) {
    return nearest_planes_at(sc.planes, sc.plane_obj, sc.n_planes, r);
}

// Scene::intersect (scene.rs:247-249), brute force: every object tested.
// min_by_key(FloatNotNan(t)): a NaN t (only a plane can produce one) is the
// minimum key and the first in file order wins outright; otherwise smallest t,
// ties to the FIRST object in file order.
template <bool kCount = false, class SpherePtr>
__device__ __forceinline__ Hit nearest_brute(const DevScene& sc, SpherePtr S, const Ray& r, Work* w = nullptr) {
    Hit h;
    h.t = __builtin_huge_val();
    h.obj = INT32_MAX;
    h.prim = 0;
    h.nan_t = false;
    for (int i = 0; i < sc.n_planes; ++i) {
        double t;
        if (!plane_t(sc.planes[i], r, t)) continue;
        const int32_t obj = sc.plane_obj[i];
        if (t != t) {
            if (!h.nan_t) { h.nan_t = true; h.t = t; h.obj = obj; h.prim = ~i; }
        } else if (!h.nan_t && (t < h.t || (t == h.t && obj < h.obj))) {
            h.t = t; h.obj = obj; h.prim = ~i;
        }
    }
    if (h.nan_t) return h;      // no sphere can produce a NaN t
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;     // direction.sqnorm()
    const SphK sk = sphere_k(a);
    const int n = sc.n_spheres;
    if constexpr (kCount) w->spheres += n;
#pragma unroll 2
    for (int i = 0; i < n; ++i) {
        const DevSphere s = S[i];
        double t;
        if (sphere_t(s, r, sk, t)) {
            const int32_t obj = sc.sphere_obj[i];
            if (t < h.t || (t == h.t && obj < h.obj)) { h.t = t; h.obj = obj; h.prim = i; }
        }
    }
    return h;
}

// The shadow test of raytrace.rs:41-49: `intersect(shadow ray)` is Some and
// (range is None or t*t < range).  Equivalent any-hit form:
//  * no range (directional light): shadowed iff ANY object reports a hit;
//  * with range (point light): if any plane reports a NaN t the nearest hit
//    is that NaN hit and NaN*NaN < r2 is false -> lit; otherwise shadowed iff
//    SOME hit has t*t < r2 (t_min <= t_i and rounding is monotone, so the
//    nearest one then qualifies too).
template <bool kCount = false, class SpherePtr>
__device__ __forceinline__ bool occluded_brute(const DevScene& sc, SpherePtr S, const Ray& r, bool has_range, double r2,
                                               Work* w = nullptr) {
    bool plane_block = false;
    for (int i = 0; i < sc.n_planes; ++i) {
        double t;
        if (!plane_t(sc.planes[i], r, t)) continue;
        if (!has_range) return true;
        if (t != t) return false;
        plane_block |= t * t < r2;
    }
    if (plane_block) return true;
    const double a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    const SphK sk = sphere_k(a);
    const int n = sc.n_spheres;
    for (int i = 0; i < n; ++i) {
        const DevSphere s = S[i];
        double t;
        if constexpr (kCount) ++w->spheres;
        if (sphere_t(s, r, sk, t)) {
            if (!has_range || t * t < r2) return true;
        }
    }
    return false;
}

}  // namespace rtamd
