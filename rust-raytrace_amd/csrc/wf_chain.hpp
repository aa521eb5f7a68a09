// What the shading kernels (wf_shade.hip), the fold (wf_fold.hip) and the fused tail
// (wf_tail.hip), which does both in registers, share: a shade record's load and Phong sum, the
// shadow mask through the light-view grids, and the fold of a chain's levels.
#pragma once
#include "wf_device.hpp"

namespace rtamd {
namespace {

// A shade record's fields (loaded ahead of its shading by wf_shade).
struct ShadeIn {
    double ptx, pty, ptz, dx, dy, dz, sig;
    int32_t obj, prim;
    uint32_t c, mask;
};

__device__ __forceinline__ ShadeIn shade_load(const WfBufs& b, size_t at, bool mask) {
    ShadeIn in;
    in.ptx = ldn_if<2>(&b.rf(0)[at]); in.pty = ldn_if<2>(&b.rf(1)[at]); in.ptz = ldn_if<2>(&b.rf(2)[at]);
    in.dx = ldn_if<2>(&b.rf(3)[at]); in.dy = ldn_if<2>(&b.rf(4)[at]); in.dz = ldn_if<2>(&b.rf(5)[at]);
    in.sig = ldn_if<2>(&b.rf(6)[at]);
    in.obj = static_cast<int32_t>(ldn_if<2>(&b.ru(0)[at]));
    in.prim = static_cast<int32_t>(ldn_if<2>(&b.ru(1)[at]));
    in.c = ldn_if<2>(&b.ru(2)[at]);                         // the record's chain
    in.mask = mask ? b.ru(3)[at] : 0u;
    return in;
}

// What a shading leaves for the fused tail: the local colour, whether the hit
// reflects, its Schlick factor and the normal turned toward the ray.
struct ShadeOut {
    Col res;
    bool specular;
    double f, nx, ny, nz;
};

// The Phong sum of one shade record of generation k (raytrace.rs:31-56) with
// the shadow mask of its lights (bit l set: light l shadowed): a specular hit
// pushes the level's local colour (its reflection ray was already queued by
// wf_nearest); any other hit ends the chain with it.  kTerm = false (the fused
// tail): a non-specular hit's colour is returned for the caller's in-register
// fold instead of being written as the chain's terminal.
template <bool kFresnel, bool kTerm = true, bool kPack = false>
__device__ __forceinline__ ShadeOut shade_compute(const DevScene& sc, const WfBufs& b, int k, const ShadeIn& in) {
    const double ptx = in.ptx, pty = in.pty, ptz = in.ptz, dx = in.dx, dy = in.dy, dz = in.dz, sig = in.sig;
    const int32_t obj = in.obj;
    const uint32_t c = in.c, mask = in.mask;
    const DevMaterial& m = sc.mats[obj];
    Col res{m.amb[0], m.amb[1], m.amb[2]};                               // raytrace.rs:32
    double nx, ny, nz;
    hit_normal(sc, sc.spheres, in.prim, ptx, pty, ptz, nx, ny, nz);
    const double nd = nx * dx + ny * dy + nz * dz;
    const Shading sh = shading_flags<kFresnel>(m, sig, nd);
    const bool diffuse = sh.diffuse, specular = sh.specular;
    if (nd > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    for (int l = 0; l < sc.n_lights; ++l) {
        if ((mask >> l) & 1u) continue;                                  // shadowed (raytrace.rs:42-49)
        const DevLight& L = sc.lights[l];
        double lx, ly, lz, r2;
        light_dir(L, ptx, pty, ptz, lx, ly, lz, r2);
        add_light(res, m, L, diffuse, specular, sh.f, lx, ly, lz, nx, ny, nz, dx, dy, dz);
    }
    if (specular) {
        const size_t st = static_cast<size_t>(k) * b.capa + c;
        if constexpr (kPack) {
            store_level(b, st, res, kFresnel && m.kind == kMatFresnel ? sh.f : 1.0);
            stn(&b.lobj()[st], obj);
        } else {
            stn(&b.lf(0)[st], res.r); stn(&b.lf(1)[st], res.g); stn(&b.lf(2)[st], res.b);
            stn(&b.lobj()[st], obj);
            if (kFresnel && m.kind == kMatFresnel) stn(&b.lf(3)[st], sh.f);
        }
    } else if (kTerm) {
        set_terminal(b, c, res, k);
    }
    return ShadeOut{res, specular, sh.f, nx, ny, nz};
}

// The shadow mask of a lit hit at (ptx, pty, ptz) on sphere `prim` through the
// light-view grids (raytrace.rs:39-49; the host checked every light has one):
// the operations of wf_occlusion's grid source.
template <bool kCount>
__device__ __forceinline__ uint32_t grid_shadow_mask(const DevScene& sc, const BvhView& v, double ptx, double pty,
                                                     double ptz, int32_t prim, Work& wsh) {
    uint32_t mask = 0;
    for (int l = 0; l < sc.n_lights; ++l) {
        double lx, ly, lz, r2;
        (void)light_dir(sc.lights[l], ptx, pty, ptz, lx, ly, lz, r2);
        const Ray sray{ptx + lx * kEps, pty + ly * kEps, ptz + lz * kEps, lx, ly, lz};
        if (occluded_lgrid<kCount>(sc, v, sc.lgrid[l], sray, r2, ptx, pty, ptz, prim, &wsh)) mask |= 1u << l;
    }
    return mask;
}

// The fold factor of a level is the specular colour of its object times, for
// FresnelMaterial, the level's Schlick factor (raytrace.rs:63 / 163).  The chain is folded inner-first exactly as the
// recursion returns (acc = res_k + ks_k * acc); the loads of four levels are
// issued together so a pixel costs about two memory round trips per four
// levels instead of two per level.
// The level's factor f comes with its colour (WfLevel: the writer stored 1.0 for
// a hit that is not Fresnel), so the only dependent fetch is ks by the level's
// object (an LDS copy of every object's ks measured within noise: DESIGN.md §9).
// kPack false: the levels in the word-per-array form (levels_packed, device_layout.hpp).
template <bool kFresnel>
__device__ __forceinline__ Col fold_level_words(const DevScene& sc, const WfBufs& b, uint32_t p, int nlev, Col acc) {
    constexpr int U = RT_FOLD_UNROLL;
    for (int k = nlev - 1; k >= 0; k -= U) {
        double sr[U], sg[U], sb[U];
        int32_t ob[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k - u >= 0) {
                const size_t at = static_cast<size_t>(k - u) * b.capa + p;
                ob[u] = ldn_if<kNtFold>(&b.lobj()[at]);
                sr[u] = ldn_if<kNtFold>(&b.lf(0)[at]); sg[u] = ldn_if<kNtFold>(&b.lf(1)[at]); sb[u] = ldn_if<kNtFold>(&b.lf(2)[at]);
            }
        }
        double kr[U], kg[U], kb[U], kf[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k - u >= 0) {
                const DevMaterial& m = sc.mats[ob[u]];
                kr[u] = m.ks[0]; kg[u] = m.ks[1]; kb[u] = m.ks[2];
                kf[u] = kFresnel && m.kind == kMatFresnel ? ldn_if<kNtFold>(&b.lf(3)[static_cast<size_t>(k - u) * b.capa + p]) : 1.0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k - u >= 0) {                  // res + (ks * child) * f, f = 1 for Phong (raytrace.rs:63 / 163)
                acc.r = sr[u] + (kr[u] * acc.r) * kf[u];
                acc.g = sg[u] + (kg[u] * acc.g) * kf[u];
                acc.b = sb[u] + (kb[u] * acc.b) * kf[u];
            }
        }
    }
    return acc;
}
template <bool kFresnel, bool kPack>
__device__ __forceinline__ Col fold_levels(const DevScene& sc, const WfBufs& b, uint32_t p, int nlev, Col acc) {
    if constexpr (!kPack) return fold_level_words<kFresnel>(sc, b, p, nlev, acc);
    constexpr int U = RT_FOLD_UNROLL;
    for (int k = nlev - 1; k >= 0; k -= U) {
        WfLevel lv[U];
        int32_t ob[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k - u >= 0) {
                const size_t at = static_cast<size_t>(k - u) * b.capa + p;
                ob[u] = ldn_if<kNtFold>(&b.lobj()[at]);
                lv[u] = load_level<kFresnel>(b, at);
            }
        }
        double kr[U], kg[U], kb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k - u >= 0) {
                const DevMaterial& m = sc.mats[ob[u]];
                kr[u] = m.ks[0]; kg[u] = m.ks[1]; kb[u] = m.ks[2];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k - u >= 0) {                  // res + (ks * child) * f, f = 1 for Phong (raytrace.rs:63 / 163)
                const double kf = kFresnel ? lv[u].f : 1.0;
                acc.r = lv[u].r + (kr[u] * acc.r) * kf;
                acc.g = lv[u].g + (kg[u] * acc.g) * kf;
                acc.b = lv[u].b + (kb[u] * acc.b) * kf;
            }
        }
    }
    return acc;
}

}  // namespace
}  // namespace rtamd
