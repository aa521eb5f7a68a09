// Shading: the hit's normal, the light directions, the material flags and one light's terms.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "trace_types.hpp"
#include "trace_rng.hpp"
#include "trace_prims.hpp"

namespace rtamd {

// The surface normal the reference's intersect() returned for the winner:
// sphere normalize(ray.cast(t) - center) (shapes.rs:61,66); plane: as in the
// file (shapes.rs:108).  pt == ray.cast(t) bit-for-bit.
__device__ __forceinline__ void hit_normal(const DevScene& sc, const DevSphere* S, int32_t prim, double ptx, double pty,
                                           double ptz, double& nx, double& ny, double& nz) {
    if (prim >= 0) {
        const DevSphere s = S[prim];
        const double ux = ptx - s.cx, uy = pty - s.cy, uz = ptz - s.cz;
#if RT_DIVK
        const DivK l = div_k(sqrt_win(ux * ux + uy * uy + uz * uz));
        nx = div_by(ux, l); ny = div_by(uy, l); nz = div_by(uz, l);
#else
        const double l = sqrt(ux * ux + uy * uy + uz * uz);
        nx = ux / l; ny = uy / l; nz = uz / l;
#endif
    } else {
        const DevPlane& p = sc.planes[~prim];
        nx = p.nx; ny = p.ny; nz = p.nz;
    }
}

// Light direction and squared range (scene.rs:122-138).  Returns has_range.
__device__ __forceinline__ bool light_dir(const DevLight& L, double ptx, double pty, double ptz, double& lx, double& ly,
                                          double& lz, double& r2) {
    if (L.kind == 0) {                       // PointLight
        const double vx = L.v[0] - ptx, vy = L.v[1] - pty, vz = L.v[2] - ptz;
        r2 = vx * vx + vy * vy + vz * vz;    // location.sqdist(pt)
#if RT_DIVK
        const DivK l = div_k(sqrt_win(r2));  // == norm of the same vector
        lx = div_by(vx, l); ly = div_by(vy, l); lz = div_by(vz, l);
#else
        const double l = sqrt(r2);           // == norm of the same vector
        lx = vx / l; ly = vy / l; lz = vz / l;
#endif
        return true;
    }
    lx = -L.v[0]; ly = -L.v[1]; lz = -L.v[2];  // DirectionalLight: -direction, not normalised
    r2 = 0.0;
    return false;
}

// AreaLight (scene.rs:142-155): a PointLight at origin + side1*u + side2*w, u
// drawn before w, both keyed on the hit's path key and the light's index.
__device__ __forceinline__ bool light_dir_keyed(const DevLight& L, int l, uint64_t key, double ptx, double pty, double ptz,
                                                double& lx, double& ly, double& lz, double& r2) {
    if (L.kind != kLightArea) return light_dir(L, ptx, pty, ptz, lx, ly, lz, r2);
    const double u = key_f64(key, 2u + 2u * static_cast<uint32_t>(l));
    const double w = key_f64(key, 3u + 2u * static_cast<uint32_t>(l));
    const double qx = (L.v[0] + L.v[3] * u) + L.v[6] * w;
    const double qy = (L.v[1] + L.v[4] * u) + L.v[7] * w;
    const double qz = (L.v[2] + L.v[5] * u) + L.v[8] * w;
    const double vx = qx - ptx, vy = qy - pty, vz = qz - ptz;
    r2 = vx * vx + vy * vy + vz * vz;
    const double n = sqrt(r2);
    lx = vx / n; ly = vy / n; lz = vz / n;
    return true;
}

// FresnelMaterial's Schlick factor from the UNflipped n.d (raytrace.rs:128-136),
// in the reference's operation order.
__device__ __forceinline__ double fresnel_factor(const DevMaterial& m, double nd) {
    double r0 = (m.ior - 1.0) / (m.ior + 1.0);
    r0 = r0 * r0;
    const double omcos = 1.0 - fabs(nd);
    const double omcos2 = omcos * omcos;
    const double f = r0 + (((1.0 - r0) * omcos2) * omcos2) * omcos;
    return f > 1.0 ? 1.0 : f;                                       // clamp_one, raytrace.rs:26-28
}

// The per-hit flags of PhongMaterial / FresnelMaterial::color.  `f` is the
// Fresnel factor (1.0 for Phong): every Fresnel expression multiplies the
// Phong one by f in a position where x * 1.0 == x exactly, so one code path
// reproduces both materials bit for bit.
struct Shading {
    bool diffuse, specular;
    double f;
};

// kFresnel = false: the scene has no FresnelMaterial (f is the constant 1.0).
template <bool kFresnel = true>
__device__ __forceinline__ Shading shading_flags(const DevMaterial& m, double sig, double nd) {
    Shading s;
    s.f = kFresnel && m.kind == kMatFresnel ? fresnel_factor(m, nd) : 1.0;
    s.diffuse = m.kd_sig * sig > kMinSignificance;                  // raytrace.rs:35 / 137
    s.specular = (m.ks_sig * s.f) * sig > kMinSignificance;         // raytrace.rs:36 / 138
    return s;
}

// The specular term's power (raytrace.rs:55): c = clamp_zero(n . normalize(l - d)), the half
// vector's cosine, and pow(c, exponent).  add_light's own lines, as a function of their own
// so that rt_shade_check (probes.hip) reports the c and p that add_light uses.
__device__ __forceinline__ double spec_power(const DevMaterial& m, double lx, double ly, double lz, double nx, double ny,
                                             double nz, double dx, double dy, double dz, double& c) {
    const double hx = lx - dx, hy = ly - dy, hz = lz - dz;
#if RT_DIVK
    const DivK hl = div_k(sqrt_win(hx * hx + hy * hy + hz * hz));
    c = clamp_zero(nx * div_by(hx, hl) + ny * div_by(hy, hl) + nz * div_by(hz, hl));
#else
    const double hl = sqrt(hx * hx + hy * hy + hz * hz);
    c = clamp_zero(nx * (hx / hl) + ny * (hy / hl) + nz * (hz / hl));
#endif
    return pow(c, m.exponent);
}

// The diffuse and specular terms of one unshadowed light (raytrace.rs:51-56,
// Fresnel: 151-156, where the specular term is ((ks * lc) * f) * pow).
__device__ __forceinline__ void add_light(Col& res, const DevMaterial& m, const DevLight& L, bool diffuse, bool specular,
                                          double f, double lx, double ly, double lz, double nx, double ny, double nz,
                                          double dx, double dy, double dz) {
    if (diffuse) {
        const double s = clamp_zero(lx * nx + ly * ny + lz * nz);
        res.r = res.r + ((m.kd[0] * L.color[0]) * s) * kFrac1Pi;
        res.g = res.g + ((m.kd[1] * L.color[1]) * s) * kFrac1Pi;
        res.b = res.b + ((m.kd[2] * L.color[2]) * s) * kFrac1Pi;
    }
    if (specular) {
        double c;
        const double p = spec_power(m, lx, ly, lz, nx, ny, nz, dx, dy, dz, c);
        res.r = res.r + ((m.ks[0] * L.color[0]) * f) * p;
        res.g = res.g + ((m.ks[1] * L.color[1]) * f) * p;
        res.b = res.b + ((m.ks[2] * L.color[2]) * f) * p;
    }
}

// Mirror direction and the offset origin of raytrace.rs:60-62.
__device__ __forceinline__ Ray reflect_ray(const Ray& r, double ptx, double pty, double ptz, double nx, double ny,
                                           double nz) {
    const double dn = r.dx * nx + r.dy * ny + r.dz * nz;
    const double k2 = 2.0 * dn;
    const double rdx = r.dx - nx * k2, rdy = r.dy - ny * k2, rdz = r.dz - nz * k2;
    return Ray{ptx + rdx * kEps, pty + rdy * kEps, ptz + rdz * kEps, rdx, rdy, rdz};
}

}  // namespace rtamd
