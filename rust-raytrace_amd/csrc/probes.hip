// Diagnostic kernels: pieces of the device arithmetic (trace_common.hpp) run side by side with
// the compiler's own, for rt_div_a2_check, rt_sqrt_check and rt_cull_check, or record by record
// for a host model to restate (rt_isect_check, rt_shade_check).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_layout.hpp"
#include "launch_api.hpp"
#include "trace_common.hpp"
#include "wf_launch.hpp"

namespace rtamd {

// Diagnostic (rt_div_a2_check): the sphere test's division t = x / (2a) as
// sphere_t computes it (sphere_k's hoisted reciprocal finished by div_a2) and
// as the compiler's own f64 division, side by side.
__global__ __launch_bounds__(256) void div_a2_probe(const double* x, const double* a, uint32_t n, double* fast,
                                                    double* slow) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const SphK k = sphere_k(a[i]);
        fast[i] = div_a2(x[i], k);
        slow[i] = x[i] / (2.0 * a[i]);
    }
}

// Diagnostic (rt_sqrt_check): the sphere test's square root as sphere_roots computes it
// (sqrt_win) and as the compiler's own f64 sqrt, side by side.
__global__ __launch_bounds__(256) void sqrt_probe(const double* x, uint32_t n, double* fast, double* slow) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        fast[i] = sqrt_win(x[i]);
        slow[i] = sqrt(x[i]);
    }
}

// Diagnostic (rt_cull_check): the conservative f32 culling arithmetic of the tree walks, one
// record per work-item, through the functions the walks call: make_raybox (with the far-origin
// rule at `reach`), t_limit, box_hit, the whole-LDS walk's box_hit_nf on the near / far bounds
// it would read (near_is_lo), and the compact stack entries of 16 and 18 code bits.
__global__ __launch_bounds__(256) void cull_probe(uint32_t n, const double* rays, const float* boxes, const double* t,
                                                  const int32_t* codes, float reach, int32_t* out_i, float* out_f) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double* q = rays + 6ull * i;
        Ray r;
        r.ox = q[0]; r.oy = q[1]; r.oz = q[2]; r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
        const float* B = boxes + 6ull * i;
        const float lo[3] = {B[0], B[1], B[2]}, hi[3] = {B[3], B[4], B[5]};
        const RayBox rb = make_raybox(r, reach);
        const float tl = t_limit(rb, t[i]);
        float tn, tn_nf;
        const bool hit = box_hit(lo, hi, rb, tl, tn);
        const bool lx = near_is_lo(rb.ix), ly = near_is_lo(rb.iy), lz = near_is_lo(rb.iz);
        const bool hit_nf = box_hit_nf(lx ? lo[0] : hi[0], ly ? lo[1] : hi[1], lz ? lo[2] : hi[2], lx ? hi[0] : lo[0],
                                       ly ? hi[1] : lo[1], lz ? hi[2] : lo[2], rb, tl, tn_nf);
        const uint32_t e16 = stk_entry_c<16>(codes[i], tn), e18 = stk_entry_c<18>(codes[i], tn);
        int32_t* oi = out_i + 5ull * i;
        float* of = out_f + 5ull * i;
        oi[0] = rb.te; oi[1] = hit ? 1 : 0; oi[2] = hit_nf ? 1 : 0; oi[3] = stk_node_c<16>(e16); oi[4] = stk_node_c<18>(e18);
        of[0] = tl; of[1] = tn; of[2] = tn_nf; of[3] = stk_t_c<16>(e16); of[4] = stk_t_c<18>(e18);
    }
}

// Diagnostic (rt_isect_check): the exact f64 sphere and plane tests, one record per work-item,
// through the functions the render kernels call: sphere_k, sphere_t in both forms (branch-free
// and branchy), plane_t, and for a sphere hit the hit point as the kernels form it (o + d t) and
// hit_normal.  in: 16 doubles per record (ray origin, direction, sphere centre, rr, plane point,
// normal); out_i: 3 per record (hit of sphere_t<true>, of sphere_t<false>, of plane_t); out_d: 15
// per record (the three t, then point and normal of the branch-free hit, then of the branchy
// one).  A miss reports t = 0 and a zero point and normal; plane_t's t is reported as computed.
__global__ __launch_bounds__(256) void isect_probe(uint32_t n, const double* in, int32_t* out_i, double* out_d) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double* q = in + 16ull * i;
        const Ray r{q[0], q[1], q[2], q[3], q[4], q[5]};
        const DevSphere s{q[6], q[7], q[8], q[9]};
        const DevPlane p{q[10], q[11], q[12], q[13], q[14], q[15]};
        const DevScene sc{};                   // hit_normal reads it for a plane only
        const SphK sk = sphere_k(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz);
        int32_t* oi = out_i + 3ull * i;
        double* od = out_d + 15ull * i;
        double t[2] = {0.0, 0.0};
        const bool h[2] = {sphere_t<true>(s, r, sk, t[0]), sphere_t<false>(s, r, sk, t[1])};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double pt[3] = {0.0, 0.0, 0.0}, nr[3] = {0.0, 0.0, 0.0};
            if (h[k]) {
                pt[0] = r.ox + r.dx * t[k]; pt[1] = r.oy + r.dy * t[k]; pt[2] = r.oz + r.dz * t[k];   // ray.cast(t)
                hit_normal(sc, &s, 0, pt[0], pt[1], pt[2], nr[0], nr[1], nr[2]);
            }
            oi[k] = h[k] ? 1 : 0;
            od[k] = h[k] ? t[k] : 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) { od[3 + 6 * k + a] = pt[a]; od[6 + 6 * k + a] = nr[a]; }
        }
        double tp;
        oi[2] = plane_t(p, r, tp) ? 1 : 0;
        od[2] = tp;
    }
}

// Diagnostic (rt_shade_check): the shading arithmetic of one hit, one material and one light, one
// record per work-item, through the functions the render kernels call: light_dir, fresnel_factor,
// shading_flags, reflect_ray, spec_power and add_light (with both flags on, into a zeroed colour),
// on the normal oriented against the ray as the kernels orient it (n.d > 0: -n; the factor and
// the flags take the unflipped n.d); then pow, sin and cos on three operand columns of their own,
// the plain calls the path kernel makes.  in_d: 29 doubles per record (point 3, normal 3, ray
// direction 3, kd 3, ks 3, kd_sig, ks_sig, exponent, ior, light v 3, light colour 3, significance,
// pow x, pow y, trig x); in_i: 2 per record (material kind, light kind); out_d: 20 per record
// (light direction 3, r2, fresnel_factor, f, reflected ray 6, c, p, colour 3, pow, sin, cos);
// out_i: 3 per record (has_range, diffuse, specular).
__global__ __launch_bounds__(256) void shade_probe(uint32_t n, const double* in_d, const int32_t* in_i, int32_t* out_i,
                                                   double* out_d) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double* q = in_d + 29ull * i;
        const double rnx = q[3], rny = q[4], rnz = q[5];
        const Ray r{0.0, 0.0, 0.0, q[6], q[7], q[8]};
        DevMaterial m{};
        DevLight L{};
#pragma unroll
        for (int a = 0; a < 3; ++a) { m.kd[a] = q[9 + a]; m.ks[a] = q[12 + a]; L.v[a] = q[19 + a]; L.color[a] = q[22 + a]; }
        m.kd_sig = q[15]; m.ks_sig = q[16]; m.exponent = q[17]; m.ior = q[18];
        m.kind = in_i[2ull * i];
        L.kind = in_i[2ull * i + 1];
        const double sig = q[25];
        const double nd = rnx * r.dx + rny * r.dy + rnz * r.dz;         // as the kernels orient the normal
        const bool flip = nd > 0.0;
        const double nx = flip ? -rnx : rnx, ny = flip ? -rny : rny, nz = flip ? -rnz : rnz;
        double lx, ly, lz, r2;
        const bool has_range = light_dir(L, q[0], q[1], q[2], lx, ly, lz, r2);
        const Shading sh = shading_flags<true>(m, sig, nd);
        const Ray rr = reflect_ray(r, q[0], q[1], q[2], nx, ny, nz);
        double c;
        const double p = spec_power(m, lx, ly, lz, nx, ny, nz, r.dx, r.dy, r.dz, c);
        Col res{0.0, 0.0, 0.0};
        add_light(res, m, L, true, true, sh.f, lx, ly, lz, nx, ny, nz, r.dx, r.dy, r.dz);
        double* od = out_d + 20ull * i;
        od[0] = lx; od[1] = ly; od[2] = lz; od[3] = r2;
        od[4] = fresnel_factor(m, nd); od[5] = sh.f;
        od[6] = rr.ox; od[7] = rr.oy; od[8] = rr.oz; od[9] = rr.dx; od[10] = rr.dy; od[11] = rr.dz;
        od[12] = c; od[13] = p;
        od[14] = res.r; od[15] = res.g; od[16] = res.b;
        od[17] = pow(q[26], q[27]); od[18] = sin(q[28]); od[19] = cos(q[28]);
        int32_t* oi = out_i + 3ull * i;
        oi[0] = has_range ? 1 : 0; oi[1] = sh.diffuse ? 1 : 0; oi[2] = sh.specular ? 1 : 0;
    }
}

hipError_t launch_isect_probe(uint32_t n, const double* in, int32_t* out_i, double* out_d, hipStream_t s) {
    const uint32_t blocks = std::max(1u, std::min(4096u, (n + 255u) / 256u));
    hipLaunchKernelGGL(isect_probe, dim3(blocks), dim3(256), 0, s, n, in, out_i, out_d);
    return hipGetLastError();
}

hipError_t launch_shade_probe(uint32_t n, const double* in_d, const int32_t* in_i, int32_t* out_i, double* out_d,
                              hipStream_t s) {
    const uint32_t blocks = std::max(1u, std::min(4096u, (n + 255u) / 256u));
    hipLaunchKernelGGL(shade_probe, dim3(blocks), dim3(256), 0, s, n, in_d, in_i, out_i, out_d);
    return hipGetLastError();
}

hipError_t launch_cull_probe(uint32_t n, const double* rays, const float* boxes, const double* t, const int32_t* codes,
                             float reach, int32_t* out_i, float* out_f, hipStream_t s) {
    const uint32_t blocks = std::max(1u, std::min(4096u, (n + 255u) / 256u));
    hipLaunchKernelGGL(cull_probe, dim3(blocks), dim3(256), 0, s, n, rays, boxes, t, codes, reach, out_i, out_f);
    return hipGetLastError();
}

hipError_t launch_sqrt_probe(const double* x, uint32_t n, double* fast, double* slow, hipStream_t s) {
    const uint32_t blocks = std::max(1u, std::min(4096u, (n + 255u) / 256u));
    hipLaunchKernelGGL(sqrt_probe, dim3(blocks), dim3(256), 0, s, x, n, fast, slow);
    return hipGetLastError();
}

hipError_t launch_div_a2_probe(const double* x, const double* a, uint32_t n, double* fast, double* slow, hipStream_t s) {
    const uint32_t blocks = std::max(1u, std::min(4096u, (n + 255u) / 256u));
    hipLaunchKernelGGL(div_a2_probe, dim3(blocks), dim3(256), 0, s, x, a, n, fast, slow);
    return hipGetLastError();
}

RT_UNIT_WARM(probes)

}  // namespace rtamd
