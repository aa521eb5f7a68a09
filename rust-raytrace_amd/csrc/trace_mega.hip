// Per-pixel ray tracing on CDNA4 (gfx950): the megakernel.
//
// Two schedules of the same exact math (trace_common.hpp):
//
//  * trace_frame_kernel ("megakernel", this file): one work-item per pixel runs the whole
//    recursive ray_color / PhongMaterial::color chain (raytrace.rs:30-67,
//    261-276) as a loop.  Simple, but a wave lives as long as its deepest
//    pixel and holds all shading state across every intersection loop.
//
//  * wavefront (wf_*, wf_device.hpp): one generation per recursion depth, one small kernel per
//    step of a generation.
#define RT_UNIT trace_mega      // reads the sRGB table: its own copy (trace_types.hpp)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_layout.hpp"
#include "launch_api.hpp"
#include "trace_common.hpp"
#include "wf_launch.hpp"

namespace rtamd {

namespace {

constexpr int kBlock = 256;                 // 4 waves

// kSky (a skybox scene's instantiations): a ray that misses, at any depth, takes the skybox's colour in
// its direction (raytrace.rs:234-256) instead of the solid background.
template <bool kSky, class SpherePtr>
__device__ Col trace_chain(const DevScene& sc, SpherePtr S, Ray ray, uint32_t max_depth, uint32_t& rays,
                           uint32_t& shadows) {
    double st_r[kMaxLevels], st_g[kMaxLevels], st_b[kMaxLevels], st_f[kMaxLevels];
    int32_t st_obj[kMaxLevels];
    int lvl = 0;
    double sig = 1.0;
    uint32_t depth = 0;
    Col term;
    for (;;) {
        const Hit h = nearest_brute(sc, S, ray);
        ++rays;
        if (h.obj == INT32_MAX) {                                  // raytrace.rs:228-256
            if constexpr (kSky) term = background(sc, ray);
            else term = Col{sc.bg[0], sc.bg[1], sc.bg[2]};
            break;
        }
        const DevMaterial& m = sc.mats[h.obj];
        Col res{m.amb[0], m.amb[1], m.amb[2]};
        if (depth > max_depth) { term = res; break; }             // raytrace.rs:33
        const double ptx = ray.ox + ray.dx * h.t, pty = ray.oy + ray.dy * h.t, ptz = ray.oz + ray.dz * h.t;
        double nx, ny, nz;
        hit_normal(sc, sc.spheres, h.prim, ptx, pty, ptz, nx, ny, nz);
        const double nd = nx * ray.dx + ny * ray.dy + nz * ray.dz;
        const Shading sh = shading_flags(m, sig, nd);
        const bool diffuse = sh.diffuse, specular = sh.specular;
        if (nd > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        if (diffuse || specular) {
            for (int li = 0; li < sc.n_lights; ++li) {
                const DevLight& L = sc.lights[li];
                double lx, ly, lz, r2;
                const bool has_range = light_dir(L, ptx, pty, ptz, lx, ly, lz, r2);
                const Ray sray{ptx + lx * kEps, pty + ly * kEps, ptz + lz * kEps, lx, ly, lz};
                ++rays;
                ++shadows;
                if (occluded_brute(sc, S, sray, has_range, r2)) continue;
                add_light(res, m, L, diffuse, specular, sh.f, lx, ly, lz, nx, ny, nz, ray.dx, ray.dy, ray.dz);
            }
        }
        if (!specular) { term = res; break; }
        st_r[lvl] = res.r; st_g[lvl] = res.g; st_b[lvl] = res.b; st_obj[lvl] = h.obj; st_f[lvl] = sh.f;
        ++lvl;
        ray = reflect_ray(ray, ptx, pty, ptz, nx, ny, nz);
        sig = (sh.f * sig) * m.ks_sig;                             // raytrace.rs:63 / 163
        ++depth;
    }
    Col acc = term;                                                // fold inner-first (raytrace.rs:63 / 163)
    for (int k = lvl - 1; k >= 0; --k) {
        const DevMaterial& m = sc.mats[st_obj[k]];
        acc.r = st_r[k] + (m.ks[0] * acc.r) * st_f[k];
        acc.g = st_g[k] + (m.ks[1] * acc.g) * st_f[k];
        acc.b = st_b[k] + (m.ks[2] * acc.b) * st_f[k];
    }
    return acc;
}

template <bool kLds, bool kSky = false>
__global__ __launch_bounds__(kBlock) void trace_frame_kernel(DevScene sc, FrameParams fp) {
    extern __shared__ __attribute__((aligned(16))) DevSphere lds_spheres[];
    if constexpr (kLds) {
        for (int i = threadIdx.x; i < sc.n_spheres; i += kBlock) lds_spheres[i] = sc.spheres[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // 16x16 pixel tile per workgroup, 8x8 per wave
    const uint32_t lx = blockIdx.x * 16u + (wave & 1) * 8u + (lane & 7);
    const uint32_t ly = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    uint32_t rays = 0, shadows = 0;
    if (lx < fp.tile_w && ly < fp.rows) {
        const Ray cam = camera_ray(sc, fp, lx, fp.row0 + ly, 0u);
        Col c;
        if constexpr (kLds) c = trace_chain<kSky>(sc, static_cast<const DevSphere*>(lds_spheres), cam, fp.max_depth, rays, shadows);
        else c = trace_chain<kSky>(sc, sc.spheres, cam, fp.max_depth, rays, shadows);
        write_pixel(fp, lx, fp.row0 + ly, average_samples(c, fp.spp));
        rays *= fp.spp;          // identical centre-jitter samples: traced once, counted as the reference issues them
        shadows *= fp.spp;
    }
    for (int off = 32; off > 0; off >>= 1) {
        rays += __shfl_xor(rays, off, 64);
        shadows += __shfl_xor(shadows, off, 64);
    }
    if (lane == 0) {
        const uint32_t shard = (blockIdx.y * gridDim.x + blockIdx.x) % kCounterShards;
        atomicAdd(&fp.counters[shard], static_cast<unsigned long long>(rays));
        atomicAdd(&fp.counters[kCounterShards + shard], static_cast<unsigned long long>(shadows));
    }
}

}  // namespace

// mode: 1 = spheres staged in LDS, 2 = read from global.
hipError_t launch_trace_frame(const DevScene& sc, const FrameParams& fp, int mode, hipStream_t stream) {
    const dim3 grid((fp.tile_w + 15) / 16, (fp.rows + 15) / 16);
    const bool lds = mode == 1;
    const size_t lds_bytes = lds ? static_cast<size_t>(sc.n_spheres) * sizeof(DevSphere) : 0;
    return dispatch_bools(
        [&](auto kLds, auto kSky) {
            hipLaunchKernelGGL((trace_frame_kernel<kLds(), kSky()>), grid, dim3(kBlock), lds_bytes, stream, sc, fp);
            return hipGetLastError();
        },
        lds, sc.skybox);
}

RT_UNIT_WARM(trace_mega)
RT_UNIT_SRGB(trace_mega)

}  // namespace rtamd
