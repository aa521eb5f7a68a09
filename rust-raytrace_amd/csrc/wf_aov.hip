// First-hit feature buffers (include/raytrace_amd.h, rt_render_aov): what Scene::intersect
// (scene.rs:247-249) answers for the camera rays of a tile -- depth, normal, albedo, coverage,
// object id -- averaged over the AA samples as main.rs:47-56 averages colours.  No shading, no
// queue, no working set: one launch of aov_primary over the tile, from the sphere source the
// planner names (render_plan.hpp, plan_aov_source), through the same camera_ray, stage_lds and
// nearest_any as the wavefront's camera pass.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wf_device.hpp"
#include "wf_launch.hpp"

namespace rtamd {
namespace {

// One pixel per work-item; consecutive lanes take consecutive pixels of a row (tile row-major
// index p), so every store instruction of a wave covers one contiguous range.  The samples of a
// pixel are traced in order and added in order to f64 sums kept in registers (up to 8: 16 VGPRs);
// kJitter false (RT_JITTER_CENTER): the samples are identical, so the ray is traced once and the
// sums are still formed with fp.spp additions, as average_samples does.  A channel whose buffer
// is null (a kernel argument: uniform branches) computes and stores nothing.
template <int kSrc, bool kJitter>
__global__ __launch_bounds__(kWfThreads, Src<kSrc>::waves) void aov_primary(DevScene sc, FrameParams fp, AovOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const BvhView v = stage_lds<kSrc, true>(sc, lds);
    __syncthreads();                                       // publishes the LDS staging
    const uint64_t npix = static_cast<uint64_t>(fp.tile_w) * fp.tile_h;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWfThreads;
    const bool want_n = out.normal != nullptr, want_a = out.albedo != nullptr;
    const uint32_t traced = kJitter ? fp.spp : 1u, repeat = kJitter ? 1u : fp.spp;
    const double aa = static_cast<double>(fp.spp);
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * kWfThreads + threadIdx.x; p < npix; p += stride) {
        const uint32_t lx = static_cast<uint32_t>(p % fp.tile_w), row = static_cast<uint32_t>(p / fp.tile_w);
        double s_t = 0.0, s_nx = 0.0, s_ny = 0.0, s_nz = 0.0, s_r = 0.0, s_g = 0.0, s_b = 0.0, s_c = 0.0;   // main.rs:47
        int32_t obj0 = -1;
        for (uint32_t a = 0; a < traced; ++a) {
            const Ray r = camera_ray(sc, fp, lx, row, a);
            const Hit h = nearest_any<kSrc, false>(sc, v, r, nullptr);
            double t = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0, cov = 0.0;
            if (h.obj != INT32_MAX) {
                t = h.t;
                cov = 1.0;
                if (want_n) {
                    const double ptx = r.ox + r.dx * h.t, pty = r.oy + r.dy * h.t, ptz = r.oz + r.dz * h.t;   // ray.cast(t)
                    hit_normal(sc, v.sph, h.prim, ptx, pty, ptz, nx, ny, nz);
                    if (nx * r.dx + ny * r.dy + nz * r.dz > 0.0) { nx = -nx; ny = -ny; nz = -nz; }           // raytrace.rs:38
                }
                if (want_a) {
                    const DevMaterial& m = sc.mats[h.obj];
                    cr = m.kd[0]; cg = m.kd[1]; cb = m.kd[2];
                }
                if (a == 0) obj0 = h.obj;
            }
            for (uint32_t k = 0; k < repeat; ++k) {                                                           // main.rs:48-55
                s_t = s_t + t; s_c = s_c + cov;
                if (want_n) { s_nx = s_nx + nx; s_ny = s_ny + ny; s_nz = s_nz + nz; }
                if (want_a) { s_r = s_r + cr; s_g = s_g + cg; s_b = s_b + cb; }
            }
        }
        if (out.depth) stn(&out.depth[p], static_cast<float>(s_t / aa));                                      // main.rs:56
        if (out.coverage) stn(&out.coverage[p], static_cast<float>(s_c / aa));
        if (want_n) {
            float* q = out.normal + 3 * p;
            stn(&q[0], static_cast<float>(s_nx / aa)); stn(&q[1], static_cast<float>(s_ny / aa)); stn(&q[2], static_cast<float>(s_nz / aa));
        }
        if (want_a) {
            float* q = out.albedo + 3 * p;
            stn(&q[0], static_cast<float>(s_r / aa)); stn(&q[1], static_cast<float>(s_g / aa)); stn(&q[2], static_cast<float>(s_b / aa));
        }
        if (out.object) stn(&out.object[p], obj0);
    }
    // the render's rays: every sample of every pixel is one Scene::intersect query; this workgroup's
    // pixels are the 1024-pixel blocks c with c % gridDim.x == blockIdx.x
    if (threadIdx.x == 0) {
        const uint64_t full = npix / kWfThreads, rem = npix % kWfThreads, G = gridDim.x, b = blockIdx.x;
        uint64_t mine = full > b ? (full - b + G - 1) / G * kWfThreads : 0;
        if (full % G == b) mine += rem;
        atomicAdd(&fp.counters[b % kCounterShards], static_cast<unsigned long long>(mine * fp.spp));
    }
}

template <int kSrc>
hipError_t launch_aov_src(const DevScene& sc, const FrameParams& fp, const AovOut& out, uint32_t workgroups, hipStream_t s) {
    const size_t lds = staged_bytes<kSrc>(sc);
    if (fp.jitter) hipLaunchKernelGGL((aov_primary<kSrc, true>), dim3(workgroups), dim3(kWfThreads), lds, s, sc, fp, out);
    else hipLaunchKernelGGL((aov_primary<kSrc, false>), dim3(workgroups), dim3(kWfThreads), lds, s, sc, fp, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_aov(const DevScene& sc, const FrameParams& fp, const AovOut& out, int src, uint32_t workgroups,
                      hipStream_t s) {
    switch (src) {
    case kSrcGlobal: return launch_aov_src<kSrcGlobal>(sc, fp, out, workgroups, s);
    case kSrcLds: return launch_aov_src<kSrcLds>(sc, fp, out, workgroups, s);
    case kSrcBvhG: return launch_aov_src<kSrcBvhG>(sc, fp, out, workgroups, s);
    case kSrcBvhPH: return launch_aov_src<kSrcBvhPH>(sc, fp, out, workgroups, s);
    case kSrcBvhPHC: return launch_aov_src<kSrcBvhPHC>(sc, fp, out, workgroups, s);
    case kSrcBvhL8: return launch_aov_src<kSrcBvhL8>(sc, fp, out, workgroups, s);
    case kSrcBvhP: return launch_aov_src<kSrcBvhP>(sc, fp, out, workgroups, s);
    case kSrcBvhL8C: return launch_aov_src<kSrcBvhL8C>(sc, fp, out, workgroups, s);
    case kSrcCamGridL: return launch_aov_src<kSrcCamGridL>(sc, fp, out, workgroups, s);
    case kSrcCamGridG: return launch_aov_src<kSrcCamGridG>(sc, fp, out, workgroups, s);
    default: return hipErrorInvalidValue;
    }
}

RT_UNIT_WARM(wf_aov)

}  // namespace rtamd
