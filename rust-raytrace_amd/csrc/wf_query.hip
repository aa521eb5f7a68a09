// Ray queries (include/raytrace_amd.h, rt_query_nearest / rt_query_occluded): Scene::intersect (scene.rs:247-249)
// and the shadow test of raytrace.rs:43-50 for rays the caller supplies, [n, 6] f64 in device memory (origin,
// direction; the direction as given).  No shading, no queue, no working set: one launch over the rays from the
// sphere source the planner names (render_plan.hpp, plan_query_source / plan_query_occ_source), through the same
// stage_lds, nearest_any / occluded_any and hit_normal as the wavefront's kernels and aov_primary.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "render_plan.hpp"
#include "wf_device.hpp"
#include "wf_launch.hpp"

namespace rtamd {
namespace {

// Ray i: 48 bytes from a 16-byte aligned base (the host checks it), as three 16-byte loads; each ray is read once.
__device__ __forceinline__ Ray load_query_ray(const double* rays, uint64_t i) {
    const F64x2* p = reinterpret_cast<const F64x2*>(rays + 6 * i);
    const F64x2 a = ldn(p), b = ldn(p + 1), c = ldn(p + 2);
    return Ray{a[0], a[1], b[0], b[1], c[0], c[1]};
}

// The launch's rays, counted by the workgroup that owns them: workgroup b traces the 1024-ray blocks c with
// c % gridDim.x == b (rt_stats.rays; kShadow: rt_stats.shadow_rays too, a shadow query is both).
template <bool kShadow>
__device__ __forceinline__ void tally_rays(unsigned long long* counters, uint64_t n) {
    if (threadIdx.x != 0) return;
    const uint64_t full = n / kWfThreads, rem = n % kWfThreads, G = gridDim.x, b = blockIdx.x;
    uint64_t mine = full > b ? (full - b + G - 1) / G * kWfThreads : 0;
    if (full % G == b) mine += rem;
    atomicAdd(&counters[b % kCounterShards], static_cast<unsigned long long>(mine));
    if constexpr (kShadow) atomicAdd(&counters[kCounterShards + b % kCounterShards], static_cast<unsigned long long>(mine));
}

// One ray per work-item, consecutive lanes on consecutive rays, so every load and store instruction of a wave
// covers one contiguous range.  A channel whose buffer is null (a kernel argument: uniform branches) computes and
// stores nothing.  A miss: t +inf, object -1, normal 0; the normal is the shape's, not oriented against the ray.
template <int kSrc>
__global__ __launch_bounds__(kWfThreads, Src<kSrc>::waves) void query_nearest(DevScene sc, unsigned long long* counters,
                                                                              const double* rays, uint32_t n, QueryOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const BvhView v = stage_lds<kSrc, true>(sc, lds);
    __syncthreads();                                       // publishes the LDS staging
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWfThreads;
    const bool want_n = out.normal != nullptr;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWfThreads + threadIdx.x; i < n; i += stride) {
        const Ray r = load_query_ray(rays, i);
        const Hit h = nearest_any<kSrc, false>(sc, v, r, nullptr);
        const bool hit = h.obj != INT32_MAX;
        if (out.t) stn(&out.t[i], hit ? h.t : __builtin_huge_val());
        if (out.object) stn(&out.object[i], hit ? h.obj : -1);
        if (want_n) {
            double nx = 0.0, ny = 0.0, nz = 0.0;
            if (hit) {
                const double ptx = r.ox + r.dx * h.t, pty = r.oy + r.dy * h.t, ptz = r.oz + r.dz * h.t;   // ray.cast(t)
                hit_normal(sc, v.sph, h.prim, ptx, pty, ptz, nx, ny, nz);
            }
            double* q = out.normal + 3 * i;
            stn(&q[0], nx); stn(&q[1], ny); stn(&q[2], nz);
        }
    }
    tally_rays<false>(counters, n);
}

// raytrace.rs:43-50 per ray: r2 null is the directional light's rule (any hit occludes), else the point light's
// with the caller's squared range r2[i].  No hint: the caller's rays start on no sphere the library knows of.
// The shadow walks read the whole-LDS binary tree in its plain node encoding (stage_lds<kSrc, false>, as
// wf_occlusion stages it), not the nearest-hit walk's byte offsets.
template <int kSrc>
__global__ __launch_bounds__(kWfThreads, Src<kSrc>::waves) void query_occluded(DevScene sc, unsigned long long* counters,
                                                                               const double* rays, const double* r2, uint32_t n,
                                                                               uint8_t* occluded) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const BvhView v = stage_lds<kSrc, false>(sc, lds);
    __syncthreads();                                       // publishes the LDS staging
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWfThreads;
    const bool has_range = r2 != nullptr;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWfThreads + threadIdx.x; i < n; i += stride) {
        const Ray r = load_query_ray(rays, i);
        const double range = has_range ? ldn(&r2[i]) : 0.0;
        const bool occ = occluded_any<kSrc, false>(sc, v, r, has_range, range, -1, nullptr);
        stn(&occluded[i], occ ? 1 : 0);
    }
    tally_rays<true>(counters, n);
}

template <int kSrc>
hipError_t launch_nearest_q(const DevScene& sc, unsigned long long* counters, const double* rays, uint32_t n,
                            const QueryOut& out, uint32_t workgroups, hipStream_t s) {
    hipLaunchKernelGGL((query_nearest<kSrc>), dim3(workgroups), dim3(kWfThreads), staged_bytes<kSrc>(sc), s, sc, counters, rays,
                       n, out);
    return hipGetLastError();
}

template <int kSrc>
hipError_t launch_occluded_q(const DevScene& sc, unsigned long long* counters, const double* rays, const double* r2,
                             uint32_t n, uint8_t* occluded, uint32_t workgroups, hipStream_t s) {
    hipLaunchKernelGGL((query_occluded<kSrc>), dim3(workgroups), dim3(kWfThreads), staged_bytes<kSrc>(sc), s, sc, counters,
                       rays, r2, n, occluded);
    return hipGetLastError();
}

}  // namespace

// The cases are render_plan.hpp's lists of instantiated sources (which the planner's query_source_known reads too).
hipError_t launch_query_nearest(const DevScene& sc, unsigned long long* counters, const double* rays, uint32_t n,
                                const QueryOut& out, int src, uint32_t workgroups, hipStream_t s) {
    switch (src) {
#define RT_X(k) case k: return launch_nearest_q<k>(sc, counters, rays, n, out, workgroups, s);
    RT_QUERY_NEAREST_SRCS(RT_X)
#undef RT_X
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_query_occluded(const DevScene& sc, unsigned long long* counters, const double* rays, const double* r2,
                                 uint32_t n, uint8_t* occluded, int src, uint32_t workgroups, hipStream_t s) {
    switch (src) {
#define RT_X(k) case k: return launch_occluded_q<k>(sc, counters, rays, r2, n, occluded, workgroups, s);
    RT_QUERY_OCC_SRCS(RT_X)
#undef RT_X
    default: return hipErrorInvalidValue;
    }
}

RT_UNIT_WARM(wf_query)

}  // namespace rtamd
