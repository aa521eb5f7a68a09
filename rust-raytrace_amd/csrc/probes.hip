// Diagnostic kernels: pieces of the device arithmetic (trace_common.hpp) run side by side with
// the compiler's own, for rt_div_a2_check, rt_sqrt_check and rt_cull_check.
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
