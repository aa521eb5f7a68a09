// Host-side launchers of the kernels in the .hip translation units (called by rt_render.cpp and
// rt_device.cpp): trace_mega.hip, the wavefront schedule's wf_sequence.hip and, behind it, its
// kernel families (wf_launch.hpp), wf_output.hip, wf_aov.hip, wf_query.hip, probes.hip and path_kernel.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_layout.hpp"

namespace rtamd {

// Kernel families of the wavefront schedule (rt_ctx_kernel_times indices).
enum KernelFamily : int8_t {
    kKfNearest = 0, kKfOcclusion = 1, kKfShade = 2, kKfFold = 3, kKfTally = 4, kKfCamera = 5, kKfCompose = 6, kKfTail = 7, kKfCount = 8
};

// Per-launch timing (RT_TIME_KERNELS): begin() records a start event before a
// launch (after any cross-stream wait), mark() an end event after it, noting
// (start, end, family): the elapsed time between the two is that launch's
// duration (one LaunchMarks per stream).  Events
// come from a pool owned by the context; intervals accumulate over renders
// until harvested (rt_ctx_kernel_times).
struct LaunchInterval {
    int start, end;
    KernelFamily fam;
};

struct LaunchMarks {
    std::vector<hipEvent_t>* pool = nullptr;
    int* used = nullptr;                   // events of the pool in use
    std::vector<LaunchInterval>* out = nullptr;
    int prev = -1;
    static constexpr int kMaxEvents = 1 << 16;

    hipError_t record(hipStream_t s, int& idx) {
        idx = -1;
        if (*used >= kMaxEvents) return hipSuccess;    // not harvested: stop recording
        if (*used == static_cast<int>(pool->size())) {
            hipEvent_t e;
            const hipError_t err = hipEventCreate(&e);
            if (err != hipSuccess) return err;
            pool->push_back(e);
        }
        idx = (*used)++;
        return hipEventRecord((*pool)[idx], s);
    }
    hipError_t begin(hipStream_t s) { return record(s, prev); }
    hipError_t mark(hipStream_t s, KernelFamily f) {
        int idx;
        const hipError_t e = record(s, idx);
        if (e == hipSuccess && idx >= 0 && prev >= 0) out->push_back(LaunchInterval{prev, idx, f});
        prev = idx;
        return e;
    }
};

hipError_t launch_trace_frame(const DevScene& sc, const FrameParams& fp, int mode, hipStream_t stream);
// The streams of one wavefront lane: a runs the nearest-hit chain and the
// fold; the shadow + shading kernels of generation k run on b[k % nb] (b[i] ==
// a: one in-order stream).  near_done: kMaxGenerations events; b_done: one
// per b stream; marks may be null.  Sphere sources and the supported
// (nearest, shadow) pairs: wf_device.hpp kSrc* and wf_sequence.hip launch_wavefront.
constexpr int kMaxBStreams = 4;
struct WfStreams {
    hipStream_t a;
    hipStream_t b[kMaxBStreams];
    int nb;
    hipEvent_t* near_done;
    hipEvent_t b_done[kMaxBStreams];
    LaunchMarks* ma;
    LaunchMarks* mb[kMaxBStreams];
    int cam;            // generation 0: 0 per-ray traversal of the nearest-hit source, 3 / 4 the camera's view
                        // grid with the spheres in LDS / through L2
    int grid_occ;       // every light has a light-view grid: shadow kernel without a tree walk,
                        // spheres from LDS (1) or HBM/L2 (2); 0: the general shadow kernel
    hipEvent_t* fold_ev;// recorded once the chunk's pixels are final (null: no event)
    int tail_fuse;        // > 0: the chains running at generation tail_fuse - 1 finish in one wf_tail
    int tail_wgs;         //   launch on stream a (that many workgroups, all resident: one per CU;
    int tail_width;       //   chains per wave, 0 auto), which folds them; the others fold on b[0]
    // sparse host copies (b.mark set): after generation 0 (sp_cam), stream sp_s runs the segment
    // kernels into sp_bits / sp_cnt / sp_off (then sp_ready); after the fold stream a packs the
    // flagged segments into sp_bgr / sp_rgb (null: that output is off).  sp_s null: off.
    // lazy_tally: no wf_tally launch; the caller runs launch_tally later, when statistics are
    // asked for (the queue sizes it reads stay in the working set until the next render)
    bool lazy_tally = false;
    // dj_flags (device, kDjWords words): the b streams join stream a on the device (launch_signal /
    // launch_join) instead of through events; dj_next: the last join number handed out (the lane's,
    // advanced per join).  Null: events.
    uint64_t* dj_flags = nullptr;
    uint64_t* dj_next = nullptr;
    uint64_t* dj_err = nullptr;         // device address of the lane's page-locked error word
    hipStream_t sp_s = nullptr;
    hipEvent_t sp_cam = nullptr, sp_ready = nullptr;
    uint32_t *sp_bits = nullptr, *sp_cnt = nullptr, *sp_off = nullptr;
    uint8_t* sp_bgr = nullptr;
    float* sp_rgb = nullptr;
};
hipError_t launch_wavefront(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int src, int src_occ,
                            bool count, const WfStreams& ws, hipEvent_t mark, int mark_gen);
hipError_t upload_srgb_table(const double* avg255);
// wf_tally of one chunk (rays, shadow rays and per-generation queue sizes into b.totals /
// b.gen_totals) on stream s: what launch_wavefront runs at the end unless ws.lazy_tally.
hipError_t launch_tally(const FrameParams& fp, const WfBufs& b, int n_lights, int generations, hipStream_t s);
// Device-side stream join: flag words 0 .. kDjFlags-1 (one per b stream).  launch_signal stores
// n into *flag after the stream's earlier work; launch_join waits until flag i >= n for every
// bit i of mask, or sets *err (a page-locked host word) after 2 s and goes on.
constexpr int kDjFlags = 4, kDjWords = 8;
hipError_t launch_signal(uint64_t* flag, uint64_t n, hipStream_t s);
hipError_t launch_join(uint64_t* flags, uint32_t mask, uint64_t n, uint64_t* err, hipStream_t s);
// Sparse host copies (tuning sparse_out): pixels per row segment; after the camera pass
// (b.mark set) segbits / rowcnt / rowoff of the chunk's rows (wf_chain_segs + wf_row_scan);
// after the fold the flagged segments packed in row order (wf_chain_pack).
constexpr uint32_t kSegPx = 16;
hipError_t launch_chain_segs(const FrameParams& fp, const WfBufs& b, uint32_t* segbits, uint32_t* rowcnt, uint32_t* rowoff,
                             hipStream_t s);
hipError_t launch_chain_pack(const FrameParams& fp, const uint32_t* segbits, const uint32_t* rowoff, uint8_t* pk_bgr,
                             float* pk_rgb, hipStream_t s);
// rt_ctx_reserve: a no-op launch of `workgroups` 1024-thread workgroups with private memory
// on stream s (sets up the stream's queue and scratch), then an empty launch from every other
// kernel translation unit but path_kernel.hip, so that each code object is loaded;
// launch_path_warmup loads path_kernel.hip's.
hipError_t launch_warmup(uint32_t workgroups, hipStream_t s);
hipError_t launch_path_warmup(hipStream_t s);
// Diagnostic: div_a2(x, sphere_k(a)) and x / (2a) on the device (rt_div_a2_check).
hipError_t launch_div_a2_probe(const double* x, const double* a, uint32_t n, double* fast, double* slow, hipStream_t s);
// Diagnostic: sqrt_win(x) and sqrt(x) on the device (rt_sqrt_check).
hipError_t launch_sqrt_probe(const double* x, uint32_t n, double* fast, double* slow, hipStream_t s);
// Diagnostic: the tree walks' f32 culling arithmetic on n (ray, box, t, code) records (rt_cull_check).
hipError_t launch_cull_probe(uint32_t n, const double* rays, const float* boxes, const double* t, const int32_t* codes,
                             float reach, int32_t* out_i, float* out_f, hipStream_t s);
// Diagnostic: sphere_t in both forms, plane_t, the hit point and hit_normal on n records of 16 doubles
// (rt_isect_check; probes.hip has the layouts).
hipError_t launch_isect_probe(uint32_t n, const double* in, int32_t* out_i, double* out_d, hipStream_t s);
// Diagnostic: light_dir, fresnel_factor, shading_flags, reflect_ray, spec_power, add_light and the device's
// pow / sin / cos on n records of 29 doubles and 2 ints (rt_shade_check).
hipError_t launch_shade_probe(uint32_t n, const double* in_d, const int32_t* in_i, int32_t* out_i, double* out_d,
                              hipStream_t s);

// First-hit feature buffers (wf_aov.hip, rt_render_aov): device buffers of the tile, tile row-major; null: the
// channel is not selected and costs nothing.  normal and albedo: 3 floats per pixel.
struct AovOut {
    float* depth;
    float* normal;
    float* albedo;
    float* coverage;
    int32_t* object;
};
// aov_primary from sphere source src (render_plan.hpp, plan_aov_source; an unknown one: hipErrorInvalidValue) over the
// whole tile of fp (fp.spp samples per pixel, fp.jitter, fp.seed), `workgroups` workgroups of kWfThreads; each
// workgroup adds its pixels * fp.spp to a shard of fp.counters (the rays of the render).
hipError_t launch_aov(const DevScene& sc, const FrameParams& fp, const AovOut& out, int src, uint32_t workgroups,
                      hipStream_t s);

// Ray queries (wf_query.hip, rt_query_nearest / rt_query_occluded): n caller-supplied rays, 6 doubles each (origin,
// direction) from a 16-byte aligned device address.  Outputs per ray; null: the channel is not selected and costs
// nothing.  normal: 3 doubles per ray.
struct QueryOut {
    double* t;
    int32_t* object;
    double* normal;
};
// query_nearest / query_occluded from sphere source src (render_plan.hpp, plan_query_source / plan_query_occ_source;
// an unknown one: hipErrorInvalidValue), `workgroups` workgroups of kWfThreads striding over the rays; each workgroup
// adds its rays to a shard of counters (FrameParams::counters: rays, and for occlusion shadow rays too).  r2 null: no
// range (the directional light's rule).  n > 0.
hipError_t launch_query_nearest(const DevScene& sc, unsigned long long* counters, const double* rays, uint32_t n,
                                const QueryOut& out, int src, uint32_t workgroups, hipStream_t s);
hipError_t launch_query_occluded(const DevScene& sc, unsigned long long* counters, const double* rays, const double* r2,
                                 uint32_t n, uint8_t* occluded, int src, uint32_t workgroups, hipStream_t s);

// The denoiser (wf_denoise.hip, rt_denoise_device; the rule: include/raytrace_amd.h).  Device images of w x h
// pixels.  DnRec: one 16-byte record per pixel, a colour (r, g, b, and the variance-guided forms' variance, else 0)
// or a guide (normal x, y, z, depth).
struct alignas(16) DnRec {
    float x, y, z, w;
};
struct DnFilter {
    uint32_t w, h;
    uint32_t flags, squarings;      // rt_denoise_flags, rt_denoise_params::normal_squarings
    double sigma_color, sigma_depth;
};
// The variance-guided forms (rt_denoise_var_device): the colour record's fourth float carries the pixel's scalar
// variance from pass to pass; out_variance (w x h floats, may be null) is what the last pass leaves of it.
struct DnVar {
    double sigma_variance, variance_floor;
    float* out_variance;
};
// The pack pass: the caller's tight f32 images (normal / depth null where their flag is off: zeros; albedo read under
// RT_DN_DEMODULATE only) into one colour and one guide record per pixel.  variance (w x h x 3 floats) non-null: the
// variance-guided form, which also packs the scalar variance.
hipError_t launch_denoise_pack(const DnFilter& f, const float* rgb, const float* normal, const float* depth,
                               const float* albedo, DnRec* colour, DnRec* guide, hipStream_t s, const float* variance = nullptr);
// One filter pass of step `step` from `src` into `dst`; lds: the tile-staging form (step <= kDnLdsMaxStep only,
// else hipErrorInvalidValue).  grid: the plan's (one workgroup per kDnTileW x kDnTileH tile).  var non-null: the
// variance-guided form.
hipError_t launch_denoise_pass(const DnFilter& f, uint32_t step, bool lds, const DnRec* src, const DnRec* guide, DnRec* dst,
                               uint32_t grid_x, uint32_t grid_y, hipStream_t s, const DnVar* var = nullptr);
// The last pass: as above, then remodulated by `albedo` (RT_DN_DEMODULATE) and written as f32 (out_rgb, tight; may be
// null) and sRGB B G R bytes (out_bgr, rows of bgr_pitch bytes, padding left alone; may be null).
hipError_t launch_denoise_last(const DnFilter& f, uint32_t step, bool lds, const DnRec* src, const DnRec* guide,
                               const float* albedo, float* out_rgb, uint8_t* out_bgr, uint32_t bgr_pitch, uint32_t grid_x,
                               uint32_t grid_y, hipStream_t s, const DnVar* var = nullptr);

// The general path (path_kernel.hip): every material / light / camera class,
// keyed random draws, one work-item per pixel over the HBM recursion stack.
// staged: binary BVH + spheres in LDS (path_lds_bytes(sc, true) must fit).
size_t path_lds_bytes(const DevScene& sc, bool staged);
int path_waves_per_simd();          // the path kernel's occupancy (its launch bounds)
// accumulate (rt_render_accumulate): the instantiations that add samples [fp.aa_pass, fp.aa_pass + fp.aa_spp) of
// every pixel to the running sums in fp.aa_acc (tile row-major) and write no pixel.
hipError_t launch_path(const DevScene& sc, const FrameParams& fp, const PathStack& st, bool staged, hipStream_t stream,
                       bool accumulate = false);
// rt_accum_resolve: the tile's pixels from its running sums (fp.aa_acc, 3 f64 per tile pixel, tile row-major) of
// fp.aa_spp samples each: sum / samples, rounded once to f32 and quantised from the f64 value, written row by row
// (fp.out_rgb / out_bgr, bgr_pitch, pad_end; rows [0, fp.rows)).  workgroups: the grid's upper bound.
hipError_t launch_accum_resolve(const FrameParams& fp, uint32_t workgroups, hipStream_t s);
// rt_accum_noise: the estimate of a moments accumulator (fp.aa_acc: the tile's sums, then the
// plane of its sums of squares; fp.aa_spp >= 2 samples; rows [0, fp.rows) = the whole tile): variance (3 f32 per
// pixel) and error (1 f32 per pixel), either may be null, and the pixels whose error is not <= threshold added to
// *above, which the caller zeroed on s before.
hipError_t launch_accum_noise(const FrameParams& fp, uint32_t workgroups, double err_floor, double threshold, float* variance,
                              float* error, unsigned long long* above, hipStream_t s);

}  // namespace rtamd
