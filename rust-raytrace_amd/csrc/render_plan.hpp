// The schedule of a render as arithmetic on plain data: which algorithm and sphere
// sources, how the streams are shaped, how a tile is cut into chunks and regions,
// where the fused tail starts and how a lane's working set is laid out.  Pure
// functions of the scene's facts, the tuning array, the CU count and the validated
// options: no HIP, no rt_ctx, no I/O (the caller prints the verbose lines from
// what is returned), so every decision can be checked without a GPU
// (tests/native/plan_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "device_layout.hpp"
#include "raytrace_amd.h"
#include "tuning.hpp"

namespace rtamd {

// LDS per traversal workgroup for staged scene data (1024 threads, two resident per CU)
constexpr size_t kLdsBudget = 72 * 1024;
constexpr int kPlanMaxBStreams = 4;     // = launch_api.hpp kMaxBStreams (checked where both are seen)

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What the planner reads of an uploaded scene (filled from rt_ctx by the caller).
struct SceneFacts {
    int32_t n_spheres = 0, n_bvh = 0, n_bvh4 = 0, n_q4 = 0, n_lights = 0;
    bool has_half = false;            // binary16 nodes were built (DevScene::bvh_h)
    bool has_cgrid = false;           // the camera's view grid was built (DevScene::cgrid)
    bool needs_path = false;          // a class only the path kernel implements
    bool deep_bvh4 = false, short_stack = false, short_stack18 = false, q4_ok = false, all_lights_gridded = false;
};

// ---- algorithm ------------------------------------------------------------------------
// RT_ALGO_AUTO resolved to path / wavefront / brute LDS / brute global, or, with aa_wavefront
// (the tuning key) set, to RT_ALGO_WAVEFRONT_AA for a chain-class scene of <= 32 lights rendered
// with random jitter and spp > 1.  Returns RT_OK, or the status of a refusal with its text in *err.
int plan_algo(const SceneFacts& sf, int algo, int jitter, uint32_t spp, int* mode, const char** err, int aa_wavefront = 0);
// Whether a render of `mode` runs one chain pass per AA sample: RT_ALGO_WAVEFRONT_AA with random
// jitter and spp > 1 (with centre jitter or one sample it is RT_ALGO_WAVEFRONT's render).
inline bool plan_aa_passes(int mode, int jitter, uint32_t spp) {
    return mode == RT_ALGO_WAVEFRONT_AA && jitter != RT_JITTER_CENTER && spp > 1;
}

// ---- accumulating renders (rt_render_accumulate) ------------------------------------------
// The schedule of a call that adds samples [S, S + n) to an accumulator's running sums.
//   mode       RT_ALGO_PATH or RT_ALGO_WAVEFRONT_AA: the only algorithms that trace every sample.  RT_ALGO_AUTO is
//              the path kernel unless the scene is of chain classes with at most 32 lights and aa_wavefront (the
//              tuning key) is set; jitter and n do not enter: an accumulating render never averages identical samples
//   passes     RT_ALGO_WAVEFRONT_AA: one chain pass per sample, forced: also for n == 1 and centre jitter
//              (plan_aa_passes is not asked); pass i runs with aa_pass = S + i, the global sample index
//   G          RT_ALGO_PATH: lanes per pixel, from this call's n (plan_path_group), not from a total
//   sparse     never: no pixel is final in an accumulating render
//   resolve    never per chunk: the sums are resolved by rt_accum_resolve, whenever asked
struct AccumPlan {
    int mode = RT_ALGO_PATH;
    uint32_t passes = 0;              // chain passes per chunk (0: the path kernel)
    bool sparse = false, chunk_resolve = false;
};
// Flags an accumulating call accepts: RT_COUNT_WORK | RT_TIME_KERNELS.
constexpr uint32_t kAccumFlags = RT_COUNT_WORK | RT_TIME_KERNELS;
constexpr uint32_t kAccumMaxSamples = 1u << 31;
// Returns RT_OK, or the status of a refusal with its text in *err: flags outside kAccumFlags and a count that would
// pass 2^31 are RT_E_INVALID, algorithms 1-4 RT_E_UNSUPPORTED, an unknown algorithm RT_E_INVALID, and
// RT_ALGO_WAVEFRONT_AA's own refusals (a path-only class, more than 32 lights) as plan_algo gives them.
int plan_accumulate(const SceneFacts& sf, int algo, uint32_t flags, uint32_t first, uint32_t n, int aa_wavefront,
                    AccumPlan* plan, const char** err);
// The path kernel's lanes per pixel: enough work-items to fill the chip (T_full of them), at most one per sample of
// the `samples` this launch traces per pixel; a power of two <= 64.  override_g: tuning path_group (0: none).
uint32_t plan_path_group(uint64_t npix, uint32_t samples, uint32_t T_full, int64_t override_g);

// ---- moments accumulators (rt_accum_create_moments) ------------------------
// The accumulator's device buffer in doubles: 3 per tile pixel, the sums; with moments 3 more per pixel, the sums
// of squares, as a plane of their own after the sums (24 B / 48 B per pixel).  false: the bytes pass 2^64.
bool plan_accum_doubles(uint64_t pixels, bool moments, uint64_t* doubles);
// Which kind of accumulator a call takes.  rt_accum_upload replaces the sums alone, which would leave a moments
// accumulator's squares stale: refused there; rt_accum_upload_moments / download_moments and the noise calls need
// the squares: refused on a plain accumulator.  Every other call works on both kinds.
enum class AccumCall { upload, upload_moments, download_moments, noise };
int plan_accum_call(AccumCall call, bool has_moments, const char** err);
// rt_accum_noise / rt_accum_noise_host: a moments accumulator of at least 2 samples (the variance divides by
// N - 1), and a floor and a threshold that are finite and > 0.  RT_OK, or RT_E_INVALID with its text in *err.
int plan_noise(bool has_moments, uint32_t samples, double floor, double threshold, const char** err);

// ---- sphere sources ---------------------------------------------------------------------
// (nearest, occlusion) sphere sources of a wavefront render, see launch_api.hpp; pfx2 / pfxq: the
// nodes of the binary / quantised tree a prefix source stages in LDS (DevScene::pfx2 / pfxq, which
// the caller stores when sets_prefix: RT_ALGO_WAVEFRONT_BRUTE leaves them as they are).
struct SourcePair {
    int src = 0, src_occ = 0;
    bool sets_prefix = false;
    int32_t pfx2 = 0, pfxq = 0;
};
SourcePair plan_sources(const SceneFacts& sf, const int64_t* tune, int mode);

// ---- first-hit feature buffers (rt_render_aov) ----------------------------------------------
// The sphere source of aov_primary (wf_aov.hip), one camera ray per sample and pixel:
//   the camera's view grid where the scene has one (22 spheres in LDS, 23 through L2), as generation 0 takes it
//     (tuning cam 3 or -1; any other value: off);
//   else the source the wavefront's later generations take for this tree (plan_sources): the whole tree in LDS
//     (7, 9), an LDS prefix beyond it (5, 6, 8), the binary tree through L2 (2) where neither applies;
//   else (a scene without spheres' tree, or tuning src 0 / 1) brute force, the sphere list from LDS (1) when it
//     fits 64 KB, else through the caches (0).
// Tuning src forces a family as it does for the wavefront; its shadow partner (src_occ) is of no concern here and
// is filled in, so that src alone selects.  The quantised tree (25, 26, tuning qtree) has no AOV instantiation:
// such a request takes what the scene would get without it.  pfx2: DevScene::pfx2 for the prefix sources.
struct AovSource {
    int src = 0;
    int32_t pfx2 = 0;
};
AovSource plan_aov_source(const SceneFacts& sf, const int64_t* tune);
// Whether aov_primary has an instantiation for sphere source src (launch_aov's cases).
constexpr bool aov_source_known(int src) {
    return src == 0 || src == 1 || src == 2 || (src >= 5 && src <= 9) || src == 22 || src == 23;
}
// The call's argument checks that need no device: channels a non-empty mask of rt_aov, every selected pointer set.
// ptrs: depth, normal, albedo, coverage, object.  RT_OK or RT_E_INVALID with its text in *err.
constexpr uint32_t kAovAll = 31u;
int plan_aov_args(uint32_t channels, const void* const ptrs[5], const char** err);
// Workgroups of the launch: one 1024-thread workgroup per 1024 pixels, at most two per CU (all resident).
uint32_t plan_aov_workgroups(uint64_t npix, int n_cu);

// ---- ray queries (rt_query_nearest / rt_query_occluded) ---------------------------------------
// The sphere source of query_nearest (wf_query.hip), one caller-supplied ray per work-item: what plan_aov_source
// gives with the camera's view grid left out (the grid is built around the camera's position and says nothing about
// a foreign origin): tuning cam does not enter, tuning src forces 0, 1, 2, 5, 6, 7, 8, 9 as there, and the quantised
// tree (25, 26, tuning qtree) takes what the scene would get without it.  pfx2: DevScene::pfx2 for the prefix sources.
struct QuerySource {
    int src = 0;
    int32_t pfx2 = 0;
};
QuerySource plan_query_source(const SceneFacts& sf, const int64_t* tune);
// The sphere source of query_occluded: the shadow source plan_sources pairs for RT_ALGO_WAVEFRONT without any forcing
// (the 4-wide tree whole in LDS, 10, or through L2, 11; a tree the 4-wide stack could overflow: the binary tree, 7 in
// LDS or 2); a scene without a spheres' tree: brute force from LDS (1) when the list fits 64 KB, else through the
// caches (0).  The light grids (14, 15) belong to the scene's own lights and say nothing about a caller's ray: they
// are never chosen.  Tuning src_occ forces 0, 1 (0 when the list does not fit), 2, 7, 8, 10, 11 where the scene has
// that structure and it fits; 14 / 15 ask for the tree they fall back to (10 in LDS, 11 beyond); any other value, or
// one that is not available, takes the automatic choice.  Tuning src does not enter.
QuerySource plan_query_occ_source(const SceneFacts& sf, const int64_t* tune);
// The sphere sources query_nearest / query_occluded are instantiated for: one list each, from which both the
// launchers' cases (wf_query.hip) and the planner's check below are made, so that they cannot drift apart.
#define RT_QUERY_NEAREST_SRCS(X) X(0) X(1) X(2) X(5) X(6) X(7) X(8) X(9)
#define RT_QUERY_OCC_SRCS(X) X(0) X(1) X(2) X(7) X(8) X(10) X(11)
#define RT_QUERY_SRC_IS(s) || src == (s)
constexpr bool query_source_known(int src) { return false RT_QUERY_NEAREST_SRCS(RT_QUERY_SRC_IS); }
constexpr bool query_occ_source_known(int src) { return false RT_QUERY_OCC_SRCS(RT_QUERY_SRC_IS); }
// The call's argument checks that need no device.  What every call gets: flags RT_TIME_KERNELS alone.  nearest:
// channels a non-empty mask of rt_hit_channel.  With n > 0: rays set, and (device) 16-byte aligned; nearest: bufs (the
// caller's struct) set and every selected pointer of ptrs (t, object, normal) set; occlusion: occluded set.  With
// n == 0 no pointer is looked at.  RT_OK or RT_E_INVALID with its text in *err.
constexpr uint32_t kHitAll = 7u;
constexpr uint32_t kQueryFlags = RT_TIME_KERNELS;
struct QueryArgs {
    bool occlusion = false, device = false;
    const void* rays = nullptr;
    uint32_t n = 0, channels = 0, flags = 0;
    bool has_bufs = false;                       // nearest: the rt_hit_buffers struct is not NULL
    const void* ptrs[3] = {nullptr, nullptr, nullptr};
    const void* occluded = nullptr;
};
int plan_query_args(const QueryArgs& a, const char** err);
// Workgroups of the launch, by plan_aov_workgroups' rule: one 1024-thread workgroup per 1024 rays, at most two per
// CU (all resident); the workgroups stride over the rays beyond that.
uint32_t plan_query_workgroups(uint64_t n, int n_cu);

// ---- denoiser (rt_denoise / rt_denoise_device) ---------------------------------------------------
// The call's argument checks that need no device, in the order include/raytrace_amd.h lists them; p and in are the
// caller's structs (either may be null: refused).  RT_OK or RT_E_INVALID with its text in *err.
constexpr uint32_t kDnAllFlags = RT_DN_NORMAL | RT_DN_DEPTH | RT_DN_COLOR | RT_DN_DEMODULATE;
constexpr uint32_t kDnMaxIterations = 8, kDnMaxSquarings = 10;
int plan_denoise_args(const rt_denoise_params* p, const rt_denoise_inputs* in, const void* out_rgb, const void* out_bgr,
                      const char** err);
// rt_denoise_var / rt_denoise_var_device: the checks above in their order, with "all three outputs NULL" (out_rgb,
// out_bgr, var->out_variance) where they have "both outputs NULL", then those of the rt_denoise_variance struct
// (null: refused).  The passes are plan_denoise's: the variance rides in the colour record, the scratch is the same.
int plan_denoise_var_args(const rt_denoise_params* p, const rt_denoise_inputs* in, const rt_denoise_variance* var,
                          const void* out_rgb, const void* out_bgr, const char** err);
// The passes of a checked call.  Pass i has step 2^i.  A pass whose step is 1 or 2 has the LDS form (wf_denoise.hip
// stages the workgroup's kDnTileW x kDnTileH tile and a halo of 2 * step pixels, which fits its static LDS up to
// step kDnLdsMaxStep); every later pass reads its taps through L2.  variant 1: every pass direct; 2: LDS where it
// exists; 0: kDnAutoVariant, the one measured faster.  The last pass writes the caller's outputs.
// Scratch: two colour images and one guide image of 16 B per pixel, each 256-byte aligned.
constexpr uint32_t kDnTileW = 64, kDnTileH = 8, kDnLdsMaxStep = 2;
constexpr uint32_t kDnAutoVariant = 2;
constexpr uint64_t kDnRecordBytes = 16;
struct DenoisePlan {
    uint32_t passes = 0;
    uint32_t step[kDnMaxIterations] = {};
    bool lds[kDnMaxIterations] = {};
    uint32_t variant = 1;             // what ran for the steps <= kDnLdsMaxStep (the verbose line's V)
    uint32_t grid_x = 0, grid_y = 0;  // workgroups of a filter pass: one per tile
    uint64_t image_bytes = 0;         // one scratch image, aligned
    uint64_t scratch_bytes = 0;       // all three
};
DenoisePlan plan_denoise(const rt_denoise_params& p);

// ---- streams ----------------------------------------------------------------------------
struct StreamShape {
    bool split = false;     // shadow + shading kernels on b streams of their own
    int n_b = 1;            // that many
    int cam = 0;            // generation 0: 0 per ray, 3 / 4 the camera's view grid (spheres in LDS / through L2)
    int grid_occ = 0;       // shadow kernel without a tree walk: spheres from LDS (1) or HBM/L2 (2); 0: general
    uint32_t wg_major = 1;  // chunk dealing
    int mark_gen = 0;       // lanes: the next chunk starts after this generation
};
StreamShape plan_streams(const SceneFacts& sf, const int64_t* tune, int mode, int src, uint32_t max_depth);

// ---- chunks -----------------------------------------------------------------------------
// Working-set bytes per element (device_layout.hpp, WfBufs): written once, read by the budget
// (wf_bytes_per_slot) and by the carve-up (wf_layout).
constexpr uint64_t kWfQueueBytes = 2ull * 8 * 8;     // per queue entry: two queues of 8 8-byte fields
constexpr uint64_t kWfRecBytes = 7 * 8 + 4 * 4;      // per queue entry and level: a shade record
constexpr uint64_t kWfLevBytes = 4 * 8 + 4;          // per chain and level: local colour, Schlick factor, object
constexpr uint64_t kWfTermBytes = 3 * 8 + 1;         // per chain: terminal colour, levels pushed
constexpr uint64_t kWfCpixBytes = 4;                 // per queue entry: the chain's pixel
constexpr uint64_t kWfPmapBytes = 4;                 // per chunk pixel: the pixel map
constexpr uint64_t kWfCcolBytes = 16;                // per chain: the chain colours
constexpr uint64_t kWfAccBytes = 3 * 8;              // per chunk pixel, AA passes only: the f64 running sum

// Working-set bytes per pixel slot of a chunk (wf_layout's sections, per slot):
// two queues, one shade-record array and one level array per lit generation,
// terminals and level counts, the chain's pixel, the pixel map and the chain colours; aa (a render
// of one pass per AA sample): also the running sums.
constexpr uint64_t wf_bytes_per_slot(uint64_t levels, bool aa = false) {
    return kWfQueueBytes + levels * kWfRecBytes + levels * kWfLevBytes + kWfTermBytes + kWfCpixBytes + kWfPmapBytes +
           kWfCcolBytes + (aa ? kWfAccBytes : 0);
}

// The chunk cap in pixels: tuning chunk_pixels, else what `budget` bytes (all lanes) hold at `levels`.
uint64_t plan_cap_px(const int64_t* tune, uint64_t budget, uint64_t levels, bool aa = false);

struct ChunkPlan {
    uint32_t tile_w = 0, tile_h = 0;
    uint32_t tiles_x = 0;             // 8x8 tiles per row
    uint32_t chunk_rows = 0;          // rows of the largest chunk (a multiple of 8): what the working set is sized for
    uint32_t n_chunks = 0;
    uint32_t first_rows = 0;          // > 0: two chunks of first_rows and tile_h - first_rows rows (host_first)
    int n_lanes = 1;
    uint32_t row0(uint32_t ci) const { return first_rows ? (ci ? first_rows : 0u) : ci * chunk_rows; }
    uint32_t nrows(uint32_t ci) const {
        if (first_rows) return ci ? tile_h - first_rows : first_rows;
        const uint32_t left = tile_h - ci * chunk_rows;
        return chunk_rows < left ? chunk_rows : left;
    }
    uint32_t cap() const { return tile_w * chunk_rows; }      // pixel capacity of a lane's working set
    uint64_t next_cap_px() const {                            // out of memory: half the pixels per chunk
        const uint64_t h = static_cast<uint64_t>(chunk_rows) * tile_w / 2;
        return h > 1 ? h : 1;
    }
};
// One call per attempt of the render's out-of-memory retry (cap_px: plan_cap_px, then next_cap_px).
// bands: the render is rt_render's into host memory (host_chunks / host_first apply).
ChunkPlan plan_chunks(const int64_t* tune, uint64_t cap_px, uint32_t tile_w, uint32_t tile_h, bool bands);

// ---- regions ----------------------------------------------------------------------------
struct RegionPlan {
    uint32_t slots = 0;               // generation-0 slots of the largest chunk (8x8 tiles)
    uint32_t G = 1, R = 0;            // regions per queue, entries per region
};
RegionPlan plan_regions(const int64_t* tune, int n_cu, const ChunkPlan& cp);

// ---- fused tail -------------------------------------------------------------------------
// The generation the fused tail (wf_tail) starts at for chunks of `slots` generation-0 slots; 0: none.
int plan_tail_fuse(const SceneFacts& sf, const int64_t* tune, int src, uint64_t slots, uint32_t max_depth);

// ---- working-set layout -----------------------------------------------------------------
// A lane's wavefront working set for chunks of up to `cap` pixels: every queue and shade-record
// array is G regions of R entries; the shade records have one such array per lit generation
// (`levels` = max_depth + 1); aa: also the running sums of a render of one pass per AA sample
// (3 f64 per chunk pixel, the last section).  Sections 256-byte aligned; the queues start at 0.
struct WfLayout {
    uint64_t qcap = 0;                // queue capacity G * R (>= generation-0 slots)
    uint64_t capa = 0;                // qcap rounded up to 64: per-chain arrays (chain = generation-0 record entry)
    uint64_t s_queue = 0, s_rec = 0, s_lev = 0, s_term = 0, s_reg = 0, s_cpix = 0, s_pmap = 0, s_ccol = 0, s_acc = 0;
    uint64_t o_rec = 0, o_lev = 0, o_term = 0, o_rq = 0, o_rs = 0, o_cpix = 0, o_pmap = 0, o_ccol = 0, o_acc = 0;
    uint64_t total = 0;
};
WfLayout wf_layout(uint32_t cap, uint32_t G, uint32_t R, uint32_t levels, bool aa = false);

}  // namespace rtamd
