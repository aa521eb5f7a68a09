// Schedule knobs of a context (rt_ctx_set_tuning).  The defaults are the
// measured-best settings; nothing is read from the environment,
// so a render's schedule depends only on the scene, the options and these.
// HIP-free: the render planner (render_plan.hpp) and its CPU test read it too.
#pragma once

#include <cstdint>

namespace rtamd {

// One list: X(enum suffix, name, default, lowest, highest) generates both TuneKey and kTune[],
// so a key set by name is always read through its own enum index.
// -1 in src / src_occ / cam / split: chosen per scene.  Round 5 removed the knobs of
// variants measured slower and off by default (DESIGN.md §9 keeps their rows): fuse,
// lists, lists0, fuse_from, prefix4_kb, cam_prefix_kb, tail_from, tail_max, eager_fold,
// fold_split, bmerge, wave_max, tail_fold, tail_shade, fold_wgs, shade_wgs.
#define RT_TUNE_KEYS(X)                                                                                              \
    /* wavefront chunk cap (0: what the working-set budget holds at the depth) */                                    \
    X(ChunkPixels, "chunk_pixels", 0, 0, INT32_MAX)                                                                  \
    /* 0: 2 (4 for a quantised tree beyond the LDS budget) */                                                        \
    X(BvhLeaf, "bvh_leaf", 0, 0, 8)                                                                                  \
    /* light-view grids for point-light shadow queries */                                                            \
    X(Lgrid, "light_grids", 1, 0, 1)                                                                                 \
    /* 0: from the median sphere's angular size */                                                                   \
    X(LgridRes, "light_grid_res", 0, 0, 4096)                                                                        \
    /* nearest-hit sphere source (wf_device.hpp kSrc*) */                                                            \
    X(Src, "src", -1, -1, 26)                                                                                        \
    /* shadow sphere source */                                                                                       \
    X(SrcOcc, "src_occ", -1, -1, 26)                                                                                 \
    /* LDS prefixes stay <= 150 KB: with the queue counters (<= 8.4 KB at 2048 regions) a                            \
       workgroup's LDS then fits gfx950's 160 KB */                                                                  \
    /* LDS prefix of the binary (or quantised) tree (KB) for trees beyond LDS */                                     \
    X(PrefixKb2, "prefix_kb", 64, 1, 150)                                                                            \
    /* chunk lanes (each its own streams and working set) */                                                         \
    X(Lanes, "lanes", 1, 1, 8)                                                                                       \
    /* lanes: chunk c+1 starts after this generation of chunk c */                                                   \
    X(StaggerGen, "stagger_gen", 1, 0, 64)                                                                           \
    /* regions per queue (0: 2 x CUs) */                                                                             \
    X(Regions, "regions", 0, 0, 2048)                                                                                \
    /* 0: every wavefront kernel on one in-order stream (-1: per tree) */                                            \
    X(Split, "split", -1, -1, 1)                                                                                     \
    /* streams for the shadow + shading kernels */                                                                   \
    X(BStreams, "bstreams", 2, 1, 4)                                                                                 \
    /* generation 0: 3 the camera's view grid (-1: where built), else per ray */                                     \
    X(Cam, "cam", -1, -1, 3)                                                                                         \
    /* chunk dealing: 1 workgroup-major, 0 workgroup-first */                                                        \
    X(Deal, "deal", 1, 0, 1)                                                                                         \
    /* queues below this size are dealt workgroup-first */                                                           \
    X(SpreadBelow, "spread_below", 0, 0, INT32_MAX)                                                                  \
    /* path kernel: lanes per pixel (0: auto) */                                                                     \
    X(PathGroup, "path_group", 0, 0, 64)                                                                             \
    /* b streams CU-masked (own hardware queue): 1 every CU, 2/3/4 only 3/4, 1/2, 1/4 of them */                     \
    X(CuMask, "cu_mask", 1, 0, 4)                                                                                    \
    /* nearest-hit chain on a high-priority stream (round 4: C3 2.969-2.974                                          \
       vs 2.983-2.998 ms, 8-way share 0.713 vs 0.741 ms, C4 equal; same box) */                                      \
    X(Prio, "prio", 1, 0, 1)                                                                                         \
    /* print the chosen schedule (and a working set that does not fit) to stderr */                                  \
    X(Verbose, "verbose", 0, 0, 1)                                                                                   \
    /* shadow kernel without a tree walk when every light has a grid */                                              \
    X(GridOcc, "grid_occ", 1, 0, 1)                                                                                  \
    /* 32-bit nearest-hit stack entries, 32 of them (src 9; src 6 for half-node trees) */                            \
    X(Compact, "compact_stack", 1, 0, 1)                                                                             \
    /* trees beyond LDS: binary16 node bounds for the prefix source (src 5) */                                       \
    X(Half, "half_nodes", 1, 0, 1)                                                                                   \
    /* wavefront working set of all lanes together (MB; 0: min(80 GB,                                                \
       85% of the device's free memory)); chunks are sized to it */                                                  \
    X(WfBudgetMb, "wf_budget_mb", 0, 0, INT32_MAX)                                                                   \
    /* the camera's view grid: cells per face side (0: from the scene's                                              \
       frame size, -1: no grid); takes effect at the next rt_scene_upload */                                         \
    X(CamGridRes, "cam_grid_res", 0, -1, 4096)                                                                       \
    /* 1: the nearest-hit chain's stream CU-masked (a hardware queue of its                                          \
       own, so another context's frame is never queued behind it) */                                                 \
    X(AQueue, "a_queue", 0, 0, 1)                                                                                    \
    /* > 0: the chains running at generation tail_fuse - 1 of a src-9 frame whose                                    \
       lights all have light-view grids finish in one launch (wf_tail); 0 off, -1 auto */                            \
    X(TailFuse, "tail_fuse", -1, -1, 32)                                                                             \
    /* ... with this many chains per wave (0: auto) */                                                               \
    X(TailWidth, "tail_width", 0, 0, 64)                                                                             \
    /* 1: trees beyond the f32 tree's LDS budget take the quantised 4-wide                                           \
       tree (src 25 whole in LDS, 26 LDS prefix + L2) for the nearest hit;                                           \
       measured slower than binary16 (C4 55.0 vs 50.4 ms, C5 330 vs 307 ms) */                                       \
    X(QTree, "qtree", 0, 0, 1)                                                                                       \
    /* 1: the frame is written row by row by wf_compose from the fold's                                              \
       chain-ordered colours (coalesced stores); 0: per pixel by the                                                 \
       camera pass and the fold (C3 3.104-3.123 vs 3.235-3.243 ms with                                               \
       1: the pass itself takes 113 us, the scattered stores it                                                      \
       replaces cost the camera pass and the fold less than that) */                                                 \
    X(Compose, "compose", 0, 0, 1)                                                                                   \
    /* rt_render into host memory: at least this many chunks, so the D2H                                             \
       copy of one chunk's rows overlaps the next chunk's generations */                                             \
    X(HostChunks, "host_chunks", 1, 1, 64)                                                                           \
    /* with host_chunks 2: the first chunk's share of the rows in percent                                            \
       (0: equal chunks) */                                                                                          \
    X(HostFirst, "host_first", 0, 0, 90)                                                                             \
    /* rt_render into host memory, one chunk: copy the frame after the camera                                        \
       pass, then only the 16-pixel segments holding chain pixels (§3.11;                                            \
       C3 BGR 4.00 -> 3.46-3.63 ms, RGB + BGR 8.09-8.17 -> 7.67-7.72 ms) */                                          \
    X(SparseOut, "sparse_out", 1, 0, 1)                                                                              \
    /* 1: a one-lane render's nearest-hit chain runs on the caller's stream                                          \
       itself (no fork / join hop between hardware queues at the start and                                           \
       end of the render; the chain then runs at the caller stream's priority;                                       \
       round 6, same box: 8-way C3 share 0.632-0.633 vs 0.650-0.657 ms, 4-way                                        \
       0.899 vs 0.926 ms, C3 2.767-2.779 vs 2.788-2.790 ms, C4 equal) */                                             \
    X(ChainOnCaller, "chain_on_caller", 1, 0, 1)                                                                     \
    /* rt_render's device -> host copies of the frame: 0 hipMemcpyAsync on the                                       \
       copy stream, e (1..16) the device's SDMA engine e - 1 driven directly                                         \
       (hsa_amd_memory_async_copy_on_engine), -1 its first four engines in turn,                                     \
       -2 (default) -1 for a row-banded tile (a rank's share: band_stride > 1),                                      \
       0 otherwise (round 6, same box: C3 8-way share into a page-locked frame                                       \
       BGR 1.02 vs 1.35 ms, RGB + BGR 1.43 vs 1.74 ms with -1; C4 share BGR 7.36                                     \
       vs 8.28 ms; the whole C3 frame BGR 3.65 vs 3.80 ms with 0) */                                   \
    X(CopyEngine, "copy_engine", -2, -2, 16)                                                                         \
    /* 1: the b streams join the chain's stream on the device (a one-wave                                            \
       kernel polling a flag the b stream's last kernel is followed by),                                             \
       0: through events (a barrier packet on the chain's queue) */                                                  \
    X(DevJoin, "dev_join", 1, 0, 1)                                                                                  \
    /* 1: RT_ALGO_AUTO renders a chain-class scene (<= 32 lights) with random                                        \
       jitter and spp > 1 as RT_ALGO_WAVEFRONT_AA (one chain pass per AA                                             \
       sample) instead of on the path kernel */                                                \
    X(AaWavefront, "aa_wavefront", 0, 0, 1)

enum TuneKey : int {
#define RT_TUNE_ENUM(id, name, dflt, lo, hi) kTune##id,
    RT_TUNE_KEYS(RT_TUNE_ENUM)
#undef RT_TUNE_ENUM
    kTuneCount
};
struct TuneDef {
    const char* name;
    int64_t dflt, lo, hi;
};
constexpr TuneDef kTune[kTuneCount] = {
#define RT_TUNE_DEF(id, name, dflt, lo, hi) {name, dflt, lo, hi},
    RT_TUNE_KEYS(RT_TUNE_DEF)
#undef RT_TUNE_DEF
};

}  // namespace rtamd
