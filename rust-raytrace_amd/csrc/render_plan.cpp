// The render planner (render_plan.hpp): every schedule decision the project has measured
// (DESIGN.md §6 and §9), as arithmetic on plain integers.
#include "render_plan.hpp"

#include <algorithm>
#include <cmath>

namespace rtamd {

int plan_algo(const SceneFacts& sf, int algo, int jitter, uint32_t spp, int* mode, const char** err, int aa_wavefront) {
    const size_t lds_bytes = static_cast<size_t>(sf.n_spheres) * sizeof(DevSphere);
    const bool fits_lds = lds_bytes <= 64 * 1024;
    int m = algo;
    // one chain pass per AA sample (RT_ALGO_WAVEFRONT_AA): asked for, or AUTO's choice under tuning
    // aa_wavefront for what only the path kernel renders otherwise (random jitter, spp > 1)
    if (m == RT_ALGO_AUTO && aa_wavefront != 0 && !sf.needs_path && sf.n_lights <= 32 && jitter != RT_JITTER_CENTER && spp > 1)
        m = RT_ALGO_WAVEFRONT_AA;
    if (m == RT_ALGO_WAVEFRONT_AA) {
        *mode = m;
        if (sf.needs_path) {
            *err = "RT_ALGO_WAVEFRONT_AA renders chain scenes only: IndirectPhong / Transparent materials, AreaLight and "
                   "DepthOfFieldCamera need RT_ALGO_PATH";
            return RT_E_UNSUPPORTED;
        }
        if (sf.n_lights > 32) {
            *err = "RT_ALGO_WAVEFRONT_AA handles at most 32 lights (the wavefront path's limit); use RT_ALGO_PATH";
            return RT_E_UNSUPPORTED;
        }
        return RT_OK;
    }
    // the stochastic / branching classes, and random jitter with several AA
    // samples per pixel, run on the path kernel only (the chain schedules trace
    // one camera ray per pixel: centre jitter, or random jitter with spp = 1)
    const bool path_only = sf.needs_path || (jitter != RT_JITTER_CENTER && spp > 1);
    if (m == RT_ALGO_AUTO)
        m = path_only ? RT_ALGO_PATH
                      : (sf.n_lights <= 32 ? RT_ALGO_WAVEFRONT : (fits_lds ? RT_ALGO_BRUTE_LDS : RT_ALGO_BRUTE_GLOBAL));
    *mode = m;
    if (path_only && m != RT_ALGO_PATH) {
        *err = "IndirectPhong / Transparent materials, AreaLight, DepthOfFieldCamera and random jitter with "
               "spp > 1 need RT_ALGO_PATH";
        return RT_E_UNSUPPORTED;
    }
    if (m == RT_ALGO_BRUTE_LDS && lds_bytes > 160 * 1024) {
        *err = "sphere list does not fit in LDS; use RT_ALGO_BRUTE_GLOBAL";
        return RT_E_INVALID;
    }
    if ((m == RT_ALGO_WAVEFRONT || m == RT_ALGO_WAVEFRONT_BRUTE) && sf.n_lights > 32) {
        *err = "the wavefront path handles at most 32 lights";
        return RT_E_UNSUPPORTED;
    }
    return RT_OK;
}

int plan_accumulate(const SceneFacts& sf, int algo, uint32_t flags, uint32_t first, uint32_t n, int aa_wavefront,
                    AccumPlan* plan, const char** err) {
    *plan = AccumPlan{};
    if (flags & ~kAccumFlags) {
        *err = "rt_render_accumulate takes RT_COUNT_WORK and RT_TIME_KERNELS only";
        return RT_E_INVALID;
    }
    if (first > kAccumMaxSamples || n > kAccumMaxSamples - first) {
        *err = "the accumulator's sample count would pass 2^31";
        return RT_E_INVALID;
    }
    if (algo >= RT_ALGO_BRUTE_LDS && algo <= RT_ALGO_WAVEFRONT_BRUTE) {
        *err = "an accumulating render traces every sample: RT_ALGO_PATH, RT_ALGO_WAVEFRONT_AA or RT_ALGO_AUTO";
        return RT_E_UNSUPPORTED;
    }
    if (algo != RT_ALGO_AUTO && algo != RT_ALGO_PATH && algo != RT_ALGO_WAVEFRONT_AA) {
        *err = "bad algo";
        return RT_E_INVALID;
    }
    int m = algo;
    if (m == RT_ALGO_AUTO) m = aa_wavefront != 0 && !sf.needs_path && sf.n_lights <= 32 ? RT_ALGO_WAVEFRONT_AA : RT_ALGO_PATH;
    if (m == RT_ALGO_WAVEFRONT_AA) {
        // the mode's own refusals (jitter and spp do not enter them)
        int mode = m;
        if (const int rc = plan_algo(sf, m, RT_JITTER_RANDOM, 2, &mode, err, 0); rc != RT_OK) return rc;
        plan->passes = n;
    }
    plan->mode = m;
    return RT_OK;
}

uint32_t plan_path_group(uint64_t npix, uint32_t samples, uint32_t T_full, int64_t override_g) {
    uint32_t G = 1;
    while (G < 64 && 2 * G <= samples && npix * G < T_full) G *= 2;
    if (override_g) G = static_cast<uint32_t>(override_g);   // A/B override
    if (G == 0 || (G & (G - 1)) || G > 64) G = 1;
    return G;
}

bool plan_accum_doubles(uint64_t pixels, bool moments, uint64_t* doubles) {
    const uint64_t per = moments ? 6 : 3;
    if (pixels > UINT64_MAX / (8 * per)) return false;
    *doubles = per * pixels;
    return true;
}

int plan_accum_call(AccumCall call, bool has_moments, const char** err) {
    if (call == AccumCall::upload) {
        if (!has_moments) return RT_OK;
        *err = "rt_accum_upload on a moments accumulator would leave its squares stale: rt_accum_upload_moments";
        return RT_E_INVALID;
    }
    if (has_moments) return RT_OK;
    *err = call == AccumCall::noise ? "the accumulator keeps no second moments (rt_accum_create_moments)"
                                    : "a plain accumulator has no squares to move (rt_accum_create_moments)";
    return RT_E_INVALID;
}

int plan_noise(bool has_moments, uint32_t samples, double floor, double threshold, const char** err) {
    if (const int rc = plan_accum_call(AccumCall::noise, has_moments, err); rc != RT_OK) return rc;
    if (samples < 2) {
        *err = "a variance needs at least 2 samples";
        return RT_E_INVALID;
    }
    if (!std::isfinite(floor) || !(floor > 0.0)) {
        *err = "the noise floor must be finite and > 0";
        return RT_E_INVALID;
    }
    if (!std::isfinite(threshold) || !(threshold > 0.0)) {
        *err = "the noise threshold must be finite and > 0";
        return RT_E_INVALID;
    }
    return RT_OK;
}

SourcePair plan_sources(const SceneFacts& sf, const int64_t* tune, int mode) {
    SourcePair p;
    if (mode != RT_ALGO_WAVEFRONT) {
        const bool fits_lds = static_cast<size_t>(sf.n_spheres) * sizeof(DevSphere) <= 64 * 1024;
        p.src = p.src_occ = fits_lds ? 1 : 0;
        return p;
    }
    // LDS per traversal workgroup (1024 threads, two resident per CU): the
    // whole BVH + sphere list when they fit, else the top of the tree.
    const size_t node_bytes = static_cast<size_t>(sf.n_bvh) * sizeof(DevBvhNode);
    const size_t sph_bytes = static_cast<size_t>(sf.n_spheres) * (sizeof(DevSphere) + sizeof(int32_t));
    const size_t node4_bytes = static_cast<size_t>(sf.n_bvh4) * kBvh4Planes * sizeof(DevBvh4Plane);
    // (nearest, occlusion) sphere sources, see launch_api.hpp.  Default: the
    // binary tree for the nearest-hit query and the 4-wide tree for the
    // shadow query, each staged whole in LDS with the spheres when it fits
    // (measured best at C3); tuning "src" / "src_occ" override.
    int src, src_occ;
    const bool fit2 = node_bytes + sph_bytes <= kLdsBudget;
    const bool fit4 = node4_bytes + sph_bytes <= kLdsBudget;
    const bool q4_fits = static_cast<size_t>(sf.n_q4) * sizeof(DevQNode4) <= kLdsBudget;
    const bool compact = tune[kTuneCompact] != 0;
    // is (nearest, shadow) source pair (a, o) available for this scene (launch_wavefront's pairs)?
    auto pair_ok = [&](int a, int o) {
        if (sf.deep_bvh4) return (a == 7 && o == 7 && fit2) || (a == 2 && o == 2);   // the 4-wide stack could overflow
        switch (a * 100 + o) {
        case 202: case 211: return true;
        case 707: case 710: return fit2 && (o == 7 || fit4);
        case 910: return fit2 && fit4 && sf.short_stack;
        case 511: return sf.has_half;
        case 611: return sf.has_half && sf.short_stack18;
        case 811: return true;
        case 2511: return sf.q4_ok && q4_fits;
        case 2611: return sf.q4_ok;
        default: return false;
        }
    };
    // Default: both trees whole in LDS with the spheres (measured best at C3), the binary
    // tree for the nearest hit (compact stack entries where the tree allows) and the 4-wide
    // tree for shadow rays without a light grid; trees beyond LDS: the binary tree's
    // breadth-first top in LDS (binary16 bounds where representable, twice the nodes)
    // and the 4-wide shadow tree through L2; the quantised tree with tuning "qtree".
    if (fit2 && fit4) {
        src = sf.short_stack && compact ? 9 : 7;
        src_occ = 10;
    } else {
        src = !sf.has_half || tune[kTuneHalf] == 0 ? 8 : sf.short_stack18 && compact ? 6 : 5;
        src_occ = 11;
        if (sf.q4_ok && tune[kTuneQTree] != 0) src = q4_fits ? 25 : 26;
    }
    if (sf.deep_bvh4) src_occ = src = fit2 ? 7 : 2;
    if (tune[kTuneSrc] >= 0) {                   // forced (A/B measurement, tests)
        src = static_cast<int>(tune[kTuneSrc]);
        src_occ = tune[kTuneSrcOcc] >= 0 ? static_cast<int>(tune[kTuneSrcOcc]) : src;
    }
    if (!pair_ok(src, src_occ)) {               // unsupported or unavailable here: the binary tree through L2
        src = 2;
        src_occ = sf.deep_bvh4 ? 2 : 11;
    }
    p.src = src;
    p.src_occ = src_occ;
    // LDS prefix (tuning "prefix_kb"): measured at C4, 64 KB of binary nodes for the nearest-hit kernels
    const int kb2 = static_cast<int>(tune[kTunePrefixKb2]);
    p.sets_prefix = true;
    p.pfx2 = static_cast<int32_t>(static_cast<size_t>(std::max(kb2, 1)) * 1024 / sizeof(DevBvhNode));
    p.pfxq = static_cast<int32_t>(static_cast<size_t>(std::max(kb2, 1)) * 1024 / sizeof(DevQNode4));
    return p;
}

AovSource plan_aov_source(const SceneFacts& sf, const int64_t* tune) {
    AovSource a;
    int64_t t[kTuneCount];
    for (int i = 0; i < kTuneCount; ++i) t[i] = tune[i];
    t[kTuneQTree] = 0;
    int64_t forced = t[kTuneSrc];
    if (forced == 25 || forced == 26) forced = t[kTuneSrc] = -1;
    // src alone selects: the shadow source plan_sources pairs it with
    if (forced >= 0) t[kTuneSrcOcc] = forced == 9 ? 10 : forced == 5 || forced == 6 || forced == 8 ? 11 : forced;
    const SourcePair sp = plan_sources(sf, t, RT_ALGO_WAVEFRONT);
    a.pfx2 = sp.pfx2;
    const size_t list_bytes = static_cast<size_t>(sf.n_spheres) * (sizeof(DevSphere) + sizeof(int32_t));
    const int brute = static_cast<size_t>(sf.n_spheres) * sizeof(DevSphere) <= 64 * 1024 ? 1 : 0;
    if ((t[kTuneCam] == 3 || t[kTuneCam] < 0) && sf.has_cgrid) a.src = list_bytes <= kLdsBudget ? 22 : 23;
    else if (forced == 0 || forced == 1 || sf.n_bvh == 0) a.src = forced == 0 ? 0 : brute;
    else a.src = sp.src;
    return a;
}

int plan_aov_args(uint32_t channels, const void* const ptrs[5], const char** err) {
    if (channels == 0) {
        *err = "rt_render_aov: no channel selected";
        return RT_E_INVALID;
    }
    if (channels & ~kAovAll) {
        *err = "rt_render_aov: unknown channel bits";
        return RT_E_INVALID;
    }
    for (int i = 0; i < 5; ++i)
        if (((channels >> i) & 1u) && !ptrs[i]) {
            *err = "rt_render_aov: a selected channel's buffer is NULL";
            return RT_E_INVALID;
        }
    return RT_OK;
}

uint32_t plan_aov_workgroups(uint64_t npix, int n_cu) {
    const uint64_t need = (npix + kWfThreads - 1) / kWfThreads;
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(need, 2ull * static_cast<uint64_t>(std::max(n_cu, 1)))));
}

QuerySource plan_query_source(const SceneFacts& sf, const int64_t* tune) {
    SceneFacts f = sf;
    f.has_cgrid = false;                          // the camera's grid is no structure for a foreign origin
    const AovSource a = plan_aov_source(f, tune);
    return QuerySource{a.src, a.pfx2};
}

QuerySource plan_query_occ_source(const SceneFacts& sf, const int64_t* tune) {
    QuerySource q;
    int64_t t[kTuneCount];
    for (int i = 0; i < kTuneCount; ++i) t[i] = tune[i];
    t[kTuneQTree] = 0;
    t[kTuneSrc] = t[kTuneSrcOcc] = -1;
    const SourcePair sp = plan_sources(sf, t, RT_ALGO_WAVEFRONT);
    q.pfx2 = sp.pfx2;
    const size_t sph_bytes = static_cast<size_t>(sf.n_spheres) * (sizeof(DevSphere) + sizeof(int32_t));
    const bool fit2 = static_cast<size_t>(sf.n_bvh) * sizeof(DevBvhNode) + sph_bytes <= kLdsBudget;
    const bool fit4 = static_cast<size_t>(sf.n_bvh4) * kBvh4Planes * sizeof(DevBvh4Plane) + sph_bytes <= kLdsBudget;
    const int brute = static_cast<size_t>(sf.n_spheres) * sizeof(DevSphere) <= 64 * 1024 ? 1 : 0;
    const bool tree = sf.n_bvh > 0;
    const bool wide = tree && !sf.deep_bvh4;     // the 4-wide stack could overflow otherwise
    q.src = tree ? sp.src_occ : brute;
    int64_t forced = tune[kTuneSrcOcc];
    if (forced == 14 || forced == 15) forced = fit4 ? 10 : 11;
    switch (forced) {
    case 0: q.src = 0; break;
    case 1: q.src = brute; break;
    case 2: case 8: if (tree) q.src = static_cast<int>(forced); break;
    case 7: if (tree && fit2) q.src = 7; break;
    case 10: if (wide && fit4) q.src = 10; break;
    case 11: if (wide) q.src = 11; break;
    default: break;
    }
    return q;
}

int plan_query_args(const QueryArgs& a, const char** err) {
    if (a.flags & ~kQueryFlags) {
        *err = "ray query: flags take RT_TIME_KERNELS only";
        return RT_E_INVALID;
    }
    if (!a.occlusion) {
        if (a.channels == 0) {
            *err = "rt_query_nearest: no channel selected";
            return RT_E_INVALID;
        }
        if (a.channels & ~kHitAll) {
            *err = "rt_query_nearest: unknown channel bits";
            return RT_E_INVALID;
        }
    }
    if (a.n == 0) return RT_OK;
    if (!a.rays) {
        *err = "ray query: rays is NULL";
        return RT_E_INVALID;
    }
    if (a.device && (reinterpret_cast<uintptr_t>(a.rays) & 15u)) {
        *err = "ray query: the device rays are not 16-byte aligned (a ray is read as three 16-byte loads)";
        return RT_E_INVALID;
    }
    if (a.occlusion) {
        if (!a.occluded) {
            *err = "rt_query_occluded: occluded is NULL";
            return RT_E_INVALID;
        }
        return RT_OK;
    }
    if (!a.has_bufs) {
        *err = "rt_query_nearest: the buffer struct is NULL";
        return RT_E_INVALID;
    }
    for (int i = 0; i < 3; ++i)
        if (((a.channels >> i) & 1u) && !a.ptrs[i]) {
            *err = "rt_query_nearest: a selected channel's buffer is NULL";
            return RT_E_INVALID;
        }
    return RT_OK;
}

uint32_t plan_query_workgroups(uint64_t n, int n_cu) { return plan_aov_workgroups(n, n_cu); }

namespace {

bool dn_sigma_ok(double v) { return std::isfinite(v) && v > 0.0; }

// The checks rt_denoise and rt_denoise_var share, each text under the name of the entry point that was called.
// out_var: rt_denoise_var's third output (null for rt_denoise, and for a null rt_denoise_variance).
#define DN_TEXT(text) (var_call ? "rt_denoise_var: " text : "rt_denoise: " text)
int denoise_args(bool var_call, const rt_denoise_params* p, const rt_denoise_inputs* in, const void* out_rgb, const void* out_bgr,
                 const void* out_var, const char** err) {
    auto refuse = [&](const char* why) {
        *err = why;
        return RT_E_INVALID;
    };
    if (!p || !in) return refuse(DN_TEXT("null argument"));
    if (p->width == 0 || p->height == 0) return refuse(DN_TEXT("width and height must be > 0"));
    if (p->iterations < 1 || p->iterations > kDnMaxIterations) return refuse(DN_TEXT("iterations must be 1..8"));
    if (p->flags & ~kDnAllFlags) return refuse(DN_TEXT("unknown flag bits"));
    if (p->normal_squarings > kDnMaxSquarings) return refuse(DN_TEXT("normal_squarings must be 0..10"));
    if (p->variant > 2) return refuse(DN_TEXT("variant must be 0, 1 or 2"));
    if (!in->rgb) return refuse(DN_TEXT("the rgb input is NULL"));
    if (((p->flags & RT_DN_NORMAL) && !in->normal) || ((p->flags & RT_DN_DEPTH) && !in->depth) ||
        ((p->flags & RT_DN_DEMODULATE) && !in->albedo))
        return refuse(DN_TEXT("a selected guide's buffer is NULL"));
    if ((p->flags & RT_DN_DEPTH) && !dn_sigma_ok(p->sigma_depth)) return refuse(DN_TEXT("sigma_depth must be finite and > 0"));
    if ((p->flags & RT_DN_COLOR) && !dn_sigma_ok(p->sigma_color)) return refuse(DN_TEXT("sigma_color must be finite and > 0"));
    if (!out_rgb && !out_bgr && !out_var) return refuse(var_call ? "rt_denoise_var: all three outputs are NULL" : "rt_denoise: both outputs are NULL");
    if (p->bgr_pitch != 0 && p->bgr_pitch / 3 < p->width) return refuse(DN_TEXT("bgr_pitch is below 3 * width"));
    if (out_rgb == static_cast<const void*>(in->rgb)) return refuse(DN_TEXT("out_rgb must not be the rgb input"));
    return RT_OK;
}
#undef DN_TEXT

}  // namespace

int plan_denoise_args(const rt_denoise_params* p, const rt_denoise_inputs* in, const void* out_rgb, const void* out_bgr,
                      const char** err) {
    return denoise_args(false, p, in, out_rgb, out_bgr, nullptr, err);
}

int plan_denoise_var_args(const rt_denoise_params* p, const rt_denoise_inputs* in, const rt_denoise_variance* var,
                          const void* out_rgb, const void* out_bgr, const char** err) {
    auto refuse = [&](const char* why) {
        *err = why;
        return RT_E_INVALID;
    };
    if (const int rc = denoise_args(true, p, in, out_rgb, out_bgr, var ? var->out_variance : nullptr, err); rc != RT_OK) return rc;
    if (!var) return refuse("rt_denoise_var: the rt_denoise_variance struct is NULL");
    if (!var->variance) return refuse("rt_denoise_var: the variance input is NULL");
    if (!dn_sigma_ok(var->sigma_variance)) return refuse("rt_denoise_var: sigma_variance must be finite and > 0");
    if (!dn_sigma_ok(var->variance_floor)) return refuse("rt_denoise_var: variance_floor must be finite and > 0");
    if (var->out_variance == var->variance) return refuse("rt_denoise_var: out_variance must not be the variance input");
    return RT_OK;
}

DenoisePlan plan_denoise(const rt_denoise_params& p) {
    DenoisePlan d;
    d.passes = p.iterations;
    const uint32_t variant = p.variant ? p.variant : kDnAutoVariant;
    d.variant = variant;
    for (uint32_t i = 0; i < d.passes && i < kDnMaxIterations; ++i) {
        d.step[i] = 1u << i;
        d.lds[i] = variant == 2 && d.step[i] <= kDnLdsMaxStep;
    }
    d.grid_x = (p.width + kDnTileW - 1) / kDnTileW;
    d.grid_y = (p.height + kDnTileH - 1) / kDnTileH;
    d.image_bytes = align_up(static_cast<uint64_t>(p.width) * p.height * kDnRecordBytes, 256);
    d.scratch_bytes = 3 * d.image_bytes;
    return d;
}

StreamShape plan_streams(const SceneFacts& sf, const int64_t* tune, int mode, int src, uint32_t max_depth) {
    StreamShape s;
    // tuning "split" 0: every kernel on one in-order stream (A/B measurement);
    // "deal": 1 workgroup-major chunk dealing (default), 0 workgroup-first;
    // "bstreams": streams for the shadow + shading kernels (default 2;
    // generations alternate over them).
    // default: two B streams when the tree is in LDS (C3: 3.30 vs 3.71 ms on one stream);
    // one stream when the nearest-hit walk reads the tree through L2 below its LDS prefix,
    // where the overlapped shadow / shading waves slow that chain more than they hide
    // (C4 55.2 vs 56.6-57.3 ms, C5 318 vs 330 ms, binary16 nodes; round 5 with the
    // high-priority chain: C4 51.9 vs 50.4 ms)
    const bool prefix_src = src == 5 || src == 6 || src == 8 || src == 26;
    s.split = tune[kTuneSplit] < 0 ? !prefix_src : tune[kTuneSplit] != 0;
    // two b streams (consecutive generations' shadows and shading overlap): measured
    // 3.87 -> 3.78 ms at C3 once the shading runs in its own kernel; three are slower
    s.n_b = std::max(1, std::min(kPlanMaxBStreams, static_cast<int>(tune[kTuneBStreams])));
    // generation 0: the camera's view grid (any sphere source), spheres staged in LDS when they
    // fit (3), else through L2 (4); the default where built (C3 camera pass 520 -> 327 us, 3.46 ->
    // 3.26 ms per frame on one box, against the camera-view tile walk it replaced); otherwise
    // (tuning "cam" other than 3 or -1, or no grid) per ray through the nearest-hit source
    s.cam = 0;
    if ((tune[kTuneCam] == 3 || (tune[kTuneCam] < 0 && mode == RT_ALGO_WAVEFRONT)) && sf.has_cgrid)
        s.cam = static_cast<size_t>(sf.n_spheres) * (sizeof(DevSphere) + sizeof(int32_t)) <= kLdsBudget ? 3 : 4;
    // every light gridded: the shadow kernel without a tree walk (spheres staged in LDS when
    // they fit in 64 KB); tuning "grid_occ" 0 keeps the general kernel
    s.grid_occ = (sf.all_lights_gridded && tune[kTuneGridOcc] != 0)
                     ? (static_cast<size_t>(sf.n_spheres) * sizeof(DevSphere) <= 64 * 1024 ? 1 : 2)
                     : 0;
    s.wg_major = tune[kTuneDeal] != 0 ? 1u : 0u;
    s.mark_gen = std::max(0, std::min<int>(static_cast<int>(tune[kTuneStaggerGen]), static_cast<int>(max_depth) + 1));
    return s;
}

uint64_t plan_cap_px(const int64_t* tune, uint64_t budget, uint64_t levels, bool aa) {
    const uint64_t cap_px = static_cast<uint64_t>(tune[kTuneChunkPixels]);
    if (cap_px != 0) return cap_px;
    return std::max<uint64_t>(1, budget / static_cast<uint64_t>(tune[kTuneLanes]) / wf_bytes_per_slot(levels, aa));
}

// Chunks of whole rows, multiples of 8 (the generation-0 8x8 tiles), sized so
// the lanes' working sets (wf_layout: queues, one shade-record array and one
// level array per lit generation, terminals) fit the budget:
// tuning "wf_budget_mb", else min(80 GB, 85% of the free device memory)
// (hipMemGetInfo), e.g. C4's 8192^2 frame in one chunk at depth 8 (62.8 vs
// 63.9 ms as two) and C5 in 7 at depth 16.  Balanced: a frame slightly over
// the cap becomes two halves, not a full chunk plus a sliver that pays every
// generation's launch latency again.  If hipMalloc still runs out of memory
// (another context, a caller's buffers), the chunks are halved and the
// allocation retried; results do not depend on the chunking.
ChunkPlan plan_chunks(const int64_t* tune, uint64_t cap_px, uint32_t tile_w, uint32_t tile_h, bool bands) {
    ChunkPlan p;
    p.tile_w = tile_w;
    p.tile_h = tile_h;
    p.tiles_x = (tile_w + 7) / 8;
    const int lanes_req = static_cast<int>(tune[kTuneLanes]);
    // rt_render into host memory: chunks of at most tile_h / host_chunks rows (the copy of a
    // chunk's rows overlaps the later chunks' generations); host_first sizes the first of two
    uint32_t first_rows = 0;
    if (bands && tune[kTuneHostChunks] > 1) {
        const uint64_t hc = static_cast<uint64_t>(tune[kTuneHostChunks]);
        const uint64_t pf = static_cast<uint64_t>(tune[kTuneHostFirst]);
        if (hc == 2 && pf > 0) {
            first_rows = static_cast<uint32_t>(std::max<uint64_t>(8, (tile_h * pf / 100) / 8 * 8));
            if (first_rows >= tile_h) first_rows = 0;
            else cap_px = std::min<uint64_t>(cap_px, static_cast<uint64_t>((std::max(first_rows, tile_h - first_rows) + 7) / 8 * 8) * tile_w);
        }
        if (first_rows == 0) cap_px = std::min<uint64_t>(cap_px, ((tile_h + hc - 1) / hc + 7) / 8 * 8 * tile_w);
    }
    uint32_t chunk_rows = static_cast<uint32_t>(std::max<uint64_t>(8, std::min<uint64_t>(cap_px / tile_w, UINT32_MAX) / 8 * 8));
    chunk_rows = std::min(chunk_rows, (tile_h + 7) / 8 * 8);
    const uint32_t n_chunks = (tile_h + chunk_rows - 1) / chunk_rows;
    chunk_rows = std::max<uint32_t>(8, ((tile_h + n_chunks - 1) / n_chunks + 7) / 8 * 8);
    if (first_rows) {                      // two chunks of first_rows and tile_h - first_rows rows
        const uint32_t need = (std::max(first_rows, tile_h - first_rows) + 7) / 8 * 8;
        if (n_chunks == 2 && need * static_cast<uint64_t>(tile_w) <= cap_px) chunk_rows = need;
        else first_rows = 0;
    }
    p.chunk_rows = chunk_rows;
    p.n_chunks = n_chunks;
    p.first_rows = first_rows;
    p.n_lanes = std::max(1, std::min<int>(lanes_req, static_cast<int>(n_chunks)));
    return p;
}

RegionPlan plan_regions(const int64_t* tune, int n_cu, const ChunkPlan& cp) {
    RegionPlan r;
    r.slots = cp.tiles_x * 64 * (cp.chunk_rows / 8);
    // G regions = workgroups per queue launch: two per CU, i.e. every
    // workgroup resident at once (1024 threads with the LDS-staged BVH),
    // so the wave-chunk dealing spreads even a small tail queue over the
    // whole chip in one round; fewer for small chunks; R covers every slot.
    const int g_env = static_cast<int>(tune[kTuneRegions]);
    uint32_t G = g_env > 0 ? static_cast<uint32_t>(g_env) : 2u * static_cast<uint32_t>(n_cu);
    G = std::max<uint32_t>(1, std::min<uint32_t>({G, static_cast<uint32_t>(kMaxRegions), (r.slots + kWfThreads - 1) / kWfThreads}));
    r.G = G;
    r.R = (r.slots + G * kWfThreads - 1) / (G * kWfThreads) * kWfThreads;
    return r;
}

// fused tail (tuning tail_fuse = T): the src-9 tree and light-view grid shadows
int plan_tail_fuse(const SceneFacts& sf, const int64_t* tune, int src, uint64_t slots, uint32_t max_depth) {
    // auto: from generation 4 for chunks of <= 4.5 M pixel slots (one rank's share of a 4- or
    // 8-way C3 frame), from 5 up to 9 M (a 2-way share); with the tail's own fold on one box:
    // 8-way share 0.855 -> 0.751 ms, 4-way 1.140 -> 1.040, 2-way 1.725 -> 1.642 (round 5
    // re-check: 4-way T 5 / 6 1.030 / 1.052 vs 1.039, 2-way T 6 / 7 1.675 / 1.683 vs 1.636-1.642)
    const uint64_t S = slots;
    int T = static_cast<int>(tune[kTuneTailFuse]);
    // above 9 M slots (the whole C3 frame): from generation max_depth - 1 when that is
    // >= 4 (round 5, depth 8: T = 7 2.898-2.902 vs 2.943-2.945 ms without the tail; 6 /
    // 8 / 9: 2.961 / 2.947-2.960 / 2.970 ms)
    if (T < 0) {
        const int late = static_cast<int>(max_depth) - 1;
        T = S <= 4500000u ? 4 : S <= 9000000u ? 5 : (late >= 4 ? late : 0);
    }
    const bool ok = T >= 1 && static_cast<uint32_t>(T) <= max_depth + 1 && src == 9 && sf.all_lights_gridded &&
                    tune[kTuneGridOcc] != 0;
    return ok ? T : 0;
}

WfLayout wf_layout(uint32_t cap, uint32_t G, uint32_t R, uint32_t levels, bool aa) {
    WfLayout w;
    const uint64_t q = static_cast<uint64_t>(G) * R;
    const uint64_t capa = align_up(q, 64);
    w.qcap = q;
    w.capa = capa;
    // section sizes (device_layout.hpp, WfBufs)
    w.s_queue = kWfQueueBytes * q;
    w.s_rec = static_cast<uint64_t>(levels) * q * kWfRecBytes;
    w.s_lev = static_cast<uint64_t>(levels) * capa * kWfLevBytes;
    w.s_term = capa * kWfTermBytes;
    w.s_reg = static_cast<uint64_t>(kMaxGenerations) * G * 4;
    w.s_cpix = q * kWfCpixBytes;
    w.s_pmap = static_cast<uint64_t>(cap) * kWfPmapBytes;
    w.s_ccol = capa * kWfCcolBytes;
    w.s_acc = aa ? static_cast<uint64_t>(cap) * kWfAccBytes : 0;
    uint64_t off = align_up(w.s_queue, 256);
    w.o_rec = off; off = align_up(off + w.s_rec, 256);
    w.o_lev = off; off = align_up(off + w.s_lev, 256);
    w.o_term = off; off = align_up(off + w.s_term, 256);
    w.o_rq = off; off = align_up(off + w.s_reg, 256);
    w.o_rs = off; off = align_up(off + w.s_reg, 256);
    w.o_cpix = off; off = align_up(off + w.s_cpix, 256);
    w.o_pmap = off; off = align_up(off + w.s_pmap, 256);
    w.o_ccol = off; off = align_up(off + w.s_ccol, 256);
    w.o_acc = off; off = align_up(off + w.s_acc, 256);
    w.total = off;
    return w;
}

}  // namespace rtamd
