// C ABI: frame / tile rendering.  The schedule comes from the planner (render_plan.hpp); here
// are the lanes and their working sets, the launches, rt_render's host path, rt_ctx_reserve and
// the statistics of the last render.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt_ctx.hpp"

using namespace rtamd;

static_assert(kPlanMaxBStreams == kMaxBStreams, "the planner's b-stream bound mirrors launch_api.hpp");

namespace {

SceneFacts scene_facts(const rt_ctx* c) {
    SceneFacts f;
    f.n_spheres = c->dsc.n_spheres; f.n_bvh = c->dsc.n_bvh; f.n_bvh4 = c->dsc.n_bvh4; f.n_q4 = c->dsc.n_q4;
    f.n_lights = c->dsc.n_lights;
    f.has_half = c->dsc.bvh_h != nullptr;
    f.has_cgrid = c->dsc.cgrid != nullptr;
    f.needs_path = c->dsc.needs_path != 0;
    f.deep_bvh4 = c->deep_bvh4; f.short_stack = c->short_stack; f.short_stack18 = c->short_stack18;
    f.q4_ok = c->q4_ok; f.all_lights_gridded = c->all_lights_gridded;
    return f;
}

// The b streams need hardware queues of their own: HIP deals streams over a
// few shared queues (GPU_MAX_HW_QUEUES), and two streams on one queue run
// strictly in submission order.  A CU-masked stream (mask = every CU) gets a
// dedicated queue.  Created on demand: every extra hardware queue costs the
// firmware scheduler, measurably slowing the others.
int ensure_bstreams(rt_ctx* c, rt_ctx::Lane& M, int nb) {
    std::vector<uint32_t> mask((c->n_cu + 31) / 32, 0u);
    const int keep = 5 - static_cast<int>(std::max<int64_t>(1, c->t(kTuneCuMask)));   // of every 4 CUs
    for (int cu = 0; cu < c->n_cu; ++cu)
        if (cu % 4 < keep) mask[cu / 32] |= 1u << (cu % 32);
    while (static_cast<int>(M.sb.size()) < nb) {
        hipStream_t s = nullptr;
        if (c->t(kTuneCuMask) == 0 ||
            hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(mask.size()), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        }
        M.sb.push_back(s);
        hipEvent_t e = nullptr;
        HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        M.b_done.push_back(e);
    }
    return RT_OK;
}

int flush_tally(rt_ctx* c);

// Release a lane's working set once the lane's own streams are idle: the only place lane
// memory is freed.  Called by
//   - drop_lanes (rt_ctx_destroy; rt_ctx_set_tuning when cu_mask, prio or a_queue changes),
//   - ensure_wf, before it allocates a larger working set (after the pending render's end),
//   - ensure_wavefront, for every lane, before a render retries with smaller chunks.
// A tally still pending (c->tally.on: a one-chunk render whose statistics nobody has read yet)
// holds pointers into a working set, so it is settled first: run now, on the context's stream,
// and waited for.  The counters then hold that render's totals and a later rt_ctx_stats /
// rt_ctx_generation_counts only reads them.  (rt_ctx_destroy drops the tally before it gets here.)
void release_lane_memory(rt_ctx* c, rt_ctx::Lane& L) {
    if (L.s) (void)hipStreamSynchronize(L.s);
    for (hipStream_t x : L.sb) if (x) (void)hipStreamSynchronize(x);
    if (!L.mem) return;
    const bool settled = c->tally.on;
    if (settled) {
        (void)flush_tally(c);              // clears tally.on whatever it returns
        (void)hipStreamSynchronize(c->stream);
    }
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: lane working set released (%llu MB), tally settled %d\n",
                     static_cast<unsigned long long>(L.bytes >> 20), settled ? 1 : 0);
    (void)hipFree(L.mem);
    L.mem = nullptr;
    L.bytes = 0;
}

// Default working-set budget of a render (all lanes): 85% of what the device
// has free plus what this context's lanes already hold, at most kWfBudget.
uint64_t default_wf_budget(rt_ctx* c) {
    size_t fr = 0, total = 0;
    uint64_t held = 0;
    for (const auto& L : c->lanes) held += L.bytes;
    if (hipMemGetInfo(&fr, &total) != hipSuccess) {
        (void)hipGetLastError();
        return kWfBudget;
    }
    return std::min<uint64_t>(kWfBudget, static_cast<uint64_t>(0.85 * static_cast<double>(fr + held)));
}

int ensure_lanes(rt_ctx* c, int n) {
    while (static_cast<int>(c->lanes.size()) < n) {
        rt_ctx::Lane L;
        c->lanes.push_back(L);
        rt_ctx::Lane& M = c->lanes.back();
        // prio: the nearest-hit chain (the critical path) on a high-priority stream
        int lo = 0, hi = 0;
        std::vector<uint32_t> all((c->n_cu + 31) / 32, 0u);
        for (int cu = 0; cu < c->n_cu; ++cu) all[cu / 32] |= 1u << (cu % 32);
        if (c->t(kTunePrio) && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) {
            HIP_TRY(c, hipStreamCreateWithPriority(&M.s, hipStreamNonBlocking, hi));
        } else if (c->t(kTuneAQueue) == 0 ||
                   hipExtStreamCreateWithCUMask(&M.s, static_cast<uint32_t>(all.size()), all.data()) != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(c, hipStreamCreateWithFlags(&M.s, hipStreamNonBlocking));
        }
        HIP_TRY(c, hipEventCreateWithFlags(&M.mark, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&M.done, hipEventDisableTiming));
        M.near_done.assign(kMaxGenerations, nullptr);
        for (hipEvent_t& e : M.near_done) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&M.dj), kDjWords * sizeof(uint64_t)));
        HIP_TRY(c, hipMemset(M.dj, 0, kDjWords * sizeof(uint64_t)));
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&M.dj_err), sizeof(uint64_t), hipHostMallocMapped));
        *M.dj_err = 0;
        HIP_TRY(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&M.dj_err_dev), M.dj_err, 0));
    }
    return RT_OK;
}

// A lane's wavefront working set for chunks of up to `cap` pixels, laid out by wf_layout and
// grown on demand.
int ensure_wf(rt_ctx* c, rt_ctx::Lane& L, uint32_t cap, uint32_t G, uint32_t R, uint32_t levels, bool aa) {
    WfBufs& b = L.b;
    const WfLayout w = wf_layout(cap, G, R, levels, aa);
    b.o_rec = w.o_rec; b.o_lev = w.o_lev; b.o_term = w.o_term; b.o_rq = w.o_rq; b.o_rs = w.o_rs;
    b.o_cpix = w.o_cpix; b.o_pmap = w.o_pmap; b.o_ccol = w.o_ccol;
    const uint64_t off = w.total;
    if (off > L.bytes) {
        if (L.mem) {
            // every render still using it is done (its chain may have run on a caller's stream)
            if (c->render_pending) (void)hipEventSynchronize(c->render_done);
            release_lane_memory(c, L);
        }
        // ask only for what the device has free, less the runtime's scratch headroom: a request
        // beyond it is answered without hipMalloc (the runtime has crashed inside a failing
        // hipMalloc of a few hundred GB, seen with an explicit oversized wf_budget_mb), and a
        // working set that took the last free bytes would leave nothing for the scratch the
        // runtime allocates per hardware queue at a kernel's first launch there.  The free
        // memory is the device's: other contexts and processes count, so the caller's halving
        // of the chunks is reported under tuning verbose and in rt_stats.chunks.
        size_t fr = 0, total = 0;
        if (hipMemGetInfo(&fr, &total) == hipSuccess && (off > fr || fr - off < kRuntimeHeadroom)) {
            if (c->t(kTuneVerbose))
                std::fprintf(stderr, "rtamd: working set of %llu MB does not fit %llu MB free (less %llu MB headroom): "
                             "halving the chunk\n", static_cast<unsigned long long>(off >> 20),
                             static_cast<unsigned long long>(fr >> 20), static_cast<unsigned long long>(kRuntimeHeadroom >> 20));
            return fail(c, RT_E_NOMEM, "wavefront working set of " + std::to_string(off >> 20) + " MB does not fit (" +
                                           std::to_string(fr >> 20) + " MB free)");
        }
        (void)hipGetLastError();
        const hipError_t e = hipMalloc(&L.mem, off);
        if (e == hipErrorOutOfMemory) {          // the caller retries with smaller chunks
            (void)hipGetLastError();
            L.mem = nullptr;
            if (c->t(kTuneVerbose))
                std::fprintf(stderr, "rtamd: hipMalloc of %llu MB failed: halving the chunk\n",
                             static_cast<unsigned long long>(off >> 20));
            return fail(c, RT_E_NOMEM, "wavefront working set of " + std::to_string(off >> 20) + " MB does not fit");
        }
        if (e != hipSuccess) return hip_fail(c, e, "hipMalloc(wavefront working set)");
        L.bytes = off;
        if (c->t(kTuneVerbose))
            std::fprintf(stderr, "rtamd: lane working set grown to %llu KB\n", static_cast<unsigned long long>(off >> 10));
    }
    b.mem = static_cast<unsigned char*>(L.mem);
    // the running sums of a render of one pass per AA sample (the layout's last section)
    L.acc = aa ? reinterpret_cast<double*>(static_cast<unsigned char*>(L.mem) + w.o_acc) : nullptr;
    b.totals = c->d_counters + kTotals;
    b.gen_totals = c->d_counters + kGenTotals;
    b.qcap = w.qcap;
    b.cap = cap;
    b.capa = static_cast<uint32_t>(w.capa);
    b.levels = levels;
    b.G = G;
    b.R = R;
    return RT_OK;
}

int check_opts(rt_ctx* c, const rt_render_opts* o, uint32_t& spp, uint32_t& band, uint32_t& stride, uint32_t& pitch) {
    if (!o) return fail(c, RT_E_INVALID, "null opts");
    if (o->width == 0 || o->height == 0) return fail(c, RT_E_INVALID, "empty frame");
    if (o->jitter != RT_JITTER_CENTER && o->jitter != RT_JITTER_RANDOM) return fail(c, RT_E_INVALID, "bad jitter mode");
    if (o->max_depth > RT_MAX_DEPTH_LIMIT) return fail(c, RT_E_INVALID, "max_depth above RT_MAX_DEPTH_LIMIT");
    band = o->band ? o->band : 1;
    stride = o->band_stride ? o->band_stride : 1;
    if (o->band_phase >= stride) return fail(c, RT_E_INVALID, "band_phase >= band_stride");
    if (static_cast<uint64_t>(o->x0) + o->tile_w > o->width) return fail(c, RT_E_INVALID, "tile exceeds frame width");
    if (o->tile_h) {
        uint64_t j = o->tile_h - 1;
        uint64_t last = o->y0 + ((j / band) * stride + o->band_phase) * band + j % band;
        if (last >= o->height) return fail(c, RT_E_INVALID, "tile exceeds frame height");
    }
    spp = o->spp ? o->spp : c->scene_spp;                     // 0: the scene's Options.antialias
    if (spp == 0) return fail(c, RT_E_INVALID, "spp is 0 and the scene's antialias is 0");
    pitch = o->bgr_pitch ? o->bgr_pitch : 3 * o->tile_w;
    if (pitch < 3 * o->tile_w) return fail(c, RT_E_INVALID, "bgr_pitch < 3*tile_w");
    if (o->algo < RT_ALGO_AUTO || o->algo > RT_ALGO_WAVEFRONT_AA) return fail(c, RT_E_INVALID, "bad algo");
    return RT_OK;
}

// What begin_render hands every schedule: the stream, the frame's parameters, the samples per pixel.
struct RenderCall {
    hipStream_t st = nullptr;
    FrameParams fp{};
    uint32_t spp = 1;
};

// Option checks, the render's stream (which waits for the context's previous render) and FrameParams.
int begin_render(rt_ctx* c, const rt_render_opts* o, void* d_rgb, void* d_bgr, void* stream, RenderCall& rcall) {
    if (!c->has_scene) return fail(c, RT_E_NOSCENE, "no scene uploaded");
    uint32_t spp, band, stride, pitch;
    int rc = check_opts(c, o, spp, band, stride, pitch);
    if (rc != RT_OK) return rc;
    if (o->flags & RT_OUT_FRAME_ROWS) return fail(c, RT_E_INVALID, "RT_OUT_FRAME_ROWS is for rt_render's host buffers");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    // The context's working sets (counters, wavefront buffers, path stacks) are
    // shared by its renders: a render on another stream waits for the previous one.
    // (on the stream the previous render ended on, stream order alone suffices)
    if (c->render_pending && st != c->done_stream) HIP_TRY(c, hipStreamWaitEvent(st, c->render_done, 0));
    FrameParams& fp = rcall.fp;
    fp = FrameParams{};
    fp.hw = static_cast<double>(o->width) / 2.0;              // main.rs:39-41
    fp.hh = static_cast<double>(o->height) / 2.0;
    fp.scale = std::fmax(1.0 / fp.hw, 1.0 / fp.hh);
    fp.x0 = o->x0; fp.tile_w = o->tile_w; fp.y0 = o->y0; fp.tile_h = o->tile_h;
    fp.band = band; fp.band_stride = stride; fp.band_phase = o->band_phase;
    fp.max_depth = o->max_depth;
    fp.spp = spp;
    fp.bgr_pitch = pitch;
    fp.pad_end = 3 * o->tile_w;
    fp.out_rgb = (o->flags & RT_OUT_RGB_F32) ? static_cast<float*>(d_rgb) : nullptr;
    fp.out_bgr = (o->flags & RT_OUT_BGR_U8) ? static_cast<uint8_t*>(d_bgr) : nullptr;
    fp.counters = c->d_counters;
    fp.jitter = o->jitter;
    fp.seed = o->seed;
    fp.srgb = c->d_srgb;
    {
        // The background pixel exactly as average_samples + to_srgb produce it on the
        // device (same f64 operations): camera misses are written by wf_nearest directly.
        double px[3];
        for (int k = 0; k < 3; ++k) {
            const double cam = (0.0 + c->dsc.bg[k]) / 1.0;        // raytrace.rs:270-276, one camera sample
            double acc = 0.0;
            for (uint32_t q = 0; q < spp; ++q) acc = acc + cam;    // main.rs:47-55
            px[k] = acc / static_cast<double>(spp);
            fp.bg_rgb[k] = static_cast<float>(px[k]);
        }
        fp.bg_bgr[0] = to_srgb(px[2]);                             // color.rs:628-632, B G R
        fp.bg_bgr[1] = to_srgb(px[1]);
        fp.bg_bgr[2] = to_srgb(px[0]);
    }
    fp.row0 = 0;
    fp.rows = o->tile_h;
    rcall.st = st;
    rcall.spp = spp;
    return RT_OK;
}

// The render's end on its stream: the next render (and the statistics) wait for render_done.
int end_render(rt_ctx* c, hipStream_t st, bool timed) {
    HIP_TRY(c, hipEventRecord(c->render_done, st));
    c->done_stream = st;
    c->render_pending = true;
    c->last_timed = timed;
    return RT_OK;
}

// the statistics counters start at zero: cleared by the render, or, for a one-chunk wavefront
// render without RT_COUNT_WORK (its tally is lazy), by flush_tally just before that tally
int zero_counters(rt_ctx* c, hipStream_t st) {
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, kCounterWords * sizeof(unsigned long long), st));
    return RT_OK;
}

// The schedule of one wavefront render (render_plan.hpp).
struct WfPlan {
    bool aa = false;                   // one pass per AA sample (RT_ALGO_WAVEFRONT_AA, random jitter, spp > 1)
    SourcePair sp;
    StreamShape sh;
    ChunkPlan cp;
    RegionPlan rg;
    int tail_fuse = 0;
};

// Lanes, b streams and working sets for the plan's chunks.  If a working set does not fit
// (another context, a caller's buffers), the chunks are halved and the allocation retried;
// results do not depend on the chunking.
int ensure_wavefront(rt_ctx* c, const rt_render_opts* o, RenderReq req, uint64_t cap_px, WfPlan& p) {
    const uint32_t levels = o->max_depth + 1;
    for (;;) {
        p.cp = plan_chunks(c->tune, cap_px, o->tile_w, o->tile_h, req.bands);
        int rc = ensure_lanes(c, p.cp.n_lanes);
        if (rc != RT_OK) return rc;
        p.rg = plan_regions(c->tune, c->n_cu, p.cp);
        for (int l = 0; l < p.cp.n_lanes && rc == RT_OK; ++l) {
            if (p.sh.split && (rc = ensure_bstreams(c, c->lanes[l], p.sh.n_b)) != RT_OK) return rc;
            rc = ensure_wf(c, c->lanes[l], p.cp.cap(), p.rg.G, p.rg.R, levels, p.aa);
        }
        if (rc == RT_OK) return RT_OK;
        if (rc != RT_E_NOMEM || p.cp.chunk_rows <= 8) return rc;
        for (auto& L : c->lanes) release_lane_memory(c, L);     // retry with half the pixels per chunk
        cap_px = p.cp.next_cap_px();
    }
}

// rt_ctx_reserve: warm every stream the planned render would use instead of launching it.
int warm_wavefront(rt_ctx* c, RenderReq req, hipStream_t st, const WfPlan& p) {
    std::vector<hipStream_t> ss{st};
    if (req.bands) {                       // rt_render's copy stream and its band events
        if (const int rc = ensure_copy_stream(c); rc != RT_OK) return rc;
        ss.push_back(c->copy_stream);
        for (uint32_t i = 0; i < p.cp.n_chunks && i < static_cast<uint32_t>(kMaxBands); ++i)
            if (!c->band_ev[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->band_ev[i], hipEventDisableTiming));
    }
    for (int l = 0; l < p.cp.n_lanes; ++l) {
        ss.push_back(c->lanes[l].s);
        if (p.sh.split)
            for (int i = 0; i < p.sh.n_b; ++i) ss.push_back(c->lanes[l].sb[i]);
    }
    return warm_streams(c, ss);
}

// How one render's chunks are launched (fixed for the render).
struct WfRun {
    hipStream_t st = nullptr;          // the caller's stream
    bool count = false;                // RT_COUNT_WORK
    bool lazy_tally = false;           // one chunk on one lane: the tally waits for a statistics call
    bool timed = false;                // per-launch timing (needs one in-order stream per lane)
    bool on_caller = false;            // the chain runs on the caller's stream itself
    LaunchMarks marks, marks_b[kMaxBStreams];
};

// The streams, events and buffers launch_wavefront gets for chunk ci on lane L (the context's
// state is not changed: ws.fold_ev points at its band event).
WfStreams wire_streams(rt_ctx* c, const WfPlan& p, WfRun& run, rt_ctx::Lane& L, uint32_t ci, const FrameParams& fp) {
    const bool split = p.sh.split;
    WfStreams ws{};
    ws.a = run.on_caller ? run.st : L.s;
    ws.nb = split ? p.sh.n_b : 1;
    for (int i = 0; i < ws.nb; ++i) {
        ws.b[i] = split ? L.sb[i] : ws.a;
        ws.b_done[i] = split ? L.b_done[i] : nullptr;
        ws.mb[i] = run.timed ? (split ? &run.marks_b[i] : &run.marks) : nullptr;
    }
    ws.near_done = L.near_done.data();
    ws.tail_fuse = p.tail_fuse;
    ws.tail_width = static_cast<int>(c->t(kTuneTailWidth));
    ws.tail_wgs = static_cast<int>(std::min<uint32_t>(p.rg.G, static_cast<uint32_t>(c->n_cu)));
    ws.ma = run.timed ? &run.marks : nullptr;
    if (split && c->t(kTuneDevJoin)) {
        ws.dj_flags = L.dj;
        ws.dj_next = &L.dj_n;
        ws.dj_err = L.dj_err_dev;
    }
    ws.lazy_tally = run.lazy_tally;
    ws.cam = p.sh.cam;
    ws.fold_ev = c->n_bands == 0 ? nullptr : &c->band_ev[ci];
    if (c->sparse_on) {
        ws.sp_s = c->copy_stream;
        ws.sp_cam = c->sp_cam;
        ws.sp_ready = c->sp_ready;
        ws.sp_bits = c->d_sp_bits; ws.sp_cnt = c->d_sp_cnt; ws.sp_off = c->d_sp_off;
        ws.sp_bgr = fp.out_bgr ? c->d_sp_bgr : nullptr;
        ws.sp_rgb = fp.out_rgb ? c->d_sp_rgb : nullptr;
    }
    ws.grid_occ = p.sh.grid_occ;
    return ws;
}

// The planned chunks, dealt round-robin over the lanes.
int launch_chunks(rt_ctx* c, const rt_render_opts* o, RenderReq req, const RenderCall& rcall, const WfPlan& p) {
    const hipStream_t st = rcall.st;
    const int n_lanes = p.cp.n_lanes;
    WfRun run;
    run.st = st;
    run.count = (o->flags & RT_COUNT_WORK) != 0;
    // (a render of several passes tallies each pass as it ends: the next pass reuses the queue sizes)
    run.lazy_tally = p.cp.n_chunks == 1 && n_lanes == 1 && !p.aa;
    if (!run.lazy_tally || run.count)
        if (const int rc = zero_counters(c, st); rc != RT_OK) return rc;
    // per-launch timing needs one in-order stream
    run.timed = (o->flags & RT_TIME_KERNELS) != 0 && n_lanes == 1;
    for (int i = -1; i < kMaxBStreams; ++i) {
        LaunchMarks* m = i < 0 ? &run.marks : &run.marks_b[i];
        m->pool = &c->tev;
        m->used = &c->t_used;
        m->out = &c->tint;
    }
    // the chain on the caller's stream (tuning chain_on_caller, one lane), or on the lane's own
    // (high-priority) stream after a fork from the caller's; the b streams need no fork: their
    // first work waits for the chain's generation 0 (near_done), which comes after it
    run.on_caller = c->t(kTuneChainOnCaller) != 0 && n_lanes == 1;
    c->ev0_set = !req.skip_ev0;
    if (c->ev0_set) HIP_TRY(c, hipEventRecord(c->ev0, st));
    if (!run.on_caller) {
        HIP_TRY(c, hipEventRecord(c->fork, st));
        for (int l = 0; l < n_lanes; ++l) HIP_TRY(c, hipStreamWaitEvent(c->lanes[l].s, c->fork, 0));
    }
    for (uint32_t ci = 0; ci < p.cp.n_chunks; ++ci) {
        rt_ctx::Lane& L = c->lanes[ci % n_lanes];
        if (ci > 0 && n_lanes > 1) HIP_TRY(c, hipStreamWaitEvent(L.s, c->lanes[(ci - 1) % n_lanes].mark, 0));
        FrameParams f = rcall.fp;
        f.row0 = p.cp.row0(ci);
        f.rows = p.cp.nrows(ci);
        WfBufs b = L.b;
        b.slots = p.cp.tiles_x * 64 * ((f.rows + 7) / 8);
        const WfStreams ws = wire_streams(c, p, run, L, ci, rcall.fp);
        if (ws.dj_flags) c->dj_used = true;     // the render joins its streams on the device (check_join_error)
        if (run.lazy_tally) {
            c->tally.on = true;
            c->tally.zero = !run.count;     // (a counted render zeroed them above: its test counts are in them)
            c->tally.fp = f;
            c->tally.b = b;
            c->tally.n_lights = c->dsc.n_lights;
            c->tally.gens = static_cast<int>(o->max_depth) + 2;
        }
        // RT_ALGO_WAVEFRONT_AA: the chunk's passes back to back on its lane (stream order and the
        // passes' own joins order a pixel's samples); the last one resolves the chunk's rows, and
        // only it records the lane's mark and the chunk's band event
        // rt_render_accumulate: passes S .. S + n - 1 (aa_pass: the global sample index, so aa_add's "pass 0
        // stores" is "the first sample stores") straight onto the accumulator's rows of the chunk (the sums
        // are tile-wide; a chunk addresses them by its first row); aa_spp is 0, which no pass number + 1
        // reaches: launch_wavefront never runs the per-chunk accum_resolve
        const uint32_t passes = req.accumulate ? req.acc_n : p.aa ? f.aa_spp : 1u;
        for (uint32_t a = 0; a < passes; ++a) {
            const bool last = a + 1 == passes;
            f.aa_pass = req.acc_first + a;
            f.aa_acc = req.accumulate ? req.acc + 3 * static_cast<size_t>(f.row0) * f.tile_w : p.aa ? L.acc : nullptr;
            f.aa_flags = (p.aa && last && ci + 1 == p.cp.n_chunks ? kAaTallyGens : 0u) | (req.acc_moments ? kAaMoments : 0u);
            WfStreams wp = ws;
            if (!last) wp.fold_ev = nullptr;
            HIP_TRY(c, launch_wavefront(c->dsc, f, b, p.sp.src, p.sp.src_occ, run.count, wp, last ? L.mark : nullptr,
                                        p.sh.mark_gen));
        }
    }
    for (int l = 0; l < n_lanes && !run.on_caller; ++l) {
        HIP_TRY(c, hipEventRecord(c->lanes[l].done, c->lanes[l].s));
        HIP_TRY(c, hipStreamWaitEvent(st, c->lanes[l].done, 0));
    }
    c->wf_used = true;
    return RT_OK;
}

// RT_ALGO_WAVEFRONT / RT_ALGO_WAVEFRONT_BRUTE: plan, make sure of lanes, streams and working
// sets, then the dry warm-up (rt_ctx_reserve) or the launches.
int render_wavefront(rt_ctx* c, const rt_render_opts* o, RenderReq req, const RenderCall& rcall, const SceneFacts& sf,
                     int mode, bool aa) {
    const FrameParams& fp = rcall.fp;
    WfPlan p;
    p.aa = aa;
    p.sp = plan_sources(sf, c->tune, mode);
    if (p.sp.sets_prefix) {
        c->dsc.pfx2 = p.sp.pfx2;
        c->dsc.pfxq = p.sp.pfxq;
    }
    p.sh = plan_streams(sf, c->tune, mode, p.sp.src, o->max_depth);
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: wavefront src %d occ %d cam %d deep4 %d short_stack %d split %d pfx %d/%d\n",
                     p.sp.src, p.sp.src_occ, p.sh.cam, c->deep_bvh4 ? 1 : 0, c->short_stack ? 1 : 0, p.sh.split ? 1 : 0,
                     c->dsc.pfx2, c->dsc.pfxq);
    // the chunk cap: tuning "chunk_pixels", else what the working-set budget (tuning "wf_budget_mb",
    // else default_wf_budget) holds at this depth
    uint64_t budget = 0;
    if (c->t(kTuneChunkPixels) == 0)
        budget = c->t(kTuneWfBudgetMb) > 0 ? static_cast<uint64_t>(c->t(kTuneWfBudgetMb)) << 20 : default_wf_budget(c);
    int rc = ensure_wavefront(c, o, req, plan_cap_px(c->tune, budget, o->max_depth + 1ull, aa), p);
    if (rc != RT_OK) return rc;
    p.tail_fuse = plan_tail_fuse(sf, c->tune, p.sp.src, static_cast<uint64_t>(p.cp.tiles_x) * 64u * (p.cp.chunk_rows / 8),
                                 o->max_depth);
    // sparse host copies: a whole tile (contiguous rows or row bands) in one chunk on one lane,
    // pixels written where they end
    // (not for passes per AA sample: no pixel is final before the chunk's resolve)
    c->sparse_on = req.sparse && !aa && p.cp.n_chunks == 1 && p.cp.n_lanes == 1 && c->t(kTuneCompose) == 0 &&
                   (fp.out_rgb || fp.out_bgr);
    if (c->sparse_on) {
        bool ok = false;
        if ((rc = ensure_sparse(c, rcall.st, o->tile_w, o->tile_h, fp.out_bgr != nullptr, fp.out_rgb != nullptr, &ok)) != RT_OK)
            return rc;
        if (!ok && c->t(kTuneVerbose)) std::fprintf(stderr, "rtamd: sparse copy buffers do not fit: plain copies\n");
        c->sparse_on = ok;
    }
    if (req.dry) return warm_wavefront(c, req, rcall.st, p);
    for (int l = 0; l < p.cp.n_lanes; ++l) {
        c->lanes[l].b.tiles_x = p.cp.tiles_x;
        c->lanes[l].b.wg_major = p.sh.wg_major;
        c->lanes[l].b.spread_below = static_cast<uint32_t>(c->t(kTuneSpreadBelow));
        c->lanes[l].b.compose = c->t(kTuneCompose) != 0 ? 1u : 0u;
        c->lanes[l].b.mark = c->sparse_on ? 1u : 0u;
    }
    c->last_chunks = p.cp.n_chunks;
    // rt_render copies each chunk's rows as soon as that chunk's fold is done (the fold
    // runs in chain order, so a chunk's rows are final together)
    c->n_bands = 0;
    if (req.bands && p.cp.n_chunks <= static_cast<uint32_t>(kMaxBands)) {
        for (uint32_t i = 0; i < p.cp.n_chunks; ++i) {
            if (!c->band_ev[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->band_ev[i], hipEventDisableTiming));
            c->band_row0[i] = p.cp.row0(i);
            c->band_nrows[i] = p.cp.nrows(i);
        }
        c->n_bands = static_cast<int>(p.cp.n_chunks);
    }
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: chunks %u x %u rows (first %u), lanes %d, G %u, R %u\n", p.cp.n_chunks, p.cp.chunk_rows,
                     p.cp.first_rows, p.cp.n_lanes, p.rg.G, p.rg.R);
    if (aa && !req.accumulate && c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: aa passes %u, chunks %u x %u rows, resolve after each chunk's last pass, sums %s\n",
                     fp.aa_spp, p.cp.n_chunks, p.cp.chunk_rows, c->t(kTuneCompose) ? "row by row (compose)" : "per pixel");
    if (req.accumulate && c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: accumulate samples [%u, %u) passes%s\n"
                             "rtamd: aa passes %u, chunks %u x %u rows, no resolve (the accumulator keeps the sums), sums %s\n",
                     req.acc_first, req.acc_first + req.acc_n, req.acc_moments ? " moments" : "", req.acc_n, p.cp.n_chunks, p.cp.chunk_rows,
                     c->t(kTuneCompose) ? "row by row (compose)" : "per pixel");
    return launch_chunks(c, o, req, rcall, p);
}

// RT_ALGO_PATH: a persistent grid, enough work-items to fill every CU; each owns one
// recursion stack of max_depth + 1 frames (PathStack)
int render_path(rt_ctx* c, const rt_render_opts* o, RenderReq req, RenderCall& rcall) {
    const hipStream_t st = rcall.st;
    const uint64_t npix = static_cast<uint64_t>(o->tile_w) * o->tile_h;
    // work-items per CU = the kernel's occupancy (4 SIMDs x waves per SIMD x 64 lanes)
    const uint32_t T_full = static_cast<uint32_t>(c->n_cu) * 256u * static_cast<uint32_t>(path_waves_per_simd());
    // lanes per pixel: enough work-items to fill the chip, at most one per AA sample (an accumulating
    // render: per sample of this call)
    const uint32_t G = plan_path_group(npix, req.accumulate ? req.acc_n : rcall.spp, T_full, c->t(kTunePathGroup));
    rcall.fp.path_group = G;
    if (req.accumulate) {                // samples [aa_pass, aa_pass + aa_spp) onto the sums at aa_acc
        rcall.fp.aa_pass = req.acc_first;
        rcall.fp.aa_spp = req.acc_n;
        rcall.fp.aa_acc = req.acc;
        rcall.fp.aa_flags = req.acc_moments ? kAaMoments : 0u;
    }
    const uint32_t T = static_cast<uint32_t>(std::min<uint64_t>(T_full, (npix * G + 255) / 256 * 256));
    PathStack ps{};
    ps.T = T;
    ps.levels = o->max_depth + 1;
    const size_t need = PathStack::bytes(T, ps.levels);
    if (need > c->path_bytes) {
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->d_path) (void)hipFree(c->d_path);
        c->d_path = nullptr;
        c->path_bytes = 0;
        HIP_TRY(c, hipMalloc(&c->d_path, need));
        c->path_bytes = need;
    }
    ps.mem = static_cast<unsigned char*>(c->d_path);
    if (req.dry) return warm_streams(c, {st});
    if (const int rc = zero_counters(c, st); rc != RT_OK) return rc;
    const bool staged = path_lds_bytes(c->dsc, true) <= 48 * 1024;
    if (req.accumulate && c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: accumulate samples [%u, %u) path%s\n", req.acc_first, req.acc_first + req.acc_n,
                     req.acc_moments ? " moments" : "");
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: path G %u T %u staged %d npix %llu\n", G, T, staged ? 1 : 0,
                     static_cast<unsigned long long>(npix));
    c->ev0_set = true;
    HIP_TRY(c, hipEventRecord(c->ev0, st));
    HIP_TRY(c, launch_path(c->dsc, rcall.fp, ps, staged, st, req.accumulate));
    return RT_OK;
}

// RT_ALGO_BRUTE_LDS / RT_ALGO_BRUTE_GLOBAL: the megakernel
int render_brute(rt_ctx* c, RenderReq req, const RenderCall& rcall, int mode) {
    if (req.dry) return warm_streams(c, {rcall.st});
    if (const int rc = zero_counters(c, rcall.st); rc != RT_OK) return rc;
    c->ev0_set = true;
    HIP_TRY(c, hipEventRecord(c->ev0, rcall.st));
    HIP_TRY(c, launch_trace_frame(c->dsc, rcall.fp, mode, rcall.st));
    return RT_OK;
}

int render_device(rt_ctx* c, const rt_render_opts* o, void* d_rgb, void* d_bgr, void* stream, RenderReq req) {
    RenderCall rcall;
    int rc = begin_render(c, o, d_rgb, d_bgr, stream, rcall);
    if (rc != RT_OK) return rc;
    const hipStream_t st = rcall.st;
    if (req.zero_pad) rcall.fp.pad_end = rcall.fp.bgr_pitch;
    const SceneFacts sf = scene_facts(c);
    int mode = o->algo;
    const char* refusal = nullptr;
    AccumPlan ap;
    if (req.accumulate) {        // rt_render_accumulate: its own rules (passes forced, every sample traced)
        if ((rc = plan_accumulate(sf, o->algo, o->flags, req.acc_first, req.acc_n, static_cast<int>(c->t(kTuneAaWavefront)),
                                  &ap, &refusal)) != RT_OK)
            return fail(c, rc, refusal);
        if (req.acc_n == 0) return RT_OK;                           // nothing to render
        mode = ap.mode;
    } else if ((rc = plan_algo(sf, o->algo, o->jitter, rcall.spp, &mode, &refusal, static_cast<int>(c->t(kTuneAaWavefront)))) != RT_OK)
        return fail(c, rc, refusal);
    // RT_ALGO_WAVEFRONT_AA: one pass of RT_ALGO_WAVEFRONT's schedule per AA sample, each a render of
    // one sample per pixel (its tally counts its own rays) that adds to the pixels' running sums;
    // with centre jitter or one sample it is RT_ALGO_WAVEFRONT's render
    const bool aa = req.accumulate ? ap.passes > 0 : plan_aa_passes(mode, o->jitter, rcall.spp);
    if (mode == RT_ALGO_WAVEFRONT_AA) mode = RT_ALGO_WAVEFRONT;
    if (aa) {
        rcall.fp.aa_spp = req.accumulate ? 0u : rcall.spp;                 // (accumulating: nothing divides)
        rcall.fp.spp = 1;
        for (int k = 0; k < 3; ++k) rcall.fp.aa_bg[k] = (0.0 + c->dsc.bg[k]) / 1.0;   // raytrace.rs:270-276, one camera sample
    }
    if (!req.dry) {
        c->tally.on = false;
        c->last_pixels = static_cast<uint64_t>(o->tile_w) * o->tile_h;
        c->last_stream = st;
        c->last_spp_traced = 1;
        c->last_chunks = 0;
    }
    c->n_bands = 0;
    c->sparse_on = false;
    const bool empty = o->tile_w == 0 || o->tile_h == 0;
    if (req.dry && empty) return warm_streams(c, {st});
    if (empty) {
        if ((rc = zero_counters(c, st)) != RT_OK) return rc;
        return end_render(c, st, false);
    }
    if (mode == RT_ALGO_WAVEFRONT || mode == RT_ALGO_WAVEFRONT_BRUTE) rc = render_wavefront(c, o, req, rcall, sf, mode, aa);
    else if (mode == RT_ALGO_PATH) rc = render_path(c, o, req, rcall);
    else rc = render_brute(c, req, rcall, mode);
    if (rc != RT_OK || req.dry) return rc;
    // the chain schedules (wavefront, megakernel) trace one camera ray tree per
    // pixel and count it spp times: the spp centre-jitter samples are identical
    // (not the passes per AA sample: every sample is traced)
    if (mode != RT_ALGO_PATH && !aa) c->last_spp_traced = rcall.spp;
    return end_render(c, st, true);
}

// The tally a one-chunk render left pending, after that render, on the context's stream.
int flush_tally(rt_ctx* c) {
    if (!c->tally.on) return RT_OK;
    c->tally.on = false;
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->render_done, 0));
    if (c->tally.zero) HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, kCounterWords * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, launch_tally(c->tally.fp, c->tally.b, c->tally.n_lights, c->tally.gens, c->stream));
    return RT_OK;
}

// rt_render and rt_ctx_reserve(host): the layout on both sides, the device frame of the tile
// and the request the render gets.
struct HostRender {
    OutMap mr, mb;
    rt_render_opts oo{};       // the options of the render into the device frame
    RenderReq req;
};
int host_request(rt_ctx* c, const rt_render_opts* o, bool rgb, bool bgr, bool dry, HostRender& h) {
    uint32_t spp, band, stride, pitch;
    int rc = check_opts(c, o, spp, band, stride, pitch);
    if (rc != RT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t dev_pitch = pitch;
    if ((rc = host_layout(c, o, pitch, h.mr, h.mb, &dev_pitch)) != RT_OK) return rc;
    h.oo = *o;
    h.oo.flags = (o->flags & ~(RT_OUT_RGB_F32 | RT_OUT_BGR_U8 | RT_OUT_FRAME_ROWS)) | (rgb ? RT_OUT_RGB_F32 : 0) |
                 (bgr ? RT_OUT_BGR_U8 : 0);
    h.oo.bgr_pitch = dev_pitch;
    // an earlier rt_render's copies (copy stream) are done with d_rgb / d_bgr: copy_to_host returns
    // only once its last piece has been drained or synchronised
    if ((rc = ensure_host_frame(c, rgb ? h.mr.dev_pitch * o->tile_h : 0, bgr ? h.mb.dev_pitch * o->tile_h : 0)) != RT_OK)
        return rc;
    h.req = RenderReq{};
    h.req.bands = true;
    h.req.zero_pad = true;
    h.req.sparse = c->t(kTuneSparseOut) != 0;
    h.req.banded_copy = stride > 1;
    h.req.dry = dry;
    return RT_OK;
}

int render_host(rt_ctx* c, const rt_render_opts* o, float* out_rgb, uint8_t* out_bgr, rt_stats* stats) {
    HostRender h;
    int rc = host_request(c, o, out_rgb != nullptr, out_bgr != nullptr, false, h);
    if (rc != RT_OK) return rc;
    if ((rc = render_device(c, &h.oo, c->d_rgb, c->d_bgr, nullptr, h.req)) != RT_OK) return rc;
    if (c->sparse_on) {
        if ((rc = copy_sparse(c, h.req, o, out_rgb, out_bgr, h.mr, h.mb)) != RT_OK) return rc;
    } else {
        if (out_bgr && (rc = copy_to_host(c, h.req, out_bgr, c->d_bgr, h.mb, o->tile_h)) != RT_OK) return rc;
        if (out_rgb && (rc = copy_to_host(c, h.req, out_rgb, c->d_rgb, h.mr, o->tile_h)) != RT_OK) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stats) return rt_ctx_stats(c, stats);
    return check_join_error(c);
}

// rt_ctx_reserve: render_device's allocations and streams without its launches (dry), plus, for
// rt_render (host), the device frame, the staging slices and the sparse copies' pinned buffers.
int reserve(rt_ctx* c, const rt_render_opts* o, int host, void* stream) {
    if (!c->has_scene) return fail(c, RT_E_NOSCENE, "no scene uploaded");
    if (!host) {
        RenderReq req;
        req.dry = true;
        return render_device(c, o, nullptr, nullptr, stream, req);
    }
    const bool rgb = (o->flags & RT_OUT_RGB_F32) != 0, bgr = (o->flags & RT_OUT_BGR_U8) != 0;
    HostRender h;
    int rc = host_request(c, o, rgb, bgr, true, h);
    if (rc != RT_OK) return rc;
    if ((rc = render_device(c, &h.oo, c->d_rgb, c->d_bgr, nullptr, h.req)) != RT_OK) return rc;
    for (int i = 0; i < kRing; ++i) {               // the staging slices of pageable destinations
        if (!c->pin[i]) HIP_TRY(c, hipHostMalloc(&c->pin[i], c->pin_cap, hipHostMallocDefault));
        if (!c->pin_ev[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
    }
    if (c->sparse_on) {
        const uint64_t nseg = (o->tile_w + kSegPx - 1) / kSegPx, words = (nseg + 31) / 32;
        if ((rc = ensure_pinned(c, c->h_sp_meta, c->h_sp_meta_cap, (o->tile_h + 1ull) * 4 + o->tile_h * words * 4)) != RT_OK)
            return rc;
        // the packed segments' pinned buffer at its worst case (every segment flagged), up to 1 GB;
        // a render that needs more grows it
        const uint64_t worst = nseg * o->tile_h * 3 * kSegPx * ((bgr ? 1 : 0) + (rgb ? 4 : 0));
        if ((rc = ensure_pinned(c, c->h_sp_pk, c->h_sp_pk_cap, std::max<uint64_t>(1, std::min<uint64_t>(worst, 1ull << 30)))) != RT_OK)
            return rc;
        for (int j = 0; j < rt_ctx::kSpRanges; ++j)
            if (!c->sp_ev[j]) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_ev[j], hipEventDisableTiming));
    }
    // the copy engine's queue is set up at its first copy (tens of ms): one small copy now
    if (const uint32_t engine = sdma_engine(c, h.req)) {
        constexpr int si = rt_ctx::kSdmaSignals - 1;
        if ((rc = sdma_copy(c, engine, si, c->pin[0], c->d_counters, 4096)) != RT_OK || (rc = sdma_wait(c, si)) != RT_OK)
            return rc;
    }
    return RT_OK;
}

}  // namespace

namespace rtamd {

int warm_streams(rt_ctx* c, const std::vector<hipStream_t>& ss) {
    for (hipStream_t s : ss) {
        if (!s) continue;
        HIP_TRY(c, launch_warmup(static_cast<uint32_t>(2 * c->n_cu), s));
        HIP_TRY(c, launch_path_warmup(s));
    }
    for (hipStream_t s : ss)
        if (s) HIP_TRY(c, hipStreamSynchronize(s));
    return RT_OK;
}

int render_accumulate(rt_ctx* c, const rt_render_opts* o, double* sums, uint32_t first, uint32_t n, void* stream, bool moments) {
    RenderReq req;
    req.accumulate = true;
    req.acc = sums;
    req.acc_first = first;
    req.acc_n = n;
    req.acc_moments = moments;
    return render_device(c, o, nullptr, nullptr, stream, req);
}

// rt_render_aov / rt_render_aov_device behind their argument checks (rt_aov.cpp): a render of the context like
// every other (begin_render: the geometry checks rt_render makes, the stream's wait for the previous render;
// end_render), one launch of aov_primary from the source the planner names.  The fields an AOV render ignores
// (max_depth, algo, bgr_pitch, flags but RT_TIME_KERNELS) do not reach the checks.
int render_aov(rt_ctx* c, const rt_render_opts* o, const AovOut& out, uint32_t channels, void* stream) {
    rt_render_opts b = *o;
    b.max_depth = 0; b.algo = RT_ALGO_AUTO; b.bgr_pitch = 0; b.flags = 0;
    RenderCall rcall;
    if (const int rc = begin_render(c, &b, nullptr, nullptr, stream, rcall); rc != RT_OK) return rc;
    const hipStream_t st = rcall.st;
    const AovSource as = plan_aov_source(scene_facts(c), c->tune);
    c->dsc.pfx2 = as.pfx2;
    const uint64_t npix = static_cast<uint64_t>(o->tile_w) * o->tile_h;
    c->tally.on = false;
    c->last_pixels = npix;
    c->last_stream = st;
    // centre jitter: one of the spp identical samples is traced and counted spp times
    c->last_spp_traced = o->jitter == RT_JITTER_CENTER ? rcall.spp : 1;
    c->last_chunks = 0;
    c->n_bands = 0;
    c->sparse_on = false;
    if (const int rc = zero_counters(c, st); rc != RT_OK) return rc;
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: aov src %d spp %u channels 0x%x pixels %llu\n", as.src, rcall.spp, channels,
                     static_cast<unsigned long long>(npix));
    c->ev0_set = true;
    HIP_TRY(c, hipEventRecord(c->ev0, st));
    if (npix) {
        const bool timed = (o->flags & RT_TIME_KERNELS) != 0;
        LaunchMarks m;
        m.pool = &c->tev; m.used = &c->t_used; m.out = &c->tint;
        if (timed) HIP_TRY(c, m.begin(st));
        HIP_TRY(c, launch_aov(c->dsc, rcall.fp, out, as.src, plan_aov_workgroups(npix, c->n_cu), st));
        if (timed) HIP_TRY(c, m.mark(st, kKfCamera));
    }
    return end_render(c, st, true);
}

// rt_query_nearest / rt_query_occluded behind their argument checks (rt_query.cpp): a render of the context like
// every other (the stream's wait for the previous render, as begin_render makes it: a query has no tile geometry
// for that function to check; end_render), one launch of query_nearest or query_occluded from the source the
// planner names.  No tile, no pixels, no working set: rays = traced_rays = n.
int render_query(rt_ctx* c, const QueryCall& q, void* stream) {
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (c->render_pending && st != c->done_stream) HIP_TRY(c, hipStreamWaitEvent(st, c->render_done, 0));
    const SceneFacts sf = scene_facts(c);
    const QuerySource qs = q.occlusion ? plan_query_occ_source(sf, c->tune) : plan_query_source(sf, c->tune);
    c->dsc.pfx2 = qs.pfx2;
    c->tally.on = false;
    c->last_pixels = 0;
    c->last_stream = st;
    c->last_spp_traced = 1;
    c->last_chunks = 0;
    c->n_bands = 0;
    c->sparse_on = false;
    if (const int rc = zero_counters(c, st); rc != RT_OK) return rc;
    const uint32_t wgs = plan_query_workgroups(q.n, c->n_cu);
    if (c->t(kTuneVerbose)) {
        if (q.occlusion)
            std::fprintf(stderr, "rtamd: query occluded src %d rays %u range %d workgroups %u\n", qs.src, q.n, q.ranged ? 1 : 0,
                         q.n ? wgs : 0u);
        else
            std::fprintf(stderr, "rtamd: query nearest src %d rays %u channels 0x%x workgroups %u\n", qs.src, q.n, q.channels,
                         q.n ? wgs : 0u);
    }
    c->ev0_set = true;
    HIP_TRY(c, hipEventRecord(c->ev0, st));
    if (q.n) {
        const bool timed = (q.flags & RT_TIME_KERNELS) != 0;
        LaunchMarks m;
        m.pool = &c->tev; m.used = &c->t_used; m.out = &c->tint;
        if (timed) HIP_TRY(c, m.begin(st));
        if (q.occlusion) HIP_TRY(c, launch_query_occluded(c->dsc, c->d_counters, q.rays, q.r2, q.n, q.occluded, qs.src, wgs, st));
        else HIP_TRY(c, launch_query_nearest(c->dsc, c->d_counters, q.rays, q.n, q.out, qs.src, wgs, st));
        if (timed) HIP_TRY(c, m.mark(st, q.occlusion ? kKfOcclusion : kKfNearest));
    }
    return end_render(c, st, true);
}

void drop_lanes(rt_ctx* c) {
    for (auto& L : c->lanes) {
        release_lane_memory(c, L);
        if (L.mark) (void)hipEventDestroy(L.mark);
        if (L.done) (void)hipEventDestroy(L.done);
        for (hipEvent_t e : L.b_done) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : L.near_done) if (e) (void)hipEventDestroy(e);
        if (L.s) (void)hipStreamDestroy(L.s);
        for (hipStream_t x : L.sb) if (x) (void)hipStreamDestroy(x);
        if (L.dj) (void)hipFree(L.dj);
        if (L.dj_err) (void)hipHostFree(L.dj_err);
    }
    c->lanes.clear();
}

// A device-side join that gave up (wf_join's 2 s limit) since the last check: reported once (the
// error word is cleared), by the rt_render whose synchronisation follows it or by rt_ctx_stats.
// Only contexts whose renders joined on the device have anything to read (c->dj_used).
int check_join_error(rt_ctx* c) {
    if (!c->dj_used) return RT_OK;
    for (auto& L : c->lanes) {
        if (!L.dj_err || !__atomic_load_n(L.dj_err, __ATOMIC_ACQUIRE)) continue;
        __atomic_store_n(L.dj_err, 0ull, __ATOMIC_RELEASE);
        return fail(c, RT_E_HIP, "a device-side stream join timed out (tuning dev_join): the render's results are not valid");
    }
    return RT_OK;
}

}  // namespace rtamd

extern "C" {

int rt_render_device(rt_ctx* c, const rt_render_opts* o, void* d_rgb, void* d_bgr, void* stream) {
    if (!c) return RT_E_INVALID;
    RenderReq req;
    req.skip_ev0 = o && !(o->flags & (RT_TIME_KERNELS | RT_COUNT_WORK));
    return guarded(c, [&] { return render_device(c, o, d_rgb, d_bgr, stream, req); });
}

int rt_render(rt_ctx* c, const rt_render_opts* o, float* out_rgb, uint8_t* out_bgr, rt_stats* stats) {
    if (!c || !o) return RT_E_INVALID;
    return guarded(c, [&] { return render_host(c, o, out_rgb, out_bgr, stats); });
}

int rt_ctx_reserve(rt_ctx* c, const rt_render_opts* o, int host, void* stream) {
    if (!c || !o) return RT_E_INVALID;
    return guarded(c, [&] { return reserve(c, o, host, stream); });
}

int rt_ctx_stats(rt_ctx* c, rt_stats* s) {
    if (!c || !s) return RT_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = flush_tally(c); rc != RT_OK) return rc;
    unsigned long long h[kCounterWords];
    if (c->last_stream) HIP_TRY(c, hipStreamSynchronize(c->last_stream));
    HIP_TRY(c, hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memset(s, 0, sizeof *s);
    for (int i = 0; i < kCounterShards; ++i) { s->rays += h[i]; s->shadow_rays += h[kCounterShards + i]; }
    s->rays += h[kTotals] + h[kTotals + 1];
    s->shadow_rays += h[kTotals + 1];
    s->box_tests = h[kTotals + 2] + h[kTotals + 4];
    s->sphere_tests = h[kTotals + 3] + h[kTotals + 5];
    s->shadow_box_tests = h[kTotals + 4];
    s->shadow_sphere_tests = h[kTotals + 5];
    s->pixels = c->last_pixels;
    s->traced_rays = c->last_spp_traced > 1 ? s->rays / c->last_spp_traced : s->rays;
    s->chunks = c->last_chunks;
    if (const int rc = check_join_error(c); rc != RT_OK) return rc;
    if (c->last_timed && c->ev0_set) {
        float ms = 0.f;
        HIP_TRY(c, hipEventSynchronize(c->render_done));
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->render_done));
        s->kernel_ms = ms;
    }
    return RT_OK;
}

int rt_ctx_generation_counts(rt_ctx* c, uint32_t* queue, uint32_t* shaded, int n) {
    if (!c || n < 0 || (n && (!queue || !shaded))) return RT_E_INVALID;
    if (!c->wf_used) return fail(c, RT_E_NOSCENE, "no wavefront render yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = flush_tally(c); rc != RT_OK) return rc;
    if (c->last_stream) HIP_TRY(c, hipStreamSynchronize(c->last_stream));
    unsigned long long h[kCntWords];
    HIP_TRY(c, hipMemcpyAsync(h, c->d_counters + kGenTotals, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < n && k < kCntS; ++k) {
        queue[k] = static_cast<uint32_t>(h[kCntQ + k]);
        shaded[k] = static_cast<uint32_t>(h[kCntS + k]);
    }
    return RT_OK;
}

int rt_ctx_kernel_times(rt_ctx* c, double* ms, uint32_t* launches, int n) {
    if (!c || n < 0 || (n && (!ms || !launches))) return RT_E_INVALID;
    for (int i = 0; i < n; ++i) { ms[i] = 0.0; launches[i] = 0; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->t_used > 0) HIP_TRY(c, hipEventSynchronize(c->tev[c->t_used - 1]));
    for (const LaunchInterval& iv : c->tint) {
        float e = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&e, c->tev[iv.start], c->tev[iv.end]));
        if (iv.fam < n) { ms[iv.fam] += e; ++launches[iv.fam]; }
    }
    c->tint.clear();
    c->t_used = 0;
    return RT_OK;
}

}  // extern "C"
