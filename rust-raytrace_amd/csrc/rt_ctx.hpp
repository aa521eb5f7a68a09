// The device context behind the C ABI (include/raytrace_amd.h), its error helpers, and what the
// translation units that implement it share: rt_device.cpp (create / destroy, tuning, probes),
// rt_scene_upload.cpp, rt_render.cpp (the render path, lanes, reserve, statistics), rt_accum.cpp
// (progressive rendering: the accumulator and its calls), rt_aov.cpp (first-hit feature buffers: the entry
// points' checks and the host variant), rt_query.cpp (ray queries: the same), rt_denoise.cpp (the denoiser: checks,
// scratch, passes, host variant) and rt_copy.cpp (device -> host copies).
#pragma once

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_layout.hpp"
#include "host_copy_pool.hpp"
#include "host_scene.hpp"
#include "launch_api.hpp"
#include "render_plan.hpp"
#include "tuning.hpp"

namespace rtamd {

constexpr int kMaxBands = 16;           // row bands of one rt_render copied as they finish
constexpr int kRing = 4;                // pinned staging slices in flight
constexpr size_t kSlice = 8u << 20;     // bytes per staging slice

// What one render was asked for beyond its rt_render_opts, by the entry point that issued it;
// passed by value down the render and copy functions.
struct RenderReq {
    bool bands = false;        // rt_render: fold in bands, an event after each (the copy of a band overlaps the rest)
    bool sparse = false;       // rt_render with tuning sparse_out: mark the chain pixels and pack them
    // rt_render_device without RT_TIME_KERNELS / RT_COUNT_WORK: no ev0 (rt_stats.kernel_ms 0): the
    // marker between consecutive renders on the caller's stream cost ~4-6 us of device time per
    // frame (8-way C3 share 0.655-0.656 vs 0.659-0.662 ms, C3 2.800 vs 2.812 ms, same box)
    bool skip_ev0 = false;
    bool banded_copy = false;  // rt_render writes a row-banded tile (copy_engine -2)
    // rt_render: the device frame is the context's, and its rows are copied to the host whole: their
    // padding (bgr_pitch > 3 * tile_w) is written as zero (main.rs:42).  rt_render_device writes
    // pixels only: the rest of a caller's rows is the caller's
    bool zero_pad = false;
    // rt_ctx_reserve: every allocation and stream the render would make, then warm_streams
    // instead of the launches; counters and the last render's statistics are left alone
    bool dry = false;
    // rt_render_accumulate: the render adds samples [acc_first, acc_first + acc_n) of every tile pixel to the running
    // sums at acc (3 f64 per tile pixel, tile row-major) and writes no pixel (render_plan.hpp, plan_accumulate)
    bool accumulate = false;
    double* acc = nullptr;             // (null: an empty tile)
    uint32_t acc_first = 0, acc_n = 0;
    bool acc_moments = false;          // a moments accumulator: the squares' plane follows the tile's sums (kAaMoments)
};

}  // namespace rtamd

// Progressive rendering (include/raytrace_amd.h): the running sums of one tile on the device and what they
// are bound to.  Owned by the caller; its device memory by the context, which frees it when it is destroyed
// first (ctx becomes null: only rt_accum_destroy is valid then).
struct rt_accum {
    rt_ctx* ctx = nullptr;
    rt_render_opts o{};                // the bound options; spp, flags, algo and bgr_pitch are zero
    uint64_t scene_gen = 0;            // rt_ctx::scene_gen at create / reset
    double* d_sums = nullptr;          // 3 * npix f64, tile row-major (null: an empty tile)
    uint64_t npix = 0;
    uint32_t samples = 0;
    bool moments = false;              // rt_accum_create_moments: d_sums holds 6 * npix doubles, the sums and then the
                                       //   plane of the sums of squares
    unsigned long long* d_above = nullptr;   // rt_accum_noise's counter (allocated with a moments accumulator)
    unsigned long long* h_above = nullptr;   // ... and where its value lands on the host (page-locked, the accumulator's)
    bool timed = false;                // the last accumulate had RT_TIME_KERNELS: a resolve is timed too
    // a device resolve reads the sums on a caller's stream: the next accumulate (which writes them) waits for it
    hipEvent_t read_done = nullptr;
    bool read_pending = false;
};

struct rt_ctx {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr;             // start of the last render (its end: render_done, also a timing event)
    void* d_blob = nullptr;
    size_t blob_bytes = 0;
    rtamd::DevScene dsc{};
    bool has_scene = false;
    uint64_t scene_gen = 0;          // counts rt_scene_upload calls: what an rt_accum is bound to
    std::vector<rt_accum*> accums;   // the accumulators alive on this context (rt_accum.cpp)
    bool deep_bvh4 = false;          // the 4-wide tree could overflow the traversal stack: binary tree only
    bool short_stack = false;        // binary tree fits the compact nearest-hit stack (16-bit codes, depth <= 32)
    bool short_stack18 = false;      // ... with 18-bit codes (the binary16 prefix source, src 6)
    bool q4_ok = false;              // the quantised 4-wide tree was built (DevScene::q4)
    bool all_lights_gridded = false; // every light is a point light with a light-view grid
    unsigned long long* d_counters = nullptr;
    double* d_srgb = nullptr;         // the 255 sRGB thresholds (path kernel)
    void* d_path = nullptr;           // path kernel recursion stack (PathStack)
    size_t path_bytes = 0;
    float* d_rgb = nullptr;
    size_t rgb_cap = 0;
    uint8_t* d_bgr = nullptr;
    size_t bgr_cap = 0;
    uint64_t last_pixels = 0;
    bool last_timed = false;
    bool ev0_set = true;                   // ev0 was recorded at the start of the last render
    hipStream_t last_stream = nullptr;
    // Wavefront lanes: each owns a stream and a working set (grown on demand,
    // kept across renders).  Row chunks of a render are dealt round-robin over
    // the lanes; chunk c+1 starts once chunk c has passed its bulk generations,
    // so its big launches overlap chunk c's latency-bound tail.
    struct Lane {
        hipStream_t s = nullptr;
        std::vector<hipStream_t> sb;       // shadow + shading kernels of the generations
        hipEvent_t mark = nullptr, done = nullptr;
        std::vector<hipEvent_t> b_done;    // one per sb stream
        std::vector<hipEvent_t> near_done; // per generation: nearest-hit kernel finished (s -> sb)
        void* mem = nullptr;
        size_t bytes = 0;
        rtamd::WfBufs b{};
        double* acc = nullptr;             // RT_ALGO_WAVEFRONT_AA: the chunk pixels' running sums, in mem (else null)
        uint64_t* dj = nullptr;            // device-side join flags (kDjWords words, zeroed once)
        uint64_t dj_n = 0;                 // the last join number handed out on them
        uint64_t* dj_err = nullptr;        // page-locked: a join gave up (host address; dj_err_dev the device's)
        uint64_t* dj_err_dev = nullptr;
    };
    std::vector<Lane> lanes;
    // RT_TIME_KERNELS: launch intervals accumulated since the last harvest
    std::vector<hipEvent_t> tev;
    int t_used = 0;
    std::vector<rtamd::LaunchInterval> tint;
    hipEvent_t fork = nullptr;
    bool wf_used = false;
    // a one-chunk wavefront render leaves its tally (ray counts, per-generation queue sizes) to
    // the first rt_ctx_stats / rt_ctx_generation_counts after it (flush_tally): not on the chain.
    // It points into a lane's working set: release_lane_memory settles it before that is freed.
    struct PendingTally {
        bool on = false;
        bool zero = false;                 // the render left the counters to be cleared before the tally
        rtamd::FrameParams fp{};
        rtamd::WfBufs b{};
        int n_lights = 0, gens = 0;
    } tally;
    uint32_t scene_spp = 1;           // the uploaded scene's Options.antialias (rt_render_opts.spp = 0)
    hipEvent_t render_done = nullptr; // end of the last render on its stream: the next one waits for it
    bool render_pending = false;
    hipStream_t done_stream = nullptr;     // the stream render_done was recorded on
    uint32_t last_spp_traced = 1;     // chain schedules trace one of spp identical centre-jitter samples
    uint32_t last_chunks = 0;         // wavefront chunks of the last render (0: other schedules)
    // rt_render: pinned staging slices for the device -> host copy of the outputs, a copy
    // stream that waits for each finished row band, and the host threads that empty the slices
    void* pin[rtamd::kRing] = {};
    size_t pin_cap = rtamd::kSlice;        // bytes per staging slice (larger for rows wider than kSlice)
    hipEvent_t pin_ev[rtamd::kRing] = {};
    hipStream_t copy_stream = nullptr;
    int n_bands = 0;                       // bands of the last render (0: copy after render_done)
    hipEvent_t band_ev[rtamd::kMaxBands] = {};
    uint32_t band_row0[rtamd::kMaxBands] = {}, band_nrows[rtamd::kMaxBands] = {};
    rtamd::HostCopyPool pool;
    // sparse host copies (tuning sparse_out): device segment bits / row counts /
    // row offsets / packed BGR / packed RGB, the pinned host copies of the first three and of the
    // packed segments, and an event per piece of the packed copy
    bool sparse_on = false;                // the last render marked its chain pixels and packed them
    void* d_sp = nullptr;
    size_t sp_cap = 0;
    uint32_t* d_sp_bits = nullptr, *d_sp_cnt = nullptr, *d_sp_off = nullptr;
    uint8_t* d_sp_bgr = nullptr;
    float* d_sp_rgb = nullptr;
    void* h_sp_meta = nullptr;
    size_t h_sp_meta_cap = 0;
    void* h_sp_pk = nullptr;
    size_t h_sp_pk_cap = 0;
    hipEvent_t sp_cam = nullptr, sp_ready = nullptr, cp_done = nullptr;
    static constexpr int kSpRanges = 16;   // row ranges of the packed copy, each scattered as it lands
    hipEvent_t sp_ev[kSpRanges] = {};
    // copies on an SDMA engine (tuning copy_engine): the device's and a CPU agent, the engine, and
    // one completion signal per staging slice / packed range / direct copy batch
    int sdma_state = 0;                    // 0 not set up, 1 usable, -1 unavailable
    bool dj_used = false;                  // a render joined its streams on the device (check_join_error)
    hsa_agent_t hsa_gpu{}, hsa_cpu{};
    uint32_t sdma_avail = 0, sdma_pref = 0, sdma_turn = 0;
    static constexpr int kSdmaSignals = rtamd::kRing + kSpRanges + 1;
    hsa_signal_t sdma_sig[kSdmaSignals] = {};
    // the denoiser's scratch (rt_denoise.cpp): two colour images and one guide image, grown on demand; dn_done: the
    // end of the last denoise on its stream, which the next one waits for (the scratch is shared)
    void* d_dn = nullptr;
    size_t dn_cap = 0;
    hipEvent_t dn_done = nullptr;
    bool dn_pending = false;
    int64_t tune[rtamd::kTuneCount];
    std::string err;
    rt_ctx() {
        for (int i = 0; i < rtamd::kTuneCount; ++i) tune[i] = rtamd::kTune[i].dflt;
        // a device-side join spins while the b streams finish: it needs their kernels to run beside
        // it, which kernel serialisation (rocprofv3 --pmc, AMD_SERIALIZE_KERNEL) does not allow (the
        // join would wait out its 2 s limit): joins through events there
        auto on = [](const char* v) { return v && *v && std::strcmp(v, "0") != 0 && strcasecmp(v, "false") != 0; };
        if (on(std::getenv("ROCPROF_COUNTER_COLLECTION")) || on(std::getenv("AMD_SERIALIZE_KERNEL")))
            tune[rtamd::kTuneDevJoin] = 0;
    }
    int64_t t(rtamd::TuneKey k) const { return tune[k]; }
};

namespace rtamd {

// What the scene upload derives on the host with the reference's own f64 operations, so that the
// device reads the same bits (rt_scene_upload.cpp; the probes of rt_device.cpp form them the same way).
inline double significance(const rt_color& c) { return c.r + c.g + c.b; }   // color.rs:637-639
inline double sphere_rr(double radius) { return radius * radius; }          // shapes.rs:65, DevSphere::rr

inline int fail(rt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    set_thread_error(msg);
    return code;
}

inline int hip_fail(rt_ctx* c, hipError_t e, const char* what) {
    return fail(c, RT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(c, expr)                                                     \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) return ::rtamd::hip_fail((c), _e, #expr);      \
    } while (0)

// No C++ exception crosses the ABI: allocation failures become RT_E_NOMEM.
template <class F>
int guarded(rt_ctx* c, F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(c, RT_E_NOMEM, "host allocation failed");
    } catch (const std::exception& e) {
        return fail(c, RT_E_INVALID, e.what());
    } catch (...) {
        return fail(c, RT_E_INVALID, "unexpected exception");
    }
}

// counters: [0, 256) rays per shard (megakernel), [256, 512) shadow rays per
// shard, [512, 520) wavefront totals (see WfBufs::totals), [520, 520 + kCntWords)
// per-generation queue sizes summed over chunks
constexpr int kTotals = 2 * kCounterShards;
constexpr int kGenTotals = kTotals + 8;
constexpr int kCounterWords = kGenTotals + kCntWords;
constexpr uint64_t kWfBudget = 80ull << 30;     // default wavefront working set per lane (of 288 GB HBM)
// device memory a working set must leave free: the runtime's per-queue scratch
// (up to 32 waves x 256 CUs x 64 lanes x ~600 B per queue, for several queues)
constexpr size_t kRuntimeHeadroom = 4ull << 30;

// ---- rt_render.cpp ------------------------------------------------------------------------
// A no-op launch with private memory on every stream of `ss` (the code objects load, each
// hardware queue and its scratch are set up), then wait for them.
int warm_streams(rt_ctx* c, const std::vector<hipStream_t>& ss);
// Free every lane (streams, events, working set) once its work is done; a pending tally is
// settled first (release_lane_memory).
void drop_lanes(rt_ctx* c);
int check_join_error(rt_ctx* c);
// rt_render_accumulate behind its argument checks: one render of o's tile (o: the accumulator's bound options
// with the call's algo and flags) that adds samples [first, first + n) to `sums`.  n == 0: the checks only.
// moments: `sums` is a moments accumulator's (6 f64 per tile pixel: the sums, then the plane of the sums of squares).
int render_accumulate(rt_ctx* c, const rt_render_opts* o, double* sums, uint32_t first, uint32_t n, void* stream,
                      bool moments = false);

// rt_render_aov behind its argument checks: one render of o's tile into the selected device buffers of `out`
// (channels: the rt_aov mask, for the verbose line) on `stream` (null: the context's own).
int render_aov(rt_ctx* c, const rt_render_opts* o, const AovOut& out, uint32_t channels, void* stream);

// rt_query_nearest / rt_query_occluded behind their argument checks: one render of n rays (device memory, 16-byte
// aligned) into the selected device buffers on `stream` (null: the context's own).  n == 0: a render that launches
// nothing.
struct QueryCall {
    bool occlusion = false;
    const double* rays = nullptr;
    const double* r2 = nullptr;        // occlusion: the squared ranges, or null (no range)
    bool ranged = false;               // occlusion: the caller gave ranges (r2 itself stays null for an empty batch)
    uint32_t n = 0, channels = 0, flags = 0;
    QueryOut out{};                    // nearest: the selected channels (the others null)
    uint8_t* occluded = nullptr;
};
int render_query(rt_ctx* c, const QueryCall& q, void* stream);

// ---- rt_accum.cpp -------------------------------------------------------------------------
// rt_ctx_destroy: free the device memory of the accumulators still alive and detach them.
void orphan_accums(rt_ctx* c);

// ---- rt_copy.cpp --------------------------------------------------------------------------
// Where rt_render puts a device row (RT_OUT_FRAME_ROWS or not): local row j of the tile, dev_pitch
// bytes apart on the device, row_bytes of it copied, lands at host byte offset host_row(j) *
// host_pitch + host_x.  A plain tile: host_row(j) = j, the host rows laid out as the device's; a
// frame: the tile's frame row (rt_render_opts: y0 + ((j/band)*band_stride + band_phase)*band + j%band).
struct OutMap {
    size_t dev_pitch = 0, row_bytes = 0, host_pitch = 0, host_x = 0;
    bool frame = false;
    uint32_t y0 = 0, band = 1, stride = 1, phase = 0;
    size_t host_row(uint32_t j) const {
        return frame ? y0 + (static_cast<size_t>(j / band) * stride + phase) * band + j % band : j;
    }
    size_t host_off(uint32_t j) const { return host_row(j) * host_pitch + host_x; }
    // consecutive rows are one contiguous byte range on both sides
    bool contiguous() const { return dev_pitch == host_pitch && row_bytes == dev_pitch && host_x == 0; }
    // local rows j and j + 1 sit in consecutive host rows
    bool next_row(uint32_t j) const { return host_row(j + 1) == host_row(j) + 1; }
};
int ensure_copy_stream(rt_ctx* c);
int ensure_sparse(rt_ctx* c, hipStream_t st, uint32_t tw, uint32_t rows, bool bgr, bool rgb, bool* ok);
int ensure_pinned(rt_ctx* c, void*& p, size_t& cap, size_t bytes);
int ensure_host_frame(rt_ctx* c, size_t rgb_bytes, size_t bgr_bytes);
int host_layout(rt_ctx* c, const rt_render_opts* o, uint32_t pitch, OutMap& mr, OutMap& mb, uint32_t* dev_bgr_pitch);
uint32_t sdma_engine(rt_ctx* c, RenderReq req);
int sdma_wait(rt_ctx* c, int si);
int sdma_copy(rt_ctx* c, uint32_t engines, int si, void* dst, const void* src, size_t bytes);
int copy_to_host(rt_ctx* c, RenderReq req, void* dst, const void* src, const OutMap& m, uint32_t rows,
                 hipEvent_t after = nullptr, bool sync = true);
int copy_sparse(rt_ctx* c, RenderReq req, const rt_render_opts* o, float* out_rgb, uint8_t* out_bgr, const OutMap& mr,
                const OutMap& mb);

}  // namespace rtamd
