// CPU check of the render planner (csrc/render_plan.cpp alone: no HIP, no GPU).  The expected
// values were derived by hand from the expressions the planner was lifted from.
#include <cstdint>
#include <cstdio>

#include "render_plan.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

struct Tune {
    int64_t v[kTuneCount];
    Tune() {
        for (int i = 0; i < kTuneCount; ++i) v[i] = kTune[i].dflt;
    }
    Tune& set(TuneKey k, int64_t x) { v[k] = x; return *this; }
};

constexpr int kCus = 256;
constexpr uint64_t kNoCap = uint64_t{1} << 40;

static void chunk_cases() {
    {   // one chunk
        Tune t;
        const ChunkPlan c = plan_chunks(t.v, kNoCap, 64, 64, false);
        const RegionPlan r = plan_regions(t.v, kCus, c);
        CHECK(c.chunk_rows == 64 && c.n_chunks == 1 && c.first_rows == 0 && c.n_lanes == 1);
        CHECK(c.row0(0) == 0 && c.nrows(0) == 64 && c.cap() == 64 * 64);
        CHECK(r.slots == 4096 && r.G == 4 && r.R == 1024);
    }
    {   // many small chunks
        Tune t;
        t.set(kTuneChunkPixels, 1000);
        const uint64_t cap_px = plan_cap_px(t.v, 0, 9);
        CHECK(cap_px == 1000);
        const ChunkPlan c = plan_chunks(t.v, cap_px, 100, 50, false);
        const RegionPlan r = plan_regions(t.v, kCus, c);
        CHECK(c.n_chunks == 7 && c.chunk_rows == 8 && c.tiles_x == 13 && c.n_lanes == 1);
        for (uint32_t i = 0; i < 6; ++i) CHECK(c.row0(i) == 8 * i && c.nrows(i) == 8);
        CHECK(c.row0(6) == 48 && c.nrows(6) == 2);
        CHECK(r.slots == 832 && r.G == 1 && r.R == 1024);
        t.set(kTuneLanes, 2);
        CHECK(plan_chunks(t.v, cap_px, 100, 50, false).n_lanes == 2);
        CHECK(plan_chunks(t.v, kNoCap, 100, 50, false).n_lanes == 1);      // never more lanes than chunks
    }
    {   // balanced split: 40 + 32 rows, not 64 + 8
        Tune t;
        const ChunkPlan c = plan_chunks(t.v, 4096, 64, 72, false);
        CHECK(c.n_chunks == 2 && c.chunk_rows == 40);
        CHECK(c.row0(0) == 0 && c.nrows(0) == 40 && c.row0(1) == 40 && c.nrows(1) == 32);
        CHECK(c.next_cap_px() == 40 * 64 / 2);
    }
    {   // host chunks (rt_render into host memory only)
        Tune t;
        t.set(kTuneHostChunks, 4);
        const ChunkPlan c = plan_chunks(t.v, kNoCap, 64, 64, true);
        CHECK(c.n_chunks == 4 && c.chunk_rows == 16 && c.first_rows == 0);
        for (uint32_t i = 0; i < 4; ++i) CHECK(c.row0(i) == 16 * i && c.nrows(i) == 16);
        CHECK(plan_chunks(t.v, kNoCap, 64, 64, false).n_chunks == 1);
    }
    {   // host first
        Tune t;
        t.set(kTuneHostChunks, 2).set(kTuneHostFirst, 25);
        const ChunkPlan c = plan_chunks(t.v, kNoCap, 64, 64, true);
        CHECK(c.first_rows == 16 && c.n_chunks == 2 && c.chunk_rows == 48);
        CHECK(c.row0(0) == 0 && c.nrows(0) == 16 && c.row0(1) == 16 && c.nrows(1) == 48);
        // the retry after an allocation failure gives the uneven split up
        const ChunkPlan d = plan_chunks(t.v, c.next_cap_px(), 64, 64, true);
        CHECK(d.first_rows == 0 && d.chunk_rows == 24 && d.n_chunks == 3);
    }
    {   // the default cap: the budget over the lanes and the bytes per slot
        Tune t;
        CHECK(plan_cap_px(t.v, 1149 * 1000, 9) == 1000);
        t.set(kTuneLanes, 2);
        CHECK(plan_cap_px(t.v, 1149 * 1000, 9) == 500);
        CHECK(plan_cap_px(t.v, 0, 9) == 1);
    }
    CHECK(wf_bytes_per_slot(9) == 1149);
    CHECK(wf_bytes_per_slot(1) == 285);
    for (uint64_t l = 1; l <= 32; ++l) CHECK(wf_bytes_per_slot(l) == 177 + 108 * l);
}

static void layout_cases() {
    const struct { uint32_t cap, G, R, levels; } cases[] = {
        {64 * 64, 4, 1024, 9}, {800, 1, 1024, 1}, {100 * 8, 1, 1024, 17}, {2560 * 1440, 512, 8192, 9},
        {4096u * 4096u, 512, 32768, 31}, {1, 1, 1024, 5}, {123457, 121, 1024, 4},
    };
    for (const auto& k : cases) {
        const WfLayout w = wf_layout(k.cap, k.G, k.R, k.levels);
        CHECK(w.qcap == static_cast<uint64_t>(k.G) * k.R);
        CHECK(w.capa >= w.qcap && w.capa % 64 == 0 && w.capa < w.qcap + 64);
        const uint64_t off[] = {w.o_rec, w.o_lev, w.o_term, w.o_rq, w.o_rs, w.o_cpix, w.o_pmap, w.o_ccol, w.total};
        const uint64_t size[] = {w.s_queue, w.s_rec, w.s_lev, w.s_term, w.s_reg, w.s_reg, w.s_cpix, w.s_pmap, w.s_ccol};
        uint64_t prev = 0;      // the queues start at 0
        for (int i = 0; i < 9; ++i) {
            CHECK(off[i] % 256 == 0);
            CHECK(off[i] > prev || (i == 0 && off[i] > 0));
            CHECK(off[i] >= prev + size[i] && off[i] < prev + size[i] + 256);   // each section holds its size, no more padding
            prev = off[i];
        }
        CHECK(w.total >= w.qcap * (wf_bytes_per_slot(k.levels) - kWfPmapBytes));
        CHECK(w.s_pmap == 4ull * k.cap);
    }
}

static SceneFacts small_scene() {     // both trees and the spheres fit the LDS budget
    SceneFacts f;
    f.n_spheres = 100; f.n_bvh = 99; f.n_bvh4 = 40; f.n_lights = 2;
    f.short_stack = f.short_stack18 = true;
    return f;
}
static SceneFacts big_scene() {       // trees beyond LDS
    SceneFacts f;
    f.n_spheres = 10000; f.n_bvh = 9999; f.n_bvh4 = 4000; f.n_lights = 2;
    return f;
}

static void source_cases() {
    const int W = RT_ALGO_WAVEFRONT;
    {
        Tune t;
        const SceneFacts f = small_scene();
        const SourcePair p = plan_sources(f, t.v, W);
        CHECK(p.src == 9 && p.src_occ == 10);
        CHECK(p.sets_prefix && p.pfx2 == 1024 && p.pfxq == 1365);
        CHECK(plan_streams(f, t.v, W, p.src, 8).split);
        t.set(kTuneCompact, 0);
        const SourcePair q = plan_sources(f, t.v, W);
        CHECK(q.src == 7 && q.src_occ == 10);
    }
    {
        Tune t;
        SceneFacts f = big_scene();
        f.has_half = true;
        f.short_stack18 = true;
        SourcePair p = plan_sources(f, t.v, W);
        CHECK(p.src == 6 && p.src_occ == 11);
        CHECK(!plan_streams(f, t.v, W, p.src, 8).split);
        f.short_stack18 = false;
        p = plan_sources(f, t.v, W);
        CHECK(p.src == 5 && p.src_occ == 11);
        f.has_half = false;
        p = plan_sources(f, t.v, W);
        CHECK(p.src == 8 && p.src_occ == 11);
    }
    {
        Tune t;
        SceneFacts f = small_scene();
        f.deep_bvh4 = true;
        SourcePair p = plan_sources(f, t.v, W);
        CHECK(p.src == 7 && p.src_occ == 7);
        f = big_scene();
        f.deep_bvh4 = true;
        p = plan_sources(f, t.v, W);
        CHECK(p.src == 2 && p.src_occ == 2);
    }
    {   // a forced source the scene cannot serve: the binary tree through L2
        Tune t;
        t.set(kTuneSrc, 25);
        const SourcePair p = plan_sources(small_scene(), t.v, W);
        CHECK(p.src == 2 && p.src_occ == 11);
    }
    {   // every sphere tested: the list from LDS when it fits 64 KB; the prefixes stay as they are
        Tune t;
        SourcePair p = plan_sources(small_scene(), t.v, RT_ALGO_WAVEFRONT_BRUTE);
        CHECK(p.src == 1 && p.src_occ == 1 && !p.sets_prefix);
        p = plan_sources(big_scene(), t.v, RT_ALGO_WAVEFRONT_BRUTE);
        CHECK(p.src == 0 && p.src_occ == 0);
    }
}

static void stream_cases() {
    const int W = RT_ALGO_WAVEFRONT;
    Tune t;
    SceneFacts f = small_scene();
    StreamShape s = plan_streams(f, t.v, W, 9, 8);
    CHECK(s.n_b == 2 && s.cam == 0 && s.grid_occ == 0 && s.wg_major == 1 && s.mark_gen == 1);
    f.has_cgrid = f.all_lights_gridded = true;
    s = plan_streams(f, t.v, W, 9, 8);
    CHECK(s.cam == 3 && s.grid_occ == 1);
    CHECK(plan_streams(f, t.v, RT_ALGO_WAVEFRONT_BRUTE, 1, 8).cam == 0);
    f = big_scene();
    f.has_cgrid = f.all_lights_gridded = true;
    s = plan_streams(f, t.v, W, 5, 8);
    CHECK(s.cam == 4 && s.grid_occ == 2 && !s.split);
    t.set(kTuneSplit, 1).set(kTuneGridOcc, 0).set(kTuneCam, 0).set(kTuneStaggerGen, 64).set(kTuneDeal, 0);
    s = plan_streams(f, t.v, W, 5, 3);
    CHECK(s.split && s.grid_occ == 0 && s.cam == 0 && s.mark_gen == 4 && s.wg_major == 0);
}

static void tail_cases() {
    Tune t;
    SceneFacts f = small_scene();
    f.all_lights_gridded = true;
    CHECK(plan_tail_fuse(f, t.v, 9, 4500000, 8) == 4);
    CHECK(plan_tail_fuse(f, t.v, 9, 9000000, 8) == 5);
    CHECK(plan_tail_fuse(f, t.v, 9, 16000000, 8) == 7);
    CHECK(plan_tail_fuse(f, t.v, 7, 4500000, 8) == 0);
    CHECK(plan_tail_fuse(f, t.v, 9, 16000000, 3) == 0);
    CHECK(plan_tail_fuse(f, t.v, 9, 4500000, 2) == 0);       // generation 4 does not exist at depth 2
    f.all_lights_gridded = false;
    CHECK(plan_tail_fuse(f, t.v, 9, 4500000, 8) == 0);
    f.all_lights_gridded = true;
    t.set(kTuneTailFuse, 0);
    CHECK(plan_tail_fuse(f, t.v, 9, 4500000, 8) == 0);
    t.set(kTuneTailFuse, 6);
    CHECK(plan_tail_fuse(f, t.v, 9, 16000000, 8) == 6);
}

static void algo_cases() {
    int mode = -1;
    const char* err = nullptr;
    SceneFacts f = small_scene();
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_CENTER, 4, &mode, &err) == RT_OK && mode == RT_ALGO_WAVEFRONT);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 1, &mode, &err) == RT_OK && mode == RT_ALGO_WAVEFRONT);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err) == RT_OK && mode == RT_ALGO_PATH);
    f.n_lights = 33;
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_CENTER, 1, &mode, &err) == RT_OK && mode == RT_ALGO_BRUTE_LDS);
    err = nullptr;
    CHECK(plan_algo(f, RT_ALGO_WAVEFRONT, RT_JITTER_CENTER, 1, &mode, &err) == RT_E_UNSUPPORTED && err);
    f.n_spheres = 2049;        // 32 B each: beyond 64 KB
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_CENTER, 1, &mode, &err) == RT_OK && mode == RT_ALGO_BRUTE_GLOBAL);
    CHECK(plan_algo(f, RT_ALGO_BRUTE_LDS, RT_JITTER_CENTER, 1, &mode, &err) == RT_OK);
    f.n_spheres = 5121;        // beyond 160 KB
    err = nullptr;
    CHECK(plan_algo(f, RT_ALGO_BRUTE_LDS, RT_JITTER_CENTER, 1, &mode, &err) == RT_E_INVALID && err);
    f = small_scene();
    f.needs_path = true;
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_CENTER, 1, &mode, &err) == RT_OK && mode == RT_ALGO_PATH);
    err = nullptr;
    CHECK(plan_algo(f, RT_ALGO_WAVEFRONT, RT_JITTER_CENTER, 1, &mode, &err) == RT_E_UNSUPPORTED && err);
}

int main() {
    chunk_cases();
    layout_cases();
    source_cases();
    stream_cases();
    tail_cases();
    algo_cases();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("plan_check ok\n");
    return 0;
}
