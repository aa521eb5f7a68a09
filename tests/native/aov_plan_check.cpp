// CPU check of the planner's cases for the first-hit feature buffers (csrc/render_plan.cpp alone: no HIP, no
// GPU): which sphere source aov_primary gets for which scene and tuning, the argument checks that need no
// device, and the launch's workgroups.  The expected values follow from the rules in render_plan.hpp
// (plan_aov_source) and include/raytrace_amd.h (rt_render_aov's refusals).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

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
    Tune& set(TuneKey k, int64_t x) {
        v[k] = x;
        return *this;
    }
};

static SceneFacts small_scene() {     // tree and spheres fit LDS, compact stacks possible
    SceneFacts f;
    f.n_spheres = 200; f.n_bvh = 199; f.n_bvh4 = 70; f.n_lights = 2;
    f.short_stack = f.short_stack18 = true;
    f.has_half = true;
    return f;
}

static SceneFacts big_scene() {       // 100k spheres: nothing fits LDS
    SceneFacts f;
    f.n_spheres = 100000; f.n_bvh = 50000; f.n_bvh4 = 17000; f.n_lights = 2;
    f.has_half = true;
    return f;
}

static void source_cases() {
    static_assert(RT_AOV_DEPTH == 1 && RT_AOV_NORMAL == 2 && RT_AOV_ALBEDO == 4 && RT_AOV_COVERAGE == 8 && RT_AOV_OBJECT == 16,
                  "the values the header documents");
    static_assert(RT_ABI_VERSION == 10 && RT_KF_COUNT == 8, "ABI 9 adds functions and types only");
    // the camera's view grid where the scene has one: spheres in LDS when the list fits, else through L2
    SceneFacts f = small_scene();
    f.has_cgrid = true;
    CHECK(plan_aov_source(f, Tune().v).src == 22);
    CHECK(plan_aov_source(f, Tune().set(kTuneCam, 3).v).src == 22);
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 7).v).src == 22);          // generation 0 takes the grid whatever src says
    f.n_spheres = 3000;                                                      // 3000 * 36 B > 72 KB
    CHECK(plan_aov_source(f, Tune().v).src == 23);
    // the grid off (tuning cam) or not built: the source the later generations take
    f = small_scene();
    f.has_cgrid = true;
    CHECK(plan_aov_source(f, Tune().set(kTuneCam, 0).v).src == 9);
    f.has_cgrid = false;
    CHECK(plan_aov_source(f, Tune().v).src == 9);                            // the whole tree in LDS, compact stack
    CHECK(plan_aov_source(f, Tune().set(kTuneCam, 3).v).src == 9);           // (asked for, not built)
    CHECK(plan_aov_source(f, Tune().set(kTuneCompact, 0).v).src == 7);
    f.short_stack = false;
    CHECK(plan_aov_source(f, Tune().v).src == 7);
    // beyond LDS: the prefix sources
    f = big_scene();
    CHECK(plan_aov_source(f, Tune().v).src == 5);
    f.short_stack18 = true;
    CHECK(plan_aov_source(f, Tune().v).src == 6);
    CHECK(plan_aov_source(f, Tune().set(kTuneHalf, 0).v).src == 8);
    f.has_half = false;
    CHECK(plan_aov_source(f, Tune().v).src == 8);
    // the prefix follows tuning prefix_kb: KB of 64-byte nodes
    CHECK(plan_aov_source(f, Tune().v).pfx2 == 64 * 1024 / 64);
    CHECK(plan_aov_source(f, Tune().set(kTunePrefixKb2, 1).v).pfx2 == 16);
    // the quantised tree has no instantiation: what the scene gets without it
    f = big_scene();
    f.q4_ok = true; f.n_q4 = 9000;
    CHECK(plan_aov_source(f, Tune().set(kTuneQTree, 1).v).src == 5);
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 26).v).src == 5);
    // tuning src forces a family by itself (its shadow partner is filled in)
    f = small_scene();
    for (int s : {2, 7, 9, 8, 5, 6}) CHECK(plan_aov_source(f, Tune().set(kTuneSrc, s).v).src == s);
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 9).set(kTuneSrcOcc, 10).v).src == 9);
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 1).v).src == 1);
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 0).v).src == 0);
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 14).v).src == 2);          // no nearest-hit source: the binary tree through L2
    f.has_half = false;
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 5).v).src == 2);           // not built for this scene
    f = big_scene();
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 7).v).src == 2);           // does not fit
    CHECK(plan_aov_source(f, Tune().set(kTuneSrc, 1).v).src == 0);           // the list does not fit 64 KB
    // a tree the 4-wide stack could overflow: the binary tree only
    f = small_scene();
    f.deep_bvh4 = true;
    CHECK(plan_aov_source(f, Tune().v).src == 7);
    // no tree at all: brute force
    f = SceneFacts{};
    CHECK(plan_aov_source(f, Tune().v).src == 1);
    f.n_spheres = 1;
    CHECK(plan_aov_source(f, Tune().v).src == 1);
    // every answer has an instantiation
    for (int s = -1; s <= 26; ++s)
        for (int cam : {-1, 0, 3})
            for (const SceneFacts& g : {small_scene(), big_scene(), SceneFacts{}}) {
                SceneFacts h = g;
                CHECK(aov_source_known(plan_aov_source(h, Tune().set(kTuneSrc, s).set(kTuneCam, cam).v).src));
                h.has_cgrid = h.n_spheres > 0;
                CHECK(aov_source_known(plan_aov_source(h, Tune().set(kTuneSrc, s).set(kTuneCam, cam).v).src));
            }
    CHECK(!aov_source_known(25) && !aov_source_known(10) && !aov_source_known(3));
}

static void argument_cases() {
    float d = 0, n = 0, a = 0, c = 0;
    int32_t o = 0;
    const void* all[5] = {&d, &n, &a, &c, &o};
    const char* err = nullptr;
    CHECK(plan_aov_args(31, all, &err) == RT_OK);
    for (uint32_t m = 1; m < 32; ++m) CHECK(plan_aov_args(m, all, &err) == RT_OK);
    err = nullptr;
    CHECK(plan_aov_args(0, all, &err) == RT_E_INVALID && err && std::strstr(err, "no channel"));
    err = nullptr;
    CHECK(plan_aov_args(32, all, &err) == RT_E_INVALID && err && std::strstr(err, "unknown"));
    CHECK(plan_aov_args(31 | 1u << 31, all, &err) == RT_E_INVALID);
    // a selected channel needs its pointer; an unselected one does not
    for (int i = 0; i < 5; ++i) {
        const void* p[5] = {&d, &n, &a, &c, &o};
        p[i] = nullptr;
        err = nullptr;
        CHECK(plan_aov_args(31, p, &err) == RT_E_INVALID && err && std::strstr(err, "NULL"));
        CHECK(plan_aov_args(1u << i, p, &err) == RT_E_INVALID);
        CHECK(plan_aov_args(31u & ~(1u << i), p, &err) == RT_OK);
    }
    const void* none[5] = {};
    CHECK(plan_aov_args(RT_AOV_DEPTH, none, &err) == RT_E_INVALID);
}

static void workgroup_cases() {
    CHECK(plan_aov_workgroups(0, 256) == 1);
    CHECK(plan_aov_workgroups(1, 256) == 1);
    CHECK(plan_aov_workgroups(1024, 256) == 1);
    CHECK(plan_aov_workgroups(1025, 256) == 2);
    CHECK(plan_aov_workgroups(96 * 64, 256) == 6);
    CHECK(plan_aov_workgroups(4096ull * 4096, 256) == 512);       // two resident workgroups per CU
    CHECK(plan_aov_workgroups(1ull << 40, 256) == 512);
    CHECK(plan_aov_workgroups(4096ull * 4096, 0) == 2);
}

int main() {
    source_cases();
    argument_cases();
    workgroup_cases();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("aov_plan_check ok\n");
    return 0;
}
