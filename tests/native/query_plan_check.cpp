// CPU check of the planner's cases for the ray queries (csrc/render_plan.cpp alone: no HIP, no GPU): which sphere
// source query_nearest and query_occluded get for which scene and tuning, the argument checks that need no device,
// and the launch's workgroups.  The expected values follow from the rules in render_plan.hpp (plan_query_source,
// plan_query_occ_source, plan_query_args) and include/raytrace_amd.h (the refusals of rt_query_nearest /
// rt_query_occluded).
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

static void nearest_source_cases() {
    static_assert(RT_HIT_T == 1 && RT_HIT_OBJECT == 2 && RT_HIT_NORMAL == 4, "the values the header documents");
    static_assert(kHitAll == (RT_HIT_T | RT_HIT_OBJECT | RT_HIT_NORMAL), "every channel");
    static_assert(RT_ABI_VERSION == 10 && RT_KF_COUNT == 8, "the queries add functions and types only");
    static_assert(sizeof(rt_hit_buffers) == 3 * sizeof(void*), "three pointers");
    // the camera's view grid is present but never chosen, whatever tuning cam says
    SceneFacts f = small_scene();
    f.has_cgrid = true;
    for (int cam : {-1, 0, 3, 4}) {
        CHECK(plan_query_source(f, Tune().set(kTuneCam, cam).v).src == 9);
        CHECK(plan_aov_source(f, Tune().set(kTuneCam, cam).v).src == (cam == 3 || cam == -1 ? 22 : 9));   // (the AOV takes it)
    }
    f.n_spheres = 3000;                                                      // the AOV's 23
    CHECK(plan_query_source(f, Tune().v).src != 23 && plan_query_source(f, Tune().v).src != 22);
    // without the grid: exactly plan_aov_source
    for (const SceneFacts& g : {small_scene(), big_scene(), SceneFacts{}})
        for (int s = -1; s <= 26; ++s)
            for (int cam : {-1, 0, 3}) {
                const Tune t = Tune().set(kTuneSrc, s).set(kTuneCam, cam);
                SceneFacts h = g;
                const QuerySource q = plan_query_source(h, t.v);
                const AovSource a = plan_aov_source(h, t.v);
                CHECK(q.src == a.src && q.pfx2 == a.pfx2);
                CHECK(query_source_known(q.src));
                h.has_cgrid = h.n_spheres > 0;
                CHECK(plan_query_source(h, t.v).src == a.src);               // the grid changes nothing
            }
    // the automatic choices
    f = small_scene();
    CHECK(plan_query_source(f, Tune().v).src == 9);
    CHECK(plan_query_source(f, Tune().set(kTuneCompact, 0).v).src == 7);
    f = big_scene();                                                         // a tree beyond LDS
    CHECK(plan_query_source(f, Tune().v).src == 5);
    f.short_stack18 = true;
    CHECK(plan_query_source(f, Tune().v).src == 6);
    f.has_half = false;
    CHECK(plan_query_source(f, Tune().v).src == 8);
    CHECK(plan_query_source(f, Tune().set(kTunePrefixKb2, 1).v).pfx2 == 16);
    // forced sources
    f = small_scene();
    for (int s : {0, 1, 2, 5, 6, 7, 8, 9}) CHECK(plan_query_source(f, Tune().set(kTuneSrc, s).v).src == s);
    f = big_scene();
    CHECK(plan_query_source(f, Tune().set(kTuneSrc, 1).v).src == 0);         // the list does not fit 64 KB
    CHECK(plan_query_source(f, Tune().set(kTuneSrc, 7).v).src == 2);         // does not fit
    // the quantised tree has no instantiation: the automatic choice
    f.q4_ok = true; f.n_q4 = 9000;
    CHECK(plan_query_source(f, Tune().set(kTuneSrc, 25).v).src == 5);
    CHECK(plan_query_source(f, Tune().set(kTuneSrc, 26).v).src == 5);
    CHECK(plan_query_source(f, Tune().set(kTuneQTree, 1).v).src == 5);
    // a scene without spheres, and one sphere without a tree: brute force from LDS
    f = SceneFacts{};
    CHECK(plan_query_source(f, Tune().v).src == 1);
    f.n_spheres = 1;
    CHECK(plan_query_source(f, Tune().v).src == 1);
    CHECK(!query_source_known(22) && !query_source_known(23) && !query_source_known(25) && !query_source_known(10));
}

static void occlusion_source_cases() {
    // the pair plan_sources gives RT_ALGO_WAVEFRONT: the 4-wide tree whole in LDS, or through L2 beyond it
    SceneFacts f = small_scene();
    CHECK(plan_query_occ_source(f, Tune().v).src == 10);
    CHECK(plan_query_occ_source(f, Tune().v).src == plan_sources(f, Tune().v, RT_ALGO_WAVEFRONT).src_occ);
    f = big_scene();
    CHECK(plan_query_occ_source(f, Tune().v).src == 11);
    CHECK(plan_query_occ_source(f, Tune().v).src == plan_sources(f, Tune().v, RT_ALGO_WAVEFRONT).src_occ);
    // tuning src (the nearest hit's) does not enter
    f = small_scene();
    for (int s : {0, 1, 2, 7, 9, 25}) CHECK(plan_query_occ_source(f, Tune().set(kTuneSrc, s).v).src == 10);
    // every light gridded: the light grids are the scene's own lights' and are never chosen
    f.all_lights_gridded = true;
    CHECK(plan_query_occ_source(f, Tune().v).src == 10);
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 14).v).src == 10);
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 15).v).src == 10);
    f = big_scene();
    f.all_lights_gridded = true;
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 14).v).src == 11);
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 15).v).src == 11);
    // forced sources where the scene has them
    f = small_scene();
    for (int s : {0, 1, 2, 7, 8, 10, 11}) CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, s).v).src == s);
    f = big_scene();
    for (int s : {0, 2, 8, 11}) CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, s).v).src == s);
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 1).v).src == 0);  // the list does not fit 64 KB
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 7).v).src == 11); // does not fit: the automatic choice
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 10).v).src == 11);
    for (int s : {3, 5, 6, 9, 22, 25, 26, 99}) CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, s).v).src == 11);
    CHECK(plan_query_occ_source(f, Tune().set(kTunePrefixKb2, 1).set(kTuneSrcOcc, 8).v).pfx2 == 16);
    // a tree the 4-wide stack could overflow: the binary tree only
    f = small_scene();
    f.deep_bvh4 = true;
    CHECK(plan_query_occ_source(f, Tune().v).src == 7);
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 10).v).src == 7);
    CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, 11).v).src == 7);
    f = big_scene();
    f.deep_bvh4 = true;
    CHECK(plan_query_occ_source(f, Tune().v).src == 2);
    // a scene without spheres, or without a tree: brute force
    f = SceneFacts{};
    CHECK(plan_query_occ_source(f, Tune().v).src == 1);
    f.n_spheres = 1;
    CHECK(plan_query_occ_source(f, Tune().v).src == 1);
    for (int s : {2, 7, 8, 10, 11}) CHECK(plan_query_occ_source(f, Tune().set(kTuneSrcOcc, s).v).src == 1);
    f.n_spheres = 3000;                                                      // no tree, 96 KB of spheres
    CHECK(plan_query_occ_source(f, Tune().v).src == 0);
    // every answer has an instantiation
    for (int s = -1; s <= 30; ++s)
        for (const SceneFacts& g : {small_scene(), big_scene(), SceneFacts{}}) {
            SceneFacts h = g;
            CHECK(query_occ_source_known(plan_query_occ_source(h, Tune().set(kTuneSrcOcc, s).v).src));
            h.deep_bvh4 = true;
            CHECK(query_occ_source_known(plan_query_occ_source(h, Tune().set(kTuneSrcOcc, s).v).src));
        }
    CHECK(!query_occ_source_known(14) && !query_occ_source_known(15) && !query_occ_source_known(9) &&
          !query_occ_source_known(5));
}

static QueryArgs good_nearest(const void* rays, const void* const p[3]) {
    QueryArgs a;
    a.rays = rays; a.n = 4; a.channels = kHitAll; a.has_bufs = true;
    for (int i = 0; i < 3; ++i) a.ptrs[i] = p[i];
    return a;
}

static void argument_cases() {
    alignas(16) double rays[4 * 6 + 2] = {};
    double t = 0, nrm = 0;
    int32_t obj = 0;
    uint8_t occ = 0;
    const void* const all[3] = {&t, &obj, &nrm};
    const char* err = nullptr;
    // nearest
    QueryArgs a = good_nearest(rays, all);
    CHECK(plan_query_args(a, &err) == RT_OK);
    for (uint32_t m = 1; m <= 7; ++m) { a.channels = m; CHECK(plan_query_args(a, &err) == RT_OK); }
    a = good_nearest(rays, all); a.channels = 0; err = nullptr;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "no channel"));
    a.channels = 8; err = nullptr;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "unknown"));
    a.channels = 7u | 1u << 31;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID);
    a = good_nearest(rays, all); a.flags = RT_TIME_KERNELS;
    CHECK(plan_query_args(a, &err) == RT_OK);
    for (uint32_t fl : {1u, 2u, 4u, 16u, 8u | 4u, 1u << 31}) {
        a.flags = fl; err = nullptr;
        CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "RT_TIME_KERNELS"));
    }
    a = good_nearest(nullptr, all); err = nullptr;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "rays"));
    a = good_nearest(rays, all); a.has_bufs = false; err = nullptr;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "struct"));
    for (int i = 0; i < 3; ++i) {            // a selected channel needs its pointer; an unselected one does not
        const void* p[3] = {&t, &obj, &nrm};
        p[i] = nullptr;
        a = good_nearest(rays, p); err = nullptr;
        CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "NULL"));
        a.channels = 1u << i;
        CHECK(plan_query_args(a, &err) == RT_E_INVALID);
        a.channels = 7u & ~(1u << i);
        CHECK(plan_query_args(a, &err) == RT_OK);
    }
    // the device variant: 16-byte alignment of the rays (a view offset by one ray keeps it, by one double loses it)
    a = good_nearest(rays, all); a.device = true;
    CHECK(plan_query_args(a, &err) == RT_OK);
    a.rays = rays + 6;
    CHECK(plan_query_args(a, &err) == RT_OK);
    a.rays = rays + 1; err = nullptr;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID && err && std::strstr(err, "aligned"));
    a.device = false;                        // the host variant stages the rays: any pointer
    CHECK(plan_query_args(a, &err) == RT_OK);
    // n == 0: no pointer is looked at, but flags and channels still are
    a = QueryArgs{}; a.channels = RT_HIT_T;
    CHECK(plan_query_args(a, &err) == RT_OK);
    a.device = true; a.rays = rays + 1;
    CHECK(plan_query_args(a, &err) == RT_OK);
    a.channels = 0;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID);
    a.channels = RT_HIT_T; a.flags = RT_COUNT_WORK;
    CHECK(plan_query_args(a, &err) == RT_E_INVALID);
    // occlusion
    QueryArgs o;
    o.occlusion = true; o.rays = rays; o.n = 4; o.occluded = &occ;
    CHECK(plan_query_args(o, &err) == RT_OK);                // channels do not enter
    o.flags = RT_TIME_KERNELS;
    CHECK(plan_query_args(o, &err) == RT_OK);
    o.flags = RT_OUT_RGB_F32;
    CHECK(plan_query_args(o, &err) == RT_E_INVALID);
    o.flags = 0; o.occluded = nullptr; err = nullptr;
    CHECK(plan_query_args(o, &err) == RT_E_INVALID && err && std::strstr(err, "occluded"));
    o.occluded = &occ; o.rays = nullptr;
    CHECK(plan_query_args(o, &err) == RT_E_INVALID);
    o.rays = rays + 1; o.device = true;
    CHECK(plan_query_args(o, &err) == RT_E_INVALID);
    o.device = false;
    CHECK(plan_query_args(o, &err) == RT_OK);
    o = QueryArgs{}; o.occlusion = true;                     // n == 0
    CHECK(plan_query_args(o, &err) == RT_OK);
}

static void workgroup_cases() {
    CHECK(plan_query_workgroups(0, 256) == 1);
    CHECK(plan_query_workgroups(1, 256) == 1);
    CHECK(plan_query_workgroups(1024, 256) == 1);
    CHECK(plan_query_workgroups(1025, 256) == 2);
    CHECK(plan_query_workgroups(512 * 1024, 256) == 512);         // two resident workgroups per CU
    CHECK(plan_query_workgroups(512 * 1024 + 1025, 256) == 512);  // the workgroups stride beyond that
    CHECK(plan_query_workgroups(0xFFFFFFFFull, 256) == 512);
    CHECK(plan_query_workgroups(4096ull * 4096, 0) == 2);
    for (uint64_t n : {0ull, 1ull, 1023ull, 1025ull, 600000ull, 1ull << 32})
        for (int cu : {0, 1, 64, 256, 304}) CHECK(plan_query_workgroups(n, cu) == plan_aov_workgroups(n, cu));
}

int main() {
    nearest_source_cases();
    occlusion_source_cases();
    argument_cases();
    workgroup_cases();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("query_plan_check ok\n");
    return 0;
}
