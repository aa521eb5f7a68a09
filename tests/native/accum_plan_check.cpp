// CPU check of the planner's rules for an accumulating render (rt_render_accumulate; csrc/render_plan.cpp
// alone: no HIP, no GPU): the algorithm choice and the refusals, the forced passes, the path kernel's lanes
// per pixel from the call's own n, no sparse copies and no per-chunk resolve.  The expected values follow
// from the rules in include/raytrace_amd.h.
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

static SceneFacts chain_scene() {
    SceneFacts f;
    f.n_spheres = 100; f.n_bvh = 99; f.n_bvh4 = 40; f.n_lights = 2;
    f.short_stack = f.short_stack18 = true;
    return f;
}

static void algo_cases() {
    const int AA = RT_ALGO_WAVEFRONT_AA, PATH = RT_ALGO_PATH;
    AccumPlan p;
    const char* err = nullptr;
    SceneFacts f = chain_scene();
    // the path kernel: every class; no passes
    CHECK(plan_accumulate(f, PATH, 0, 0, 4, 0, &p, &err) == RT_OK && p.mode == PATH && p.passes == 0);
    f.needs_path = true;
    CHECK(plan_accumulate(f, PATH, 0, 3, 1, 1, &p, &err) == RT_OK && p.mode == PATH && p.passes == 0);
    // the passes: forced, one per sample of the call, also for one sample (and whatever the jitter: it is no argument)
    f = chain_scene();
    for (uint32_t n : {1u, 2u, 16u}) {
        CHECK(plan_accumulate(f, AA, 0, 7, n, 0, &p, &err) == RT_OK && p.mode == AA && p.passes == n);
        CHECK(!p.sparse && !p.chunk_resolve);
    }
    f.n_lights = 32;
    CHECK(plan_accumulate(f, AA, 0, 0, 2, 0, &p, &err) == RT_OK && p.mode == AA);
    // ... refused as the mode refuses a one-shot render
    f.n_lights = 33;
    err = nullptr;
    CHECK(plan_accumulate(f, AA, 0, 0, 2, 0, &p, &err) == RT_E_UNSUPPORTED && err && std::strstr(err, "32 lights"));
    f = chain_scene();
    f.needs_path = true;
    err = nullptr;
    CHECK(plan_accumulate(f, AA, 0, 0, 2, 0, &p, &err) == RT_E_UNSUPPORTED && err && std::strstr(err, "RT_ALGO_PATH"));
    // RT_ALGO_AUTO: today's rule without jitter and spp: the path kernel, unless chain classes and aa_wavefront
    f = chain_scene();
    CHECK(plan_accumulate(f, RT_ALGO_AUTO, 0, 0, 4, 0, &p, &err) == RT_OK && p.mode == PATH && p.passes == 0);
    CHECK(plan_accumulate(f, RT_ALGO_AUTO, 0, 0, 4, 1, &p, &err) == RT_OK && p.mode == AA && p.passes == 4);
    CHECK(plan_accumulate(f, RT_ALGO_AUTO, 0, 5, 1, 1, &p, &err) == RT_OK && p.mode == AA && p.passes == 1);
    f.n_lights = 33;
    CHECK(plan_accumulate(f, RT_ALGO_AUTO, 0, 0, 4, 1, &p, &err) == RT_OK && p.mode == PATH);
    f = chain_scene();
    f.needs_path = true;
    CHECK(plan_accumulate(f, RT_ALGO_AUTO, 0, 0, 4, 1, &p, &err) == RT_OK && p.mode == PATH);
    // algorithms 1-4 trace one sample for all: unsupported; anything else is no algorithm
    f = chain_scene();
    for (int algo : {RT_ALGO_BRUTE_LDS, RT_ALGO_BRUTE_GLOBAL, RT_ALGO_WAVEFRONT, RT_ALGO_WAVEFRONT_BRUTE}) {
        err = nullptr;
        CHECK(plan_accumulate(f, algo, 0, 0, 1, 1, &p, &err) == RT_E_UNSUPPORTED && err);
    }
    for (int algo : {-1, 7, 100}) CHECK(plan_accumulate(f, algo, 0, 0, 1, 0, &p, &err) == RT_E_INVALID);
    // flags: RT_COUNT_WORK and RT_TIME_KERNELS only
    for (uint32_t fl : {0u, uint32_t(RT_COUNT_WORK), uint32_t(RT_TIME_KERNELS), uint32_t(RT_COUNT_WORK | RT_TIME_KERNELS)})
        CHECK(plan_accumulate(f, PATH, fl, 0, 1, 0, &p, &err) == RT_OK);
    for (uint32_t fl : {uint32_t(RT_OUT_RGB_F32), uint32_t(RT_OUT_BGR_U8), uint32_t(RT_OUT_FRAME_ROWS), 32u, 0x80000000u,
                        uint32_t(RT_COUNT_WORK | RT_OUT_BGR_U8)}) {
        err = nullptr;
        CHECK(plan_accumulate(f, PATH, fl, 0, 1, 0, &p, &err) == RT_E_INVALID && err);
    }
    // the count: up to 2^31, not past it; n == 0 passes the checks (the caller renders nothing)
    CHECK(plan_accumulate(f, PATH, 0, 0, 0, 0, &p, &err) == RT_OK);
    CHECK(plan_accumulate(f, AA, 0, 9, 0, 0, &p, &err) == RT_OK && p.passes == 0);
    CHECK(plan_accumulate(f, PATH, 0, 0, 1u << 31, 0, &p, &err) == RT_OK);
    CHECK(plan_accumulate(f, PATH, 0, (1u << 31) - 1, 1, 0, &p, &err) == RT_OK);
    CHECK(plan_accumulate(f, PATH, 0, 1u << 31, 0, 0, &p, &err) == RT_OK);
    CHECK(plan_accumulate(f, PATH, 0, 1u << 31, 1, 0, &p, &err) == RT_E_INVALID);
    CHECK(plan_accumulate(f, PATH, 0, 1, 1u << 31, 0, &p, &err) == RT_E_INVALID);
    CHECK(plan_accumulate(f, PATH, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, &p, &err) == RT_E_INVALID);
    // an ordinary render's rules are as they were
    int mode = -1;
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err) == RT_OK && mode == PATH);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_CENTER, 4, &mode, &err) == RT_OK && mode == RT_ALGO_WAVEFRONT);
    CHECK(!plan_aa_passes(AA, RT_JITTER_RANDOM, 1) && !plan_aa_passes(AA, RT_JITTER_CENTER, 4));
}

static void group_cases() {
    // 256 CUs x 256 work-items x 2 waves per SIMD
    const uint32_t T = 256u * 256u * 2u;
    // from the call's n: one sample never shares a pixel, however many the accumulator already holds
    CHECK(plan_path_group(96 * 64, 1, T, 0) == 1);
    CHECK(plan_path_group(96 * 64, 2, T, 0) == 2);
    CHECK(plan_path_group(96 * 64, 3, T, 0) == 2);
    CHECK(plan_path_group(96 * 64, 16, T, 0) == 16);
    CHECK(plan_path_group(96 * 64, 1024, T, 0) == 32);            // 6144 * 32 >= T stops the doubling
    CHECK(plan_path_group(1, 1u << 31, T, 0) == 64);
    CHECK(plan_path_group(1024 * 1024, 16, T, 0) == 1);           // the frame fills the chip
    CHECK(plan_path_group(0, 16, T, 0) == 16);
    // the tuning override, as an ordinary render takes it: a power of two <= 64, else 1
    CHECK(plan_path_group(96 * 64, 1, T, 8) == 8);
    CHECK(plan_path_group(96 * 64, 16, T, 64) == 64);
    CHECK(plan_path_group(96 * 64, 16, T, 3) == 1);
    CHECK(plan_path_group(96 * 64, 16, T, 128) == 1);
    for (uint32_t n = 1; n < 200; ++n) {
        const uint32_t G = plan_path_group(48 * 32, n, T, 0);
        CHECK(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && G <= n);
    }
}

static void layout_cases() {
    // the passes of an accumulating call use RT_ALGO_WAVEFRONT_AA's plan (chunks and working set), so a
    // reserve with that algorithm covers them: the cap and the layout depend on nothing of the call's n
    int64_t tune[kTuneCount];
    for (int i = 0; i < kTuneCount; ++i) tune[i] = kTune[i].dflt;
    const uint64_t budget = 1ull << 30;
    CHECK(plan_cap_px(tune, budget, 9, true) == budget / wf_bytes_per_slot(9, true));
    static_assert(kAccumFlags == (RT_COUNT_WORK | RT_TIME_KERNELS), "the two flags the header allows");
    static_assert(kAccumMaxSamples == 1u << 31, "the header's bound");
    static_assert(kWfAccBytes == 24, "24 B per pixel, as the accumulator");
}

int main() {
    algo_cases();
    group_cases();
    layout_cases();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("accum_plan_check ok\n");
    return 0;
}
