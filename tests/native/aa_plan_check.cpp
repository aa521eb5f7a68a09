// CPU check of the planner's cases for RT_ALGO_WAVEFRONT_AA (csrc/render_plan.cpp alone: no HIP,
// no GPU): which renders the mode accepts and refuses, what RT_ALGO_AUTO answers with and without
// tuning aa_wavefront, that the other algorithms answer as before, and the working-set layout and
// budget with the running sums.  The expected values follow from the rules in include/raytrace_amd.h.
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

static SceneFacts chain_scene() {     // Phong / Fresnel spheres and planes, two lights
    SceneFacts f;
    f.n_spheres = 100; f.n_bvh = 99; f.n_bvh4 = 40; f.n_lights = 2;
    f.short_stack = f.short_stack18 = true;
    return f;
}

static void algo_cases() {
    const int AA = RT_ALGO_WAVEFRONT_AA;
    static_assert(RT_ALGO_WAVEFRONT_AA == 6, "the value the header documents");
    int mode = -1;
    const char* err = nullptr;
    SceneFacts f = chain_scene();
    // accepted for a chain scene with any jitter and spp; passes per sample only for (random, > 1)
    CHECK(plan_algo(f, AA, RT_JITTER_RANDOM, 4, &mode, &err) == RT_OK && mode == AA);
    CHECK(plan_aa_passes(mode, RT_JITTER_RANDOM, 4));
    CHECK(plan_algo(f, AA, RT_JITTER_CENTER, 4, &mode, &err) == RT_OK && mode == AA);
    CHECK(!plan_aa_passes(mode, RT_JITTER_CENTER, 4));
    CHECK(plan_algo(f, AA, RT_JITTER_RANDOM, 1, &mode, &err) == RT_OK && mode == AA);
    CHECK(!plan_aa_passes(mode, RT_JITTER_RANDOM, 1));
    CHECK(!plan_aa_passes(RT_ALGO_WAVEFRONT, RT_JITTER_RANDOM, 4) && !plan_aa_passes(RT_ALGO_PATH, RT_JITTER_RANDOM, 4));
    f.n_lights = 32;
    CHECK(plan_algo(f, AA, RT_JITTER_RANDOM, 4, &mode, &err) == RT_OK && mode == AA);
    // refused: a class only the path kernel renders, more than 32 lights; the texts say so
    f = chain_scene();
    f.needs_path = true;
    err = nullptr;
    CHECK(plan_algo(f, AA, RT_JITTER_RANDOM, 4, &mode, &err) == RT_E_UNSUPPORTED && err && std::strstr(err, "RT_ALGO_PATH"));
    err = nullptr;
    CHECK(plan_algo(f, AA, RT_JITTER_CENTER, 1, &mode, &err) == RT_E_UNSUPPORTED && err);
    f = chain_scene();
    f.n_lights = 33;
    err = nullptr;
    CHECK(plan_algo(f, AA, RT_JITTER_RANDOM, 4, &mode, &err) == RT_E_UNSUPPORTED && err && std::strstr(err, "32 lights"));
    // RT_ALGO_AUTO: the path kernel unless tuning aa_wavefront is set, then mode 6 for (random, > 1) only
    f = chain_scene();
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err) == RT_OK && mode == RT_ALGO_PATH);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err, 0) == RT_OK && mode == RT_ALGO_PATH);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err, 1) == RT_OK && mode == AA);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 1, &mode, &err, 1) == RT_OK && mode == RT_ALGO_WAVEFRONT);
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_CENTER, 4, &mode, &err, 1) == RT_OK && mode == RT_ALGO_WAVEFRONT);
    f.n_lights = 33;
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err, 1) == RT_OK && mode == RT_ALGO_PATH);
    f = chain_scene();
    f.needs_path = true;
    CHECK(plan_algo(f, RT_ALGO_AUTO, RT_JITTER_RANDOM, 4, &mode, &err, 1) == RT_OK && mode == RT_ALGO_PATH);
    // the other chain algorithms still refuse random jitter with several samples, whatever the key says
    f = chain_scene();
    for (int aw = 0; aw < 2; ++aw) {
        for (int algo : {RT_ALGO_WAVEFRONT, RT_ALGO_WAVEFRONT_BRUTE, RT_ALGO_BRUTE_LDS, RT_ALGO_BRUTE_GLOBAL}) {
            err = nullptr;
            CHECK(plan_algo(f, algo, RT_JITTER_RANDOM, 2, &mode, &err, aw) == RT_E_UNSUPPORTED && err);
            CHECK(plan_algo(f, algo, RT_JITTER_CENTER, 2, &mode, &err, aw) == RT_OK && mode == algo);
        }
        CHECK(plan_algo(f, RT_ALGO_PATH, RT_JITTER_RANDOM, 2, &mode, &err, aw) == RT_OK && mode == RT_ALGO_PATH);
    }
}

static void tuning_cases() {
    // appended after the existing keys, default 0, values 0 and 1
    CHECK(kTuneAaWavefront == kTuneCount - 1);
    CHECK(std::strcmp(kTune[kTuneAaWavefront].name, "aa_wavefront") == 0);
    CHECK(kTune[kTuneAaWavefront].dflt == 0 && kTune[kTuneAaWavefront].lo == 0 && kTune[kTuneAaWavefront].hi == 1);
    CHECK(std::strcmp(kTune[kTuneAaWavefront - 1].name, "dev_join") == 0);
}

static void layout_cases() {
    // the running sums: 3 f64 per chunk pixel, the last section, counted by the budget
    const uint32_t cap = 128 * 32, G = 4, R = 1024, levels = 9;
    const WfLayout w0 = wf_layout(cap, G, R, levels), w = wf_layout(cap, G, R, levels, true);
    CHECK(w0.s_acc == 0 && w0.total == wf_layout(cap, G, R, levels, false).total);
    CHECK(w.s_acc == 24ull * cap && w.o_acc % 256 == 0);
    CHECK(w.o_acc >= w.o_ccol + w.s_ccol && w.o_acc < w.o_ccol + w.s_ccol + 256);
    CHECK(w.total >= w.o_acc + w.s_acc && w.total < w.o_acc + w.s_acc + 256);
    CHECK(w.o_rec == w0.o_rec && w.o_lev == w0.o_lev && w.o_term == w0.o_term && w.o_pmap == w0.o_pmap && w.o_ccol == w0.o_ccol);
    CHECK(w.total == w0.total + align_up(w.s_acc, 256));
    CHECK(wf_bytes_per_slot(levels, true) == wf_bytes_per_slot(levels) + 24);
    int64_t tune[kTuneCount];
    for (int i = 0; i < kTuneCount; ++i) tune[i] = kTune[i].dflt;
    const uint64_t budget = 1ull << 30;
    CHECK(plan_cap_px(tune, budget, levels, true) == budget / wf_bytes_per_slot(levels, true));
    CHECK(plan_cap_px(tune, budget, levels, true) < plan_cap_px(tune, budget, levels));
    tune[kTuneChunkPixels] = 4096;
    CHECK(plan_cap_px(tune, budget, levels, true) == 4096);
}

int main() {
    algo_cases();
    tuning_cases();
    layout_cases();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("aa_plan_check ok\n");
    return 0;
}
