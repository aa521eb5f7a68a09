// CPU check of the planner for skybox chain scenes (csrc/render_plan.cpp alone: no HIP, no GPU).
// A SkyboxBackground is no planner fact: rt_scene_upload no longer counts it under needs_path, and
// SceneFacts has no field for it (no decision depends on it: the sky passes need no plan).  So the
// facts of a skybox scene of chain classes are those of the same scene with a solid background,
// view grid included, and every algorithm is planned alike; a skybox scene with a path-only class
// (needs_path) is refused by the chain algorithms as before, in texts that name the classes left.
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

// What rt_scene_upload reports for scenes.skybox_chain_scene: three spheres, a plane, two lights
// (one directional: not every light gridded), the camera's view grid built (!needs_path).
static SceneFacts chain_facts(bool skybox) {
    SceneFacts f;
    f.n_spheres = 3; f.n_bvh = 2; f.n_bvh4 = 1; f.n_q4 = 1; f.n_lights = 2;
    f.short_stack = f.short_stack18 = true;
    f.has_cgrid = true;
    f.needs_path = false;          // the skybox sets nothing
    (void)skybox;
    return f;
}

static bool chain_algo(int a) {
    return a == RT_ALGO_WAVEFRONT || a == RT_ALGO_WAVEFRONT_BRUTE || a == RT_ALGO_BRUTE_LDS || a == RT_ALGO_BRUTE_GLOBAL;
}

int main() {
    int64_t tune[kTuneCount];
    for (int i = 0; i < kTuneCount; ++i) tune[i] = kTune[i].dflt;
    for (int algo : {RT_ALGO_AUTO, RT_ALGO_BRUTE_LDS, RT_ALGO_BRUTE_GLOBAL, RT_ALGO_WAVEFRONT, RT_ALGO_WAVEFRONT_BRUTE,
                     RT_ALGO_PATH, RT_ALGO_WAVEFRONT_AA})
        for (int jitter : {RT_JITTER_CENTER, RT_JITTER_RANDOM})
            for (uint32_t spp : {1u, 4u})
                for (int aw = 0; aw < 2; ++aw) {
                    int m_sky = -1, m_solid = -2;
                    const char *e_sky = nullptr, *e_solid = nullptr;
                    const int r_sky = plan_algo(chain_facts(true), algo, jitter, spp, &m_sky, &e_sky, aw);
                    const int r_solid = plan_algo(chain_facts(false), algo, jitter, spp, &m_solid, &e_solid, aw);
                    CHECK(r_sky == r_solid && m_sky == m_solid);
                    // the chain algorithms render it whenever they render the solid scene: one camera
                    // ray per pixel (the per-sample passes take random jitter with several samples)
                    const bool several = jitter != RT_JITTER_CENTER && spp > 1;
                    if (chain_algo(algo)) CHECK((r_sky == RT_OK) == !several);
                    if (algo == RT_ALGO_WAVEFRONT_AA || algo == RT_ALGO_PATH) CHECK(r_sky == RT_OK && m_sky == algo);
                    if (algo == RT_ALGO_AUTO)
                        CHECK(r_sky == RT_OK && m_sky == (several ? (aw ? RT_ALGO_WAVEFRONT_AA : RT_ALGO_PATH) : RT_ALGO_WAVEFRONT));
                    if (r_sky == RT_OK) {          // ... on the same sources and streams
                        const SourcePair a = plan_sources(chain_facts(true), tune, m_sky), b = plan_sources(chain_facts(false), tune, m_solid);
                        CHECK(a.src == b.src && a.src_occ == b.src_occ);
                        const StreamShape s = plan_streams(chain_facts(true), tune, m_sky, a.src, 4),
                                          t = plan_streams(chain_facts(false), tune, m_solid, b.src, 4);
                        CHECK(s.cam == t.cam && s.split == t.split && s.n_b == t.n_b && s.grid_occ == t.grid_occ);
                    }
                    // a skybox scene with a Transparent sphere or a DoF camera: refused as before
                    SceneFacts p = chain_facts(true);
                    p.needs_path = true;
                    p.has_cgrid = false;
                    int m = -1;
                    const char* e = nullptr;
                    const int r = plan_algo(p, algo, jitter, spp, &m, &e, aw);
                    if (algo == RT_ALGO_AUTO || algo == RT_ALGO_PATH) CHECK(r == RT_OK && m == RT_ALGO_PATH);
                    else CHECK(r == RT_E_UNSUPPORTED && e && std::strstr(e, "RT_ALGO_PATH") && !std::strstr(e, "kybox"));
                }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("sky_plan_check ok\n");
    return 0;
}
