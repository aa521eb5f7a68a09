// CPU check of the planner's cases for the variance-guided denoiser (csrc/render_plan.cpp alone: no HIP, no GPU):
// every refusal include/raytrace_amd.h lists for rt_denoise_var / rt_denoise_var_device, in its order -- those of
// rt_denoise with "all three outputs NULL" in the place of "both outputs NULL", then those of the rt_denoise_variance
// struct -- and that the passes and the scratch are plan_denoise's, unchanged.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

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

static float g_rgb[3], g_normal[3], g_depth[1], g_albedo[3], g_out[3], g_var[3], g_out_var[1];
static uint8_t g_bgr[3];

static rt_denoise_params good_params() {
    rt_denoise_params p{};
    p.width = 70; p.height = 66; p.iterations = 5;
    p.flags = RT_DN_NORMAL | RT_DN_DEPTH | RT_DN_COLOR | RT_DN_DEMODULATE;
    p.normal_squarings = 5; p.variant = 0; p.bgr_pitch = 0;
    p.sigma_color = 1.0; p.sigma_depth = 0.05;
    return p;
}
static rt_denoise_inputs good_inputs() { return rt_denoise_inputs{g_rgb, g_normal, g_depth, g_albedo}; }
static rt_denoise_variance good_var() { return rt_denoise_variance{g_var, g_out_var, 2.0, 1.0 / 1048576.0}; }

static bool ok(const rt_denoise_params* p, const rt_denoise_inputs* in, const rt_denoise_variance* v, const void* rgb, const void* bgr) {
    const char* why = nullptr;
    return plan_denoise_var_args(p, in, v, rgb, bgr, &why) == RT_OK;
}

static bool refused(const rt_denoise_params* p, const rt_denoise_inputs* in, const rt_denoise_variance* v, const void* rgb,
                    const void* bgr, const char* word) {
    const char* why = nullptr;
    const int rc = plan_denoise_var_args(p, in, v, rgb, bgr, &why);
    if (rc != RT_E_INVALID || !why || !std::strstr(why, word)) {
        std::printf("  got rc %d, text %s (wanted \"%s\")\n", rc, why ? why : "(none)", word);
        return false;
    }
    return true;
}

// rt_denoise's refusals, through the new entry: the same answers in the same order
static void inherited_cases() {
    static_assert(RT_ABI_VERSION == 10 && RT_KF_COUNT == 8, "the variance-guided denoiser adds functions and one struct only");
    static_assert(sizeof(rt_denoise_params) == 48 && sizeof(rt_denoise_inputs) == 4 * sizeof(void*), "as they were");
    static_assert(sizeof(rt_denoise_variance) == 2 * sizeof(void*) + 16, "the documented layout");
    static_assert(offsetof(rt_denoise_variance, variance) == 0 && offsetof(rt_denoise_variance, out_variance) == sizeof(void*) &&
                      offsetof(rt_denoise_variance, sigma_variance) == 2 * sizeof(void*) &&
                      offsetof(rt_denoise_variance, variance_floor) == 2 * sizeof(void*) + 8,
                  "the documented layout");
    rt_denoise_params p = good_params();
    rt_denoise_inputs in = good_inputs();
    rt_denoise_variance v = good_var();
    CHECK(ok(&p, &in, &v, g_out, g_bgr));
    CHECK(refused(nullptr, &in, &v, g_out, g_bgr, "null"));
    CHECK(refused(&p, nullptr, &v, g_out, g_bgr, "null"));
    p = good_params(); p.width = 0; CHECK(refused(&p, &in, &v, g_out, g_bgr, "width"));
    p = good_params(); p.height = 0; CHECK(refused(&p, &in, &v, g_out, g_bgr, "height"));
    p = good_params(); p.iterations = 0; CHECK(refused(&p, &in, &v, g_out, g_bgr, "iterations"));
    p = good_params(); p.iterations = 9; CHECK(refused(&p, &in, &v, g_out, g_bgr, "iterations"));
    p = good_params(); p.flags = 16; CHECK(refused(&p, &in, &v, g_out, g_bgr, "flag"));      // no new flag bit
    p = good_params(); p.normal_squarings = 11; CHECK(refused(&p, &in, &v, g_out, g_bgr, "normal_squarings"));
    p = good_params(); p.variant = 3; CHECK(refused(&p, &in, &v, g_out, g_bgr, "variant"));
    p = good_params();
    in = good_inputs(); in.rgb = nullptr; CHECK(refused(&p, &in, &v, g_out, g_bgr, "rgb"));
    in = good_inputs(); in.normal = nullptr; CHECK(refused(&p, &in, &v, g_out, g_bgr, "guide"));
    in = good_inputs(); in.depth = nullptr; CHECK(refused(&p, &in, &v, g_out, g_bgr, "guide"));
    in = good_inputs(); in.albedo = nullptr; CHECK(refused(&p, &in, &v, g_out, g_bgr, "guide"));
    in = good_inputs();
    const double bad[] = {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
    for (double s : bad) {
        p = good_params(); p.sigma_depth = s; CHECK(refused(&p, &in, &v, g_out, g_bgr, "sigma_depth"));
        p.flags &= ~static_cast<uint32_t>(RT_DN_DEPTH); CHECK(ok(&p, &in, &v, g_out, g_bgr));
        p = good_params(); p.sigma_color = s; CHECK(refused(&p, &in, &v, g_out, g_bgr, "sigma_color"));
        p.flags &= ~static_cast<uint32_t>(RT_DN_COLOR); CHECK(ok(&p, &in, &v, g_out, g_bgr));
    }
    p = good_params();
    p.bgr_pitch = 3 * 70 - 1; CHECK(refused(&p, &in, &v, g_out, g_bgr, "bgr_pitch"));
    p.bgr_pitch = 3 * 70 + 2; CHECK(ok(&p, &in, &v, g_out, g_bgr));
    p = good_params();
    CHECK(refused(&p, &in, &v, g_rgb, g_bgr, "out_rgb"));
}

static void output_cases() {
    rt_denoise_params p = good_params();
    rt_denoise_inputs in = good_inputs();
    rt_denoise_variance v = good_var();
    // any one output is enough
    CHECK(ok(&p, &in, &v, g_out, nullptr));
    CHECK(ok(&p, &in, &v, nullptr, g_bgr));
    CHECK(ok(&p, &in, &v, nullptr, nullptr));                 // out_variance alone
    v.out_variance = nullptr;
    CHECK(ok(&p, &in, &v, g_out, nullptr));
    CHECK(ok(&p, &in, &v, nullptr, g_bgr));
    CHECK(refused(&p, &in, &v, nullptr, nullptr, "three outputs"));
    // a null struct has no third output: the outputs answer first, as their place in the order says
    CHECK(refused(&p, &in, nullptr, nullptr, nullptr, "three outputs"));
}

static void variance_cases() {
    rt_denoise_params p = good_params();
    rt_denoise_inputs in = good_inputs();
    rt_denoise_variance v = good_var();
    CHECK(refused(&p, &in, nullptr, g_out, g_bgr, "rt_denoise_variance"));
    v = good_var(); v.variance = nullptr; CHECK(refused(&p, &in, &v, g_out, g_bgr, "variance input"));
    const double bad[] = {0.0, -0.0, -1.0, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                          std::numeric_limits<double>::quiet_NaN()};
    for (double s : bad) {
        v = good_var(); v.sigma_variance = s; CHECK(refused(&p, &in, &v, g_out, g_bgr, "sigma_variance"));
        v = good_var(); v.variance_floor = s; CHECK(refused(&p, &in, &v, g_out, g_bgr, "variance_floor"));
    }
    v = good_var(); v.sigma_variance = 5e-324; v.variance_floor = 1e308; CHECK(ok(&p, &in, &v, g_out, g_bgr));
    v = good_var(); v.sigma_variance = 1e308; v.variance_floor = 5e-324; CHECK(ok(&p, &in, &v, g_out, g_bgr));
    v = good_var(); v.out_variance = g_var; CHECK(refused(&p, &in, &v, g_out, g_bgr, "out_variance"));
    // the variance is read whatever the flags are, also by a plain blur
    p.flags = 0; p.sigma_color = p.sigma_depth = 0.0;
    in = rt_denoise_inputs{g_rgb, nullptr, nullptr, nullptr};
    v = good_var(); CHECK(ok(&p, &in, &v, g_out, g_bgr));
    v.variance = nullptr; CHECK(refused(&p, &in, &v, g_out, g_bgr, "variance input"));
}

// the order: the first failing check of the header's list answers
static void order_cases() {
    rt_denoise_inputs in = good_inputs();
    rt_denoise_variance v = good_var();
    rt_denoise_params p = good_params();
    // every check of rt_denoise comes before every check of the struct
    v.variance = nullptr; v.sigma_variance = 0.0;
    p.width = 0; CHECK(refused(&p, &in, &v, g_out, g_bgr, "width"));
    p = good_params(); p.bgr_pitch = 1; CHECK(refused(&p, &in, &v, g_out, g_bgr, "bgr_pitch"));
    p = good_params(); CHECK(refused(&p, &in, &v, g_rgb, g_bgr, "out_rgb"));
    CHECK(refused(&p, &in, nullptr, g_rgb, g_bgr, "out_rgb"));
    p = good_params(); p.variant = 9; CHECK(refused(&p, &in, nullptr, nullptr, nullptr, "variant"));
    // outputs before pitch before out_rgb == rgb, as in rt_denoise
    p = good_params(); p.bgr_pitch = 1; v = good_var(); v.out_variance = nullptr;
    CHECK(refused(&p, &in, &v, nullptr, nullptr, "three outputs"));
    // within the struct: null struct, variance, sigma_variance, variance_floor, out_variance == variance
    p = good_params();
    v = good_var(); v.variance = nullptr; v.sigma_variance = 0.0; v.variance_floor = 0.0;
    CHECK(refused(&p, &in, &v, g_out, g_bgr, "variance input"));
    v.variance = g_var; v.out_variance = g_var; CHECK(refused(&p, &in, &v, g_out, g_bgr, "sigma_variance"));
    v.sigma_variance = 2.0; CHECK(refused(&p, &in, &v, g_out, g_bgr, "variance_floor"));
    v.variance_floor = 1.0; CHECK(refused(&p, &in, &v, g_out, g_bgr, "out_variance"));
    v.out_variance = g_out_var; CHECK(ok(&p, &in, &v, g_out, g_bgr));
}

// the passes are plan_denoise's and the scratch has the same size: the variance rides in the colour record
static void plan_cases() {
    rt_denoise_params p = good_params();
    const DenoisePlan d = plan_denoise(p);
    CHECK(d.passes == 5 && d.grid_x == 2 && d.grid_y == 9);
    CHECK(d.image_bytes == 73984 && d.scratch_bytes == 3 * d.image_bytes);
    static_assert(kDnRecordBytes == 16, "one dwordx4 per record: three colours and the variance");
    p.width = 4096; p.height = 4096;
    CHECK(plan_denoise(p).scratch_bytes == 3ull << 28);
}

int main() {
    inherited_cases();
    output_cases();
    variance_cases();
    order_cases();
    plan_cases();
    if (failures) {
        std::printf("denoise_var_plan_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("denoise_var_plan_check ok\n");
    return 0;
}
