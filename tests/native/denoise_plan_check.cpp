// CPU check of the planner's cases for the denoiser (csrc/render_plan.cpp alone: no HIP, no GPU): every refusal
// include/raytrace_amd.h lists for rt_denoise / rt_denoise_device, in its order, and the per-pass plan (steps, the
// form of each pass under each variant, the grid, the scratch bytes).  The expected values follow from the rules in
// render_plan.hpp (plan_denoise_args, plan_denoise).
#include <cmath>
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

static float g_rgb[3], g_normal[3], g_depth[1], g_albedo[3], g_out[3];
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

static bool refused(const rt_denoise_params* p, const rt_denoise_inputs* in, const void* rgb, const void* bgr, const char* word) {
    const char* why = nullptr;
    const int rc = plan_denoise_args(p, in, rgb, bgr, &why);
    if (rc != RT_E_INVALID || !why || !std::strstr(why, word)) {
        std::printf("  got rc %d, text %s (wanted \"%s\")\n", rc, why ? why : "(none)", word);
        return false;
    }
    return true;
}

static void argument_cases() {
    static_assert(RT_DN_NORMAL == 1 && RT_DN_DEPTH == 2 && RT_DN_COLOR == 4 && RT_DN_DEMODULATE == 8, "the values the header documents");
    static_assert(RT_ABI_VERSION == 10 && RT_KF_COUNT == 8, "the denoiser adds functions and types only");
    static_assert(sizeof(rt_denoise_params) == 48 && sizeof(rt_denoise_inputs) == 4 * sizeof(void*), "the documented layout");
    const char* why = nullptr;
    rt_denoise_params p = good_params();
    rt_denoise_inputs in = good_inputs();
    CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    CHECK(plan_denoise_args(&p, &in, g_out, nullptr, &why) == RT_OK);
    CHECK(plan_denoise_args(&p, &in, nullptr, g_bgr, &why) == RT_OK);
    // a null argument
    CHECK(refused(nullptr, &in, g_out, g_bgr, "null"));
    CHECK(refused(&p, nullptr, g_out, g_bgr, "null"));
    // sizes, iterations, flags, squarings, variant
    p = good_params(); p.width = 0; CHECK(refused(&p, &in, g_out, g_bgr, "width"));
    p = good_params(); p.height = 0; CHECK(refused(&p, &in, g_out, g_bgr, "height"));
    p = good_params(); p.iterations = 0; CHECK(refused(&p, &in, g_out, g_bgr, "iterations"));
    p = good_params(); p.iterations = 9; CHECK(refused(&p, &in, g_out, g_bgr, "iterations"));
    p = good_params(); p.iterations = 8; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p = good_params(); p.iterations = 1; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p = good_params(); p.flags = 16; CHECK(refused(&p, &in, g_out, g_bgr, "flag"));
    p = good_params(); p.flags |= 1u << 31; CHECK(refused(&p, &in, g_out, g_bgr, "flag"));
    p = good_params(); p.normal_squarings = 11; CHECK(refused(&p, &in, g_out, g_bgr, "normal_squarings"));
    p = good_params(); p.normal_squarings = 10; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p = good_params(); p.normal_squarings = 0; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p = good_params(); p.variant = 3; CHECK(refused(&p, &in, g_out, g_bgr, "variant"));
    // a selected guide's pointer; one that is not selected is not looked at
    p = good_params();
    in = good_inputs(); in.rgb = nullptr; CHECK(refused(&p, &in, g_out, g_bgr, "rgb"));
    in = good_inputs(); in.normal = nullptr; CHECK(refused(&p, &in, g_out, g_bgr, "guide"));
    in = good_inputs(); in.depth = nullptr; CHECK(refused(&p, &in, g_out, g_bgr, "guide"));
    in = good_inputs(); in.albedo = nullptr; CHECK(refused(&p, &in, g_out, g_bgr, "guide"));
    p.flags = 0; p.sigma_color = p.sigma_depth = 0.0;           // a plain blur reads neither guides nor sigmas
    in = rt_denoise_inputs{g_rgb, nullptr, nullptr, nullptr};
    CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p.flags = RT_DN_NORMAL; in.normal = g_normal; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    // a selected sigma: finite and > 0
    in = good_inputs();
    const double bad[] = {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
    for (double v : bad) {
        p = good_params(); p.sigma_depth = v; CHECK(refused(&p, &in, g_out, g_bgr, "sigma_depth"));
        p.flags &= ~static_cast<uint32_t>(RT_DN_DEPTH); CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
        p = good_params(); p.sigma_color = v; CHECK(refused(&p, &in, g_out, g_bgr, "sigma_color"));
        p.flags &= ~static_cast<uint32_t>(RT_DN_COLOR); CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    }
    p = good_params(); p.sigma_depth = 5e-324; p.sigma_color = 1e308; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    // outputs and pitch
    p = good_params();
    CHECK(refused(&p, &in, nullptr, nullptr, "outputs"));
    p.bgr_pitch = 3 * 70 - 1; CHECK(refused(&p, &in, g_out, g_bgr, "bgr_pitch"));
    p.bgr_pitch = 3 * 70; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p.bgr_pitch = 3 * 70 + 2; CHECK(plan_denoise_args(&p, &in, g_out, g_bgr, &why) == RT_OK);
    p = good_params(); p.width = 0x60000000u; p.bgr_pitch = 0x20000001u;      // 3 * width wraps in 32 bits
    CHECK(refused(&p, &in, g_out, g_bgr, "bgr_pitch"));
    p = good_params();
    CHECK(refused(&p, &in, g_rgb, g_bgr, "out_rgb"));
    // the order: the first failing check of the header's list answers
    p = good_params(); p.width = 0; p.iterations = 0; CHECK(refused(&p, &in, nullptr, nullptr, "width"));
    p = good_params(); p.variant = 9; CHECK(refused(&p, &in, nullptr, nullptr, "variant"));
}

static void plan_cases() {
    rt_denoise_params p = good_params();
    for (uint32_t variant = 0; variant <= 2; ++variant) {
        p.variant = variant;
        for (uint32_t it = 1; it <= 8; ++it) {
            p.iterations = it;
            const DenoisePlan d = plan_denoise(p);
            const uint32_t ran = variant ? variant : kDnAutoVariant;
            CHECK(d.passes == it && d.variant == ran);
            for (uint32_t i = 0; i < it; ++i) {
                CHECK(d.step[i] == (1u << i));
                CHECK(d.lds[i] == (ran == 2 && d.step[i] <= 2));
            }
        }
    }
    static_assert(kDnAutoVariant == 1 || kDnAutoVariant == 2, "auto is one of the two forms");
    static_assert(kDnLdsMaxStep == 2 && kDnRecordBytes == 16, "steps 1 and 2; one dwordx4 per record");
    // the LDS form's tile and halo at its largest step: two records per staged pixel, within a workgroup's 64 KB
    static_assert((kDnTileW + 4 * kDnLdsMaxStep) * (kDnTileH + 4 * kDnLdsMaxStep) * 2 * kDnRecordBytes <= 48 * 1024, "fits LDS");
    // grid: one workgroup per tile, ragged edges rounded up
    p = good_params();
    DenoisePlan d = plan_denoise(p);
    CHECK(d.grid_x == 2 && d.grid_y == 9);
    CHECK(d.image_bytes == 73984 && d.image_bytes % 256 == 0 && d.image_bytes >= 70ull * 66 * 16);
    CHECK(d.scratch_bytes == 3 * d.image_bytes);
    p.width = 1; p.height = 1; d = plan_denoise(p);
    CHECK(d.grid_x == 1 && d.grid_y == 1 && d.image_bytes == 256 && d.scratch_bytes == 768);
    p.width = 64; p.height = 8; d = plan_denoise(p);
    CHECK(d.grid_x == 1 && d.grid_y == 1);
    p.width = 65; p.height = 9; d = plan_denoise(p);
    CHECK(d.grid_x == 2 && d.grid_y == 2);
    p.width = 4096; p.height = 4096; d = plan_denoise(p);
    CHECK(d.grid_x == 64 && d.grid_y == 512 && d.image_bytes == 4096ull * 4096 * 16 && d.scratch_bytes == 3ull << 28);
    p.width = 1u << 20; p.height = 1u << 20; d = plan_denoise(p);           // no 32-bit wrap in the byte counts
    CHECK(d.image_bytes == 1ull << 44);
}

int main() {
    argument_cases();
    plan_cases();
    if (failures) {
        std::printf("denoise_plan_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("denoise_plan_check ok\n");
    return 0;
}
