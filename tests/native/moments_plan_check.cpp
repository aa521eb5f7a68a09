// CPU check of the planner's rules for moments accumulators (csrc/render_plan.cpp alone: no
// HIP, no GPU): which calls each kind of accumulator refuses, the noise calls' argument checks, the device
// buffer's size with its overflow.  The expected values follow from the rules in include/raytrace_amd.h.  (The
// checkpoint file's own size arithmetic is host_checkpoint.cpp's, checked by checkpoint2_check.cpp.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
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

static void call_cases() {
    const char* err = nullptr;
    // a plain accumulator: rt_accum_upload as before; nothing that needs the squares
    CHECK(plan_accum_call(AccumCall::upload, false, &err) == RT_OK);
    for (AccumCall c : {AccumCall::upload_moments, AccumCall::download_moments, AccumCall::noise}) {
        err = nullptr;
        CHECK(plan_accum_call(c, false, &err) == RT_E_INVALID && err && std::strstr(err, "rt_accum_create_moments"));
        CHECK(plan_accum_call(c, true, &err) == RT_OK);
    }
    // a moments accumulator: the sums alone cannot be replaced
    err = nullptr;
    CHECK(plan_accum_call(AccumCall::upload, true, &err) == RT_E_INVALID && err && std::strstr(err, "stale"));
}

static void noise_cases() {
    const char* err = nullptr;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(plan_noise(true, 2, 1e-3, 0.05, &err) == RT_OK);
    CHECK(plan_noise(true, 1u << 31, 4.9e-324, 1.7e308, &err) == RT_OK);       // any finite value > 0
    err = nullptr;
    CHECK(plan_noise(false, 8, 1e-3, 0.05, &err) == RT_E_INVALID && err);
    for (uint32_t n : {0u, 1u}) {
        err = nullptr;
        CHECK(plan_noise(true, n, 1e-3, 0.05, &err) == RT_E_INVALID && err && std::strstr(err, "2 samples"));
    }
    for (double bad : {0.0, -0.0, -1.0, inf, -inf, nan}) {
        err = nullptr;
        CHECK(plan_noise(true, 4, bad, 0.05, &err) == RT_E_INVALID && err && std::strstr(err, "floor"));
        err = nullptr;
        CHECK(plan_noise(true, 4, 1e-3, bad, &err) == RT_E_INVALID && err && std::strstr(err, "threshold"));
    }
}

static void size_cases() {
    uint64_t d = 0;
    CHECK(plan_accum_doubles(0, false, &d) && d == 0);
    CHECK(plan_accum_doubles(0, true, &d) && d == 0);
    CHECK(plan_accum_doubles(48 * 32, false, &d) && d == 3 * 48 * 32);          // 24 B per pixel
    CHECK(plan_accum_doubles(48 * 32, true, &d) && d == 6 * 48 * 32);           // 48 B per pixel
    // a tile of 2^29 x 2^29 pixels still fits 64 bits with moments; the largest the options can name, 2^32 - 1 on
    // each side, does not, with or without them
    CHECK(plan_accum_doubles(1ull << 58, true, &d) && d == 6ull << 58);
    const uint64_t side = 0xFFFFFFFFull;
    CHECK(!plan_accum_doubles(side * side, true, &d) && !plan_accum_doubles(side * side, false, &d));
    // ... nor need a pixel count from a file: 2^59 pixels are 24 * 2^59 bytes of sums, and 48 * 2^59 wraps
    CHECK(plan_accum_doubles(1ull << 59, false, &d) && d == 3ull << 59);
    d = 7;
    CHECK(!plan_accum_doubles(1ull << 59, true, &d) && d == 7);
    CHECK(!plan_accum_doubles(1ull << 60, false, &d));
    CHECK(!plan_accum_doubles(1ull << 61, false, &d) && !plan_accum_doubles(1ull << 61, true, &d));
    CHECK(plan_accum_doubles(UINT64_MAX / 24, false, &d) && !plan_accum_doubles(UINT64_MAX / 24 + 1, false, &d));
    CHECK(plan_accum_doubles(UINT64_MAX / 48, true, &d) && !plan_accum_doubles(UINT64_MAX / 48 + 1, true, &d));
}

int main() {
    call_cases();
    noise_cases();
    size_cases();
    // an accumulating call's own rules are as they were, whatever the kind of accumulator
    static_assert(kAccumFlags == (RT_COUNT_WORK | RT_TIME_KERNELS), "the two flags the header allows");
    static_assert(kAccumMaxSamples == 1u << 31, "the header's bound");
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("moments_plan_check ok\n");
    return 0;
}
