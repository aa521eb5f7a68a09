// The types and constants every device unit shares: the per-unit sRGB table and its quantiser,
// the reference's constants, Ray / Hit / Col and the work counters.
//
// Exactness: every operation is the reference's f64 operation in the
// reference's order, compiled with -ffp-contract=off (no FMA fusion; Rust never
// fuses).  f64 add/mul/div/sqrt are IEEE correctly rounded on gfx950, so the
// only possible difference from the CPU is pow() (raytrace.rs:55): OCML vs
// glibc, <= 1 ulp (measured through rt_shade_check, tests/test_gpu_prims.py: at most one
// representable value from correctly rounded; bit-identical on every parity scene so far).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtamd {

// The sRGB quantisation table (host_color.cpp), one copy per code object that reads it: without
// relocatable device code a translation unit's kernels see only its own.  Such a unit defines
// RT_UNIT (its name) before its includes and gets its copy here, under a name of its own so that
// the copies link into one library (upload_srgb_table fills them all: wf_launch.hpp,
// RT_SRGB_UNITS).  External linkage on purpose: an internal table that the host also names is
// addressed through the GOT, a load more in every kernel that reads it.
#ifdef RT_UNIT
#define RT_CAT_(a, b) a##b
#define RT_CAT(a, b) RT_CAT_(a, b)
#define c_srgb_avg RT_CAT(c_srgb_avg_, RT_UNIT)
__constant__ double c_srgb_avg[255];
#else
extern __constant__ double c_srgb_avg[255];     // (a unit that never reads it)
#endif

constexpr double kMinSignificance = 1.0 / 256.0 / 2.0;            // raytrace.rs:17
constexpr double kEps = 0.00001;                                   // raytrace.rs:43,62
constexpr double kFrac1Pi = 0.318309886183790671537767526745028724; // f64::consts::FRAC_1_PI

struct Ray {
    double ox, oy, oz, dx, dy, dz;
};

struct Hit {
    double t;
    int32_t obj;        // object id, INT32_MAX = no hit
    int32_t prim;       // sphere index (>= 0) or ~plane index (< 0)
    bool nan_t;
};

struct Col {
    double r, g, b;
};

// Work counters (only in the kCount instantiations): boxes = slab tests,
// spheres = exact quadratic tests.
struct Work {
    uint32_t boxes = 0, spheres = 0;
#if RT_STAMP
    unsigned long long cyc[3] = {0, 0, 0};     // RT_STAMP builds: nearest_bvh_bl's descend / leaf / pop loops
    uint32_t wsteps[3] = {0, 0, 0};            // ... and the wave's iterations of them (counted by its first active lane)
#endif
};
#if RT_STAMP
#define RT_WSTAMP(v)                                                              \
    do {                                                                          \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");              \
        v = __builtin_amdgcn_s_memtime();                                         \
    } while (0)
#define RT_WSTEP(i) \
    do {                                                                          \
        if (static_cast<unsigned>(__builtin_amdgcn_readfirstlane(__lane_id())) == __lane_id()) ++w->wsteps[i]; \
    } while (0)
#else
#define RT_WSTAMP(v) ((void)0)
#define RT_WSTEP(i) ((void)0)
#endif

__device__ __forceinline__ double clamp_zero(double x) { return x < 0.0 ? 0.0 : x; }   // raytrace.rs:20-23

// color.rs:593-600 as a binary search over the strictly increasing table.
__device__ __forceinline__ uint8_t to_srgb(double v, const double* table) {
    if (!(v < table[254])) return 255;           // also NaN
    int lo = 0, hi = 254;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int mid = (lo + hi) >> 1;
        bool lt = v < table[mid];
        hi = lt ? mid : hi;
        lo = lt ? lo : mid + 1;
    }
    return static_cast<uint8_t>(lo);
}

__device__ __forceinline__ uint8_t to_srgb(double v) { return to_srgb(v, c_srgb_avg); }

}  // namespace rtamd
