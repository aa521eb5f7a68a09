// Internal to the kernel translation units (launch_api.hpp is what the rest of the library sees):
// the launchers one kernel family offers the others, the choice of a kernel's template arguments
// from run-time flags (dispatch_bools), and what every code object carries (a warm-up launch,
// its copy of the sRGB table).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_layout.hpp"
#include "launch_api.hpp"

namespace rtamd {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for the run-time bools b0, b1, ...:
// a generic lambda receives them as constants, `auto kSky` used as `kSky()`.  Every combination of
// the lambda's body is instantiated, so a combination that has no kernel is excluded there with
// `if constexpr` (it then adds no kernel to the code object).
template <class F>
hipError_t dispatch_bools(F&& f) {
    return f();
}
template <class F, class... Bools>
hipError_t dispatch_bools(F&& f, bool b0, Bools... rest) {
    if (b0) return dispatch_bools([&](auto... cs) { return f(std::true_type{}, cs...); }, rest...);
    return dispatch_bools([&](auto... cs) { return f(std::false_type{}, cs...); }, rest...);
}

// wf_nearest of generation k from sphere source kSrc on stream s (wf_nearest.hpp; instantiated in
// the wf_nearest_*.hip unit of the source's group).  Generation 0 is the camera pass.
template <int kSrc>
hipError_t launch_nearest_src(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, bool count, hipStream_t s);

// wf_shade.hip: the shadow queries (source src_occ, or a light-grid source by grid_occ: see
// WfStreams) and the shading of generation k on stream sb; packed: the levels' layout.
hipError_t launch_shading(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int k, int src_occ, int grid_occ,
                          bool count, bool packed, hipStream_t sb, LaunchMarks* mb);

// wf_tail.hip: the fused tail from generation T on, `wgs` workgroups, `width` chains per wave (0: auto).
hipError_t launch_tail(const DevScene& sc, const FrameParams& fp, const WfBufs& b, int T, bool count, bool packed, int wgs,
                       int width, hipStream_t s);

// wf_fold.hip: a skybox scene's terminals, then the fold of the chains of lo <= nlev <= hi.
hipError_t launch_fold(const DevScene& sc, const FrameParams& fp, const WfBufs& b, hipStream_t s, LaunchMarks* m,
                       uint32_t lo, uint32_t hi, bool packed);

// wf_output.hip: a skybox scene's camera misses (no compose route); the frame, or the pass's
// samples, row by row from the pixel map (compose route).
hipError_t launch_sky_pixels(const DevScene& sc, const FrameParams& fp, const WfBufs& b, hipStream_t s, LaunchMarks* m);
hipError_t launch_compose(const DevScene& sc, const FrameParams& fp, const WfBufs& b, hipStream_t s);

// Every translation unit with kernels is a code object of its own, loaded by its first launch:
// RT_UNIT_WARM(unit) gives the unit an empty kernel and unit_warm_<unit>, which launches it
// (launch_warmup runs them all).  RT_UNIT_SRGB(unit) gives a unit that reads c_srgb_avg (it
// defines RT_UNIT for its copy, trace_types.hpp) the upload of that copy, unit_srgb_<unit>
// (upload_srgb_table runs them all).  The lists below name the units; wf_sequence.hip, which
// holds launch_warmup and the real warm-up kernel, is in none of them.
#define RT_NEAREST_UNITS(X) X(wf_nearest_flat) X(wf_nearest_bvh) X(wf_nearest_prefix) X(wf_nearest_q4)
#define RT_WARM_UNITS(X) X(trace_mega) RT_NEAREST_UNITS(X) X(wf_shade) X(wf_tail) X(wf_fold) X(wf_output) X(probes) X(wf_aov) X(wf_query) X(wf_denoise)
#define RT_SRGB_UNITS(X) X(trace_mega) RT_NEAREST_UNITS(X) X(wf_tail) X(wf_fold) X(wf_output) X(wf_denoise)

#define RT_UNIT_WARM(unit)                                  \
    namespace {                                             \
    __global__ void warm_##unit() {}                        \
    }                                                       \
    hipError_t unit_warm_##unit(hipStream_t s) {            \
        warm_##unit<<<dim3(1), dim3(64), 0, s>>>();         \
        return hipGetLastError();                           \
    }
#define RT_UNIT_SRGB(unit)                                                                   \
    hipError_t unit_srgb_##unit(const double* avg255) {                                      \
        return hipMemcpyToSymbol(HIP_SYMBOL(c_srgb_avg), avg255, 255 * sizeof(double));      \
    }

#define RT_X(unit) hipError_t unit_warm_##unit(hipStream_t s);
RT_WARM_UNITS(RT_X)
#undef RT_X
#define RT_X(unit) hipError_t unit_srgb_##unit(const double* avg255);
RT_SRGB_UNITS(RT_X)
#undef RT_X

}  // namespace rtamd
