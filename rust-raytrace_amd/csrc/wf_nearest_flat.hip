// wf_nearest without a tree: the sphere list (brute force) and the camera's view grid.
#define RT_UNIT wf_nearest_flat
#include "wf_nearest.hpp"

namespace rtamd {

template hipError_t launch_nearest_src<kSrcGlobal>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcLds>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcCamGridL>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcCamGridG>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);

RT_NEAREST_UNIT(wf_nearest_flat)

}  // namespace rtamd
