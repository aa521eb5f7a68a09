// wf_nearest through the binary BVH, read whole: from HBM/L2, or staged in LDS with the spheres.
#define RT_UNIT wf_nearest_bvh
#include "wf_nearest.hpp"

namespace rtamd {

template hipError_t launch_nearest_src<kSrcBvhG>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcBvhL8>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcBvhL8C>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);

RT_NEAREST_UNIT(wf_nearest_bvh)

}  // namespace rtamd
