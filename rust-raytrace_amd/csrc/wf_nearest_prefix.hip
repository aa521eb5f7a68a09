// wf_nearest through the binary BVH with the top of the tree in LDS (f32 or binary16 bounds).
#define RT_UNIT wf_nearest_prefix
#include "wf_nearest.hpp"

namespace rtamd {

template hipError_t launch_nearest_src<kSrcBvhP>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcBvhPH>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcBvhPHC>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);

RT_NEAREST_UNIT(wf_nearest_prefix)

}  // namespace rtamd
