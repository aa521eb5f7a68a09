// wf_nearest through the quantised 4-wide tree (whole, or its top, in LDS).
#define RT_UNIT wf_nearest_q4
#include "wf_nearest.hpp"

namespace rtamd {

template hipError_t launch_nearest_src<kSrcQ4>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);
template hipError_t launch_nearest_src<kSrcQ4P>(const DevScene&, const FrameParams&, const WfBufs&, int, bool, hipStream_t);

RT_NEAREST_UNIT(wf_nearest_q4)

}  // namespace rtamd
