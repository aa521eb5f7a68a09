// Device-side exact restatement of the reference's per-ray math, shared by the
// megakernel (trace_mega.hip), the wavefront kernels (wf_*.hip) and the path kernel
// (path_kernel.hip).  This file only gathers the topical headers, in dependency order;
// a unit that needs one part may include that part alone (after device_layout.hpp):
//   trace_types.hpp   the note on exactness, the sRGB table and quantiser, Ray / Hit / Col / Work
//   trace_rng.hpp     the keyed RNG
//   trace_prims.hpp   exact division and square root, sphere and plane tests, the brute-force scans
//   trace_view.hpp    BvhView, the staged grid headers, the LDS node layouts
//   trace_bvh.hpp     slab tests, traversal stacks, the three walks of the binary tree
//   trace_bvh4.hpp    the 4-wide tree and the quantised 4-wide tree
//   trace_grid.hpp    the light-view grids and the camera's view grid
//   trace_shade.hpp   normals, light directions, material flags, one light's terms, reflection
//   trace_frame.hpp   camera ray, pixel writer, the background (the skybox sampler's one copy)
#pragma once

#include "device_layout.hpp"
#include "trace_types.hpp"
#include "trace_rng.hpp"
#include "trace_prims.hpp"
#include "trace_view.hpp"
#include "trace_bvh.hpp"
#include "trace_bvh4.hpp"
#include "trace_grid.hpp"
#include "trace_shade.hpp"
#include "trace_frame.hpp"
