// Where a traversal reads its data: BvhView (LDS copies or HBM/L2), the staged grid headers,
// and the LDS node layouts with their fetch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_layout.hpp"

namespace rtamd {

// A DevLightGrid header as the grid sources keep it in LDS: the per-face fields re-packed so
// that one face's five words sit together (one ds_read_b128 and one ds_read_b32), the rest in
// the 48 bytes before them.  240 B per grid.
struct alignas(16) LdsGridFace {
    int32_t fx0, fy0, fw, fh;
    uint32_t off_base;
    uint32_t _pad[3];
};
struct alignas(16) LdsGridHdr {
    double lx, ly, lz;
    int32_t R;
    uint32_t always_begin, always_end;
    uint32_t _pad[3];
    LdsGridFace face[6];
};
static_assert(sizeof(LdsGridFace) == 32 && sizeof(LdsGridHdr) == 240, "LDS grid header layout");
// Planes beyond this many stay in L2 (a grid source then reads them as before): 8 * (48 + 4) B
// of LDS at the most, next to the spheres' tens of KB.
constexpr int32_t kStagedPlanes = 8;

// Where the traversal reads its data: the first `nl` BVH nodes (breadth-first
// order, i.e. the top of the tree) from an LDS copy, the rest from HBM/L2;
// spheres and their object ids from LDS when the whole list fits, else HBM.
struct BvhView {
    const float2* lnodes;        // LDS nodes, axis-pair-major (stage_node_planes): 6 bound-pair arrays then the child pairs
    int32_t nl;
    const DevBvhNode* pnodes;    // prefix sources: nodes [0, nl) in LDS as DevBvhNode (array of nodes)
    const DevBvhNode* gnodes;
    const DevSphere* sph;
    const int32_t* obj;
    const DevBvh4Plane* p4;      // 4-wide tree planes (LDS or HBM), stride n4
    int32_t n4;
    const DevBvhNodeH* hpnodes;  // half-node prefix source: nodes [0, nl) in LDS (binary16 bounds)
    const DevBvhNodeH* hgnodes;  // ... and the whole half-node tree in HBM/L2
    const DevQNode4* q4l;        // quantised 4-wide tree: nodes [0, nq) in LDS, the rest from q4g (HBM/L2)
    const DevQNode4* q4g;
    int32_t nq;
    // The scene constants of a grid source (stage_grid_consts, wf_device.hpp), all in LDS; null
    // where the kernel stages none, and the helpers then read them through L2 as before.
    const LdsGridHdr* ghdr;      // one header per light (shadow grids) or the camera grid's one
    const DevLight* llights;     // the lights (shadow grid sources only)
    const DevPlane* lplanes;     // the planes and their object ids, when n_planes <= kStagedPlanes
    const int32_t* lplane_obj;
};

// The view of the scene's trees and spheres in HBM (what a source does not stage in LDS).
__device__ __forceinline__ BvhView global_view(const DevScene& sc) {
    BvhView v{};
    v.gnodes = sc.bvh;
    v.sph = sc.spheres;
    v.obj = sc.sphere_obj;
    v.p4 = sc.bvh4;
    v.n4 = sc.n_bvh4;
    v.q4g = sc.q4;
    return v;
}

// LDS copy of binary nodes [0, n), AXIS-PAIR-MAJOR: for axis a the lo_a
// bounds of the two children of node i as one pair at L[(2a) * n + i] and
// the hi_a bounds at L[(2a + 1) * n + i] (float2), the child pair at
// ((int2*)(L + 6n))[i]; 56 B per node.  A ray reads only the pairs its slab
// test needs: per axis the NEAR pair (lo when 1/d_a >= 0, else hi) and the
// FAR pair, both children at once (nearest_bvh_bl), and every 8-B read of a
// wave spreads over all 32 8-B bank slots (the pair arrays have an 8-B stride).
__host__ __device__ constexpr size_t node_planes_bytes(int32_t n) { return (static_cast<size_t>(n) * 56u + 15u) / 16u * 16u; }

// kByteOff (nearest_bvh_bl's walk): an inner child c is stored as the byte
// offset (c + 1) * 8 of its pairs, so a visit addresses every array with one add
// and no shift, and 0 (an inline constant) is free to mean "no node"; leaf codes
// (negative) are unchanged.
__host__ __device__ constexpr int32_t node_byte_off(int32_t c) { return c >= 0 ? (c + 1) * 8 : c; }

template <int kThreads, bool kByteOff = false>
__device__ __forceinline__ const float2* stage_node_planes(const DevBvhNode* src, int32_t n, unsigned char* lds) {
    float2* L = reinterpret_cast<float2*>(lds);
    int2* C = reinterpret_cast<int2*>(L + 6 * n);
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const DevBvhNode nd = src[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            L[(2 * a) * n + i] = make_float2(nd.lo0[a], nd.lo1[a]);
            L[(2 * a + 1) * n + i] = make_float2(nd.hi0[a], nd.hi1[a]);
        }
        C[i] = kByteOff ? make_int2(node_byte_off(nd.c0), node_byte_off(nd.c1)) : make_int2(nd.c0, nd.c1);
    }
    return L;
}

__device__ __forceinline__ DevBvhNode lds_node(const float2* L, int32_t n, int32_t i) {
    DevBvhNode nd;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float2 lo = L[(2 * a) * n + i], hi = L[(2 * a + 1) * n + i];
        nd.lo0[a] = lo.x; nd.lo1[a] = lo.y;
        nd.hi0[a] = hi.x; nd.hi1[a] = hi.y;
    }
    const int2 cc = reinterpret_cast<const int2*>(L + 6 * n)[i];
    nd.c0 = cc.x; nd.c1 = cc.y;
    return nd;
}

__device__ __forceinline__ float half_bits_f(uint16_t h) {
    return static_cast<float>(__builtin_bit_cast(_Float16, h));     // exact (v_cvt_f32_f16)
}

// kNodes: 0 = every node from HBM/L2, 1 = LDS prefix + HBM, 2 = every node in LDS,
// 3 = LDS prefix + HBM of binary16 nodes (DevBvhNodeH, bounds rounded outward:
// decoded exactly, each box contains the f32 node's box)
template <int kNodes>
__device__ __forceinline__ DevBvhNode fetch_node(const BvhView& v, int32_t i) {
    if constexpr (kNodes == 3) {
        const DevBvhNodeH h = *(i < v.nl ? v.hpnodes + i : v.hgnodes + i);
        DevBvhNode nd;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            nd.lo0[a] = half_bits_f(h.b[a]); nd.hi0[a] = half_bits_f(h.b[3 + a]);
            nd.lo1[a] = half_bits_f(h.b[6 + a]); nd.hi1[a] = half_bits_f(h.b[9 + a]);
        }
        nd.c0 = h.c0; nd.c1 = h.c1;
        return nd;
    } else if constexpr (kNodes == 2) {
        return lds_node(v.lnodes, v.nl, i);
    } else if constexpr (kNodes == 1) {
        // one flat load from LDS or HBM/L2: the same layout on both sides, so no
        // divergent branch (a plane-major prefix measured C4 70.8 -> 79.0 ms)
        return *(i < v.nl ? v.pnodes + i : v.gnodes + i);
    } else {
        return v.gnodes[i];
    }
}

}  // namespace rtamd
