// C ABI: scene upload to HBM (rt_scene_upload) and the host-only diagnostics that build the
// same grids and trees (rt_light_grid_candidates, rt_view_grid_candidates, rt_qtree_nodes).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "bvh_build.hpp"
#include "rt_ctx.hpp"

using namespace rtamd;

namespace {

static_assert(kMatPhong == RT_MAT_PHONG && kMatFresnel == RT_MAT_FRESNEL && kMatIndirect == RT_MAT_INDIRECT_PHONG &&
                  kMatTransparent == RT_MAT_TRANSPARENT,
              "DevMaterial::kind mirrors rt_material_kind");
static_assert(kLightArea == RT_LIGHT_AREA, "DevLight::kind mirrors rt_light_kind");

}  // namespace

extern "C" {

int rt_light_grid_candidates(const rt_scene* s, int light, int resolution, const double* points, uint32_t n_points,
                             int32_t* counts, int32_t* ids, size_t cap, int64_t* info) {
    if (!s || (n_points && (!points || !counts)) || (cap && !ids)) return RT_E_INVALID;
    if (light < 0 || light >= static_cast<int>(s->lights.size()) || resolution < 0 || resolution > 4096)
        return RT_E_INVALID;
    try {
        std::vector<DevSphere> spheres;
        std::vector<double> srad;
        std::vector<int32_t> obj;
        double extent = 0.0;
        for (size_t i = 0; i < s->objects.size(); ++i) {
            const rt_object& o = s->objects[i];
            if (o.shape != RT_SHAPE_SPHERE) continue;
            spheres.push_back(DevSphere{o.geom[0], o.geom[1], o.geom[2], sphere_rr(o.geom[3])});
            srad.push_back(o.geom[3]);
            obj.push_back(static_cast<int32_t>(i));
            const double r = std::fabs(o.geom[3]);
            for (int k = 0; k < 3; ++k)
                for (double v : {o.geom[k] - r, o.geom[k] + r})
                    if (std::isfinite(v)) extent = std::max(extent, std::fabs(v));
        }
        std::vector<DevLight> lights;
        for (const rt_light& l : s->lights) {
            DevLight d{};
            for (int k = 0; k < 9; ++k) d.v[k] = l.v[k];
            d.kind = l.kind;
            lights.push_back(d);
        }
        const LightGridResult lg = build_light_grids(spheres, srad, lights, 1e-5 * (1.0 + extent), resolution);
        if (info) {
            info[0] = lg.grids[light].R;
            int64_t cells = 0;
            for (int f = 0; f < 6; ++f) cells += static_cast<int64_t>(lg.grids[light].fw[f]) * lg.grids[light].fh[f];
            info[1] = cells;
            info[2] = static_cast<int64_t>(lg.ent.size());
        }
        std::vector<int32_t> cand;
        size_t used = 0;
        for (uint32_t i = 0; i < n_points; ++i) {
            if (!light_grid_candidates(lg, light, points + 3 * i, cull_reach(extent), cand)) { counts[i] = -1; continue; }
            counts[i] = static_cast<int32_t>(cand.size());
            for (int32_t k : cand) {
                if (used == cap) return fail(nullptr, RT_E_INVALID, "candidate buffer too small");
                ids[used++] = obj[k];
            }
        }
        return RT_OK;
    } catch (const std::exception& e) {
        return fail(nullptr, RT_E_NOMEM, e.what());
    }
}

// The view grid's automatic resolution: a cell about 8 x 8 pixels of the scene's frame.
static int view_grid_res(const rt_scene* s, int64_t forced) {
    if (forced > 0) return static_cast<int>(forced);
    const double* M = s->camera.matrix;
    const double imd = std::sqrt(M[2] * M[2] + M[5] * M[5] + M[8] * M[8]);
    const double side = static_cast<double>(std::max(std::max(s->width, s->height), 64u));
    return std::isfinite(imd) ? static_cast<int>(std::lround(std::clamp(imd * side / 8.0, 16.0, 2048.0))) : 64;
}
constexpr size_t kViewGridEntries = size_t{32} << 20;
// the view grid's list entries: at most 32 M, and about 4096 per sphere (C3 holds 395 per sphere)
static size_t view_grid_cap(size_t n_spheres) { return std::min(kViewGridEntries, (size_t{1} << 20) + 4096 * n_spheres); }

int rt_view_grid_candidates(const rt_scene* s, int resolution, const double* dirs, uint32_t n_dirs, int32_t* counts,
                            int32_t* ids, float* nears, size_t cap, int64_t* info) {
    if (!s || (n_dirs && (!dirs || !counts)) || (cap && (!ids || !nears)) || resolution < 0 || resolution > 4096)
        return RT_E_INVALID;
    try {
        std::vector<DevSphere> spheres;
        std::vector<double> srad;
        std::vector<int32_t> obj;
        double extent = 0.0;
        for (size_t i = 0; i < s->objects.size(); ++i) {
            const rt_object& o = s->objects[i];
            if (o.shape != RT_SHAPE_SPHERE) continue;
            spheres.push_back(DevSphere{o.geom[0], o.geom[1], o.geom[2], sphere_rr(o.geom[3])});
            srad.push_back(o.geom[3]);
            obj.push_back(static_cast<int32_t>(i));
            const double r = std::fabs(o.geom[3]);
            for (int k = 0; k < 3; ++k)
                for (double v : {o.geom[k] - r, o.geom[k] + r})
                    if (std::isfinite(v)) extent = std::max(extent, std::fabs(v));
        }
        // as rt_scene_upload: no grid for a camera beyond the culling domain (every ray: -1)
        const double* cpos = s->camera.position;
        LightGridResult g;
        if (beyond_reach(cpos, cull_reach(extent))) g.grids.push_back(DevLightGrid{});
        else g = build_view_grid(spheres, srad, cpos, 1e-5 * (1.0 + extent), view_grid_res(s, resolution),
                                 view_grid_cap(spheres.size()));
        const DevLightGrid& G = g.grids[0];
        if (info) {
            info[0] = G.R;
            int64_t cells = 0;
            for (int f = 0; f < 6; ++f) cells += static_cast<int64_t>(G.fw[f]) * G.fh[f];
            info[1] = cells;
            info[2] = static_cast<int64_t>(g.ent.size());
        }
        size_t used = 0;
        auto put = [&](const DevLgEntry& e) {
            if (used == cap) throw std::length_error("candidate buffer too small");
            ids[used] = obj[e.sph];
            nears[used++] = e.near;
        };
        for (uint32_t i = 0; i < n_dirs; ++i) {
            const size_t before = used;
            for (uint32_t e = G.always_begin; e < G.always_end; ++e) put(g.ent[e]);
            // the device's lookup (nearest_cgrid): f32 direction, dominant axis, clamped cell
            const float dx = static_cast<float>(dirs[3 * i]), dy = static_cast<float>(dirs[3 * i + 1]),
                        dz = static_cast<float>(dirs[3 * i + 2]);
            const float ax = std::fabs(dx), ay = std::fabs(dy), az = std::fabs(dz);
            const int fa = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
            const float da = fa == 0 ? dx : fa == 1 ? dy : dz;
            const float db = fa == 0 ? dy : fa == 1 ? dz : dx;
            const float dc = fa == 0 ? dz : fa == 1 ? dx : dy;
            if (G.R <= 0 || !(std::fabs(da) > 0.0f && std::fabs(da) < 3.0e38f)) { counts[i] = -1; used = before; continue; }
            const int f = 2 * fa + (da < 0.0f ? 1 : 0);
            const float inv = 1.0f / std::fabs(da);
            const float R = static_cast<float>(G.R);
            const int ci = std::min(std::max(static_cast<int>(std::floor((db * inv + 1.0f) * 0.5f * R)), 0), G.R - 1);
            const int cj = std::min(std::max(static_cast<int>(std::floor((dc * inv + 1.0f) * 0.5f * R)), 0), G.R - 1);
            const int li = ci - G.fx0[f], lj = cj - G.fy0[f];
            if (li >= 0 && lj >= 0 && li < G.fw[f] && lj < G.fh[f]) {
                const uint32_t cell = G.off_base[f] + static_cast<uint32_t>(lj * G.fw[f] + li);
                for (uint32_t e = g.off[cell]; e < g.off[cell + 1]; ++e) put(g.ent[e]);
            }
            counts[i] = static_cast<int32_t>(used - before);
        }
        return RT_OK;
    } catch (const std::length_error& e) {
        return fail(nullptr, RT_E_INVALID, e.what());
    } catch (const std::exception& e) {
        return fail(nullptr, RT_E_NOMEM, e.what());
    }
}

int rt_qtree_nodes(const rt_scene* s, int leaf_max, void* nodes, float* boxes, int32_t* sphere_first,
                   int32_t* sphere_count, size_t cap_nodes, int64_t* info) {
    if (!s || leaf_max < 0 || leaf_max > 8 || (cap_nodes && (!nodes || !boxes || !sphere_first || !sphere_count)))
        return RT_E_INVALID;
    try {
        std::vector<double> sx, sy, sz, srad;
        double extent = 0.0;
        for (const rt_object& o : s->objects) {
            if (o.shape != RT_SHAPE_SPHERE) continue;
            sx.push_back(o.geom[0]); sy.push_back(o.geom[1]); sz.push_back(o.geom[2]); srad.push_back(o.geom[3]);
            const double r = std::fabs(o.geom[3]);
            for (int k = 0; k < 3; ++k)
                for (double v : {o.geom[k] - r, o.geom[k] + r})
                    if (std::isfinite(v)) extent = std::max(extent, std::fabs(v));
        }
        const double pad = 1e-5 * (1.0 + extent);
        // the quantised tree's leaf rule (scene_upload with tuning qtree): 2, or 4 when that tree
        // and the spheres would not fit the LDS budget
        int leaf = leaf_max > 0 ? leaf_max : 2;
        BvhResult bvh = build_sphere_bvh(sx, sy, sz, srad, pad, leaf);
        if (leaf_max == 0 && bvh.nodes.size() * sizeof(DevBvhNode) + sx.size() * (sizeof(DevSphere) + 4) > kLdsBudget)
            bvh = build_sphere_bvh(sx, sy, sz, srad, pad, leaf = 4);
        const Bvh4Result b4 = collapse_bvh4(bvh);
        const int need = bvh4_stack_need(b4);
        const std::vector<DevQNode4> q = need <= kQ4Stack ? quantize_bvh4(b4) : std::vector<DevQNode4>{};
        if (info) { info[0] = static_cast<int64_t>(q.size()); info[1] = need; info[2] = leaf; }
        if (cap_nodes == 0) return RT_OK;                  // a size query: info[] alone
        if (q.size() > cap_nodes) return fail(nullptr, RT_E_INVALID, "node buffer too small");
        if (q.empty()) return RT_OK;
        const int32_t N = b4.n_nodes;
        std::memcpy(nodes, q.data(), q.size() * sizeof(DevQNode4));
        for (size_t i = 0; i < q.size(); ++i)
            for (int k = 0; k < 4; ++k) {
                const int32_t ch = b4.planes[static_cast<size_t>(6) * N + i].i[k];
                for (int a = 0; a < 3; ++a) {
                    boxes[(i * 4 + k) * 6 + a] = ch == kBvh4Empty ? NAN : b4.planes[static_cast<size_t>(2 * a) * N + i].f[k];
                    boxes[(i * 4 + k) * 6 + 3 + a] = ch == kBvh4Empty ? NAN : b4.planes[static_cast<size_t>(2 * a + 1) * N + i].f[k];
                }
                const bool leafc = ch != kBvh4Empty && ch < 0;
                sphere_first[i * 4 + k] = leafc ? (~ch) >> 3 : -1;
                sphere_count[i * 4 + k] = leafc ? ((~ch) & 7) + 1 : 0;
            }
        return RT_OK;
    } catch (const std::exception& e) {
        return fail(nullptr, RT_E_NOMEM, e.what());
    }
}

static int scene_upload(rt_ctx* c, const rt_scene* s) {
    HIP_TRY(c, hipSetDevice(c->device));
    // Every class of the reference has a device implementation: Phong / Fresnel
    // chains on the wavefront path, under a solid or a skybox background, the
    // stochastic and branching classes on the path kernel (needs_path).
    if (s->background_kind != RT_BG_SOLID && s->background_kind != RT_BG_SKYBOX)
        return fail(c, RT_E_INVALID, "bad background kind");
    const bool skybox = s->background_kind == RT_BG_SKYBOX;
    if (skybox)
        for (const HostTexture& t : s->skybox)
            if (t.width == 0 || t.height == 0 || t.rgb.size() != static_cast<size_t>(t.width) * t.height * 3)
                return fail(c, RT_E_INVALID, "skybox face without texels");
    if (s->camera.kind != RT_CAMERA_SIMPLE && s->camera.kind != RT_CAMERA_DOF)
        return fail(c, RT_E_INVALID, "bad camera kind");
    if (s->camera.kind == RT_CAMERA_DOF && s->camera.samples == 0)
        return fail(c, RT_E_INVALID, "DepthOfFieldCamera with 0 samples");
    bool needs_path = s->camera.kind == RT_CAMERA_DOF;
    std::vector<DevSphere> spheres;
    std::vector<double> sx, sy, sz, srad;
    std::vector<int32_t> sphere_obj, plane_obj;
    std::vector<DevPlane> planes;
    std::vector<DevMaterial> mats(s->objects.size());
    std::vector<DevLight> lights;
    for (size_t i = 0; i < s->objects.size(); ++i) {
        const rt_object& o = s->objects[i];
        if (o.material < RT_MAT_PHONG || o.material > RT_MAT_TRANSPARENT)
            return fail(c, RT_E_INVALID, "object " + std::to_string(i) + ": bad material kind");
        needs_path |= o.material == RT_MAT_INDIRECT_PHONG || o.material == RT_MAT_TRANSPARENT;
        if (o.shape == RT_SHAPE_SPHERE) {
            spheres.push_back(DevSphere{o.geom[0], o.geom[1], o.geom[2], sphere_rr(o.geom[3])});
            sphere_obj.push_back(static_cast<int32_t>(i));
            sx.push_back(o.geom[0]); sy.push_back(o.geom[1]); sz.push_back(o.geom[2]); srad.push_back(o.geom[3]);
        } else if (o.shape == RT_SHAPE_PLANE) {
            planes.push_back(DevPlane{o.geom[0], o.geom[1], o.geom[2], o.geom[3], o.geom[4], o.geom[5]});
            plane_obj.push_back(static_cast<int32_t>(i));
        } else {
            return fail(c, RT_E_INVALID, "object " + std::to_string(i) + ": bad shape kind");
        }
        DevMaterial& m = mats[i];
        std::memset(&m, 0, sizeof m);
        const rt_color* src[3] = {&o.diffuse, &o.specular, &o.ambient};
        double* dst[3] = {m.kd, m.ks, m.amb};
        for (int k = 0; k < 3; ++k) { dst[k][0] = src[k]->r; dst[k][1] = src[k]->g; dst[k][2] = src[k]->b; }
        m.exponent = o.exponent;
        m.kd_sig = significance(o.diffuse);
        m.ks_sig = significance(o.specular);
        m.ior = o.ior;
        m.kind = o.material;
        m.samples = o.material == RT_MAT_INDIRECT_PHONG ? o.samples : 0;
    }
    for (size_t i = 0; i < s->lights.size(); ++i) {
        const rt_light& l = s->lights[i];
        if (l.kind < RT_LIGHT_POINT || l.kind > RT_LIGHT_AREA)
            return fail(c, RT_E_INVALID, "light " + std::to_string(i) + ": bad light kind");
        needs_path |= l.kind == RT_LIGHT_AREA;
        DevLight d{};
        for (int k = 0; k < 9; ++k) d.v[k] = l.v[k];
        d.color[0] = l.color.r; d.color[1] = l.color.g; d.color[2] = l.color.b;
        d.kind = l.kind;
        lights.push_back(d);
    }
    // Sphere BVH; spheres (and their object ids) are stored in its leaf order.
    // Box padding scales with the largest sphere-box coordinate (BVH exactness).
    double extent = 0.0;
    for (size_t k = 0; k < spheres.size(); ++k) {
        const double r = std::fabs(srad[k]);
        for (double v : {sx[k] - r, sx[k] + r, sy[k] - r, sy[k] + r, sz[k] - r, sz[k] + r})
            if (std::isfinite(v)) extent = std::max(extent, std::fabs(v));
    }
    // Leaves of 2 spheres measured fastest at C3; 4 when that tree and the
    // spheres would not fit the traversal kernels' LDS budget (tuning "bvh_leaf" overrides).
    const double pad = 1e-5 * (1.0 + extent);
    const int leaf_env = static_cast<int>(c->t(kTuneBvhLeaf));
    BvhResult bvh = build_sphere_bvh(sx, sy, sz, srad, pad, leaf_env > 0 ? leaf_env : 2);
    // leaves of 2 whatever the tree's size (C4 49.4 vs 50.3 ms, C5 293.3 vs 297.1 ms with 4 on one
    // box); 4 only for the quantised tree (tuning qtree), whose C4 tree then fits the LDS
    if (leaf_env <= 0 && c->t(kTuneQTree) != 0 &&
        bvh.nodes.size() * sizeof(DevBvhNode) + spheres.size() * (sizeof(DevSphere) + 4) > kLdsBudget)
        bvh = build_sphere_bvh(sx, sy, sz, srad, pad, 4);
    const Bvh4Result bvh4 = collapse_bvh4(bvh);
    // traversal stacks hold 64 entries (trace_bvh.hpp kBvhStack / kBvh4Stack)
    if (bvh_depth(bvh) > 64) return fail(c, RT_E_UNSUPPORTED, "sphere BVH deeper than the traversal stack");
    c->deep_bvh4 = bvh4_stack_need(bvh4) > 64;
    // compact stack (trace_bvh.hpp kShortStack, stk_entry16): the stack never holds more
    // entries than the deepest inner node's depth; node indices and leaf codes
    // (first << 3 | count - 1) must fit a signed 16-bit field; the whole-LDS walk stores inner
    // nodes as byte offsets (c + 1) * 8 (trace_view.hpp node_byte_off)
    c->short_stack = bvh_depth(bvh) <= 32 && bvh.nodes.size() < 4095 && spheres.size() <= 4096;
    c->short_stack18 = bvh_depth(bvh) <= 32 && bvh.nodes.size() < 131072 && spheres.size() <= 16383;
    // binary16 nodes only for trees that do not fit LDS whole (the prefix source reads them)
    const bool big_tree = bvh.nodes.size() * sizeof(DevBvhNode) + spheres.size() * (sizeof(DevSphere) + 4) > kLdsBudget;
    const std::vector<DevBvhNodeH> hnodes = big_tree ? half_nodes(bvh) : std::vector<DevBvhNodeH>{};
    // the quantised 4-wide tree (nearest_q4's stack holds kQ4Stack entries), for every tree
    // (tuning qtree, or src 25 / 26, select it)
    const std::vector<DevQNode4> qnodes = bvh4_stack_need(bvh4) <= kQ4Stack ? quantize_bvh4(bvh4) : std::vector<DevQNode4>{};
    std::vector<double> r_leaf(spheres.size());
    {
        std::vector<DevSphere> s2(spheres.size());
        std::vector<int32_t> o2(spheres.size());
        for (size_t k = 0; k < spheres.size(); ++k) {
            s2[k] = spheres[bvh.order[k]]; o2[k] = sphere_obj[bvh.order[k]]; r_leaf[k] = srad[bvh.order[k]];
        }
        spheres.swap(s2);
        sphere_obj.swap(o2);
    }
    // light-view grids of the point lights (tuning: "light_grids" 0 disables, "light_grid_res" forces the resolution)
    LightGridResult lg;
    if (c->t(kTuneLgrid) != 0) lg = build_light_grids(spheres, r_leaf, lights, pad, static_cast<int>(c->t(kTuneLgridRes)));
    // the camera's view grid (generation 0, tuning "cam" 3): a cell about 8 x 8 pixels of the
    // scene's own frame size, im_dist * max(W, H) / 8 cells per face side (tuning "cam_grid_res");
    // only for scenes the wavefront schedule can render (the path kernel never reads it)
    LightGridResult cg;
    // ... and whose camera lies inside the culling domain (device_layout.hpp): from farther away the
    // padded boxes do not hold every hit the quadratic reports, and generation 0 walks the tree
    const float reach = cull_reach(extent);
    const double* cpos = s->camera.position;
    if (s->camera.kind == RT_CAMERA_SIMPLE && !needs_path && c->t(kTuneCamGridRes) >= 0 &&
        !beyond_reach(cpos, reach))
        cg = build_view_grid(spheres, r_leaf, s->camera.position, pad, view_grid_res(s, c->t(kTuneCamGridRes)),
                             view_grid_cap(spheres.size()));
    // One blob: [spheres][sphere_obj][planes][plane_obj][mats][lights][bvh], 256-B aligned pieces.
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t at = off; off = align_up(off + bytes, 256); return at; };
    const size_t o_sph = place(spheres.size() * sizeof(DevSphere));
    const size_t o_sobj = place(sphere_obj.size() * sizeof(int32_t));
    const size_t o_pl = place(planes.size() * sizeof(DevPlane));
    const size_t o_pobj = place(plane_obj.size() * sizeof(int32_t));
    const size_t o_mat = place(mats.size() * sizeof(DevMaterial));
    const size_t o_li = place(lights.size() * sizeof(DevLight));
    const size_t o_bvh = place(bvh.nodes.size() * sizeof(DevBvhNode));
    const size_t o_bvh4 = place(bvh4.planes.size() * sizeof(DevBvh4Plane));
    const size_t o_bvhh = place(hnodes.size() * sizeof(DevBvhNodeH));
    const size_t o_q4 = place(qnodes.size() * sizeof(DevQNode4));
    const size_t o_srgbv = place(256 * sizeof(double));
    const size_t o_lg = place(lg.grids.size() * sizeof(DevLightGrid));
    const size_t o_lgoff = place(lg.off.size() * sizeof(uint32_t));
    const size_t o_lgent = place(lg.ent.size() * sizeof(DevLgEntry));
    const size_t o_cg = place(cg.grids.size() * sizeof(DevLightGrid));
    const size_t o_cgoff = place(cg.off.size() * sizeof(uint32_t));
    const size_t o_cgent = place(cg.ent.size() * sizeof(DevLgEntry));
    size_t tex_bytes = 0;
    uint64_t face_off[6] = {0, 0, 0, 0, 0, 0};
    if (skybox)
        for (int k = 0; k < 6; ++k) { face_off[k] = tex_bytes; tex_bytes += s->skybox[k].rgb.size(); }
    const size_t o_tex = place(tex_bytes);
    const size_t total = off ? off : 256;
    std::vector<uint8_t> host(total, 0);
    auto put = [&](size_t at, const void* p, size_t bytes) { if (bytes) std::memcpy(host.data() + at, p, bytes); };
    put(o_sph, spheres.data(), spheres.size() * sizeof(DevSphere));
    put(o_sobj, sphere_obj.data(), sphere_obj.size() * sizeof(int32_t));
    put(o_pl, planes.data(), planes.size() * sizeof(DevPlane));
    put(o_pobj, plane_obj.data(), plane_obj.size() * sizeof(int32_t));
    put(o_mat, mats.data(), mats.size() * sizeof(DevMaterial));
    put(o_li, lights.data(), lights.size() * sizeof(DevLight));
    put(o_bvh, bvh.nodes.data(), bvh.nodes.size() * sizeof(DevBvhNode));
    put(o_bvh4, bvh4.planes.data(), bvh4.planes.size() * sizeof(DevBvh4Plane));
    put(o_bvhh, hnodes.data(), hnodes.size() * sizeof(DevBvhNodeH));
    put(o_q4, qnodes.data(), qnodes.size() * sizeof(DevQNode4));
    put(o_srgbv, srgb_values_table(), 256 * sizeof(double));
    put(o_lg, lg.grids.data(), lg.grids.size() * sizeof(DevLightGrid));
    put(o_lgoff, lg.off.data(), lg.off.size() * sizeof(uint32_t));
    put(o_lgent, lg.ent.data(), lg.ent.size() * sizeof(DevLgEntry));
    put(o_cg, cg.grids.data(), cg.grids.size() * sizeof(DevLightGrid));
    put(o_cgoff, cg.off.data(), cg.off.size() * sizeof(uint32_t));
    put(o_cgent, cg.ent.data(), cg.ent.size() * sizeof(DevLgEntry));
    if (skybox)
        for (int k = 0; k < 6; ++k) put(o_tex + face_off[k], s->skybox[k].rgb.data(), s->skybox[k].rgb.size());
    // every render still reading the old blob (on any stream) must be done before it is overwritten
    if (c->render_pending) HIP_TRY(c, hipEventSynchronize(c->render_done));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_blob && c->blob_bytes < total) { (void)hipFree(c->d_blob); c->d_blob = nullptr; c->blob_bytes = 0; }
    if (!c->d_blob) {
        HIP_TRY(c, hipMalloc(&c->d_blob, total));
        c->blob_bytes = total;
    }
    HIP_TRY(c, hipMemcpy(c->d_blob, host.data(), total, hipMemcpyHostToDevice));
    auto* base = static_cast<uint8_t*>(c->d_blob);
    DevScene& d = c->dsc;
    d = DevScene{};
    d.cull_reach = reach;
    d.spheres = reinterpret_cast<const DevSphere*>(base + o_sph);
    d.sphere_obj = reinterpret_cast<const int32_t*>(base + o_sobj);
    d.planes = reinterpret_cast<const DevPlane*>(base + o_pl);
    d.plane_obj = reinterpret_cast<const int32_t*>(base + o_pobj);
    d.mats = reinterpret_cast<const DevMaterial*>(base + o_mat);
    d.lights = reinterpret_cast<const DevLight*>(base + o_li);
    d.bvh = reinterpret_cast<const DevBvhNode*>(base + o_bvh);
    d.bvh_root = bvh.root;
    d.n_spheres = static_cast<int32_t>(spheres.size());
    d.n_planes = static_cast<int32_t>(planes.size());
    d.n_lights = static_cast<int32_t>(lights.size());
    d.n_bvh = static_cast<int32_t>(bvh.nodes.size());
    d.bvh4 = reinterpret_cast<const DevBvh4Plane*>(base + o_bvh4);
    d.bvh4_root = bvh4.root;
    d.n_bvh4 = bvh4.n_nodes;
    d.bvh_h = hnodes.empty() ? nullptr : reinterpret_cast<const DevBvhNodeH*>(base + o_bvhh);
    d.q4 = qnodes.empty() ? nullptr : reinterpret_cast<const DevQNode4*>(base + o_q4);
    d.n_q4 = static_cast<int32_t>(qnodes.size());
    c->q4_ok = !qnodes.empty();
    d.has_fresnel = 0;
    for (const DevMaterial& m : mats) d.has_fresnel |= m.kind == kMatFresnel ? 1 : 0;
    d.needs_path = needs_path ? 1 : 0;
    d.skybox = skybox ? 1 : 0;
    d.tex = base + o_tex;
    d.srgb_values = reinterpret_cast<const double*>(base + o_srgbv);
    for (int k = 0; k < 6; ++k)
        d.faces[k] = DevTexFace{skybox ? s->skybox[k].width : 0u, skybox ? s->skybox[k].height : 0u, face_off[k]};
    d.cam_dof = s->camera.kind == RT_CAMERA_DOF ? 1 : 0;
    d.cam_samples = d.cam_dof ? s->camera.samples : 1u;
    d.cam_focus = s->camera.focus;
    d.cam_aperture = s->camera.aperture;
    {   // camera.rs:98: im_dist = (matrix * Vec3(0, 0, 1)).norm()
        const double* M = s->camera.matrix;
        const double zx = (M[0] * 0.0 + M[1] * 0.0) + M[2] * 1.0;
        const double zy = (M[3] * 0.0 + M[4] * 0.0) + M[5] * 1.0;
        const double zz = (M[6] * 0.0 + M[7] * 0.0) + M[8] * 1.0;
        d.cam_im_dist = std::sqrt(zx * zx + zy * zy + zz * zz);
    }
    for (int k = 0; k < 3; ++k) d.cam_pos[k] = s->camera.position[k];
    for (int k = 0; k < 9; ++k) d.cam_m[k] = s->camera.matrix[k];
    d.bg[0] = s->background.r; d.bg[1] = s->background.g; d.bg[2] = s->background.b;
    d.lgrid = lg.grids.empty() ? nullptr : reinterpret_cast<const DevLightGrid*>(base + o_lg);
    d.lg_off = reinterpret_cast<const uint32_t*>(base + o_lgoff);
    d.lg_ent = reinterpret_cast<const DevLgEntry*>(base + o_lgent);
    d.cgrid = (cg.grids.empty() || cg.grids[0].R <= 0) ? nullptr : reinterpret_cast<const DevLightGrid*>(base + o_cg);
    d.cg_off = reinterpret_cast<const uint32_t*>(base + o_cgoff);
    d.cg_ent = reinterpret_cast<const DevLgEntry*>(base + o_cgent);
    c->all_lights_gridded = !lights.empty() && lg.grids.size() == lights.size();
    for (const DevLightGrid& g : lg.grids) c->all_lights_gridded = c->all_lights_gridded && g.R > 0;
    c->scene_spp = s->antialias;
    c->has_scene = true;
    ++c->scene_gen;                   // accumulators bound to the previous scene refuse until reset
    return RT_OK;
}

int rt_scene_upload(rt_ctx* c, const rt_scene* s) {
    if (!c || !s) return RT_E_INVALID;
    return guarded(c, [&] { return scene_upload(c, s); });
}

}  // extern "C"
