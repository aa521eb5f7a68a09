/*
 * raytrace_amd.h -- C ABI of the MI355X-native per-pixel ray-tracing path.
 *
 * This is the drop-in boundary for j-dong/rust-raytrace's hot path.  The
 * reference has no FFI of its own: its "operator API" is Rust trait objects
 * (Shape / Material / LightModel / Background / Camera) called once per pixel
 * sample from the serial loop in main.rs:45-57.  A per-sample FFI call is far
 * too fine-grained for a GPU and `dyn` objects cannot cross a C ABI, so the
 * boundary sits one level up: the host parses and flattens the Scene, and the
 * library renders whole frames / tiles / row bands on one device.
 *
 * Entry point -> reference interface it replaces:
 *   rt_scene_parse        serialize.rs:427-441   pub fn deserialize(&String) -> Result<Scene, SyntaxError>
 *   rt_scene_from_desc    scene.rs:201-212       building a `Scene { objects, lights, camera, background, options }` in code
 *   rt_camera_simple_new  camera.rs:51-63        SimplePerspectiveCamera::new
 *   rt_camera_look_at     camera.rs:67-73        SimplePerspectiveCamera::look_at
 *   rt_render / rt_render_device
 *                         main.rs:39-57 + raytrace.rs:270-276 (raytrace) + raytrace.rs:261-267
 *                         (ray_color) + raytrace.rs:30-67 (PhongMaterial::color) + scene.rs:247-249
 *                         (Scene::intersect) + shapes.rs:50-112 (Sphere/Plane::intersect)
 *   rt_render_accumulate / rt_accum_resolve
 *                         main.rs:47-56 split over calls: `res = res + raytrace(..)` for a range of the
 *                         AA samples, and `res / antialias` + write_bgr whenever a frame is wanted
 *   rt_render_aov / rt_render_aov_device
 *                         main.rs:39-56 with `raytrace(..)` replaced by what Scene::intersect (scene.rs:247-249)
 *                         answers for the camera ray: Hit.t, the shape's normal (shapes.rs:72, 79, 108) and the
 *                         hit object; no shading
 *   rt_query_nearest / rt_query_occluded (and their _device variants)
 *                         scene.rs:247-249 Scene::intersect and raytrace.rs:43-50 (the shadow test) for rays the
 *                         caller supplies
 *   rt_scene_set_skybox   scene.rs:174-188       SkyboxBackground { px, nx, py, ny, pz, nz }
 *   rt_texture_load       texture.rs:34-37       Texture::load (BMP and binary PPM here; the image crate decodes more)
 *   rt_to_srgb            color.rs:593-600       fn to_srgb (used by Color::write_bgr, color.rs:628-632)
 *   rt_bmp_header         bmp.rs:10-61           pub fn write_header
 *   rt_write_bmp          main.rs:34-59          header + bottom-up BGR rows to a file
 *
 * Conventions:
 *   - Every function returns RT_OK (0) or a negative RT_E_* code.  No C++
 *     exception or abort crosses the ABI.  rt_last_error() describes the last
 *     failure of a context (thread-local text for context-free calls).
 *   - All pointers are caller-owned; the library copies what it keeps.
 *   - One rt_ctx per device; calls on one context are not thread-safe;
 *     different contexts may be driven concurrently (one host thread per GPU).
 *   - A context's renders are ordered: each waits (on the device, not the
 *     host) for the context's previous render, whatever streams they were
 *     issued on, because they share the context's working set.  A stream
 *     passed to rt_render_device must outlive the renders issued on it (a
 *     render on the same stream as the previous one relies on stream order).
 *     rt_scene_upload waits for every render still reading the old scene.
 *   - Nothing is read from the environment: a render's schedule depends only
 *     on the scene, the options and the context's tuning (rt_ctx_set_tuning).
 *   - All scene arithmetic is IEEE f64 exactly as the reference (no FMA
 *     contraction); output colours are the f64 result rounded once to f32,
 *     and the u8 BGR bytes are quantised from the f64 value on the device.
 *   - Pixel row 0 is the image BOTTOM (the first row written, main.rs:45/58).
 */
#ifndef RAYTRACE_AMD_H
#define RAYTRACE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 10: rt_isect_check and rt_shade_check added (record-level diagnostics of the sphere and plane tests and
 * of the shading arithmetic, DESIGN.md 4 "Primitive probes").  No struct, enum value or tuning key changed.
 * Still 10: the ray queries (enum rt_hit_channel, rt_hit_buffers, rt_query_nearest / rt_query_occluded and their
 * device variants) add functions, one enum and one struct, and alter nothing a caller built against ABI 10 passes
 * or reads; RT_KF_COUNT is still 8.  A caller that needs them looks the symbols up.
 * Still 10: the denoiser (enum rt_denoise_flags, rt_denoise_params, rt_denoise_inputs, rt_denoise and
 * rt_denoise_device) adds functions, one enum and two structs in the same way; no tuning key.
 * Still 10: second moments (rt_accum_create_moments, rt_accum_has_moments, rt_accum_download_moments /
 * upload_moments, rt_accum_noise / noise_host, rt_checkpoint_write_moments / read_moments) add functions only:
 * no struct, enum or tuning key; accum_noise is timed under RT_KF_COMPOSE.
 * Still 10: the variance-guided denoiser (rt_denoise_variance, rt_denoise_var and rt_denoise_var_device) adds two
 * functions and one struct; rt_denoise_params, rt_denoise_inputs and rt_denoise_flags are as they were, no tuning key.
 * 9: first-hit feature buffers: enum rt_aov, rt_aov_buffers, rt_render_aov and rt_render_aov_device
 * (depth, normal, albedo, coverage and object id of the camera rays' first hits).  Functions and types
 * added only: no struct, enum value or tuning key changed, RT_KF_COUNT is still 8.
 * 8: rt_cull_check and rt_cull_reach added (diagnostics of the conservative f32 culling and of the
 * far-origin rule).  No struct, enum value or tuning key changed.
 * 7: progressive rendering: rt_accum (a device-resident f64 accumulator of one tile) with
 * rt_accum_create / destroy / samples / reset, rt_render_accumulate, rt_accum_resolve / resolve_host,
 * rt_accum_download / upload, and the host-only rt_checkpoint_write / read.  No struct, enum value or
 * tuning key changed.
 * 6: rt_algo gained RT_ALGO_WAVEFRONT_AA (one wavefront pass per jittered AA sample); tuning key
 * aa_wavefront added.  No struct changed.
 * 5: rt_out_flags gained RT_OUT_FRAME_ROWS (rt_render writes a banded tile
 * straight into its rows of a whole-frame host buffer); rt_ctx_reserve added;
 * rt_sqrt_check added; rt_kernel_family index 6 is RT_KF_COMPOSE (earlier ABI-4 builds named it
 * RT_KF_SHADOW); the tuning keys fuse, lists,
 * lists0, fuse_from, prefix4_kb, cam_prefix_kb, tail_from, tail_max,
 * eager_fold, fold_split, bmerge, wave_max, tail_fold, tail_shade, fold_wgs and
 * shade_wgs (variants measured slower and removed) are gone:
 * rt_ctx_set_tuning answers RT_E_INVALID for them; tuning keys chain_on_caller,
 * copy_engine and dev_join added.  rt_stats unchanged (80 B); its kernel_ms is 0
 * after an rt_render_device without RT_TIME_KERNELS / RT_COUNT_WORK.
 * 4: rt_abi_version() added; RT_KF_TAIL (RT_KF_COUNT 8).  A caller checks
 * rt_abi_version() == RT_ABI_VERSION of the header it was built against before
 * passing any struct; any change of a struct, enum value or tuning key bumps it. */
#define RT_ABI_VERSION 10

enum rt_status {
    RT_OK = 0,
    RT_E_INVALID = -1,      /* bad argument */
    RT_E_NODEVICE = -2,     /* no HIP device / bad device index */
    RT_E_HIP = -3,          /* HIP runtime error (see rt_last_error) */
    RT_E_NOMEM = -4,
    RT_E_UNSUPPORTED = -5,  /* scene uses a class the device path does not implement yet */
    RT_E_PARSE = -6,        /* scene text failed to parse (SyntaxError) */
    RT_E_NOSCENE = -7,      /* render before upload */
    RT_E_IO = -8
};

/* ---- scene model (flattened mirror of scene.rs / shapes.rs / camera.rs) ---- */
enum rt_shape_kind { RT_SHAPE_SPHERE = 0, RT_SHAPE_PLANE = 1 };                 /* shapes.rs:42-112 */
enum rt_material_kind {                                                          /* scene.rs:32-89 */
    RT_MAT_PHONG = 0, RT_MAT_INDIRECT_PHONG = 1, RT_MAT_FRESNEL = 2, RT_MAT_TRANSPARENT = 3
};
enum rt_light_kind { RT_LIGHT_POINT = 0, RT_LIGHT_DIRECTIONAL = 1, RT_LIGHT_AREA = 2 };  /* scene.rs:117-155 */
enum rt_camera_kind { RT_CAMERA_SIMPLE = 0, RT_CAMERA_DOF = 1 };                 /* camera.rs:29-123 */
enum rt_background_kind { RT_BG_SOLID = 0, RT_BG_SKYBOX = 1 };                  /* scene.rs:164-188 */

typedef struct { double r, g, b; } rt_color;                                     /* color.rs:15-22 */

typedef struct {
    int32_t shape;          /* rt_shape_kind */
    int32_t material;       /* rt_material_kind */
    double geom[6];         /* sphere: center x,y,z, radius   plane: point x,y,z, normal x,y,z */
    rt_color diffuse;       /* Phong / IndirectPhong / Fresnel */
    rt_color specular;
    rt_color ambient;       /* Phong / IndirectPhong / Fresnel */
    double exponent;
    double ior;             /* Fresnel / Transparent */
    uint32_t samples;       /* IndirectPhong */
    uint32_t _pad;
} rt_object;

typedef struct {
    int32_t kind;           /* rt_light_kind */
    int32_t _pad;
    double v[9];            /* point: location; directional: direction; area: origin, side1, side2 */
    rt_color color;
} rt_light;

typedef struct {
    int32_t kind;           /* rt_camera_kind */
    uint32_t samples;       /* DepthOfFieldCamera samples (1 for simple) */
    double position[3];     /* SimplePerspectiveCamera.position */
    double matrix[9];       /* SimplePerspectiveCamera.matrix, row-major M[i][j] */
    double focus, aperture; /* DepthOfFieldCamera */
} rt_camera;

typedef struct {
    const rt_object* objects; uint32_t n_objects;
    const rt_light* lights;   uint32_t n_lights;
    rt_camera camera;
    int32_t background_kind;  /* a desc carries RT_BG_SOLID; textures go through rt_scene_set_skybox */
    rt_color background;
    uint32_t width, height, antialias;   /* scene.rs:191-198 Options */
} rt_scene_desc;

/* texture.rs:22-26: an RGB8 image, rows top-down, width*height*3 bytes (caller-owned). */
typedef struct {
    uint32_t width, height;
    const uint8_t* rgb;
} rt_texture;

typedef struct rt_scene rt_scene;   /* host-side parsed scene (opaque) */
typedef struct rt_ctx rt_ctx;       /* one device context (opaque) */

/* ---- host-side scene API ---- */
int rt_scene_parse(const char* text, size_t len, rt_scene** out, char* err, size_t err_len);
int rt_scene_from_desc(const rt_scene_desc* desc, rt_scene** out);
/* Borrow the flattened view of a scene (valid until rt_scene_free). */
int rt_scene_get_desc(const rt_scene* scene, rt_scene_desc* out);
void rt_scene_free(rt_scene* scene);
/* Make the scene's background a SkyboxBackground with faces px, nx, py, ny, pz, nz (copied). */
int rt_scene_set_skybox(rt_scene* scene, const rt_texture faces[6]);
/* Diagnostic, host only (no device): the spheres the light-view grid of point
 * light `light` (built as rt_scene_upload builds it) hands a
 * shadow query from each point of `points` (n_points x 3 doubles): the same
 * candidate list, in the same order, as the device tests after the planes and
 * the hint.  counts[i] = its length, or -1 when the device tests every sphere
 * (degenerate direction, or no grid for this light); ids = the candidates'
 * object ids (file order, scene.rs:248), concatenated, at most cap in all.
 * info[0..2] = cells per face side, stored cells, list entries.  resolution:
 * cells per face side (0 = the upload's automatic choice, else 1..4096).
 * Replaces nothing in the reference (its shadow query scans every object,
 * scene.rs:247-249); tests check the lists against that scan. */
int rt_light_grid_candidates(const rt_scene* scene, int light, int resolution, const double* points, uint32_t n_points,
                             int32_t* counts, int32_t* ids, size_t cap, int64_t* info);
/* Diagnostic, host only: the camera's view grid (built as
 * rt_scene_upload builds it, spheres in file order) for camera-ray directions
 * `dirs` (n_dirs x 3 doubles): for each direction the spheres the device may
 * test -- the always list, then the direction's whole cell list in increasing
 * distance bound (the device stops once a bound exceeds its best t) --
 * counts[i] = its length, or -1 when the device tests every sphere; ids = object
 * ids, nears = each entry's distance bound (f32), both concatenated, at most cap
 * in all.  info[0..2] = cells per face side, stored cells, list entries.
 * resolution: cells per face side (0: from the scene's frame size).  Replaces
 * nothing in the reference (scene.rs:247-249 scans every object); tests check
 * the lists against that scan. */
int rt_view_grid_candidates(const rt_scene* scene, int resolution, const double* dirs, uint32_t n_dirs,
                            int32_t* counts, int32_t* ids, float* nears, size_t cap, int64_t* info);
/* Diagnostic, host only: the quantised 4-wide sphere tree (DESIGN.md §3.10,
 * built as rt_scene_upload builds it; leaf_max 0: the upload's leaf size) and
 * the f32 child boxes it rounds outward.  nodes: 48 B per node (the device
 * layout, DevQNode4), at most cap_nodes; boxes: per node and child slot
 * lo x,y,z, hi x,y,z (f32; NaN for an unused slot), at most cap_nodes * 24
 * floats; sphere_first / sphere_count: per node and slot the leaf's spheres in
 * leaf order (-1 / 0 for an inner child or unused slot).  info[0..2] = nodes (0:
 * not representable, the device keeps the other trees), the traversal stack's
 * worst case, the leaf size; cap_nodes 0 is a size query (info only).  Replaces nothing in the reference (scene.rs:247-249
 * scans every object); tests decode the nodes and check every box contains its
 * f32 box. */
int rt_qtree_nodes(const rt_scene* scene, int leaf_max, void* nodes, float* boxes, int32_t* sphere_first,
                   int32_t* sphere_count, size_t cap_nodes, int64_t* info);
/* Decode an image file as Texture::load does (RGB8, rows top-down).  rgb == NULL: only the size.
 * Formats: uncompressed BMP (24/32 bit) and binary PPM; others -> RT_E_UNSUPPORTED. */
int rt_texture_load(const char* path, uint32_t* width, uint32_t* height, uint8_t* rgb, size_t cap);

int rt_camera_simple_new(const double position[3], const double look[3], const double up[3],
                         double im_dist, rt_camera* out);
int rt_camera_look_at(const double focus[3], const double look[3], const double up[3],
                      double pov, double h, rt_camera* out);

uint8_t rt_to_srgb(double v);
/* Writes the 122-byte BITMAPV4 header; *bytewidth = padded row pitch. */
int rt_bmp_header(uint8_t out[122], uint32_t width, uint32_t height, uint32_t* bytewidth);
/* Writes header + pixel array (bgr rows, bottom-up, `pitch` bytes each) to `path`. */
int rt_write_bmp(const char* path, uint32_t width, uint32_t height, const uint8_t* bgr, uint32_t pitch);

/* ---- device API ---- */
/* The RT_ABI_VERSION this library was built with. */
int rt_abi_version(void);
int rt_device_count(int* n);
int rt_ctx_create(int device, rt_ctx** out);
void rt_ctx_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);
/* Copies the scene to HBM in the device layout.  Classes the device path does
 * not implement -> RT_E_UNSUPPORTED.  A SkyboxBackground's texels go with every
 * scene that has one and do not choose the schedule: a skybox scene of chain classes (Phong /
 * Fresnel, point / directional lights, the simple camera) renders on every rt_algo. */
int rt_scene_upload(rt_ctx* ctx, const rt_scene* scene);

enum rt_jitter {
    RT_JITTER_CENTER = 0,   /* jx = jy = 0.5 (deterministic parity mode, main.rs:51-52) */
    RT_JITTER_RANDOM = 1    /* jx, jy drawn per AA sample (main.rs:51-52) from the keyed RNG (rt_render_opts.seed) */
};
enum rt_out_flags {
    RT_OUT_RGB_F32 = 1,
    RT_OUT_BGR_U8 = 2,
    RT_COUNT_WORK = 4,         /* also count box / sphere tests (instrumented kernels; wavefront only) */
    RT_TIME_KERNELS = 8,       /* record a timing event after every launch (wavefront, one stream) */
    RT_OUT_FRAME_ROWS = 16     /* rt_render only: out_rgb / out_bgr hold the WHOLE frame (height rows; f32
                                  rows of 3*width floats, BGR rows of bgr_pitch bytes, 0 -> 3*width) and the
                                  tile's pixel (x, local row j) lands in column x0 + x of its frame row
                                  y0 + ((j/band)*band_stride + band_phase)*band + j%band; nothing else of
                                  the buffers is written.  The multi-GPU host gather (main.rs:45-58 split
                                  over devices): each context renders its row bands straight into one
                                  shared page-locked frame, the copies overlapping its render. */
};
enum rt_algo {
    RT_ALGO_AUTO = 0,
    RT_ALGO_BRUTE_LDS = 1,      /* megakernel, sphere list staged in LDS */
    RT_ALGO_BRUTE_GLOBAL = 2,   /* megakernel, sphere list read through the caches */
    RT_ALGO_WAVEFRONT = 3,      /* per-depth launches over compacted ray queues, sphere BVH (default) */
    RT_ALGO_WAVEFRONT_BRUTE = 4, /* the same schedule, every sphere tested (linear scan like scene.rs:248) */
                                /* (1-4 and 6, the chain algorithms: solid or skybox background; a ray that misses
                                   takes the skybox's colour in its direction, raytrace.rs:234-256) */
    RT_ALGO_PATH = 5,           /* per-pixel recursion over an HBM stack: every material / light / camera class
                                   (IndirectPhong, Transparent, AreaLight, DepthOfField, random jitter); AUTO picks
                                   it whenever the scene or the jitter mode needs it (a skybox alone does not) */
    RT_ALGO_WAVEFRONT_AA = 6    /* RT_ALGO_WAVEFRONT's schedule run once per AA sample (main.rs:47-56): every sample
                                   of a pixel gets its own jitter (rt_jitter, any spp >= 1) and its own ray tree;
                                   the samples are summed in f64 in sample order and divided by spp, bit for bit
                                   what RT_ALGO_PATH renders.  With RT_JITTER_CENTER or spp 1 it is
                                   RT_ALGO_WAVEFRONT's render.  A scene that needs RT_ALGO_PATH (IndirectPhong,
                                   Transparent, AreaLight, DepthOfField) or has more than 32 lights ->
                                   RT_E_UNSUPPORTED.  AUTO picks it only under tuning aa_wavefront.  Skybox: a
                                   sample whose camera ray misses adds the skybox's colour along that sample's ray. */
};

typedef struct {
    uint32_t width, height;   /* full frame: defines the pixel -> (-1,1) mapping (main.rs:39-41) */
    uint32_t x0, tile_w;      /* columns [x0, x0 + tile_w) */
    uint32_t y0, tile_h;      /* local row j -> global row y0 + ((j/band)*band_stride + band_phase)*band + j%band */
    uint32_t band, band_stride, band_phase;   /* 0 -> 1: contiguous rows */
    uint32_t max_depth;       /* reference MAX_DEPTH = 4 (raytrace.rs:18); <= RT_MAX_DEPTH_LIMIT */
    uint32_t spp;             /* AA samples (Options.antialias); 0 -> the uploaded scene's value */
    int32_t jitter;           /* rt_jitter */
    uint32_t flags;           /* rt_out_flags */
    int32_t algo;             /* rt_algo */
    uint32_t bgr_pitch;       /* bytes per output BGR row; 0 -> 3*tile_w.  The bytes of a row past its
                                 3*tile_w pixel bytes: rt_render writes them as zero (BMP row padding,
                                 main.rs:42); rt_render_device leaves them as the caller's buffer has them */
    uint32_t _pad;
    uint64_t seed;            /* keyed RNG seed: every random draw is a function of (seed, pixel, AA sample,
                                 camera sample, path through the ray tree, draw id), so a frame is
                                 reproducible and independent of tiling and GPU count.  The reference
                                 seeds one sequential XorShift stream from OS entropy (main.rs:43). */
} rt_render_opts;

#define RT_MAX_DEPTH_LIMIT 30

typedef struct {
    uint64_t rays;            /* every Scene::intersect query issued (camera + reflection + shadow) */
    uint64_t shadow_rays;
    uint64_t pixels;
    double kernel_ms;         /* hipEvent time from the first to the last launch of the render
                                 (rt_render, and rt_render_device with RT_TIME_KERNELS or
                                 RT_COUNT_WORK; 0 for other rt_render_device renders, which
                                 record no start event: one marker fewer between frames) */
    uint64_t box_tests;       /* RT_COUNT_WORK only: BVH slab tests (2 per inner node visited) */
    uint64_t sphere_tests;    /* RT_COUNT_WORK only: exact ray-sphere quadratics evaluated */
    uint64_t shadow_box_tests, shadow_sphere_tests;   /* the shadow-query share of the two above */
    uint64_t traced_rays;     /* queries the device actually traced: `rays` / spp when a chain schedule
                                 renders spp identical centre-jitter samples once, else `rays` */
    uint64_t chunks;          /* row chunks the wavefront schedule ran the tile as (sized to the
                                 working-set budget, tuning wf_budget_mb; RT_ALGO_WAVEFRONT_AA runs spp
                                 passes per chunk and counts the chunk once); 0 for other schedules */
} rt_stats;

void rt_render_opts_default(rt_render_opts* o, uint32_t width, uint32_t height);

/* Synchronous: renders into caller-owned HOST buffers (either may be NULL).
 * Page-locked buffers (hipHostMalloc / hipHostRegister) receive the DMA
 * directly; pageable ones are filled through four pinned 8 MiB staging slices,
 * the copy engine filling slices ahead while a pool of host threads empties
 * them in order.  Pass only the outputs needed: BGR alone moves 3 B per pixel
 * instead of 15 (C3, 4096^2: DESIGN.md §6 gives the measured end-to-end time). */
int rt_render(rt_ctx* ctx, const rt_render_opts* opts, float* out_rgb, uint8_t* out_bgr, rt_stats* stats);
/* Asynchronous on `stream` (a hipStream_t; NULL = the context's own stream):
 * renders into caller-owned DEVICE buffers.  Statistics of the most recent
 * render are read with rt_ctx_stats (which synchronises). */
int rt_render_device(rt_ctx* ctx, const rt_render_opts* opts, void* d_rgb, void* d_bgr, void* stream);
/* Prepare the context for renders with these options, synchronously and
 * without rendering: the schedule's streams and hardware queues, its working
 * set (sized exactly as the render sizes it), rt_render's device frame and
 * sparse-copy buffers (host = 1) and the kernels' code objects.  A later
 * rt_render / rt_render_device with the same options (or smaller ones) then
 * allocates nothing: a process that renders one frame (main.rs:13-60) calls
 * it after rt_scene_upload, e.g. while it parses or opens its output.  Needs
 * an uploaded scene (the schedule depends on it); RT_E_NOMEM if the working
 * set does not fit even as the smallest chunks.  stream: the hipStream_t the
 * rt_render_device calls will be issued on (its hardware queue is set up too;
 * NULL = the context's own stream, which rt_render uses). */
int rt_ctx_reserve(rt_ctx* ctx, const rt_render_opts* opts, int host, void* stream);
/* Statistics of the most recent render (a refused call is no render); synchronises
 * with it.  They, and rt_ctx_generation_counts, stay readable, with the same
 * values and as often as wanted, after rt_ctx_reserve (whatever it allocates
 * or frees), rt_ctx_set_tuning (also of the keys that rebuild the streams) and
 * rt_scene_upload of another scene: the next render replaces them, nothing else. */
int rt_ctx_stats(rt_ctx* ctx, rt_stats* stats);
/* ---- first-hit feature buffers (AOVs) ----
 * What Scene::intersect (scene.rs:223-249) answers for the camera rays, averaged over the AA samples as colours
 * are (main.rs:47-56), without any shading.  For tile pixel (x, local row j) and AA sample a in [0, spp):
 *   ray_a = the camera ray rt_render traces for (x, j, a): the pixel mapping of main.rs:39-41, 50-53 from the
 *           geometry fields of rt_render_opts, jitter and seed (RT_JITTER_CENTER: jx = jy = 0.5; RT_JITTER_RANDOM:
 *           the keyed draws of sample a), then camera.rs:78.  Under RT_JITTER_RANDOM the buffers line up sample for
 *           sample with the colours RT_ALGO_PATH and RT_ALGO_WAVEFRONT_AA render.
 *   h_a   = Scene::intersect(ray_a): the smallest t, the first object in file order on a tie, and a NaN t (only a
 *           plane's 0/0 gives one) beats everything (scene.rs:223-249).
 * Per-sample values v_a:            hit                                                          miss
 *   depth                           h.t                                                          0.0
 *   normal x, y, z                  the shape's normal: sphere normalize(ray.cast(t) - centre)   0.0, 0.0, 0.0
 *                                   (shapes.rs:72, 79), plane as in the file, not normalised
 *                                   (shapes.rs:108); negated when dot(normal, ray.direction)
 *                                   > 0.0 (the rule of raytrace.rs:38, here for every material)
 *   albedo r, g, b                  the hit object's `diffuse` as rt_scene_get_desc reports      0.0, 0.0, 0.0
 *                                   it, whatever its material
 *   coverage                        1.0                                                          0.0
 * Every float channel is averaged as main.rs:47-56 averages colours: sum = 0.0; sum = sum + v_a for a = 0 .. spp-1
 * in sample order; out = (float)(sum / (double)spp): one rounding to f32, NaN propagates (a plane's NaN t gives a
 * NaN depth and leaves the other channels finite).  With RT_JITTER_CENTER the samples are identical: the ray is
 * traced once and the sum still formed with spp additions.  The mean of a channel over the samples that hit is
 * channel / coverage.
 * object (int32): the object id (file order, what Hit::obj holds) of sample 0's hit, -1 when sample 0 misses.
 *
 * Buffers are tile row-major, tile_h rows of tile_w elements (normal and albedo: 3 floats per pixel); local row
 * j is frame row y0 + ((j/band)*band_stride + band_phase)*band + j%band as for rt_render.  Read of opts: width,
 * height, x0, tile_w, y0, tile_h, band, band_stride, band_phase, spp (0: the scene's), jitter, seed, and of flags
 * RT_TIME_KERNELS alone (the launch's time is counted under RT_KF_CAMERA); max_depth, algo, the other flags and
 * bgr_pitch are ignored (no RT_OUT_FRAME_ROWS).  channels: a non-empty mask of rt_aov; only the selected buffers
 * are read from the struct and written.
 * RT_E_INVALID: channels 0 or with unknown bits, a selected channel whose pointer is NULL, tile geometry that
 * rt_render would refuse; RT_E_NOSCENE: no scene uploaded; RT_E_UNSUPPORTED: a DepthOfFieldCamera (its rays go
 * through cos and sin: not a bit-exact feature).  Every other scene class is served.
 * An AOV render is a render of the context: ordered on the device after the previous one; afterwards rt_ctx_stats
 * reports rays = pixels * spp, shadow_rays 0, pixels, chunks 0 and traced_rays = pixels under RT_JITTER_CENTER,
 * else rays.  A refused call is no render: the statistics stay the previous render's. */
enum rt_aov { RT_AOV_DEPTH = 1, RT_AOV_NORMAL = 2, RT_AOV_ALBEDO = 4, RT_AOV_COVERAGE = 8, RT_AOV_OBJECT = 16 };
typedef struct { float* depth; float* normal; float* albedo; float* coverage; int32_t* object; } rt_aov_buffers;
/* Synchronous, into caller-owned HOST buffers. */
int rt_render_aov(rt_ctx* ctx, const rt_render_opts* opts, uint32_t channels, const rt_aov_buffers* host, rt_stats* stats);
/* Asynchronous on `stream` (NULL: the context's own), into caller-owned DEVICE buffers. */
int rt_render_aov_device(rt_ctx* ctx, const rt_render_opts* opts, uint32_t channels, const rt_aov_buffers* dev, void* stream);
/* ---- ray queries: nearest hit and occlusion for caller-supplied rays ----
 * Scene::intersect (scene.rs:247-249) and the shadow test of raytrace.rs:43-50 for rays the caller builds: a baking
 * pass, a line-of-sight test, a picking ray, rays made in tensors.  No shading, no recursion, no averaging.
 *   rays[6 i ..] = origin x, y, z then direction x, y, z of ray i (f64): the [n, 6] layout of rt_cull_check and
 *   rt_isect_check.  The direction is used as given, not normalised (Ray in shapes.rs does not normalise it either):
 *   t is in units of the direction's length, and scaling a direction by 2^k scales every t by 2^-k exactly.
 * Nearest hit: h = Scene::intersect(ray): the smallest t, the first object in file order on a tie, and a NaN t (only
 * a plane's 0/0 gives one) beats everything (scene.rs:223-249).
 *   output            hit                                                                   miss
 *   t[i]              h.t                                                                   +inf
 *   object[i]         the object id (file order, what Hit::obj holds)                       -1
 *   normal[3 i ..]    the shape's normal as the intersection returns it: sphere             0.0, 0.0, 0.0
 *                     normalize(ray.cast(t) - centre) (shapes.rs:72, 79), plane as in the
 *                     file, not normalised (shapes.rs:108)
 *   All f64, no rounding.  The normal is NOT oriented against the ray; a caller who wants the orientation of
 *   rt_render_aov's normal applies raytrace.rs:38: negate it when dot(normal, ray.direction) > 0.0.
 *   channels: a non-empty mask of rt_hit_channel; only the selected buffers are read from the struct and written.
 * Occlusion: raytrace.rs:43-50 verbatim.  occluded[i] = 1 when Scene::intersect(ray) is Some(h) and (r2 is NULL or
 *   h.t * h.t < r2[i]), else 0.  r2 NULL is the directional light's rule (scene.rs:131-139: no range), r2 the point
 *   light's with the caller's squared range (scene.rs:125).  A plane's NaN t under a range is therefore not occluded
 *   (NaN < r2 is false) and without a range it is.  The shadow ray raytrace.rs:43 itself issues from a hit point pt
 *   towards a light direction ldir is origin = pt + ldir * 1e-5, direction = ldir.
 * Domain of a ray: six finite components; |origin| <= 1e30 on every axis; the direction's largest component magnitude
 *   in [2^-256, 2^256]; r2[i] not NaN and >= 0 (+inf allowed); and of the scene, for the queries: the spheres' extent
 *   (the largest |centre +- radius|, rt_cull_reach's argument) <= 1e30 and every radius >= 1e-60.  Inside it the
 *   answers are the reference's, bit for bit.  The exact tests are the reference's f64 operations in its order whatever
 *   the magnitudes, but the tree sources cull with f32 boxes, and a box holds every hit the exact quadratic can report
 *   only while the quadratic's intermediates keep their relative precision: a = d.d, b*b, 4a*c and the discriminant
 *   neither overflow nor lose bits to underflow ("BVH exactness" item 1).  A wider bound such as 2^+-500
 *   breaks that: with direction (2^500, 0, 0) from the coordinate origin, b*b overflows to +inf for a sphere of radius
 *   2500 centred 3000 BEHIND the origin, the reference reports a hit at t = +inf (shapes.rs:65-79), the brute sources
 *   do as well, and every tree source culls the box and reports a miss.  With 2^+-256, |origin| and extent <= 2^100:
 *   a <= 2^514, |b| <= 2^360, b*b and 4a*c <= 2^722; a >= 2^-512, and b*b or 4a*c can fall below 2^-1022 only for
 *   features below 2^-200 (hence the radius bound).  Within that the culling runs on the direction scaled by a power of
 *   two whenever its largest component leaves [2^-20, 2^20] (every t limit scaled alike), and an origin beyond the
 *   scene's culling domain (rt_cull_reach) is not culled at all: it tests every sphere; 1e30 keeps the origin's f32
 *   image finite.  Outside the domain the values are unspecified (and may differ between tuning src values), but
 *   nothing is read or written out of bounds.
 * flags: RT_TIME_KERNELS alone (the launch is counted under RT_KF_NEAREST, an occlusion query's under
 *   RT_KF_OCCLUSION); any other bit -> RT_E_INVALID.
 * A query is a render of the context, as an AOV render is: ordered on the device after the previous render;
 *   afterwards rt_ctx_stats reports rays = traced_rays = n, shadow_rays 0 (nearest) or n (occlusion), pixels 0,
 *   chunks 0 and the work counters 0.  n = 0 is a valid render that launches nothing and touches no buffer (no
 *   pointer is looked at).  A query neither needs nor frees the wavefront working set, an rt_accum or what
 *   rt_ctx_reserve prepared.
 * Refusals, each no render (the statistics stay the previous render's): RT_E_INVALID for unknown flag bits, channels
 *   0 or with unknown bits, and with n > 0 a NULL rays / occluded / struct, a selected channel whose pointer is NULL,
 *   and in the device variants a d_rays that is not 16-byte aligned (the kernel reads a ray as three 16-byte loads;
 *   the host variants stage the rays, so any pointer is accepted there); RT_E_NOSCENE: no scene uploaded; RT_E_NOMEM:
 *   the host variant's device buffers do not fit.  There is no RT_E_UNSUPPORTED case: only geometry is read, so every
 *   scene class, camera and background is served. */
enum rt_hit_channel { RT_HIT_T = 1, RT_HIT_OBJECT = 2, RT_HIT_NORMAL = 4 };
typedef struct { double* t; int32_t* object; double* normal; } rt_hit_buffers;
/* Synchronous, caller-owned HOST buffers (staged through device buffers the call allocates and frees). */
int rt_query_nearest(rt_ctx* ctx, const double* rays, uint32_t n, uint32_t channels, const rt_hit_buffers* host,
                     uint32_t flags, rt_stats* stats);
int rt_query_occluded(rt_ctx* ctx, const double* rays, const double* r2, uint32_t n, uint8_t* occluded, uint32_t flags,
                      rt_stats* stats);
/* Asynchronous on `stream` (NULL: the context's own), caller-owned DEVICE buffers. */
int rt_query_nearest_device(rt_ctx* ctx, const double* d_rays, uint32_t n, uint32_t channels, const rt_hit_buffers* dev,
                            uint32_t flags, void* stream);
int rt_query_occluded_device(rt_ctx* ctx, const double* d_rays, const double* d_r2, uint32_t n, uint8_t* d_occluded,
                             uint32_t flags, void* stream);
/* ---- denoiser: an edge-avoiding a-trous wavelet filter guided by the first-hit feature buffers ----
 * What a caller does with a 4- or 16-sample frame of a noisy scene (IndirectPhong, AreaLight, random jitter) and
 * the buffers rt_render_aov gives for it: `iterations` passes of the 5x5 B3-spline kernel with holes (Dammertz et
 * al. 2010), pass i with step s = 2^i, every tap's weight cut down where normal, depth or colour differ.  Not a
 * render: no scene is needed, and rt_ctx_stats / rt_ctx_generation_counts are left as they were.
 *
 * The rule.  All arithmetic is IEEE f64 + - * / and comparisons, never fused, in exactly this order; every f32
 * read is widened to f64 first.
 * Inputs, each tight row-major as rt_render_device / rt_render_aov_device write a whole-frame tile: rgb [h, w, 3]
 *   f32; the guides, each read only when its flag is set: normal [h, w, 3], depth [h, w], albedo [h, w, 3] f32.
 * Demodulation (RT_DN_DEMODULATE), per channel before the first pass: c = a > 0.0 ? (double)(float)(c / a) : c.
 * Pass i at pixel p: sum = (0, 0, 0), wsum = 0; for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner) the tap is
 *   q = p + s * (dx, dy); a tap outside the image is skipped.
 *     kw = K[|dy|] * K[|dx|], K = {3/8, 1/4, 1/16}
 *     the centre tap (q == p): wt = kw; it is never skipped.
 *     any other tap: wt = kw, then for the flags that are set, in this order,
 *       RT_DN_NORMAL  d = (nx_p*nx_q + ny_p*ny_q) + nz_p*nz_q;  d = d > 0.0 ? d : 0.0;  normal_squarings times
 *                     d = d*d;  wt = wt*d
 *       RT_DN_DEPTH   dz = z_p - z_q;  t = sigma_depth * (double)s;  wt = wt / (1.0 + (dz*dz)/(t*t))
 *       RT_DN_COLOR   dr, dg, db = c_p - c_q per channel (this pass's input colours);  e = (dr*dr + dg*dg) + db*db;
 *                     sc = sigma_color / (double)s;  wt = wt / (1.0 + e/(sc*sc))
 *       and the tap is skipped unless wt > 0.0 and all three channels of c_q are finite.
 *     a kept tap: sum_ch = sum_ch + wt*c_q_ch;  wsum = wsum + wt.
 *   v_ch = sum_ch / wsum.  Between passes v is rounded once to f32.
 * After the last pass, in f64 (RT_DN_DEMODULATE): v = a > 0.0 ? v*a : v.  out_rgb = (float)v; out_bgr = the sRGB
 *   byte of the f64 value v, B G R, as every pixel writer of the library forms it; rows of bgr_pitch bytes
 *   (0 -> 3*width) whose bytes past the pixels are left alone, as rt_render_device leaves them.
 * What follows from it: a non-finite pixel keeps to itself (its neighbours skip it, and it is its own centre
 *   tap); a pixel whose guide is NaN (a plane's 0/0 depth) keeps its own colour and is skipped by its neighbours
 *   (every weight but the centre's is NaN); miss pixels (normal 0) average only with themselves unless
 *   RT_DN_NORMAL is off.  A -0.0 that is kept comes back as +0.0 (the sums start from +0.0).  flags 0 is a plain
 *   B3 blur.
 *
 * variant: 0 the library's choice, 1 every pass reads its taps through L2 (direct), 2 the passes of steps 1 and 2
 *   stage the workgroup's tile and halo in LDS (later passes are direct in both).  The results are the same bits.
 * Scratch (two colour images and one guide image, 16 B per pixel each) belongs to the context, grows on demand
 *   and is freed by rt_ctx_destroy; RT_E_NOMEM when it does not fit.  Because it is shared, a call is ordered on
 *   the device after the context's previous denoise, whatever stream that ran on.
 * RT_E_INVALID, before anything changes: a null argument; width or height 0; iterations outside 1..8; unknown flag
 *   bits; normal_squarings > 10; variant > 2; a selected guide's pointer NULL (albedo for RT_DN_DEMODULATE); a
 *   selected sigma (sigma_depth with RT_DN_DEPTH, sigma_color with RT_DN_COLOR) that is not finite and > 0; both
 *   outputs NULL; a nonzero bgr_pitch below 3*width; out_rgb == rgb. */
enum rt_denoise_flags { RT_DN_NORMAL = 1, RT_DN_DEPTH = 2, RT_DN_COLOR = 4, RT_DN_DEMODULATE = 8 };
typedef struct {
    uint32_t width, height;
    uint32_t iterations;        /* 1..8: pass i has step 2^i */
    uint32_t flags;             /* rt_denoise_flags */
    uint32_t normal_squarings;  /* 0..10: the normal weight is max(dot, 0)^(2^normal_squarings) */
    uint32_t variant;           /* 0 auto, 1 direct, 2 LDS tiles at steps 1 and 2 */
    uint32_t bgr_pitch;         /* bytes per output BGR row; 0 -> 3*width */
    uint32_t _pad;
    double sigma_color;
    double sigma_depth;
} rt_denoise_params;
typedef struct {
    const float* rgb;
    const float* normal;
    const float* depth;
    const float* albedo;
} rt_denoise_inputs;
/* Asynchronous on `stream` (NULL: the context's own), DEVICE buffers; either output may be NULL, not both. */
int rt_denoise_device(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_inputs* dev, float* d_out_rgb,
                      uint8_t* d_out_bgr, void* stream);
/* Synchronous, HOST buffers: device buffers allocated, filled, filtered, copied back and freed.  No performance claim. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_inputs* host, float* out_rgb,
               uint8_t* out_bgr);
/* ---- denoiser, variance-guided: a colour weight scaled by the pixel's own noise (SVGF, Schied et al. 2017) ----
 * What a caller with a moments accumulator does: rt_accum_noise gives the variance of every pixel's mean, and the
 * filter then tells a colour edge that is signal (a shadow edge, a texture, a reflection: no normal or depth edge)
 * from one that is noise, pixel by pixel, where RT_DN_COLOR has one global sigma_color.
 *
 * The rule.  Every rule of rt_denoise above holds unchanged (f64, never fused, the written order, every f32 read
 * widened first); only the following is added.
 * Inputs: variance [h, w, 3] f32, tight, exactly what rt_accum_noise writes; sigma_variance and variance_floor.
 * Pack, per pixel p, one scalar variance: per channel k, u_k = (double)variance[3p+k]; with RT_DN_DEMODULATE and
 *   a_k > 0.0: u_k = u_k / (a_k*a_k); then u_k = u_k > 0.0 ? u_k : 0.0 (a NaN, a negative value and -0.0 become
 *   +0.0).  var_p = (float)((u_r + u_g) + u_b).
 * Pass i at pixel p, before the taps: gs = 0, gw = 0; for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = p + (dx, dy)
 *   (always one pixel apart, not the pass's step; a q outside the image is skipped):
 *     gk = G[|dy|] * G[|dx|], G = {1/2, 1/4};  gs = gs + gk*var_q;  gw = gw + gk
 *   g = gs / gw;  den = (sigma_variance*sigma_variance)*g + variance_floor;  vs = 0.
 *   any tap but the centre, after the RT_DN_COLOR step if that flag is set and before the skip test (unchanged):
 *     e = (dr*dr + dg*dg) + db*db as RT_DN_COLOR forms it (this pass's input colours);  wt = wt / (1.0 + e/den)
 *   a kept tap, the centre included: vs = vs + (wt*wt)*var_q.
 *   After the taps: x = vs / (wsum*wsum);  x = x > 0.0 ? x : 0.0.  Between passes (float)x is the pixel's variance,
 *   as the f32 colour is its colour.
 * After the last pass out_variance [h, w] f32 (optional) = (float)x.  With RT_DN_DEMODULATE it is in the units of
 *   the demodulated signal: it is not multiplied back by the albedo.
 * No sqrt, no exp: e and the variance are both colour squared.
 * What follows from it: every stored variance lies in [0, +inf] (never NaN, never negative).  With variance 2^100
 *   everywhere and colours of ordinary magnitude e/den < 2^-53, every new divisor is exactly 1.0, and out_rgb and
 *   out_bgr are rt_denoise's bit for bit under every flag mask.  A constant dyadic image is still a fixed point
 *   for any variance, and a non-finite colour pixel still keeps to itself.  With variance 0 everywhere a tap
 *   across a colour step e carries at most kw * variance_floor / e.
 *
 * Ordering, scratch (the same images: the variance rides in the colour record's fourth float, so the size is
 *   unchanged) and "not a render" are as for rt_denoise; a call is ordered after the context's previous denoise
 *   of either kind.
 * RT_E_INVALID, before anything changes: every refusal of rt_denoise in its order, with "all three outputs NULL"
 *   (out_rgb, out_bgr, out_variance) in the place of "both outputs NULL"; then a NULL rt_denoise_variance; a NULL
 *   variance; a sigma_variance or a variance_floor that is not finite and > 0; out_variance == variance. */
typedef struct {
    const float* variance;      /* [h, w, 3]: the variance of the mean, per channel (rt_accum_noise) */
    float* out_variance;        /* [h, w] or NULL: the filtered scalar variance */
    double sigma_variance;
    double variance_floor;
} rt_denoise_variance;
/* Asynchronous on `stream` (NULL: the context's own), DEVICE buffers; any output may be NULL, not all three. */
int rt_denoise_var_device(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_inputs* dev,
                          const rt_denoise_variance* dev_var, float* d_out_rgb, uint8_t* d_out_bgr, void* stream);
/* Synchronous, HOST buffers, as rt_denoise.  No performance claim. */
int rt_denoise_var(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_inputs* host,
                   const rt_denoise_variance* host_var, float* out_rgb, uint8_t* out_bgr);
/* ---- progressive rendering (main.rs:47-56 split over calls) ----
 * The reference's pixel is `res = BLACK; for _ in 0..antialias { res = res + raytrace(..) }; res / antialias`
 * (main.rs:47-56).  An rt_accum keeps `res` of every pixel of one tile on the device between calls: f64
 * running sums r, g, b (24 B per pixel, tile row-major) and the number of samples in them.  Every random draw
 * is keyed by (seed, pixel, AA sample index, ..) and by nothing that depends on the sample count, and a sum
 * is continued one sample at a time in sample order, so accumulating samples [0, k) and then [k, n) gives,
 * bit for bit, the one-shot render with spp = n and RT_JITTER_RANDOM (RT_ALGO_PATH / RT_ALGO_WAVEFRONT_AA),
 * and a resolve after k samples is exactly the one-shot render with spp = k.
 *
 * Lifetime: an accumulator belongs to the context it was created on.  Destroy it before the context, or
 * after: rt_ctx_destroy frees the device memory of the accumulators still alive, and the only call valid
 * on such an accumulator afterwards is rt_accum_destroy (every other answers RT_E_INVALID).  Like the
 * context's other calls, an accumulator's are not thread-safe. */
typedef struct rt_accum rt_accum;   /* f64 running sums r,g,b of one tile (24 B per pixel, tile row-major) + the number of samples in them */

/* main.rs:47 `let mut res = BLACK` for every pixel of the tile: binds the accumulator to the options that
 * define the image (width, height, x0, tile_w, y0, tile_h, band, band_stride, band_phase, max_depth, jitter,
 * seed) and to the scene uploaded at this moment (RT_E_NOSCENE without one).  opts->spp, algo, flags and
 * bgr_pitch are not bound.  After rt_scene_upload of another scene every call but rt_accum_samples,
 * rt_accum_reset and rt_accum_destroy answers RT_E_INVALID until rt_accum_reset. */
int rt_accum_create(rt_ctx* ctx, const rt_render_opts* opts, rt_accum** out);
void rt_accum_destroy(rt_accum* acc);
int rt_accum_samples(const rt_accum* acc, uint32_t* samples);
/* main.rs:47 again: samples = 0, bound to the scene uploaded now.  Nothing is cleared: the first sample
 * accumulated afterwards stores 0.0 + s_0 without reading. */
int rt_accum_reset(rt_accum* acc);
/* main.rs:48-55 for n_samples turns of the loop: traces samples [S, S + n_samples) of every tile pixel (S: the
 * accumulator's count) and adds each to the pixel's sum, in sample order, one at a time: for S == 0 the first
 * step stores 0.0 + s_0 (a -0.0 sample becomes +0.0, stale memory is never read), otherwise the sum is loaded,
 * the samples added, the sum stored.  No division.  Then the count is S + n_samples.  Asynchronous on `stream`
 * (NULL: the context's own), a render of the context, ordered on the device like every other; afterwards
 * rt_ctx_stats gives this call's own rays, shadow_rays, pixels, chunks and traced_rays == rays.  Every
 * sample is traced, also one sample or centre jitter.  algo: RT_ALGO_PATH (every class), RT_ALGO_WAVEFRONT_AA
 * (chain classes, at most 32 lights: one wavefront pass per sample), RT_ALGO_AUTO (the path kernel, unless
 * the scene is of chain classes with at most 32 lights and tuning aa_wavefront is 1); 1-4 -> RT_E_UNSUPPORTED.
 * Consecutive calls may use different algorithms.  flags: RT_COUNT_WORK and RT_TIME_KERNELS only.
 * n_samples 0: RT_OK, nothing rendered.  A count that would pass 2^31 -> RT_E_INVALID.  A refused call is no
 * render: the statistics stay the previous render's. */
int rt_render_accumulate(rt_ctx* ctx, rt_accum* acc, uint32_t n_samples, int32_t algo, uint32_t flags, void* stream);
/* main.rs:56 `(res / antialias).write_bgr(..)` with antialias = the accumulator's count, whenever wanted:
 * pixel = sum / (double)samples, rounded once to f32 (d_rgb, tile_h * tile_w * 3 floats) and quantised from
 * the f64 value (d_bgr, tile_h rows of bgr_pitch bytes, 0 -> 3 * tile_w); NaN propagates.  Either buffer may
 * be NULL.  Device buffers, asynchronous on `stream`, after the accumulates issued so far; the bytes of a row
 * past its pixels are left as they are.  The accumulator is not modified.  samples == 0 -> RT_E_INVALID.
 * Tile-shaped outputs only (no RT_OUT_FRAME_ROWS). */
int rt_accum_resolve(rt_ctx* ctx, rt_accum* acc, uint32_t bgr_pitch, void* d_rgb, void* d_bgr, void* stream);
/* The same into host buffers, synchronous; the bytes of a BGR row past its pixels are written as zero
 * (BMP row padding, main.rs:42). */
int rt_accum_resolve_host(rt_ctx* ctx, rt_accum* acc, uint32_t bgr_pitch, float* out_rgb, uint8_t* out_bgr);
/* The sums (3 * tile_w * tile_h doubles; cap_doubles smaller -> RT_E_INVALID) and the count, to the host and
 * back: with rt_checkpoint_write / read, main.rs:47-56 stopped in one process and continued in another.
 * Synchronous.  rt_accum_upload replaces sums and count (n_doubles must be 3 * tile_w * tile_h; samples
 * <= 2^31); samples 0 is rt_accum_reset. */
int rt_accum_download(rt_ctx* ctx, rt_accum* acc, double* sums, size_t cap_doubles, uint32_t* samples);
int rt_accum_upload(rt_ctx* ctx, rt_accum* acc, const double* sums, size_t n_doubles, uint32_t samples);
/* host only, no device: the checkpoint file of a progressive render.  Little-endian: an 88-byte header
 * (magic "RTAMDCKP", format version u32 = 1, then u32 width, height, x0, tile_w, y0, tile_h, band,
 * band_stride, band_phase, max_depth, i32 jitter, u32 samples, u32 reserved = 0, u64 seed, u64 scene_hash,
 * u64 pixels = tile_w * tile_h) followed by 3 * pixels f64 sums.  scene_hash: the caller's identification of the scene
 * (the CLI: FNV-1a 64 of the scene text).  rt_checkpoint_write writes n_doubles == 3 * tile_w * tile_h sums
 * (else RT_E_INVALID) to a temporary name beside `path` and renames it.  rt_checkpoint_read fills opts'
 * bound fields (the others zero), scene_hash and samples, and, with sums != NULL, the sums (cap_doubles
 * smaller than the file's -> RT_E_INVALID); sums NULL: header only.  RT_E_IO: the file cannot be opened;
 * RT_E_INVALID: wrong magic or version, a truncated file, a pixel count that is not tile_w * tile_h, a size
 * that would overflow.  Nothing of the file is trusted before it is checked. */
int rt_checkpoint_write(const char* path, const rt_render_opts* opts, uint64_t scene_hash, uint32_t samples, const double* sums, size_t n_doubles);
int rt_checkpoint_read(const char* path, rt_render_opts* opts, uint64_t* scene_hash, uint32_t* samples, double* sums, size_t cap_doubles);

/* ---- second moments: per-pixel variance and a noise count ------------------------------
 * A moments accumulator keeps, beside the sum S_c of every pixel and channel, the sum of squares Q_c (48 B
 * per pixel; the squares are a plane of their own after the tile's sums, both allocated at creation).  It is an
 * rt_accum in every other respect: rt_render_accumulate, rt_accum_resolve / resolve_host, rt_accum_download,
 * rt_accum_reset, rt_accum_samples and rt_accum_destroy take both kinds, S has the bits a plain accumulator has,
 * and the call's rays, shadow rays and statistics are the plain call's.  ABI version, structs, enums and
 * RT_KF_COUNT are unchanged: these are new functions only.
 *
 * The rule.  All arithmetic is f64; every operation written below is ONE IEEE operation: a product and the
 * sum or difference that follows it are two roundings, never an fma.
 *   Moments.  Sample k contributes q = s_c * s_c, s being the value added to S_c.  Sample 0 stores 0.0 + q
 *   without reading Q (stale memory is never read; rt_accum_reset clears nothing); sample k > 0 loads Q, adds q
 *   and stores.  A call never sums its own squares among themselves first, so Q, like S, does not depend on how
 *   the samples were split over calls or algorithms.  NaN and +-inf propagate as IEEE gives them.
 *   Estimate, for n = samples >= 2, N = (double)n:
 *     mean_c = S_c / N;  d_c = Q_c - (S_c * mean_c);
 *     v_c = (d_c < 0.0) ? 0.0 : d_c / (N * (N - 1.0))        (a NaN d_c stays NaN): the variance of the mean;
 *     err = sqrt((v_r + v_g) + v_b) / (floor + ((|mean_r| + |mean_g|) + |mean_b|));
 *     a pixel is above when !(err <= threshold), on the f64 value: a NaN err is above.
 *   variance: f32 [tile_h, tile_w, 3] = (float)v_c; error: f32 [tile_h, tile_w] = (float)err; above: the number
 *   of pixels above (an integer: independent of the order the device counts in). */
int rt_accum_create_moments(rt_ctx* ctx, const rt_render_opts* opts, rt_accum** out);   /* as rt_accum_create */
int rt_accum_has_moments(const rt_accum* acc, int32_t* flag);                            /* 1 or 0 */
/* rt_accum_upload on a moments accumulator -> RT_E_INVALID (it would leave Q stale).  These two move Q (3 * tile_w
 * * tile_h doubles; of no samples: zeros) and, uploading, replace sums, squares and count together; on a plain
 * accumulator -> RT_E_INVALID.  Synchronous, as rt_accum_download / upload. */
int rt_accum_download_moments(rt_ctx* ctx, rt_accum* acc, double* squares, size_t cap_doubles);
int rt_accum_upload_moments(rt_ctx* ctx, rt_accum* acc, const double* sums, const double* squares, size_t n_doubles, uint32_t samples);
/* The estimate.  d_variance / d_error: device buffers (3 * tile_w * tile_h / tile_w * tile_h floats), either may be
 * NULL (both NULL: the count alone).  Ordered like rt_accum_resolve: on `stream`, after the accumulates issued so
 * far, and the next accumulate waits for it; the call returns after synchronising on the result, with *above
 * written.  Reads S and Q, never writes them.  RT_E_INVALID, and nothing changed (*above included): a plain
 * accumulator, samples < 2, a floor or threshold that is not finite or not > 0, a stale scene binding.  Timed
 * under RT_KF_COMPOSE when the accumulator's last rt_render_accumulate had RT_TIME_KERNELS. */
int rt_accum_noise(rt_ctx* ctx, rt_accum* acc, double floor, double threshold, void* d_variance, void* d_error, uint64_t* above, void* stream);
/* ... into host memory (plain path: device buffers for the call, copies out). */
int rt_accum_noise_host(rt_ctx* ctx, rt_accum* acc, double floor, double threshold, float* variance, float* error, uint64_t* above);
/* host only: the checkpoint of a moments accumulator.  The same 88-byte header with format version 2, followed by
 * 3 * pixels f64 sums and then 3 * pixels f64 squares.  The version 2 reader refuses a version 1 file and
 * rt_checkpoint_read refuses a version 2 file (RT_E_INVALID both ways); otherwise as rt_checkpoint_write / read,
 * n_doubles / cap_doubles counting each of the two arrays (3 * tile_w * tile_h).  sums and squares both NULL:
 * header only. */
int rt_checkpoint_write_moments(const char* path, const rt_render_opts* opts, uint64_t scene_hash, uint32_t samples,
                                const double* sums, const double* squares, size_t n_doubles);
int rt_checkpoint_read_moments(const char* path, rt_render_opts* opts, uint64_t* scene_hash, uint32_t* samples, double* sums,
                               double* squares, size_t cap_doubles);
/* Diagnostic (device): the sphere test's division t = x / (2a) (shapes.rs:68,75)
 * computed as the device computes it (the per-ray reciprocal of 2a finished with
 * the division's own correction steps, DESIGN.md §4 "Division by 2a") -> fast[i],
 * and as the device's own f64 division -> slow[i], for n operand pairs.  Tests
 * compare both with IEEE division bit for bit.  Synchronous. */
int rt_div_a2_check(rt_ctx* ctx, const double* x, const double* a, uint32_t n, double* fast, double* slow);
/* Diagnostic (device): the sphere test's square root (shapes.rs:67) as the device
 * computes it (the f64 sqrt sequence without its scaling of operands below 2^-767,
 * DESIGN.md §4) -> fast[i], and the device's own sqrt -> slow[i].  Tests compare
 * both with IEEE sqrt bit for bit.  Synchronous. */
int rt_sqrt_check(rt_ctx* ctx, const double* x, uint32_t n, double* fast, double* slow);
/* Diagnostic (device): the conservative f32 culling arithmetic of the tree walks ("BVH
 * exactness" items 2, 3 and 6), computed by the functions the traversal kernels call, for n records.
 * Record i: rays[6 i ..] = ray origin and direction (f64); boxes[6 i ..] = box lo x, y, z, hi x, y, z
 * (f32); t[i] = a hit distance >= 0, or +inf for none; codes[i] = a node index or leaf code.  reach:
 * the culling domain a scene would carry (rt_cull_reach, an f32 value; +inf: every origin inside).  Outputs, 5 per
 * record: out_i = { the slab tests' exponent te (they run on t 2^te); the slab test's verdict (0 / 1)
 * with the limit out_f[0]; the verdict of the form the whole-LDS walk runs (near / far bounds); the
 * code read back from a 16-bit compact stack entry made of (codes[i], out_f[1]); from an 18-bit one };
 * out_f = { the f32 limit for t[i] in scaled t (>= t 2^te); the slab test's widened entry t; the near /
 * far form's; the entry t read back from the 16-bit compact entry; from the 18-bit one }.  A ray whose
 * origin lies beyond reach on some axis (finite as f32) reports both verdicts 1 and entry t 0 for
 * every finite box: the far-origin rule.  Tests compare with exact arithmetic on the host
 * (tests/test_gpu_culling.py).  Synchronous. */
int rt_cull_check(rt_ctx* ctx, uint32_t n, const double* rays, const float* boxes, const double* t, const int32_t* codes,
                  double reach, int32_t* out_i, float* out_f);
/* Diagnostic (device): the exact f64 sphere and plane tests (shapes.rs:60-89, 100-112), computed by the
 * functions the render kernels call, for n records.  Record i: records[16 i ..] = ray origin, ray direction,
 * sphere centre, sphere radius, plane point, plane normal (f64; the radius is squared on the host as the scene
 * upload squares it).  Outputs: out_i[3 i ..] = { hit of the branch-free sphere test (the form every LDS and
 * BVH walk runs); hit of the branchy form (the binary16 walk of trees beyond LDS); hit of the plane test };
 * out_d[15 i ..] = { t of the branch-free form; t of the branchy form; the plane's t as computed, whatever
 * the verdict (NaN, +-inf, +-0 included); hit point o + d t and normal (shapes.rs:61,66) of the branch-free
 * form's hit, 6 values; the same of the branchy form's }.  A sphere miss reports t 0 and a zero point and
 * normal.  Tests compare with an operation-by-operation f64 model that is pinned to the oracle
 * (tests/prim_model.py, tests/test_gpu_prims.py).  Synchronous. */
int rt_isect_check(rt_ctx* ctx, uint32_t n, const double* records, int32_t* out_i, double* out_d);
/* Diagnostic (device): the shading arithmetic of one hit, one material and one light (raytrace.rs:30-62,
 * 123-163; scene.rs:122-138), computed by the functions the render kernels call, and the device's pow, sin
 * and cos, for n records.  Record i: records[27 i ..] = hit point 3, shape normal 3 (as the intersection
 * returned it: the probe orients it against the ray as the kernels do), incoming ray direction 3, diffuse 3,
 * specular 3, exponent, ior, light location (point) or direction (directional) 3, light colour 3, the ray's
 * significance, then three operands of their own: x and y of pow(x, y), x of sin(x) and cos(x);
 * kinds[2 i ..] = { rt_material_kind (RT_MAT_PHONG or RT_MAT_FRESNEL), rt_light_kind (RT_LIGHT_POINT or
 * RT_LIGHT_DIRECTIONAL) }.  Outputs: out_i[3 i ..] = { the light has a range; the diffuse flag; the specular
 * flag (raytrace.rs:35-36 / 137-138) }; out_d[20 i ..] = { light direction 3; squared range; the Schlick factor
 * of the material's ior whatever its kind; the factor f the flags used (1 for Phong); the mirror ray's origin
 * and direction (raytrace.rs:60-62) 6; the half vector's clamped cosine c; p = pow(c, exponent); the colour one
 * unshadowed light adds to black with both flags on 3; pow(x, y); sin(x); cos(x) }.  Synchronous. */
int rt_shade_check(rt_ctx* ctx, uint32_t n, const double* records, const int32_t* kinds, int32_t* out_i, double* out_d);
/* host only: the culling domain of a scene whose spheres' largest finite |centre +- radius| is extent,
 * 32 (1 + extent) rounded down to f32: rays, shade points and cameras whose f32-rounded coordinates lie
 * within it on every axis are culled through the padded boxes, the others test every sphere (DESIGN.md
 * 4, "the far-origin rule"). */
double rt_cull_reach(double extent);
/* Queue sizes of the last wavefront chunk (RT_ALGO_WAVEFRONT_AA: of its last pass): queue[k] = rays traced at depth k
 * (generation 0: 0, the camera rays are not queued), shaded[k] = hits that
 * issued shadow queries.  Diagnostic. */
int rt_ctx_generation_counts(rt_ctx* ctx, uint32_t* queue, uint32_t* shaded, int n);
/* Per kernel family, over every RT_TIME_KERNELS render since the previous
 * call: summed launch time (ms, hipEvent pairs around each launch) and launch
 * count; then resets.  Synchronises with the last timed launch.  Families:
 * rt_kernel_family.  Renders split over several chunk streams are not timed. */
enum rt_kernel_family {
    RT_KF_NEAREST = 0,      /* wf_nearest, generations >= 1; query_nearest of an RT_TIME_KERNELS rt_query_nearest */
    RT_KF_OCCLUSION = 1,    /* wf_occlusion: every (record, light) pair of a generation; query_occluded of an
                               RT_TIME_KERNELS rt_query_occluded */
    RT_KF_SHADE = 2,        /* wf_shade */
    RT_KF_FOLD = 3,         /* wf_fold */
    RT_KF_TALLY = 4,        /* wf_tally */
    RT_KF_CAMERA = 5,       /* wf_nearest, generation 0 (camera rays); aov_primary of an RT_TIME_KERNELS AOV render */
    RT_KF_COMPOSE = 6,      /* wf_compose: the row-ordered frame pass (tuning compose); RT_ALGO_WAVEFRONT_AA:
                               accum_resolve after a chunk's last pass (and wf_aa_compose per pass, tuning compose);
                               accum_resolve of an rt_accum_resolve after an RT_TIME_KERNELS rt_render_accumulate;
                               skybox scenes: wf_sky_pixels after the camera pass (compose 0) and wf_sky_term
                               before each fold */
    RT_KF_TAIL = 7,         /* wf_tail: the fused generations >= tail_fuse */
    RT_KF_COUNT = 8
};
int rt_ctx_kernel_times(rt_ctx* ctx, double* ms, uint32_t* launches, int n);

/* Schedule tuning of a context (A/B measurement; the defaults are the measured
 * best).  Keys (rt_tuning_key(i) for i = 0, 1, ... until NULL):
 * chunk_pixels (wavefront chunk cap, 0: from the working-set budget), bvh_leaf, light_grids, light_grid_res
 * (these three take effect at the next rt_scene_upload), src, src_occ (the
 * nearest-hit and shadow sphere sources, wf_device.hpp kSrc*; an unsupported
 * pair falls back to the binary tree through L2), prefix_kb (KB of the tree's
 * top staged in LDS for trees beyond LDS), lanes, stagger_gen, regions, split,
 * bstreams, cam (generation 0: 3 the camera's view grid, -1 where built, other
 * values per ray), deal, spread_below, path_group, cu_mask, prio, verbose,
 * grid_occ, compact_stack (small trees: 32-bit nearest-hit stack entries),
 * half_nodes (trees beyond LDS: binary16 node bounds for the prefix walk),
 * wf_budget_mb (wavefront working set of all chunk lanes, MB; 0: min(80 GB, 85%
 * of the device's free memory); a hipMalloc that still fails halves the chunks),
 * cam_grid_res (the view grid's cells per face side, 0 from the scene's frame
 * size, -1 none; at the next rt_scene_upload), a_queue (1: the nearest-hit
 * chain's stream gets a hardware queue of its own), tail_fuse (T >= 1: the
 * chains still running at generation T-1 of a frame on the src-9 tree whose
 * lights all have light-view grids finish in one launch, one chain per
 * work-item through its remaining bounces, folded there; 0 off, -1 auto),
 * tail_width (that launch's chains per wave, 0 auto), qtree (1: trees beyond
 * LDS take the quantised 4-wide tree for the nearest hit), compose (1: the
 * chains' final colours go to a per-chain buffer and one row-ordered pass,
 * RT_KF_COMPOSE, writes the frame with coalesced stores; 0: each chain writes
 * its pixel as it ends), host_chunks (rt_render into host memory: at least
 * this many chunks, the D2H copy of each chunk's rows overlapping the later
 * chunks), host_first (with host_chunks 2: the first chunk's percentage of
 * the rows, 0 equal), sparse_out (rt_render into host memory, a one-chunk
 * wavefront render: the frame is copied after the camera pass while the
 * generations run, then only the 16-pixel row segments holding pixels whose
 * chain was still running, packed on the device), chain_on_caller (1: a
 * one-lane render's nearest-hit chain runs on the caller's stream itself, no
 * fork and join between hardware queues; 0: on the context's high-priority
 * chain stream), copy_engine (rt_render's device -> host copies: 0
 * hipMemcpyAsync, e = 1..16 the device's SDMA engine e - 1 driven directly,
 * -1 its engines 0-3 in turn, -2 (default) -1 for a row-banded tile
 * (band_stride > 1) and 0 otherwise; a device without usable engines takes
 * hipMemcpyAsync), dev_join (1: the b streams join the chain's
 * stream on the device, a one-wave kernel polling flags that the b streams set
 * after their work; 0: through events; a join that waits 2 s gives up and
 * makes the next rt_render or rt_ctx_stats fail; the default is 0 in a process whose
 * kernels are serialised, ROCPROF_COUNTER_COLLECTION or AMD_SERIALIZE_KERNEL
 * set, where the b streams could not run beside the join), aa_wavefront (1:
 * RT_ALGO_AUTO renders a scene of the chain classes with at most 32 lights, random
 * jitter and spp > 1 as RT_ALGO_WAVEFRONT_AA instead of RT_ALGO_PATH; default 0).
 * cu_mask, prio and a_queue rebuild the context's streams (after pending work) when changed.
 * Unknown key or value out of range -> RT_E_INVALID.  Results never depend on
 * them (tests/test_gpu_parity.py renders under several and compares bits). */
int rt_ctx_set_tuning(rt_ctx* ctx, const char* key, int64_t value);
int rt_ctx_get_tuning(const rt_ctx* ctx, const char* key, int64_t* value);
const char* rt_tuning_key(int index);

#ifdef __cplusplus
}
#endif
#endif
