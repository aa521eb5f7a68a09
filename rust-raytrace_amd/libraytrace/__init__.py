"""ctypes binding of librtamd.so (include/raytrace_amd.h) for tests and bench.

The product is the C ABI + HIP kernels; this module is plumbing that lets the
pytest suite and bench.py drive it.  The names mirror the reference crate
`libraytrace` (Cargo.toml [lib] name): `Scene` (scene.rs:201), `deserialize`
(serialize.rs:427), `Context.render` (the pixel loop of main.rs:45-57),
`to_srgb` (color.rs:593), `bmp_header` (bmp.rs:10).

There is NO CPU fallback: if librtamd.so cannot be loaded the import fails,
and device calls without a GPU raise RtError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
# RT_LIBRTAMD: an alternative build of the same library (A/B measurement)
LIB_PATH = os.environ.get("RT_LIBRTAMD") or os.path.join(PKG_DIR, "librtamd.so")
HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "raytrace_amd.h")

RT_ABI_VERSION = 10              # include/raytrace_amd.h
RT_OK = 0
RT_E_INVALID, RT_E_NODEVICE, RT_E_HIP, RT_E_NOMEM = -1, -2, -3, -4
RT_E_UNSUPPORTED, RT_E_PARSE, RT_E_NOSCENE, RT_E_IO = -5, -6, -7, -8
RT_SHAPE_SPHERE, RT_SHAPE_PLANE = 0, 1
RT_MAT_PHONG, RT_MAT_INDIRECT_PHONG, RT_MAT_FRESNEL, RT_MAT_TRANSPARENT = 0, 1, 2, 3
RT_LIGHT_POINT, RT_LIGHT_DIRECTIONAL, RT_LIGHT_AREA = 0, 1, 2
RT_CAMERA_SIMPLE, RT_CAMERA_DOF = 0, 1
RT_BG_SOLID, RT_BG_SKYBOX = 0, 1
RT_OUT_RGB_F32, RT_OUT_BGR_U8, RT_COUNT_WORK, RT_TIME_KERNELS, RT_OUT_FRAME_ROWS = 1, 2, 4, 8, 16
KERNEL_FAMILIES = ("nearest", "occlusion", "shade", "fold", "tally", "camera", "compose", "tail")   # rt_kernel_family
RT_ALGO_AUTO, RT_ALGO_BRUTE_LDS, RT_ALGO_BRUTE_GLOBAL, RT_ALGO_WAVEFRONT, RT_ALGO_WAVEFRONT_BRUTE = 0, 1, 2, 3, 4
RT_ALGO_PATH = 5
RT_ALGO_WAVEFRONT_AA = 6        # one wavefront pass per jittered AA sample
RT_JITTER_CENTER, RT_JITTER_RANDOM = 0, 1
RT_AOV_DEPTH, RT_AOV_NORMAL, RT_AOV_ALBEDO, RT_AOV_COVERAGE, RT_AOV_OBJECT = 1, 2, 4, 8, 16     # rt_aov
RT_AOV_ALL = 31
RT_DN_NORMAL, RT_DN_DEPTH, RT_DN_COLOR, RT_DN_DEMODULATE = 1, 2, 4, 8                      # rt_denoise_flags
# rt_aov bit -> (rt_aov_buffers field, elements per pixel, dtype)
AOV_CHANNELS = {RT_AOV_DEPTH: ("depth", 1, np.float32), RT_AOV_NORMAL: ("normal", 3, np.float32),
                RT_AOV_ALBEDO: ("albedo", 3, np.float32), RT_AOV_COVERAGE: ("coverage", 1, np.float32),
                RT_AOV_OBJECT: ("object", 1, np.int32)}
RT_HIT_T, RT_HIT_OBJECT, RT_HIT_NORMAL = 1, 2, 4      # rt_hit_channel
RT_HIT_ALL = 7
# rt_hit_channel bit -> (rt_hit_buffers field, elements per ray, dtype)
HIT_CHANNELS = {RT_HIT_T: ("t", 1, np.float64), RT_HIT_OBJECT: ("object", 1, np.int32), RT_HIT_NORMAL: ("normal", 3, np.float64)}
RT_MAX_DEPTH_LIMIT = 30


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt error {code}: {msg}")
        self.code = code


class rt_color(C.Structure):
    _fields_ = [("r", C.c_double), ("g", C.c_double), ("b", C.c_double)]


class rt_object(C.Structure):
    _fields_ = [("shape", C.c_int32), ("material", C.c_int32), ("geom", C.c_double * 6),
                ("diffuse", rt_color), ("specular", rt_color), ("ambient", rt_color),
                ("exponent", C.c_double), ("ior", C.c_double), ("samples", C.c_uint32), ("_pad", C.c_uint32)]


class rt_light(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("v", C.c_double * 9), ("color", rt_color)]


class rt_camera(C.Structure):
    _fields_ = [("kind", C.c_int32), ("samples", C.c_uint32), ("position", C.c_double * 3),
                ("matrix", C.c_double * 9), ("focus", C.c_double), ("aperture", C.c_double)]


class rt_texture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_uint8))]


class rt_scene_desc(C.Structure):
    _fields_ = [("objects", C.POINTER(rt_object)), ("n_objects", C.c_uint32),
                ("lights", C.POINTER(rt_light)), ("n_lights", C.c_uint32),
                ("camera", rt_camera), ("background_kind", C.c_int32), ("background", rt_color),
                ("width", C.c_uint32), ("height", C.c_uint32), ("antialias", C.c_uint32)]


class rt_render_opts(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("x0", C.c_uint32), ("tile_w", C.c_uint32),
                ("y0", C.c_uint32), ("tile_h", C.c_uint32), ("band", C.c_uint32), ("band_stride", C.c_uint32),
                ("band_phase", C.c_uint32), ("max_depth", C.c_uint32), ("spp", C.c_uint32),
                ("jitter", C.c_int32), ("flags", C.c_uint32), ("algo", C.c_int32),
                ("bgr_pitch", C.c_uint32), ("_pad", C.c_uint32), ("seed", C.c_uint64)]


class rt_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("pixels", C.c_uint64),
                ("kernel_ms", C.c_double), ("box_tests", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("shadow_box_tests", C.c_uint64), ("shadow_sphere_tests", C.c_uint64), ("traced_rays", C.c_uint64),
                ("chunks", C.c_uint64)]


class rt_aov_buffers(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("coverage", C.c_void_p),
                ("object", C.c_void_p)]


class rt_hit_buffers(C.Structure):
    _fields_ = [("t", C.c_void_p), ("object", C.c_void_p), ("normal", C.c_void_p)]


class rt_denoise_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32),
                ("normal_squarings", C.c_uint32), ("variant", C.c_uint32), ("bgr_pitch", C.c_uint32), ("_pad", C.c_uint32),
                ("sigma_color", C.c_double), ("sigma_depth", C.c_double)]


class rt_denoise_inputs(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("albedo", C.c_void_p)]


class rt_denoise_variance(C.Structure):
    _fields_ = [("variance", C.c_void_p), ("out_variance", C.c_void_p), ("sigma_variance", C.c_double),
                ("variance_floor", C.c_double)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make -C rust-raytrace_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    sig = {
        "rt_scene_parse": (C.c_int, [C.c_char_p, C.c_size_t, P(C.c_void_p), C.c_char_p, C.c_size_t]),
        "rt_scene_from_desc": (C.c_int, [P(rt_scene_desc), P(C.c_void_p)]),
        "rt_scene_get_desc": (C.c_int, [C.c_void_p, P(rt_scene_desc)]),
        "rt_scene_free": (None, [C.c_void_p]),
        "rt_scene_set_skybox": (C.c_int, [C.c_void_p, P(rt_texture)]),
        "rt_texture_load": (C.c_int, [C.c_char_p, P(C.c_uint32), P(C.c_uint32), P(C.c_uint8), C.c_size_t]),
        "rt_camera_simple_new": (C.c_int, [P(C.c_double), P(C.c_double), P(C.c_double), C.c_double, P(rt_camera)]),
        "rt_camera_look_at": (C.c_int, [P(C.c_double), P(C.c_double), P(C.c_double), C.c_double, C.c_double,
                                        P(rt_camera)]),
        "rt_to_srgb": (C.c_uint8, [C.c_double]),
        "rt_bmp_header": (C.c_int, [P(C.c_uint8), C.c_uint32, C.c_uint32, P(C.c_uint32)]),
        "rt_write_bmp": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, P(C.c_uint8), C.c_uint32]),
        "rt_abi_version": (C.c_int, []),
        "rt_device_count": (C.c_int, [P(C.c_int)]),
        "rt_ctx_create": (C.c_int, [C.c_int, P(C.c_void_p)]),
        "rt_ctx_destroy": (None, [C.c_void_p]),
        "rt_last_error": (C.c_char_p, [C.c_void_p]),
        "rt_scene_upload": (C.c_int, [C.c_void_p, C.c_void_p]),
        "rt_render_opts_default": (None, [P(rt_render_opts), C.c_uint32, C.c_uint32]),
        "rt_render": (C.c_int, [C.c_void_p, P(rt_render_opts), P(C.c_float), P(C.c_uint8), P(rt_stats)]),
        "rt_render_device": (C.c_int, [C.c_void_p, P(rt_render_opts), C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_ctx_reserve": (C.c_int, [C.c_void_p, P(rt_render_opts), C.c_int, C.c_void_p]),
        "rt_ctx_stats": (C.c_int, [C.c_void_p, P(rt_stats)]),
        "rt_render_aov": (C.c_int, [C.c_void_p, P(rt_render_opts), C.c_uint32, P(rt_aov_buffers), P(rt_stats)]),
        "rt_render_aov_device": (C.c_int, [C.c_void_p, P(rt_render_opts), C.c_uint32, P(rt_aov_buffers), C.c_void_p]),
        "rt_query_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(rt_hit_buffers), C.c_uint32,
                                       P(rt_stats)]),
        "rt_query_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                        P(rt_stats)]),
        "rt_query_nearest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(rt_hit_buffers),
                                              C.c_uint32, C.c_void_p]),
        "rt_query_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.c_void_p]),
        "rt_denoise": (C.c_int, [C.c_void_p, P(rt_denoise_params), P(rt_denoise_inputs), C.c_void_p, C.c_void_p]),
        "rt_denoise_device": (C.c_int, [C.c_void_p, P(rt_denoise_params), P(rt_denoise_inputs), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
        "rt_denoise_var": (C.c_int, [C.c_void_p, P(rt_denoise_params), P(rt_denoise_inputs), P(rt_denoise_variance),
                                     C.c_void_p, C.c_void_p]),
        "rt_denoise_var_device": (C.c_int, [C.c_void_p, P(rt_denoise_params), P(rt_denoise_inputs), P(rt_denoise_variance),
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_accum_create": (C.c_int, [C.c_void_p, P(rt_render_opts), P(C.c_void_p)]),
        "rt_accum_destroy": (None, [C.c_void_p]),
        "rt_accum_samples": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
        "rt_accum_reset": (C.c_int, [C.c_void_p]),
        "rt_render_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_void_p]),
        "rt_accum_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_accum_resolve_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, P(C.c_float), P(C.c_uint8)]),
        "rt_accum_download": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_double), C.c_size_t, P(C.c_uint32)]),
        "rt_accum_upload": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_double), C.c_size_t, C.c_uint32]),
        "rt_checkpoint_write": (C.c_int, [C.c_char_p, P(rt_render_opts), C.c_uint64, C.c_uint32, P(C.c_double),
                                          C.c_size_t]),
        "rt_checkpoint_read": (C.c_int, [C.c_char_p, P(rt_render_opts), P(C.c_uint64), P(C.c_uint32), P(C.c_double),
                                         C.c_size_t]),
        "rt_accum_create_moments": (C.c_int, [C.c_void_p, P(rt_render_opts), P(C.c_void_p)]),
        "rt_accum_has_moments": (C.c_int, [C.c_void_p, P(C.c_int32)]),
        "rt_accum_download_moments": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_double), C.c_size_t]),
        "rt_accum_upload_moments": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_double), P(C.c_double), C.c_size_t, C.c_uint32]),
        "rt_accum_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, P(C.c_uint64),
                                     C.c_void_p]),
        "rt_accum_noise_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, P(C.c_float), P(C.c_float),
                                          P(C.c_uint64)]),
        "rt_checkpoint_write_moments": (C.c_int, [C.c_char_p, P(rt_render_opts), C.c_uint64, C.c_uint32, P(C.c_double),
                                                  P(C.c_double), C.c_size_t]),
        "rt_checkpoint_read_moments": (C.c_int, [C.c_char_p, P(rt_render_opts), P(C.c_uint64), P(C.c_uint32), P(C.c_double),
                                                 P(C.c_double), C.c_size_t]),
        "rt_ctx_generation_counts": (C.c_int, [C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_int]),
        "rt_ctx_kernel_times": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_uint32), C.c_int]),
        "rt_light_grid_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(C.c_double), C.c_uint32,
                                               P(C.c_int32), P(C.c_int32), C.c_size_t, P(C.c_int64)]),
        "rt_view_grid_candidates": (C.c_int, [C.c_void_p, C.c_int, P(C.c_double), C.c_uint32, P(C.c_int32),
                                              P(C.c_int32), P(C.c_float), C.c_size_t, P(C.c_int64)]),
        "rt_qtree_nodes": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, P(C.c_float), P(C.c_int32), P(C.c_int32),
                                     C.c_size_t, P(C.c_int64)]),
        "rt_div_a2_check": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double), C.c_uint32, P(C.c_double),
                                      P(C.c_double)]),
        "rt_sqrt_check": (C.c_int, [C.c_void_p, P(C.c_double), C.c_uint32, P(C.c_double), P(C.c_double)]),
        "rt_cull_check": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_float), P(C.c_double), P(C.c_int32),
                                    C.c_double, P(C.c_int32), P(C.c_float)]),
        "rt_isect_check": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_int32), P(C.c_double)]),
        "rt_shade_check": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_int32), P(C.c_int32), P(C.c_double)]),
        "rt_cull_reach": (C.c_double, [C.c_double]),
        "rt_ctx_set_tuning": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
        "rt_ctx_get_tuning": (C.c_int, [C.c_void_p, C.c_char_p, P(C.c_int64)]),
        "rt_tuning_key": (C.c_char_p, [C.c_int]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if lib.rt_abi_version() != RT_ABI_VERSION:      # the ctypes mirrors below follow this header version
        raise ImportError(f"{LIB_PATH} has ABI {lib.rt_abi_version()}, these bindings expect {RT_ABI_VERSION}: rebuild")
    return lib


lib = _load()


def _err(ctx=None):
    m = lib.rt_last_error(ctx)
    return m.decode(errors="replace") if m else ""


def _check(rc, ctx=None):
    if rc != RT_OK:
        raise RtError(rc, _err(ctx))


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def camera_simple_new(position, look, up, im_dist):
    """camera.rs:51-63"""
    cam = rt_camera()
    _check(lib.rt_camera_simple_new(_d3(position), _d3(look), _d3(up), float(im_dist), C.byref(cam)))
    return cam


def camera_look_at(focus, look, up, pov, h):
    """camera.rs:67-73"""
    cam = rt_camera()
    _check(lib.rt_camera_look_at(_d3(focus), _d3(look), _d3(up), float(pov), float(h), C.byref(cam)))
    return cam


def to_srgb(v):
    """color.rs:593-600"""
    return lib.rt_to_srgb(float(v))


def bmp_header(width, height):
    """bmp.rs:10-61 -> (122 header bytes, bytewidth)"""
    buf = (C.c_uint8 * 122)()
    bw = C.c_uint32()
    _check(lib.rt_bmp_header(buf, width, height, C.byref(bw)))
    return bytes(buf), bw.value


def texture_load(path):
    """texture.rs:34-37 Texture::load -> uint8 [height, width, 3], rows top-down (BMP / binary PPM)."""
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib.rt_texture_load(path.encode(), C.byref(w), C.byref(h), None, 0))
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib.rt_texture_load(path.encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                               out.size))
    return out


def write_bmp(path, width, height, bgr, pitch):
    arr = np.ascontiguousarray(bgr, dtype=np.uint8)
    _check(lib.rt_write_bmp(path.encode(), width, height, arr.ctypes.data_as(C.POINTER(C.c_uint8)), pitch))


class Scene:
    """A parsed / built scene (scene.rs:201-212), owned by the C library."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    @classmethod
    def deserialize(cls, text):
        """serialize.rs:427: parse scene text, raising RtError(RT_E_PARSE, "row:col: ...")."""
        raw = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = lib.rt_scene_parse(raw, len(raw), C.byref(h), err, 512)
        if rc != RT_OK:
            raise RtError(rc, err.value.decode(errors="replace"))
        return cls(h.value)

    @classmethod
    def from_desc(cls, desc):
        h = C.c_void_p()
        _check(lib.rt_scene_from_desc(C.byref(desc), C.byref(h)))
        return cls(h.value)

    def view_grid_candidates(self, dirs, cap=1 << 23, resolution=0):
        """Diagnostic (host only): for each camera-ray direction, (object ids,
        distance bounds) the camera's view grid hands the device (None when it
        tests every sphere), and (R, stored cells, list entries)."""
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = d.shape[0]
        counts = np.zeros(n, np.int32)
        ids = np.zeros(cap, np.int32)
        nears = np.zeros(cap, np.float32)
        info = np.zeros(3, np.int64)
        _check(lib.rt_view_grid_candidates(self._h, int(resolution), d.ctypes.data_as(C.POINTER(C.c_double)), n,
                                           counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                           ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                           nears.ctypes.data_as(C.POINTER(C.c_float)), cap,
                                           info.ctypes.data_as(C.POINTER(C.c_int64))))
        out, at = [], 0
        for c in counts:
            if c < 0:
                out.append(None)
            else:
                out.append((ids[at:at + c].copy(), nears[at:at + c].copy()))
                at += c
        return out, tuple(int(x) for x in info)

    def light_grid_candidates(self, light, points, cap=1 << 22, resolution=0):
        """Diagnostic (host only): for each point p, the object ids the light-view
        grid of point light `light` hands a shadow query from p (None when the
        device tests every sphere), and (R, stored cells, list entries).
        resolution: cells per face side (0 = the upload's automatic choice)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        counts = np.zeros(n, np.int32)
        ids = np.zeros(cap, np.int32)
        info = np.zeros(3, np.int64)
        _check(lib.rt_light_grid_candidates(self._h, light, int(resolution), pts.ctypes.data_as(C.POINTER(C.c_double)), n,
                                            counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                            ids.ctypes.data_as(C.POINTER(C.c_int32)), cap,
                                            info.ctypes.data_as(C.POINTER(C.c_int64))))
        out, at = [], 0
        for c in counts:
            if c < 0:
                out.append(None)
            else:
                out.append(ids[at:at + c].copy())
                at += c
        return out, tuple(int(x) for x in info)

    def qtree_nodes(self, leaf_max=0, cap=1 << 16):
        """Diagnostic (host only): the quantised 4-wide tree rt_scene_upload builds
        (DevQNode4 records as a structured array, empty when not representable),
        the f32 child boxes [n, 4, 6] (lo xyz, hi xyz; NaN unused), each slot's
        leaf spheres (first, count; -1 / 0 for inner children) and (nodes, stack
        worst case, leaf size)."""
        dt = np.dtype([("frame", "<i4", 3), ("base", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("child", "<u2", 4)])
        assert dt.itemsize == 48
        nodes = np.zeros(cap, dt)
        boxes = np.zeros((cap, 4, 6), np.float32)
        first = np.zeros((cap, 4), np.int32)
        count = np.zeros((cap, 4), np.int32)
        info = np.zeros(3, np.int64)
        _check(lib.rt_qtree_nodes(self._h, int(leaf_max), nodes.ctypes.data_as(C.c_void_p),
                                  boxes.ctypes.data_as(C.POINTER(C.c_float)), first.ctypes.data_as(C.POINTER(C.c_int32)),
                                  count.ctypes.data_as(C.POINTER(C.c_int32)), cap, info.ctypes.data_as(C.POINTER(C.c_int64))))
        n = int(info[0])
        return nodes[:n].copy(), boxes[:n].copy(), first[:n].copy(), count[:n].copy(), tuple(int(x) for x in info)

    def set_skybox(self, faces):
        """SkyboxBackground { px, nx, py, ny, pz, nz } from six uint8 [h, w, 3] arrays (copied)."""
        arrs = [np.ascontiguousarray(f, dtype=np.uint8) for f in faces]
        assert len(arrs) == 6 and all(a.ndim == 3 and a.shape[2] == 3 for a in arrs)
        tex = (rt_texture * 6)()
        for t, a in zip(tex, arrs):
            t.width, t.height = a.shape[1], a.shape[0]
            t.rgb = a.ctypes.data_as(C.POINTER(C.c_uint8))
        _check(lib.rt_scene_set_skybox(self._h, tex))

    def desc(self):
        d = rt_scene_desc()
        _check(lib.rt_scene_get_desc(self._h, C.byref(d)))
        d._owner = self          # the desc borrows the scene's arrays: keep the scene alive
        return d

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib.rt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cull_reach(extent):
    """rt_cull_reach: the culling domain of a scene whose spheres' largest |centre +- radius| is extent."""
    return lib.rt_cull_reach(float(extent))


def device_count():
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    return n.value


def render_opts(width, height, **kw):
    o = rt_render_opts()
    lib.rt_render_opts_default(C.byref(o), width, height)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown render option {k}")
        setattr(o, k, v)
    return o


def denoise_params(width, height, iterations=5, flags=RT_DN_NORMAL | RT_DN_DEPTH, normal_squarings=5, variant=0,
                   bgr_pitch=0, sigma_color=1.0, sigma_depth=0.05):
    """An rt_denoise_params; the defaults are the settings the denoiser was tried with."""
    return rt_denoise_params(width=width, height=height, iterations=iterations, flags=flags,
                             normal_squarings=normal_squarings, variant=variant, bgr_pitch=bgr_pitch, _pad=0,
                             sigma_color=sigma_color, sigma_depth=sigma_depth)


def sources_id():
    """16 hex digits identifying the native sources (csrc/ and include/) this
    checkout builds: ties committed profile figures (profiles/pmc_traffic.json)
    to the kernels they were measured on."""
    import hashlib
    h = hashlib.sha256()
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (os.path.join(pkg, "csrc"), os.path.join(os.path.dirname(pkg), "include")):
        for name in sorted(os.listdir(d)):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def tuning_keys():
    keys, i = [], 0
    while True:
        k = lib.rt_tuning_key(i)
        if not k:
            return keys
        keys.append(k.decode())
        i += 1


def env_tuning(text=None):
    """Tuning from RT_TUNE="key=value,key=value" (a convenience of this binding
    for A/B tools, read only when asked: Context(tuning="env"); the library
    itself never reads the environment).  Malformed items raise ValueError."""
    text = os.environ.get("RT_TUNE", "") if text is None else text
    out = {}
    for item in filter(None, (x.strip() for x in text.split(","))):
        k, sep, v = item.partition("=")
        if not sep or not k.strip():
            raise ValueError(f"RT_TUNE item {item!r} is not key=value")
        try:
            out[k.strip()] = int(v)
        except ValueError:
            raise ValueError(f"RT_TUNE item {item!r}: value is not an integer") from None
    return out


class Context:
    """One device (rt_ctx).  Mirrors the reference's main.rs render step.
    tuning: {key: value} schedule knobs (rt_ctx_set_tuning); "env" = the RT_TUNE
    environment variable (A/B tools); None = the library's defaults."""

    def __init__(self, device=0, tuning=None):
        h = C.c_void_p()
        _check(lib.rt_ctx_create(device, C.byref(h)))
        self._h = h
        self.device = device
        for k, v in (env_tuning() if tuning == "env" else (tuning or {})).items():
            self.set_tuning(k, v)

    def set_tuning(self, key, value):
        _check(lib.rt_ctx_set_tuning(self._h, key.encode(), int(value)), self._h)

    def get_tuning(self, key):
        v = C.c_int64()
        _check(lib.rt_ctx_get_tuning(self._h, key.encode(), C.byref(v)), self._h)
        return v.value

    def upload(self, scene):
        _check(lib.rt_scene_upload(self._h, scene.handle), self._h)

    def render(self, opts, rgb=True, bgr=True, out=None, stats=True):
        """Synchronous render of opts' tile into host numpy arrays.
        Returns (rgb float32 [tile_h, tile_w, 3] or None, bgr uint8 [tile_h, pitch] or None, stats).
        With RT_OUT_FRAME_ROWS in opts.flags, out= holds whole-frame arrays (height rows) and the tile's
        rows are written into their frame rows.
        out: (rgb, bgr) arrays to reuse (either None to skip that output); stats=False passes
        no rt_stats (the drop-in call of INTEGRATION.md: no counter read-back), returns None."""
        frame = bool(opts.flags & RT_OUT_FRAME_ROWS)
        pitch = opts.bgr_pitch or 3 * (opts.width if frame else opts.tile_w)
        rows, cols = (opts.height, opts.width) if frame else (opts.tile_h, opts.tile_w)
        if out is not None:
            out_rgb, out_bgr = out
            rgb, bgr = out_rgb is not None, out_bgr is not None
            assert not rgb or (out_rgb.dtype == np.float32 and out_rgb.size >= rows * cols * 3
                               and out_rgb.flags.c_contiguous)
            assert not bgr or (out_bgr.dtype == np.uint8 and out_bgr.size >= rows * pitch
                               and out_bgr.flags.c_contiguous)
        else:
            assert not frame, "RT_OUT_FRAME_ROWS renders into caller frames: pass out=(rgb, bgr)"
            out_rgb = np.zeros((opts.tile_h, opts.tile_w, 3), np.float32) if rgb else None
            out_bgr = np.full((opts.tile_h, pitch), 0xCD, np.uint8) if bgr else None
        st = rt_stats() if stats else None
        rc = lib.rt_render(self._h, C.byref(opts),
                           out_rgb.ctypes.data_as(C.POINTER(C.c_float)) if rgb else None,
                           out_bgr.ctypes.data_as(C.POINTER(C.c_uint8)) if bgr else None,
                           C.byref(st) if stats else None)
        _check(rc, self._h)
        return out_rgb, out_bgr, st

    def render_device(self, opts, d_rgb_ptr, d_bgr_ptr, stream_ptr=None):
        """Asynchronous render into device buffers (raw pointers, e.g. torch tensor.data_ptr())."""
        _check(lib.rt_render_device(self._h, C.byref(opts), C.c_void_p(d_rgb_ptr or 0),
                                    C.c_void_p(d_bgr_ptr or 0), C.c_void_p(stream_ptr or 0)), self._h)

    def render_aov(self, opts, channels=RT_AOV_ALL, out=None, stats=True):
        """rt_render_aov: the first-hit feature buffers of opts' tile (synchronous) -> ({name: array}, stats).
        Arrays: depth, coverage float32 [tile_h, tile_w]; normal, albedo float32 [tile_h, tile_w, 3]; object
        int32 [tile_h, tile_w]; only the selected channels.  out: {name: array} to write into instead (a
        selected channel missing from it is passed as NULL: the call is refused)."""
        arrays, bufs = {}, rt_aov_buffers()
        for bit, (name, n, dt) in AOV_CHANNELS.items():
            if out is not None:
                a = out.get(name)
                if a is not None:
                    assert a.dtype == dt and a.size >= opts.tile_h * opts.tile_w * n and a.flags.c_contiguous
            elif channels & bit:
                a = np.zeros((opts.tile_h, opts.tile_w) + ((n,) if n > 1 else ()), dt)
            else:
                a = None
            if a is not None:
                arrays[name] = a
                setattr(bufs, name, a.ctypes.data)
        st = rt_stats() if stats else None
        _check(lib.rt_render_aov(self._h, C.byref(opts), int(channels), C.byref(bufs), C.byref(st) if stats else None),
               self._h)
        return arrays, st

    def render_aov_device(self, opts, channels, ptrs, stream_ptr=None):
        """rt_render_aov_device: asynchronous, into device buffers; ptrs: {name: raw device pointer} (e.g. torch
        tensor.data_ptr()) for the channels' names depth, normal, albedo, coverage, object."""
        bufs = rt_aov_buffers()
        for name, ptr in ptrs.items():
            if name not in [v[0] for v in AOV_CHANNELS.values()]:
                raise TypeError(f"unknown AOV channel {name}")
            setattr(bufs, name, ptr or None)
        _check(lib.rt_render_aov_device(self._h, C.byref(opts), int(channels), C.byref(bufs), C.c_void_p(stream_ptr or 0)),
               self._h)

    def query_nearest(self, rays, channels=RT_HIT_ALL, out=None, stats=True, flags=0):
        """rt_query_nearest: Scene::intersect for caller-supplied rays (synchronous) -> ({name: array}, stats).
        rays: anything np.ascontiguousarray(.., float64) turns into [n, 6] (origin, direction; not normalised).
        Arrays: t float64 [n] (+inf: miss), object int32 [n] (-1: miss), normal float64 [n, 3] (the shape's, not
        oriented); only the selected channels.  out: {name: array} to write into instead (a selected channel
        missing from it is passed as NULL: the call is refused)."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = r.shape[0]
        arrays, bufs = {}, rt_hit_buffers()
        for bit, (name, k, dt) in HIT_CHANNELS.items():
            if out is not None:
                a = out.get(name)
                if a is not None:
                    assert a.dtype == dt and a.size >= n * k and a.flags.c_contiguous
            elif channels & bit:
                a = np.zeros((n, k) if k > 1 else (n,), dt)
            else:
                a = None
            if a is not None:
                arrays[name] = a
                setattr(bufs, name, a.ctypes.data)
        st = rt_stats() if stats else None
        _check(lib.rt_query_nearest(self._h, r.ctypes.data, n, int(channels), C.byref(bufs), int(flags),
                                    C.byref(st) if stats else None), self._h)
        return arrays, st

    def query_occluded(self, rays, r2=None, out=None, stats=True, flags=0):
        """rt_query_occluded: the shadow test of raytrace.rs:43-50 for caller-supplied rays (synchronous) ->
        (uint8 [n], stats).  r2: None (any hit occludes: the directional light's rule) or the squared ranges [n]
        (occluded when t * t < r2: the point light's).  out: a uint8 array to write into instead."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = r.shape[0]
        rr = None
        if r2 is not None:
            rr = np.ascontiguousarray(r2, dtype=np.float64).reshape(-1)
            assert rr.shape == (n,)
        occ = np.zeros(n, np.uint8) if out is None else out
        assert occ.dtype == np.uint8 and occ.size >= n and occ.flags.c_contiguous
        st = rt_stats() if stats else None
        _check(lib.rt_query_occluded(self._h, r.ctypes.data, rr.ctypes.data if rr is not None else None, n,
                                     occ.ctypes.data, int(flags), C.byref(st) if stats else None), self._h)
        return occ, st

    def query_nearest_device(self, d_rays_ptr, n, channels, ptrs, stream_ptr=None, flags=0):
        """rt_query_nearest_device: asynchronous; d_rays_ptr: raw device pointer of [n, 6] float64 rays (16-byte
        aligned), ptrs: {name: raw device pointer} for the channels' names t, object, normal."""
        bufs = rt_hit_buffers()
        for name, ptr in ptrs.items():
            if name not in [v[0] for v in HIT_CHANNELS.values()]:
                raise TypeError(f"unknown hit channel {name}")
            setattr(bufs, name, ptr or None)
        _check(lib.rt_query_nearest_device(self._h, C.c_void_p(d_rays_ptr or 0), int(n), int(channels), C.byref(bufs),
                                           int(flags), C.c_void_p(stream_ptr or 0)), self._h)

    def query_occluded_device(self, d_rays_ptr, d_r2_ptr, n, d_occluded_ptr, stream_ptr=None, flags=0):
        """rt_query_occluded_device: asynchronous; raw device pointers (d_r2_ptr None / 0: no range)."""
        _check(lib.rt_query_occluded_device(self._h, C.c_void_p(d_rays_ptr or 0), C.c_void_p(d_r2_ptr or 0), int(n),
                                            C.c_void_p(d_occluded_ptr or 0), int(flags), C.c_void_p(stream_ptr or 0)),
               self._h)

    def denoise(self, rgb, guides=None, rgb_out=True, bgr_out=True, **params):
        """rt_denoise: the edge-avoiding a-trous filter on host arrays (synchronous) -> (rgb float32 [h, w, 3] or None,
        bgr uint8 [h, pitch] or None).  rgb: float32 [h, w, 3]; guides: {"normal": [h, w, 3], "depth": [h, w],
        "albedo": [h, w, 3]} float32, those the flags select; params: denoise_params' keywords."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w = rgb.shape[:2]
        p = denoise_params(w, h, **params)
        keep = [rgb]
        ins = rt_denoise_inputs(rgb=rgb.ctypes.data)
        for name, a in (guides or {}).items():
            if name not in ("normal", "depth", "albedo"):
                raise TypeError(f"unknown guide {name}")
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.size == h * w * (1 if name == "depth" else 3), name
            keep.append(a)
            setattr(ins, name, a.ctypes.data)
        pitch = p.bgr_pitch or 3 * w
        out_rgb = np.zeros((h, w, 3), np.float32) if rgb_out else None
        out_bgr = np.full((h, pitch), 0xCD, np.uint8) if bgr_out else None
        _check(lib.rt_denoise(self._h, C.byref(p), C.byref(ins), out_rgb.ctypes.data if rgb_out else None,
                              out_bgr.ctypes.data if bgr_out else None), self._h)
        return out_rgb, out_bgr

    def denoise_device(self, params, d_rgb_ptr, guide_ptrs, d_out_rgb_ptr, d_out_bgr_ptr, stream_ptr=None):
        """rt_denoise_device: asynchronous, on device buffers (raw pointers, e.g. torch tensor.data_ptr()).  params:
        denoise_params(..); guide_ptrs: {"normal" / "depth" / "albedo": pointer}."""
        ins = rt_denoise_inputs(rgb=d_rgb_ptr or None)
        for name, ptr in (guide_ptrs or {}).items():
            if name not in ("normal", "depth", "albedo"):
                raise TypeError(f"unknown guide {name}")
            setattr(ins, name, ptr or None)
        _check(lib.rt_denoise_device(self._h, C.byref(params), C.byref(ins), C.c_void_p(d_out_rgb_ptr or 0),
                                     C.c_void_p(d_out_bgr_ptr or 0), C.c_void_p(stream_ptr or 0)), self._h)

    def denoise_var(self, rgb, variance, guides=None, sigma_variance=2.0, variance_floor=2.0 ** -20, variance_out=False,
                    rgb_out=True, bgr_out=True, **params):
        """rt_denoise_var: the variance-guided filter on host arrays (synchronous) -> (rgb, bgr, variance float32 [h, w]
        or None), rgb and bgr as denoise gives them.  variance: float32 [h, w, 3], the variance of the mean
        (Accumulator.noise); guides and params as for denoise."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w = rgb.shape[:2]
        p = denoise_params(w, h, **params)
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        assert variance.size == h * w * 3, "variance"
        keep = [rgb, variance]
        ins = rt_denoise_inputs(rgb=rgb.ctypes.data)
        for name, a in (guides or {}).items():
            if name not in ("normal", "depth", "albedo"):
                raise TypeError(f"unknown guide {name}")
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.size == h * w * (1 if name == "depth" else 3), name
            keep.append(a)
            setattr(ins, name, a.ctypes.data)
        pitch = p.bgr_pitch or 3 * w
        out_rgb = np.zeros((h, w, 3), np.float32) if rgb_out else None
        out_bgr = np.full((h, pitch), 0xCD, np.uint8) if bgr_out else None
        out_var = np.zeros((h, w), np.float32) if variance_out else None
        var = rt_denoise_variance(variance=variance.ctypes.data, out_variance=out_var.ctypes.data if variance_out else None,
                                  sigma_variance=sigma_variance, variance_floor=variance_floor)
        _check(lib.rt_denoise_var(self._h, C.byref(p), C.byref(ins), C.byref(var), out_rgb.ctypes.data if rgb_out else None,
                                  out_bgr.ctypes.data if bgr_out else None), self._h)
        return out_rgb, out_bgr, out_var

    def denoise_var_device(self, params, d_rgb_ptr, d_variance_ptr, guide_ptrs, d_out_rgb_ptr, d_out_bgr_ptr, d_out_variance_ptr=None,
                           sigma_variance=2.0, variance_floor=2.0 ** -20, stream_ptr=None):
        """rt_denoise_var_device: asynchronous, on device buffers (raw pointers), as denoise_device; d_variance_ptr:
        [h, w, 3] floats (Accumulator.noise_device writes them), d_out_variance_ptr: [h, w] floats or None."""
        ins = rt_denoise_inputs(rgb=d_rgb_ptr or None)
        for name, ptr in (guide_ptrs or {}).items():
            if name not in ("normal", "depth", "albedo"):
                raise TypeError(f"unknown guide {name}")
            setattr(ins, name, ptr or None)
        var = rt_denoise_variance(variance=d_variance_ptr or None, out_variance=d_out_variance_ptr or None,
                                  sigma_variance=sigma_variance, variance_floor=variance_floor)
        _check(lib.rt_denoise_var_device(self._h, C.byref(params), C.byref(ins), C.byref(var), C.c_void_p(d_out_rgb_ptr or 0),
                                         C.c_void_p(d_out_bgr_ptr or 0), C.c_void_p(stream_ptr or 0)), self._h)

    def reserve(self, opts, host=False, stream_ptr=None):
        """rt_ctx_reserve: allocate and warm up everything a render with opts needs (host: rt_render's
        buffers too; stream_ptr: the stream render_device will be called with), so that render runs warm."""
        _check(lib.rt_ctx_reserve(self._h, C.byref(opts), 1 if host else 0, C.c_void_p(stream_ptr or 0)), self._h)

    def stats(self):
        st = rt_stats()
        _check(lib.rt_ctx_stats(self._h, C.byref(st)), self._h)
        return st

    def generation_counts(self, n=34):
        q = (C.c_uint32 * n)()
        s = (C.c_uint32 * n)()
        _check(lib.rt_ctx_generation_counts(self._h, q, s, n), self._h)
        return list(q), list(s)

    def div_a2_check(self, x, a):
        """Diagnostic: (the sphere test's x / (2a) as the device computes it, the
        device's own f64 division) for float64 arrays x, a (rt_div_a2_check)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert x.shape == a.shape and x.ndim == 1
        fast = np.empty_like(x)
        slow = np.empty_like(x)
        P = C.POINTER(C.c_double)
        _check(lib.rt_div_a2_check(self._h, x.ctypes.data_as(P), a.ctypes.data_as(P), x.size, fast.ctypes.data_as(P),
                                   slow.ctypes.data_as(P)), self._h)
        return fast, slow

    def sqrt_check(self, x):
        """Diagnostic: (the sphere test's sqrt as the device computes it, the device's own
        f64 sqrt) for a float64 array x (rt_sqrt_check)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 1
        fast = np.empty_like(x)
        slow = np.empty_like(x)
        P = C.POINTER(C.c_double)
        _check(lib.rt_sqrt_check(self._h, x.ctypes.data_as(P), x.size, fast.ctypes.data_as(P), slow.ctypes.data_as(P)),
               self._h)
        return fast, slow

    def cull_check(self, rays, boxes, t, codes, reach=float("inf")):
        """Diagnostic (rt_cull_check): the tree walks' f32 culling arithmetic on n records: rays [n, 6]
        float64 (origin, direction), boxes [n, 6] float32 (lo, hi), t [n] float64 (+inf: no limit), codes
        [n] int32, reach the culling domain (cull_reach(extent); inf: every origin inside).  Returns a dict
        of [n] arrays: te, tlim, hit, tnear (box_hit), hit_nf, tnear_nf (the whole-LDS walk's near / far
        form), node16, t16, node18, t18 (the compact stack entries of (code, tnear) read back)."""
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        boxes = np.ascontiguousarray(boxes, dtype=np.float32)
        t = np.ascontiguousarray(t, dtype=np.float64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        n = t.size
        assert rays.shape == (n, 6) and boxes.shape == (n, 6) and t.shape == (n,) and codes.shape == (n,)
        oi = np.empty((n, 5), np.int32)
        of = np.empty((n, 5), np.float32)
        PD, PF, PI = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _check(lib.rt_cull_check(self._h, n, rays.ctypes.data_as(PD), boxes.ctypes.data_as(PF), t.ctypes.data_as(PD),
                                 codes.ctypes.data_as(PI), float(reach), oi.ctypes.data_as(PI), of.ctypes.data_as(PF)),
               self._h)
        return {"te": oi[:, 0], "hit": oi[:, 1] != 0, "hit_nf": oi[:, 2] != 0, "node16": oi[:, 3], "node18": oi[:, 4],
                "tlim": of[:, 0], "tnear": of[:, 1], "tnear_nf": of[:, 2], "t16": of[:, 3], "t18": of[:, 4]}

    def isect_check(self, rays, spheres, planes):
        """Diagnostic (rt_isect_check): the exact sphere and plane tests on n records: rays [n, 6] (origin,
        direction), spheres [n, 4] (centre, radius), planes [n, 6] (point, normal), float64.  Returns a dict of
        arrays: hit_bf, t_bf, pt_bf [n, 3], n_bf [n, 3] (the branch-free sphere test), hit_br, t_br, pt_br, n_br
        (the branchy form), hit_pl, t_pl (the plane test; t as computed whatever the verdict)."""
        rec = np.ascontiguousarray(np.concatenate([np.asarray(rays, np.float64), np.asarray(spheres, np.float64),
                                                   np.asarray(planes, np.float64)], axis=1))
        n = rec.shape[0]
        assert rec.shape == (n, 16)
        oi = np.empty((n, 3), np.int32)
        od = np.empty((n, 15), np.float64)
        PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _check(lib.rt_isect_check(self._h, n, rec.ctypes.data_as(PD), oi.ctypes.data_as(PI), od.ctypes.data_as(PD)),
               self._h)
        return {"hit_bf": oi[:, 0] != 0, "hit_br": oi[:, 1] != 0, "hit_pl": oi[:, 2] != 0, "t_bf": od[:, 0],
                "t_br": od[:, 1], "t_pl": od[:, 2], "pt_bf": od[:, 3:6], "n_bf": od[:, 6:9], "pt_br": od[:, 9:12],
                "n_br": od[:, 12:15]}

    def shade_check(self, records, kinds):
        """Diagnostic (rt_shade_check): the shading arithmetic and the device's pow / sin / cos on n records:
        records [n, 27] float64 (point 3, shape normal 3, ray direction 3, kd 3, ks 3, exponent, ior, light v 3,
        light colour 3, significance, pow x, pow y, trig x), kinds [n, 2] int32 (material kind, light kind).
        Returns a dict of arrays: ldir [n, 3], r2, has_range, fresnel, f, diffuse, specular, refl [n, 6] (the
        mirror ray's origin and direction), c, p, col [n, 3], pow, sin, cos."""
        rec = np.ascontiguousarray(records, dtype=np.float64)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        n = rec.shape[0]
        assert rec.shape == (n, 27) and kinds.shape == (n, 2)
        oi = np.empty((n, 3), np.int32)
        od = np.empty((n, 20), np.float64)
        PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _check(lib.rt_shade_check(self._h, n, rec.ctypes.data_as(PD), kinds.ctypes.data_as(PI), oi.ctypes.data_as(PI),
                                  od.ctypes.data_as(PD)), self._h)
        return {"ldir": od[:, 0:3], "r2": od[:, 3], "fresnel": od[:, 4], "f": od[:, 5], "refl": od[:, 6:12],
                "c": od[:, 12], "p": od[:, 13], "col": od[:, 14:17], "pow": od[:, 17], "sin": od[:, 18],
                "cos": od[:, 19], "has_range": oi[:, 0] != 0, "diffuse": oi[:, 1] != 0, "specular": oi[:, 2] != 0}

    def accumulator(self, opts, moments=False):
        """rt_accum_create: a progressive render of opts' tile (main.rs:47-56 split over calls), bound to
        opts' image-defining fields and to the scene uploaded now.  moments: rt_accum_create_moments, an
        accumulator that also keeps every pixel's sums of squares (Accumulator.noise)."""
        return Accumulator(self, opts, moments)

    def kernel_times(self):
        """{family: (summed ms, launches)} over the RT_TIME_KERNELS renders since
        the previous call (then reset); synchronises with the last timed launch."""
        n = len(KERNEL_FAMILIES)
        ms = (C.c_double * n)()
        cnt = (C.c_uint32 * n)()
        _check(lib.rt_ctx_kernel_times(self._h, ms, cnt, n), self._h)
        return {f: (ms[i], cnt[i]) for i, f in enumerate(KERNEL_FAMILIES)}

    def close(self):
        if self._h:
            lib.rt_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accumulator:
    """rt_accum: the f64 running sums of one tile on the device and the number of samples in them.
    add(n) traces samples [samples, samples + n) and adds them in sample order; resolve() gives the
    image of the samples so far (sum / samples), as often as wanted.  Close it before its Context, or
    after (then only close() does anything)."""

    def __init__(self, ctx, opts, moments=False):
        self._ctx = ctx
        h = C.c_void_p()
        create = lib.rt_accum_create_moments if moments else lib.rt_accum_create
        _check(create(ctx._h, C.byref(opts), C.byref(h)), ctx._h)
        self._h = h
        self.tile_w, self.tile_h = opts.tile_w, opts.tile_h

    @property
    def samples(self):
        n = C.c_uint32()
        _check(lib.rt_accum_samples(self._h, C.byref(n)))
        return n.value

    def add(self, n, algo=RT_ALGO_AUTO, flags=0, stream_ptr=None):
        """rt_render_accumulate (asynchronous; Context.stats() gives this call's own statistics)."""
        _check(lib.rt_render_accumulate(self._ctx._h, self._h, int(n), int(algo), int(flags), C.c_void_p(stream_ptr or 0)),
               self._ctx._h)

    def resolve(self, rgb=True, bgr=True, pitch=0):
        """rt_accum_resolve_host -> (rgb float32 [tile_h, tile_w, 3] or None, bgr uint8 [tile_h, pitch] or None)."""
        p = pitch or 3 * self.tile_w
        out_rgb = np.zeros((self.tile_h, self.tile_w, 3), np.float32) if rgb else None
        out_bgr = np.full((self.tile_h, p), 0xCD, np.uint8) if bgr else None
        _check(lib.rt_accum_resolve_host(self._ctx._h, self._h, int(pitch),
                                         out_rgb.ctypes.data_as(C.POINTER(C.c_float)) if rgb else None,
                                         out_bgr.ctypes.data_as(C.POINTER(C.c_uint8)) if bgr else None), self._ctx._h)
        return out_rgb, out_bgr

    def resolve_device(self, d_rgb_ptr, d_bgr_ptr, pitch=0, stream_ptr=None):
        """rt_accum_resolve into device buffers (raw pointers), asynchronous."""
        _check(lib.rt_accum_resolve(self._ctx._h, self._h, int(pitch), C.c_void_p(d_rgb_ptr or 0), C.c_void_p(d_bgr_ptr or 0),
                                    C.c_void_p(stream_ptr or 0)), self._ctx._h)

    def reset(self):
        _check(lib.rt_accum_reset(self._h), self._ctx._h)

    def download(self, cap=None):
        """rt_accum_download -> (sums float64 [tile_h, tile_w, 3], samples); cap: the capacity passed (a test's)."""
        sums = np.zeros((self.tile_h, self.tile_w, 3), np.float64)
        n = C.c_uint32()
        _check(lib.rt_accum_download(self._ctx._h, self._h, sums.ctypes.data_as(C.POINTER(C.c_double)),
                                     sums.size if cap is None else int(cap), C.byref(n)), self._ctx._h)
        return sums, n.value

    def upload(self, sums, samples):
        arr = np.ascontiguousarray(sums, dtype=np.float64)
        _check(lib.rt_accum_upload(self._ctx._h, self._h, arr.ctypes.data_as(C.POINTER(C.c_double)), arr.size, int(samples)),
               self._ctx._h)

    @property
    def has_moments(self):
        f = C.c_int32()
        _check(lib.rt_accum_has_moments(self._h, C.byref(f)))
        return bool(f.value)

    def download_moments(self, cap=None):
        """rt_accum_download_moments -> squares float64 [tile_h, tile_w, 3]; cap: the capacity passed (a test's)."""
        sq = np.zeros((self.tile_h, self.tile_w, 3), np.float64)
        _check(lib.rt_accum_download_moments(self._ctx._h, self._h, sq.ctypes.data_as(C.POINTER(C.c_double)),
                                             sq.size if cap is None else int(cap)), self._ctx._h)
        return sq

    def upload_moments(self, sums, squares, samples):
        s = np.ascontiguousarray(sums, dtype=np.float64)
        q = np.ascontiguousarray(squares, dtype=np.float64)
        if s.size != q.size:
            raise ValueError("sums and squares differ in size")
        PD = C.POINTER(C.c_double)
        _check(lib.rt_accum_upload_moments(self._ctx._h, self._h, s.ctypes.data_as(PD), q.ctypes.data_as(PD), s.size,
                                           int(samples)), self._ctx._h)

    def noise(self, floor, threshold, variance=True, error=True):
        """rt_accum_noise_host -> (variance float32 [tile_h, tile_w, 3] or None, error float32 [tile_h, tile_w]
        or None, above): the variance of the mean, the relative error and the pixels with !(err <= threshold)."""
        var = np.zeros((self.tile_h, self.tile_w, 3), np.float32) if variance else None
        err = np.zeros((self.tile_h, self.tile_w), np.float32) if error else None
        above = C.c_uint64()
        PF = C.POINTER(C.c_float)
        _check(lib.rt_accum_noise_host(self._ctx._h, self._h, float(floor), float(threshold),
                                       var.ctypes.data_as(PF) if variance else None,
                                       err.ctypes.data_as(PF) if error else None, C.byref(above)), self._ctx._h)
        return var, err, above.value

    def noise_device(self, floor, threshold, d_variance_ptr=None, d_error_ptr=None, stream_ptr=None):
        """rt_accum_noise into device buffers (raw pointers, either may be None) -> above."""
        above = C.c_uint64()
        _check(lib.rt_accum_noise(self._ctx._h, self._h, float(floor), float(threshold), C.c_void_p(d_variance_ptr or 0),
                                  C.c_void_p(d_error_ptr or 0), C.byref(above), C.c_void_p(stream_ptr or 0)), self._ctx._h)
        return above.value

    def close(self):
        if self._h:
            lib.rt_accum_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def checkpoint_write(path, opts, scene_hash, samples, sums):
    """rt_checkpoint_write (host only): the bound fields of opts, scene_hash, samples and the sums to `path`."""
    arr = np.ascontiguousarray(sums, dtype=np.float64)
    _check(lib.rt_checkpoint_write(os.fsencode(path), C.byref(opts), int(scene_hash), int(samples),
                                   arr.ctypes.data_as(C.POINTER(C.c_double)), arr.size))


def checkpoint_read(path, header_only=False):
    """rt_checkpoint_read -> (opts, scene_hash, samples, sums float64 [tile_h, tile_w, 3] or None)."""
    o = rt_render_opts()
    h, n = C.c_uint64(), C.c_uint32()
    _check(lib.rt_checkpoint_read(os.fsencode(path), C.byref(o), C.byref(h), C.byref(n), None, 0))
    if header_only:
        return o, h.value, n.value, None
    sums = np.zeros((o.tile_h, o.tile_w, 3), np.float64)
    _check(lib.rt_checkpoint_read(os.fsencode(path), C.byref(o), C.byref(h), C.byref(n),
                                  sums.ctypes.data_as(C.POINTER(C.c_double)), sums.size))
    return o, h.value, n.value, sums


def checkpoint_write_moments(path, opts, scene_hash, samples, sums, squares):
    """rt_checkpoint_write_moments (host only): a format version 2 file, the sums and then the squares."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    q = np.ascontiguousarray(squares, dtype=np.float64)
    if s.size != q.size:
        raise ValueError("sums and squares differ in size")
    PD = C.POINTER(C.c_double)
    _check(lib.rt_checkpoint_write_moments(os.fsencode(path), C.byref(opts), int(scene_hash), int(samples),
                                           s.ctypes.data_as(PD), q.ctypes.data_as(PD), s.size))


def checkpoint_read_moments(path, header_only=False):
    """rt_checkpoint_read_moments -> (opts, scene_hash, samples, sums, squares), float64 [tile_h, tile_w, 3] or None."""
    o = rt_render_opts()
    h, n = C.c_uint64(), C.c_uint32()
    _check(lib.rt_checkpoint_read_moments(os.fsencode(path), C.byref(o), C.byref(h), C.byref(n), None, None, 0))
    if header_only:
        return o, h.value, n.value, None, None
    sums = np.zeros((o.tile_h, o.tile_w, 3), np.float64)
    sq = np.zeros((o.tile_h, o.tile_w, 3), np.float64)
    PD = C.POINTER(C.c_double)
    _check(lib.rt_checkpoint_read_moments(os.fsencode(path), C.byref(o), C.byref(h), C.byref(n), sums.ctypes.data_as(PD),
                                          sq.ctypes.data_as(PD), sums.size))
    return o, h.value, n.value, sums, sq


def scene_hash(text):
    """FNV-1a 64 of the scene text: what the CLI's --checkpoint binds a checkpoint to."""
    h = 0xcbf29ce484222325
    for b in (text.encode() if isinstance(text, str) else bytes(text)):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def header_functions():
    """Names of every function include/raytrace_amd.h declares (for the export test)."""
    import re
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\**\s*(rt_[a-z_0-9]+)\s*\(", text, flags=re.M)))
