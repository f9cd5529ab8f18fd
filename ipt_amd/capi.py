"""ctypes binding of include/ipt_capi.h (libipt_hip.so).

This is the Python-side view of the drop-in boundary: the same entry points a
cgo / JNI / ctypes caller of the reference would bind.
Only plain pointers cross it. The library has no CPU fallback: every rendering
call needs a gfx950 device and fails loudly (IptError) otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libipt_hip.so"

IPT_OK = 0
IPT_E_INVALID = -1
IPT_DDF_COSINE, IPT_DDF_LIGHT, IPT_DDF_MIXTURE, IPT_DDF_COSINE_TABLE = 0, 1, 2, 3
IPT_E_DEVICE = -2
IPT_E_UNSUPPORTED = -3
IPT_E_NOSCENE = -4
IPT_E_OOM = -5

IPT_GEOM_SPHERE_IN_BOX = 0
IPT_GEOM_SPHERES_IN_BOX = 1
IPT_GEOM_FLOOR = 2
IPT_GEOM_CORNER = 3
IPT_GEOM_SPHERES = 4
IPT_GEOM_SMALLPT = 5
IPT_LIGHT_AREA_DIAMOND = 0
IPT_LIGHT_AREA_TRIANGLE = 1
IPT_LIGHT_SPHERE, IPT_LIGHT_POINT, IPT_LIGHT_OUTER_SPHERE = 2, 3, 4
IPT_FLAG_COUNTERS = 1
IPT_FLAG_GUI_PLANE = 2  # Gui::addRay's row map instead of GridRenderPlane::addRay's (ABI 7)
IPT_FLAG_PREVIEW = 4  # ray_power_preview instead of ray_power_recursive (ABI 7 addition)
IPT_FLAG_COMPACT = 8  # the path kernel's pool holds the traced samples alone (ABI 7 addition)
IPT_REPLAY_MAX_SAMPLES = 1 << 24  # ipt_replay_samples: spp * width * height per call (ABI 7 addition)

F3 = C.c_float * 3


class AreaLight(C.Structure):
    _fields_ = [("position", F3), ("x_axis", F3), ("y_axis", F3), ("power", C.c_float),
                ("type", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("position", F3), ("direction", F3), ("right", F3), ("up", F3)]


class Sphere(C.Structure):
    _fields_ = [("center", F3), ("radius", C.c_float)]


class Scene(C.Structure):
    _fields_ = [("geometry_kind", C.c_int32), ("n_lights", C.c_int32),
                ("lights", C.POINTER(AreaLight)), ("n_spheres", C.c_int32),
                ("spheres", C.POINTER(Sphere)), ("camera", Camera)]


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
                ("spp_offset", C.c_int32), ("n_rays", C.c_int32), ("depth_max", C.c_int32),
                ("seed", C.c_uint64), ("tile_rows", C.c_int32), ("n_shards", C.c_int32),
                ("shard_id", C.c_int32), ("flags", C.c_uint32)]


class Image(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("counters", C.c_void_p), ("sums", C.c_void_p),
                ("pixel_max", C.c_void_p)]


class DisplayParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("glare_cutoff", C.c_float),
                ("flags", C.c_uint32)]


class DisplayStatsParams(C.Structure):  # ABI 7 additions
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("glare_cutoff", C.c_float),
                ("hist_buckets", C.c_int32), ("white_rank", C.c_int64), ("flags", C.c_uint32)]


class PgmParams(C.Structure):  # ABI 7 additions
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("smooth_side", C.c_int32), ("max_side", C.c_int32),
                ("contrast", C.c_float), ("gamma", C.c_float), ("max_value", C.c_float), ("flags", C.c_uint32)]


class AdaptParams(C.Structure):  # ABI 7 additions (adaptive sampling)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("min_count", C.c_uint32),
                ("rel_tol", C.c_float), ("abs_tol", C.c_float), ("flags", C.c_uint32)]


class Guide(C.Structure):  # ABI 7 additions (denoising): ipt_guide, 32 B
    _fields_ = [("pos", F3), ("kind", C.c_uint32), ("normal", F3), ("zero", C.c_uint32)]


# ipt_guide as a numpy record, one per destination pixel
GuideRecord = np.dtype([("pos", np.float32, 3), ("kind", np.uint32), ("normal", np.float32, 3),
                        ("zero", np.uint32)])


class DenoiseParams(C.Structure):  # ABI 7 additions (denoising)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("sigma_l", C.c_float),
                ("normal_pow", C.c_int32), ("sigma_z", C.c_float)]


# the filter's defaults (DESIGN.md "Denoising"): 5 iterations, colour within 4
# standard errors, normals to the 2^5 = 32nd power, planes within 0.1 units
DENOISE_DEFAULTS = dict(iterations=5, sigma_l=4.0, normal_pow=5, sigma_z=0.1)


class ReprojectParams(C.Structure):  # ABI 7 additions (temporal reprojection)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_uint32), ("prev_camera", Camera),
                ("sigma_z", C.c_float), ("normal_min", C.c_float), ("max_count", C.c_uint32)]


# the reprojection's defaults (DESIGN.md "Temporal reprojection"): the denoiser's
# plane distance, normals within about 26 degrees, a history of at most 64 samples
REPROJECT_DEFAULTS = dict(sigma_z=0.1, normal_min=0.9, max_count=64)


ABI_VERSION = 7  # include/ipt_capi.h IPT_ABI_VERSION
ABI_LAYOUT_COMPATIBLE = (3, 4, 5, 6, 7)  # versions with this binding's struct layouts (IPT_ABI_COMPAT only)

COUNTER_NAMES = ("paths", "traced_rays", "surface_hits", "light_hits", "expanded_nodes",
                 "iterations", "light_samples", "skipped", "sphere_frames", "light_traces",
                 "drifted", "bvh_nodes", "sphere_tests", "light_nodes", "light_tests")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


EXPORTED_SYMBOLS = (
    "ipt_abi_version", "ipt_last_error", "ipt_create", "ipt_destroy", "ipt_upload_scene",
    "ipt_render", "ipt_render_device", "ipt_render_device_async", "ipt_render_wait", "ipt_render_values",
    "ipt_get_counters",
    "ipt_reset_counters", "ipt_last_kernel_ms", "ipt_math_host", "ipt_math_device",
    "ipt_shard_plan", "ipt_get_profile", "ipt_math_selfcheck", "ipt_smooth", "ipt_glare", "ipt_ddf_sample", "ipt_ddf_value",
    "ipt_philox", "ipt_transfer_bytes",
    "ipt_display_device", "ipt_display", "ipt_powf_host", "ipt_powf_device",
    "ipt_display_stats_device", "ipt_display_stats",
    "ipt_smooth_device", "ipt_pgm_device", "ipt_pgm", "ipt_logf_host", "ipt_logf_device",
    "ipt_preview_values", "ipt_replay_samples",
    "ipt_render_masked_device_async", "ipt_render_masked_device", "ipt_adapt_device", "ipt_render_adaptive",
    "ipt_last_units", "ipt_compact_plan", "ipt_last_instance",
    "ipt_guides_device", "ipt_guides", "ipt_denoise_device", "ipt_denoise", "ipt_denoise_pass_ms",
    "ipt_reproject_device", "ipt_reproject",
)

# path-kernel phases of the IPT_PROF profile (ipt_kernels.hip IPT_PHASE ids)
PROFILE_PHASES = ("step", "pop", "new_path", "iteration", "philox", "frame_worker",
                  "walk_cell", "light_sample", "trace", "geometry", "push", "wg_step")
# step segments of the IPT_STAMP diagnostic build (IPT_STAMP_AT ids)
STAMP_SEGMENTS = ("loop_top", "refill", "pop_early", "pre_prologue", "prologue_philox_frame", "exit_test",
                  "pop", "frame_prefetch", "new_path_direction", "lights", "mixture_geometry", "resolve_push")

_lib = None


class IptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ipt error {code}: {msg}")
        self.code = code


def load(path: str | os.PathLike | None = None):
    """Load libipt_hip.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("IPT_LIB_PATH", LIB_PATH))
    if not p.exists():
        raise IptError(IPT_E_DEVICE, f"{p} is not built; run __graft_entry__.build()")
    lib = C.CDLL(str(p))
    lib.ipt_abi_version.restype = C.c_int
    # (IPT_ABI_COMPAT=1: A/B tooling loading an older variant library; only
    # the versions whose struct layouts this binding shares are accepted -- ABI
    # 4 added entry points to 3 without touching a layout -- and the entry
    # points an older library lacks are then unavailable)
    v = lib.ipt_abi_version()
    if v != ABI_VERSION:
        if not (os.environ.get("IPT_ABI_COMPAT") and v in ABI_LAYOUT_COMPATIBLE):
            raise IptError(IPT_E_INVALID, f"{p}: ABI {v} != {ABI_VERSION}; rebuild")
        import warnings
        warnings.warn(f"{p}: loading ABI {v} under IPT_ABI_COMPAT (binding is ABI {ABI_VERSION})")
    lib.ipt_last_error.restype = C.c_char_p
    lib.ipt_last_error.argtypes = [C.c_void_p]
    lib.ipt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.ipt_destroy.argtypes = [C.c_void_p]
    lib.ipt_destroy.restype = None
    lib.ipt_upload_scene.argtypes = [C.c_void_p, C.POINTER(Scene)]
    lib.ipt_render.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Image)]
    lib.ipt_render_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Image), C.c_void_p]
    if hasattr(lib, "ipt_render_device_async"):
        lib.ipt_render_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Image), C.c_void_p]
        lib.ipt_render_wait.argtypes = [C.c_void_p]
    if hasattr(lib, "ipt_transfer_bytes"):
        lib.ipt_transfer_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ipt_render_values.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p]
    lib.ipt_get_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
    lib.ipt_reset_counters.argtypes = [C.c_void_p]
    lib.ipt_math_selfcheck.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64,
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.ipt_ddf_sample.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.ipt_ddf_value.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.ipt_smooth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.POINTER(C.c_float)]
    lib.ipt_glare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    lib.ipt_get_profile.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    lib.ipt_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.ipt_math_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    lib.ipt_math_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    lib.ipt_shard_plan.argtypes = [C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.ipt_philox.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int64]
    if hasattr(lib, "ipt_display_device"):  # ABI 6
        lib.ipt_display_device.argtypes = [C.c_void_p, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ipt_display.argtypes = [C.c_void_p, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
        lib.ipt_powf_host.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_int64]
        lib.ipt_powf_device.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64]
    if hasattr(lib, "ipt_display_stats_device"):  # ABI 7 additions
        lib.ipt_display_stats_device.argtypes = [C.c_void_p, C.POINTER(DisplayStatsParams)] + [C.c_void_p] * 7
        lib.ipt_display_stats.argtypes = [C.c_void_p, C.POINTER(DisplayStatsParams)] + [C.c_void_p] * 6
    if hasattr(lib, "ipt_pgm_device"):  # ABI 7 additions
        lib.ipt_smooth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p]
        lib.ipt_pgm_device.argtypes = [C.c_void_p, C.POINTER(PgmParams)] + [C.c_void_p] * 6
        lib.ipt_pgm.argtypes = [C.c_void_p, C.POINTER(PgmParams)] + [C.c_void_p] * 5
        lib.ipt_logf_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.ipt_logf_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    if hasattr(lib, "ipt_preview_values"):  # ABI 7 addition
        lib.ipt_preview_values.argtypes = [C.c_void_p, C.POINTER(Params)] + [C.c_void_p] * 4
    if hasattr(lib, "ipt_replay_samples"):  # ABI 7 addition
        lib.ipt_replay_samples.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Image),
                                           C.c_void_p]
    if hasattr(lib, "ipt_adapt_device"):  # ABI 7 additions (adaptive sampling)
        lib.ipt_render_masked_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Image), C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
        lib.ipt_render_masked_device.argtypes = lib.ipt_render_masked_device_async.argtypes
        lib.ipt_adapt_device.argtypes = [C.c_void_p, C.POINTER(AdaptParams)] + [C.c_void_p] * 6
        lib.ipt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AdaptParams), C.c_int32,
                                            C.POINTER(Image), C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "ipt_last_units"):  # ABI 7 additions (unit compaction)
        lib.ipt_last_units.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ipt_compact_plan.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(lib, "ipt_last_instance"):  # ABI 7 addition (instance probe)
        lib.ipt_last_instance.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    if hasattr(lib, "ipt_denoise_device"):  # ABI 7 additions (denoising)
        lib.ipt_guides_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p]
        lib.ipt_guides.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p]
        lib.ipt_denoise_device.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)] + [C.c_void_p] * 7
        lib.ipt_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)] + [C.c_void_p] * 6
        lib.ipt_denoise_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    if hasattr(lib, "ipt_reproject_device"):  # ABI 7 additions (temporal reprojection)
        lib.ipt_reproject_device.argtypes = [C.c_void_p, C.POINTER(ReprojectParams)] + [C.c_void_p] * 10
        lib.ipt_reproject.argtypes = [C.c_void_p, C.POINTER(ReprojectParams)] + [C.c_void_p] * 9
    if path is None:
        _lib = lib
    return lib


def _check(lib, ctx, rc):
    if rc != IPT_OK:
        raise IptError(rc, lib.ipt_last_error(ctx).decode(errors="replace"))


def make_scene(desc: dict) -> tuple[Scene, list]:
    """Build an ipt_scene from the dict produced by ipt_amd.scenes; returns the
    struct and the Python objects that keep its arrays alive."""
    lights = desc.get("lights", [])
    la = (AreaLight * max(len(lights), 1))()
    for i, L in enumerate(lights):
        la[i].position[:] = L["position"]
        la[i].x_axis[:] = L["x_axis"]
        la[i].y_axis[:] = L["y_axis"]
        la[i].power = L["power"]
        la[i].type = L.get("type", IPT_LIGHT_AREA_DIAMOND)
    spheres = desc.get("spheres", [])
    sa = (Sphere * max(len(spheres), 1))()
    for i, (c, r) in enumerate(spheres):
        sa[i].center[:] = c
        sa[i].radius = r
    cam = desc["camera"]
    s = Scene()
    s.geometry_kind = desc["geometry_kind"]
    s.n_lights = len(lights)
    s.lights = C.cast(la, C.POINTER(AreaLight))
    s.n_spheres = len(spheres)
    s.spheres = C.cast(sa, C.POINTER(Sphere))
    s.camera.position[:] = cam["position"]
    s.camera.direction[:] = cam["direction"]
    s.camera.right[:] = cam["right"]
    s.camera.up[:] = cam["up"]
    return s, [la, sa]


def make_params(width, height, spp, spp_offset=0, n_rays=16, depth_max=8, seed=20241223,
                tile_rows=0, n_shards=1, shard_id=0, flags=0) -> Params:
    p = Params()
    p.width, p.height, p.spp, p.spp_offset = width, height, spp, spp_offset
    p.n_rays, p.depth_max, p.seed = n_rays, depth_max, seed
    p.tile_rows, p.n_shards, p.shard_id, p.flags = tile_rows, n_shards, shard_id, flags
    return p


def make_display_params(width, height, glare_cutoff=0.0, flags=0) -> DisplayParams:
    p = DisplayParams()
    p.width, p.height, p.glare_cutoff, p.flags = width, height, glare_cutoff, flags
    return p


def make_display_stats_params(width, height, glare_cutoff=0.0, hist_buckets=0, white_rank=-1,
                              flags=0) -> DisplayStatsParams:
    p = DisplayStatsParams()
    p.width, p.height, p.glare_cutoff, p.flags = width, height, glare_cutoff, flags
    p.hist_buckets, p.white_rank = hist_buckets, white_rank
    return p


def make_pgm_params(width, height, smooth_side=0, max_side=0, contrast=500.0, gamma=0.6, max_value=0.0,
                    flags=0) -> PgmParams:
    """main.cpp's written output: smooth_side 2, max_side 5, contrast 500, gamma 0.6f."""
    p = PgmParams()
    p.width, p.height, p.smooth_side, p.max_side = width, height, smooth_side, max_side
    p.contrast, p.gamma, p.max_value, p.flags = contrast, gamma, max_value, flags
    return p


def make_adapt_params(width, height, min_count=8, rel_tol=0.05, abs_tol=1e-3, flags=0) -> AdaptParams:
    """ipt_adapt_device's parameters; flags: 0 or IPT_FLAG_GUI_PLANE (the plane's row map)."""
    p = AdaptParams()
    p.width, p.height, p.min_count, p.flags = width, height, min_count, flags
    p.rel_tol, p.abs_tol = rel_tol, abs_tol
    return p


def make_denoise_params(width, height, iterations=DENOISE_DEFAULTS["iterations"],
                        sigma_l=DENOISE_DEFAULTS["sigma_l"], normal_pow=DENOISE_DEFAULTS["normal_pow"],
                        sigma_z=DENOISE_DEFAULTS["sigma_z"]) -> DenoiseParams:
    """ipt_denoise_device's parameters: iteration k taps at step 1 << k."""
    p = DenoiseParams()
    p.width, p.height, p.iterations, p.normal_pow = width, height, iterations, normal_pow
    p.sigma_l, p.sigma_z = sigma_l, sigma_z
    return p


def make_reproject_params(width, height, prev_camera, flags=0, sigma_z=REPROJECT_DEFAULTS["sigma_z"],
                          normal_min=REPROJECT_DEFAULTS["normal_min"],
                          max_count=REPROJECT_DEFAULTS["max_count"]) -> ReprojectParams:
    """ipt_reproject_device's parameters; prev_camera: a scene description's
    camera dict (position, direction, right, up), the one the previous planes
    and guides were taken with; flags: 0 or IPT_FLAG_GUI_PLANE (both frames')."""
    p = ReprojectParams()
    p.width, p.height, p.flags, p.max_count = width, height, flags, max_count
    p.sigma_z, p.normal_min = sigma_z, normal_min
    for k in ("position", "direction", "right", "up"):
        getattr(p.prev_camera, k)[:] = prev_camera[k]
    return p


def white_rank_for(width, height, fraction) -> int:
    """The reference's rank expression (gui.cpp:13): (ulong)(int(w*h) * fraction), in double."""
    return int(float(int(width) * int(height)) * float(fraction))


class Context:
    """One ipt_ctx on one HIP device."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.ipt_create(device, C.byref(h))
        if rc != IPT_OK:
            raise IptError(rc, self.lib.ipt_last_error(None).decode(errors="replace"))
        self.h = h
        self._keep = None

    def close(self):
        if self.h:
            self.lib.ipt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, desc: dict):
        s, keep = make_scene(desc)
        _check(self.lib, self.h, self.lib.ipt_upload_scene(self.h, C.byref(s)))
        self._keep = keep

    def render_values(self, p: Params):
        n = p.spp * p.width * p.height
        vals = np.zeros(n, np.float32)
        codes = np.zeros(n, np.uint8)
        _check(self.lib, self.h, self.lib.ipt_render_values(
            self.h, C.byref(p), vals.ctypes.data, codes.ctypes.data))
        shape = (p.spp, p.height, p.width)
        return vals.reshape(shape), codes.reshape(shape)

    def preview_values(self, p: Params, kinds: bool = True, hits: bool = True):
        """The preview estimator's samples (ipt_preview_values): (values, codes,
        kinds or None, hits or None), shaped [spp][H][W] and [spp][H][W][6]."""
        n = p.spp * p.width * p.height
        vals = np.zeros(n, np.float32)
        codes = np.zeros(n, np.uint8)
        kd = np.zeros(n, np.uint8) if kinds else None
        ht = np.zeros(6 * n, np.float32) if hits else None
        _check(self.lib, self.h, self.lib.ipt_preview_values(
            self.h, C.byref(p), vals.ctypes.data, codes.ctypes.data,
            kd.ctypes.data if kinds else None, ht.ctypes.data if hits else None))
        shape = (p.spp, p.height, p.width)
        return (vals.reshape(shape), codes.reshape(shape), kd.reshape(shape) if kinds else None,
                ht.reshape(shape + (6,)) if hits else None)

    def render(self, p: Params, img: dict):
        """Host-buffer render into img = {pixels, counters, sums?, pixel_max?} (numpy)."""
        im = Image()
        im.pixels = img["pixels"].ctypes.data
        im.counters = img["counters"].ctypes.data
        im.sums = img["sums"].ctypes.data if img.get("sums") is not None else None
        im.pixel_max = img["pixel_max"].ctypes.data if img.get("pixel_max") is not None else None
        _check(self.lib, self.h, self.lib.ipt_render(self.h, C.byref(p), C.byref(im)))

    def transfer_bytes(self) -> tuple[int, int]:
        """(host -> device, device -> host) bytes of the last render() call."""
        h2d, d2h = C.c_uint64(), C.c_uint64()
        _check(self.lib, self.h, self.lib.ipt_transfer_bytes(self.h, C.byref(h2d), C.byref(d2h)))
        return int(h2d.value), int(d2h.value)

    def render_device(self, p: Params, pixels_ptr, counters_ptr, sums_ptr=None, max_ptr=None,
                      stream=None):
        im = Image()
        im.pixels, im.counters, im.sums, im.pixel_max = pixels_ptr, counters_ptr, sums_ptr, max_ptr
        _check(self.lib, self.h, self.lib.ipt_render_device(self.h, C.byref(p), C.byref(im), stream))

    def render_device_async(self, p: Params, pixels_ptr, counters_ptr, sums_ptr=None, max_ptr=None,
                            stream=None):
        """Queue the render (ipt_render_device_async); complete on `stream`'s
        order or after wait()."""
        im = Image()
        im.pixels, im.counters, im.sums, im.pixel_max = pixels_ptr, counters_ptr, sums_ptr, max_ptr
        _check(self.lib, self.h, self.lib.ipt_render_device_async(self.h, C.byref(p), C.byref(im), stream))

    def replay_samples(self, p: Params, values, codes, pixels_ptr, counters_ptr, sums_ptr=None, max_ptr=None,
                       stream=None):
        """The render plane's replay of the caller's samples (ipt_replay_samples):
        values float32 and codes uint8, [spp][H][W] as render_values returns
        them, into a device image. Synchronous. None for values or codes is
        passed on as NULL; the library checks everything else."""
        v = None if values is None else np.ascontiguousarray(values, np.float32)
        c = None if codes is None else np.ascontiguousarray(codes, np.uint8)
        for a in (v, c):
            if a is not None and a.size < p.spp * p.width * p.height:
                raise ValueError("fewer samples than spp * width * height")
        im = Image()
        im.pixels, im.counters, im.sums, im.pixel_max = pixels_ptr, counters_ptr, sums_ptr, max_ptr
        _check(self.lib, self.h, self.lib.ipt_replay_samples(
            self.h, C.byref(p), None if v is None else v.ctypes.data, None if c is None else c.ctypes.data,
            C.byref(im), stream))

    def render_masked_device(self, p: Params, pixels_ptr, counters_ptr, sums_ptr=None, max_ptr=None,
                             mask_ptr=None, m2_ptr=None, stream=None):
        """ipt_render_masked_device: render_device with a per-pixel sample mask
        (uint8 [H][W] by nominal destination, None = all active) and a
        second-moment plane (float32 [H][W], None = not kept)."""
        im = Image()
        im.pixels, im.counters, im.sums, im.pixel_max = pixels_ptr, counters_ptr, sums_ptr, max_ptr
        _check(self.lib, self.h, self.lib.ipt_render_masked_device(self.h, C.byref(p), C.byref(im), mask_ptr, m2_ptr,
                                                                   stream))

    def render_masked_device_async(self, p: Params, pixels_ptr, counters_ptr, sums_ptr=None, max_ptr=None,
                                   mask_ptr=None, m2_ptr=None, stream=None):
        """Queue the masked render (ipt_render_masked_device_async); complete on
        `stream`'s order or after wait()."""
        im = Image()
        im.pixels, im.counters, im.sums, im.pixel_max = pixels_ptr, counters_ptr, sums_ptr, max_ptr
        _check(self.lib, self.h, self.lib.ipt_render_masked_device_async(self.h, C.byref(p), C.byref(im), mask_ptr,
                                                                         m2_ptr, stream))

    def adapt_device(self, ap: AdaptParams, pixels_ptr, counters_ptr, m2_ptr, mask_ptr, stats_ptr=None, stream=None):
        """Queue ipt_adapt_device: the next mask (uint8 at mask_ptr) from the
        plane, and {active, starved, nan, 0} (uint32) at stats_ptr."""
        _check(self.lib, self.h, self.lib.ipt_adapt_device(self.h, C.byref(ap), pixels_ptr, counters_ptr, m2_ptr,
                                                           mask_ptr, stats_ptr, stream))

    def render_adaptive(self, p: Params, ap: AdaptParams, round_spp: int, img: dict, m2=None, mask=None):
        """The adaptive loop on host buffers (ipt_render_adaptive): up to p.spp
        passes in rounds of round_spp into img = {pixels, counters, sums?,
        pixel_max?}; m2 (float32) and mask (uint8) numpy arrays or None.
        Returns {active, starved, nan, passes}."""
        im = Image()
        im.pixels = img["pixels"].ctypes.data
        im.counters = img["counters"].ctypes.data
        im.sums = img["sums"].ctypes.data if img.get("sums") is not None else None
        im.pixel_max = img["pixel_max"].ctypes.data if img.get("pixel_max") is not None else None
        st = np.zeros(4, np.uint32)
        _check(self.lib, self.h, self.lib.ipt_render_adaptive(
            self.h, C.byref(p), C.byref(ap), round_spp, C.byref(im), None if m2 is None else m2.ctypes.data,
            None if mask is None else mask.ctypes.data, st.ctypes.data))
        return {"active": int(st[0]), "starved": int(st[1]), "nan": int(st[2]), "passes": int(st[3])}

    def guides_device(self, p: Params, guides_ptr, stream=None):
        """Queue ipt_guides_device: the first hit of pass p.spp_offset's preview
        sample per destination pixel (GuideRecord [H][W] at guides_ptr);
        p.spp must be 1. Complete on `stream`'s order or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_guides_device(self.h, C.byref(p), guides_ptr, stream))

    def guides(self, p: Params) -> np.ndarray:
        """Host-buffer guide plane (ipt_guides): GuideRecord [H][W]."""
        g = np.zeros((p.height, p.width), GuideRecord)
        _check(self.lib, self.h, self.lib.ipt_guides(self.h, C.byref(p), g.ctypes.data))
        return g

    def denoise_device(self, dp: DenoiseParams, pixels_ptr, counters_ptr, m2_ptr, guides_ptr, out_ptr,
                       var_out_ptr=None, stream=None):
        """Queue ipt_denoise_device: the guided a-trous filter of the plane into
        out_ptr (float32 [H][W]) and, optionally, the filtered variance of the
        mean into var_out_ptr. Complete on `stream`'s order or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_denoise_device(self.h, C.byref(dp), pixels_ptr, counters_ptr, m2_ptr,
                                                             guides_ptr, out_ptr, var_out_ptr, stream))

    def denoise_pass_ms(self):
        """[prepare, iteration 0, ...] kernel ms of the last denoise_device call
        made under IPT_DENOISE_PROFILE=1 (ipt_denoise_pass_ms)."""
        ms = (C.c_float * 7)()
        _check(self.lib, self.h, self.lib.ipt_denoise_pass_ms(self.h, ms))
        return [float(x) for x in ms]

    def denoise(self, dp: DenoiseParams, pixels, counters, m2, guides, var: bool = True):
        """Host-buffer filter (ipt_denoise): (out, var_out or None), float32
        [H*W]; guides a GuideRecord array."""
        px = np.ascontiguousarray(pixels, np.float32).reshape(-1)
        cn = np.ascontiguousarray(counters, np.uint32).reshape(-1)
        mm = np.ascontiguousarray(m2, np.float32).reshape(-1)
        gd = np.ascontiguousarray(guides, GuideRecord).reshape(-1)
        n = dp.width * dp.height
        for a in (px, cn, mm, gd):
            if a.size < n:
                raise ValueError("a buffer holds fewer than width * height elements")
        out = np.empty(max(n, 0), np.float32)
        vo = np.empty(max(n, 0), np.float32) if var else None
        _check(self.lib, self.h, self.lib.ipt_denoise(self.h, C.byref(dp), px.ctypes.data, cn.ctypes.data,
                                                      mm.ctypes.data, gd.ctypes.data, out.ctypes.data,
                                                      vo.ctypes.data if var else None))
        return out, vo

    def reproject_device(self, rp: ReprojectParams, prev_pixels_ptr, prev_counters_ptr, prev_m2_ptr, prev_guides_ptr,
                         cur_guides_ptr, out_pixels_ptr, out_counters_ptr, out_m2_ptr, stats_ptr=None, stream=None):
        """Queue ipt_reproject_device: the previous camera's planes resampled
        to the new frame (float32, uint32, float32 [H][W] at the out pointers)
        and {reused, disoccluded, not_surface, 0} (uint32) at stats_ptr.
        Complete on `stream`'s order or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_reproject_device(
            self.h, C.byref(rp), prev_pixels_ptr, prev_counters_ptr, prev_m2_ptr, prev_guides_ptr, cur_guides_ptr,
            out_pixels_ptr, out_counters_ptr, out_m2_ptr, stats_ptr, stream))

    def reproject(self, rp: ReprojectParams, prev_pixels, prev_counters, prev_m2, prev_guides, cur_guides):
        """Host-buffer reprojection (ipt_reproject): (pixels float32, counters
        uint32, m2 float32, each [H*W], {reused, disoccluded, not_surface});
        the guides are GuideRecord arrays."""
        px = np.ascontiguousarray(prev_pixels, np.float32).reshape(-1)
        cn = np.ascontiguousarray(prev_counters, np.uint32).reshape(-1)
        mm = np.ascontiguousarray(prev_m2, np.float32).reshape(-1)
        pg = np.ascontiguousarray(prev_guides, GuideRecord).reshape(-1)
        cg = np.ascontiguousarray(cur_guides, GuideRecord).reshape(-1)
        n = rp.width * rp.height
        for a in (px, cn, mm, pg, cg):
            if a.size < n:
                raise ValueError("a buffer holds fewer than width * height elements")
        opx, ocn, om2 = np.empty(max(n, 0), np.float32), np.empty(max(n, 0), np.uint32), np.empty(max(n, 0), np.float32)
        st = np.zeros(4, np.uint32)
        _check(self.lib, self.h, self.lib.ipt_reproject(
            self.h, C.byref(rp), px.ctypes.data, cn.ctypes.data, mm.ctypes.data, pg.ctypes.data, cg.ctypes.data,
            opx.ctypes.data, ocn.ctypes.data, om2.ctypes.data, st.ctypes.data))
        return opx, ocn, om2, {"reused": int(st[0]), "disoccluded": int(st[1]), "not_surface": int(st[2])}

    def wait(self):
        _check(self.lib, self.h, self.lib.ipt_render_wait(self.h))

    @property
    def has_async(self) -> bool:
        return hasattr(self.lib, "ipt_render_device_async")

    def counters(self) -> dict:
        c = Counters()
        _check(self.lib, self.h, self.lib.ipt_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        _check(self.lib, self.h, self.lib.ipt_reset_counters(self.h))

    def math_selfcheck(self, fn: int, lo_bits: int = 0, hi_bits: int = 1 << 32):
        """(mismatches, first differing bit pattern) of the device fast path of
        math fn against its exact restatement over [lo_bits, hi_bits)."""
        bad, first = C.c_uint64(), C.c_uint32()
        _check(self.lib, self.h, self.lib.ipt_math_selfcheck(self.h, fn, lo_bits, hi_bits, C.byref(bad),
                                                             C.byref(first)))
        return int(bad.value), int(first.value)

    def ddf_sample(self, kind: int, params, u: np.ndarray) -> np.ndarray:
        """n directions from n x {pick, u1, u2} uniforms (ipt_ddf_sample)."""
        pr = np.ascontiguousarray(np.pad(np.asarray(params, np.float32), (0, 8))[:8])
        uu = np.ascontiguousarray(u, np.float32).reshape(-1, 3)
        out = np.empty((len(uu), 3), np.float32)
        _check(self.lib, self.h, self.lib.ipt_ddf_sample(self.h, kind, pr.ctypes.data, uu.ctypes.data, len(uu),
                                                         out.ctypes.data))
        return out

    def ddf_value(self, kind: int, params, dirs: np.ndarray) -> np.ndarray:
        pr = np.ascontiguousarray(np.pad(np.asarray(params, np.float32), (0, 8))[:8])
        dd = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.empty(len(dd), np.float32)
        _check(self.lib, self.h, self.lib.ipt_ddf_value(self.h, kind, pr.ctypes.data, dd.ctypes.data, len(dd),
                                                        out.ctypes.data))
        return out

    def smooth(self, pixels: np.ndarray, width: int, height: int, side: int, in_place: bool = True):
        """GridRenderPlane::smooth (in_place) / computeSmoothedMax on the GPU:
        returns (pixels after the call, max_value)."""
        px = np.ascontiguousarray(pixels, dtype=np.float32).copy()
        mx = C.c_float()
        _check(self.lib, self.h, self.lib.ipt_smooth(self.h, px.ctypes.data, width, height, side,
                                                     1 if in_place else 0, C.byref(mx)))
        return px, float(mx.value)

    def glare(self, img: np.ndarray, width: int, height: int, cutoff: float) -> np.ndarray:
        """Gui's glare bloom (gui.cpp:28-52) on the GPU."""
        src = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty_like(src)
        _check(self.lib, self.h, self.lib.ipt_glare(self.h, src.ctypes.data, out.ctypes.data, width, height,
                                                    C.c_float(cutoff)))
        return out

    def display_device(self, params: DisplayParams, pixels_ptr, gray8_ptr, processed_ptr=None, tone_ptr=None,
                       stream=None):
        """Queue the display pipeline on device buffers (ipt_display_device):
        glare (params.glare_cutoff > 0), tone map, 8-bit. Complete on
        `stream`'s order or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_display_device(self.h, C.byref(params), pixels_ptr, processed_ptr,
                                                             tone_ptr, gray8_ptr, stream))

    def display(self, pixels: np.ndarray, width: int, height: int, glare_cutoff: float = 0.0) -> dict:
        """Host-buffer display pipeline (ipt_display): {processed, tone, gray8}."""
        src = np.ascontiguousarray(pixels, dtype=np.float32)
        out = {"processed": np.empty(src.size, np.float32), "tone": np.empty(src.size, np.float32),
               "gray8": np.empty(src.size, np.uint8)}
        _check(self.lib, self.h, self.lib.ipt_display(
            self.h, C.byref(make_display_params(width, height, glare_cutoff)),
            src.ctypes.data if src.size else None, out["processed"].ctypes.data, out["tone"].ctypes.data,
            out["gray8"].ctypes.data))
        return out

    def display_stats_device(self, params: DisplayStatsParams, pixels_ptr, processed_ptr=None, tone_ptr=None,
                             gray8_ptr=None, hist_ptr=None, stats_ptr=None, stream=None):
        """Queue the display pipeline with its statistics on device buffers
        (ipt_display_stats_device): the Gui's histogram (params.hist_buckets
        uint32 counts at hist_ptr), {mx, mx/100000, white, 0} at stats_ptr,
        and tone / gray8 with the white point of params.white_rank. Every
        output is optional; complete on `stream`'s order or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_display_stats_device(
            self.h, C.byref(params), pixels_ptr, processed_ptr, tone_ptr, gray8_ptr, hist_ptr, stats_ptr, stream))

    def display_stats(self, pixels: np.ndarray, width: int, height: int, glare_cutoff: float = 0.0,
                      hist_buckets: int = 400, white_rank: int = -1) -> dict:
        """Host-buffer display statistics (ipt_display_stats):
        {processed, tone, gray8, hist, stats}."""
        src = np.ascontiguousarray(pixels, dtype=np.float32)
        out = {"processed": np.empty(src.size, np.float32), "tone": np.empty(src.size, np.float32),
               "gray8": np.empty(src.size, np.uint8), "hist": np.zeros(max(hist_buckets, 0), np.uint32),
               "stats": np.empty(4, np.float32)}
        _check(self.lib, self.h, self.lib.ipt_display_stats(
            self.h, C.byref(make_display_stats_params(width, height, glare_cutoff, hist_buckets, white_rank)),
            src.ctypes.data if src.size else None, out["processed"].ctypes.data, out["tone"].ctypes.data,
            out["gray8"].ctypes.data, out["hist"].ctypes.data if hist_buckets > 0 else None,
            out["stats"].ctypes.data))
        return out

    def smooth_device(self, in_ptr, out_ptr, width: int, height: int, side: int, max_ptr=None, stream=None):
        """Queue GridRenderPlane::smooth (out_ptr, which may equal in_ptr) or
        computeSmoothedMax (out_ptr None) on device buffers (ipt_smooth_device);
        max_value goes to the float at max_ptr. Complete on `stream`'s order
        or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_smooth_device(self.h, in_ptr, out_ptr, width, height, side, max_ptr,
                                                            stream))

    def pgm_device(self, params: PgmParams, pixels_ptr, pixel_max_ptr=None, smoothed_ptr=None, gray8_ptr=None,
                   stats_ptr=None, stream=None):
        """Queue main.cpp's PGM chain on device buffers (ipt_pgm_device):
        smooth, smoothed max, n_val bytes at gray8_ptr, {max_value used,
        logf(contrast), 0, 0} at stats_ptr. Every output is optional; complete
        on `stream`'s order or after wait()."""
        _check(self.lib, self.h, self.lib.ipt_pgm_device(self.h, C.byref(params), pixels_ptr, pixel_max_ptr,
                                                         smoothed_ptr, gray8_ptr, stats_ptr, stream))

    def pgm(self, pixels: np.ndarray, width: int, height: int, smooth_side: int = 0, max_side: int = 0,
            contrast: float = 500.0, gamma: float = 0.6, max_value: float = 0.0, pixel_max=None) -> dict:
        """Host-buffer PGM chain (ipt_pgm): {smoothed, gray8, stats}."""
        src = np.ascontiguousarray(pixels, dtype=np.float32)
        pm = None if pixel_max is None else np.ascontiguousarray(pixel_max, dtype=np.float32)
        out = {"smoothed": np.empty(src.size, np.float32), "gray8": np.empty(src.size, np.uint8),
               "stats": np.empty(4, np.float32)}
        _check(self.lib, self.h, self.lib.ipt_pgm(
            self.h, C.byref(make_pgm_params(width, height, smooth_side, max_side, contrast, gamma, max_value)),
            src.ctypes.data if src.size else None, None if pm is None else pm.ctypes.data,
            out["smoothed"].ctypes.data, out["gray8"].ctypes.data, out["stats"].ctypes.data))
        return out

    def logf_device(self, x: np.ndarray) -> np.ndarray:
        """logf(x) as the PGM kernels compute it, on the device."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        _check(self.lib, self.h, self.lib.ipt_logf_device(self.h, x.ctypes.data, out.ctypes.data, x.size))
        return out

    def powf_device(self, x: np.ndarray, y: float) -> np.ndarray:
        """powf(x, y) as the display kernels compute it, on the device."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        _check(self.lib, self.h, self.lib.ipt_powf_device(self.h, x.ctypes.data, C.c_float(y), out.ctypes.data,
                                                          x.size))
        return out

    def profile(self) -> dict:
        """{phase: (wave executions, active lanes)} from an IPT_PROF build."""
        n = 2 * len(PROFILE_PHASES) + 12
        buf = (C.c_uint64 * n)()
        _check(self.lib, self.h, self.lib.ipt_get_profile(self.h, buf, n))
        out = {ph: (int(buf[2 * i]), int(buf[2 * i + 1])) for i, ph in enumerate(PROFILE_PHASES)}
        base = 2 * len(PROFILE_PHASES)
        out["stamps"] = {sg: int(buf[base + i]) for i, sg in enumerate(STAMP_SEGMENTS)}
        return out

    def last_kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        _check(self.lib, self.h, self.lib.ipt_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_units(self):
        """(dense units, units the pools handed out, units traced) of the
        full-estimator launches completed by the last wait (ipt_last_units)."""
        out = (C.c_uint64 * 3)()
        _check(self.lib, self.h, self.lib.ipt_last_units(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def last_instance(self):
        """(MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED): the path_kernel instance
        of the context's most recent path-kernel launch (ipt_last_instance)."""
        out = (C.c_int32 * 6)()
        _check(self.lib, self.h, self.lib.ipt_last_instance(self.h, out))
        return tuple(int(v) for v in out)

    def compact_plan(self, p: Params, mask_ptr=None):
        """The compaction plan of the call's first launch (ipt_compact_plan):
        (src uint32[n_active], the dense units in compact order; n_active;
        start, the pool's first unit). mask_ptr: a device mask or None."""
        per_launch = p.spp * p.width * p.height
        src = np.zeros(max(per_launch, 1), np.uint32)
        n, start = C.c_uint64(), C.c_uint64()
        _check(self.lib, self.h, self.lib.ipt_compact_plan(self.h, C.byref(p), mask_ptr, src.ctypes.data, per_launch,
                                                           C.byref(n), C.byref(start)))
        return src[:int(n.value)].copy(), int(n.value), int(start.value)

    def math_device(self, fn: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        _check(self.lib, self.h, self.lib.ipt_math_device(self.h, fn, x.ctypes.data, out.ctypes.data, x.size))
        return out


def philox(ctr, key, ctx: "Context | None" = None) -> np.ndarray:
    """Philox4x32-10 blocks as the kernels compute them (ipt_philox): ctr
    [n][4] uint32, key (k0, k1); ctx None = the library's host build."""
    lib = load()
    c = np.ascontiguousarray(np.asarray(ctr, np.uint32).reshape(-1, 4))
    out = np.zeros_like(c)
    h = ctx.h if ctx is not None else None
    rc = lib.ipt_philox(h, int(key[0]), int(key[1]), c.ctypes.data, out.ctypes.data, len(c))
    if rc != IPT_OK:
        raise IptError(rc, lib.ipt_last_error(h).decode(errors="replace") if h else "ipt_philox")
    return out


def math_host(fn: int, x: np.ndarray) -> np.ndarray:
    lib = load()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    rc = lib.ipt_math_host(fn, x.ctypes.data, out.ctypes.data, x.size)
    if rc != IPT_OK:
        raise IptError(rc, "ipt_math_host")
    return out


def powf_host(x: np.ndarray, y: float) -> np.ndarray:
    """powf(x, y) by the library's host build of the display kernels' powf_."""
    lib = load()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    rc = lib.ipt_powf_host(x.ctypes.data, C.c_float(y), out.ctypes.data, x.size)
    if rc != IPT_OK:
        raise IptError(rc, "ipt_powf_host")
    return out


def logf_host(x: np.ndarray) -> np.ndarray:
    """logf(x) by the library's host build of the PGM kernels' logf_."""
    lib = load()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    rc = lib.ipt_logf_host(x.ctypes.data, out.ctypes.data, x.size)
    if rc != IPT_OK:
        raise IptError(rc, "ipt_logf_host")
    return out


MATH_FNS = {"acosf": 0, "sinf": 1, "cosf": 2, "acos_f64_f32": 3, "sincosf_sin": 4,
            "sincosf_cos": 5, "sqrtf": 6, "div_pi": 7, "two_pi_times": 8, "div_pairs": 9,
            "div_inrange_pairs": 10, "longer_pairs": 11, "udiv_exact_pairs": 12,
            "sqrt_inrange": 13, "frame_angle_sin": 14, "frame_angle_cos": 15}
SELFCHECK_FRAME_FAST = 16  # ipt_math_selfcheck only: fast vs exact sphere-in-box frame
# ipt_math_selfcheck only: reciprocal with 1 / 2 Newton corrections vs the round-4 three-correction
# sequence; the range-free division vs IEEE over the division pairs / near-all-ones divisors
SELFCHECK_RCP1, SELFCHECK_RCP2, SELFCHECK_DIV_PAIRS, SELFCHECK_DIV_ONES = 17, 18, 19, 20
# ipt_math_selfcheck only: the range-free division over every pair of significands (pattern
# indices up to 2^46) and the reciprocal's exact scaling over the range (all 2^32 floats)
SELFCHECK_DIV_ALL_SIGNIFICANDS, SELFCHECK_RCP_SCALING = 21, 22


def shard_plan(p: Params):
    """(owned_rows bool[H], candidate source rows int[]) of a sharded render;
    the candidates follow the plane's row map (p.flags & IPT_FLAG_GUI_PLANE)."""
    lib = load()
    owned = np.zeros(p.height, np.uint8)
    cand = np.zeros(p.height, np.int32)
    n = C.c_int32()
    rc = lib.ipt_shard_plan(C.byref(p), owned.ctypes.data, cand.ctypes.data, C.byref(n))
    if rc != IPT_OK:
        raise IptError(rc, "ipt_shard_plan")
    return owned.astype(bool), cand[:n.value].copy()
