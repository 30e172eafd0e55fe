"""ctypes mirror of include/ptx.h (type declarations only -- no behaviour).

Every structure here must match the C header field for field; tests/test_abi.py
checks the sizes against the compiled library.
"""
import ctypes as C

PTX_ABI_VERSION = 4

PTX_MAT_LAMBERTIAN, PTX_MAT_METAL, PTX_MAT_DIELECTRIC = 0, 1, 2
PTX_TEX_SOLID, PTX_TEX_CHECKER = 0, 1
PTX_BG_BLACK, PTX_BG_SKY = 0, 1
PTX_LEAF_SIMD, PTX_LEAF_ARRAY = 0, 1
PTX_KERNEL_NAMES = ("generate", "trace", "shade", "accum", "film", "bounce")
PTX_N_KERNELS = 6
PTX_RENDER_ASYNC = 1
PTX_LIGHTING_REFERENCE, PTX_LIGHTING_PATH_ORDER, PTX_LIGHTING_SAMPLED = 0, 1, 2
PTX_LIGHTING_NAMES = ("reference", "path-order", "sampled")
PTX_MAX_LIGHT_TRIANGLES = 64


def lighting_mode(mode):
    """A PTX_LIGHTING_* value from the value itself or from its name in PTX_LIGHTING_NAMES."""
    if isinstance(mode, str):
        if mode not in PTX_LIGHTING_NAMES:
            raise ValueError(f"lighting must be one of {', '.join(PTX_LIGHTING_NAMES)} (got {mode!r})")
        return PTX_LIGHTING_NAMES.index(mode)
    mode = int(mode)
    if not 0 <= mode < len(PTX_LIGHTING_NAMES):
        raise ValueError(f"lighting must be 0, 1 or 2 (got {mode})")
    return mode

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("index", C.c_double), ("emit", C.c_double * 3)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32),
                ("even", C.c_double * 3), ("odd", C.c_double * 3)]


class Camera(C.Structure):
    _fields_ = [("lower_left_x", C.c_double), ("lower_left_y", C.c_double), ("view_x", C.c_double), ("view_y", C.c_double)]


class Background(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("horizon", C.c_double * 3), ("zenith", C.c_double * 3)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("n_spheres", C.c_int32), ("sphere_x", c_double_p), ("sphere_y", c_double_p), ("sphere_z", c_double_p),
        ("sphere_r", c_double_p), ("sphere_material", c_int32_p),
        ("n_vertices", C.c_int32), ("vertex_x", c_double_p), ("vertex_y", c_double_p), ("vertex_z", c_double_p),
        ("n_triangles", C.c_int32), ("tri_indices", c_int32_p), ("tri_uv", c_double_p), ("tri_material", c_int32_p),
        ("n_floor_triangles", C.c_int32), ("floor_vertices", c_double_p), ("floor_uv", c_double_p),
        ("floor_material", c_int32_p),
        ("n_materials", C.c_int32), ("materials", C.POINTER(Material)),
        ("n_textures", C.c_int32), ("textures", C.POINTER(Texture)),
        ("camera", Camera), ("background", Background),
        ("leaf_kind", C.c_int32), ("length_cutoff", C.c_int32), ("num_bins", C.c_int32), ("reserved", C.c_int32),
    ]


class RenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("samples_per_pixel", C.c_int32), ("max_bounces", C.c_int32),
        ("band_rows", C.c_int32), ("band_first", C.c_int32), ("band_step", C.c_int32),
        ("count_work", C.c_int32), ("time_kernels", C.c_int32), ("passes_per_batch", C.c_int32),
        ("n_gpus", C.c_int32), ("flags", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("samples", C.c_int64), ("segments", C.c_int64), ("nodes_tested", C.c_int64), ("prims_tested", C.c_int64),
        ("floor_tested", C.c_int64), ("render_ms", C.c_double),
        ("kernel_ms", C.c_double * PTX_N_KERNELS), ("kernel_launches", C.c_int64 * PTX_N_KERNELS),
        ("tree_nodes", C.c_int32), ("tree_depth", C.c_int32), ("tree_leaves", C.c_int32), ("leaf_slots", C.c_int32),
        ("build_ms", C.c_double), ("traversal_in_lds", C.c_int32), ("bvh_built_on_gpu", C.c_int32),
        ("filter_undecided", C.c_int64), ("filter_fallback_steps", C.c_int64),
        ("peer_copies", C.c_int32), ("staged_copies", C.c_int32),
        ("solo_launches", C.c_int32), ("carry_launches", C.c_int32),
        ("primary_lane_walks", C.c_int32), ("lds_oct_launches", C.c_int32),
    ]


class ProgressiveParams(C.Structure):
    _fields_ = [("passes_per_update", C.c_int32), ("want_error", C.c_int32), ("target_rel_err", C.c_double)]


class AdaptiveParams(C.Structure):
    _fields_ = [("min_passes", C.c_int32), ("passes_per_round", C.c_int32), ("target_rel_err", C.c_double),
                ("radiance_floor", C.c_double)]


PTX_FEATURE_DOUBLES = 8  # albedo r g b, normal x y z, depth, hits
PTX_DENOISE_DEMODULATE = 1


class DenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("normal_power_log2", C.c_int32), ("feature_passes", C.c_int32), ("flags", C.c_int32),
                ("sigma_luminance", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double)]


PTX_HISTORY_DOUBLES = 12  # M1 r g b, M2 r g b, N, hf, normal x y z, zc


class TemporalCamera(C.Structure):  # ptx_temporal_camera, 128 bytes
    _fields_ = [("origin", C.c_double * 3), ("rotation", C.c_double * 9), ("view", Camera)]


class TemporalParams(C.Structure):  # ptx_temporal_params, 32 bytes
    _fields_ = [("max_history_passes", C.c_double), ("normal_threshold", C.c_double), ("depth_tolerance", C.c_double),
                ("min_weight", C.c_double)]


def temporal_camera(origin, rotation, view):
    """An abi.TemporalCamera from an origin (3), a rotation (3 x 3, row-major) and a view: a Camera or its four fields."""
    import numpy as np
    o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    r = np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
    v = view if isinstance(view, Camera) else Camera(*[float(a) for a in view])
    return TemporalCamera((C.c_double * 3)(*o), (C.c_double * 9)(*r), Camera(v.lower_left_x, v.lower_left_y, v.view_x, v.view_y))


PTX_PROJECTION_PERSPECTIVE, PTX_PROJECTION_LATLONG = 0, 1
PTX_PROJECTION_NAMES = ("perspective", "latlong")


def projection_kind(projection):
    """A PTX_PROJECTION_* value from the value itself or from its name in PTX_PROJECTION_NAMES."""
    if isinstance(projection, str):
        if projection not in PTX_PROJECTION_NAMES:
            raise ValueError(f"projection must be one of {', '.join(PTX_PROJECTION_NAMES)} (got {projection!r})")
        return PTX_PROJECTION_NAMES.index(projection)
    return int(projection)


PTX_RAYS_NORMALIZE = 1


class RaysParams(C.Structure):  # ptx_rays_params, 16 bytes
    _fields_ = [("max_bounces", C.c_int32), ("rays_per_bin", C.c_int32), ("flags", C.c_int32), ("count_work", C.c_int32)]


def rays_params(max_bounces=8, rays_per_bin=1, normalize=False, count_work=False):
    """An abi.RaysParams for ptx_render_rays / ptx_render_rays_device."""
    return RaysParams(int(max_bounces), int(rays_per_bin), PTX_RAYS_NORMALIZE if normalize else 0, int(bool(count_work)))


PTX_FILM_MAX_ORDER, PTX_FILM_MAX_RADIUS = 16, 7
PTX_FILM_RENORMALISE = 1


class FilmParams(C.Structure):
    _fields_ = [("order", C.c_int32), ("pixel_radius", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


def film_params(film=None, renormalise=None):
    """An abi.FilmParams from None (order 5, radius 1, no renormalisation), an (order, radius) or (order, radius, renormalise)
    tuple, or a FilmParams; checked as the library checks it (ValueError)."""
    if isinstance(film, FilmParams):
        f = FilmParams(film.order, film.pixel_radius, film.flags, film.reserved)
    else:
        t = (5, 1) if film is None else tuple(film)
        if len(t) not in (2, 3):
            raise ValueError("film must be (order, radius) or (order, radius, renormalise)")
        f = FilmParams(int(t[0]), int(t[1]), PTX_FILM_RENORMALISE if len(t) == 3 and t[2] else 0, 0)
    if renormalise is not None:
        f.flags = PTX_FILM_RENORMALISE if renormalise else 0
    if not 1 <= f.order <= PTX_FILM_MAX_ORDER:
        raise ValueError(f"film order must be in [1, {PTX_FILM_MAX_ORDER}] (got {f.order})")
    if not 0 <= f.pixel_radius <= PTX_FILM_MAX_RADIUS:
        raise ValueError(f"film radius must be in [0, {PTX_FILM_MAX_RADIUS}] (got {f.pixel_radius})")
    if f.order < 2 * f.pixel_radius + 1:
        raise ValueError(f"film order {f.order} is smaller than 2 * radius + 1 = {2 * f.pixel_radius + 1}: the reference's kernel is "
                         "lopsided there")
    if f.flags & ~PTX_FILM_RENORMALISE or f.reserved:
        raise ValueError("unknown bits in the film's flags")
    return f


# display outputs (include/ptx.h): the pixel formats with their numpy dtype and channels, the transfers, the tone curves
PTX_PIXEL_RGB8, PTX_PIXEL_RGBA8, PTX_PIXEL_RGB32F, PTX_PIXEL_RGBA32F = range(4)
PTX_PIXEL_NAMES = ("rgb8", "rgba8", "rgb32f", "rgba32f")
PTX_PIXEL_LAYOUT = (("uint8", 3), ("uint8", 4), ("float32", 3), ("float32", 4))
PTX_TRANSFER_REFERENCE, PTX_TRANSFER_LINEAR, PTX_TRANSFER_SRGB = range(3)
PTX_TRANSFER_NAMES = ("reference", "linear", "srgb")
PTX_TONE_NONE, PTX_TONE_REINHARD, PTX_TONE_ACES = range(3)
PTX_TONE_NAMES = ("none", "reinhard", "aces")


class DisplayParams(C.Structure):  # ptx_display_params, 40 bytes
    _fields_ = [("format", C.c_int32), ("transfer", C.c_int32), ("tone", C.c_int32), ("flags", C.c_int32), ("exposure", C.c_double),
                ("reserved", C.c_int32 * 4)]


def _named(value, names, what):
    if isinstance(value, str):
        if value not in names:
            raise ValueError(f"{what} must be one of {', '.join(names)} (got {value!r})")
        return names.index(value)
    return int(value)


def display_params(display=None, format=None, transfer=None, tone=None, exposure=None):
    """An abi.DisplayParams from None (RGB8, reference, no tone curve, exposure 1) or a DisplayParams, with the named fields set: each
    a PTX_* value or its name in PTX_PIXEL_NAMES / PTX_TRANSFER_NAMES / PTX_TONE_NAMES.  Not checked here: the library's refusals
    (PtxError, the rule in the message) are the ones to see."""
    d = DisplayParams(PTX_PIXEL_RGB8, PTX_TRANSFER_REFERENCE, PTX_TONE_NONE, 0, 1.0)
    if display is not None:
        C.memmove(C.byref(d), C.byref(display), C.sizeof(d))
    if format is not None:
        d.format = _named(format, PTX_PIXEL_NAMES, "format")
    if transfer is not None:
        d.transfer = _named(transfer, PTX_TRANSFER_NAMES, "transfer")
    if tone is not None:
        d.tone = _named(tone, PTX_TONE_NAMES, "tone")
    if exposure is not None:
        d.exposure = float(exposure)
    return d


# ptx_update_display_fn: (user, passes_done, rel_err, pixels, err) -> non-zero stops the render
UPDATE_DISPLAY_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p)

PTX_IMAGE_BILINEAR, PTX_IMAGE_REPEAT_U, PTX_IMAGE_REPEAT_V = 1, 2, 4
PTX_IMAGE_MAX_SIZE = 16384

# ptx_walk_rays: which of the bounce kernels' walks to run (include/ptx.h)
(PTX_WALK_SHARED_ASM, PTX_WALK_OCT_ASM, PTX_WALK_SHARED_DIV, PTX_WALK_PACKET, PTX_WALK_SHARED_ASM_ZERO, PTX_WALK_OCT_ASM_ZERO,
 PTX_WALK_SHARED_DIV_ZERO, PTX_WALK_SHARED_ASM_TAIL, PTX_WALK_OCT_ASM_TAIL, PTX_WALK_SHARED_DIV_TAIL) = range(10)
# ptx_walk_next_leaf: the walks with a node loop of their own (no PACKET, no _TAIL)
PTX_NEXT_LEAF_WALKS = (PTX_WALK_SHARED_ASM, PTX_WALK_OCT_ASM, PTX_WALK_SHARED_DIV, PTX_WALK_SHARED_ASM_ZERO, PTX_WALK_OCT_ASM_ZERO,
                       PTX_WALK_SHARED_DIV_ZERO)

# ptx_kernel_table: the kernel families its names begin with, in table order (include/ptx.h)
PTX_KERNEL_FAMILIES = ("k_trace", "k_shade_pool", "k_bounce_carry", "k_bounce")


class Image(C.Structure):  # ptx_image
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32), ("rgb", c_double_p)]


def image(array, flags=0):
    """(abi.Image, the array it points into) from an (H, W, 3) array of linear binary64 texels, row 0 = v 0; the caller keeps the
    second value alive for the duration of the call (the library copies the texels)."""
    import numpy as np
    a = np.ascontiguousarray(array, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("an image must be an array of shape (height, width, 3)")
    return Image(a.shape[1], a.shape[0], int(flags), 0, a.ctypes.data_as(c_double_p)), a


# ptx_round_fn: (user, round, passes_done, active_next, samples, rel_err, rgb, err, passes) -> non-zero stops the render
ROUND_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                       C.c_void_p)


# ptx_tile_list_stats: int64_t out[5]
TileListStats = C.c_int64 * 5
TILE_LIST_STATS = ("list_launches", "tiles", "walk_tiles", "longest_list", "fallback_chunks")

PTX_LIGHT_POINT, PTX_LIGHT_SPOT = 0, 1


class Light(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("position", C.c_double * 3), ("direction", C.c_double * 3),
                ("color", C.c_double * 3), ("power", C.c_double)]


class PpmParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("max_bounces", C.c_int32),
                ("photon_count", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_double)]


class PpmStats(C.Structure):
    _fields_ = [("photons_stored", C.c_int64), ("photon_rays", C.c_int64), ("eye_rays", C.c_int64), ("neighbors", C.c_int64),
                ("photon_ms", C.c_double), ("build_ms", C.c_double), ("gather_ms", C.c_double), ("total_ms", C.c_double),
                ("last_radius", C.c_double), ("device_trees", C.c_int64), ("gpu_built_trees", C.c_int64)]


def ppm_params(width=600, height=None, iterations=10, max_bounces=4, photon_count=75000, alpha=2.0 / 3.0):
    """Defaults of Progressive_photon_map.Args.parse (progressive_photon_map.ml:17-54)."""
    p = PpmParams()
    p.width, p.height = width, width if height is None else height
    p.iterations, p.max_bounces, p.photon_count, p.alpha = iterations, max_bounces, photon_count, alpha
    return p
