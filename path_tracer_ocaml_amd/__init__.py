"""path_tracer_ocaml_amd -- MI355X-native drop-in for the sampling hot path of dalev/path-tracer-ocaml.

The product is the C-ABI shared library ``libptx_hip.so`` (HIP kernels for gfx950 + host BVH builder,
sources in ``csrc/``, interface in ``include/ptx.h``).  This package is only the thin ctypes binding the
tests and the benchmark use, plus a Python mirror of the reference's operator surface
(``Integrator.create / render``, ``Render_command.Args``) in :mod:`path_tracer_ocaml_amd.integrator`.

There is NO CPU fallback: loading fails loudly if the HIP library is missing, and every compute entry
point returns an error when no HIP device is present.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTX_LIB overrides the library path (kernel-variant experiments); the default is the in-tree build
LIB_PATH = os.environ.get("PTX_LIB") or os.path.join(_HERE, "libptx_hip.so")
_LIB = None

dp = abi.c_double_p
ip = abi.c_int32_p


class PtxError(RuntimeError):
    pass


EXPORTS = (
    "ptx_version", "ptx_leaf_size", "ptx_last_error", "ptx_device_count", "ptx_scene_create", "ptx_scene_destroy",
    "ptx_scene_stats", "ptx_render", "ptx_local_rows", "ptx_global_row", "ptx_render_raw_device",
    "ptx_film_resolve_device", "ptx_trace_samples", "ptx_intersect_rays", "ptx_scene_tree", "ptx_lds_sample",
    "ptx_math_eval", "ptx_ppm_render", "ptx_debug_first_scatter", "ptx_render_multi", "ptx_scene_replicate",
    "ptx_film_resolve_banded_device", "ptx_film_resolve_banded_queue", "ptx_release_workspaces",
    "ptx_image_pin", "ptx_image_unpin", "ptx_render_passes_device", "ptx_pixel_error_device", "ptx_render_progressive",
    "ptx_render_pixels_device", "ptx_film_resolve_counts_device", "ptx_pixel_error_counts_device", "ptx_render_adaptive",
    "ptx_scene_set_lighting", "ptx_scene_lighting",
    "ptx_render_features_device", "ptx_denoise_defaults", "ptx_denoise_device", "ptx_render_denoised",
    "ptx_film_defaults", "ptx_film_weights", "ptx_scene_set_film", "ptx_scene_film", "ptx_film_resolve_ex_device",
    "ptx_film_resolve_banded_ex_device", "ptx_film_resolve_counts_ex_device", "ptx_tile_list_stats",
    "ptx_scene_set_texture_image", "ptx_scene_set_environment", "ptx_scene_texture_image", "ptx_scene_environment",
    "ptx_texture_eval", "ptx_environment_eval", "ptx_walk_rays", "ptx_walk_next_leaf",
    "ptx_scene_set_environment_sampling", "ptx_scene_environment_sampling", "ptx_environment_distribution",
    "ptx_environment_sample", "ptx_environment_pdf",
    "ptx_scene_set_lens", "ptx_scene_lens",
    "ptx_scene_set_camera_pose", "ptx_scene_camera_pose", "ptx_camera_rays",
    "ptx_temporal_defaults", "ptx_temporal_accumulate_device", "ptx_render_temporal", "ptx_temporal_reset",
    "ptx_scene_set_sphere_light_sampling", "ptx_scene_sphere_lights", "ptx_light_table", "ptx_light_sample", "ptx_light_pdf",
    "ptx_render_rays_device", "ptx_render_rays", "ptx_scene_set_camera_projection", "ptx_scene_camera_projection",
    "ptx_scene_set_camera_shutter", "ptx_scene_camera_shutter",
    "ptx_kernel_table", "ptx_scene_launched_kernels", "ptx_scene_clear_launched_kernels",
    "ptx_display_defaults", "ptx_display_check", "ptx_display_pixel_bytes", "ptx_display_thresholds", "ptx_display_apply",
    "ptx_display_image_device", "ptx_display_range_device", "ptx_image_pin_bytes", "ptx_render_display", "ptx_render_progressive_display",
)

PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64)
# ptx_update_fn: (user, passes_done, rel_err, rgb, err) -> non-zero stops the render
UPDATE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p)
ROUND_FN = abi.ROUND_FN
# ptx_ppm_iteration_fn: (user, iteration, radius, photon_map_length, img_sum)
PPM_ITERATION_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_double, C.c_int64, dp)


def lib():
    """Loads libptx_hip.so; raises PtxError if it has not been built (run __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise PtxError(f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                       "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # PyTorch bundles its own libamdhip64.so.7.  Two HIP runtimes in one process cannot both own the GPU
    # ("No HIP GPUs are available" from whichever initialises second), so when torch is installed load it
    # FIRST: libptx_hip.so's DT_NEEDED libamdhip64.so.7 then binds to the copy that is already mapped.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional: the C ABI does not need it
        pass
    L = C.CDLL(LIB_PATH)
    L.ptx_version.restype = C.c_int32
    L.ptx_leaf_size.restype = C.c_int32
    L.ptx_last_error.restype = C.c_char_p
    L.ptx_device_count.restype = C.c_int32
    L.ptx_scene_create.restype = C.c_void_p
    L.ptx_scene_create.argtypes = [C.POINTER(abi.SceneDesc), C.c_int32]
    L.ptx_scene_destroy.argtypes = [C.c_void_p]
    L.ptx_scene_stats.argtypes = [C.c_void_p, C.POINTER(abi.Stats)]
    if hasattr(L, "ptx_tile_list_stats"):  # (a PTX_LIB built from an older tree, in an A/B, has none)
        L.ptx_tile_list_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.ptx_render.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), dp, C.POINTER(abi.Stats), C.c_void_p, C.c_void_p]
    L.ptx_local_rows.argtypes = [C.POINTER(abi.RenderParams)]
    L.ptx_global_row.argtypes = [C.POINTER(abi.RenderParams), C.c_int32]
    L.ptx_render_raw_device.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_void_p, C.c_void_p,
                                        C.POINTER(abi.Stats)]
    L.ptx_film_resolve_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptx_film_resolve_banded_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p]
    L.ptx_film_resolve_banded_queue.argtypes = L.ptx_film_resolve_banded_device.argtypes
    L.ptx_render_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(abi.RenderParams), dp, C.POINTER(abi.Stats),
                                   C.c_void_p, C.c_void_p]
    L.ptx_scene_replicate.restype = C.c_void_p
    L.ptx_scene_replicate.argtypes = [C.c_void_p, C.c_int32]
    L.ptx_release_workspaces.restype = None
    L.ptx_image_pin.argtypes = [C.c_void_p, dp, C.c_int64]
    L.ptx_image_unpin.argtypes = [C.c_void_p]
    L.ptx_render_passes_device.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
    L.ptx_pixel_error_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         dp, C.c_void_p]
    L.ptx_render_progressive.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.POINTER(abi.ProgressiveParams), dp, dp,
                                         ip, C.POINTER(abi.Stats), C.c_void_p, C.c_void_p]
    L.ptx_render_pixels_device.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
    L.ptx_film_resolve_counts_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
    L.ptx_pixel_error_counts_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, dp, C.c_void_p]
    L.ptx_render_adaptive.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.POINTER(abi.AdaptiveParams), dp, dp, ip,
                                      C.POINTER(abi.Stats), C.c_void_p, C.c_void_p]
    L.ptx_trace_samples.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp,
                                    C.POINTER(abi.Stats)]
    L.ptx_intersect_rays.argtypes = [C.c_void_p, C.c_int64, dp, dp, dp, ip, C.POINTER(abi.Stats)]
    L.ptx_scene_tree.argtypes = [C.c_void_p, dp, ip, C.c_int32, ip, C.c_int32]
    L.ptx_lds_sample.argtypes = [C.c_int32, C.c_int32, C.c_int64, ip, ip, dp]
    L.ptx_math_eval.argtypes = [C.c_int32, C.c_int32, C.c_int64, dp, dp, dp]
    L.ptx_ppm_render.argtypes = [C.c_void_p, C.POINTER(abi.PpmParams), C.POINTER(abi.Light), C.c_int32, dp,
                                 C.POINTER(abi.PpmStats), C.c_void_p, C.c_void_p]
    L.ptx_scene_set_lighting.argtypes = [C.c_void_p, C.c_int32]
    L.ptx_scene_lighting.argtypes = [C.c_void_p, ip, ip, dp]
    L.ptx_render_features_device.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.POINTER(abi.Stats)]
    L.ptx_denoise_defaults.argtypes = [C.POINTER(abi.DenoiseParams)]
    L.ptx_denoise_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(abi.DenoiseParams), C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptx_render_denoised.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.POINTER(abi.ProgressiveParams),
                                      C.POINTER(abi.DenoiseParams), dp, dp, dp, ip, C.POINTER(abi.Stats), C.c_void_p, C.c_void_p]
    fp = C.POINTER(abi.FilmParams)
    L.ptx_film_defaults.argtypes = [fp]
    L.ptx_film_weights.argtypes = [fp, dp, dp]
    L.ptx_scene_set_film.argtypes = [C.c_void_p, fp]
    L.ptx_scene_film.argtypes = [C.c_void_p, fp]
    L.ptx_film_resolve_ex_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptx_film_resolve_banded_ex_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, C.c_void_p, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_void_p, C.c_void_p]
    L.ptx_film_resolve_counts_ex_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, fp, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
    if hasattr(L, "ptx_scene_set_texture_image"):  # (a PTX_LIB built from an older tree, in an A/B, has none)
        imp = C.POINTER(abi.Image)
        L.ptx_scene_set_texture_image.argtypes = [C.c_void_p, C.c_int32, imp]
        L.ptx_scene_set_environment.argtypes = [C.c_void_p, imp, dp]
        L.ptx_scene_texture_image.argtypes = [C.c_void_p, C.c_int32, imp]
        L.ptx_scene_environment.argtypes = [C.c_void_p, imp, dp]
        L.ptx_texture_eval.argtypes = [C.c_void_p, C.c_int32, C.c_int64, dp, dp]
        L.ptx_environment_eval.argtypes = [C.c_void_p, C.c_int64, dp, dp]
    if hasattr(L, "ptx_scene_set_environment_sampling"):  # (likewise)
        L.ptx_scene_set_environment_sampling.argtypes = [C.c_void_p, C.c_int32]
        L.ptx_scene_environment_sampling.argtypes = [C.c_void_p, ip, dp]
        L.ptx_environment_distribution.argtypes = [C.c_void_p, dp, dp]
        L.ptx_environment_sample.argtypes = [C.c_void_p, C.c_int64, dp, dp, ip]
        L.ptx_environment_pdf.argtypes = [C.c_void_p, C.c_int64, dp, dp]
    if hasattr(L, "ptx_scene_set_sphere_light_sampling"):  # (likewise)
        L.ptx_scene_set_sphere_light_sampling.argtypes = [C.c_void_p, C.c_int32]
        L.ptx_scene_sphere_lights.argtypes = [C.c_void_p, ip, ip, dp]
        L.ptx_light_table.argtypes = [C.c_void_p, dp, dp]
        L.ptx_light_sample.argtypes = [C.c_void_p, C.c_int64, dp, dp, dp, ip]
        L.ptx_light_pdf.argtypes = [C.c_void_p, C.c_int64, dp, dp, dp]
    if hasattr(L, "ptx_walk_rays"):  # (likewise)
        L.ptx_walk_rays.argtypes = [C.c_void_p, C.c_int32, C.c_int64, dp, dp, dp, ip]
    if hasattr(L, "ptx_walk_next_leaf"):  # (likewise)
        L.ptx_walk_next_leaf.argtypes = [C.c_void_p, C.c_int32, C.c_int64, dp, dp, ip, dp, ip]
    if hasattr(L, "ptx_kernel_table"):  # (likewise)
        L.ptx_kernel_table.argtypes = [C.c_char_p, C.c_int64]
        L.ptx_scene_launched_kernels.argtypes = [C.c_void_p, ip, C.c_int32]
        L.ptx_scene_clear_launched_kernels.argtypes = [C.c_void_p]
    if hasattr(L, "ptx_scene_set_lens"):  # (likewise)
        L.ptx_scene_set_lens.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.ptx_scene_lens.argtypes = [C.c_void_p, dp, dp]
    if hasattr(L, "ptx_scene_set_camera_pose"):  # (likewise)
        L.ptx_scene_set_camera_pose.argtypes = [C.c_void_p, dp, dp, C.POINTER(abi.Camera)]
        L.ptx_scene_camera_pose.argtypes = [C.c_void_p, dp, dp, C.POINTER(abi.Camera)]
        L.ptx_camera_rays.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp]
    if hasattr(L, "ptx_render_temporal"):  # (likewise)
        tpp, tcp = C.POINTER(abi.TemporalParams), C.POINTER(abi.TemporalCamera)
        L.ptx_temporal_defaults.argtypes = [tpp]
        L.ptx_temporal_accumulate_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, tpp, C.c_int32, C.c_int32, tcp, tcp] + \
            [C.c_void_p] * 8 + [C.POINTER(C.c_int64), C.c_void_p]
        L.ptx_render_temporal.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), tpp, C.POINTER(abi.DenoiseParams), C.c_int32,
                                          C.c_int32, dp, dp, dp, C.POINTER(C.c_int64), C.POINTER(abi.Stats)]
        L.ptx_temporal_reset.argtypes = [C.c_void_p]
    if hasattr(L, "ptx_render_rays_device"):  # (likewise)
        rpp = C.POINTER(abi.RaysParams)
        L.ptx_render_rays_device.argtypes = [C.c_void_p, rpp, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(abi.Stats)]
        L.ptx_render_rays.argtypes = [C.c_void_p, rpp, C.c_int64, dp, dp, ip, dp, dp, C.POINTER(abi.Stats)]
    if hasattr(L, "ptx_scene_set_camera_projection"):  # (likewise)
        L.ptx_scene_set_camera_projection.argtypes = [C.c_void_p, C.c_int32]
        L.ptx_scene_camera_projection.argtypes = [C.c_void_p]
    if hasattr(L, "ptx_scene_set_camera_shutter"):  # (likewise)
        L.ptx_scene_set_camera_shutter.argtypes = [C.c_void_p, dp, dp, C.c_double]
        L.ptx_scene_camera_shutter.argtypes = [C.c_void_p, dp, dp, dp]
    if hasattr(L, "ptx_render_display"):  # (likewise)
        dpp = C.POINTER(abi.DisplayParams)
        L.ptx_display_defaults.argtypes = [dpp]
        L.ptx_display_check.argtypes = [dpp]
        L.ptx_display_pixel_bytes.argtypes = [C.c_int32]
        L.ptx_display_thresholds.argtypes = [dp]
        L.ptx_display_apply.argtypes = [dpp, C.c_int64, dp, C.c_void_p]
        L.ptx_display_image_device.argtypes = [C.c_int32, dpp, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptx_display_range_device.argtypes = [C.c_int32, dpp, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptx_image_pin_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.ptx_render_display.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), dpp, C.c_void_p, C.POINTER(abi.Stats), C.c_void_p,
                                         C.c_void_p]
        L.ptx_render_progressive_display.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.POINTER(abi.ProgressiveParams),
                                                     C.POINTER(abi.DenoiseParams), dpp, C.c_void_p, dp, ip, C.POINTER(abi.Stats),
                                                     C.c_void_p, C.c_void_p]
    _LIB = L
    return L


def last_error():
    return (lib().ptx_last_error() or b"").decode()


def _check(rc):
    if rc != 0:
        raise PtxError(f"ptx call failed ({rc}): {last_error()}")


def _dp(a):
    return a.ctypes.data_as(dp)


def _ip(a):
    return a.ctypes.data_as(ip)


def kernel_table():
    """ptx_kernel_table: the names of the instantiations of k_trace, k_shade_pool, k_bounce_carry and k_bounce the library is built
    with, in table order (the indices ptx_scene_launched_kernels reports).  Needs no device."""
    n = lib().ptx_kernel_table(None, 0)
    if n < 0:
        _check(n)
    buf = C.create_string_buffer(128 * n + 1)
    got = lib().ptx_kernel_table(buf, len(buf))
    if got < 0:
        _check(got)
    names = buf.value.decode().split("\n")[:-1]
    assert len(names) == got == n
    return names


def render_params(width, height, samples_per_pixel=1, max_bounces=8, band_rows=32, band_first=0, band_step=0,
                  count_work=False, time_kernels=False, passes_per_batch=0, n_gpus=0, asynchronous=False):
    p = abi.RenderParams()
    p.n_gpus = n_gpus
    p.flags = abi.PTX_RENDER_ASYNC if asynchronous else 0  # ptx_render_raw_device: queue the frame, do not wait for it
    p.width, p.height, p.samples_per_pixel, p.max_bounces = width, height, samples_per_pixel, max_bounces
    p.band_rows, p.band_first, p.band_step = band_rows, band_first, band_step
    p.count_work, p.time_kernels, p.passes_per_batch = int(count_work), int(time_kernels), passes_per_batch
    return p


def stats_dict(st):
    return {
        "samples": st.samples, "segments": st.segments, "nodes_tested": st.nodes_tested,
        "prims_tested": st.prims_tested, "floor_tested": st.floor_tested, "render_ms": st.render_ms,
        "kernel_ms": {n: st.kernel_ms[i] for i, n in enumerate(abi.PTX_KERNEL_NAMES)},
        "kernel_launches": {n: st.kernel_launches[i] for i, n in enumerate(abi.PTX_KERNEL_NAMES)},
        "tree_nodes": st.tree_nodes, "tree_depth": st.tree_depth, "tree_leaves": st.tree_leaves,
        "leaf_slots": st.leaf_slots, "build_ms": st.build_ms,
        "traversal_in_lds": bool(st.traversal_in_lds), "bvh_built_on_gpu": bool(st.bvh_built_on_gpu),
        "filter_undecided": st.filter_undecided, "filter_fallback_steps": st.filter_fallback_steps,
        "peer_copies": st.peer_copies, "staged_copies": st.staged_copies, "solo_launches": st.solo_launches,
        "carry_launches": st.carry_launches, "primary_lane_walks": st.primary_lane_walks, "lds_oct_launches": st.lds_oct_launches,
    }


class Scene:
    """A scene resident in HBM on one GPU (ptx_scene): BVH built on the host like Shape_tree.create."""

    def __init__(self, desc, device=0, keepalive=None):
        """desc: ctypes pointer to (or instance of) abi.SceneDesc."""
        self._keep = keepalive
        self.device = device
        ptr = desc if isinstance(desc, C.POINTER(abi.SceneDesc)) else C.pointer(desc)
        self._h = lib().ptx_scene_create(ptr, device)
        if not self._h:
            raise PtxError(f"ptx_scene_create failed: {last_error()}")

    @classmethod
    def _adopt(cls, handle, device, keepalive=None):
        s = cls.__new__(cls)
        s._keep, s.device, s._h = keepalive, device, handle
        return s

    def replicate(self, device):
        """ptx_scene_replicate: the same flattened scene uploaded to another device (no second BVH build)."""
        h = lib().ptx_scene_replicate(self._h, device)
        if not h:
            raise PtxError(f"ptx_scene_replicate failed: {last_error()}")
        return Scene._adopt(h, device, keepalive=self)

    def set_lighting(self, mode):
        """ptx_scene_set_lighting: abi.PTX_LIGHTING_REFERENCE / _PATH_ORDER / _SAMPLED or its name ("reference", "path-order",
        "sampled").  Sticky; every later render of this scene reads it."""
        _check(lib().ptx_scene_set_lighting(self._h, abi.lighting_mode(mode)))

    def lighting(self):
        """ptx_scene_lighting: (mode, light triangles, their total area); the last two are 0 until "sampled" has been set."""
        mode, n = C.c_int32(0), C.c_int32(0)
        area = C.c_double(0.0)
        _check(lib().ptx_scene_lighting(self._h, C.byref(mode), C.byref(n), C.byref(area)))
        return mode.value, n.value, area.value

    def set_film(self, order=None, radius=None, renormalise=False):
        """ptx_scene_set_film: the reconstruction filter Binomial.create ~order ~pixel_radius every later render of this scene films
        with, and whether border pixels are renormalised by the weight that stayed inside the image.  Sticky; set_film() restores
        the default (5, 1, no renormalisation)."""
        if order is None and radius is None:
            _check(lib().ptx_scene_set_film(self._h, None))
            return
        f = abi.film_params((order, radius, renormalise))
        _check(lib().ptx_scene_set_film(self._h, C.byref(f)))

    def film(self):
        """ptx_scene_film: (order, radius, renormalise)"""
        f = abi.FilmParams()
        _check(lib().ptx_scene_film(self._h, C.byref(f)))
        return f.order, f.pixel_radius, bool(f.flags & abi.PTX_FILM_RENORMALISE)

    def set_lens(self, radius, focus_distance):
        """ptx_scene_set_lens: a thin lens of this radius around the camera's origin, focused on the plane at focus_distance in
        front of it; every later render of this scene has its depth of field.  Sticky; radius 0 switches the lens off (the
        pinhole, bit for bit)."""
        _check(lib().ptx_scene_set_lens(self._h, float(radius), float(focus_distance)))

    def lens(self):
        """ptx_scene_lens: (radius, focus_distance); radius 0.0 = off"""
        r, f = C.c_double(), C.c_double()
        _check(lib().ptx_scene_lens(self._h, C.byref(r), C.byref(f)))
        return r.value, f.value

    def set_camera_pose(self, origin=None, rotation=None, view=None):
        """ptx_scene_set_camera_pose: the camera stands at `origin` (3 doubles) of the scene's space, turned by `rotation` (3 x 3,
        row-major, posed camera space -> scene space) and, with `view` = (lower_left_x, lower_left_y, view_x, view_y), looks through
        a frustum of its own; every later render of this scene is taken from there, with no rebuild.  Sticky.  origin and rotation
        go together; view alone keeps origin 0 and the identity.  All three None switch the pose off (the scene's own camera and
        its own launches, bit for bit); anything else, the identity included, switches it on."""
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        r = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        v = None if view is None else abi.Camera(*(float(c) for c in view))
        _check(lib().ptx_scene_set_camera_pose(self._h, None if o is None else _dp(o), None if r is None else _dp(r),
                                               None if v is None else C.byref(v)))

    @property
    def camera_pose(self):
        """ptx_scene_camera_pose: None while the pose is off, else (origin (3,), rotation (3, 3), view) with view the four fields in
        effect (the pose's own, else the scene's)"""
        o, r, v = np.zeros(3), np.zeros(9), abi.Camera()
        rc = lib().ptx_scene_camera_pose(self._h, _dp(o), _dp(r), C.byref(v))
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        return o, r.reshape(3, 3), (v.lower_left_x, v.lower_left_y, v.view_x, v.view_y)

    def set_camera_projection(self, projection):
        """ptx_scene_set_camera_projection: "perspective" (the pinhole, the state of every scene that never called this) or
        "latlong" -- a 360-degree panorama in the environment map's (u, v) convention, taken from the pose's origin (the scene's
        own while the pose is off) -- or the abi.PTX_PROJECTION_* value.  Sticky.  Refused while a lens is on."""
        _check(lib().ptx_scene_set_camera_projection(self._h, abi.projection_kind(projection)))

    @property
    def camera_projection(self):
        """ptx_scene_camera_projection: "perspective" or "latlong" """
        rc = lib().ptx_scene_camera_projection(self._h)
        if rc < 0:
            _check(rc)
        return abi.PTX_PROJECTION_NAMES[rc]

    def set_camera_shutter(self, translation=None, axis=None, angle=0.0):
        """ptx_scene_set_camera_shutter: while a frame is exposed the camera moves from the pose's origin by `translation` (3 doubles,
        scene space) and turns by `angle` radians about the unit vector `axis` (scene space), at constant velocity: every later
        render of this scene is blurred by that motion (camera_shutter_between gives the three from two poses).  Sticky.
        translation and axis go together; None (or no argument) switches the shutter off -- the scene's own launches, bit for bit;
        anything else, a zero motion included, switches it on."""
        if translation is None and axis is None:
            _check(lib().ptx_scene_set_camera_shutter(self._h, None, None, float(angle)))
            return
        t = None if translation is None else np.ascontiguousarray(translation, dtype=np.float64).reshape(3)
        k = None if axis is None else np.ascontiguousarray(axis, dtype=np.float64).reshape(3)
        _check(lib().ptx_scene_set_camera_shutter(self._h, None if t is None else _dp(t), None if k is None else _dp(k), float(angle)))

    @property
    def camera_shutter(self):
        """ptx_scene_camera_shutter: None while the shutter is off, else (translation (3,), axis (3,), angle)"""
        t, k, a = np.zeros(3), np.zeros(3), C.c_double()
        rc = lib().ptx_scene_camera_shutter(self._h, _dp(t), _dp(k), C.cast(C.byref(a), dp))
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        return t, k, a.value

    def camera_rays(self, width, height, samples_per_pixel, max_bounces, xs, ys, passes):
        """ptx_camera_rays (diagnostic): (origins (n, 3), directions (n, 3)) of the camera rays this scene's renders launch for the
        (x, y, pass) triples -- under its pose, its lens, or neither"""
        xs = np.ascontiguousarray(xs, dtype=np.int32)
        ys = np.ascontiguousarray(ys, dtype=np.int32)
        passes = np.ascontiguousarray(passes, dtype=np.int32)
        p = render_params(width, height, samples_per_pixel, max_bounces)
        o, d = np.zeros((len(xs), 3)), np.zeros((len(xs), 3))
        _check(lib().ptx_camera_rays(self._h, C.byref(p), len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(o), _dp(d)))
        return o, d

    def set_texture_image(self, index, image, bilinear=False, repeat=(False, False)):
        """ptx_scene_set_texture_image: from now on every material that points at entry `index` of the scene's texture table
        evaluates `image`, an (H, W, 3) array of linear binary64 texels (row 0 is v = 0; the library copies it); None restores the
        descriptor's texture.  bilinear: interpolate the four nearest texels instead of taking the one (u, v) falls into;
        repeat = (in u, in v): wrap around instead of clamping to the edge.  Sticky; every later render of this scene reads it."""
        if image is None:
            _check(lib().ptx_scene_set_texture_image(self._h, int(index), None))
            return
        flags = ((abi.PTX_IMAGE_BILINEAR if bilinear else 0) | (abi.PTX_IMAGE_REPEAT_U if repeat[0] else 0)
                 | (abi.PTX_IMAGE_REPEAT_V if repeat[1] else 0))
        img, keep = abi.image(image, flags)
        _check(lib().ptx_scene_set_texture_image(self._h, int(index), C.byref(img)))
        del keep

    def texture_image(self, index):
        """ptx_scene_texture_image: (width, height, flags) of the image on entry `index`, or None"""
        out = abi.Image()
        _check(lib().ptx_scene_texture_image(self._h, int(index), C.byref(out)))
        return (out.width, out.height, out.flags) if out.width else None

    def set_environment(self, image, rotation=None, bilinear=True):
        """ptx_scene_set_environment: a ray that leaves the scene returns the colour `image` (an (H, W, 3) array, latitude-longitude:
        u runs once around the y axis, v from -y (row 0) to +y) holds in its direction; rotation: the row-major 3 x 3 matrix from
        camera space to the environment's space (None = identity).  None restores the descriptor's background.  Sticky."""
        if image is None:
            _check(lib().ptx_scene_set_environment(self._h, None, None))
            return
        img, keep = abi.image(image, abi.PTX_IMAGE_BILINEAR if bilinear else 0)
        rot = None
        if rotation is not None:
            rot = np.ascontiguousarray(rotation, dtype=np.float64).reshape(-1)
            if rot.size != 9:
                raise ValueError("rotation must be a 3 x 3 matrix")
        _check(lib().ptx_scene_set_environment(self._h, C.byref(img), _dp(rot) if rot is not None else None))
        del keep

    def environment(self):
        """ptx_scene_environment: ((width, height, flags), the 3 x 3 rotation), or None"""
        out = abi.Image()
        rot = np.zeros(9)
        _check(lib().ptx_scene_environment(self._h, C.byref(out), _dp(rot)))
        return ((out.width, out.height, out.flags), rot.reshape(3, 3)) if out.width else None

    def set_environment_sampling(self, on=True):
        """ptx_scene_set_environment_sampling: in "sampled" lighting a Diffuse scatter also draws directions from the environment
        image, in proportion to luminance x sin(theta) per texel (and "sampled" then accepts a scene without emissive triangles).
        Needs an environment whose rotation is orthonormal and whose total weight is positive.  Sticky."""
        _check(lib().ptx_scene_set_environment_sampling(self._h, 1 if on else 0))

    def environment_sampling(self):
        """ptx_scene_environment_sampling: (on, the density's total weight T; 0.0 while off)"""
        on = C.c_int32(0)
        total = C.c_double(0.0)
        _check(lib().ptx_scene_environment_sampling(self._h, C.byref(on), C.byref(total)))
        return bool(on.value), total.value

    def environment_distribution(self):
        """ptx_environment_distribution (host only, sampling must be on): (the running sums of the rows m (H,), the running sums
        inside every row c (H, W))"""
        env = self.environment()
        if env is None:
            raise PtxError("environment_distribution: the scene has no environment")
        w, h = env[0][0], env[0][1]
        m, c = np.zeros(h), np.zeros((h, w))
        _check(lib().ptx_environment_distribution(self._h, _dp(m), _dp(c)))
        return m, c

    def environment_sample(self, ab):
        """ptx_environment_sample: the device's own sampling function on the (n, 2) pairs ab -> (unit directions (n, 3), the texels
        drawn (n, 2) as (ix, iy))"""
        ab = np.ascontiguousarray(ab, dtype=np.float64).reshape(-1, 2)
        dirs, texel = np.zeros((len(ab), 3)), np.zeros((len(ab), 2), dtype=np.int32)
        _check(lib().ptx_environment_sample(self._h, len(ab), _dp(ab), _dp(dirs), _ip(texel)))
        return dirs, texel

    def environment_pdf(self, directions):
        """ptx_environment_pdf: the density per solid angle with which environment sampling draws each of the (n, 3) directions"""
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(len(d))
        _check(lib().ptx_environment_pdf(self._h, len(d), _dp(d), _dp(out)))
        return out

    def set_sphere_light_sampling(self, on=True):
        """ptx_scene_set_sphere_light_sampling: in "sampled" lighting the light half also draws directions towards the scene's
        emissive tree spheres, uniformly over the cone each spans from the hit (and "sampled" then accepts a scene without emissive
        triangles).  Needs 1 .. 64 emissive spheres.  Sticky."""
        _check(lib().ptx_scene_set_sphere_light_sampling(self._h, 1 if on else 0))

    def sphere_lights(self):
        """ptx_scene_sphere_lights: (on, the number of sphere lights, W_total = the joined light table's last running sum; 0 and
        0.0 while off)"""
        on, n = C.c_int32(0), C.c_int32(0)
        total = C.c_double(0.0)
        _check(lib().ptx_scene_sphere_lights(self._h, C.byref(on), C.byref(n), C.byref(total)))
        return bool(on.value), n.value, total.value

    def light_table(self):
        """ptx_light_table (host only): (the light triangles' records (n, 14) {a, b, c, normal, A, cum}, the sphere lights'
        records (n, 8) {c, r, r2, W, cum, 0})"""
        n_tri = self.lighting()[1]
        n_sph = self.sphere_lights()[1]
        tri, sph = np.zeros((n_tri, 14)), np.zeros((n_sph, 8))
        _check(lib().ptx_light_table(self._h, _dp(tri) if n_tri else None, _dp(sph) if n_sph else None))
        return tri, sph

    def light_sample(self, points, uv):
        """ptx_light_sample: the shade step's own light-half sampling function, triangles and spheres together, at the (n, 3) points
        on the (n, 2) sampler pairs uv -> (world-space unit directions (n, 3), the joined table's entry drawn (n,))"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        if len(p) != len(uv):
            raise ValueError("points and uv must have the same length")
        dirs, index = np.zeros((len(p), 3)), np.zeros(len(p), dtype=np.int32)
        _check(lib().ptx_light_sample(self._h, len(p), _dp(p), _dp(uv), _dp(dirs), _ip(index)))
        return dirs, index

    def light_pdf(self, points, directions):
        """ptx_light_pdf: the light half's density per solid angle of each of the (n, 3) world directions at the (n, 3) points"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if len(p) != len(d):
            raise ValueError("points and directions must have the same length")
        out = np.zeros(len(p))
        _check(lib().ptx_light_pdf(self._h, len(p), _dp(p), _dp(d), _dp(out)))
        return out

    def texture_eval(self, index, uv):
        """ptx_texture_eval: entry `index` of the texture table (its image, or its solid / checker texture) evaluated on the device
        at the (n, 2) texture coordinates uv -> (n, 3)"""
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        out = np.zeros((len(uv), 3))
        _check(lib().ptx_texture_eval(self._h, int(index), len(uv), _dp(uv), _dp(out)))
        return out

    def environment_eval(self, directions):
        """ptx_environment_eval: what a ray leaving the scene in each of the (n, 3) directions returns -> (n, 3)"""
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(d), 3))
        _check(lib().ptx_environment_eval(self._h, len(d), _dp(d), _dp(out)))
        return out

    def stats(self):
        st = abi.Stats()
        _check(lib().ptx_scene_stats(self._h, C.byref(st)))
        return stats_dict(st)

    def tile_list_stats(self):
        """ptx_tile_list_stats: the camera tile lists of the last render on this handle"""
        out = abi.TileListStats()
        _check(lib().ptx_tile_list_stats(self._h, out))
        return dict(zip(abi.TILE_LIST_STATS, out))

    def tree(self):
        st = self.stats()
        n, slots = st["tree_nodes"], st["leaf_slots"]
        bbox = np.zeros((n, 6))
        info = np.zeros((n, 4), dtype=np.int32)
        order = np.zeros(max(slots, 1), dtype=np.int32)
        got = lib().ptx_scene_tree(self._h, _dp(bbox), _ip(info), n, _ip(order), slots)
        assert got == n
        return bbox, info, order[:slots]

    def render(self, width, height, samples_per_pixel, max_bounces, progress=None, out=None, **kw):
        """ptx_render: post-gamma f64 framebuffer (H, W, 3) on the host + stats.  `out`: the caller's (H, W, 3) float64
        C-contiguous array to fill (the reference renders into the Bimage it was given, render_command.ml:65)."""
        p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
        if out is None:
            out = np.zeros((height, width, 3))
        elif out.shape != (height, width, 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous float64 array of shape (height, width, 3)")
        st = abi.Stats()
        cb = PROGRESS_FN(lambda user, n: progress(n)) if progress else None
        _check(lib().ptx_render(self._h, C.byref(p), _dp(out), C.byref(st), C.cast(cb, C.c_void_p) if cb else None, None))
        return out, stats_dict(st)

    def pin_image(self, image):
        """ptx_image_pin: page-lock the caller's (H, W, 3) float64 image for as long as renders go into it (one DMA per frame
        instead of a staged copy).  The image must stay alive until unpin_image() / close()."""
        if image.dtype != np.float64 or not image.flags["C_CONTIGUOUS"]:
            raise ValueError("image must be a C-contiguous float64 array")
        _check(lib().ptx_image_pin(self._h, _dp(image), image.size))
        self._pinned_image = image  # keeps it mapped while the registration exists

    def unpin_image(self):
        _check(lib().ptx_image_unpin(self._h))
        self._pinned_image = None

    def image_pin_bytes(self, image):
        """ptx_image_pin_bytes: pin_image for a display image (any C-contiguous uint8 or float32 array).  One pinned image per
        scene, of either kind; unpin_image() releases it."""
        if image.dtype not in (np.uint8, np.float32) or not image.flags["C_CONTIGUOUS"]:
            raise ValueError("image must be a C-contiguous uint8 or float32 array")
        _check(lib().ptx_image_pin_bytes(self._h, C.c_void_p(image.ctypes.data), image.nbytes))
        self._pinned_image = image  # keeps it mapped while the registration exists

    def render_display(self, width, height, samples_per_pixel, max_bounces, format="rgb8", transfer="reference", tone="none",
                       exposure=1.0, progress=None, out=None, **kw):
        """ptx_render_display: render() whose image comes back as display pixels -- a uint8 or float32 array of shape (H, W, 3 or
        4), bit for bit display_apply(render()'s image) -- converted on the device and copied as what it is.  `out`: the caller's
        array of that shape and dtype to fill.  Returns (pixels, stats)."""
        d = abi.display_params(None, format, transfer, tone, exposure)
        out = _display_arg(out, width, height, d.format, "out")
        p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
        st = abi.Stats()
        cb = PROGRESS_FN(lambda user, n: progress(n)) if progress else None
        _check(lib().ptx_render_display(self._h, C.byref(p), C.byref(d), C.c_void_p(out.ctypes.data), C.byref(st),
                                        C.cast(cb, C.c_void_p) if cb else None, None))
        return out, stats_dict(st)

    def render_progressive_display(self, width, height, samples_per_pixel, max_bounces, passes_per_update, denoise=None,
                                   format="rgb8", transfer="reference", tone="none", exposure=1.0, on_update=None,
                                   target_rel_err=0.0, want_error=True, out=None, err_out=None, **kw):
        """ptx_render_progressive_display: render_progressive -- with `denoise` (True for the defaults, a dict or an
        abi.DenoiseParams) render_denoised -- whose updates are display pixels.  on_update(passes_done, rel_err, pixels, err) sees
        the (H, W, 3 or 4) display image of the update and the f64 per-pixel error (None without want_error).  Returns
        (pixels, err, passes_done, stats)."""
        d = abi.display_params(None, format, transfer, tone, exposure)
        dn = None if denoise is None or denoise is False else denoise_params(None if denoise is True else denoise)
        want_error = bool(want_error) or dn is not None
        out = _display_arg(out, width, height, d.format, "out")
        err_out = _image_arg(err_out, width, height, "err_out") if want_error else None
        p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
        pp = abi.ProgressiveParams()
        pp.passes_per_update, pp.want_error, pp.target_rel_err = int(passes_per_update), int(want_error), float(target_rel_err)
        raised = []

        def trampoline(user, passes_done, rel_err, pixels, err):
            if raised:
                return 1
            try:
                return 1 if on_update(passes_done, rel_err, out, err_out) else 0
            except BaseException as e:  # noqa: BLE001 -- carried across the C frames, raised again below
                raised.append(e)
                return 1

        cb = abi.UPDATE_DISPLAY_FN(trampoline) if on_update is not None else None
        done = C.c_int32(0)
        st = abi.Stats()
        rc = lib().ptx_render_progressive_display(self._h, C.byref(p), C.byref(pp), C.byref(dn) if dn is not None else None,
                                                  C.byref(d), C.c_void_p(out.ctypes.data),
                                                  _dp(err_out) if err_out is not None else None, C.byref(done), C.byref(st),
                                                  C.cast(cb, C.c_void_p) if cb else None, None)
        if raised:
            raise raised[0]
        _check(rc)
        return out, err_out, done.value, stats_dict(st)

    def render_raw_device(self, params, d_raw_ptr, stream=None):
        """ptx_render_raw_device: raw per-pixel sums for this rank's rows into DEVICE memory."""
        st = abi.Stats()
        _check(lib().ptx_render_raw_device(self._h, C.byref(params), C.c_void_p(d_raw_ptr),
                                           C.c_void_p(stream) if stream else None, C.byref(st)))
        return stats_dict(st)

    def render_passes_device(self, params, pass_first, pass_count, d_raw_ptr, d_sq_ptr=None, stream=None):
        """ptx_render_passes_device: passes [pass_first, pass_first + pass_count) of the frame of params.samples_per_pixel
        passes ADDED to this rank's raw sums in DEVICE memory (never zeroed), and their squares to d_sq_ptr if given."""
        st = abi.Stats()
        _check(lib().ptx_render_passes_device(self._h, C.byref(params), int(pass_first), int(pass_count), C.c_void_p(d_raw_ptr),
                                              C.c_void_p(d_sq_ptr) if d_sq_ptr else None,
                                              C.c_void_p(stream) if stream else None, C.byref(st)))
        return stats_dict(st)

    def render_progressive(self, width, height, samples_per_pixel, max_bounces, passes_per_update, on_update=None,
                           target_rel_err=0.0, want_error=True, out=None, err_out=None, **kw):
        """ptx_render_progressive: the frame as a sequence of updates, one after every `passes_per_update` passes and one after
        the last.  on_update(passes_done, rel_err, rgb, err) is called after each with the (H, W, 3) image filmed from the
        passes done so far and its per-pixel standard error (None without want_error); a truthy return stops the render, and
        so does rel_err <= target_rel_err when the target is > 0.  An exception raised by on_update stops the render and is
        raised again here.  Returns (rgb, err, passes_done, stats); rgb is the image of the last update."""
        if int(passes_per_update) < 1:
            raise ValueError("passes_per_update must be >= 1")
        if not float(target_rel_err) >= 0.0:
            raise ValueError("target_rel_err must be >= 0")
        if (float(target_rel_err) > 0.0 or err_out is not None) and not want_error:
            raise ValueError("target_rel_err and err_out need want_error")
        if kw.get("n_gpus", 0) > 1:
            raise ValueError("progressive rendering runs on one GPU")
        out = _image_arg(out, width, height, "out")
        err_out = _image_arg(err_out, width, height, "err_out") if want_error else None
        p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
        pp = abi.ProgressiveParams()
        pp.passes_per_update, pp.want_error, pp.target_rel_err = int(passes_per_update), int(bool(want_error)), float(target_rel_err)
        raised = []

        def trampoline(user, passes_done, rel_err, rgb, err):
            if raised:
                return 1
            try:
                return 1 if on_update(passes_done, rel_err, out, err_out) else 0
            except BaseException as e:  # noqa: BLE001 -- carried across the C frames, raised again below
                raised.append(e)
                return 1

        cb = UPDATE_FN(trampoline) if on_update is not None else None
        done = C.c_int32(0)
        st = abi.Stats()
        rc = lib().ptx_render_progressive(self._h, C.byref(p), C.byref(pp), _dp(out),
                                          _dp(err_out) if err_out is not None else None, C.byref(done), C.byref(st),
                                          C.cast(cb, C.c_void_p) if cb else None, None)
        if raised:
            raise raised[0]
        _check(rc)
        return out, err_out, done.value, stats_dict(st)

    def render_pixels_device(self, params, pass_first, pass_count, d_pixels_ptr, n_pixels, d_raw_ptr, d_sq_ptr=None,
                             stream=None):
        """ptx_render_pixels_device: passes [pass_first, pass_first + pass_count) of the frame of params.samples_per_pixel passes
        for the n_pixels DISTINCT indices y * W + x of the DEVICE list d_pixels_ptr (int32), ADDED to the whole-image raw sums
        (and their squares to d_sq_ptr if given); unlisted pixels are untouched."""
        if int(n_pixels) < 0:
            raise ValueError("n_pixels must be >= 0")
        st = abi.Stats()
        _check(lib().ptx_render_pixels_device(self._h, C.byref(params), int(pass_first), int(pass_count),
                                              C.c_void_p(d_pixels_ptr) if d_pixels_ptr else None, int(n_pixels),
                                              C.c_void_p(d_raw_ptr), C.c_void_p(d_sq_ptr) if d_sq_ptr else None,
                                              C.c_void_p(stream) if stream else None, C.byref(st)))
        return stats_dict(st)

    def render_adaptive(self, width, height, spp, depth, target_rel_err, min_passes=8, passes_per_round=8,
                        radiance_floor=1e-3, on_round=None, out=None, err_out=None, passes_out=None, **kw):
        """ptx_render_adaptive: round 1 gives every pixel min(min_passes, spp) passes, every later round gives the pixels that have
        not converged (per-pixel standard error e <= target_rel_err * max(|mean|, radiance_floor)) passes_per_round more, up to
        spp.  on_round(round, passes_done, active_next, samples, rel_err, rgb, err, passes) is called after each with the (H, W, 3)
        image, its per-pixel error and the (H, W) int32 pass counts; a truthy return stops the render.  An exception raised by
        on_round stops the render and is raised again here.  Returns (rgb, err, passes, stats) of the last round."""
        if int(min_passes) < 2:
            raise ValueError("min_passes must be >= 2")
        if int(passes_per_round) < 1:
            raise ValueError("passes_per_round must be >= 1")
        if not float(target_rel_err) >= 0.0:
            raise ValueError("target_rel_err must be >= 0")
        if not float(radiance_floor) >= 0.0:
            raise ValueError("radiance_floor must be >= 0")
        if kw.get("n_gpus", 0) > 1 or kw.get("band_step", 0) > 1:
            raise ValueError("adaptive rendering runs on one GPU over the whole image")
        out = _image_arg(out, width, height, "out")
        err_out = _image_arg(err_out, width, height, "err_out")
        if passes_out is None:
            passes_out = np.zeros((height, width), dtype=np.int32)
        elif passes_out.shape != (height, width) or passes_out.dtype != np.int32 or not passes_out.flags["C_CONTIGUOUS"]:
            raise ValueError("passes_out must be a C-contiguous int32 array of shape (height, width)")
        p = render_params(width, height, spp, depth, **kw)
        ap = abi.AdaptiveParams()
        ap.min_passes, ap.passes_per_round = int(min_passes), int(passes_per_round)
        ap.target_rel_err, ap.radiance_floor = float(target_rel_err), float(radiance_floor)
        raised = []

        def trampoline(user, rnd, passes_done, active_next, samples, rel_err, rgb, err, passes):
            if raised:
                return 1
            try:
                return 1 if on_round(rnd, passes_done, active_next, samples, rel_err, out, err_out, passes_out) else 0
            except BaseException as e:  # noqa: BLE001 -- carried across the C frames, raised again below
                raised.append(e)
                return 1

        cb = ROUND_FN(trampoline) if on_round is not None else None
        st = abi.Stats()
        rc = lib().ptx_render_adaptive(self._h, C.byref(p), C.byref(ap), _dp(out), _dp(err_out), _ip(passes_out), C.byref(st),
                                       C.cast(cb, C.c_void_p) if cb else None, None)
        if raised:
            raise raised[0]
        _check(rc)
        return out, err_out, passes_out, stats_dict(st)

    def render_features_device(self, params, pass_first, pass_count, d_feat_ptr, stream=None):
        """ptx_render_features_device: the first-hit feature records (albedo, normal, depth, hits: 8 doubles per pixel) of passes
        [pass_first, pass_first + pass_count) of the frame of params.samples_per_pixel passes ADDED to the whole-image feature
        sums in DEVICE memory (never zeroed), in pass order."""
        if getattr(params, "n_gpus", 0) > 1 or getattr(params, "band_step", 0) > 1:
            raise ValueError("a feature pass runs on one GPU over the whole image")
        st = abi.Stats()
        _check(lib().ptx_render_features_device(self._h, C.byref(params), int(pass_first), int(pass_count), C.c_void_p(d_feat_ptr),
                                                C.c_void_p(stream) if stream else None, C.byref(st)))
        return stats_dict(st)

    def render_denoised(self, width, height, samples_per_pixel, max_bounces, passes_per_update, denoise=None, on_update=None,
                        target_rel_err=0.0, out=None, err_out=None, feat_out=None, **kw):
        """ptx_render_denoised: render_progressive whose updates show the image filtered by the variance-guided a-trous denoiser
        (`denoise`: an abi.DenoiseParams, a dict of its fields over the defaults, or None for denoise_defaults()).  The error is
        always kept; on_update(passes_done, rel_err, rgb, err) sees the denoised image and the un-denoised per-pixel standard
        error.  feat_out ((H, W, 8) float64, or True to have one made) receives the first-hit feature means.  Returns
        (rgb, err, feat or None, passes_done, stats)."""
        if int(passes_per_update) < 2:
            raise ValueError("passes_per_update must be >= 2")
        if int(samples_per_pixel) < 2:
            raise ValueError("samples_per_pixel must be >= 2")
        if not float(target_rel_err) >= 0.0:
            raise ValueError("target_rel_err must be >= 0")
        if kw.get("n_gpus", 0) > 1 or kw.get("band_step", 0) > 1:
            raise ValueError("denoised rendering runs on one GPU over the whole image")
        dn = denoise_params(denoise)
        out = _image_arg(out, width, height, "out")
        err_out = _image_arg(err_out, width, height, "err_out")
        if feat_out is True:
            feat_out = np.zeros((height, width, abi.PTX_FEATURE_DOUBLES))
        elif feat_out is not None and (getattr(feat_out, "shape", None) != (height, width, abi.PTX_FEATURE_DOUBLES)
                                       or feat_out.dtype != np.float64 or not feat_out.flags["C_CONTIGUOUS"]):
            raise ValueError("feat_out must be a C-contiguous float64 array of shape (height, width, 8)")
        p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
        pp = abi.ProgressiveParams()
        pp.passes_per_update, pp.want_error, pp.target_rel_err = int(passes_per_update), 1, float(target_rel_err)
        raised = []

        def trampoline(user, passes_done, rel_err, rgb, err):
            if raised:
                return 1
            try:
                return 1 if on_update(passes_done, rel_err, out, err_out) else 0
            except BaseException as e:  # noqa: BLE001 -- carried across the C frames, raised again below
                raised.append(e)
                return 1

        cb = UPDATE_FN(trampoline) if on_update is not None else None
        done = C.c_int32(0)
        st = abi.Stats()
        rc = lib().ptx_render_denoised(self._h, C.byref(p), C.byref(pp), C.byref(dn), _dp(out), _dp(err_out),
                                       _dp(feat_out) if feat_out is not None else None, C.byref(done), C.byref(st),
                                       C.cast(cb, C.c_void_p) if cb else None, None)
        if raised:
            raise raised[0]
        _check(rc)
        return out, err_out, feat_out, done.value, stats_dict(st)

    def render_temporal(self, width, height, samples_per_pixel, max_bounces, pass_first, pass_count, temporal=None, denoise=None,
                        want_err=False, want_motion=False, out=None, **kw):
        """ptx_render_temporal: one frame of a sequence -- passes [pass_first, pass_first + pass_count) of the sequence's
        `samples_per_pixel`, accumulated onto the history this handle keeps by reprojecting every first hit through the last
        frame's camera and this one's (the scene's pose).  Advance pass_first from frame to frame: the same slice under a still
        camera adds the same samples again.  `temporal`: an abi.TemporalParams, a dict over the defaults, or None;
        `denoise`: None for no spatial filter, else as render_denoised takes it (True: the defaults).
        Returns (rgb, err or None, motion or None, history_pixels, stats)."""
        if int(pass_count) < 2:
            raise ValueError("pass_count must be >= 2")
        if kw.get("n_gpus", 0) > 1 or kw.get("band_step", 0) > 1:
            raise ValueError("temporal rendering runs on one GPU over the whole image")
        tp = temporal_params(temporal)
        dn = None if denoise is None or denoise is False else denoise_params(None if denoise is True else denoise)
        out = _image_arg(out, width, height, "out")
        err = np.zeros((height, width, 3)) if want_err else None
        motion = np.zeros((height, width, 3)) if want_motion else None
        p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
        took = C.c_int64(0)
        st = abi.Stats()
        _check(lib().ptx_render_temporal(self._h, C.byref(p), C.byref(tp), C.byref(dn) if dn is not None else None, int(pass_first),
                                         int(pass_count), _dp(out), _dp(err) if want_err else None,
                                         _dp(motion) if want_motion else None, C.byref(took), C.byref(st)))
        return out, err, motion, took.value, stats_dict(st)

    def temporal_reset(self):
        """ptx_temporal_reset: drops the frame history this handle keeps (after a change of lighting, textures or environment)"""
        _check(lib().ptx_temporal_reset(self._h))

    def trace_samples(self, width, height, samples_per_pixel, max_bounces, xs, ys, passes, count_work=False):
        xs = np.ascontiguousarray(xs, dtype=np.int32)
        ys = np.ascontiguousarray(ys, dtype=np.int32)
        passes = np.ascontiguousarray(passes, dtype=np.int32)
        p = render_params(width, height, samples_per_pixel, max_bounces, count_work=count_work)
        out = np.zeros((len(xs), 3))
        st = abi.Stats()
        _check(lib().ptx_trace_samples(self._h, C.byref(p), len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(out), C.byref(st)))
        return out, stats_dict(st)

    def render_rays(self, origins, directions, offsets=None, max_bounces=8, rays_per_bin=1, normalize=False, want_sq=False,
                    count_work=False):
        """ptx_render_rays: the radiance along the caller's rays -- origins and directions (n, 3), unit directions unless
        `normalize` -- under this scene's shading state, ray i's path reading the sampler at offsets[i] (None: i).  Returns
        (sums (n / rays_per_bin, 3), squares or None, stats): bin b is the left fold of rays [b m, (b + 1) m) in ray order onto
        zeros, so rays_per_bin = 1 gives the per-ray radiance."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"origins {o.shape} and directions {d.shape} differ in shape")
        n = o.shape[0]
        off = None
        if offsets is not None:
            off64 = np.asarray(offsets, dtype=np.int64).reshape(-1)
            if off64.shape[0] != n:
                raise ValueError(f"{off64.shape[0]} offsets for {n} rays")
            if n and (off64.min() < -2**31 or off64.max() >= 2**31):
                raise ValueError("a sampler offset does not fit 32 bits")
            off = np.ascontiguousarray(off64, dtype=np.int32)
        p = abi.rays_params(max_bounces, rays_per_bin, normalize, count_work)
        bins = n // p.rays_per_bin if p.rays_per_bin >= 1 else 0
        out = np.zeros((bins, 3))
        sq = np.zeros((bins, 3)) if want_sq else None
        st = abi.Stats()
        _check(lib().ptx_render_rays(self._h, C.byref(p), n, _dp(o), _dp(d), None if off is None else _ip(off), _dp(out),
                                     None if sq is None else _dp(sq), C.byref(st)))
        return out, sq, stats_dict(st)

    def render_rays_device(self, n, d_origins_ptr, d_directions_ptr, d_sum_ptr, d_offsets_ptr=None, d_sq_ptr=None, max_bounces=8,
                           rays_per_bin=1, normalize=False, count_work=False, stream=None):
        """ptx_render_rays_device: the same on DEVICE pointers of this scene's device (origins and directions n x 3 doubles,
        offsets n int32 or None), ADDED to the (n / rays_per_bin) x 3 sums at d_sum_ptr (never zeroed), the squares to d_sq_ptr if
        given; queued on `stream` and waited for."""
        p = abi.rays_params(max_bounces, rays_per_bin, normalize, count_work)
        st = abi.Stats()
        _check(lib().ptx_render_rays_device(self._h, C.byref(p), int(n), C.c_void_p(d_origins_ptr), C.c_void_p(d_directions_ptr),
                                            C.c_void_p(d_offsets_ptr) if d_offsets_ptr else None, C.c_void_p(d_sum_ptr),
                                            C.c_void_p(d_sq_ptr) if d_sq_ptr else None, C.c_void_p(stream) if stream else None,
                                            C.byref(st)))
        return stats_dict(st)

    def intersect_rays(self, origins, directions):
        o = np.ascontiguousarray(origins, dtype=np.float64)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        n = o.shape[0]
        t = np.zeros(n)
        prim = np.zeros(n, dtype=np.int32)
        st = abi.Stats()
        _check(lib().ptx_intersect_rays(self._h, n, _dp(o), _dp(d), _dp(t), _ip(prim), C.byref(st)))
        return t, prim, stats_dict(st)

    def walk_rays(self, walk, origins, directions):
        """ptx_walk_rays: one of the bounce kernels' walks (abi.PTX_WALK_*) on explicit rays -> (t, prim) as intersect_rays gives
        them.  PtxError for a walk the scene cannot take, and for a PACKET or _ZERO walk with an origin that is not +0.0."""
        o = np.ascontiguousarray(origins, dtype=np.float64)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        n = o.shape[0]
        t = np.zeros(n)
        prim = np.zeros(n, dtype=np.int32)
        _check(lib().ptx_walk_rays(self._h, int(walk), n, _dp(o), _dp(d), _dp(t), _ip(prim)))
        return t, prim

    def walk_next_leaf(self, walk, origins, directions, nodes, t_max):
        """ptx_walk_next_leaf: per (ray, node of tree()'s numbering, closest hit so far) the first slot of the next leaf whose box
        test the walk (abi.PTX_NEXT_LEAF_WALKS) passes, starting with the visit of the node; -1 when the walk runs off the tree."""
        o = np.ascontiguousarray(origins, dtype=np.float64)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        k = np.ascontiguousarray(nodes, dtype=np.int32)
        tm = np.ascontiguousarray(t_max, dtype=np.float64)
        n = o.shape[0]
        if d.shape[0] != n or k.shape[0] != n or tm.shape[0] != n:
            raise ValueError("origins, directions, nodes and t_max must have one entry per triple")
        leaf = np.zeros(n, dtype=np.int32)
        _check(lib().ptx_walk_next_leaf(self._h, int(walk), n, _dp(o), _dp(d), _ip(k), _dp(tm), _ip(leaf)))
        return leaf

    def launched_kernels(self):
        """ptx_scene_launched_kernels: the names (kernel_table()'s) of the hot kernels' instantiations launched on this handle since
        it was created or since clear_launched_kernels(), in table order"""
        names = kernel_table()
        idx = np.zeros(len(names), dtype=np.int32)
        n = lib().ptx_scene_launched_kernels(self._h, _ip(idx), len(idx))
        if n < 0:
            _check(n)
        return [names[i] for i in idx[:n]]

    def clear_launched_kernels(self):
        _check(lib().ptx_scene_clear_launched_kernels(self._h))

    def ppm_render(self, params, lights, callback=None):
        """ptx_ppm_render: Progressive_photon_map.Make(Scene).go without the gamma / PNG step -> img_sum (H, W, 3).
        callback(iteration, radius, length, image) is called after every iteration (0-based) with that iteration's radius, the
        length of its photon list and a copy of the running img_sum.  An exception it raises is raised again here, after the
        render has finished (the C entry point has no way to stop early); the later iterations are not reported."""
        arr = (abi.Light * len(lights))(*lights)
        h, w = params.height, params.width
        img = np.zeros((h, w, 3))
        st = abi.PpmStats()
        raised = []

        def trampoline(user, iteration, radius, length, img_sum):
            if raised:
                return
            try:
                callback(iteration, radius, length, np.ctypeslib.as_array(img_sum, shape=(h, w, 3)).copy())
            except BaseException as e:  # noqa: BLE001 -- carried across the C frames, raised again below
                raised.append(e)

        cb = PPM_ITERATION_FN(trampoline) if callback is not None else None
        rc = lib().ptx_ppm_render(self._h, C.byref(params), arr, len(lights), _dp(img), C.byref(st),
                                  C.cast(cb, C.c_void_p) if cb else None, None)
        if raised:
            raise raised[0]
        _check(rc)
        return img, {f: getattr(st, f) for f, _ in abi.PpmStats._fields_}

    def close(self):
        if getattr(self, "_h", None):
            lib().ptx_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_pose_look_at(scene_look_at, eye, target, up, aspect, fov_deg):
    """host.camera_pose_look_at: (origin, rotation, view) for Scene.set_camera_pose -- the camera (eye, target, up, aspect, fov_deg)
    over a scene built for the camera whose Mat4.look_at rows are scene_look_at"""
    from . import host
    return host.camera_pose_look_at(scene_look_at, eye, target, up, aspect, fov_deg)


def camera_shutter_between(origin0, rotation0, origin1, rotation1):
    """host.camera_shutter_between: (translation, axis, angle) for Scene.set_camera_shutter -- the motion that takes the camera from
    pose 0 to pose 1 (two results of camera_pose_look_at) while the shutter is open; the turn is R1 R0^T."""
    return host.camera_shutter_between(origin0, rotation0, origin1, rotation1)


def _image_arg(a, width, height, name):
    if a is None:
        return np.zeros((height, width, 3))
    if a.shape != (height, width, 3) or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name} must be a C-contiguous float64 array of shape (height, width, 3)")
    return a


def _display_arg(a, width, height, fmt, name):
    dtype, channels = abi.PTX_PIXEL_LAYOUT[fmt] if 0 <= fmt < len(abi.PTX_PIXEL_LAYOUT) else ("uint8", 3)  # (the library refuses it)
    if a is None:
        return np.zeros((height, width, channels), dtype=dtype)
    if a.shape != (height, width, channels) or a.dtype != np.dtype(dtype) or not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name} must be a C-contiguous {dtype} array of shape (height, width, {channels})")
    return a


def display_defaults():
    """ptx_display_defaults: RGB8, the reference's transfer, no tone curve, exposure 1.0"""
    d = abi.DisplayParams()
    _check(lib().ptx_display_defaults(C.byref(d)))
    return d


def display_pixel_bytes(fmt):
    """ptx_display_pixel_bytes: 3, 4, 12 or 16"""
    n = lib().ptx_display_pixel_bytes(abi._named(fmt, abi.PTX_PIXEL_NAMES, "format"))
    if n < 0:
        _check(n)
    return n


def display_thresholds():
    """ptx_display_thresholds: the 255 sRGB thresholds the library searches, [k - 1] = T[k].  Needs no device."""
    t = np.zeros(255)
    _check(lib().ptx_display_thresholds(_dp(t)))
    return t


def display_apply(image, display=None, **fields):
    """ptx_display_apply: the display rule on the host over a float64 array of shape (..., 3); returns the uint8 or float32 array
    of shape (..., 3 or 4).  `display`: an abi.DisplayParams or None; fields: format=, transfer=, tone=, exposure= over it."""
    d = abi.display_params(display, **fields)
    a = np.ascontiguousarray(image, dtype=np.float64)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("image must have shape (..., 3)")
    _check(lib().ptx_display_check(C.byref(d)))
    dtype, channels = abi.PTX_PIXEL_LAYOUT[d.format]
    out = np.zeros(a.shape[:-1] + (channels,), dtype=dtype)
    _check(lib().ptx_display_apply(C.byref(d), a.size // 3, _dp(a), C.c_void_p(out.ctypes.data)))
    return out


def display_image_device(device, n_pixels, d_rgb_ptr, d_out_ptr, display=None, stream=None, pixel_first=0, **fields):
    """ptx_display_image_device: the display rule over n_pixels pixels of a DEVICE f64 image (16-byte aligned) into DEVICE display
    pixels (16-byte aligned); waits for `stream`.  With pixel_first, ptx_display_range_device: pixels [pixel_first, pixel_first +
    n_pixels) of the two images, nothing outside them written."""
    d = abi.display_params(display, **fields)
    if pixel_first:
        _check(lib().ptx_display_range_device(int(device), C.byref(d), int(pixel_first), int(n_pixels), C.c_void_p(d_rgb_ptr),
                                              C.c_void_p(d_out_ptr), C.c_void_p(stream) if stream else None))
        return
    _check(lib().ptx_display_image_device(int(device), C.byref(d), int(n_pixels), C.c_void_p(d_rgb_ptr), C.c_void_p(d_out_ptr),
                                          C.c_void_p(stream) if stream else None))


def pixel_error_device(device, width, rows, passes_done, d_raw_ptr, d_sq_ptr, d_err_ptr=None, stream=None):
    """ptx_pixel_error_device: per-pixel standard error of the sample mean after `passes_done` passes from the DEVICE sums
    (raw, squares) into d_err_ptr (if given); returns the frame's rel_err = sqrt(sum se^2) / sqrt(sum mean^2)."""
    rel = C.c_double(0.0)
    _check(lib().ptx_pixel_error_device(device, width, rows, passes_done, C.c_void_p(d_raw_ptr), C.c_void_p(d_sq_ptr),
                                        C.c_void_p(d_err_ptr) if d_err_ptr else None, C.byref(rel),
                                        C.c_void_p(stream) if stream else None))
    return rel.value


def denoise_defaults():
    """ptx_denoise_defaults: levels 5, normal_power_log2 5, feature_passes 8, demodulation on, sigmas 4.0, 0.05, 0.2"""
    d = abi.DenoiseParams()
    _check(lib().ptx_denoise_defaults(C.byref(d)))
    return d


def denoise_params(denoise=None):
    """An abi.DenoiseParams from None (the defaults), a dict of fields over the defaults (`demodulate` sets the flag), or a
    DenoiseParams; checked as the library checks it (ValueError)."""
    if isinstance(denoise, abi.DenoiseParams):
        d = denoise
    else:
        d = denoise_defaults()
        fields = {f for f, _ in abi.DenoiseParams._fields_}
        for k, v in (denoise or {}).items():
            if k == "demodulate":
                d.flags = (d.flags | abi.PTX_DENOISE_DEMODULATE) if v else (d.flags & ~abi.PTX_DENOISE_DEMODULATE)
            elif k in fields:
                setattr(d, k, v)
            else:
                raise ValueError(f"unknown denoiser setting {k!r}")
    if not 0 <= d.levels <= 8:
        raise ValueError("levels must be in [0, 8]")
    if not 0 <= d.normal_power_log2 <= 8:
        raise ValueError("normal_power_log2 must be in [0, 8]")
    if d.feature_passes < 0:
        raise ValueError("feature_passes must be >= 0")
    if d.flags & ~abi.PTX_DENOISE_DEMODULATE:
        raise ValueError("unknown bits in flags")
    for name in ("sigma_luminance", "sigma_depth", "sigma_albedo"):
        v = getattr(d, name)
        if not (v > 0.0 and v < float("inf")):
            raise ValueError(f"{name} must be > 0 and finite")
    return d


def denoise_device(device, width, height, denoise, passes_done, feature_passes_done, d_raw_ptr, d_err_ptr, d_feat_ptr, d_out_ptr,
                   d_passes_ptr=None, stream=None):
    """ptx_denoise_device: the a-trous filter over DEVICE raw sums (W*H*3), their per-pixel standard error (W*H*3) and the
    feature sums of `feature_passes_done` passes (W*H*8) into d_out_ptr: denoised sums on the input's scale.  k = passes_done, or
    each pixel's own count from d_passes_ptr (int32, every count >= 2)."""
    dn = denoise_params(denoise)
    if not d_passes_ptr and int(passes_done) < 2:
        raise ValueError("passes_done must be >= 2")
    if int(feature_passes_done) < 1:
        raise ValueError("feature_passes_done must be >= 1")
    if int(width) <= 0 or int(height) <= 0:
        raise ValueError("bad dimensions")
    _check(lib().ptx_denoise_device(device, int(width), int(height), C.byref(dn), int(passes_done),
                                    C.c_void_p(d_passes_ptr) if d_passes_ptr else None, int(feature_passes_done),
                                    C.c_void_p(d_raw_ptr), C.c_void_p(d_err_ptr), C.c_void_p(d_feat_ptr), C.c_void_p(d_out_ptr),
                                    C.c_void_p(stream) if stream else None))


def temporal_defaults():
    """ptx_temporal_defaults: max_history_passes 64, normal_threshold 0.9, depth_tolerance 0.02, min_weight 2^-10"""
    t = abi.TemporalParams()
    _check(lib().ptx_temporal_defaults(C.byref(t)))
    return t


def temporal_params(temporal=None):
    """An abi.TemporalParams from None (the defaults), a dict of fields over the defaults, or a TemporalParams; checked as the
    library checks it (ValueError)."""
    if isinstance(temporal, abi.TemporalParams):
        t = temporal
    else:
        t = temporal_defaults()
        fields = {f for f, _ in abi.TemporalParams._fields_}
        for k, v in (temporal or {}).items():
            if k not in fields:
                raise ValueError(f"unknown temporal setting {k!r}")
            setattr(t, k, float(v))
    inf = float("inf")
    if not 0.0 <= t.max_history_passes < inf:
        raise ValueError("max_history_passes must be >= 0 and finite")
    if not -1.0 <= t.normal_threshold <= 1.0:
        raise ValueError("normal_threshold must be in [-1, 1]")
    if not 0.0 <= t.depth_tolerance < inf:
        raise ValueError("depth_tolerance must be >= 0 and finite")
    if not 0.0 <= t.min_weight < 1.0:
        raise ValueError("min_weight must be in [0, 1)")
    return t


def temporal_accumulate_device(device, width, height, temporal, passes_done, feature_passes_done, cur_camera, prev_camera, d_raw_ptr,
                               d_sq_ptr, d_feat_ptr, d_hist_prev_ptr, d_hist_out_ptr, d_raw_out_ptr, d_err_out_ptr,
                               d_motion_out_ptr=None, stream=None):
    """ptx_temporal_accumulate_device: this frame's DEVICE sums (raw, squares: W*H*3), feature sums (W*H*8) and the previous
    history (W*H*12, or None) reprojected from prev_camera into cur_camera (abi.TemporalCamera; prev_camera None only with no
    history) -> the new history, the accumulated sums as of passes_done passes, their standard error and, if asked for, the
    motion (W*H*3).  Returns the number of pixels that took history."""
    tp = temporal_params(temporal)
    took = C.c_int64(0)
    vp = lambda a: C.c_void_p(a) if a else None  # noqa: E731
    _check(lib().ptx_temporal_accumulate_device(int(device), int(width), int(height), C.byref(tp), int(passes_done),
                                                int(feature_passes_done), C.byref(cur_camera),
                                                C.byref(prev_camera) if prev_camera is not None else None, vp(d_raw_ptr), vp(d_sq_ptr),
                                                vp(d_feat_ptr), vp(d_hist_prev_ptr), vp(d_hist_out_ptr), vp(d_raw_out_ptr),
                                                vp(d_err_out_ptr), vp(d_motion_out_ptr), C.byref(took), vp(stream)))
    return took.value


def film_defaults():
    """ptx_film_defaults: (order, radius, renormalise) = (5, 1, False)"""
    f = abi.FilmParams()
    _check(lib().ptx_film_defaults(C.byref(f)))
    return f.order, f.pixel_radius, bool(f.flags & abi.PTX_FILM_RENORMALISE)


def film_weights(order, radius):
    """ptx_film_weights (host only): Binomial.create ~order ~pixel_radius as (w1d of 2r + 1 weights, w2d = their outer product)."""
    f = abi.film_params((order, radius))
    n = 2 * f.pixel_radius + 1
    w1, w2 = np.zeros(n), np.zeros((n, n))
    _check(lib().ptx_film_weights(C.byref(f), _dp(w1), _dp(w2)))
    return w1, w2


def film_resolve_counts_device(device, width, height, d_raw_ptr, d_passes_ptr, d_rgb_ptr, stream=None, film=None):
    """ptx_film_resolve_counts_device: the film of DEVICE raw sums with a per-pixel pass count (int32, H x W); film: what
    abi.film_params takes (ptx_film_resolve_counts_ex_device)"""
    if film is not None:
        f = abi.film_params(film)
        _check(lib().ptx_film_resolve_counts_ex_device(device, width, height, C.byref(f), C.c_void_p(d_raw_ptr), C.c_void_p(d_passes_ptr),
                                                       C.c_void_p(d_rgb_ptr), C.c_void_p(stream) if stream else None))
        return
    _check(lib().ptx_film_resolve_counts_device(device, width, height, C.c_void_p(d_raw_ptr), C.c_void_p(d_passes_ptr),
                                                C.c_void_p(d_rgb_ptr), C.c_void_p(stream) if stream else None))


def pixel_error_counts_device(device, width, rows, d_passes_ptr, d_raw_ptr, d_sq_ptr, d_err_ptr=None, stream=None):
    """ptx_pixel_error_counts_device: pixel_error_device with each pixel's own pass count (int32, rows x W); returns rel_err"""
    rel = C.c_double(0.0)
    _check(lib().ptx_pixel_error_counts_device(device, width, rows, C.c_void_p(d_passes_ptr), C.c_void_p(d_raw_ptr),
                                               C.c_void_p(d_sq_ptr), C.c_void_p(d_err_ptr) if d_err_ptr else None,
                                               C.byref(rel), C.c_void_p(stream) if stream else None))
    return rel.value


def render_multi(scenes, width, height, samples_per_pixel, max_bounces, progress=None, **kw):
    """ptx_render_multi: one image over several scene replicas (one per GPU) inside this process."""
    p = render_params(width, height, samples_per_pixel, max_bounces, **kw)
    out = np.zeros((height, width, 3))
    st = abi.Stats()
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    cb = PROGRESS_FN(lambda user, n: progress(n)) if progress else None
    _check(lib().ptx_render_multi(arr, len(scenes), C.byref(p), _dp(out), C.byref(st),
                                  C.cast(cb, C.c_void_p) if cb else None, None))
    return out, stats_dict(st)


def film_resolve_banded_device(device, width, height, samples_per_pixel, d_gathered_ptr, n_ranks, band_rows, pad_rows,
                               d_rgb_ptr, stream=None, wait=True, film=None):
    """wait=False: ptx_film_resolve_banded_queue -- the pass is queued on `stream`, the call does not wait for it.
    film: what abi.film_params takes (ptx_film_resolve_banded_ex_device, which always waits)."""
    if film is not None:
        if not wait:
            raise ValueError("a film other than the default has no queued form: wait must be True")
        f = abi.film_params(film)
        _check(lib().ptx_film_resolve_banded_ex_device(device, width, height, samples_per_pixel, C.byref(f), C.c_void_p(d_gathered_ptr),
                                                       n_ranks, band_rows, pad_rows, C.c_void_p(d_rgb_ptr),
                                                       C.c_void_p(stream) if stream else None))
        return
    fn = lib().ptx_film_resolve_banded_device if wait else lib().ptx_film_resolve_banded_queue
    _check(fn(device, width, height, samples_per_pixel, C.c_void_p(d_gathered_ptr), n_ranks, band_rows, pad_rows,
              C.c_void_p(d_rgb_ptr), C.c_void_p(stream) if stream else None))


def film_resolve_device(device, width, height, samples_per_pixel, d_raw_ptr, d_rgb_ptr, stream=None, film=None):
    """film: what abi.film_params takes (ptx_film_resolve_ex_device)"""
    if film is not None:
        f = abi.film_params(film)
        _check(lib().ptx_film_resolve_ex_device(device, width, height, samples_per_pixel, C.byref(f), C.c_void_p(d_raw_ptr),
                                                C.c_void_p(d_rgb_ptr), C.c_void_p(stream) if stream else None))
        return
    _check(lib().ptx_film_resolve_device(device, width, height, samples_per_pixel, C.c_void_p(d_raw_ptr),
                                         C.c_void_p(d_rgb_ptr), C.c_void_p(stream) if stream else None))


def local_rows(params):
    return lib().ptx_local_rows(C.byref(params))


def global_row(params, local_row):
    return lib().ptx_global_row(C.byref(params), local_row)


def lds_sample(dimension, offsets, dims, device=0):
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    out = np.zeros(len(offsets))
    _check(lib().ptx_lds_sample(device, dimension, len(offsets), _ip(offsets), _ip(dims), _dp(out)))
    return out


MATH_FN = {"hypot": 0, "sin": 1, "cos": 2, "acos": 3, "atan2": 4, "pow5": 5, "sqrt": 6, "div": 7, "fma": 8,
           "rnorm3": 9, "rnorm_frame": 10, "sqrt_nonneg": 11, "rcp_mid": 12, "div_mid": 13, "sqrt_mid": 14}


def math_eval(fn, a, b=None, device=0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    bb = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
    out = np.zeros_like(a)
    _check(lib().ptx_math_eval(device, MATH_FN[fn], a.size, _dp(a), _dp(bb) if bb is not None else None, _dp(out)))
    return out
