"""Python mirror of the reference's operator surface for this path.

* :class:`Args` / :func:`args_term`  <- ``Render_command.Args`` (render_command/src/render_command.ml:6-48)
* :class:`Integrator` (``create`` / ``render``) <- ``Integrator`` (path_tracer/src/integrator.mli:4-16)
* :func:`run` <- ``Render_command.Make(Scene).run`` (render_command.ml:64-109)

The opaque closures ``intersect`` / ``background`` of the reference's ``Scene`` argument are replaced by the
declarative scene (a :class:`path_tracer_ocaml_amd.host.HostScene` or any ``ptx_scene_desc``); everything runs
on the GPU through libptx_hip.so -- there is no CPU path here.
"""
import argparse
import time
from dataclasses import dataclass

import numpy as np

from . import Scene


@dataclass
class Args:  # Render_command.Args.t
    width: int
    height: int
    samples_per_pixel: int = 1
    output: str = "output.png"
    no_progress: bool = False
    max_bounces: int = 8


def args_term(parser=None):
    """Cmdliner term of the reference: -d/--dimension W,H (required), --samples-per-pixel (1), -o/--output
    (output.png), --no-progress, --max-ray-bounces (8)."""
    p = parser or argparse.ArgumentParser()

    def dimension(s):
        w, h = s.split(",")
        return int(w), int(h)

    p.add_argument("-d", "--dimension", type=dimension, required=True, metavar="WIDTH,HEIGHT", help="image dimensions")
    p.add_argument("--samples-per-pixel", type=int, default=1, metavar="INT", help="trace INT camera rays per pixel")
    p.add_argument("-o", "--output", default="output.png", metavar="PATH", help="write image to PATH")
    p.add_argument("--no-progress", action="store_true", help="suppress progress bar")
    p.add_argument("--max-ray-bounces", type=int, default=8, metavar="INT", help="max ray bounces")
    return p


def args_of_namespace(ns):
    w, h = ns.dimension
    return Args(w, h, ns.samples_per_pixel, ns.output, ns.no_progress, ns.max_ray_bounces)


class Integrator:
    """``Integrator.create ~width ~height ~image ~samples_per_pixel ~max_bounces ~camera ~intersect ~background``
    with (camera, intersect, background) folded into the declarative ``scene``; ``image`` is the (H, W, 3) f64
    array ``render`` fills, like the reference's Bimage.  ``lighting`` stands for the reference's ``~diffuse_plus_light`` slot:
    "reference" (the default: ``Pdf.diffuse`` and the reference's emission formula), "path-order" or "sampled"
    (Scene.set_lighting); None leaves a Scene that was handed in as it is.  ``film`` is the reconstruction filter the reference
    hard-wires (``Binomial.create ~order:5 ~pixel_radius:1``): (order, radius) or (order, radius, renormalise) for Scene.set_film;
    None leaves the scene's film as it is.  ``environment``: an (H, W, 3) latitude-longitude image, or (image, rotation) or
    (image, rotation, bilinear), for Scene.set_environment; ``images``: {texture index: image or (image, bilinear, repeat)} for
    Scene.set_texture_image.  None leaves the scene's as they are.  ``environment_sampling``: True / False for
    Scene.set_environment_sampling -- with "sampled" lighting the light density then includes (or, on a scene without emissive
    triangles, is) the environment's; True is applied after the environment and before the lighting mode, which may need it.
    ``lens``: (radius, focus_distance) for Scene.set_lens, the thin-lens camera; None leaves the scene's as it is.
    ``sphere_light_sampling``: True / False for Scene.set_sphere_light_sampling -- with "sampled" lighting the light half then holds
    the scene's emissive spheres beside its emissive triangles; like ``environment_sampling`` True is applied before the lighting mode.
    ``camera_pose``: (origin, rotation) or (origin, rotation, view) for Scene.set_camera_pose -- what camera_pose_look_at returns;
    None leaves the scene's as it is.  ``projection``: "perspective" or "latlong" (or the PTX_PROJECTION_* value) for
    Scene.set_camera_projection, applied after the lens; None leaves the scene's as it is.  ``camera_shutter``: (translation, axis,
    angle) for Scene.set_camera_shutter -- what camera_shutter_between returns; None leaves the scene's as it is."""

    def __init__(self, width, height, image, samples_per_pixel, max_bounces, scene, device=0, lighting=None, film=None,
                 environment=None, images=None, environment_sampling=None, lens=None, sphere_light_sampling=None,
                 camera_pose=None, projection=None, camera_shutter=None):
        if image.shape != (height, width, 3) or image.dtype != np.float64:
            raise ValueError("image must be a float64 array of shape (height, width, 3)")
        self.width, self.height, self.image = width, height, image
        self.samples_per_pixel, self.max_bounces = samples_per_pixel, max_bounces
        self._scene = scene if isinstance(scene, Scene) else Scene(scene.ptr, device, keepalive=scene)
        if lighting is not None and not environment_sampling and not sphere_light_sampling:
            self._scene.set_lighting(lighting)
        if film is not None:
            self._scene.set_film(*film)
        if lens is not None:
            self._scene.set_lens(*lens)
        if camera_pose is not None:
            self._scene.set_camera_pose(*camera_pose)
        if projection is not None:
            self._scene.set_camera_projection(projection)
        if camera_shutter is not None:
            self._scene.set_camera_shutter(*camera_shutter)
        if environment is not None:
            self._scene.set_environment(*(environment if isinstance(environment, tuple) else (environment,)))
        if environment_sampling is not None:
            self._scene.set_environment_sampling(bool(environment_sampling))
        if sphere_light_sampling is not None:
            self._scene.set_sphere_light_sampling(bool(sphere_light_sampling))
        if lighting is not None and (environment_sampling or sphere_light_sampling):
            self._scene.set_lighting(lighting)
        for index, img in (images or {}).items():
            self._scene.set_texture_image(index, *(img if isinstance(img, tuple) else (img,)))
        self.stats = None
        self.error = self.passes_done = None  # render_progressive
        self.passes = None  # render_adaptive
        self.features = None  # render_denoised
        self.motion = self.history_pixels = None  # render_temporal

    @classmethod
    def create(cls, *, width, height, image, samples_per_pixel, max_bounces, scene, device=0, lighting=None, film=None,
               environment=None, images=None, environment_sampling=None, lens=None, sphere_light_sampling=None,
               camera_pose=None, projection=None, camera_shutter=None):
        return cls(width, height, image, samples_per_pixel, max_bounces, scene, device, lighting, film, environment, images,
                   environment_sampling, lens, sphere_light_sampling, camera_pose, projection, camera_shutter)

    def render(self, update_progress=None):
        """``Integrator.render ~update_progress``: update_progress receives pixel counts summing to W*H."""
        rgb, st = self._scene.render(self.width, self.height, self.samples_per_pixel, self.max_bounces,
                                     progress=update_progress)
        self.image[...] = rgb
        self.stats = st
        return self.image

    def render_display(self, format="rgb8", transfer="reference", tone="none", exposure=1.0, update_progress=None, out=None):
        """``render`` whose result is display pixels (Scene.render_display): a uint8 or float32 array of shape (H, W, 3 or 4),
        converted on the device.  ``image``, the f64 Bimage, is not written."""
        pixels, st = self._scene.render_display(self.width, self.height, self.samples_per_pixel, self.max_bounces, format=format,
                                                transfer=transfer, tone=tone, exposure=exposure, progress=update_progress, out=out)
        self.stats = st
        return pixels

    def render_progressive_display(self, passes_per_update, denoise=None, format="rgb8", transfer="reference", tone="none",
                                   exposure=1.0, on_update=None, target_rel_err=0.0, want_error=True, out=None):
        """``render_progressive`` -- with ``denoise``, ``render_denoised`` -- whose updates are display pixels
        (Scene.render_progressive_display).  Returns the last update's pixels; ``error`` and ``passes_done`` as there."""
        pixels, err, done, st = self._scene.render_progressive_display(
            self.width, self.height, self.samples_per_pixel, self.max_bounces, passes_per_update, denoise=denoise, format=format,
            transfer=transfer, tone=tone, exposure=exposure, on_update=on_update, target_rel_err=target_rel_err,
            want_error=want_error, out=out)
        self.error, self.passes_done, self.stats = err, done, st
        return pixels

    def render_progressive(self, passes_per_update, on_update=None, target_rel_err=0.0, want_error=True):
        """``render`` as a sequence of updates (Scene.render_progressive): ``image`` holds the image of the last update,
        ``error`` its per-pixel standard error (None without want_error), ``passes_done`` how many passes it holds."""
        out = self.image if self.image.flags["C_CONTIGUOUS"] else None
        rgb, err, done, st = self._scene.render_progressive(self.width, self.height, self.samples_per_pixel, self.max_bounces,
                                                            passes_per_update, on_update=on_update,
                                                            target_rel_err=target_rel_err, want_error=want_error, out=out)
        if out is None:
            self.image[...] = rgb
        self.error, self.passes_done, self.stats = err, done, st
        return self.image

    def render_adaptive(self, target_rel_err, min_passes=8, passes_per_round=8, radiance_floor=1e-3, on_round=None):
        """``render`` with per-pixel pass counts (Scene.render_adaptive): ``image`` holds the image of the last round, ``error``
        its per-pixel standard error and ``passes`` each pixel's pass count (int32, H x W)."""
        out = self.image if self.image.flags["C_CONTIGUOUS"] else None
        rgb, err, passes, st = self._scene.render_adaptive(self.width, self.height, self.samples_per_pixel, self.max_bounces,
                                                           target_rel_err, min_passes=min_passes,
                                                           passes_per_round=passes_per_round, radiance_floor=radiance_floor,
                                                           on_round=on_round, out=out)
        if out is None:
            self.image[...] = rgb
        self.error, self.passes, self.stats = err, passes, st
        return self.image

    def render_denoised(self, passes_per_update, denoise=None, on_update=None, target_rel_err=0.0, want_features=False):
        """``render`` as a sequence of DENOISED updates (Scene.render_denoised): ``image`` holds the filtered image of the last
        update, ``error`` the un-denoised per-pixel standard error, ``passes_done`` its passes and ``features`` the first-hit
        feature means ((H, W, 8): albedo, normal, depth, hits) when want_features is set."""
        out = self.image if self.image.flags["C_CONTIGUOUS"] else None
        rgb, err, feat, done, st = self._scene.render_denoised(self.width, self.height, self.samples_per_pixel, self.max_bounces,
                                                               passes_per_update, denoise=denoise, on_update=on_update,
                                                               target_rel_err=target_rel_err, out=out,
                                                               feat_out=True if want_features else None)
        if out is None:
            self.image[...] = rgb
        self.error, self.passes_done, self.features, self.stats = err, done, feat, st
        return self.image

    def render_temporal(self, pass_first, pass_count, temporal=None, denoise=None, want_error=False, want_motion=False):
        """One frame of a sequence (Scene.render_temporal): passes [pass_first, pass_first + pass_count) of ``samples_per_pixel``,
        accumulated onto the history the scene keeps from the frames before, under the scene's camera pose.  ``image`` holds the
        frame, ``error`` the accumulated per-pixel standard error (with want_error), ``motion`` each pixel's (dx, dy, weight) into
        the previous frame (with want_motion) and ``history_pixels`` how many pixels took history.  Advance pass_first from frame
        to frame; Scene.temporal_reset drops the history."""
        out = self.image if self.image.flags["C_CONTIGUOUS"] else None
        rgb, err, motion, took, st = self._scene.render_temporal(self.width, self.height, self.samples_per_pixel, self.max_bounces,
                                                                 pass_first, pass_count, temporal=temporal, denoise=denoise,
                                                                 want_err=want_error, want_motion=want_motion, out=out)
        if out is None:
            self.image[...] = rgb
        self.error, self.motion, self.history_pixels, self.passes_done, self.stats = err, motion, took, pass_count, st
        return self.image


def run(args, scene, device=0, echo=print):
    """Render_command.Make(Scene).run: render, save the PNG, print ``rendered in: X ms``."""
    from . import host
    image = np.zeros((args.height, args.width, 3))
    integ = Integrator.create(width=args.width, height=args.height, image=image, samples_per_pixel=args.samples_per_pixel,
                              max_bounces=args.max_bounces, scene=scene, device=device)
    t0 = time.perf_counter()
    integ.render(None if args.no_progress else (lambda n: None))
    elapsed_ms = (time.perf_counter() - t0) * 1e3
    host.write_png(args.output, image)
    echo("rendered in: %.3f ms" % elapsed_ms)
    return image, integ.stats
