/* ptx_ml_marshal.h -- the argument marshalling of the OCaml stub, free of OCaml headers.
 *
 * ptx_stubs.c (which needs <caml/...> and cannot be compiled in this image) only unpacks OCaml values into the
 * FLAT view below -- borrowed pointers into floatarrays / Bigarrays, exactly the convention of the reference's
 * existing stub (value coords -> f64 slices read in place, sphere-intersect-rs/src/lib.rs:53-76) -- and calls
 * these functions.  Everything that can go wrong between "flat OCaml data" and the C ABI of include/ptx.h
 * therefore lives here, where tests/test_ocaml_binding.py can compile and run it (gcc, no OCaml needed).
 *
 * Flat layout (what bindings/ocaml/ptx.ml's `flatten` produces; every coordinate in CAMERA space):
 *   xs, ys, zs, rs     floatarray, one entry per sphere (Sphere.transform ~f:(Camera.transform camera),
 *                      shirley_spheres/bin/main.ml:258-260; cornell-box/bin/main.ml:70-91,218)
 *   sphere_material    int32 Bigarray, index into `materials`
 *   materials          floatarray, 6 per material : kind (0 Lambertian, 1 Metal, 2 Dielectric), texture index,
 *                      refraction index, emit r g b          (Material.t, path_tracer/src/material.ml:3-14; Hit.emit, hit.ml:5)
 *   textures           floatarray, 9 per texture  : kind (0 solid, 1 checker), width, height, even r g b, odd r g b
 *                      (Texture.solid / Texture.checker, path_tracer/src/texture.ml:16-31)
 *   camera             floatarray, 4 : lower_left_x, lower_left_y, view_x, view_y   (camera.ml:50-53)
 *   background         floatarray, 7 : kind (0 black, 1 sky), horizon r g b, zenith r g b  (main.ml:104-110)
 *   vertex_x/y/z       floatarray, one entry per mesh vertex (ganesha Mesh.t, ganesha/bin/main.ml:37-85; cornell-box's
 *                      Face.t keeps three private vertices per triangle, cornell-box/bin/main.ml:5-28)
 *   tri_indices        int32 Bigarray, 3 per triangle: a, b, c (ganesha Face.t, main.ml:92-110)
 *   tri_uv             floatarray, 6 per triangle: Face.tex_coords (ua, va), (ub, vb), (uc, vc)
 *   tri_material       int32 Bigarray, 1 per triangle, index into `materials`
 *   floor_vertices     floatarray, 9 per floor triangle: a, b, c -- tested BEFORE the tree, first hit clips t_max
 *                      (ganesha Floor.intersect, main.ml:205-260,286-298)
 *   floor_uv, floor_material   6 per floor triangle / int32 per floor triangle
 *   lights             floatarray, 11 per light: kind (0 point, 1 spot), position xyz, direction xyz, color rgb, power
 *                      (Progressive_photon_map.Light.create_point / create_spot, progressive_photon_map.ml:59-137)
 *   ppm params         floatarray, 6: width, height, iterations, max_bounces, photon_count, alpha (Args.t, :7-16)
 */
#ifndef PTX_ML_MARSHAL_H
#define PTX_ML_MARSHAL_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ptx.h"

typedef struct ptx_ml_flat {
  int32_t n_spheres;
  const double *xs, *ys, *zs, *rs;
  const int32_t* sphere_material;
  int32_t n_materials;
  const double* materials; /* 6 per material */
  int32_t n_textures;
  const double* textures;  /* 9 per texture */
  const double* camera;     /* 4 */
  const double* background; /* 7 */
  int32_t leaf_kind;        /* PTX_LEAF_SIMD (Simd_leaf) / PTX_LEAF_ARRAY (Array_leaf) */
  int32_t length_cutoff;    /* Leaf.length_cutoff: leaf_size () = 16 / 4 (main.ml:121,175) / 2 (cornell) / 8 (ganesha) */
  /* triangle mesh: all zero / NULL when the scene has none */
  int32_t n_vertices;
  const double *vertex_x, *vertex_y, *vertex_z;
  int32_t n_triangles;
  const int32_t* tri_indices; /* 3 per triangle */
  const double* tri_uv;       /* 6 per triangle */
  const int32_t* tri_material;
  int32_t n_floor_triangles;
  const double* floor_vertices; /* 9 per triangle */
  const double* floor_uv;       /* 6 per triangle */
  const int32_t* floor_material;
} ptx_ml_flat;

/* Why the last ptx_ml_scene_create of this thread returned NULL: a message of THIS layer (bad counts, no memory), or NULL when
 * the library refused the scene and ptx_last_error() holds the reason.  The stub raises ptx_ml_scene_create_error() first. */
static __thread const char* ptx_ml_create_error_;
static __attribute__((unused)) const char* ptx_ml_scene_create_error(void) { return ptx_ml_create_error_ ? ptx_ml_create_error_ : ptx_last_error(); }

/* NULL + ptx_ml_scene_create_error() on failure.  Nothing of `f` is referenced after the call returns. */
static ptx_scene* ptx_ml_scene_create(const ptx_ml_flat* f, int32_t device) {
  ptx_ml_create_error_ = NULL;
  if (!f || f->n_spheres < 0 || f->n_triangles < 0 || f->n_floor_triangles < 0 || f->n_textures < 0) {
    ptx_ml_create_error_ = "Ptx.scene_create: negative element count";
    return NULL;
  }
  if (f->n_materials <= 0) {
    ptx_ml_create_error_ = "Ptx.scene_create: the material table is empty";
    return NULL;
  }
  ptx_material* mats = (ptx_material*)calloc((size_t)f->n_materials, sizeof *mats);
  ptx_texture* texs = (ptx_texture*)calloc((size_t)(f->n_textures > 0 ? f->n_textures : 1), sizeof *texs);
  if (!mats || !texs) {
    free(mats);
    free(texs);
    ptx_ml_create_error_ = "Ptx.scene_create: out of memory for the material / texture tables";
    return NULL;
  }
  for (int32_t i = 0; i < f->n_materials; ++i) {
    const double* m = f->materials + 6 * (size_t)i;
    mats[i].kind = (int32_t)m[0];
    mats[i].texture = (int32_t)m[1];
    mats[i].index = m[2];
    memcpy(mats[i].emit, m + 3, sizeof mats[i].emit);
  }
  for (int32_t i = 0; i < f->n_textures; ++i) {
    const double* t = f->textures + 9 * (size_t)i;
    texs[i].kind = (int32_t)t[0];
    texs[i].width = (int32_t)t[1];
    texs[i].height = (int32_t)t[2];
    memcpy(texs[i].even, t + 3, sizeof texs[i].even);
    memcpy(texs[i].odd, t + 6, sizeof texs[i].odd);
  }
  ptx_scene_desc d;
  memset(&d, 0, sizeof d);
  d.n_spheres = f->n_spheres;
  d.sphere_x = f->xs; d.sphere_y = f->ys; d.sphere_z = f->zs; d.sphere_r = f->rs;
  d.sphere_material = f->sphere_material;
  d.n_vertices = f->n_vertices;
  d.vertex_x = f->vertex_x; d.vertex_y = f->vertex_y; d.vertex_z = f->vertex_z;
  d.n_triangles = f->n_triangles;
  d.tri_indices = f->tri_indices;
  d.tri_uv = f->tri_uv;
  d.tri_material = f->tri_material;
  d.n_floor_triangles = f->n_floor_triangles;
  d.floor_vertices = f->floor_vertices;
  d.floor_uv = f->floor_uv;
  d.floor_material = f->floor_material;
  d.n_materials = f->n_materials;
  d.materials = mats;
  d.n_textures = f->n_textures;
  d.textures = texs;
  d.camera.lower_left_x = f->camera[0]; d.camera.lower_left_y = f->camera[1];
  d.camera.view_x = f->camera[2]; d.camera.view_y = f->camera[3];
  d.background.kind = (int32_t)f->background[0];
  memcpy(d.background.horizon, f->background + 1, sizeof d.background.horizon);
  memcpy(d.background.zenith, f->background + 4, sizeof d.background.zenith);
  d.leaf_kind = f->leaf_kind;
  d.length_cutoff = f->length_cutoff;
  d.num_bins = 0; /* Shape_tree.create's default, 32 */
  ptx_scene* s = ptx_scene_create(&d, device); /* copies everything it keeps */
  free(mats);
  free(texs);
  return s;
}

/* Integrator.render into the Bimage's f64 RGB buffer (W*H*3, row 0 = top).  0 or a negative ptx error code. */
static int32_t ptx_ml_render(ptx_scene* s, int32_t width, int32_t height, int32_t samples_per_pixel, int32_t max_bounces,
                             int32_t n_gpus, double* image, ptx_progress_fn progress, void* user) {
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = width;
  p.height = height;
  p.samples_per_pixel = samples_per_pixel;
  p.max_bounces = max_bounces;
  p.n_gpus = n_gpus;
  return ptx_render(s, &p, image, NULL, progress, user);
}

/* Progressive_photon_map.Make(Scene).go's loop (progressive_photon_map.ml:420-451) without the prints and the PNG:
 * params6 = width, height, iterations, max_bounces, photon_count, alpha; lights11 = 11 doubles per light (above).
 * img_sum (W*H*3) receives the final sum; iteration_cb gets the running sum after every iteration. */
static int32_t ptx_ml_ppm_render(ptx_scene* s, const double* params6, const double* lights11, int32_t n_lights, double* img_sum,
                                 ptx_ppm_iteration_fn iteration_cb, void* user) {
  if (!params6 || n_lights < 0 || n_lights > 64 || (n_lights > 0 && !lights11)) return -1;
  ptx_ppm_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params6[0];
  p.height = (int32_t)params6[1];
  p.iterations = (int32_t)params6[2];
  p.max_bounces = (int32_t)params6[3];
  p.photon_count = (int32_t)params6[4];
  p.alpha = params6[5];
  ptx_light lights[64];
  memset(lights, 0, sizeof lights);
  for (int32_t i = 0; i < n_lights; ++i) {
    const double* l = lights11 + 11 * (size_t)i;
    lights[i].kind = (int32_t)l[0];
    memcpy(lights[i].position, l + 1, sizeof lights[i].position);
    memcpy(lights[i].direction, l + 4, sizeof lights[i].direction);
    memcpy(lights[i].color, l + 7, sizeof lights[i].color);
    lights[i].power = l[10];
  }
  return ptx_ppm_render(s, &p, lights, n_lights, img_sum, NULL, iteration_cb, user);
}

/* Integrator.render as a sequence of updates (ptx_render_progressive, want_error on): params6 = width, height,
 * samples_per_pixel, max_bounces, passes_per_update, target_rel_err.  image (W*H*3) holds the image of the last update, err
 * (nullable) its per-pixel standard error, *passes_done its passes; on_update runs after every update. */
static __attribute__((unused)) int32_t ptx_ml_render_progressive(ptx_scene* s, const double* params6, double* image, double* err, int32_t* passes_done,
                                                                 ptx_update_fn on_update, void* user) {
  if (!params6) return -1;
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params6[0];
  p.height = (int32_t)params6[1];
  p.samples_per_pixel = (int32_t)params6[2];
  p.max_bounces = (int32_t)params6[3];
  ptx_progressive_params pp;
  memset(&pp, 0, sizeof pp);
  pp.passes_per_update = (int32_t)params6[4];
  pp.want_error = 1;
  pp.target_rel_err = params6[5];
  return ptx_render_progressive(s, &p, &pp, image, err, passes_done, NULL, on_update, user);
}

/* Integrator.render with per-pixel pass counts (ptx_render_adaptive): params8 = width, height, samples_per_pixel, max_bounces,
 * min_passes, passes_per_round, target_rel_err, radiance_floor.  image (W*H*3) holds the image of the last round, err (nullable)
 * its per-pixel standard error, passes (nullable, W*H) the count map, *samples the sum of the map; on_round runs after every
 * round. */
static __attribute__((unused)) int32_t ptx_ml_render_adaptive(ptx_scene* s, const double* params8, double* image, double* err, int32_t* passes,
                                                              int64_t* samples, ptx_round_fn on_round, void* user) {
  if (!params8) return -1;
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params8[0];
  p.height = (int32_t)params8[1];
  p.samples_per_pixel = (int32_t)params8[2];
  p.max_bounces = (int32_t)params8[3];
  ptx_adaptive_params ap;
  memset(&ap, 0, sizeof ap);
  ap.min_passes = (int32_t)params8[4];
  ap.passes_per_round = (int32_t)params8[5];
  ap.target_rel_err = params8[6];
  ap.radiance_floor = params8[7];
  ptx_stats st;
  memset(&st, 0, sizeof st);
  const int32_t rc = ptx_render_adaptive(s, &p, &ap, image, err, passes, &st, on_round, user);
  if (samples) *samples = st.samples;
  return rc;
}

/* Integrator.render as a sequence of DENOISED updates (ptx_render_denoised): params13 = width, height, samples_per_pixel,
 * max_bounces, passes_per_update, target_rel_err, then the denoiser's levels, normal_power_log2, feature_passes, flags,
 * sigma_luminance, sigma_depth, sigma_albedo.  image (W*H*3) holds the filtered image of the last update, err (nullable) the
 * un-denoised per-pixel standard error, feat (nullable, W*H*8) the first-hit feature means, *passes_done its passes. */
static __attribute__((unused)) int32_t ptx_ml_render_denoised(ptx_scene* s, const double* params13, double* image, double* err, double* feat,
                                                              int32_t* passes_done, ptx_update_fn on_update, void* user) {
  if (!params13) return -1;
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params13[0];
  p.height = (int32_t)params13[1];
  p.samples_per_pixel = (int32_t)params13[2];
  p.max_bounces = (int32_t)params13[3];
  ptx_progressive_params pp;
  memset(&pp, 0, sizeof pp);
  pp.passes_per_update = (int32_t)params13[4];
  pp.want_error = 1;
  pp.target_rel_err = params13[5];
  ptx_denoise_params dn;
  memset(&dn, 0, sizeof dn);
  dn.levels = (int32_t)params13[6];
  dn.normal_power_log2 = (int32_t)params13[7];
  dn.feature_passes = (int32_t)params13[8];
  dn.flags = (int32_t)params13[9];
  dn.sigma_luminance = params13[10];
  dn.sigma_depth = params13[11];
  dn.sigma_albedo = params13[12];
  return ptx_render_denoised(s, &p, &pp, &dn, image, err, feat, passes_done, NULL, on_update, user);
}

/* One frame of a sequence with temporal accumulation (ptx_render_temporal): params18 = width, height, samples_per_pixel (the
 * SEQUENCE's N), max_bounces, pass_first, pass_count, then the temporal settings max_history_passes, normal_threshold,
 * depth_tolerance, min_weight, then denoise (0 = no spatial filter) and the denoiser's levels, normal_power_log2, feature_passes,
 * flags, sigma_luminance, sigma_depth, sigma_albedo (read only when denoise is not 0).  image (W*H*3) holds the frame, err (nullable)
 * the accumulated per-pixel standard error, motion (nullable, W*H*3) each pixel's (dx, dy, weight) into the frame before,
 * *history_pixels (nullable) how many pixels took history. */
static __attribute__((unused)) int32_t ptx_ml_render_temporal(ptx_scene* s, const double* params18, double* image, double* err, double* motion,
                                                              int64_t* history_pixels) {
  if (!params18) return -1;
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params18[0];
  p.height = (int32_t)params18[1];
  p.samples_per_pixel = (int32_t)params18[2];
  p.max_bounces = (int32_t)params18[3];
  ptx_temporal_params tp;
  tp.max_history_passes = params18[6];
  tp.normal_threshold = params18[7];
  tp.depth_tolerance = params18[8];
  tp.min_weight = params18[9];
  ptx_denoise_params dn;
  memset(&dn, 0, sizeof dn);
  dn.levels = (int32_t)params18[11];
  dn.normal_power_log2 = (int32_t)params18[12];
  dn.feature_passes = (int32_t)params18[13];
  dn.flags = (int32_t)params18[14];
  dn.sigma_luminance = params18[15];
  dn.sigma_depth = params18[16];
  dn.sigma_albedo = params18[17];
  return ptx_render_temporal(s, &p, &tp, params18[10] != 0.0 ? &dn : NULL, (int32_t)params18[4], (int32_t)params18[5], image, err, motion,
                             history_pixels, NULL);
}
/* Ptx.temporal_reset: drops the frame history the scene keeps (ptx_temporal_reset) */
static __attribute__((unused)) int32_t ptx_ml_temporal_reset(ptx_scene* s) { return ptx_temporal_reset(s); }

/* Ptx.set_film: the film every later render of the scene applies (ptx_scene_set_film) */
static __attribute__((unused)) int32_t ptx_ml_set_film(ptx_scene* s, int32_t order, int32_t pixel_radius, int32_t flags) {
  ptx_film_params f;
  memset(&f, 0, sizeof f);
  f.order = order;
  f.pixel_radius = pixel_radius;
  f.flags = flags;
  return ptx_scene_set_film(s, &f);
}

/* Ptx.set_lens / Ptx.lens: the thin lens every later render of the scene looks through (ptx_scene_set_lens; radius 0 = off) */
static __attribute__((unused)) int32_t ptx_ml_set_lens(ptx_scene* s, const double* pair, int64_t n_pair) {
  if (n_pair != 2) return -4; /* (radius, focus_distance) */
  return ptx_scene_set_lens(s, pair[0], pair[1]);
}
static __attribute__((unused)) int32_t ptx_ml_lens(const ptx_scene* s, double* radius, double* focus_distance) {
  return ptx_scene_lens(s, radius, focus_distance);
}

/* Ptx.set_camera_pose / Ptx.clear_camera_pose / Ptx.camera_pose: where every later render of the scene is taken from
 * (ptx_scene_set_camera_pose).  pose: the 12 doubles origin (3) then rotation (9, row-major), or n_pose = 0 for none; view: the 4
 * doubles lower_left_x, lower_left_y, view_x, view_y, or n_view = 0 for the scene's own.  -4 for any other length, or when both are
 * empty (clearing is a call of its own: nothing is switched off by accident). */
static __attribute__((unused)) int32_t ptx_ml_set_camera_pose(ptx_scene* s, const double* pose, int64_t n_pose, const double* view, int64_t n_view) {
  if ((n_pose != 0 && n_pose != 12) || (n_view != 0 && n_view != 4) || (n_pose == 0 && n_view == 0)) return -4;
  ptx_camera v;
  if (n_view) { v.lower_left_x = view[0]; v.lower_left_y = view[1]; v.view_x = view[2]; v.view_y = view[3]; }
  return ptx_scene_set_camera_pose(s, n_pose ? pose : NULL, n_pose ? pose + 3 : NULL, n_view ? &v : NULL);
}
static __attribute__((unused)) int32_t ptx_ml_clear_camera_pose(ptx_scene* s) { return ptx_scene_set_camera_pose(s, NULL, NULL, NULL); }
/* out: 16 doubles -- origin, rotation, the view in effect; returns 1 = on, 0 = off, or the library's (negative) code; -4 when out is
 * not 16 long (nothing is written) */
static __attribute__((unused)) int32_t ptx_ml_camera_pose(const ptx_scene* s, double* out, int64_t n_out) {
  if (n_out != 16) return -4;
  ptx_camera v = {0.0, 0.0, 0.0, 0.0};
  const int32_t rc = ptx_scene_camera_pose(s, out, out + 3, &v);
  if (rc < 0) return rc;
  out[12] = v.lower_left_x; out[13] = v.lower_left_y; out[14] = v.view_x; out[15] = v.view_y;
  return rc;
}

/* Ptx.set_camera_projection / Ptx.camera_projection: 0 = the pinhole, 1 = the lat-long panorama (ptx_scene_set_camera_projection) */
static __attribute__((unused)) int32_t ptx_ml_set_camera_projection(ptx_scene* s, int32_t projection) {
  return ptx_scene_set_camera_projection(s, projection);
}
static __attribute__((unused)) int32_t ptx_ml_camera_projection(const ptx_scene* s) { return ptx_scene_camera_projection(s); }

/* Ptx.set_camera_shutter / Ptx.clear_camera_shutter / Ptx.camera_shutter: how the camera moves while a frame is exposed
 * (ptx_scene_set_camera_shutter).  motion: the 7 doubles translation (3), axis (3), angle; -4 for any other length (clearing is a call of
 * its own: nothing is switched off by accident). */
static __attribute__((unused)) int32_t ptx_ml_set_camera_shutter(ptx_scene* s, const double* motion, int64_t n_motion) {
  if (n_motion != 7) return -4;
  return ptx_scene_set_camera_shutter(s, motion, motion + 3, motion[6]);
}
static __attribute__((unused)) int32_t ptx_ml_clear_camera_shutter(ptx_scene* s) { return ptx_scene_set_camera_shutter(s, NULL, NULL, 0.0); }
/* out: 7 doubles -- translation, axis, angle; returns 1 = on, 0 = off, or the library's (negative) code; -4 when out is not 7 long
 * (nothing is written) */
static __attribute__((unused)) int32_t ptx_ml_camera_shutter(const ptx_scene* s, double* out, int64_t n_out) {
  if (n_out != 7) return -4;
  return ptx_scene_camera_shutter(s, out, out + 3, out + 6);
}

/* Ptx.render_rays (ptx_render_rays): params3 = max_bounces, rays_per_bin, normalize (0 / 1); origins and directions 3 n doubles each,
 * offsets n int32 or n_offsets = 0 for offset i = i, sums 3 (n / rays_per_bin) doubles, sq as many or n_sq = 0 for none.  -4 for
 * lengths that do not fit together (nothing is read or written); the library's own refusals keep their codes. */
static __attribute__((unused)) int32_t ptx_ml_render_rays(ptx_scene* s, const double* params3, const double* origins, int64_t n_origins,
                                                          const double* directions, int64_t n_directions, const int32_t* offsets,
                                                          int64_t n_offsets, double* sums, int64_t n_sums, double* sq, int64_t n_sq) {
  ptx_rays_params p;
  memset(&p, 0, sizeof p);
  p.max_bounces = (int32_t)params3[0];
  p.rays_per_bin = (int32_t)params3[1];
  p.flags = params3[2] != 0.0 ? PTX_RAYS_NORMALIZE : 0;
  if (n_origins % 3 != 0 || n_directions != n_origins) return -4;
  const int64_t n = n_origins / 3;
  if (n_offsets != 0 && n_offsets != n) return -4;
  if (p.rays_per_bin >= 1 && n % p.rays_per_bin == 0) { /* (otherwise the library refuses the call before it touches the sums) */
    const int64_t want = 3 * (n / p.rays_per_bin);
    if (n_sums != want || (n_sq != 0 && n_sq != want)) return -4;
  }
  return ptx_render_rays(s, &p, n, origins, directions, n_offsets ? offsets : NULL, sums, n_sq ? sq : NULL, NULL);
}

/* Ptx.film_weights: the 2 * pixel_radius + 1 weights into out (n_out doubles); -4 when out is too short for an accepted film (the
 * library's own refusals keep their codes, and nothing is written) */
static __attribute__((unused)) int32_t ptx_ml_film_weights(int32_t order, int32_t pixel_radius, double* out, int64_t n_out) {
  ptx_film_params f;
  memset(&f, 0, sizeof f);
  f.order = order;
  f.pixel_radius = pixel_radius;
  double w[2 * PTX_FILM_MAX_RADIUS + 1];
  const int32_t rc = ptx_film_weights(&f, w, NULL);
  if (rc != 0) return rc;
  if (!out || n_out < 2 * pixel_radius + 1) return -4;
  memcpy(out, w, sizeof(double) * (size_t)(2 * pixel_radius + 1));
  return 0;
}

/* Ptx.set_texture_image / Ptx.clear_texture_image: width * height * 3 doubles of `rgb` (n_rgb of them are there) onto entry `index`
 * of the scene's texture table (ptx_scene_set_texture_image); width = height = 0 restores the descriptor's texture.  -4 when an
 * accepted size needs more texels than the Bigarray holds (the library's own refusals keep their codes: it checks the size before it
 * reads a texel). */
static __attribute__((unused)) int32_t ptx_ml_set_texture_image(ptx_scene* s, int32_t index, int32_t width, int32_t height, int32_t flags,
                                                                const double* rgb, int64_t n_rgb) {
  if (width == 0 && height == 0) return ptx_scene_set_texture_image(s, index, NULL);
  ptx_image img;
  memset(&img, 0, sizeof img);
  img.width = width;
  img.height = height;
  img.flags = flags;
  img.rgb = rgb;
  const int sized = width >= 1 && width <= PTX_IMAGE_MAX_SIZE && height >= 1 && height <= PTX_IMAGE_MAX_SIZE;
  if (sized && (!rgb || n_rgb < (int64_t)width * height * 3)) return -4;
  return ptx_scene_set_texture_image(s, index, &img);
}

/* Ptx.set_environment / Ptx.clear_environment (ptx_scene_set_environment): as above; rot = 9 doubles row-major, or n_rot = 0 for
 * the identity; -5 for any other length */
static __attribute__((unused)) int32_t ptx_ml_set_environment(ptx_scene* s, int32_t width, int32_t height, int32_t flags, const double* rgb,
                                                              int64_t n_rgb, const double* rot, int64_t n_rot) {
  if (width == 0 && height == 0) return ptx_scene_set_environment(s, NULL, NULL);
  if (n_rot != 0 && n_rot != 9) return -5;
  ptx_image img;
  memset(&img, 0, sizeof img);
  img.width = width;
  img.height = height;
  img.flags = flags;
  img.rgb = rgb;
  const int sized = width >= 1 && width <= PTX_IMAGE_MAX_SIZE && height >= 1 && height <= PTX_IMAGE_MAX_SIZE;
  if (sized && (!rgb || n_rgb < (int64_t)width * height * 3)) return -4;
  return ptx_scene_set_environment(s, &img, n_rot == 9 ? rot : NULL);
}

/* ---- display outputs (include/ptx.h, "display outputs") ----
 * A display as OCaml hands it over: display4 = format, transfer, tone (the PTX_* values as floats), exposure; flags and the reserved
 * words are 0.  The library's checks are the ones that refuse. */
static __attribute__((unused)) void ptx_ml_display(const double* display4, ptx_display_params* out) {
  memset(out, 0, sizeof *out);
  out->format = (int32_t)display4[0];
  out->transfer = (int32_t)display4[1];
  out->tone = (int32_t)display4[2];
  out->exposure = display4[3];
}

/* ptx_display_defaults as the four floats above */
static __attribute__((unused)) int32_t ptx_ml_display_defaults(double* display4) {
  ptx_display_params d;
  const int32_t rc = ptx_display_defaults(&d);
  if (rc != 0) return rc;
  display4[0] = (double)d.format;
  display4[1] = (double)d.transfer;
  display4[2] = (double)d.tone;
  display4[3] = d.exposure;
  return 0;
}

/* the elements of a display image of `format` per pixel (3 or 4: bytes for the 8-bit formats, binary32 values for the others), and
 * whether they are binary32; 0 for an unknown format */
static __attribute__((unused)) int32_t ptx_ml_display_channels(int32_t format, int32_t* is_float) {
  if (is_float) *is_float = format == PTX_PIXEL_RGB32F || format == PTX_PIXEL_RGBA32F;
  if (format == PTX_PIXEL_RGB8 || format == PTX_PIXEL_RGB32F) return 3;
  if (format == PTX_PIXEL_RGBA8 || format == PTX_PIXEL_RGBA32F) return 4;
  return 0;
}

/* Integrator.render whose image comes back as display pixels (ptx_render_display): params9 = width, height, samples_per_pixel,
 * max_bounces, gpus, then display4.  pixels: width * height * channels elements of the format.  -4: the image is too small. */
static __attribute__((unused)) int32_t ptx_ml_render_display(ptx_scene* s, const double* params9, void* pixels, int64_t n_elements,
                                                             ptx_progress_fn progress, void* user) {
  if (!params9) return -1;
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params9[0];
  p.height = (int32_t)params9[1];
  p.samples_per_pixel = (int32_t)params9[2];
  p.max_bounces = (int32_t)params9[3];
  p.n_gpus = (int32_t)params9[4];
  ptx_display_params d;
  ptx_ml_display(params9 + 5, &d);
  const int32_t ch = ptx_ml_display_channels(d.format, NULL);
  if (ch && p.width > 0 && p.height > 0 && n_elements < (int64_t)p.width * p.height * ch) return -4;
  return ptx_render_display(s, &p, &d, pixels, NULL, progress, user);
}

/* ptx_render_progressive_display: params18 = width, height, samples_per_pixel, max_bounces, passes_per_update, target_rel_err, then
 * display4, then denoise (0 = the plain updates of ptx_render_progressive) and the denoiser's levels, normal_power_log2,
 * feature_passes, flags, sigma_luminance, sigma_depth, sigma_albedo (read only when denoise is not 0).  pixels holds the display
 * image of the last update, err (nullable, W*H*3 doubles) its f64 per-pixel standard error, *passes_done its passes.  -4: the
 * image is too small. */
static __attribute__((unused)) int32_t ptx_ml_render_progressive_display(ptx_scene* s, const double* params18, void* pixels, int64_t n_elements,
                                                                         double* err, int32_t* passes_done,
                                                                         ptx_update_display_fn on_update, void* user) {
  if (!params18) return -1;
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = (int32_t)params18[0];
  p.height = (int32_t)params18[1];
  p.samples_per_pixel = (int32_t)params18[2];
  p.max_bounces = (int32_t)params18[3];
  ptx_progressive_params pp;
  memset(&pp, 0, sizeof pp);
  pp.passes_per_update = (int32_t)params18[4];
  pp.want_error = 1;
  pp.target_rel_err = params18[5];
  ptx_display_params d;
  ptx_ml_display(params18 + 6, &d);
  const int32_t ch = ptx_ml_display_channels(d.format, NULL);
  if (ch && p.width > 0 && p.height > 0 && n_elements < (int64_t)p.width * p.height * ch) return -4;
  ptx_denoise_params dn;
  memset(&dn, 0, sizeof dn);
  const int filter = params18[10] != 0.0;
  if (filter) {
    dn.levels = (int32_t)params18[11];
    dn.normal_power_log2 = (int32_t)params18[12];
    dn.feature_passes = (int32_t)params18[13];
    dn.flags = (int32_t)params18[14];
    dn.sigma_luminance = params18[15];
    dn.sigma_depth = params18[16];
    dn.sigma_albedo = params18[17];
  }
  return ptx_render_progressive_display(s, &p, &pp, filter ? &dn : NULL, &d, pixels, err, passes_done, NULL, on_update, user);
}

#endif /* PTX_ML_MARSHAL_H */
