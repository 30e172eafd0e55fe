/* Drives the calls ptx_stubs.c's set_camera_projection / camera_projection / render_rays stubs make, through
 * bindings/ocaml/ptx_ml_marshal.h and the real C ABI on a host-only scene (device -1: no HIP call): one sphere.  Prints one line per
 * step, "name rc [projection | the library's message]"; tests/test_ocaml_rays.py reads them. */
#include <math.h>
#include <stdio.h>

#include "ptx_ml_marshal.h"

static void line(const char* name, int32_t rc, ptx_scene* s) {
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, ptx_last_error());
    return;
  }
  printf("%s 0 %d\n", name, ptx_ml_camera_projection(s));
}

int main(void) {
  const double x = 0.0, y = 0.0, z = -3.0, r = 1.0;
  const int32_t sphere_material = 0;
  ptx_material mat;
  ptx_texture tex;
  memset(&mat, 0, sizeof mat);
  memset(&tex, 0, sizeof tex);
  mat.kind = PTX_MAT_LAMBERTIAN;
  ptx_scene_desc d;
  memset(&d, 0, sizeof d);
  d.n_spheres = 1;
  d.sphere_x = &x; d.sphere_y = &y; d.sphere_z = &z; d.sphere_r = &r; d.sphere_material = &sphere_material;
  d.n_materials = 1; d.materials = &mat;
  d.n_textures = 1; d.textures = &tex;
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -0.5; d.camera.view_x = 2.0; d.camera.view_y = 1.0;
  d.leaf_kind = PTX_LEAF_ARRAY; d.length_cutoff = 4;
  ptx_scene* s = ptx_scene_create(&d, -1);
  if (!s) {
    fprintf(stderr, "%s\n", ptx_last_error());
    return 2;
  }
  /* ---- the projection */
  line("initial", 0, s);
  line("latlong", ptx_ml_set_camera_projection(s, 1), s);
  line("unknown", ptx_ml_set_camera_projection(s, 2), s);
  line("kept", 0, s);
  {
    const double lens[2] = {0.05, 3.0};
    line("lens_under_latlong", ptx_ml_set_lens(s, lens, 2), s);
    line("perspective", ptx_ml_set_camera_projection(s, 0), s);
    line("lens", ptx_ml_set_lens(s, lens, 2), s);
    line("latlong_under_lens", ptx_ml_set_camera_projection(s, 1), s);
    const double off[2] = {0.0, 1.0};
    line("lens_off", ptx_ml_set_lens(s, off, 2), s);
  }
  line("null", ptx_ml_set_camera_projection(NULL, 1), s);
  printf("null_get %d\n", ptx_ml_camera_projection(NULL));
  /* ---- the rays: 4 rays, lengths checked before anything is read; valid lengths reach the library, which refuses a host-only scene */
  const double o[12] = {0}, dir[12] = {0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1};
  const int32_t off4[4] = {0, 1, 2, 2147483646};
  double sums[12] = {0}, sq[12] = {0};
  const double p_one[3] = {4.0, 1.0, 0.0}, p_two[3] = {4.0, 2.0, 1.0}, p_three[3] = {4.0, 3.0, 0.0}, p_zero[3] = {4.0, 0.0, 0.0};
  printf("ragged_origins %d\n", ptx_ml_render_rays(s, p_one, o, 11, dir, 11, NULL, 0, sums, 9, NULL, 0));
  printf("short_directions %d\n", ptx_ml_render_rays(s, p_one, o, 12, dir, 9, NULL, 0, sums, 12, NULL, 0));
  printf("short_offsets %d\n", ptx_ml_render_rays(s, p_one, o, 12, dir, 12, off4, 3, sums, 12, NULL, 0));
  printf("short_sums %d\n", ptx_ml_render_rays(s, p_one, o, 12, dir, 12, off4, 4, sums, 6, NULL, 0));
  printf("long_sums_for_bins %d\n", ptx_ml_render_rays(s, p_two, o, 12, dir, 12, off4, 4, sums, 12, NULL, 0));
  printf("short_squares %d\n", ptx_ml_render_rays(s, p_two, o, 12, dir, 12, off4, 4, sums, 6, sq, 3));
  line("host_only", ptx_ml_render_rays(s, p_one, o, 12, dir, 12, off4, 4, sums, 12, sq, 12), s);
  line("host_only_bins", ptx_ml_render_rays(s, p_two, o, 12, dir, 12, NULL, 0, sums, 6, NULL, 0), s);
  line("not_a_multiple", ptx_ml_render_rays(s, p_three, o, 12, dir, 12, NULL, 0, sums, 12, NULL, 0), s);
  line("zero_bin", ptx_ml_render_rays(s, p_zero, o, 12, dir, 12, NULL, 0, sums, 12, NULL, 0), s);
  int touched = 0;
  for (int i = 0; i < 12; ++i) touched += sums[i] != 0.0 || sq[i] != 0.0;
  printf("touched %d\n", touched);
  ptx_scene_destroy(s);
  return 0;
}
