/* Drives the calls ptx_stubs.c's set_environment_sampling / environment_sampling stubs make, behind the image marshalling of
 * bindings/ocaml/ptx_ml_marshal.h, through the real C ABI on a host-only scene (device -1: no HIP call): one sphere, no emitter.
 * Prints one line per step, "name rc [on total | the library's message]"; tests/test_ocaml_envlight.py reads them. */
#include <stdio.h>

#include "ptx_ml_marshal.h"

static void line(const char* name, int32_t rc, ptx_scene* s) {
  int32_t on = -1;
  double total = -1.0;
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, ptx_last_error());
    return;
  }
  if (ptx_scene_environment_sampling(s, &on, &total) != 0) on = -2;
  printf("%s 0 %d %a\n", name, on, total);
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
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -1.0; d.camera.view_x = 2.0; d.camera.view_y = 2.0;
  d.leaf_kind = PTX_LEAF_ARRAY; d.length_cutoff = 4;
  ptx_scene* s = ptx_scene_create(&d, -1);
  if (!s) {
    fprintf(stderr, "%s\n", ptx_last_error());
    return 2;
  }
  double texels[2 * 1 * 3] = {1.0, 1.0, 1.0, 0.5, 0.25, 0.25}, rot[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0}, skew[9] = {1, 0, 0, 0, 1, 0, 0, 0.5, 1};
  line("initial", 0, s);
  line("no_env", ptx_scene_set_environment_sampling(s, 1), s);
  line("lighting_refused", ptx_scene_set_lighting(s, PTX_LIGHTING_SAMPLED), s);
  if (ptx_ml_set_environment(s, 2, 1, PTX_IMAGE_BILINEAR, texels, 6, skew, 9) != 0) return 3;
  line("skew", ptx_scene_set_environment_sampling(s, 1), s);
  if (ptx_ml_set_environment(s, 2, 1, PTX_IMAGE_BILINEAR, texels, 6, rot, 9) != 0) return 3;
  line("on", ptx_scene_set_environment_sampling(s, 1), s);
  line("lighting", ptx_scene_set_lighting(s, PTX_LIGHTING_SAMPLED), s);
  line("off_refused", ptx_scene_set_environment_sampling(s, 0), s);
  line("clear_refused", ptx_ml_set_environment(s, 0, 0, 0, NULL, 0, NULL, 0), s);
  line("kept", 0, s);
  line("path_order", ptx_scene_set_lighting(s, PTX_LIGHTING_PATH_ORDER), s);
  line("off", ptx_scene_set_environment_sampling(s, 0), s);
  ptx_scene_destroy(s);
  return 0;
}
