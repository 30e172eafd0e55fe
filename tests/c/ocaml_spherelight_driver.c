/* Drives the calls ptx_stubs.c's set_sphere_light_sampling / sphere_lights stubs make through the real C ABI on host-only scenes
 * (device -1: no HIP call): one sphere that does not emit, then one that does.  Prints one line per step,
 * "name rc [on n total | the library's message]"; tests/test_ocaml_spherelight.py reads them. */
#include <stdio.h>
#include <string.h>

#include "ptx.h"

static void line(const char* name, int32_t rc, ptx_scene* s) {
  int32_t on = -1, n = -1;
  double total = -1.0;
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, ptx_last_error());
    return;
  }
  if (ptx_scene_sphere_lights(s, &on, &n, &total) != 0) on = -2;
  printf("%s 0 %d %d %a\n", name, on, n, total);
}

static ptx_scene* scene(double emit) {
  static const double x = 0.0, y = 0.0, z = -3.0, r = 0.5;
  static const int32_t sphere_material = 0;
  static ptx_material mat;
  static ptx_texture tex;
  memset(&mat, 0, sizeof mat);
  memset(&tex, 0, sizeof tex);
  mat.kind = PTX_MAT_LAMBERTIAN;
  mat.emit[0] = mat.emit[1] = mat.emit[2] = emit;
  ptx_scene_desc d;
  memset(&d, 0, sizeof d);
  d.n_spheres = 1;
  d.sphere_x = &x; d.sphere_y = &y; d.sphere_z = &z; d.sphere_r = &r; d.sphere_material = &sphere_material;
  d.n_materials = 1; d.materials = &mat;
  d.n_textures = 1; d.textures = &tex;
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -1.0; d.camera.view_x = 2.0; d.camera.view_y = 2.0;
  d.leaf_kind = PTX_LEAF_ARRAY; d.length_cutoff = 4;
  return ptx_scene_create(&d, -1);
}

int main(void) {
  ptx_scene* s = scene(0.0);
  if (!s) return 2;
  line("initial", 0, s);
  line("dark", ptx_scene_set_sphere_light_sampling(s, 1), s);
  ptx_scene_destroy(s);
  s = scene(3.0);
  if (!s) return 2;
  line("lighting_refused", ptx_scene_set_lighting(s, PTX_LIGHTING_SAMPLED), s);
  line("on", ptx_scene_set_sphere_light_sampling(s, 1), s);
  line("lighting", ptx_scene_set_lighting(s, PTX_LIGHTING_SAMPLED), s);
  line("off_refused", ptx_scene_set_sphere_light_sampling(s, 0), s);
  line("kept", 0, s);
  line("path_order", ptx_scene_set_lighting(s, PTX_LIGHTING_PATH_ORDER), s);
  line("off", ptx_scene_set_sphere_light_sampling(s, 0), s);
  ptx_scene_destroy(s);
  return 0;
}
