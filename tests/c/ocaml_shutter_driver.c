/* Drives the calls ptx_stubs.c's set_camera_shutter / clear_camera_shutter / camera_shutter stubs make, through
 * bindings/ocaml/ptx_ml_marshal.h and the real C ABI on a host-only scene (device -1: no HIP call): one sphere.  Prints one line per
 * step, "name rc [on and the 7 doubles | the library's message]"; tests/test_ocaml_shutter.py reads them. */
#include <math.h>
#include <stdio.h>

#include "ptx_ml_marshal.h"

static void line(const char* name, int32_t rc, ptx_scene* s) {
  double out[7];
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, ptx_last_error());
    return;
  }
  const int32_t on = ptx_ml_camera_shutter(s, out, 7);
  printf("%s 0 %d", name, on);
  for (int i = 0; i < 7; ++i) printf(" %a", out[i]);
  printf("\n");
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
  const double motion[7] = {0.25, -1.5, 0x1.23456789abcdep+3, 0.6, 0.0, -0.8, -0x1.8p-1};
  const double still[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double bad[7];
  line("initial", 0, s);
  line("set", ptx_ml_set_camera_shutter(s, motion, 7), s);
  memcpy(bad, motion, sizeof bad);
  bad[1] = NAN;
  line("nan_translation", ptx_ml_set_camera_shutter(s, bad, 7), s);
  memcpy(bad, motion, sizeof bad);
  bad[3] = 0.7;
  line("not_unit", ptx_ml_set_camera_shutter(s, bad, 7), s);
  memcpy(bad, motion, sizeof bad);
  bad[6] = 3.5;
  line("wide_angle", ptx_ml_set_camera_shutter(s, bad, 7), s);
  line("kept", 0, s);
  line("still", ptx_ml_set_camera_shutter(s, still, 7), s);
  line("clear", ptx_ml_clear_camera_shutter(s), s);
  line("null", ptx_ml_clear_camera_shutter(NULL), s);
  printf("short_motion %d\n", ptx_ml_set_camera_shutter(s, motion, 6));
  printf("long_motion %d\n", ptx_ml_set_camera_shutter(s, motion, 8));
  {
    double out[7];
    printf("short_out %d\n", ptx_ml_camera_shutter(s, out, 6));
  }
  line("still_clear", 0, s);
  ptx_scene_destroy(s);
  return 0;
}
