/* Drives the calls ptx_stubs.c's set_camera_pose / clear_camera_pose / camera_pose stubs make, through bindings/ocaml/ptx_ml_marshal.h
 * and the real C ABI on a host-only scene (device -1: no HIP call): one sphere.  Prints one line per step, "name rc [the 16 doubles |
 * the library's message]"; tests/test_ocaml_camera_pose.py reads them. */
#include <math.h>
#include <stdio.h>

#include "ptx_ml_marshal.h"

static void line(const char* name, int32_t rc, ptx_scene* s) {
  double out[16];
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, ptx_last_error());
    return;
  }
  const int32_t on = ptx_ml_camera_pose(s, out, 16);
  printf("%s 0 %d", name, on);
  for (int i = 0; i < 16; ++i) printf(" %a", out[i]);
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
  /* a quarter turn about y: x -> -z, z -> x */
  const double pose[12] = {0.25, -1.5, 0x1.23456789abcdep+3, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0};
  const double view[4] = {-0.75, -0.25, 1.5, 0.5};
  double bad[12];
  line("initial", 0, s);
  line("set", ptx_ml_set_camera_pose(s, pose, 12, view, 4), s);
  line("pose_only", ptx_ml_set_camera_pose(s, pose, 12, NULL, 0), s);
  line("view_only", ptx_ml_set_camera_pose(s, NULL, 0, view, 4), s);
  memcpy(bad, pose, sizeof bad);
  bad[1] = NAN;
  line("nan_origin", ptx_ml_set_camera_pose(s, bad, 12, NULL, 0), s);
  memcpy(bad, pose, sizeof bad);
  bad[5] = 1.001;
  line("not_orthonormal", ptx_ml_set_camera_pose(s, bad, 12, NULL, 0), s);
  memcpy(bad, pose, sizeof bad);
  bad[9] = 1.0; /* x -> +z: a reflection */
  line("mirror", ptx_ml_set_camera_pose(s, bad, 12, NULL, 0), s);
  {
    const double inf_view[4] = {-1.0, -1.0, INFINITY, 2.0};
    line("inf_view", ptx_ml_set_camera_pose(s, NULL, 0, inf_view, 4), s);
  }
  line("kept", 0, s);
  line("clear", ptx_ml_clear_camera_pose(s), s);
  line("null", ptx_ml_clear_camera_pose(NULL), s);
  printf("short_pose %d\n", ptx_ml_set_camera_pose(s, pose, 11, NULL, 0));
  printf("long_view %d\n", ptx_ml_set_camera_pose(s, NULL, 0, view, 5));
  printf("nothing %d\n", ptx_ml_set_camera_pose(s, NULL, 0, NULL, 0));
  {
    double out[16];
    printf("short_out %d\n", ptx_ml_camera_pose(s, out, 15));
  }
  line("still_clear", 0, s);
  ptx_scene_destroy(s);
  return 0;
}
