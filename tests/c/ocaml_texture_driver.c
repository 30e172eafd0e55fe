/* Drives the image marshalling of bindings/ocaml/ptx_ml_marshal.h (what ptx_stubs.c's set_texture_image / set_environment stubs
 * delegate to) through the real C ABI on a host-only scene (device -1: no HIP call): one sphere, two texture entries.  Prints one
 * line per step, "name rc [what the getters answer | the library's message]"; tests/test_ocaml_textures.py reads them. */
#include <stdio.h>

#include "ptx_ml_marshal.h"

static void texture_line(const char* name, int32_t rc, ptx_scene* s, int32_t index) {
  ptx_image out;
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, rc == -4 || rc == -5 ? "-" : ptx_last_error());
    return;
  }
  if (ptx_scene_texture_image(s, index, &out) != 0) out.width = out.height = out.flags = -1;
  printf("%s 0 %d %d %d\n", name, out.width, out.height, out.flags);
}
static void environment_line(const char* name, int32_t rc, ptx_scene* s) {
  ptx_image out;
  double R[9];
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, rc == -4 || rc == -5 ? "-" : ptx_last_error());
    return;
  }
  if (ptx_scene_environment(s, &out, R) != 0) out.width = out.height = out.flags = -1;
  printf("%s 0 %d %d %d %g %g %g\n", name, out.width, out.height, out.flags, R[0], R[2], R[8]);
}

int main(void) {
  const double x = 0.0, y = 0.0, z = -3.0, r = 1.0;
  const int32_t sphere_material = 0;
  ptx_material mat;
  ptx_texture tex[2];
  memset(&mat, 0, sizeof mat);
  memset(tex, 0, sizeof tex);
  mat.kind = PTX_MAT_LAMBERTIAN;
  mat.texture = 1;
  tex[1].kind = PTX_TEX_CHECKER;
  tex[1].width = tex[1].height = 5;
  ptx_scene_desc d;
  memset(&d, 0, sizeof d);
  d.n_spheres = 1;
  d.sphere_x = &x; d.sphere_y = &y; d.sphere_z = &z; d.sphere_r = &r; d.sphere_material = &sphere_material;
  d.n_materials = 1; d.materials = &mat;
  d.n_textures = 2; d.textures = tex;
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -1.0; d.camera.view_x = 2.0; d.camera.view_y = 2.0;
  d.leaf_kind = PTX_LEAF_ARRAY; d.length_cutoff = 4;
  ptx_scene* s = ptx_scene_create(&d, -1);
  if (!s) {
    fprintf(stderr, "%s\n", ptx_last_error());
    return 2;
  }
  double texels[2 * 3 * 3], rot[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0};
  for (int i = 0; i < 18; ++i) texels[i] = 0.125 * i;
  texture_line("set", ptx_ml_set_texture_image(s, 1, 3, 2, PTX_IMAGE_BILINEAR | PTX_IMAGE_REPEAT_V, texels, 18), s, 1);
  texture_line("short", ptx_ml_set_texture_image(s, 1, 3, 2, 0, texels, 17), s, 1);
  texture_line("null", ptx_ml_set_texture_image(s, 1, 3, 2, 0, NULL, 0), s, 1);
  texture_line("kept", 0, s, 1);
  texture_line("size", ptx_ml_set_texture_image(s, 1, 16385, 1, 0, texels, 18), s, 1);
  texture_line("flags", ptx_ml_set_texture_image(s, 0, 3, 2, 8, texels, 18), s, 0);
  texture_line("index", ptx_ml_set_texture_image(s, 2, 3, 2, 0, texels, 18), s, 0);
  texels[7] = 1.0 / 0.0;
  texture_line("texel", ptx_ml_set_texture_image(s, 0, 3, 2, 0, texels, 18), s, 0);
  texels[7] = 0.5;
  texture_line("clear", ptx_ml_set_texture_image(s, 1, 0, 0, 0, NULL, 0), s, 1);
  environment_line("env", ptx_ml_set_environment(s, 2, 3, PTX_IMAGE_BILINEAR, texels, 18, rot, 9), s);
  environment_line("env_identity", ptx_ml_set_environment(s, 2, 3, 0, texels, 18, NULL, 0), s);
  environment_line("env_rot_len", ptx_ml_set_environment(s, 2, 3, 0, texels, 18, rot, 8), s);
  environment_line("env_short", ptx_ml_set_environment(s, 3, 3, 0, texels, 18, NULL, 0), s);
  environment_line("env_repeat", ptx_ml_set_environment(s, 2, 3, PTX_IMAGE_REPEAT_U, texels, 18, NULL, 0), s);
  environment_line("env_clear", ptx_ml_set_environment(s, 0, 0, 0, NULL, 0, NULL, 0), s);
  ptx_scene_destroy(s);
  return 0;
}
