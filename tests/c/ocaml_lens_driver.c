/* Drives the calls ptx_stubs.c's set_lens / lens stubs make, through bindings/ocaml/ptx_ml_marshal.h and the real C ABI on a host-only
 * scene (device -1: no HIP call): one sphere.  Prints one line per step, "name rc [radius focus | the library's message]";
 * tests/test_ocaml_lens.py reads them. */
#include <math.h>
#include <stdio.h>

#include "ptx_ml_marshal.h"

static int32_t set(ptx_scene* s, double radius, double focus) {
  const double pair[2] = {radius, focus};
  return ptx_ml_set_lens(s, pair, 2);
}

static void line(const char* name, int32_t rc, ptx_scene* s) {
  double radius = -1.0, focus = -1.0;
  if (rc != 0) {
    printf("%s %d %s\n", name, rc, ptx_last_error());
    return;
  }
  if (ptx_ml_lens(s, &radius, &focus) != 0) radius = -2.0;
  printf("%s 0 %a %a\n", name, radius, focus);
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
  line("initial", 0, s);
  line("set", set(s, 0.05, 13.5), s);
  line("negative", set(s, -1.0, 2.0), s);
  line("nan", set(s, NAN, 2.0), s);
  line("no_focus", set(s, 0.25, 0.0), s);
  line("inf_focus", set(s, 0.25, INFINITY), s);
  line("kept", 0, s);
  line("off", set(s, 0.0, 3.0), s);
  line("null", set(NULL, 0.1, 1.0), s);
  {
    const double three[3] = {0.1, 1.0, 2.0};
    printf("short %d\n", ptx_ml_set_lens(s, three, 1));
    printf("long %d\n", ptx_ml_set_lens(s, three, 3));
  }
  ptx_scene_destroy(s);
  return 0;
}
