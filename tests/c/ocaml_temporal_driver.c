/* Drives the calls ptx_stubs.c's render_temporal / temporal_reset stubs make, through bindings/ocaml/ptx_ml_marshal.h and the real C
 * ABI.  Without an argument: on a host-only scene (device -1: no HIP call), the refusals.  With a device number: frames of a short
 * sequence rendered through ptx_ml_render_temporal's 18 floats and, on a second handle, through ptx_render_temporal with the structs
 * filled in by hand, compared byte for byte; then settings the library refuses, which name the field every slot lands in.  Prints
 * one line per step; tests/test_ocaml_temporal.py reads them. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "ptx_ml_marshal.h"

enum { W = 16, H = 8, N = 16, K = 4, DEPTH = 4 };

static const double kDefaults[18] = {W, H, N, DEPTH, 0, K, 64.0, 0.9, 0.02, 0x1p-10, 0.0, 5, 5, 0, 1, 4.0, 0.05, 0.2};

static void refusal(const char* name, ptx_scene* s, int slot, double v) {
  double p[18], img[W * H * 3];
  memcpy(p, kDefaults, sizeof p);
  p[slot] = v;
  const int32_t rc = ptx_ml_render_temporal(s, p, img, NULL, NULL, NULL);
  printf("%s %d %s\n", name, rc, rc ? ptx_last_error() : "-");
}

int main(int argc, char** argv) {
  const int device = argc > 1 ? atoi(argv[1]) : -1;
  const double x = 0.0, y = 0.0, z = -3.0, r = 1.0;
  const int32_t sphere_material = 0;
  ptx_material mat;
  ptx_texture tex;
  memset(&mat, 0, sizeof mat);
  memset(&tex, 0, sizeof tex);
  mat.kind = PTX_MAT_LAMBERTIAN;
  tex.kind = PTX_TEX_SOLID;
  tex.even[0] = 0.8; tex.even[1] = 0.3; tex.even[2] = 0.3;
  ptx_scene_desc d;
  memset(&d, 0, sizeof d);
  d.n_spheres = 1;
  d.sphere_x = &x; d.sphere_y = &y; d.sphere_z = &z; d.sphere_r = &r; d.sphere_material = &sphere_material;
  d.n_materials = 1; d.materials = &mat;
  d.n_textures = 1; d.textures = &tex;
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -0.5; d.camera.view_x = 2.0; d.camera.view_y = 1.0;
  d.background.kind = PTX_BG_SKY;
  d.background.horizon[0] = d.background.horizon[1] = d.background.horizon[2] = 1.0;
  d.background.zenith[0] = 0.5; d.background.zenith[1] = 0.7; d.background.zenith[2] = 1.0;
  d.leaf_kind = PTX_LEAF_ARRAY; d.length_cutoff = 4;
  double img[W * H * 3];
  if (device < 0) {
    ptx_scene* s = ptx_scene_create(&d, -1);
    if (!s) {
      fprintf(stderr, "%s\n", ptx_last_error());
      return 2;
    }
    printf("null_params %d\n", ptx_ml_render_temporal(s, NULL, img, NULL, NULL, NULL));
    refusal("host_only", s, 0, W);
    refusal("null_scene", NULL, 0, W);
    printf("reset %d\n", ptx_ml_temporal_reset(s));
    {
      const int32_t rc = ptx_ml_temporal_reset(NULL);
      printf("reset_null %d %s\n", rc, ptx_last_error());
    }
    ptx_scene_destroy(s);
    return 0;
  }
  ptx_scene* a = ptx_scene_create(&d, device);
  ptx_scene* b = ptx_scene_create(&d, device);
  if (!a || !b) {
    fprintf(stderr, "%s\n", ptx_last_error());
    return 2;
  }
  /* settings off the defaults in every slot, so that a slot read from the wrong place shows */
  const double cap = 24.0, nthr = 0.8, dtol = 0.05, minw = 0x1p-6;
  for (int f = 0; f < 3; ++f) {
    const int denoise = f == 2;
    double p[18], err_a[W * H * 3], mot_a[W * H * 3], img_b[W * H * 3], err_b[W * H * 3], mot_b[W * H * 3];
    memcpy(p, kDefaults, sizeof p);
    p[4] = f * K;
    p[6] = cap; p[7] = nthr; p[8] = dtol; p[9] = minw;
    p[10] = denoise;
    p[11] = 2; p[12] = 3; p[14] = 0; p[15] = 3.0; p[16] = 0.1; p[17] = 0.3;
    int64_t took_a = -1, took_b = -1;
    const int32_t rc_a = ptx_ml_render_temporal(a, p, img, err_a, mot_a, &took_a);
    ptx_render_params rp;
    memset(&rp, 0, sizeof rp);
    rp.width = W; rp.height = H; rp.samples_per_pixel = N; rp.max_bounces = DEPTH;
    ptx_temporal_params tp = {cap, nthr, dtol, minw};
    ptx_denoise_params dn;
    memset(&dn, 0, sizeof dn);
    dn.levels = 2; dn.normal_power_log2 = 3; dn.feature_passes = 0; dn.flags = 0;
    dn.sigma_luminance = 3.0; dn.sigma_depth = 0.1; dn.sigma_albedo = 0.3;
    const int32_t rc_b = ptx_render_temporal(b, &rp, &tp, denoise ? &dn : NULL, f * K, K, img_b, err_b, mot_b, &took_b, NULL);
    const int same = !memcmp(img, img_b, sizeof img) && !memcmp(err_a, err_b, sizeof err_a) && !memcmp(mot_a, mot_b, sizeof mot_a);
    double top = 0.0;
    for (int i = 0; i < W * H * 3; ++i) top = fmax(top, img[i]);
    printf("frame%d %d %d %d %lld %lld %a\n", f, rc_a, rc_b, same, (long long)took_a, (long long)took_b, top);
  }
  refusal("bad_width", a, 0, 0.0);
  refusal("bad_height", a, 1, -1.0);
  refusal("bad_spp", a, 2, 0.0);
  refusal("bad_depth", a, 3, 127.0);
  refusal("bad_first", a, 4, N - 2);
  refusal("bad_count", a, 5, 1.0);
  refusal("bad_cap", a, 6, -1.0);
  refusal("bad_threshold", a, 7, 1.5);
  refusal("bad_tolerance", a, 8, -1.0);
  refusal("bad_weight", a, 9, 1.0);
  refusal("unread_denoiser", a, 11, 99.0); /* denoise = 0: the denoiser's slots are not read */
  {
    double p[18];
    const struct { const char* name; int slot; double v; } bad[] = {{"bad_levels", 11, 9.0}, {"bad_power", 12, 9.0}, {"bad_passes", 13, -1.0},
                                                                   {"bad_flags", 14, 2.0}, {"bad_sigma_l", 15, 0.0}, {"bad_sigma_z", 16, -1.0},
                                                                   {"bad_sigma_a", 17, NAN}};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
      memcpy(p, kDefaults, sizeof p);
      p[10] = 1.0;
      p[bad[i].slot] = bad[i].v;
      const int32_t rc = ptx_ml_render_temporal(a, p, img, NULL, NULL, NULL);
      printf("%s %d %s\n", bad[i].name, rc, rc ? ptx_last_error() : "-");
    }
  }
  {
    int64_t took = -1;
    double p[18];
    memcpy(p, kDefaults, sizeof p);
    printf("reset %d\n", ptx_ml_temporal_reset(a));
    const int32_t rc = ptx_ml_render_temporal(a, p, img, NULL, NULL, &took);
    printf("after_reset %d %lld\n", rc, (long long)took);
  }
  ptx_scene_destroy(a);
  ptx_scene_destroy(b);
  return 0;
}
