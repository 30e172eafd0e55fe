/* Drives the calls ptx_stubs.c's display stubs make (display_defaults, render_display, render_progressive_display), through
 * bindings/ocaml/ptx_ml_marshal.h and the real C ABI.  Without an argument: the defaults, the channel counts, and on a host-only
 * scene (device -1: no HIP call) the refusals, which name the field every slot lands in.  With a device number: a frame through the
 * marshalled floats in every format against ptx_render + ptx_display_apply with the structs filled in by hand, byte for byte, and
 * the same for the last update of the progressive and denoised forms.  Prints one line per step; tests/test_ocaml_display.py reads
 * them. */
#include <stdio.h>
#include <stdlib.h>

#include "ptx_ml_marshal.h"

enum { W = 16, H = 8, N = 4, K = 2, DEPTH = 3 };

/* width, height, spp, depth, gpus, then format, transfer, tone, exposure */
static const double kRender[9] = {W, H, N, DEPTH, 1, PTX_PIXEL_RGBA8, PTX_TRANSFER_SRGB, PTX_TONE_ACES, 0.5};
/* width, height, spp, depth, K, target, display4, denoise, then the denoiser's seven */
static const double kUpdates[18] = {W, H, N, DEPTH, K, 0.0, PTX_PIXEL_RGBA8, PTX_TRANSFER_SRGB, PTX_TONE_ACES, 0.5, 0.0, 5, 5, 0, 1, 4.0, 0.05, 0.2};

static unsigned char g_out[W * H * 16 + 16]; /* the largest format, and a margin that must keep its fill */

static void refuse_render(const char* name, ptx_scene* s, int slot, double v) {
  double p[9];
  memcpy(p, kRender, sizeof p);
  p[slot] = v;
  const int32_t rc = ptx_ml_render_display(s, p, g_out, W * H * 4, NULL, NULL);
  printf("%s %d %s\n", name, rc, rc ? ptx_last_error() : "-");
}

static void refuse_updates(const char* name, ptx_scene* s, int slot, double v, int denoise) {
  double p[18];
  memcpy(p, kUpdates, sizeof p);
  p[10] = denoise;
  p[slot] = v;
  int32_t done = -1;
  const int32_t rc = ptx_ml_render_progressive_display(s, p, g_out, W * H * 4, NULL, &done, NULL, NULL);
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
  if (device < 0) {
    double d4[4] = {-1, -1, -1, -1};
    const int32_t rc_defaults = ptx_ml_display_defaults(d4);
    printf("defaults %d %g %g %g %g\n", rc_defaults, d4[0], d4[1], d4[2], d4[3]);
    for (int f = -1; f <= 4; ++f) {
      int32_t is_float = -1;
      const int32_t ch = ptx_ml_display_channels(f, &is_float);
      printf("channels%d %d %d\n", f, ch, is_float);
    }
    ptx_scene* s = ptx_scene_create(&d, -1);
    if (!s) {
      fprintf(stderr, "%s\n", ptx_last_error());
      return 2;
    }
    printf("null_params %d %d\n", ptx_ml_render_display(s, NULL, g_out, W * H * 4, NULL, NULL),
           ptx_ml_render_progressive_display(s, NULL, g_out, W * H * 4, NULL, NULL, NULL, NULL));
    /* the display slots are checked before the scene is looked at: every one lands in its field */
    refuse_render("host_only", s, 0, W);
    refuse_render("null_scene", NULL, 0, W);
    refuse_render("bad_format", s, 5, 9);
    refuse_render("bad_transfer", s, 6, 7);
    refuse_render("bad_tone", s, 7, 5);
    refuse_render("bad_exposure", s, 8, -1.0);
    refuse_render("reference_tone", s, 6, PTX_TRANSFER_REFERENCE);
    refuse_render("f32_srgb", s, 5, PTX_PIXEL_RGB32F);
    {
      double p[9];
      memcpy(p, kRender, sizeof p);
      printf("small %d\n", ptx_ml_render_display(s, p, g_out, W * H * 4 - 1, NULL, NULL));
      p[5] = PTX_PIXEL_RGB8; /* three channels: the same image is now large enough, and the scene refuses */
      printf("small_rgb8 %d\n", ptx_ml_render_display(s, p, g_out, W * H * 3, NULL, NULL));
    }
    refuse_updates("u_host_only", s, 0, W, 0);
    refuse_updates("u_bad_format", s, 6, 9, 0);
    refuse_updates("u_bad_transfer", s, 7, 7, 0);
    refuse_updates("u_bad_tone", s, 8, 5, 0);
    refuse_updates("u_bad_exposure", s, 9, -1.0, 1);
    {
      double p[18];
      memcpy(p, kUpdates, sizeof p);
      printf("u_small %d\n", ptx_ml_render_progressive_display(s, p, g_out, W * H * 4 - 1, NULL, NULL, NULL, NULL));
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
  static double rgb[W * H * 3];
  static unsigned char want[W * H * 16];
  ptx_render_params p;
  memset(&p, 0, sizeof p);
  p.width = W; p.height = H; p.samples_per_pixel = N; p.max_bounces = DEPTH; p.n_gpus = 1;
  const int32_t rc_f64 = ptx_render(b, &p, rgb, NULL, NULL, NULL);
  /* every format, with settings off the defaults in every slot */
  const double settings[4][4] = {{PTX_PIXEL_RGB8, PTX_TRANSFER_REFERENCE, PTX_TONE_NONE, 1.0},
                                 {PTX_PIXEL_RGBA8, PTX_TRANSFER_SRGB, PTX_TONE_ACES, 0.5},
                                 {PTX_PIXEL_RGB32F, PTX_TRANSFER_LINEAR, PTX_TONE_REINHARD, 2.0},
                                 {PTX_PIXEL_RGBA32F, PTX_TRANSFER_LINEAR, PTX_TONE_NONE, 0.25}};
  for (int f = 0; f < 4; ++f) {
    double q[9];
    memcpy(q, kRender, sizeof q);
    memcpy(q + 5, settings[f], sizeof settings[f]);
    ptx_display_params dp;
    memset(&dp, 0, sizeof dp);
    dp.format = (int32_t)settings[f][0]; dp.transfer = (int32_t)settings[f][1]; dp.tone = (int32_t)settings[f][2];
    dp.exposure = settings[f][3];
    const size_t bytes = (size_t)W * H * (size_t)ptx_display_pixel_bytes(dp.format);
    int32_t is_float = 0;
    const int64_t elements = (int64_t)W * H * ptx_ml_display_channels(dp.format, &is_float);
    memset(g_out, 0xA5, sizeof g_out);
    const int32_t rc_a = ptx_ml_render_display(a, q, g_out, elements, NULL, NULL);
    const int32_t rc_b = ptx_display_apply(&dp, W * H, rgb, want);
    int lit = 0;
    for (size_t k = 0; k < bytes; ++k) lit += want[k] != 0;
    printf("frame%d %d %d %d %d %d %d\n", f, rc_a, rc_b | rc_f64, memcmp(g_out, want, bytes) == 0, g_out[bytes] == 0xA5,
           elements * (is_float ? 4 : 1) == (int64_t)bytes, lit > 0);
  }
  /* the updates: the last one is the display of ptx_render's image; with the filter, of ptx_render_denoised's */
  for (int denoise = 0; denoise <= 1; ++denoise) {
    double q[18];
    memcpy(q, kUpdates, sizeof q);
    q[10] = denoise;
    q[11] = 2; q[12] = 3; q[14] = 0; q[15] = 3.0; q[16] = 0.1; q[17] = 0.3;
    ptx_display_params dp;
    ptx_ml_display(q + 6, &dp);
    static double err_a[W * H * 3], err_b[W * H * 3];
    int32_t done_a = -1, done_b = -1;
    const int32_t rc_a = ptx_ml_render_progressive_display(a, q, g_out, W * H * 4, err_a, &done_a, NULL, NULL);
    ptx_progressive_params pp;
    memset(&pp, 0, sizeof pp);
    pp.passes_per_update = K; pp.want_error = 1;
    ptx_denoise_params dn;
    memset(&dn, 0, sizeof dn);
    dn.levels = 2; dn.normal_power_log2 = 3; dn.feature_passes = 0; dn.flags = 0;
    dn.sigma_luminance = 3.0; dn.sigma_depth = 0.1; dn.sigma_albedo = 0.3;
    const int32_t rc_b = denoise ? ptx_render_denoised(b, &p, &pp, &dn, rgb, err_b, NULL, &done_b, NULL, NULL, NULL)
                                 : ptx_render_progressive(b, &p, &pp, rgb, err_b, &done_b, NULL, NULL, NULL);
    const int32_t rc_c = ptx_display_apply(&dp, W * H, rgb, want);
    printf("updates%d %d %d %d %d %d %d\n", denoise, rc_a, rc_b | rc_c, memcmp(g_out, want, (size_t)W * H * 4) == 0,
           memcmp(err_a, err_b, sizeof err_a) == 0, done_a, done_b);
  }
  refuse_updates("bad_levels", a, 11, 9, 1);
  refuse_updates("bad_sigma_a", a, 17, -1.0, 1);
  refuse_updates("unread_denoiser", a, 11, 99, 0);
  ptx_scene_destroy(a);
  ptx_scene_destroy(b);
  return 0;
}
