/* Sanitizer driver for the ORACLE (test infrastructure, CPU only): oracle/pt_oracle.c compiled with
 * -fsanitize=address,undefined into this executable and run over the three stock scenes -- scene generators, Shape_tree.create,
 * the tile-parallel path integrator, explicit-ray queries, the photon mapper.  Built by `make asan` in oracle/, run by
 * tests/test_sanitizers.py.  A checker with undefined behaviour in it proves nothing: this keeps it honest. */
#include "pt_oracle.c"

#include <stdio.h>

static int run(orc_desc* od, int w, int h, int spp, int depth, int ppm) {
  const ptx_scene_desc* d = orc_desc_get(od);
  orc_scene* sc = orc_scene_create(d);
  if (!sc) return 1;
  int info[5];
  double ms;
  orc_scene_info(sc, info, &ms);
  double* rgb = (double*)calloc((size_t)w * h * 3, sizeof(double));
  double* raw = (double*)calloc((size_t)w * h * 3, sizeof(double));
  int64_t ct[5];
  double rms = 0.0;
  if (orc_render(sc, w, h, spp, depth, 3, rgb, raw, ct, &rms) != 0) return 2;
  double o[6] = {0, 0, 0, 0.1, 0.2, 5.0}, dir[6] = {0.01, -0.02, -1.0, 0.0, 0.0, -1.0}, t[2];
  int32_t prim[2];
  int64_t ct2[5];
  orc_intersect_rays(sc, 2, o, dir, t, prim, ct2);
  if (ppm) {
    ptx_ppm_params p;
    memset(&p, 0, sizeof p);
    p.width = w; p.height = h; p.iterations = 2; p.max_bounces = 4; p.photon_count = 3000; p.alpha = 2.0 / 3.0;
    ptx_light lights[2];
    const int nl = ppm == 1 ? orc_lights_cornell(w, h, lights) : orc_lights_ganesha(sc, lights);
    int64_t st[4];
    double radius;
    memset(raw, 0, sizeof(double) * (size_t)w * h * 3);
    if (orc_ppm_render(sc, &p, lights, nl, raw, st, &radius) != 0) return 3;
    { /* the two read-only exports (photon list, eye records) of the last iteration: same run, same image */
      const int64_t cap = (int64_t)p.photon_count * p.max_bounces;
      double* ph = (double*)calloc((size_t)cap * 9, sizeof(double));
      int32_t* paths = (int32_t*)calloc((size_t)cap, sizeof(int32_t));
      int32_t* diffuse = (int32_t*)calloc((size_t)w * h, sizeof(int32_t));
      double* eye = (double*)calloc((size_t)w * h * 12, sizeof(double));
      int64_t* nb = (int64_t*)calloc((size_t)w * h, sizeof(int64_t));
      double* img2 = (double*)calloc((size_t)w * h * 3, sizeof(double));
      double dump_info[2];
      int64_t st2[4];
      const int64_t n = orc_ppm_dump(sc, &p, lights, nl, 1, cap, ph, paths, diffuse, eye, nb, dump_info, img2, st2);
      const int same = n > 0 && n <= cap && memcmp(img2, raw, sizeof(double) * (size_t)w * h * 3) == 0 && memcmp(st, st2, sizeof st) == 0 &&
                       dump_info[0] == radius;
      /* a cap smaller than the list: nothing past it may be written */
      const int64_t n_small = orc_ppm_dump(sc, &p, lights, nl, 0, 1, ph, paths, diffuse, eye, nb, dump_info, img2, st2);
      free(img2); free(ph); free(paths); free(diffuse); free(eye); free(nb);
      if (!same || n_small <= 0) return 4;
    }
  }
  printf("nodes %d depth %d segments %lld first %.6f\n", info[0], info[2], (long long)ct[1], rgb[0]);
  free(rgb);
  free(raw);
  orc_scene_destroy(sc);
  orc_desc_destroy(od);
  return 0;
}

int main(void) {
  int rc = 0;
  for (int math = 0; math < 2; ++math) {
    orc_set_math(math);
    rc |= run(orc_desc_shirley(48, 24, 0, 42), 48, 24, 2, 8, 0);
    rc |= run(orc_desc_shirley(48, 24, 1, 42), 48, 24, 2, 8, 0);
  }
  orc_set_math(0);
  rc |= run(orc_desc_cornell(32, 32, 12.0), 32, 32, 2, 16, 1);
  rc |= run(orc_desc_ganesha_like(48, 27, 2000, 7), 48, 27, 2, 8, 2);
  return rc;
}
