/* rays_oracle.c -- the CPU restatement of ptx_render_rays (include/ptx.h, "radiance along rays the caller owns"), on top of
 * camera_pose_oracle.c, which is included unchanged (and lens_oracle.c, envlight_oracle.c, texture_oracle.c and the oracle through
 * it): this library carries its own copy of the oracle (call this copy's orc_set_math(0) before comparing with the GPU).
 *
 * Written from the header's text, not from the kernels:
 *
 *   ray i = Ray.create o_i d_i, or Ray.create o_i (V3.normalize d_i) with PTX_RAYS_NORMALIZE
 *   the sampler has `dim` dimensions (the caller's: 2 + 2 max_bounces, two more with a lens) and is read at offset_i (NULL: i)
 *   the path is orcn_trace_path -- the one path loop that takes its ray as an argument, whose bounce k reads dimensions 2 + 2 k and
 *   3 + 2 k -- so dimensions 0 and 1 and the lens pair are never read here
 *
 * ORCR_MUT_*: the rule restated WRONGLY in one way, for the CPU tests' sensitivity condition; every comparison with the GPU passes 0.
 *
 * Build: oracle/Makefile's flags (tests/rays_support.py). */
#include "camera_pose_oracle.c"

enum { ORCR_MUT_NONE = 0,
       ORCR_MUT_DIMS_FROM_0 = 1 }; /* bounce k reads dimensions 2 k and 1 + 2 k: the caller's pair is taken for the first bounce's */

/* Per-ray radiance.  rays n x 6 (origin, direction); offsets nullable.  The arguments before `dim` are orcn_trace_samples'.  Returns 0,
 * or -1 when mode 2 has nothing to sample. */
ORC_API int orcr_trace_rays(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height, int env_flags,
                            const double* envR, int mode, int sampling, int dim, int normalize, int mutant, int max_bounces, int64_t n,
                            const double* rays, const int32_t* offsets, double* rgb_out, int64_t* segments_out) {
  if (mode < 0 || mode > 2 || (sampling && !env_rgb)) return -1;
  if (dim < 2 + 2 * max_bounces) return -1;
  orce_lights_t* L = (orce_lights_t*)malloc(sizeof(orce_lights_t));
  const int nl = orce_lights_build(sc, L);
  if (mode == 2 && (nl > ORCE_MAX_LIGHTS || (nl == 0 && !sampling))) { free(L); return -1; }
  orct_env_t sky = {env_width, env_height, env_flags, env_rgb, {0}};
  orce_env_t dens;
  memset(&dens, 0, sizeof dens);
  if (env_rgb) {
    memcpy(sky.R, envR, sizeof sky.R);
    if (sampling) orce_build(&dens, env_rgb, env_width, env_height, env_flags, envR);
  }
  double* alpha = (double*)malloc(sizeof(double) * (size_t)(dim + 2));
  orc_lds_alpha(dim, alpha);
  if (mutant == ORCR_MUT_DIMS_FROM_0) /* the table moved up by two: what the path loop reads at 2 + j is dimension j */
    for (int j = dim + 1; j >= 2; --j) alpha[j] = alpha[j - 2];
  int64_t segments = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double* r = rays + 6 * i;
    v3 d = v3_make(r[3], r[4], r[5]);
    if (normalize) d = v3_normalize(d);
    const ray_t ray = ray_create(v3_make(r[0], r[1], r[2]), d);
    sampler_t smp;
    smp.alpha = alpha;
    smp.offset = offsets ? offsets[i] : (int)i;
    v3 c = orcn_trace_path(sc, images, env_rgb ? &sky : NULL, sampling ? &dens : NULL, L, mode, sampling, ray, &smp, max_bounces, &segments);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  if (segments_out) *segments_out = segments;
  free(alpha);
  if (env_rgb && sampling) orce_free(&dens);
  free(L);
  return 0;
}

/* The first hit of every ray as the feature record states it (orcp_first_hits on explicit rays): feat_out n x 8 = albedo, the facing
 * normal (scene space), depth = t along the ray, hits */
ORC_API void orcr_first_hits(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height, int env_flags,
                             const double* envR, int64_t n, const double* rays, double* feat_out) {
  orct_env_t sky = {env_width, env_height, env_flags, env_rgb, {0}};
  if (env_rgb) memcpy(sky.R, envR, sizeof sky.R);
  for (int64_t i = 0; i < n; ++i) {
    const double* r = rays + 6 * i;
    const ray_t ray = ray_create(v3_make(r[0], r[1], r[2]), v3_make(r[3], r[4], r[5]));
    double t = 0.0;
    int prim = -1;
    hit_t h;
    double* f = feat_out + 8 * i;
    if (!scene_intersect(sc, &ray, &h, &t, &prim, NULL)) {
      const v3 a = orct_miss(sc, env_rgb ? &sky : NULL, &ray);
      f[0] = a.x; f[1] = a.y; f[2] = a.z;
      f[3] = f[4] = f[5] = f[6] = f[7] = 0.0;
      continue;
    }
    v3 a;
    const orct_image_t* im = orct_image_of(images, h.m);
    if (h.m->kind == PTX_MAT_DIELECTRIC) a = v3_make(1.0, 1.0, 1.0);
    else if (im) a = orct_image_m(im->rgb, im->width, im->height, im->flags, h.tex_coord.u, h.tex_coord.v, 0);
    else a = texture_eval(&sc->mt, h.m->texture, h.tex_coord);
    const int sphere = prim >= 0 && prim < sc->n_prims && sc->prims[prim].kind != PRIM_TRIANGLE;
    const v3 nn = (sphere && !h.hit_front) ? v3_neg(h.shader_space.normal) : h.shader_space.normal;
    f[0] = a.x; f[1] = a.y; f[2] = a.z;
    f[3] = nn.x; f[4] = nn.y; f[5] = nn.z;
    f[6] = t;
    f[7] = 1.0;
  }
}
