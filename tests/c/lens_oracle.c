/* lens_oracle.c -- the CPU restatement of the thin-lens camera (include/ptx.h, "thin-lens camera: aperture and focus distance"), on
 * top of envlight_oracle.c, which is included unchanged (and texture_oracle.c and the oracle through it): this library carries its
 * own copy of the oracle (call this copy's orc_set_math(0) before comparing with the GPU).
 *
 * Written from the header's text, not from the kernel:
 *
 *   q  = (llx + (vx * cx), lly + (vy * cy), -1.0)
 *   P  = (F * q.x, F * q.y, F * q.z)
 *   r  = sqrt(u);  th = (v * 2.0) * pi;  lx = r * cos(th);  ly = r * sin(th)
 *   L  = (A * lx, A * ly, +0.0)
 *   d  = normalize(P - L);  the ray is Ray.create L d
 *   sampler: d = 4 + 2 max_bounces dimensions; the pixel jitter in 0 and 1, bounce k in 2 + 2k and 3 + 2k, (u, v) in d - 2 and d - 1
 *   radius 0: the lens is OFF -- Camera.ray and the 2 + 2 max_bounces sampler, nothing of the above
 *
 * orcn_trace_samples is the one path loop with the camera ray as an ARGUMENT: orce_trace_path's loop (integrator.ml:16-69) with the
 * scatter orct_scatter's (image textures), the miss orct_miss's (an environment or the descriptor's background), the emission the
 * reference's in lighting mode 0 and in path order in modes 1 and 2, and in mode 2 the mixture of envlight_oracle.c.  Every restated
 * loop before this one builds its own ray from (cx, cy); this copy covers them all.
 *
 * ORCN_MUT_*: the rule restated WRONGLY in one way, for the CPU tests' sensitivity conditions; every comparison with the GPU passes 0.
 *
 * Build: oracle/Makefile's flags (tests/lens_support.py). */
#include "envlight_oracle.c"

enum { ORCN_MUT_NONE = 0,
       ORCN_MUT_FOCUS_ALONG_RAY = 1, /* P = F * normalize(q): the focus distance measured along the ray instead of along z */
       ORCN_MUT_R_IS_U = 2,          /* r = u instead of sqrt u */
       ORCN_MUT_DIMS_2_3 = 3 };      /* the lens pair taken at dimensions 2 and 3 instead of d - 2 and d - 1 */

static ray_t orcn_lens_ray(const ptx_camera* c, double cx, double cy, double A, double F, double u, double v, int mutant) {
  const double pi = 3.14159265358979323846;
  v3 q = v3_make(c->lower_left_x + (c->view_x * cx), c->lower_left_y + (c->view_y * cy), -1.0);
  if (mutant == ORCN_MUT_FOCUS_ALONG_RAY) q = v3_normalize(q);
  const v3 P = v3_make(F * q.x, F * q.y, F * q.z);
  const double r = mutant == ORCN_MUT_R_IS_U ? u : sqrt(u);
  const double th = (v * 2.0) * pi;
  const double lx = r * m_cos(th), ly = r * m_sin(th);
  const v3 L = v3_make(A * lx, A * ly, 0.0);
  const v3 e = v3_make(P.x - L.x, P.y - L.y, P.z - L.z);
  return ray_create(L, v3_normalize(e));
}

static int orcn_dim(double A, int max_bounces) { return (A > 0.0 ? 4 : 2) + 2 * max_bounces; }

/* the camera ray of a sample whose sampler and film coordinates orct_sample made; dim: the sampler's dimension */
static ray_t orcn_camera_ray(const orc_scene* sc, const sampler_t* smp, double cx, double cy, double A, double F, int dim, int mutant) {
  if (!(A > 0.0)) return camera_ray(&sc->camera, cx, cy);
  const int at = mutant == ORCN_MUT_DIMS_2_3 ? 2 : dim - 2;
  return orcn_lens_ray(&sc->camera, cx, cy, A, F, sample_dim(smp, at), sample_dim(smp, at + 1), mutant);
}

/* the rule on explicit inputs: cam4 = (llx, lly, vx, vy), cxcy and uv n x 2 -> rays n x 6 (origin, direction) */
ORC_API void orcn_lens_rays(const double* cam4, double A, double F, int mutant, int64_t n, const double* cxcy, const double* uv, double* rays_out) {
  const ptx_camera c = {cam4[0], cam4[1], cam4[2], cam4[3]};
  for (int64_t i = 0; i < n; ++i) {
    const ray_t r = orcn_lens_ray(&c, cxcy[2 * i], cxcy[2 * i + 1], A, F, uv[2 * i], uv[2 * i + 1], mutant);
    rays_out[6 * i] = r.origin.x; rays_out[6 * i + 1] = r.origin.y; rays_out[6 * i + 2] = r.origin.z;
    rays_out[6 * i + 3] = r.direction.x; rays_out[6 * i + 4] = r.direction.y; rays_out[6 * i + 5] = r.direction.z;
  }
}

/* the camera rays of explicit samples: rays n x 6; cxcy_out (nullable) n x 2 */
ORC_API void orcn_sample_rays(const orc_scene* sc, double A, double F, int mutant, int width, int height, int spp, int max_bounces, int64_t n,
                              const int32_t* xs, const int32_t* ys, const int32_t* passes, double* rays_out, double* cxcy_out) {
  const int dim = orcn_dim(A, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t r = orcn_camera_ray(sc, &smp, cx, cy, A, F, dim, mutant);
    rays_out[6 * i] = r.origin.x; rays_out[6 * i + 1] = r.origin.y; rays_out[6 * i + 2] = r.origin.z;
    rays_out[6 * i + 3] = r.direction.x; rays_out[6 * i + 4] = r.direction.y; rays_out[6 * i + 5] = r.direction.z;
    if (cxcy_out) { cxcy_out[2 * i] = cx; cxcy_out[2 * i + 1] = cy; }
  }
  free(alpha);
}

/* path_tracer (integrator.ml:16-69) from a given camera ray.  images / env / dens nullable; mode 0, 1, 2; `sampling`: environment
 * sampling on (needs env and dens); *segments counts the Scene.intersect calls */
static v3 orcn_trace_path(const orc_scene* sc, const orct_image_t* images, const orct_env_t* env, const orce_env_t* dens, const orce_lights_t* L,
                          int mode, int sampling, ray_t ray, const sampler_t* smp, int max_bounces, int64_t* segments) {
  int samples_index = 2;
  v3 emit0 = v3_make(0.0, 0.0, 0.0), attn0 = v3_make(1.0, 1.0, 1.0);
  const v3 black = v3_make(0.0, 0.0, 0.0);
  const int tri_on = mode == 2 && L->n > 0, env_on = mode == 2 && sampling;
  for (;;) {
    if (max_bounces <= 0) return add_mul(emit0, attn0, black);
    max_bounces = max_bounces - 1;
    hit_t h;
    *segments += 1;
    if (!scene_intersect(sc, &ray, &h, NULL, NULL, NULL)) return add_mul(emit0, attn0, orct_miss(sc, env, &ray));
    v3 emit = h.emit;
    int j = samples_index;
    double u = sample_dim(smp, j), v = sample_dim(smp, j + 1);
    samples_index = j + 2;
    scatter_t s = orct_scatter(sc, images, 0, &h, u);
    if (s.kind == SC_ABSORB) return add_mul(emit0, attn0, emit);
    v3 attenuation;
    ray_t next;
    if (s.kind == SC_SPECULAR) {
      attenuation = s.attenuation;
      next = s.ray;
    } else {
      const v3 p = h.shader_space.origin;
      v3 dir;
      if (mode != 2) dir = unit_square_to_hemisphere(u, v);
      else if (tri_on && env_on) {
        if (u < 0.25) dir = sspace_rotate(&h.shader_space, orce_light_sample(L, p, 4.0 * u, v));
        else if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_sample(dens, 4.0 * u - 1.0, v, NULL, NULL));
        else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
      } else if (env_on) {
        if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_sample(dens, 2.0 * u, v, NULL, NULL));
        else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
      } else {
        if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_light_sample(L, p, 2.0 * u, v));
        else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
      }
      double diffuse_pd = pdf_eval_diffuse(dir);
      if (diffuse_pd == 0.0) return add_mul(emit0, attn0, emit);
      double divisor = diffuse_pd;
      if (mode == 2) {
        v3 w = sspace_rotate_inv(&h.shader_space, dir);
        if (tri_on && env_on) divisor = (0.5 * diffuse_pd + 0.25 * orce_light_pd(L, p, w)) + 0.25 * orce_pd(dens, w, 0, NULL, NULL);
        else if (env_on) divisor = 0.5 * diffuse_pd + 0.5 * orce_pd(dens, w, 0, NULL, NULL);
        else divisor = 0.5 * diffuse_pd + 0.5 * orce_light_pd(L, p, w);
      }
      double pd = diffuse_pd / divisor;
      if (!pt_isfinite(pd)) return add_mul(emit0, attn0, emit);
      next = sspace_world_ray(&h.shader_space, dir);
      attenuation = v3_scale(s.attenuation, pd);
    }
    /* mode 0: the reference's emit0' = a * emit0 + emit; modes 1 and 2: path order, emit0' = attn0 * emit + emit0 */
    v3 ne = mode == 0 ? add_mul(emit, attenuation, emit0) : add_mul(emit0, attn0, emit);
    attn0 = v3_mul(attenuation, attn0);
    emit0 = ne;
    ray = next;
  }
}

/* Per-sample radiance through the lens (A = 0: off).  images: one record per texture-table index or NULL; env_rgb NULL: the
 * descriptor's background; mode 0, 1, 2 and `sampling` as the scene's state.  segments_out (nullable): the Scene.intersect calls of
 * all samples.  Returns 0, or -1 when mode 2 has nothing to sample. */
ORC_API int orcn_trace_samples(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height,
                               int env_flags, const double* R, int mode, int sampling, double A, double F, int mutant, int width, int height,
                               int spp, int max_bounces, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes,
                               double* rgb_out, int64_t* segments_out) {
  if (mode < 0 || mode > 2 || (sampling && !env_rgb)) return -1;
  orce_lights_t* L = (orce_lights_t*)malloc(sizeof(orce_lights_t));
  const int nl = orce_lights_build(sc, L);
  if (mode == 2 && (nl > ORCE_MAX_LIGHTS || (nl == 0 && !sampling))) { free(L); return -1; }
  orct_env_t sky = {env_width, env_height, env_flags, env_rgb, {0}};
  orce_env_t dens;
  memset(&dens, 0, sizeof dens);
  if (env_rgb) {
    memcpy(sky.R, R, sizeof sky.R);
    if (sampling) orce_build(&dens, env_rgb, env_width, env_height, env_flags, R);
  }
  const int dim = orcn_dim(A, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  int64_t segments = 0;
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t ray = orcn_camera_ray(sc, &smp, cx, cy, A, F, dim, mutant);
    v3 c = orcn_trace_path(sc, images, env_rgb ? &sky : NULL, sampling ? &dens : NULL, L, mode, sampling, ray, &smp, max_bounces, &segments);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  if (segments_out) *segments_out = segments;
  free(alpha);
  if (env_rgb && sampling) orce_free(&dens);
  free(L);
  return 0;
}

/* The first hit of every sample's camera ray as the feature record states it (ptx_render_features_device): feat_out n x 8 =
 * albedo, the facing normal, depth = t along the ray, hits.  A sphere's normal is negated when the hit is from inside (Sphere.hit
 * keeps the outward one for the shader space); a triangle's already faces the ray. */
ORC_API void orcn_first_hits(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height, int env_flags,
                             const double* R, double A, double F, int width, int height, int spp, int max_bounces, int64_t n, const int32_t* xs,
                             const int32_t* ys, const int32_t* passes, double* feat_out) {
  orct_env_t sky = {env_width, env_height, env_flags, env_rgb, {0}};
  if (env_rgb) memcpy(sky.R, R, sizeof sky.R);
  const int dim = orcn_dim(A, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy, t = 0.0;
    int prim = -1;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t ray = orcn_camera_ray(sc, &smp, cx, cy, A, F, dim, 0);
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
  free(alpha);
}
