/* envlight_oracle.c -- the CPU restatement of environment sampling (include/ptx.h, "importance-sampling the environment in
 * PTX_LIGHTING_SAMPLED"), on top of texture_oracle.c, which is included unchanged (and the oracle through it): this library carries
 * its own copy of the oracle (call this copy's orc_set_math(0) before comparing with the GPU), the image and environment rules of
 * texture_oracle.c, and the entry points below.
 *
 * Written from the header's text, not from the kernel:
 *
 *   density   lum = (r + g) + b, 0 unless > 0;  s_iy = sin(pi * ((iy + 0.5) / H));  w = lum * s_iy
 *             c_iy[ix] running sums left to right, r_iy = c_iy[W - 1];  m[iy] running sums of r_iy, T = m[H - 1]
 *   sample    x = a * T; iy = first row with x < m[iy] (the last row with r_iy > 0 if none); fy = min((x - m[iy - 1]) / r_iy, 1)
 *             y = b * r_iy; ix = first column with y < c_iy[ix] (the last of the row with w > 0 if none); fx = min((y - c_iy[ix - 1]) / w, 1)
 *             u = (ix + fx) / W, v = (iy + fy) / H;  al = u * (2 pi) - pi, th = v * pi
 *             m = (sin th * cos al, -cos th, -(sin th * sin al));  direction = normalize(R^T m)
 *             -- the searches here are the LINEAR scans of the definition
 *   pd        e = normalize(w), m = R e, (u, v) of the environment rule;  ix = min((long long)(u * W), W - 1), iy likewise
 *             st = sin(v * pi);  pd = st > 0 ? ((w(ix, iy) / T) * (W * H)) / ((2 (pi * pi)) * st) : 0
 *   the light list and the triangle rule: as tests/c/lighting_oracle.c states them (restated here: that file includes the oracle too)
 *   mixture   with triangles: su < 0.25 triangles on 2u := 4 su; su < 0.5 the environment on (4 su - 1, sv); else cosine on (2 su - 1, sv)
 *             divisor = (0.5 diffuse_pd + 0.25 light_pd) + 0.25 env_pd
 *             environment only: su < 0.5 the environment on (2 su, sv); divisor = 0.5 diffuse_pd + 0.5 env_pd
 *   Emission in path order (modes 1 and 2): emit0' = add_mul emit0 attn0 emit with the old attn0.
 *
 * ORCE_MUT_*: the rule restated WRONGLY in one way, for the CPU tests' sensitivity conditions; every comparison with the GPU passes 0.
 *
 * Build: oracle/Makefile's flags (tests/envlight_support.py). */
#include "texture_oracle.c"

enum { ORCE_MUT_NONE = 0, ORCE_MUT_NO_SIN = 1 /* pd without the 1 / st factor */, ORCE_MUT_HALF_WEIGHTS = 2 /* 0.5 / 0.5 for 0.25 / 0.25 */ };

typedef struct {
  int W, H, last_row;
  double T;
  double *m, *c, *w; /* H, H x W, H x W */
  const double* rgb;
  int flags;
  double R[9];
} orce_env_t;

static void orce_free(orce_env_t* e) { free(e->m); free(e->c); free(e->w); }

static void orce_build(orce_env_t* e, const double* rgb, int W, int H, int flags, const double* R) {
  const double pi = 3.14159265358979323846;
  e->W = W; e->H = H; e->rgb = rgb; e->flags = flags; e->last_row = 0;
  memcpy(e->R, R, sizeof e->R);
  e->m = (double*)malloc(sizeof(double) * (size_t)H);
  e->c = (double*)malloc(sizeof(double) * (size_t)H * (size_t)W);
  e->w = (double*)malloc(sizeof(double) * (size_t)H * (size_t)W);
  double total = 0.0;
  for (int iy = 0; iy < H; ++iy) {
    const double s = m_sin(pi * (((double)iy + 0.5) / (double)H));
    double run = 0.0;
    for (int ix = 0; ix < W; ++ix) {
      const double* t = rgb + 3 * ((size_t)iy * (size_t)W + (size_t)ix);
      double lum = (t[0] + t[1]) + t[2];
      if (!(lum > 0.0)) lum = 0.0;
      const double w = lum * s;
      run = run + w;
      e->c[(size_t)iy * W + ix] = run;
      e->w[(size_t)iy * W + ix] = w;
    }
    if (run > 0.0) e->last_row = iy;
    total = total + run;
    e->m[iy] = total;
  }
  e->T = total;
}

/* marginal_out: H, conditional_out: H x W; returns T */
ORC_API double orce_distribution(const double* rgb, int W, int H, double* marginal_out, double* conditional_out) {
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  orce_env_t e;
  orce_build(&e, rgb, W, H, 0, I);
  if (marginal_out) memcpy(marginal_out, e.m, sizeof(double) * (size_t)H);
  if (conditional_out) memcpy(conditional_out, e.c, sizeof(double) * (size_t)H * (size_t)W);
  const double T = e.T;
  orce_free(&e);
  return T;
}

static v3 orce_sample(const orce_env_t* e, double a, double b, int* ix_out, int* iy_out) {
  const double pi = 3.14159265358979323846;
  const int W = e->W, H = e->H;
  const double x = a * e->T;
  int iy = e->last_row;
  for (int j = 0; j < H; ++j)
    if (x < e->m[j]) { iy = j; break; }
  const double* c = e->c + (size_t)iy * W;
  const double* wrow = e->w + (size_t)iy * W;
  const double r = c[W - 1];
  const double fy = pt_base_min((x - (iy > 0 ? e->m[iy - 1] : 0.0)) / r, 1.0);
  const double y = b * r;
  int ix = -1;
  for (int j = 0; j < W; ++j)
    if (y < c[j]) { ix = j; break; }
  if (ix < 0) {
    ix = 0;
    for (int j = 0; j < W; ++j)
      if (wrow[j] > 0.0) ix = j;
  }
  const double fx = pt_base_min((y - (ix > 0 ? c[ix - 1] : 0.0)) / wrow[ix], 1.0);
  if (ix_out) *ix_out = ix;
  if (iy_out) *iy_out = iy;
  const double u = ((double)ix + fx) / (double)W, v = ((double)iy + fy) / (double)H;
  const double al = u * (2.0 * pi) - pi, th = v * pi;
  const double sa = m_sin(al), ca = m_cos(al), st = m_sin(th), ct = m_cos(th);
  const v3 mm = v3_make(st * ca, -ct, -(st * sa));
  const double* R = e->R;
  return v3_normalize(v3_make((R[0] * mm.x + R[3] * mm.y) + R[6] * mm.z, (R[1] * mm.x + R[4] * mm.y) + R[7] * mm.z,
                              (R[2] * mm.x + R[5] * mm.y) + R[8] * mm.z));
}

static long long orce_index(double u, int n) {
  const double p = orct_scale(u, n);
  long long i = (long long)p;
  if (i < 0) i = 0;
  return i > n - 1 ? n - 1 : i;
}

static double orce_pd(const orce_env_t* env, v3 w, int mutant, int* ix_out, int* iy_out) {
  const double pi = 3.14159265358979323846;
  const v3 e = v3_normalize(w);
  const double* R = env->R;
  const double mx = (R[0] * e.x + R[1] * e.y) + R[2] * e.z;
  const double my = (R[3] * e.x + R[4] * e.y) + R[5] * e.z;
  const double mz = (R[6] * e.x + R[7] * e.y) + R[8] * e.z;
  const double lo = my < -1.0 ? -1.0 : my;
  const double cy = lo > 1.0 ? 1.0 : lo;
  const double u = (pi + m_atan2(-mz, mx)) * (1.0 / (2.0 * pi));
  const double v = m_acos(-cy) * (1.0 / pi);
  const long long ix = orce_index(u, env->W), iy = orce_index(v, env->H);
  if (ix_out) *ix_out = (int)ix;
  if (iy_out) *iy_out = (int)iy;
  const double wt = env->w[(size_t)iy * env->W + (size_t)ix];
  const double st = m_sin(v * pi);
  if (!(st > 0.0)) return 0.0;
  if (mutant == ORCE_MUT_NO_SIN) return ((wt / env->T) * ((double)env->W * (double)env->H)) / (2.0 * (pi * pi));
  return ((wt / env->T) * ((double)env->W * (double)env->H)) / ((2.0 * (pi * pi)) * st);
}

/* the two functions on explicit inputs: ab n x 2 -> dirs n x 3, texel n x 2;  dirs n x 3 -> pd n, texel n x 2 (nullable) */
ORC_API void orce_sample_many(const double* rgb, int W, int H, const double* R, int64_t n, const double* ab, double* dirs_out, int32_t* texel_out) {
  orce_env_t e;
  orce_build(&e, rgb, W, H, 0, R);
  for (int64_t i = 0; i < n; ++i) {
    int ix, iy;
    const v3 d = orce_sample(&e, ab[2 * i], ab[2 * i + 1], &ix, &iy);
    dirs_out[3 * i] = d.x; dirs_out[3 * i + 1] = d.y; dirs_out[3 * i + 2] = d.z;
    if (texel_out) { texel_out[2 * i] = ix; texel_out[2 * i + 1] = iy; }
  }
  orce_free(&e);
}
ORC_API void orce_pd_many(const double* rgb, int W, int H, const double* R, int64_t n, const double* dirs, double* pd_out, int32_t* texel_out) {
  orce_env_t e;
  orce_build(&e, rgb, W, H, 0, R);
  for (int64_t i = 0; i < n; ++i) {
    int ix, iy;
    pd_out[i] = orce_pd(&e, v3_make(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), ORCE_MUT_NONE, &ix, &iy);
    if (texel_out) { texel_out[2 * i] = ix; texel_out[2 * i + 1] = iy; }
  }
  orce_free(&e);
}

/* ---- the light list and the triangle rule ---- */
#define ORCE_MAX_LIGHTS 64
typedef struct { v3 a, b, c, n; double area, cum; } orce_light_t;
typedef struct { int n; double area; orce_light_t l[ORCE_MAX_LIGHTS]; } orce_lights_t;

static int orce_lights_build(const orc_scene* sc, orce_lights_t* L) {
  int n = 0;
  double cum = 0.0;
  L->n = 0;
  L->area = 0.0;
  for (int i = 0; i < sc->n_prims; ++i) {
    const prim_t* p = &sc->prims[i];
    if (p->kind != PRIM_TRIANGLE) continue;
    const ptx_material* m = &sc->mt.materials[p->material];
    if (m->emit[0] == 0.0 && m->emit[1] == 0.0 && m->emit[2] == 0.0) continue;
    if (n < ORCE_MAX_LIGHTS) {
      orce_light_t* l = &L->l[n];
      const v3 cr = v3_cross(v3_sub(p->b, p->a), v3_sub(p->c, p->a));
      l->a = p->a; l->b = p->b; l->c = p->c;
      l->n = v3_normalize(cr);
      l->area = 0.5 * sqrt(v3_quadrance(cr));
      cum = cum + l->area;
      l->cum = cum;
    }
    n++;
  }
  if (n <= ORCE_MAX_LIGHTS) { L->n = n; L->area = cum; }
  return n;
}
static double orce_light_pd(const orce_lights_t* L, v3 p, v3 w) {
  double acc = 0.0;
  ray_t r = ray_create(p, w);
  for (int k = 0; k < L->n; ++k) {
    prim_t t;
    memset(&t, 0, sizeof t);
    t.kind = PRIM_TRIANGLE; t.a = L->l[k].a; t.b = L->l[k].b; t.c = L->l[k].c;
    trihit_t h;
    if (triangle_intersect(&t, &r, 0.0, 1.7976931348623157e308, &h))
      acc = acc + (h.t_hit * h.t_hit) / (L->area * fabs(v3_dot(L->l[k].n, w)));
  }
  return acc;
}
/* two_u: the rule's 2u */
static v3 orce_light_sample(const orce_lights_t* L, v3 p, double two_u, double v) {
  const double x = two_u * L->area;
  int k = L->n - 1;
  for (int j = 0; j < L->n; ++j)
    if (x < L->l[j].cum) { k = j; break; }
  const double before = k > 0 ? L->l[k - 1].cum : 0.0;
  const double u2 = pt_base_min((x - before) / L->l[k].area, 1.0);
  const double s = sqrt(u2);
  const double b1 = 1.0 - s, b2 = v * s;
  const double b0 = 1.0 - b1 - b2;
  const v3 q = v3_add(v3_add(v3_scale(L->l[k].a, b0), v3_scale(L->l[k].b, b1)), v3_scale(L->l[k].c, b2));
  return v3_normalize(v3_sub(q, p));
}

/* path_tracer (integrator.ml:16-69), the miss colour the environment's (texture_oracle.c), the emission in path order (modes 1 and 2),
 * and in mode 2 the mixture: `sampling` = environment sampling on; L->n == 0 = no light triangles */
static v3 orce_trace_path(const orc_scene* sc, const orce_env_t* env, const orct_env_t* sky, const orce_lights_t* L, int mode, int sampling,
                          int mutant, double cx, double cy, const sampler_t* smp, int max_bounces) {
  ray_t ray = camera_ray(&sc->camera, cx, cy);
  int samples_index = 2;
  v3 emit0 = v3_make(0.0, 0.0, 0.0), attn0 = v3_make(1.0, 1.0, 1.0);
  const v3 black = v3_make(0.0, 0.0, 0.0);
  const int tri_on = mode == 2 && L->n > 0, env_on = mode == 2 && sampling;
  for (;;) {
    if (max_bounces <= 0) return add_mul(emit0, attn0, black);
    max_bounces = max_bounces - 1;
    hit_t h;
    if (!scene_intersect(sc, &ray, &h, NULL, NULL, NULL)) return add_mul(emit0, attn0, orct_environment(sky, ray.direction));
    v3 emit = h.emit;
    int j = samples_index;
    double u = sample_dim(smp, j), v = sample_dim(smp, j + 1);
    samples_index = j + 2;
    scatter_t s = hit_scatter(&sc->mt, &h, u);
    if (s.kind == SC_ABSORB) return add_mul(emit0, attn0, emit);
    if (s.kind == SC_SPECULAR) {
      v3 ne = add_mul(emit0, attn0, emit);
      attn0 = v3_mul(s.attenuation, attn0);
      emit0 = ne;
      ray = s.ray;
      continue;
    }
    const v3 p = h.shader_space.origin;
    v3 dir;
    if (mode != 2) dir = unit_square_to_hemisphere(u, v);
    else if (tri_on && env_on) {
      if (u < 0.25) dir = sspace_rotate(&h.shader_space, orce_light_sample(L, p, 4.0 * u, v));
      else if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_sample(env, 4.0 * u - 1.0, v, NULL, NULL));
      else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
    } else if (env_on) {
      if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_sample(env, 2.0 * u, v, NULL, NULL));
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
      if (tri_on && env_on) {
        const double wl = mutant == ORCE_MUT_HALF_WEIGHTS ? 0.5 : 0.25;
        divisor = (0.5 * diffuse_pd + wl * orce_light_pd(L, p, w)) + wl * orce_pd(env, w, mutant, NULL, NULL);
      } else if (env_on) divisor = 0.5 * diffuse_pd + 0.5 * orce_pd(env, w, mutant, NULL, NULL);
      else divisor = 0.5 * diffuse_pd + 0.5 * orce_light_pd(L, p, w);
    }
    double pd = diffuse_pd / divisor;
    if (!pt_isfinite(pd)) return add_mul(emit0, attn0, emit);
    ray_t scattered = sspace_world_ray(&h.shader_space, dir);
    v3 attenuation = v3_scale(s.attenuation, pd);
    v3 ne = add_mul(emit0, attn0, emit);
    attn0 = v3_mul(attenuation, attn0);
    emit0 = ne;
    ray = scattered;
  }
}

/* orc_trace_samples under the environment (rgb, W, H, flags, R) in lighting mode 1 or 2, with environment sampling on or off.
 * Returns 0, or -1 when mode 2 has nothing to sample (no light triangle and sampling off) or too many triangles. */
ORC_API int orce_trace_samples(const orc_scene* sc, const double* rgb, int env_width, int env_height, int env_flags, const double* R, int mode,
                               int sampling, int mutant, int width, int height, int spp, int max_bounces, int64_t n, const int32_t* xs,
                               const int32_t* ys, const int32_t* passes, double* rgb_out) {
  if (mode != 1 && mode != 2) return -1;
  orce_lights_t* L = (orce_lights_t*)malloc(sizeof(orce_lights_t));
  const int nl = orce_lights_build(sc, L);
  if (mode == 2 && (nl > ORCE_MAX_LIGHTS || (nl == 0 && !sampling))) { free(L); return -1; }
  orce_env_t env;
  orce_build(&env, rgb, env_width, env_height, env_flags, R);
  orct_env_t sky = {env_width, env_height, env_flags, rgb, {0}};
  memcpy(sky.R, R, sizeof sky.R);
  int dim = 2 + 2 * max_bounces;
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    v3 c = orce_trace_path(sc, &env, &sky, L, mode, sampling, mutant, cx, cy, &smp, max_bounces);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  free(alpha);
  orce_free(&env);
  free(L);
  return 0;
}
