/* spherelight_oracle.c -- the CPU restatement of sphere light sampling (include/ptx.h, "cone-sampling emissive spheres in
 * PTX_LIGHTING_SAMPLED"), on top of envlight_oracle.c, which is included unchanged (and texture_oracle.c and the oracle through it): this
 * library carries its own copy of the oracle (call this copy's orc_set_math(0) before comparing with the GPU), the environment and
 * triangle rules of envlight_oracle.c, and the entry points below.
 *
 * Written from the header's text, not from the kernel:
 *
 *   list      the build list's spheres whose material emits, in its order: c, r, r2 = r * r, W = (2.0 * pi) * r2, cum running on from the
 *             triangles' A_total; W_total = the joined table's last cum
 *   sample    x = 2u * W_total; k = first entry of [triangles] @ [spheres] with x < cum_k (the last if none); before = cum_(k-1) or 0.0
 *             u2 = min((x - before) / W_k, 1.0); a triangle goes on as the triangle rule says; a sphere:
 *             f = c - p; d2 = dot f f; phi = (v * 2.0) * pi
 *             d2 <= r2: z = 1.0 - 2.0 * u2; m = 1.0 - z * z (0.0 unless > 0); s = sqrt(m); w = (s cos phi, s sin phi, z)
 *             else s2 = r2 / d2; q = s2 / (1.0 + sqrt(1.0 - s2)); t = u2 * q; ct = 1.0 - t; st = sqrt(t * (2.0 - t))
 *                  w = rotate_inv (Shader_space.create (normalize f)) (st cos phi, st sin phi, ct)
 *   pd        triangles: t^2 / (W_total |n . w|) for every one the ray meets; spheres in list order, share = W_k / W_total:
 *             d2 <= r2: + share / (4.0 * pi); else bp = dot f w; g = f - bp * w; if bp > 0 and r2 - dot g g >= 0: + share / ((2.0 * pi) * q)
 *   mixture   envlight_oracle.c's, "triangles" read as the joined table
 *
 * ORCS_MUT_*: the rule restated WRONGLY in one way, for the CPU tests' sensitivity conditions; every comparison with the GPU passes 0.
 *
 * Build: oracle/Makefile's flags (tests/spherelight_support.py). */
#include "envlight_oracle.c"

enum { ORCS_MUT_NONE = 0, ORCS_MUT_NO_SHARE = 1 /* pd without W_k / W_total */, ORCS_MUT_FOUR_PI = 2 /* 4 pi used for (2 pi) q */ };

#define ORCS_MAX_SPHERES 64
typedef struct { v3 c; double r, r2, W, cum; } orcs_sphere_t;
typedef struct {
  orce_lights_t tri; /* tri.area stays the triangles' own A_total */
  int n_tri_found, n_sph_found;
  int ns;
  double total; /* W_total */
  orcs_sphere_t s[ORCS_MAX_SPHERES];
} orcs_lights_t;

/* spheres_on = 0: the triangle table alone, total = A_total */
static void orcs_build(const orc_scene* sc, int spheres_on, orcs_lights_t* L) {
  const double pi = 3.14159265358979323846;
  L->n_tri_found = orce_lights_build(sc, &L->tri);
  L->ns = 0;
  L->n_sph_found = 0;
  double cum = L->tri.area;
  for (int i = 0; i < sc->n_prims; ++i) {
    const prim_t* p = &sc->prims[i];
    if (p->kind != PRIM_SPHERE) continue;
    const ptx_material* m = &sc->mt.materials[p->material];
    if (m->emit[0] == 0.0 && m->emit[1] == 0.0 && m->emit[2] == 0.0) continue;
    if (L->n_sph_found < ORCS_MAX_SPHERES) {
      orcs_sphere_t* s = &L->s[L->n_sph_found];
      s->c = p->center;
      s->r = p->radius;
      s->r2 = p->radius * p->radius;
      s->W = (2.0 * pi) * s->r2;
      cum = cum + s->W;
      s->cum = cum;
    }
    L->n_sph_found++;
  }
  if (spheres_on && L->n_sph_found <= ORCS_MAX_SPHERES) L->ns = L->n_sph_found;
  L->total = L->ns > 0 ? L->s[L->ns - 1].cum : L->tri.area;
}

static double orcs_q(double r2, double d2) {
  const double s2 = r2 / d2;
  return s2 / (1.0 + sqrt(1.0 - s2));
}

static v3 orcs_sphere_sample(const orcs_sphere_t* s, v3 p, double u2, double v) {
  const double pi = 3.14159265358979323846;
  const v3 f = v3_sub(s->c, p);
  const double d2 = v3_dot(f, f);
  const double phi = (v * 2.0) * pi;
  const double sn = m_sin(phi), cs = m_cos(phi);
  if (d2 <= s->r2) {
    const double z = 1.0 - 2.0 * u2;
    double m = 1.0 - z * z;
    if (!(m > 0.0)) m = 0.0;
    const double sq = sqrt(m);
    return v3_make(sq * cs, sq * sn, z);
  }
  const double t = u2 * orcs_q(s->r2, d2);
  const double ct = 1.0 - t, st = sqrt(t * (2.0 - t));
  const sspace_t frame = sspace_create(v3_normalize(f), p);
  return sspace_rotate_inv(&frame, v3_make(st * cs, st * sn, ct));
}

/* two_u: the rule's 2u; k_out: the joined table's entry */
static v3 orcs_sample(const orcs_lights_t* L, v3 p, double two_u, double v, int* k_out) {
  const int nt = L->tri.n, n = nt + L->ns;
  const double x = two_u * L->total;
  int k = n - 1;
  for (int j = 0; j < n; ++j) {
    const double cum = j < nt ? L->tri.l[j].cum : L->s[j - nt].cum;
    if (x < cum) { k = j; break; }
  }
  if (k_out) *k_out = k;
  double before = 0.0;
  if (k > 0) before = k - 1 < nt ? L->tri.l[k - 1].cum : L->s[k - 1 - nt].cum;
  if (k >= nt) {
    const orcs_sphere_t* s = &L->s[k - nt];
    return orcs_sphere_sample(s, p, pt_base_min((x - before) / s->W, 1.0), v);
  }
  const orce_light_t* t = &L->tri.l[k];
  const double u2 = pt_base_min((x - before) / t->area, 1.0);
  const double sq = sqrt(u2);
  const double b1 = 1.0 - sq, b2 = v * sq;
  const double b0 = 1.0 - b1 - b2;
  const v3 q = v3_add(v3_add(v3_scale(t->a, b0), v3_scale(t->b, b1)), v3_scale(t->c, b2));
  return v3_normalize(v3_sub(q, p));
}

static double orcs_pd(const orcs_lights_t* L, v3 p, v3 w, int mutant) {
  const double pi = 3.14159265358979323846;
  double acc = 0.0;
  ray_t r = ray_create(p, w);
  for (int k = 0; k < L->tri.n; ++k) {
    prim_t t;
    memset(&t, 0, sizeof t);
    t.kind = PRIM_TRIANGLE; t.a = L->tri.l[k].a; t.b = L->tri.l[k].b; t.c = L->tri.l[k].c;
    trihit_t h;
    if (triangle_intersect(&t, &r, 0.0, 1.7976931348623157e308, &h))
      acc = acc + (h.t_hit * h.t_hit) / (L->total * fabs(v3_dot(L->tri.l[k].n, w)));
  }
  for (int k = 0; k < L->ns; ++k) {
    const orcs_sphere_t* s = &L->s[k];
    const double share = mutant == ORCS_MUT_NO_SHARE ? 1.0 : s->W / L->total;
    const v3 f = v3_sub(s->c, p);
    const double d2 = v3_dot(f, f);
    if (d2 <= s->r2) {
      acc = acc + share / (4.0 * pi);
    } else {
      const double bp = v3_dot(f, w);
      const v3 g = v3_sub(f, v3_scale(w, bp));
      if (bp > 0.0 && s->r2 - v3_dot(g, g) >= 0.0) {
        if (mutant == ORCS_MUT_FOUR_PI) acc = acc + share / (4.0 * pi);
        else acc = acc + share / ((2.0 * pi) * orcs_q(s->r2, d2));
      }
    }
  }
  return acc;
}

/* counts_out: {light triangles found, emissive spheres found}; tri_out (nullable): 14 doubles per light triangle {a, b, c, n, A, cum};
 * sph_out (nullable): 8 doubles per sphere light {c, r, r2, W, cum, 0}.  Returns W_total of the joined table. */
ORC_API double orcs_table(const orc_scene* sc, int32_t* counts_out, double* tri_out, double* sph_out) {
  orcs_lights_t* L = (orcs_lights_t*)malloc(sizeof(orcs_lights_t));
  orcs_build(sc, 1, L);
  if (counts_out) { counts_out[0] = L->n_tri_found; counts_out[1] = L->n_sph_found; }
  if (tri_out)
    for (int k = 0; k < L->tri.n; ++k) {
      const orce_light_t* t = &L->tri.l[k];
      const double rec[14] = {t->a.x, t->a.y, t->a.z, t->b.x, t->b.y, t->b.z, t->c.x, t->c.y, t->c.z, t->n.x, t->n.y, t->n.z, t->area, t->cum};
      memcpy(tri_out + 14 * k, rec, sizeof rec);
    }
  if (sph_out)
    for (int k = 0; k < L->ns; ++k) {
      const orcs_sphere_t* s = &L->s[k];
      const double rec[8] = {s->c.x, s->c.y, s->c.z, s->r, s->r2, s->W, s->cum, 0.0};
      memcpy(sph_out + 8 * k, rec, sizeof rec);
    }
  const double total = L->total;
  free(L);
  return total;
}

/* the two functions on explicit inputs, as ptx_light_sample / ptx_light_pdf take them: uv[2 i] is the hit's first dimension (2u = 2.0 * u) */
ORC_API int orcs_sample_many(const orc_scene* sc, int64_t n, const double* points, const double* uv, double* dirs_out, int32_t* index_out) {
  orcs_lights_t* L = (orcs_lights_t*)malloc(sizeof(orcs_lights_t));
  orcs_build(sc, 1, L);
  if (L->tri.n + L->ns < 1) { free(L); return -1; }
  for (int64_t i = 0; i < n; ++i) {
    int k;
    const v3 d = orcs_sample(L, v3_make(points[3 * i], points[3 * i + 1], points[3 * i + 2]), 2.0 * uv[2 * i], uv[2 * i + 1], &k);
    dirs_out[3 * i] = d.x; dirs_out[3 * i + 1] = d.y; dirs_out[3 * i + 2] = d.z;
    if (index_out) index_out[i] = k;
  }
  free(L);
  return 0;
}
ORC_API int orcs_pd_many(const orc_scene* sc, int mutant, int64_t n, const double* points, const double* dirs, double* pd_out) {
  orcs_lights_t* L = (orcs_lights_t*)malloc(sizeof(orcs_lights_t));
  orcs_build(sc, 1, L);
  if (L->tri.n + L->ns < 1) { free(L); return -1; }
  for (int64_t i = 0; i < n; ++i)
    pd_out[i] = orcs_pd(L, v3_make(points[3 * i], points[3 * i + 1], points[3 * i + 2]), v3_make(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), mutant);
  free(L);
  return 0;
}

/* path_tracer (integrator.ml:16-69) with the emission in path order (modes 1 and 2) and in mode 2 the mixture over the joined table L
 * (L->ns == 0: sphere light sampling off) and, with `env_sampling`, the environment's density.  env == NULL: no environment at all (the
 * descriptor's background). */
static v3 orcs_trace_path(const orc_scene* sc, const orce_env_t* env, const orct_env_t* sky, const orcs_lights_t* L, int mode, int env_sampling,
                          int mutant, double cx, double cy, const sampler_t* smp, int max_bounces) {
  ray_t ray = camera_ray(&sc->camera, cx, cy);
  int samples_index = 2;
  v3 emit0 = v3_make(0.0, 0.0, 0.0), attn0 = v3_make(1.0, 1.0, 1.0);
  const v3 black = v3_make(0.0, 0.0, 0.0);
  const int lights_on = mode == 2 && L->tri.n + L->ns > 0, env_on = mode == 2 && env_sampling;
  for (;;) {
    if (max_bounces <= 0) return add_mul(emit0, attn0, black);
    max_bounces = max_bounces - 1;
    hit_t h;
    if (!scene_intersect(sc, &ray, &h, NULL, NULL, NULL)) return add_mul(emit0, attn0, orct_miss(sc, sky, &ray));
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
    else if (lights_on && env_on) {
      if (u < 0.25) dir = sspace_rotate(&h.shader_space, orcs_sample(L, p, 4.0 * u, v, NULL));
      else if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_sample(env, 4.0 * u - 1.0, v, NULL, NULL));
      else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
    } else if (env_on) {
      if (u < 0.5) dir = sspace_rotate(&h.shader_space, orce_sample(env, 2.0 * u, v, NULL, NULL));
      else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
    } else {
      if (u < 0.5) dir = sspace_rotate(&h.shader_space, orcs_sample(L, p, 2.0 * u, v, NULL));
      else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
    }
    double diffuse_pd = pdf_eval_diffuse(dir);
    if (diffuse_pd == 0.0) return add_mul(emit0, attn0, emit);
    double divisor = diffuse_pd;
    if (mode == 2) {
      v3 w = sspace_rotate_inv(&h.shader_space, dir);
      if (lights_on && env_on) divisor = (0.5 * diffuse_pd + 0.25 * orcs_pd(L, p, w, mutant)) + 0.25 * orce_pd(env, w, ORCE_MUT_NONE, NULL, NULL);
      else if (env_on) divisor = 0.5 * diffuse_pd + 0.5 * orce_pd(env, w, ORCE_MUT_NONE, NULL, NULL);
      else divisor = 0.5 * diffuse_pd + 0.5 * orcs_pd(L, p, w, mutant);
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

/* orc_trace_samples in lighting mode 1 or 2, sphere light sampling on or off, under an environment (rgb NULL: none) that is sampled or
 * not.  Returns 0, or -1 when mode 2 has nothing to sample or too many lights of a kind. */
ORC_API int orcs_trace_samples(const orc_scene* sc, const double* rgb, int env_width, int env_height, int env_flags, const double* R, int mode,
                               int spheres_on, int env_sampling, int mutant, int width, int height, int spp, int max_bounces, int64_t n,
                               const int32_t* xs, const int32_t* ys, const int32_t* passes, double* rgb_out) {
  if (mode != 1 && mode != 2) return -1;
  if (env_sampling && !rgb) return -1;
  orcs_lights_t* L = (orcs_lights_t*)malloc(sizeof(orcs_lights_t));
  orcs_build(sc, spheres_on, L);
  if (L->n_tri_found > ORCE_MAX_LIGHTS || (spheres_on && (L->n_sph_found < 1 || L->n_sph_found > ORCS_MAX_SPHERES)) ||
      (mode == 2 && L->tri.n + L->ns == 0 && !env_sampling)) {
    free(L);
    return -1;
  }
  orce_env_t env;
  orct_env_t sky;
  memset(&env, 0, sizeof env);
  memset(&sky, 0, sizeof sky);
  if (rgb) {
    orce_build(&env, rgb, env_width, env_height, env_flags, R);
    sky.width = env_width; sky.height = env_height; sky.flags = env_flags; sky.rgb = rgb;
    memcpy(sky.R, R, sizeof sky.R);
  }
  int dim = 2 + 2 * max_bounces;
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    v3 c = orcs_trace_path(sc, rgb ? &env : NULL, rgb ? &sky : NULL, L, mode, env_sampling, mutant, cx, cy, &smp, max_bounces);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  free(alpha);
  if (rgb) orce_free(&env);
  free(L);
  return 0;
}
