/* lighting_oracle.c -- the CPU restatement of the lighting modes (ptx_scene_set_lighting), on top of the
 * oracle: the oracle's source is included unchanged, so this library carries its own copy of the oracle (orc_* with their own
 * globals: call this copy's orc_set_math(0) before comparing with the GPU) plus the three entry points below.
 *
 * Written from the rule's text, not from the kernel:
 *
 *   The light list: the scene's tree triangles whose material has a non-zero emit, in build-list order; per entry the vertices,
 *   n = normalize(cross(b - a, c - a)), A_k = 0.5 * sqrt(quadrance(cross(b - a, c - a))) and the running sum cum_k.
 *
 *   At a Diffuse scatter with hit point p and shader space ss, (u, v) the hit's two sampler dimensions:
 *     if u < 0.5:  x = (2u) * A_total; k = first k with x < cum_k (the last if none)
 *                  u2 = min((x - cum_{k-1}) / A_k, 1); s = sqrt(u2); b1 = 1 - s; b2 = v * s
 *                  q = a_k * (1 - b1 - b2) + b_k * b1 + c_k * b2;  dir = rotate ss (normalize (q - p))
 *     else:        dir = unit_square_to_hemisphere (2u - 1) v
 *     diffuse_pd = dir.z < 0 ? 0 : dir.z / pi; 0 ends the path with its emission
 *     w = rotate_inv ss dir
 *     light_pd = sum over k with Triangle.intersect(tri_k, ray(p, w), 0, max_finite) = Some t of (t * t) / (A_total * |dot(n_k, w)|)
 *     divisor = 0.5 * diffuse_pd + 0.5 * light_pd; pd = diffuse_pd / divisor; non-finite ends the path
 *     attenuation = texture * pd; ray = world_ray ss dir
 *   Modes 1 and 2: emit0' = add_mul emit0 attn0 emit (the old attn0) at both scatter sites; the terminal formulas are the same in
 *   all modes.  Mode 0 is the oracle's trace_path.
 *
 * Build: oracle/Makefile's flags (tests/lighting_support.py). */
#include "../../oracle/pt_oracle.c"

#define ORCL_MAX_LIGHTS 64
typedef struct { v3 a, b, c, n; double area, cum; } orcl_light_t;
typedef struct { int n; double area; orcl_light_t l[ORCL_MAX_LIGHTS]; } orcl_lights_t;

/* returns the number of emissive tree triangles (which may exceed ORCL_MAX_LIGHTS: then the list is not usable) */
static int lights_build(const orc_scene* sc, orcl_lights_t* L) {
  int n = 0;
  double cum = 0.0;
  L->n = 0;
  L->area = 0.0;
  for (int i = 0; i < sc->n_prims; ++i) {
    const prim_t* p = &sc->prims[i];
    if (p->kind != PRIM_TRIANGLE) continue;
    const ptx_material* m = &sc->mt.materials[p->material];
    if (m->emit[0] == 0.0 && m->emit[1] == 0.0 && m->emit[2] == 0.0) continue;
    if (n < ORCL_MAX_LIGHTS) {
      orcl_light_t* l = &L->l[n];
      v3 cr = v3_cross(v3_sub(p->b, p->a), v3_sub(p->c, p->a));
      l->a = p->a; l->b = p->b; l->c = p->c;
      l->n = v3_normalize(cr);
      l->area = 0.5 * sqrt(v3_quadrance(cr));
      cum = cum + l->area;
      l->cum = cum;
    }
    n++;
  }
  if (n <= ORCL_MAX_LIGHTS) { L->n = n; L->area = cum; }
  return n;
}

/* count and total area of the light list; out9 (optional, 14 doubles per light: a, b, c, n, A, cum) */
ORC_API int orcl_lights(const orc_scene* sc, double* area_out, double* out14) {
  orcl_lights_t L;
  int n = lights_build(sc, &L);
  if (area_out) *area_out = L.area;
  if (out14)
    for (int k = 0; k < L.n; ++k) {
      const orcl_light_t* l = &L.l[k];
      double r[14] = {l->a.x, l->a.y, l->a.z, l->b.x, l->b.y, l->b.z, l->c.x, l->c.y, l->c.z, l->n.x, l->n.y, l->n.z, l->area, l->cum};
      memcpy(out14 + 14 * k, r, sizeof r);
    }
  return n;
}

static double light_pd(const orcl_lights_t* L, v3 p, v3 w) {
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

/* the density, with respect to solid angle, with which the light half picks the world direction w (3 doubles) from p */
ORC_API double orcl_light_pd(const orc_scene* sc, const double* p, const double* w) {
  orcl_lights_t L;
  if (lights_build(sc, &L) > ORCL_MAX_LIGHTS) return NAN;
  return light_pd(&L, v3_make(p[0], p[1], p[2]), v3_make(w[0], w[1], w[2]));
}

/* the same for n directions (3 doubles each) from one point */
ORC_API int orcl_light_pd_many(const orc_scene* sc, const double* p, int64_t n, const double* ws, double* out) {
  orcl_lights_t L;
  if (lights_build(sc, &L) > ORCL_MAX_LIGHTS) return -1;
  for (int64_t i = 0; i < n; ++i) out[i] = light_pd(&L, v3_make(p[0], p[1], p[2]), v3_make(ws[3 * i], ws[3 * i + 1], ws[3 * i + 2]));
  return 0;
}

static v3 light_sample_dir(const orcl_lights_t* L, const sspace_t* ss, v3 p, double u, double v) {
  double x = (2.0 * u) * L->area;
  int k = L->n - 1;
  for (int j = 0; j < L->n; ++j)
    if (x < L->l[j].cum) { k = j; break; }
  double before = k > 0 ? L->l[k - 1].cum : 0.0;
  double u2 = pt_base_min((x - before) / L->l[k].area, 1.0);
  double s = sqrt(u2);
  double b1 = 1.0 - s, b2 = v * s;
  double b0 = 1.0 - b1 - b2;
  v3 q = v3_add(v3_add(v3_scale(L->l[k].a, b0), v3_scale(L->l[k].b, b1)), v3_scale(L->l[k].c, b2));
  return sspace_rotate(ss, v3_normalize(v3_sub(q, p)));
}

/* path_tracer (integrator.ml:16-69) with the emission summed in path order, and in mode 2 the mixture pdf */
static v3 trace_path_lit(const orc_scene* sc, const orcl_lights_t* L, int mode, double cx, double cy, const sampler_t* smp, int max_bounces) {
  ray_t ray = camera_ray(&sc->camera, cx, cy);
  int samples_index = 2;
  v3 emit0 = v3_make(0.0, 0.0, 0.0), attn0 = v3_make(1.0, 1.0, 1.0);
  const v3 black = v3_make(0.0, 0.0, 0.0);
  for (;;) {
    if (max_bounces <= 0) return add_mul(emit0, attn0, black);
    max_bounces = max_bounces - 1;
    hit_t h;
    if (!scene_intersect(sc, &ray, &h, NULL, NULL, NULL)) return add_mul(emit0, attn0, scene_background(sc, &ray));
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
    v3 dir;
    if (mode == 2) {
      if (u < 0.5) dir = light_sample_dir(L, &h.shader_space, h.shader_space.origin, u, v);
      else dir = unit_square_to_hemisphere(2.0 * u - 1.0, v);
    } else {
      dir = unit_square_to_hemisphere(u, v);
    }
    double diffuse_pd = pdf_eval_diffuse(dir);
    if (diffuse_pd == 0.0) return add_mul(emit0, attn0, emit);
    double divisor = diffuse_pd;
    if (mode == 2) {
      v3 w = sspace_rotate_inv(&h.shader_space, dir);
      divisor = 0.5 * diffuse_pd + 0.5 * light_pd(L, h.shader_space.origin, w);
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

/* orc_trace_samples in lighting mode `mode`; returns 0, or -1 when mode 2 is asked of a scene whose light list is empty or too long */
ORC_API int orcl_trace_samples(const orc_scene* sc, int mode, int width, int height, int spp, int max_bounces, int64_t n,
                               const int32_t* xs, const int32_t* ys, const int32_t* passes, double* rgb_out) {
  if (mode == 0) {
    orc_trace_samples(sc, width, height, spp, max_bounces, n, xs, ys, passes, rgb_out, NULL);
    return 0;
  }
  orcl_lights_t L;
  int nl = lights_build(sc, &L);
  if (mode == 2 && (nl == 0 || nl > ORCL_MAX_LIGHTS)) return -1;
  int dim = 2 + 2 * max_bounces;
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    smp.alpha = alpha;
    smp.offset = (ys[i] * width) + xs[i] + (passes[i] * spp);
    double dx = sample_dim(&smp, 0), dy = sample_dim(&smp, 1);
    double cx = ((double)xs[i] + dx) * widthf;
    double cy = 1.0 - (((double)ys[i] + dy) * heightf);
    v3 c = trace_path_lit(sc, &L, mode, cx, cy, &smp, max_bounces);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  free(alpha);
  return 0;
}
