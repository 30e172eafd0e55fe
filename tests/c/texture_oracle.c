/* texture_oracle.c -- the CPU restatement of the image rule and the environment (include/ptx.h, "image textures and a lat-long
 * environment map"), on top of the oracle: the oracle's source is included unchanged, so this library carries its own copy of the
 * oracle (orc_* with their own globals: call this copy's orc_set_math(0) before comparing with the GPU) plus the entry points below.
 *
 * Written from the header's text, not from the kernel:
 *
 *   wrap of i on an axis of n texels: repeat ((i % n) + n) % n; clamp min(max(i, 0), n - 1)
 *   p = u * W, q = v * H; a product that is NaN or not below 2^62 in magnitude counts as 0
 *   nearest:  texel (wrap((long long)p), wrap((long long)q))
 *   bilinear: x = p - 0.5, x0 = floor(x), fx = x - x0, ix0 = wrap(x0), ix1 = wrap(x0 + 1); the same for y;
 *             top = c00 (1 - fx) + c10 fx; bot = c01 (1 - fx) + c11 fx; result = top (1 - fy) + bot fy
 *   environment: e = normalize(d); m_k = (R[3k] e.x + R[3k+1] e.y) + R[3k+2] e.z;
 *             u = (pi + atan2(-m.z, m.x)) (1 / 2 pi); v = acos(-min(max(m.y, -1), 1)) (1 / pi); repeat in u, clamp in v
 *   orct_trace_samples: the oracle's trace_path with the miss colour replaced by the environment's.
 *   orct_trace_samples_images: the same with an image table, one record per texture-table index (width 0: the descriptor's texture),
 *             and the environment optional (NULL: the oracle's own background).  A hit calls the oracle's hit_scatter; where the
 *             material's texture entry carries an image and the material is no dielectric, the colour a = image(tex_coord) takes
 *             the place of Texture.eval's: a Lambertian's attenuation is a, a metal's that did not absorb a + (1 - a) * pow5(1 -
 *             omega_i.z), grouped as hit_scatter groups it.  A dielectric ignores the image; emission stays the material's.
 *   orct_first_hits: per sample the first hit's albedo as the feature pass defines it -- (1, 1, 1) on a dielectric, the background
 *             or the environment at a miss, the texture or image colour otherwise -- a hit flag and the texture index hit (or -1).
 *
 * ORCT_MUT_*: a `mutant` argument of the two entry points above restates the rule WRONGLY in one chosen way.  The CPU tests use it
 * to show that their scenes and images tell each such mistake from the rule; every comparison with the GPU passes 0.
 *
 * Build: oracle/Makefile's flags (tests/texture_support.py). */
#include "../../oracle/pt_oracle.c"

typedef struct {
  int width, height, flags;
  const double* rgb; /* width * height * 3, row 0 = v 0 */
  double R[9];
} orct_env_t;

static long long orct_wrap(long long i, long long n, int repeat) {
  if (repeat) return ((i % n) + n) % n;
  long long lo = i < 0 ? 0 : i;
  return lo > n - 1 ? n - 1 : lo;
}
static double orct_scale(double u, int n) {
  double p = u * (double)n;
  if (p != p || fabs(p) >= 0x1p62) return 0.0;
  return p;
}
enum { ORCT_MUT_NONE = 0, ORCT_MUT_SWAP_UV, ORCT_MUT_FLIP_V, ORCT_MUT_NEAREST, ORCT_MUT_NEXT_COLUMN, ORCT_MUT_STRIDE_H,
       ORCT_MUT_TOGGLE_REPEAT_U, ORCT_MUT_TOGGLE_REPEAT_V, ORCT_MUT_METAL_PLAIN };

static v3 orct_texel(const double* rgb, int width, long long ix, long long iy) {
  const double* c = rgb + 3 * (iy * (long long)width + ix);
  return v3_make(c[0], c[1], c[2]);
}
static v3 orct_lerp(v3 a, v3 b, double t) {
  return v3_make(a.x * (1.0 - t) + b.x * t, a.y * (1.0 - t) + b.y * t, a.z * (1.0 - t) + b.z * t);
}
/* the rule; `mutant` != 0 departs from it (the wrong row stride stays inside the array by wrapping the texel's offset) */
static v3 orct_image_m(const double* rgb, int W, int H, int flags, double u, double v, int mutant) {
  if (mutant == ORCT_MUT_SWAP_UV) { double t = u; u = v; v = t; }
  if (mutant == ORCT_MUT_FLIP_V) v = 1.0 - v;
  if (mutant == ORCT_MUT_NEAREST) flags &= ~PTX_IMAGE_BILINEAR;
  if (mutant == ORCT_MUT_TOGGLE_REPEAT_U) flags ^= PTX_IMAGE_REPEAT_U;
  if (mutant == ORCT_MUT_TOGGLE_REPEAT_V) flags ^= PTX_IMAGE_REPEAT_V;
  const long long dx = mutant == ORCT_MUT_NEXT_COLUMN ? 1 : 0;
  const int rep_u = (flags & PTX_IMAGE_REPEAT_U) != 0, rep_v = (flags & PTX_IMAGE_REPEAT_V) != 0;
  const double p = orct_scale(u, W), q = orct_scale(v, H);
  long long ix[2], iy[2];
  double fx = 0.0, fy = 0.0;
  if (!(flags & PTX_IMAGE_BILINEAR)) {
    ix[0] = ix[1] = orct_wrap((long long)p + dx, W, rep_u);
    iy[0] = iy[1] = orct_wrap((long long)q, H, rep_v);
  } else {
    const double x = p - 0.5, y = q - 0.5;
    const double x0 = floor(x), y0 = floor(y);
    fx = x - x0; fy = y - y0;
    ix[0] = orct_wrap((long long)x0 + dx, W, rep_u); ix[1] = orct_wrap((long long)x0 + 1 + dx, W, rep_u);
    iy[0] = orct_wrap((long long)y0, H, rep_v); iy[1] = orct_wrap((long long)y0 + 1, H, rep_v);
  }
  v3 c[2][2];
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < 2; ++i)
      c[j][i] = mutant == ORCT_MUT_STRIDE_H ? orct_texel(rgb, 1, (iy[j] * (long long)H + ix[i]) % ((long long)W * H), 0)
                                            : orct_texel(rgb, W, ix[i], iy[j]);
  if (!(flags & PTX_IMAGE_BILINEAR)) return c[0][0];
  return orct_lerp(orct_lerp(c[0][0], c[0][1], fx), orct_lerp(c[1][0], c[1][1], fx), fy);
}
static v3 orct_image(const double* rgb, int W, int H, int flags, double u, double v) {
  return orct_image_m(rgb, W, H, flags, u, v, ORCT_MUT_NONE);
}
static v3 orct_environment(const orct_env_t* env, v3 d) {
  const double pi = 3.14159265358979323846;
  const v3 e = v3_normalize(d);
  const double* R = env->R;
  const double mx = (R[0] * e.x + R[1] * e.y) + R[2] * e.z;
  const double my = (R[3] * e.x + R[4] * e.y) + R[5] * e.z;
  const double mz = (R[6] * e.x + R[7] * e.y) + R[8] * e.z;
  const double lo = my < -1.0 ? -1.0 : my;
  const double cy = lo > 1.0 ? 1.0 : lo;
  const double u = (pi + m_atan2(-mz, mx)) * (1.0 / (2.0 * pi));
  const double v = m_acos(-cy) * (1.0 / pi);
  return orct_image(env->rgb, env->width, env->height, (env->flags & PTX_IMAGE_BILINEAR) | PTX_IMAGE_REPEAT_U, u, v);
}

ORC_API void orct_image_eval(const double* rgb, int width, int height, int flags, int64_t n, const double* uv, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    v3 c = orct_image(rgb, width, height, flags, uv[2 * i], uv[2 * i + 1]);
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
  }
}

ORC_API void orct_environment_eval(const double* rgb, int width, int height, int flags, const double* R, int64_t n, const double* dirs,
                                   double* out) {
  orct_env_t env = {width, height, flags, rgb, {0}};
  memcpy(env.R, R, sizeof env.R);
  for (int64_t i = 0; i < n; ++i) {
    v3 c = orct_environment(&env, v3_make(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
  }
}

/* path_tracer (integrator.ml:16-69) as the oracle's trace_path states it, the miss colour the environment's */
static v3 trace_path_env(const orc_scene* sc, const orct_env_t* env, double cx, double cy, const sampler_t* smp, int max_bounces) {
  ray_t ray = camera_ray(&sc->camera, cx, cy);
  int samples_index = 2;
  v3 emit0 = v3_make(0.0, 0.0, 0.0), attn0 = v3_make(1.0, 1.0, 1.0);
  const v3 black = v3_make(0.0, 0.0, 0.0);
  for (;;) {
    if (max_bounces <= 0) return add_mul(emit0, attn0, black);
    max_bounces = max_bounces - 1;
    hit_t h;
    if (!scene_intersect(sc, &ray, &h, NULL, NULL, NULL)) return add_mul(emit0, attn0, orct_environment(env, ray.direction));
    v3 emit = h.emit;
    int j = samples_index;
    double u = sample_dim(smp, j), v = sample_dim(smp, j + 1);
    samples_index = j + 2;
    scatter_t s = hit_scatter(&sc->mt, &h, u);
    if (s.kind == SC_ABSORB) return add_mul(emit0, attn0, emit);
    if (s.kind == SC_SPECULAR) {
      v3 ne = add_mul(emit, s.attenuation, emit0);
      attn0 = v3_mul(s.attenuation, attn0);
      emit0 = ne;
      ray = s.ray;
      continue;
    }
    v3 dir = unit_square_to_hemisphere(u, v);
    double diffuse_pd = pdf_eval_diffuse(dir);
    if (diffuse_pd == 0.0) return add_mul(emit0, attn0, emit);
    double pd = diffuse_pd / diffuse_pd;
    if (!pt_isfinite(pd)) return add_mul(emit0, attn0, emit);
    ray_t scattered = sspace_world_ray(&h.shader_space, dir);
    v3 attenuation = v3_scale(s.attenuation, pd);
    v3 ne = add_mul(emit, attenuation, emit0);
    attn0 = v3_mul(attenuation, attn0);
    emit0 = ne;
    ray = scattered;
  }
}

/* orc_trace_samples under the environment (rgb, width, height, flags, R) */
ORC_API void orct_trace_samples(const orc_scene* sc, const double* rgb, int env_width, int env_height, int env_flags, const double* R,
                                int width, int height, int spp, int max_bounces, int64_t n, const int32_t* xs, const int32_t* ys,
                                const int32_t* passes, double* rgb_out) {
  orct_env_t env = {env_width, env_height, env_flags, rgb, {0}};
  memcpy(env.R, R, sizeof env.R);
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
    v3 c = trace_path_env(sc, &env, cx, cy, &smp, max_bounces);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  free(alpha);
}

/* one record per texture-table index; width 0: the descriptor's texture */
typedef struct {
  const double* rgb; /* width * height * 3, row 0 = v 0 */
  int32_t width, height, flags, reserved;
} orct_image_t;

static const orct_image_t* orct_image_of(const orct_image_t* images, const ptx_material* m) {
  if (!images || m->kind == PTX_MAT_DIELECTRIC || images[m->texture].width == 0) return NULL;
  return &images[m->texture];
}

/* Material.scatter as hit_scatter states it, the texture's colour the image's where the entry carries one */
static scatter_t orct_scatter(const orc_scene* sc, const orct_image_t* images, int mutant, const hit_t* h, double u) {
  scatter_t s = hit_scatter(&sc->mt, h, u);
  const orct_image_t* im = orct_image_of(images, h->m);
  if (!im) return s;
  const v3 a = orct_image_m(im->rgb, im->width, im->height, im->flags, h->tex_coord.u, h->tex_coord.v, mutant);
  if (h->m->kind == PTX_MAT_LAMBERTIAN) s.attenuation = a;
  else if (s.kind == SC_SPECULAR) { /* a metal that did not absorb */
    const double sp = m_pow5(1.0 - h->omega_i.z);
    const v3 c = v3_scale(v3_sub(v3_make(1.0, 1.0, 1.0), a), sp);
    s.attenuation = mutant == ORCT_MUT_METAL_PLAIN ? a : v3_add(a, c);
  }
  return s;
}

static v3 orct_miss(const orc_scene* sc, const orct_env_t* env, const ray_t* ray) {
  return env ? orct_environment(env, ray->direction) : scene_background(sc, ray);
}

/* path_tracer (integrator.ml:16-69) as the oracle's trace_path states it, the miss colour the environment's (if any) and the
 * scatter orct_scatter */
static v3 trace_path_images(const orc_scene* sc, const orct_image_t* images, const orct_env_t* env, int mutant, double cx, double cy,
                            const sampler_t* smp, int max_bounces) {
  ray_t ray = camera_ray(&sc->camera, cx, cy);
  int samples_index = 2;
  v3 emit0 = v3_make(0.0, 0.0, 0.0), attn0 = v3_make(1.0, 1.0, 1.0);
  const v3 black = v3_make(0.0, 0.0, 0.0);
  for (;;) {
    if (max_bounces <= 0) return add_mul(emit0, attn0, black);
    max_bounces = max_bounces - 1;
    hit_t h;
    if (!scene_intersect(sc, &ray, &h, NULL, NULL, NULL)) return add_mul(emit0, attn0, orct_miss(sc, env, &ray));
    v3 emit = h.emit;
    int j = samples_index;
    double u = sample_dim(smp, j), v = sample_dim(smp, j + 1);
    samples_index = j + 2;
    scatter_t s = orct_scatter(sc, images, mutant, &h, u);
    if (s.kind == SC_ABSORB) return add_mul(emit0, attn0, emit);
    if (s.kind == SC_SPECULAR) {
      v3 ne = add_mul(emit, s.attenuation, emit0);
      attn0 = v3_mul(s.attenuation, attn0);
      emit0 = ne;
      ray = s.ray;
      continue;
    }
    v3 dir = unit_square_to_hemisphere(u, v);
    double diffuse_pd = pdf_eval_diffuse(dir);
    if (diffuse_pd == 0.0) return add_mul(emit0, attn0, emit);
    double pd = diffuse_pd / diffuse_pd;
    if (!pt_isfinite(pd)) return add_mul(emit0, attn0, emit);
    ray_t scattered = sspace_world_ray(&h.shader_space, dir);
    v3 attenuation = v3_scale(s.attenuation, pd);
    v3 ne = add_mul(emit, attenuation, emit0);
    attn0 = v3_mul(attenuation, attn0);
    emit0 = ne;
    ray = scattered;
  }
}

/* the camera ray of sample (x, y, pass) as sample_pixel makes it (integrator.ml:96-109) */
static void orct_sample(const double* alpha, int width, int height, int spp, int x, int y, int pass, sampler_t* smp, double* cx,
                        double* cy) {
  double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  smp->alpha = alpha;
  smp->offset = (y * width) + x + (pass * spp);
  double dx = sample_dim(smp, 0), dy = sample_dim(smp, 1);
  *cx = ((double)x + dx) * widthf;
  *cy = 1.0 - (((double)y + dy) * heightf);
}

/* orc_trace_samples under an image table (NULL: none) and an environment (env_rgb NULL: the descriptor's background) */
ORC_API void orct_trace_samples_images(const orc_scene* sc, const orct_image_t* images, int mutant, const double* env_rgb,
                                       int env_width, int env_height, int env_flags, const double* R, int width, int height, int spp,
                                       int max_bounces, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes,
                                       double* rgb_out) {
  orct_env_t env = {env_width, env_height, env_flags, env_rgb, {0}};
  if (env_rgb) memcpy(env.R, R, sizeof env.R);
  int dim = 2 + 2 * max_bounces;
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    v3 c = trace_path_images(sc, images, env_rgb ? &env : NULL, mutant, cx, cy, &smp, max_bounces);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  free(alpha);
}

/* the first hit of every sample's camera ray: albedo (n x 3), hit flag, the texture index hit (-1 at a miss and on a dielectric); uv_out (nullable, n x 2) the
 * hit's texture coordinates */
ORC_API void orct_first_hits(const orc_scene* sc, const orct_image_t* images, int mutant, const double* env_rgb, int env_width,
                             int env_height, int env_flags, const double* R, int width, int height, int spp, int max_bounces, int64_t n,
                             const int32_t* xs, const int32_t* ys, const int32_t* passes, double* albedo_out, int32_t* hit_out,
                             int32_t* texture_out, double* uv_out) {
  orct_env_t env = {env_width, env_height, env_flags, env_rgb, {0}};
  if (env_rgb) memcpy(env.R, R, sizeof env.R);
  int dim = 2 + 2 * max_bounces;
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    ray_t ray = camera_ray(&sc->camera, cx, cy);
    hit_t h;
    v3 a;
    hit_out[i] = scene_intersect(sc, &ray, &h, NULL, NULL, NULL);
    texture_out[i] = -1;
    if (uv_out) uv_out[2 * i] = uv_out[2 * i + 1] = 0.0;
    if (!hit_out[i]) a = orct_miss(sc, env_rgb ? &env : NULL, &ray);
    else {
      const orct_image_t* im = orct_image_of(images, h.m);
      texture_out[i] = h.m->kind == PTX_MAT_DIELECTRIC ? -1 : h.m->texture;
      if (uv_out) { uv_out[2 * i] = h.tex_coord.u; uv_out[2 * i + 1] = h.tex_coord.v; }
      if (h.m->kind == PTX_MAT_DIELECTRIC) a = v3_make(1.0, 1.0, 1.0);
      else if (im) a = orct_image_m(im->rgb, im->width, im->height, im->flags, h.tex_coord.u, h.tex_coord.v, mutant);
      else a = texture_eval(&sc->mt, h.m->texture, h.tex_coord);
    }
    albedo_out[3 * i] = a.x; albedo_out[3 * i + 1] = a.y; albedo_out[3 * i + 2] = a.z;
  }
  free(alpha);
}
