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
static v3 orct_texel(const double* rgb, int width, long long ix, long long iy) {
  const double* c = rgb + 3 * (iy * (long long)width + ix);
  return v3_make(c[0], c[1], c[2]);
}
static v3 orct_lerp(v3 a, v3 b, double t) {
  return v3_make(a.x * (1.0 - t) + b.x * t, a.y * (1.0 - t) + b.y * t, a.z * (1.0 - t) + b.z * t);
}
static v3 orct_image(const double* rgb, int W, int H, int flags, double u, double v) {
  const int rep_u = (flags & PTX_IMAGE_REPEAT_U) != 0, rep_v = (flags & PTX_IMAGE_REPEAT_V) != 0;
  const double p = orct_scale(u, W), q = orct_scale(v, H);
  if (!(flags & PTX_IMAGE_BILINEAR)) return orct_texel(rgb, W, orct_wrap((long long)p, W, rep_u), orct_wrap((long long)q, H, rep_v));
  const double x = p - 0.5, y = q - 0.5;
  const double x0 = floor(x), y0 = floor(y);
  const double fx = x - x0, fy = y - y0;
  const long long ix0 = orct_wrap((long long)x0, W, rep_u), ix1 = orct_wrap((long long)x0 + 1, W, rep_u);
  const long long iy0 = orct_wrap((long long)y0, H, rep_v), iy1 = orct_wrap((long long)y0 + 1, H, rep_v);
  const v3 top = orct_lerp(orct_texel(rgb, W, ix0, iy0), orct_texel(rgb, W, ix1, iy0), fx);
  const v3 bot = orct_lerp(orct_texel(rgb, W, ix0, iy1), orct_texel(rgb, W, ix1, iy1), fx);
  return orct_lerp(top, bot, fy);
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
