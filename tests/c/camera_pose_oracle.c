/* camera_pose_oracle.c -- the CPU restatement of the camera pose (include/ptx.h, "camera pose: a movable camera, no rebuild"), on top
 * of lens_oracle.c, which is included unchanged (and envlight_oracle.c, texture_oracle.c and the oracle through it): this library
 * carries its own copy of the oracle (call this copy's orc_set_math(0) before comparing with the GPU).
 *
 * Written from the header's text, not from the kernel:
 *
 *   q  = (llx + (vx * cx), lly + (vy * cy), -1.0)            with the pose's view if it has one, else the scene's
 *   no lens:  e = q;  l = none
 *   lens:     P = (F * q.x, F * q.y, F * q.z);  L as in the lens rule;  e = P - L;  l = L
 *   Rv(a) = ((r00 * a.x + r01 * a.y) + r02 * a.z, (r10 * a.x + r11 * a.y) + r12 * a.z, (r20 * a.x + r21 * a.y) + r22 * a.z)
 *   direction = normalize(Rv(e));  origin = no lens: o exactly;  lens: o + Rv(l), component by component
 *   the sampler is the pinhole's (2 + 2 max_bounces dimensions) or, with a lens, the lens's (4 + 2 max_bounces, the pair last)
 *
 * Whole paths: the camera ray is handed to orcn_trace_path, the one path loop that takes its ray as an argument.
 *
 * Build: oracle/Makefile's flags (tests/camera_pose_support.py). */
#include "lens_oracle.c"

/* pose: o[3], R[9] row-major, then has_view and view[4] */
typedef struct {
  double o[3], R[9];
  int has_view;
  ptx_camera view;
} orcp_pose_t;

static v3 orcp_rotate(const double* R, v3 a) {
  return v3_make((R[0] * a.x + R[1] * a.y) + R[2] * a.z, (R[3] * a.x + R[4] * a.y) + R[5] * a.z, (R[6] * a.x + R[7] * a.y) + R[8] * a.z);
}

/* A > 0: a lens of radius A focused at F with the pair (u, v); otherwise none of the three is read */
static ray_t orcp_pose_ray(const ptx_camera* c, const double* o, const double* R, double cx, double cy, double A, double F, double u, double v) {
  const double pi = 3.14159265358979323846;
  const v3 q = v3_make(c->lower_left_x + (c->view_x * cx), c->lower_left_y + (c->view_y * cy), -1.0);
  if (!(A > 0.0)) return ray_create(v3_make(o[0], o[1], o[2]), v3_normalize(orcp_rotate(R, q)));
  const v3 P = v3_make(F * q.x, F * q.y, F * q.z);
  const double r = sqrt(u);
  const double th = (v * 2.0) * pi;
  const double lx = r * m_cos(th), ly = r * m_sin(th);
  const v3 L = v3_make(A * lx, A * ly, 0.0);
  const v3 e = v3_make(P.x - L.x, P.y - L.y, P.z - L.z);
  const v3 rl = orcp_rotate(R, L);
  return ray_create(v3_make(o[0] + rl.x, o[1] + rl.y, o[2] + rl.z), v3_normalize(orcp_rotate(R, e)));
}

static orcp_pose_t orcp_pose(const double* o, const double* R, const double* view4) {
  orcp_pose_t p;
  memcpy(p.o, o, sizeof p.o);
  memcpy(p.R, R, sizeof p.R);
  p.has_view = view4 != NULL;
  if (view4) { p.view.lower_left_x = view4[0]; p.view.lower_left_y = view4[1]; p.view.view_x = view4[2]; p.view.view_y = view4[3]; }
  return p;
}

/* the camera ray of a sample whose sampler and film coordinates orct_sample made; dim: the sampler's dimension */
static ray_t orcp_camera_ray(const orc_scene* sc, const orcp_pose_t* p, const sampler_t* smp, double cx, double cy, double A, double F, int dim) {
  const ptx_camera* c = p->has_view ? &p->view : &sc->camera;
  double u = 0.0, v = 0.0;
  if (A > 0.0) { u = sample_dim(smp, dim - 2); v = sample_dim(smp, dim - 1); }
  return orcp_pose_ray(c, p->o, p->R, cx, cy, A, F, u, v);
}

static void orcp_put_ray(double* out, const ray_t* r) {
  out[0] = r->origin.x; out[1] = r->origin.y; out[2] = r->origin.z;
  out[3] = r->direction.x; out[4] = r->direction.y; out[5] = r->direction.z;
}

/* the rule on explicit inputs: cam4 = (llx, lly, vx, vy), cxcy and uv n x 2 -> rays n x 6 (origin, direction) */
ORC_API void orcp_pose_rays(const double* cam4, const double* o, const double* R, double A, double F, int64_t n, const double* cxcy,
                            const double* uv, double* rays_out) {
  const ptx_camera c = {cam4[0], cam4[1], cam4[2], cam4[3]};
  for (int64_t i = 0; i < n; ++i) {
    const ray_t r = orcp_pose_ray(&c, o, R, cxcy[2 * i], cxcy[2 * i + 1], A, F, uv[2 * i], uv[2 * i + 1]);
    orcp_put_ray(rays_out + 6 * i, &r);
  }
}

/* the camera rays of explicit samples: rays n x 6.  view4 NULL: the scene's own view. */
ORC_API void orcp_sample_rays(const orc_scene* sc, const double* o, const double* R, const double* view4, double A, double F, int width, int height,
                              int spp, int max_bounces, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes, double* rays_out) {
  const orcp_pose_t pose = orcp_pose(o, R, view4);
  const int dim = orcn_dim(A, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t r = orcp_camera_ray(sc, &pose, &smp, cx, cy, A, F, dim);
    orcp_put_ray(rays_out + 6 * i, &r);
  }
  free(alpha);
}

/* Per-sample radiance from the posed camera; the arguments before the pose are orcn_trace_samples'.  Returns 0, or -1 when mode 2 has
 * nothing to sample. */
ORC_API int orcp_trace_samples(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height,
                               int env_flags, const double* envR, int mode, int sampling, const double* o, const double* R, const double* view4,
                               double A, double F, int width, int height, int spp, int max_bounces, int64_t n, const int32_t* xs,
                               const int32_t* ys, const int32_t* passes, double* rgb_out, int64_t* segments_out) {
  if (mode < 0 || mode > 2 || (sampling && !env_rgb)) return -1;
  const orcp_pose_t pose = orcp_pose(o, R, view4);
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
  const int dim = orcn_dim(A, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  int64_t segments = 0;
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t ray = orcp_camera_ray(sc, &pose, &smp, cx, cy, A, F, dim);
    v3 c = orcn_trace_path(sc, images, env_rgb ? &sky : NULL, sampling ? &dens : NULL, L, mode, sampling, ray, &smp, max_bounces, &segments);
    rgb_out[3 * i] = c.x; rgb_out[3 * i + 1] = c.y; rgb_out[3 * i + 2] = c.z;
  }
  if (segments_out) *segments_out = segments;
  free(alpha);
  if (env_rgb && sampling) orce_free(&dens);
  free(L);
  return 0;
}

/* The first hit of every sample's posed camera ray as the feature record states it (orcn_first_hits with the posed ray): feat_out
 * n x 8 = albedo, the facing normal (scene space), depth = t along the posed ray, hits */
ORC_API void orcp_first_hits(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height, int env_flags,
                             const double* envR, const double* o, const double* R, const double* view4, double A, double F, int width, int height,
                             int spp, int max_bounces, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes, double* feat_out) {
  const orcp_pose_t pose = orcp_pose(o, R, view4);
  orct_env_t sky = {env_width, env_height, env_flags, env_rgb, {0}};
  if (env_rgb) memcpy(sky.R, envR, sizeof sky.R);
  const int dim = orcn_dim(A, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy, t = 0.0;
    int prim = -1;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t ray = orcp_camera_ray(sc, &pose, &smp, cx, cy, A, F, dim);
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
