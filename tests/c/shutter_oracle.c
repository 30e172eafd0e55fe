/* shutter_oracle.c -- the CPU restatement of the camera shutter (include/ptx.h, "camera shutter: motion blur between two poses"), on
 * top of rays_oracle.c, which is included unchanged (and camera_pose_oracle.c, lens_oracle.c, envlight_oracle.c, texture_oracle.c and
 * the oracle through it): this library carries its own copy of the oracle (call this copy's orc_set_math(0) before comparing with the
 * GPU).
 *
 * Written from the header's text, not from the kernel:
 *
 *   a = t * A;  (sn, cs) = sincos(a);  oc = 1.0 - cs
 *   S(w):  kw = (k.x * w.x + k.y * w.y) + k.z * w.z
 *          c  = ((k.y * w.z) - (k.z * w.y), (k.z * w.x) - (k.x * w.z), (k.x * w.y) - (k.y * w.x))
 *          S(w).i = ((w.i * cs) + (c.i * sn)) + (k.i * (kw * oc))
 *   ot = (o.x + (t * T.x), o.y + (t * T.y), o.z + (t * T.z))
 *   pose, no lens:  direction = normalize(S(Rv(q)));      origin = ot
 *   pose, lens:     direction = normalize(S(Rv(P - L)));  origin = ot + S(Rv(L)), component by component
 *   lat-long:       direction = normalize(S(Rv(e)));      origin = ot
 *   the sampler has d = 2 + 2 max_bounces (+ 2 with a lens) + 1 dimensions; t is dimension d - 1, the lens pair d - 3 and d - 2
 *
 * Whole paths: the camera ray is handed to orcn_trace_path, the one path loop that takes its ray as an argument, with the sample's
 * own offset and the d-dimensional table.
 *
 * Build: oracle/Makefile's flags (tests/shutter_support.py). */
#include "rays_oracle.c"

/* the camera state of a launch: the pose (identity at 0 while off), the view in effect, a lens (A > 0) and the projection */
typedef struct {
  double o[3], R[9];
  ptx_camera view;
  double A, F;
  int latlong;
  double T[3], k[3], angle;
} orcs_camera_t;

static int orcs_dim(const orcs_camera_t* c, int max_bounces) { return 2 + 2 * max_bounces + (c->A > 0.0 ? 2 : 0) + 1; }

static v3 orcs_turn(const double* k, double sn, double cs, double oc, v3 w) {
  const double kw = (k[0] * w.x + k[1] * w.y) + k[2] * w.z;
  const v3 c = v3_make((k[1] * w.z) - (k[2] * w.y), (k[2] * w.x) - (k[0] * w.z), (k[0] * w.y) - (k[1] * w.x));
  return v3_make(((w.x * cs) + (c.x * sn)) + (k[0] * (kw * oc)), ((w.y * cs) + (c.y * sn)) + (k[1] * (kw * oc)),
                 ((w.z * cs) + (c.z * sn)) + (k[2] * (kw * oc)));
}

/* (u, v): the lens pair (read with a lens only); t: the sample's time */
static ray_t orcs_shutter_ray(const orcs_camera_t* c, double cx, double cy, double u, double v, double t) {
  const double pi = 3.14159265358979323846;
  const double a = t * c->angle;
  const double sn = m_sin(a), cs = m_cos(a);
  const double oc = 1.0 - cs;
  const v3 ot = v3_make(c->o[0] + (t * c->T[0]), c->o[1] + (t * c->T[1]), c->o[2] + (t * c->T[2]));
  if (c->latlong) {
    const double eu = cx;
    const double ev = 1.0 - cy;
    const double al = eu * (2.0 * pi) - pi;
    const double th = ev * pi;
    const double sa = m_sin(al), ca = m_cos(al), st = m_sin(th), ct = m_cos(th);
    const v3 e = v3_make(st * ca, -ct, -(st * sa));
    return ray_create(ot, v3_normalize(orcs_turn(c->k, sn, cs, oc, orcp_rotate(c->R, e))));
  }
  const v3 q = v3_make(c->view.lower_left_x + (c->view.view_x * cx), c->view.lower_left_y + (c->view.view_y * cy), -1.0);
  if (!(c->A > 0.0)) return ray_create(ot, v3_normalize(orcs_turn(c->k, sn, cs, oc, orcp_rotate(c->R, q))));
  const v3 P = v3_make(c->F * q.x, c->F * q.y, c->F * q.z);
  const double r = sqrt(u);
  const double th = (v * 2.0) * pi;
  const double lx = r * m_cos(th), ly = r * m_sin(th);
  const v3 L = v3_make(c->A * lx, c->A * ly, 0.0);
  const v3 e = v3_make(P.x - L.x, P.y - L.y, P.z - L.z);
  const v3 sl = orcs_turn(c->k, sn, cs, oc, orcp_rotate(c->R, L));
  return ray_create(v3_make(ot.x + sl.x, ot.y + sl.y, ot.z + sl.z), v3_normalize(orcs_turn(c->k, sn, cs, oc, orcp_rotate(c->R, e))));
}

/* state: o[3], R[9], view4 (NULL: the scene's own), A, F, latlong, T[3], k[3], angle */
static orcs_camera_t orcs_camera(const orc_scene* sc, const double* o, const double* R, const double* view4, double A, double F, int latlong,
                                 const double* T, const double* k, double angle) {
  orcs_camera_t c;
  memcpy(c.o, o, sizeof c.o);
  memcpy(c.R, R, sizeof c.R);
  c.view = sc->camera;
  if (view4) { c.view.lower_left_x = view4[0]; c.view.lower_left_y = view4[1]; c.view.view_x = view4[2]; c.view.view_y = view4[3]; }
  c.A = A; c.F = F; c.latlong = latlong;
  memcpy(c.T, T, sizeof c.T);
  memcpy(c.k, k, sizeof c.k);
  c.angle = angle;
  return c;
}

/* the camera ray of a sample whose sampler and film coordinates orct_sample made; dim: the sampler's dimension */
static ray_t orcs_camera_ray(const orcs_camera_t* c, const sampler_t* smp, double cx, double cy, int dim) {
  double u = 0.0, v = 0.0;
  if (c->A > 0.0) { u = sample_dim(smp, dim - 3); v = sample_dim(smp, dim - 2); }
  return orcs_shutter_ray(c, cx, cy, u, v, sample_dim(smp, dim - 1));
}

/* the camera rays of explicit samples: rays n x 6 */
ORC_API void orcs_sample_rays(const orc_scene* sc, const double* o, const double* R, const double* view4, double A, double F, int latlong,
                              const double* T, const double* k, double angle, int width, int height, int spp, int max_bounces, int64_t n,
                              const int32_t* xs, const int32_t* ys, const int32_t* passes, double* rays_out) {
  const orcs_camera_t c = orcs_camera(sc, o, R, view4, A, F, latlong, T, k, angle);
  const int dim = orcs_dim(&c, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t r = orcs_camera_ray(&c, &smp, cx, cy, dim);
    orcp_put_ray(rays_out + 6 * i, &r);
  }
  free(alpha);
}

/* Per-sample radiance from the moving camera; the arguments before the pose are orcn_trace_samples'.  Returns 0, or -1 when mode 2 has
 * nothing to sample. */
ORC_API int orcs_trace_samples(const orc_scene* sc, const orct_image_t* images, const double* env_rgb, int env_width, int env_height,
                               int env_flags, const double* envR, int mode, int sampling, const double* o, const double* R, const double* view4,
                               double A, double F, int latlong, const double* T, const double* k, double angle, int width, int height, int spp,
                               int max_bounces, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes, double* rgb_out,
                               int64_t* segments_out) {
  if (mode < 0 || mode > 2 || (sampling && !env_rgb)) return -1;
  const orcs_camera_t c = orcs_camera(sc, o, R, view4, A, F, latlong, T, k, angle);
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
  const int dim = orcs_dim(&c, max_bounces);
  double* alpha = (double*)malloc(sizeof(double) * (size_t)dim);
  orc_lds_alpha(dim, alpha);
  int64_t segments = 0;
  for (int64_t i = 0; i < n; ++i) {
    sampler_t smp;
    double cx, cy;
    orct_sample(alpha, width, height, spp, xs[i], ys[i], passes[i], &smp, &cx, &cy);
    const ray_t ray = orcs_camera_ray(&c, &smp, cx, cy, dim);
    v3 rgb = orcn_trace_path(sc, images, env_rgb ? &sky : NULL, sampling ? &dens : NULL, L, mode, sampling, ray, &smp, max_bounces, &segments);
    rgb_out[3 * i] = rgb.x; rgb_out[3 * i + 1] = rgb.y; rgb_out[3 * i + 2] = rgb.z;
  }
  if (segments_out) *segments_out = segments;
  free(alpha);
  if (env_rgb && sampling) orce_free(&dens);
  free(L);
  return 0;
}
