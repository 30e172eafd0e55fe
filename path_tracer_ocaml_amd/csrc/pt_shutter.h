/* pt_shutter.h -- the camera ray of a camera that moves while its shutter is open (include/ptx.h, "camera shutter"), written once
 * for host and device on top of pt_camera_pose.h and pt_projection.h.
 *
 * The header states the rule operation for operation; every expression below keeps its grouping (the build has
 * -ffp-contract=off, and nothing here is an fma: v3_dot and v3_cross are, so neither is used).  tests/shutter_reference.py and
 * tests/c/shutter_oracle.c restate it from the header's text, and the CPU tests compile this file for the host and compare bit for
 * bit.
 *
 * The vector is turned AFTER Rv and BEFORE it is normalised, so T = 0 and A = 0 (cs = 1, sn = 0, oc = 0) give the posed ray of the
 * same (cx, cy, u, v) -- up to the sign of a zero component (w * 1 + c * 0 + k * 0). */
#ifndef PT_SHUTTER_H
#define PT_SHUTTER_H

#include "pt_projection.h"

/* The shutter of a launch: while it is open the camera moves from o to o + tr and turns by `angle` about the unit axis k (scene
 * space); dim is the sampler's dimension, whose last one is the sample's time */
struct PtShutter {
  double tr[3];
  double k[3];
  double angle;
  int32_t dim;
};

/* Rot(k, t A) at one time: (sn, cs) = sincos(t A), oc = 1 - cs */
struct PtShutterTurn {
  double sn, cs, oc;
};
PT_HD PtShutterTurn pt_shutter_turn(const PtShutter& sh, double t) {
  PtShutterTurn s;
  const double a = t * sh.angle;
  pt_sincos(a, &s.sn, &s.cs);
  s.oc = 1.0 - s.cs;
  return s;
}
/* S(w) = w cs + (k x w) sn + k (k . w) oc */
PT_HD V3 pt_shutter_rotate(const PtShutter& sh, const PtShutterTurn& s, V3 w) {
  const double kx = sh.k[0], ky = sh.k[1], kz = sh.k[2];
  const double kw = (kx * w.x + ky * w.y) + kz * w.z;
  const V3 c = v3((ky * w.z) - (kz * w.y), (kz * w.x) - (kx * w.z), (kx * w.y) - (ky * w.x));
  const double ko = kw * s.oc;
  return v3(((w.x * s.cs) + (c.x * s.sn)) + (kx * ko), ((w.y * s.cs) + (c.y * s.sn)) + (ky * ko), ((w.z * s.cs) + (c.z * s.sn)) + (kz * ko));
}
/* ot = o + t T */
PT_HD V3 pt_shutter_origin(const PtCameraPose& cp, const PtShutter& sh, double t) {
  return v3(cp.o[0] + (t * sh.tr[0]), cp.o[1] + (t * sh.tr[1]), cp.o[2] + (t * sh.tr[2]));
}

/* the posed camera at time t: pt_camera_pose_ray's operands, and the sample's time */
template <bool LENS>
PT_HD void pt_shutter_pose_ray(const PtCameraPose& cp, const PtShutter& sh, double cx, double cy, double radius, double focus, double u, double v,
                               double t, V3* origin, V3* direction) {
  V3 e, l;
  pt_camera_pose_vectors<LENS>(cp, cx, cy, radius, focus, u, v, &e, &l);
  const PtShutterTurn s = pt_shutter_turn(sh, t);
  const V3 ot = pt_shutter_origin(cp, sh, t);
  if (!LENS) {
    *origin = ot;
  } else {
    const V3 sl = pt_shutter_rotate(sh, s, pt_pose_rotate(cp, l));
    *origin = v3(ot.x + sl.x, ot.y + sl.y, ot.z + sl.z);
  }
  *direction = v3_normalize(pt_shutter_rotate(sh, s, pt_pose_rotate(cp, e)));
}

/* the lat-long camera at time t */
PT_HD void pt_shutter_latlong_ray(const PtCameraPose& cp, const PtShutter& sh, double cx, double cy, double t, V3* origin, V3* direction) {
  const PtShutterTurn s = pt_shutter_turn(sh, t);
  *origin = pt_shutter_origin(cp, sh, t);
  *direction = v3_normalize(pt_shutter_rotate(sh, s, pt_pose_rotate(cp, pt_latlong_vector(cx, cy))));
}

#endif /* PT_SHUTTER_H */
