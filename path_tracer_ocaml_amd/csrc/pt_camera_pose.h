/* pt_camera_pose.h -- the camera ray of a posed camera (include/ptx.h, "camera pose"), written once for host and device.
 *
 * The header states the rule operation for operation; every expression below keeps its grouping (the build has
 * -ffp-contract=off, and nothing here is an fma).  tests/c/camera_pose_oracle.c and tests/camera_pose_reference.py restate it from
 * the header's text, and the CPU tests compile this file for the host and compare bit for bit.
 *
 * The vector is rotated BEFORE it is normalised, so the identity rotation at origin 0 gives the pinhole's ray (1 * x + 0 * y is x
 * and 0 + x is x) and, with a lens, pt_lens.h's ray -- up to the sign of a zero component. */
#ifndef PT_CAMERA_POSE_H
#define PT_CAMERA_POSE_H

#include "pt_vec.h"

/* The pose of a launch: where the camera stands in scene space, its rotation (row-major: r[3 i + j] = r_ij) and the four fields
 * Camera.ray reads -- the pose's own view, or the scene's */
struct PtCameraPose {
  double o[3];
  double r[9];
  double llx, lly, vx, vy;
};

/* Rv(a) */
PT_HD V3 pt_pose_rotate(const PtCameraPose& cp, V3 a) {
  return v3((cp.r[0] * a.x + cp.r[1] * a.y) + cp.r[2] * a.z, (cp.r[3] * a.x + cp.r[4] * a.y) + cp.r[5] * a.z,
            (cp.r[6] * a.x + cp.r[7] * a.y) + cp.r[8] * a.z);
}

/* (cx, cy): the sample's film coordinates.  LENS: a lens of this radius and focus distance, (u, v) its lens pair (the steps up to
 * e and l are pt_lens.h's, which normalises where this rule has yet to rotate); otherwise the four are not read.
 * The rule's vectors before they are rotated: e (q without a lens, P - L with one) and, with a lens, l = L (pt_shutter.h turns them
 * once more before they are normalised). */
template <bool LENS>
PT_HD void pt_camera_pose_vectors(const PtCameraPose& cp, double cx, double cy, double radius, double focus, double u, double v, V3* e, V3* l) {
  const V3 q = v3(cp.llx + (cp.vx * cx), cp.lly + (cp.vy * cy), -1.0);
  if (!LENS) {
    *e = q;
    return;
  }
  const double pi = 3.14159265358979323846; /* Float.pi */
  const V3 p = v3(focus * q.x, focus * q.y, focus * q.z);
  const double r = pt_sqrt(u);
  const double th = (v * 2.0) * pi;
  double sn, cs;
  pt_sincos(th, &sn, &cs);
  *l = v3(radius * (r * cs), radius * (r * sn), 0.0);
  *e = v3_sub(p, *l);
}

template <bool LENS>
PT_HD void pt_camera_pose_ray(const PtCameraPose& cp, double cx, double cy, double radius, double focus, double u, double v, V3* origin,
                              V3* direction) {
  V3 e, l;
  pt_camera_pose_vectors<LENS>(cp, cx, cy, radius, focus, u, v, &e, &l);
  if (!LENS) {
    *origin = v3(cp.o[0], cp.o[1], cp.o[2]);
  } else {
    const V3 rl = pt_pose_rotate(cp, l);
    *origin = v3(cp.o[0] + rl.x, cp.o[1] + rl.y, cp.o[2] + rl.z);
  }
  *direction = v3_normalize(pt_pose_rotate(cp, e));
}

#endif /* PT_CAMERA_POSE_H */
