/* pt_projection.h -- the camera ray of the lat-long projection (include/ptx.h, "camera projection"), written once for host and
 * device beside pt_camera_pose.h.
 *
 * The header states the rule operation for operation; every expression below keeps its grouping (the build has
 * -ffp-contract=off, and nothing here is an fma).  tests/projection_reference.py restates it from the header's text, and the CPU
 * tests compile this file for the host and compare bit for bit.
 *
 * (u, v) are the environment map's texture coordinates and e is the environment-sampling rule's direction from them, so the
 * environment lookup of the ray of film point (cx, cy) lands on (cx, 1 - cy): a panorama is an environment map. */
#ifndef PT_PROJECTION_H
#define PT_PROJECTION_H

#include "pt_camera_pose.h"

/* e: the environment-sampling rule's direction of film point (cx, cy), before it is rotated */
PT_HD V3 pt_latlong_vector(double cx, double cy) {
  const double pi = 3.14159265358979323846; /* Float.pi */
  const double u = cx;
  const double v = 1.0 - cy;
  const double al = u * (2.0 * pi) - pi;
  const double th = v * pi;
  double sa, ca, st, ct;
  pt_sincos(al, &sa, &ca);
  pt_sincos(th, &st, &ct);
  return v3(st * ca, -ct, -(st * sa));
}

/* (cx, cy): the sample's film coordinates, exactly the pinhole's.  Of the pose, the origin and the rotation are read (origin 0 and the
 * identity while the pose is off); the view fields are not. */
PT_HD void pt_latlong_ray(const PtCameraPose& cp, double cx, double cy, V3* origin, V3* direction) {
  *origin = v3(cp.o[0], cp.o[1], cp.o[2]);
  *direction = v3_normalize(pt_pose_rotate(cp, pt_latlong_vector(cx, cy)));
}

#endif /* PT_PROJECTION_H */
