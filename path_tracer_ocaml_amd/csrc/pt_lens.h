/* pt_lens.h -- the thin-lens camera ray (include/ptx.h, "thin-lens camera"), written once for host and device.
 *
 * The header states the rule operation for operation; every expression below keeps its grouping (the build has
 * -ffp-contract=off, and nothing here is an fma).  tests/c/lens_oracle.c and tests/lens_reference.py restate it from the header's
 * text, and the CPU tests compile this file for the host and compare bit for bit. */
#ifndef PT_LENS_H
#define PT_LENS_H

#include "pt_vec.h"

/* The lens of a launch: radius A > 0, focus distance F, and the sampler's dimension d = 4 + 2 max_bounces, whose last two
 * dimensions are the lens pair */
struct PtLens {
  double radius, focus;
  int32_t dim;
};

/* (cx, cy): the sample's film coordinates; (u, v): its lens pair.  Origin and direction of the camera ray. */
PT_HD void pt_lens_ray(double llx, double lly, double vx, double vy, double cx, double cy, double radius, double focus, double u,
                       double v, V3* origin, V3* direction) {
  const double pi = 3.14159265358979323846; /* Float.pi */
  const V3 q = v3(llx + (vx * cx), lly + (vy * cy), -1.0);
  const V3 p = v3(focus * q.x, focus * q.y, focus * q.z);
  const double r = pt_sqrt(u);
  const double th = (v * 2.0) * pi;
  double sn, cs;
  pt_sincos(th, &sn, &cs); /* (pt_sin and pt_cos are its two results) */
  const V3 l = v3(radius * (r * cs), radius * (r * sn), 0.0);
  *origin = l;
  *direction = v3_normalize(v3_sub(p, l));
}

#endif /* PT_LENS_H */
