/* pt_tile_scan.h -- the camera rays' scan of their tile's sphere list (scene_host.h: PtTileRec), written once for the kernel
 * (k_bounce_carry's TILE instantiations) and for the host (tests/c/tile_lists_driver.cpp runs the shipped arithmetic on the CPU).
 *
 * It is PtTraverser::packet's Simd_leaf branch for a ray from the origin, with `leaf_first + base + k` replaced by the list's k-th
 * slot: pass 1 over the entries in lockstep (the discriminant's sign, a candidate bit), pass 2 the roots of the candidates in list
 * order -- the same expressions in the same order and the same `!(t < t_min) && t <= r.t`.  The list holds every sphere a ray of the
 * tile can meet, in the relative order the walk tests them, so the closest hit and its ties come out as the walk's, EXCEPT where
 * rounding lets the walk skip a sphere the list holds (a box test that fails by an ulp).  That can happen only next to a grazing hit
 * or next to a tie with the closest hit so far; pass 2 raises *guard there and the caller walks the tree instead (DESIGN.md
 * section 4 derives both thresholds):
 *   PT_TILE_GUARD_DISC   a candidate's discriminant below 2^-20 r^2
 *   PT_TILE_GUARD_TIE    a root within 2^-30 relative of the closest hit so far
 *
 * `slot_of(k)` names the list's k-th slot and `any(b)` says whether b holds for any ray that runs the scan together with this one
 * (the kernel: a readlane and a ballot; the host: the array and b itself), so that pass 2 visits the entries wave-uniformly. */
#ifndef PT_TILE_SCAN_H
#define PT_TILE_SCAN_H

#include "pt_vec.h"

#define PT_TILE_GUARD_DISC 0x1p-20
#define PT_TILE_GUARD_TIE 0x1p-30

struct PtTileHit {
  double t;
  int slot; /* -1: a miss */
  bool guard;
};

/* live = this ray takes part; n <= 15 entries.  GUARDS = false is the tests' mutant */
template <bool GUARDS, class SlotOf, class Any>
PT_HD PtTileHit pt_tile_scan(const double* sph, SlotOf slot_of, Any any, int n, bool live, V3 d, double t_max) {
  const double t_min = 0.0;
  /* packet constants of spheres_intersect_aux (lib.rs:115-117): a is the UNFUSED scalar dot (PtTraverser::begin) */
  const double qa = d.x * d.x + d.y * d.y + d.z * d.z;
  const double one_over_a = 1.0 / qa;
  PtTileHit r;
  r.t = t_max;
  r.slot = -1;
  r.guard = false;
  uint32_t cand = 0u, some = 0u;
  for (int k = 0; k < n; ++k) {
    const double* s = sph + (size_t)slot_of(k) * 4;
    const double fx = s[0], fy = s[1], fz = s[2]; /* the origin is (+0, +0, +0): x - (+0.0) == x bit for bit */
    const double bp_over_a = pt_fma(fx, d.x, pt_fma(fy, d.y, fz * d.z)) * one_over_a;
    const double wx = pt_fma(d.x, bp_over_a, -fx);
    const double wy = pt_fma(d.y, bp_over_a, -fy);
    const double wz = pt_fma(d.z, bp_over_a, -fz);
    const double disc = (s[3] * s[3]) - pt_fma(wx, wx, pt_fma(wy, wy, wz * wz));
    const bool ok = live && pt_bits(disc) <= 0x7ff0000000000000ull; /* "neither NaN nor sign bit set" (lib.rs:162-166) */
    cand |= (ok ? 1u : 0u) << k;
    some |= (any(ok) ? 1u : 0u) << k;
  }
  for (int k = 0; k < n; ++k) {
    if (!((some >> k) & 1u)) continue;
    if ((cand >> k) & 1u) {
      const int slot = (int)slot_of(k);
      const double* s = sph + (size_t)slot * 4;
      const double fx = s[0], fy = s[1], fz = s[2];
      const double r2 = s[3] * s[3];
      const double c = pt_fma(fx, fx, pt_fma(fy, fy, fz * fz)) - r2;
      const double bp = pt_fma(fx, d.x, pt_fma(fy, d.y, fz * d.z));
      const double bp_over_a = bp * one_over_a;
      const double wx = pt_fma(d.x, bp_over_a, -fx);
      const double wy = pt_fma(d.y, bp_over_a, -fy);
      const double wz = pt_fma(d.z, bp_over_a, -fz);
      const double disc = r2 - pt_fma(wx, wx, pt_fma(wy, wy, wz * wz));
      const double q_rhs = pt_sqrt(qa * disc);
      const double qq = pt_signbit(bp) ? (bp - q_rhs) : (bp + q_rhs);
      const double t = pt_signbit(c) ? (qq * one_over_a) : (c / qq);
      if (GUARDS) {
        if (disc < PT_TILE_GUARD_DISC * r2) r.guard = true;
        if (r.slot >= 0 && pt_fabs(t - r.t) <= PT_TILE_GUARD_TIE * r.t) r.guard = true;
      }
      if (!(t < t_min) && t <= r.t) {
        r.t = t;
        r.slot = slot;
      }
    }
  }
  return r;
}

#endif /* PT_TILE_SCAN_H */
