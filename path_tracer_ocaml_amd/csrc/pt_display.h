/* pt_display.h -- the display rule (include/ptx.h, "display outputs"), written once for host and device.
 *
 * The header states the rule operation for operation; every expression below keeps its grouping (the build has
 * -ffp-contract=off, and nothing here is an fma).  tests/display_reference.py restates it from the header's text; the host applies
 * it in csrc/scene_host.cpp (display_apply_host), the device in csrc/display.inc (k_display_image), both through these functions. */
#ifndef PT_DISPLAY_H
#define PT_DISPLAY_H

#include "../../include/ptx.h"
#include "pt_math.h"

/* The PT_DISPLAY_MUTANT_* switches here, in display.inc and in ptx_api.inc (render_into_pinned) each build one deliberately WRONG
 * library for profiles/pr_display_mutants.txt (tools/build_variant.sh): what the tests do to a broken rule.  They exist for that record
 * alone and must never be defined in a build that ships. */
#define PT_DISPLAY_THRESHOLDS 255 /* T[1] .. T[255]; entry k - 1 of the table is T[k] */

/* Stage A: the value t of one channel from v, the binary64 value of the filmed, sqrt-encoded image */
PT_HD double pt_display_value(double v, int32_t transfer, int32_t tone, double exposure) {
  if (transfer == PTX_TRANSFER_REFERENCE) return v;
  double L = (v * v) * exposure;
  L = (L > 0x1p40) ? 0x1p40 : L; /* a NaN stays a NaN; the cap keeps inf / inf out of the curves */
  if (tone == PTX_TONE_REINHARD) return L / (1.0 + L);
  if (tone == PTX_TONE_ACES) return (L * ((2.51 * L) + 0.03)) / ((L * ((2.43 * L) + 0.59)) + 0.14);
  return L;
}

/* Stage B, 8 bits, REFERENCE or LINEAR: png_write.cpp's conversion, a truncation; NaN gives 0 */
PT_HD uint8_t pt_display_code_trunc(double t) {
  double y = t * 255.0;
  if (!(y > 0.0)) y = 0.0;
  if (y > 255.0) y = 255.0;
  return (uint8_t)(int)y;
}

/* Stage B, 8 bits, SRGB: the number of k in 1 .. 255 with T[k] <= t, as eight steps of a binary search over the increasing table
 * (th[k - 1] = T[k]); the probes are 128, then +-64 ... and never leave 1 .. 255.  NaN fails every comparison and gives 0. */
PT_HD uint8_t pt_display_code_srgb(double t, const double* th) {
  int c = 0;
#ifdef PT_DISPLAY_MUTANT_LT
  for (int step = 128; step > 0; step >>= 1) c += (th[c + step - 1] < t) ? step : 0;
#else
  for (int step = 128; step > 0; step >>= 1) c += (th[c + step - 1] <= t) ? step : 0;
#endif
  return (uint8_t)c;
}

PT_HD uint8_t pt_display_code(double v, int32_t transfer, int32_t tone, double exposure, const double* th) {
  const double t = pt_display_value(v, transfer, tone, exposure);
#ifdef PT_DISPLAY_MUTANT_ROUND
  if (transfer == PTX_TRANSFER_REFERENCE) return pt_display_code_trunc(t + (0.5 / 255.0));
#endif
  return transfer == PTX_TRANSFER_SRGB ? pt_display_code_srgb(t, th) : pt_display_code_trunc(t);
}

/* Stage B, binary32: round to nearest even, no clamp; infinities and NaN pass through */
PT_HD float pt_display_f32(double v, int32_t transfer, int32_t tone, double exposure) {
  return (float)pt_display_value(v, transfer, tone, exposure);
}

#endif /* PT_DISPLAY_H */
