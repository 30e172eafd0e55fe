/* display.inc -- the display kernel (include/ptx.h, "display outputs"): a filmed binary64 image to 8-bit or binary32 pixels.
 * Included from kernels.hip in front of ptx_api.inc.  The rule itself is pt_display.h's, shared with the host.
 *
 * Not fused into the film kernels: the f64 image stays where k_film leaves it, and this pass reads it once more (DESIGN.md
 * section 8).  The kernel is not one of the four hot families and has no entry in ptx_kernel_table. */
#include "pt_display.h"

/* the 255 sRGB thresholds, T[k] at [k - 1]: computed on the host with libm (scene_host.cpp, display_thresholds) and copied to each
 * device the first time it displays (display_thresholds_device) */
__device__ double g_display_thresholds[PT_DISPLAY_THRESHOLDS];

struct PtDisplay {
  int32_t transfer, tone;
  double exposure;
};

template <int FORMAT>
struct PtDisplayFormat {
  static constexpr bool is8 = FORMAT == PTX_PIXEL_RGB8 || FORMAT == PTX_PIXEL_RGBA8;
  static constexpr int channels = (FORMAT == PTX_PIXEL_RGBA8 || FORMAT == PTX_PIXEL_RGBA32F) ? 4 : 3;
};

/* one pixel, element by element: the head and the tail of a range, whose quads belong in part to a neighbouring range */
template <int FORMAT>
__device__ __forceinline__ void pt_display_pixel(const double* __restrict__ rgb, long long p, const PtDisplay& d, const double* th,
                                                 void* __restrict__ out) {
  constexpr int C = PtDisplayFormat<FORMAT>::channels;
  if constexpr (PtDisplayFormat<FORMAT>::is8) {
    uint8_t* o = (uint8_t*)out + p * C;
    for (int c = 0; c < 3; ++c) o[c] = pt_display_code(rgb[3 * p + c], d.transfer, d.tone, d.exposure, th);
    if constexpr (C == 4) o[3] = 255;
  } else {
    float* o = (float*)out + p * C;
    for (int c = 0; c < 3; ++c) o[c] = pt_display_f32(rgb[3 * p + c], d.transfer, d.tone, d.exposure);
    if constexpr (C == 4) o[3] = 1.0f;
  }
}

__device__ __forceinline__ uint32_t pt_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t e) { return a | (b << 8) | (c << 16) | (e << 24); }

/* Pixels [p0, p1) of the flattened image at rgb (3 doubles a pixel) to the same pixels of the display image at out.  A thread owns the
 * quad of four consecutive pixels [4 q, 4 q + 4), q counted from the image's first pixel, so that its 96 bytes of input and its
 * 12 / 16 / 48 / 64 bytes of output are 16-byte (RGB8: 4-byte) aligned whatever p0 is: six 16-byte loads, then three dwords, one
 * 16-byte store, three or four 16-byte stores.  A quad that [p0, p1) covers in part -- the range of a row slab starts at row0 * width,
 * for odd widths no multiple of four -- is written element by element, and only its pixels inside the range: two ranges that share a
 * quad write disjoint bytes of it.  Grid: one thread per quad that meets the range, 256 a workgroup. */
template <int FORMAT>
__global__ __launch_bounds__(256) void k_display_image(const double* __restrict__ rgb, long long p0, long long p1, PtDisplay d,
                                                       void* __restrict__ out) {
  constexpr bool is8 = PtDisplayFormat<FORMAT>::is8;
  __shared__ double th[is8 ? PT_DISPLAY_THRESHOLDS : 1];
  if constexpr (is8) {
    if (d.transfer == PTX_TRANSFER_SRGB) { /* uniform over the launch */
      if (threadIdx.x < PT_DISPLAY_THRESHOLDS) th[threadIdx.x] = g_display_thresholds[threadIdx.x];
      __syncthreads();
    }
  }
  const long long q = p0 / 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long a = q * 4, b = a + 4;
  if (a >= p1) return;
#ifdef PT_DISPLAY_MUTANT_HEAD
  if (b > p1) {
#else
  if (a < p0 || b > p1) {
#endif
    for (long long p = (a < p0 ? p0 : a); p < (b > p1 ? p1 : b); ++p) pt_display_pixel<FORMAT>(rgb, p, d, th, out);
    return;
  }
  const double2* src = (const double2*)(rgb + a * 3);
  double v[12];
  for (int i = 0; i < 6; ++i) {
    const double2 t = src[i];
    v[2 * i] = t.x;
    v[2 * i + 1] = t.y;
  }
  if constexpr (is8) {
    uint32_t c[12];
    for (int i = 0; i < 12; ++i) c[i] = pt_display_code(v[i], d.transfer, d.tone, d.exposure, th);
    if constexpr (FORMAT == PTX_PIXEL_RGB8) {
      uint32_t* o = (uint32_t*)out + q * 3;
      o[0] = pt_pack4(c[0], c[1], c[2], c[3]);
      o[1] = pt_pack4(c[4], c[5], c[6], c[7]);
      o[2] = pt_pack4(c[8], c[9], c[10], c[11]);
    } else {
      uint4 w;
      w.x = pt_pack4(c[0], c[1], c[2], 255u);
      w.y = pt_pack4(c[3], c[4], c[5], 255u);
      w.z = pt_pack4(c[6], c[7], c[8], 255u);
      w.w = pt_pack4(c[9], c[10], c[11], 255u);
      ((uint4*)out)[q] = w;
    }
  } else {
    float f[12];
    for (int i = 0; i < 12; ++i) f[i] = pt_display_f32(v[i], d.transfer, d.tone, d.exposure);
    if constexpr (FORMAT == PTX_PIXEL_RGB32F) {
      float4* o = (float4*)out + q * 3;
      o[0] = make_float4(f[0], f[1], f[2], f[3]);
      o[1] = make_float4(f[4], f[5], f[6], f[7]);
      o[2] = make_float4(f[8], f[9], f[10], f[11]);
    } else {
      float4* o = (float4*)out + q * 4;
      for (int i = 0; i < 4; ++i) o[i] = make_float4(f[3 * i], f[3 * i + 1], f[3 * i + 2], 1.0f);
    }
  }
}
