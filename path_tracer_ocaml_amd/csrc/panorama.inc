/* panorama.inc -- the lat-long camera's kernels (included from kernels.hip; the rule: include/ptx.h and pt_projection.h).
 * A panorama's rays leave the pose's origin in every direction, which no fused camera launch can take, so a lat-long render takes the
 * posed route: it WRITES its camera rays into a path queue and bounces them from there, walk-first.  The three generators below are
 * camera_pose.inc's with pt_latlong_ray in the place of the frustum: the same entries in the same order, the same ids, offsets, holes
 * and count, so every driver the pose serves (and k_features_lens, which reads its rays back from the queue) serves a panorama
 * unchanged.  The projection reads no sampler dimension of its own.  No kernel of another path is touched. */
#include "pt_projection.h"

/* The camera ray of sample (x, gy) with sampler offset `offset`: the film coordinates exactly as pt_pose_sample_ray computes them */
__device__ __forceinline__ void pt_pano_sample_ray(const PtCameraPose& cp, const double* __restrict__ alpha, int x, int gy, int width, int height,
                                                   int offset, V3* o, V3* d) {
  const double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  const double dxs = pt_lds_get(alpha, offset, 0), dys = pt_lds_get(alpha, offset, 1);
  const double cx = ((double)x + dxs) * widthf;
  const double cy = 1.0 - (((double)gy + dys) * heightf);
  pt_latlong_ray(cp, cx, cy, o, d);
}

/* k_generate_pose for a panorama.  PATH = false writes the rays alone (the feature buffers). */
template <bool PATH>
__global__ __launch_bounds__(256) void k_generate_pano(PtSceneDev sc, PtGenParams g, PtCameraPose cp, const double* __restrict__ alpha, PtQueue q) {
  const uint32_t n = (uint32_t)g.n_pass * (uint32_t)(g.tiles_x * g.tiles_y) * 64u;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *q.count = n;
  if (i >= n) return;
  const PtPrimarySample ps = pt_primary_decode(g, i);
  if (!ps.valid) {
    q.ray[i].dx = __hiloint2double((int)PT_HOLE_HI, 0);
    return;
  }
  V3 o, d;
  pt_pano_sample_ray(cp, alpha, ps.x, ps.gy, g.width, g.height, ps.offset, &o, &d);
  if (PATH) pt_lens_store(sc, q, i, o, d, ps.id, ps.offset);
  else pt_q_store_ray(q, i, o, d);
}

/* k_generate_pixels_pose for a panorama (list mode: adaptive rounds, ptx_render_pixels_device) */
__global__ __launch_bounds__(256) void k_generate_pixels_pano(PtSceneDev sc, int width, int height, int spp, int first_pass, int n_pass,
                                                              const int32_t* __restrict__ pix, long long n_list, PtCameraPose cp,
                                                              const double* __restrict__ alpha, PtQueue q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)n_pass * n_list;
  if (i == 0) *q.count = (uint32_t)n;
  if (i >= n) return;
  const long long pass_in_batch = i / n_list, j = i - pass_in_batch * n_list;
  const int p = pix[j];
  const int gy = p / width, x = p - gy * width;
  const int offset = (gy * width) + x + ((first_pass + (int)pass_in_batch) * spp);
  V3 o, d;
  pt_pano_sample_ray(cp, alpha, x, gy, width, height, offset, &o, &d);
  pt_lens_store(sc, q, (uint32_t)i, o, d, (uint32_t)i, offset);
}

/* k_generate_list_pose for a panorama: explicit (x, y, pass) triples (ptx_trace_samples, ptx_camera_rays) */
__global__ __launch_bounds__(256) void k_generate_list_pano(PtSceneDev sc, int width, int height, int spp, long long n,
                                                            const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                            const int32_t* __restrict__ passes, PtCameraPose cp,
                                                            const double* __restrict__ alpha, PtQueue q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  const uint32_t dst = pt_wave_append(q.count, valid);
  if (!valid) return;
  const int x = xs[i], gy = ys[i], pass = passes[i];
  const int offset = (gy * width) + x + (pass * spp);
  V3 o, d;
  pt_pano_sample_ray(cp, alpha, x, gy, width, height, offset, &o, &d);
  pt_lens_store(sc, q, dst, o, d, (uint32_t)i, offset);
}
