/* camera_pose.inc -- the posed camera's kernels (included from kernels.hip; the rule: include/ptx.h and pt_camera_pose.h).
 * A posed camera's rays start wherever the pose puts them, which the fused camera launches cannot take, so a posed render WRITES its
 * camera rays into a path queue and bounces them from there like any queued rays, as a lens render does (lens.inc): the three
 * generators below are lens.inc's with the pose applied, LENS or not.  Each thread owns one entry and streams it out through
 * pt_q_store* in 16-byte stores; consecutive lanes write consecutive records, so a wave's stores of one instruction fall into one
 * contiguous 3 KiB (rays) and 2 or 4 KiB (path state) stretch that the following instructions complete.  The first-hit features read
 * their rays back from the queue: k_features_lens serves a posed render unchanged.  No kernel of another path is touched. */
#include "pt_camera_pose.h"

/* The camera ray of sample (x, gy) with sampler offset `offset`: the film coordinates exactly as pt_primary_dir, k_generate_list and
 * pt_lens_sample_ray compute them; with a lens, its pair from the sampler's last two dimensions at the same offset.  The pose adds no
 * dimension: alpha is the table the same render without a pose reads. */
template <bool LENS>
__device__ __forceinline__ void pt_pose_sample_ray(const PtCameraPose& cp, const PtLens& ln, const double* __restrict__ alpha, int x, int gy,
                                                   int width, int height, int offset, V3* o, V3* d) {
  const double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  const double dxs = pt_lds_get(alpha, offset, 0), dys = pt_lds_get(alpha, offset, 1);
  const double cx = ((double)x + dxs) * widthf;
  const double cy = 1.0 - (((double)gy + dys) * heightf);
  double u = 0.0, v = 0.0;
  if (LENS) {
    u = pt_lds_get(alpha, offset, ln.dim - 2);
    v = pt_lds_get(alpha, offset, ln.dim - 1);
  }
  pt_camera_pose_ray<LENS>(cp, cx, cy, ln.radius, ln.focus, u, v, o, d);
}

/* k_generate_lens under a pose: the same entries in the same order -- 64 consecutive entries are one 8 x 8 tile of one pass, the
 * lanes of a ragged tile that fall off the image are holes (PT_HOLE_HI) -- with the same ids, offsets and count.  PATH = false writes
 * the rays alone (the feature buffers). */
template <bool LENS, bool PATH>
__global__ __launch_bounds__(256) void k_generate_pose(PtSceneDev sc, PtGenParams g, PtCameraPose cp, PtLens ln, const double* __restrict__ alpha,
                                                       PtQueue q) {
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
  pt_pose_sample_ray<LENS>(cp, ln, alpha, ps.x, ps.gy, g.width, g.height, ps.offset, &o, &d);
  if (PATH) pt_lens_store(sc, q, i, o, d, ps.id, ps.offset);
  else pt_q_store_ray(q, i, o, d);
}

/* k_generate_pixels under a pose: the same entries, ids and count (list mode: adaptive rounds, ptx_render_pixels_device) */
template <bool LENS>
__global__ __launch_bounds__(256) void k_generate_pixels_pose(PtSceneDev sc, int width, int height, int spp, int first_pass, int n_pass,
                                                              const int32_t* __restrict__ pix, long long n_list, PtCameraPose cp, PtLens ln,
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
  pt_pose_sample_ray<LENS>(cp, ln, alpha, x, gy, width, height, offset, &o, &d);
  pt_lens_store(sc, q, (uint32_t)i, o, d, (uint32_t)i, offset);
}

/* k_generate_list under a pose: explicit (x, y, pass) triples (ptx_trace_samples, ptx_camera_rays) */
template <bool LENS>
__global__ __launch_bounds__(256) void k_generate_list_pose(PtSceneDev sc, int width, int height, int spp, long long n,
                                                            const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                            const int32_t* __restrict__ passes, PtCameraPose cp, PtLens ln,
                                                            const double* __restrict__ alpha, PtQueue q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  const uint32_t dst = pt_wave_append(q.count, valid);
  if (!valid) return;
  const int x = xs[i], gy = ys[i], pass = passes[i];
  const int offset = (gy * width) + x + (pass * spp);
  V3 o, d;
  pt_pose_sample_ray<LENS>(cp, ln, alpha, x, gy, width, height, offset, &o, &d);
  pt_lens_store(sc, q, dst, o, d, (uint32_t)i, offset);
}
