/* camera_rays.inc -- camera rays written into a path queue (included from kernels.hip; the rules: include/ptx.h and pt_lens.h,
 * pt_camera_pose.h, pt_projection.h, pt_shutter.h).
 * The fused camera launches take a pinhole at the origin for granted.  Every other camera, and every render of a list of pixels or
 * samples, WRITES its camera rays into a queue and bounces them from there like any queued rays.  A camera is one arm of
 * pt_camera_sample_ray and an enumeration of samples is one kernel templated on the camera, so nothing here is written per camera.
 * Each thread owns one entry and streams it out through pt_q_store* in 16-byte stores; consecutive lanes write consecutive records.
 * No kernel of the fused path is touched. */
#include "pt_lens.h"
#include "pt_camera_pose.h"
#include "pt_projection.h"
#include "pt_shutter.h"

/* The camera of a launch.  A new kind is four edits and nothing else: a value here, an arm in pt_camera_sample_ray, an arm in the
 * host's camera_kind and a line in the host's with_camera_kind (ptx_api.inc). */
enum PtCameraKind {
  PT_CAM_PINHOLE,   /* the scene's own camera: Camera.ray from the origin */
  PT_CAM_LENS,      /* ... through a thin lens (pt_lens.h) */
  PT_CAM_POSE,      /* a posed camera (pt_camera_pose.h) */
  PT_CAM_POSE_LENS, /* ... through a thin lens */
  PT_CAM_LATLONG,   /* the lat-long panorama from the pose's origin (pt_projection.h) */
  PT_CAM_POSE_SHUTTER,      /* the posed camera, moving while its shutter is open (pt_shutter.h) */
  PT_CAM_POSE_LENS_SHUTTER, /* ... through a thin lens */
  PT_CAM_LATLONG_SHUTTER,   /* the panorama from a moving pose */
};
/* what the kinds read besides the scene: a kind reads the fields of its rule and no other (a pinhole's alpha table has no lens pair) */
struct PtCameraArg {
  PtCameraPose pose;
  PtLens lens;
  PtShutter shutter;
};

/* render_tile's film coordinates of sample (x, gy) with sampler offset `offset` (integrator.ml:98-105) */
__device__ __forceinline__ void pt_film_coords(const double* __restrict__ alpha, int x, int gy, int width, int height, int offset, double* cx,
                                               double* cy) {
  const double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  const double dxs = pt_lds_get(alpha, offset, 0), dys = pt_lds_get(alpha, offset, 1);
  *cx = ((double)x + dxs) * widthf;
  *cy = 1.0 - (((double)gy + dys) * heightf);
}

/* The camera ray of sample (x, gy) with sampler offset `offset`.  A lens pair comes from the sampler's last two dimensions at the same
 * offset, or the two before the last where a shutter's time is the last; pose and projection add no dimension.  Each kind calls its own rule with its own operands: the kinds agree with one another
 * only up to the sign of a zero (pt_camera_pose.h), and the tests compare bits. */
template <int CAM>
__device__ __forceinline__ void pt_camera_sample_ray(const PtSceneDev& sc, const PtCameraArg& cam, const double* __restrict__ alpha, int x,
                                                     int gy, int width, int height, int offset, V3* o, V3* d) {
  constexpr bool LENS = CAM == PT_CAM_LENS || CAM == PT_CAM_POSE_LENS || CAM == PT_CAM_POSE_LENS_SHUTTER;
  constexpr bool SHUTTER = CAM == PT_CAM_POSE_SHUTTER || CAM == PT_CAM_POSE_LENS_SHUTTER || CAM == PT_CAM_LATLONG_SHUTTER;
  const PtLens& ln = cam.lens;
  double cx, cy, u = 0.0, v = 0.0;
  pt_film_coords(alpha, x, gy, width, height, offset, &cx, &cy);
  if (LENS) {
    u = pt_lds_get(alpha, offset, ln.dim - 2);
    v = pt_lds_get(alpha, offset, ln.dim - 1);
  }
  const double t = SHUTTER ? pt_lds_get(alpha, offset, cam.shutter.dim - 1) : 0.0;
  switch (CAM) {
    case PT_CAM_PINHOLE:
      *o = v3(0.0, 0.0, 0.0);
      *d = pt_camera_dir(sc, cx, cy);
      break;
    case PT_CAM_LENS:
      pt_lens_ray(sc.cam_llx, sc.cam_lly, sc.cam_vx, sc.cam_vy, cx, cy, ln.radius, ln.focus, u, v, o, d);
      break;
    case PT_CAM_POSE:
    case PT_CAM_POSE_LENS:
      pt_camera_pose_ray<LENS>(cam.pose, cx, cy, ln.radius, ln.focus, u, v, o, d);
      break;
    case PT_CAM_LATLONG:
      pt_latlong_ray(cam.pose, cx, cy, o, d);
      break;
    case PT_CAM_POSE_SHUTTER:
    case PT_CAM_POSE_LENS_SHUTTER:
      pt_shutter_pose_ray<LENS>(cam.pose, cam.shutter, cx, cy, ln.radius, ln.focus, u, v, t, o, d);
      break;
    case PT_CAM_LATLONG_SHUTTER:
      pt_shutter_latlong_ray(cam.pose, cam.shutter, cx, cy, t, o, d);
      break;
  }
}

/* a fresh path: attenuation 1, no emission carried; has_emit chooses the record */
__device__ __forceinline__ void pt_q_store_fresh(const PtSceneDev& sc, const PtQueue& q, uint32_t dst, V3 o, V3 d, uint32_t id, int offset) {
  if (sc.has_emit) pt_q_store<true>(q, dst, o, d, v3(1.0, 1.0, 1.0), v3(0.0, 0.0, 0.0), id, offset);
  else pt_q_store<false>(q, dst, o, d, v3(1.0, 1.0, 1.0), v3(0.0, 0.0, 0.0), id, offset);
}

/* The camera rays of a whole batch (g.n_pass passes of this rank's rows) in the order the fused camera launch enumerates its virtual
 * queue (pt_primary_decode): entry i = (pass_in_batch, 8x8 tile, lane), so 64 consecutive entries are one tile of one pass and a wave
 * of the bounce launch that follows walks a coherent bundle.  Every entry owns its slot (no append); the lanes of a ragged tile that
 * fall off the image are HOLES (PT_HOLE_HI, as k_shade_pool marks the unused entries of its blocks: every reader of a queue skips
 * them), so *q.count = n_pass * tiles * 64 entries, which is what the workspace of a full-frame batch is sized for.  The contribution
 * id is pt_primary_decode's: pass_in_batch * W * local_rows + y * W + x, what k_accum / k_accum_sq sum by.
 * PATH = false writes the rays alone (q.path is not touched): the feature buffers trace them and keep no path state.
 * (Never instantiated for the pinhole: its whole batch is the fused camera launch.) */
template <int CAM, bool PATH>
__global__ __launch_bounds__(256) void k_generate_tiles(PtSceneDev sc, PtGenParams g, PtCameraArg cam, const double* __restrict__ alpha, PtQueue q) {
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
  pt_camera_sample_ray<CAM>(sc, cam, alpha, ps.x, ps.gy, g.width, g.height, ps.offset, &o, &d);
  if (PATH) pt_q_store_fresh(sc, q, i, o, d, ps.id, ps.offset);
  else pt_q_store_ray(q, i, o, d);
}

/* Camera rays of passes [first_pass, first_pass + n_pass) for the listed pixels (pix[j] = y * width + x, whole image), pass-major
 * then list order: entry i = pass_in_batch * n_list + j, and its contribution id is i.  Every entry owns its slot (no append), so the
 * queue is dense and keeps the list's order; *q.count is set to the entry count (list mode: adaptive rounds, ptx_render_pixels_device). */
template <int CAM>
__global__ __launch_bounds__(256) void k_generate_pixels(PtSceneDev sc, int width, int height, int spp, int first_pass, int n_pass,
                                                         const int32_t* __restrict__ pix, long long n_list, PtCameraArg cam,
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
  pt_camera_sample_ray<CAM>(sc, cam, alpha, x, gy, width, height, offset, &o, &d);
  pt_q_store_fresh(sc, q, (uint32_t)i, o, d, (uint32_t)i, offset);
}

/* explicit (x, y, pass) triples, appended; the contribution id is the triple's index (ptx_trace_samples, ptx_camera_rays) */
template <int CAM>
__global__ __launch_bounds__(256) void k_generate_list(PtSceneDev sc, int width, int height, int spp, long long n,
                                                       const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                       const int32_t* __restrict__ passes, PtCameraArg cam,
                                                       const double* __restrict__ alpha, PtQueue q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  const uint32_t dst = pt_wave_append(q.count, valid);
  if (!valid) return;
  const int x = xs[i], gy = ys[i], pass = passes[i];
  const int offset = (gy * width) + x + (pass * spp);
  V3 o, d;
  pt_camera_sample_ray<CAM>(sc, cam, alpha, x, gy, width, height, offset, &o, &d);
  pt_q_store_fresh(sc, q, dst, o, d, (uint32_t)i, offset);
}
