/* temporal.inc -- temporal accumulation: the frame history reprojected across camera poses (included from kernels.hip).
 * An image-space kernel beside the integrator, like denoise.inc's: no render path calls it.  The rule is stated operation for
 * operation in include/ptx.h (ptx_temporal_accumulate_device); tests/temporal_reference.py restates it in numpy and the GPU tests
 * compare bit for bit, so every expression below keeps the header's grouping (the build has -ffp-contract=off). */

struct PtTemporal {
  int32_t width, height;
  int32_t has_prev; /* 0: a NULL previous history, every pixel takes "no history" */
  int32_t pad;
  double kd, kfd;
  double cap, normal_threshold, depth_tolerance, min_weight;
  PtCameraPose cur, prev;
};

constexpr int PT_TEMPORAL_TX = 32, PT_TEMPORAL_TY = 8; /* a workgroup's pixels, as k_film_wide's: a wave is two rows of 32 */

/* One thread owns pixel (x, y): it reads its own sums and feature record, up to four records of the previous history, and writes
 * its own record, sums, error and motion -- no atomics on doubles, the same bits on every run.  Under a small camera motion the
 * 32 x 8 tile's taps fall into a tile-sized patch of the previous history, so neighbouring lanes gather neighbouring 96-byte
 * records (six 16-byte loads each) and the taps a pixel shares with its neighbours come from L1 / L2.  The history count is one
 * popcount of the wave's ballot and one integer add per wave. */
__global__ __launch_bounds__(PT_TEMPORAL_TX * PT_TEMPORAL_TY) void k_temporal_accumulate(
    PtTemporal tp, const double* __restrict__ raw, const double* __restrict__ sq, const double* __restrict__ feat,
    const double* __restrict__ hist_prev, double* __restrict__ hist_out, double* __restrict__ raw_out, double* __restrict__ err_out,
    double* __restrict__ motion_out, unsigned long long* __restrict__ count) {
  const int x = (int)blockIdx.x * PT_TEMPORAL_TX + (int)(threadIdx.x % PT_TEMPORAL_TX);
  const int y = (int)blockIdx.y * PT_TEMPORAL_TY + (int)(threadIdx.x / PT_TEMPORAL_TX);
  const int W = tp.width, H = tp.height;
  bool history = false;
  if (x < W && y < H) {
    const long long p = (long long)y * W + x;
    const double kd = tp.kd, kfd = tp.kfd;
    const double mu[3] = {raw[3 * p] / kd, raw[3 * p + 1] / kd, raw[3 * p + 2] / kd};
    const double nu[3] = {sq[3 * p] / kd, sq[3 * p + 1] / kd, sq[3 * p + 2] / kd};
    const double2* f = (const double2*)(feat + p * 8);
    const double2 f1 = f[1], f2 = f[2], f3 = f[3]; /* (the albedo is not read) */
    const double h = f3.y;
    const double hf = h / kfd;
    const V3 n = v3(f1.y / kfd, f2.x / kfd, f2.y / kfd);
    const double z = h > 0.0 ? f3.x / h : 0.0;
    double fx = 0.0, fy = 0.0, sw = 0.0;
    double a1[3] = {0.0, 0.0, 0.0}, a2[3] = {0.0, 0.0, 0.0}, aN = 0.0;
    if (tp.has_prev) {
      const double cx = ((double)x + 0.5) * (1.0 / (double)W);
      const double cy = 1.0 - ((double)y + 0.5) * (1.0 / (double)H);
      V3 o, d;
      pt_camera_pose_ray<false>(tp.cur, cx, cy, 0.0, 0.0, 0.0, 0.0, &o, &d);
      V3 v = d;
      if (h > 0.0) {
        const V3 P = v3(o.x + z * d.x, o.y + z * d.y, o.z + z * d.z);
        v = v3(P.x - tp.prev.o[0], P.y - tp.prev.o[1], P.z - tp.prev.o[2]);
      }
      const double* r = tp.prev.r;
      const V3 c = v3((r[0] * v.x + r[3] * v.y) + r[6] * v.z, (r[1] * v.x + r[4] * v.y) + r[7] * v.z,
                      (r[2] * v.x + r[5] * v.y) + r[8] * v.z);
      if (c.z < 0.0) {
        const double iz = -c.z;
        const double qx = c.x / iz, qy = c.y / iz;
        fx = ((qx - tp.prev.llx) / tp.prev.vx) * (double)W - 0.5;
        fy = (1.0 - (qy - tp.prev.lly) / tp.prev.vy) * (double)H - 0.5;
        if (fx > -1.0 && fx < (double)W && fy > -1.0 && fy < (double)H) {
          const double xf = __builtin_floor(fx), yf = __builtin_floor(fy);
          const int x0 = (int)xf, y0 = (int)yf; /* in [-1, W - 1] x [-1, H - 1] */
          const double tx = fx - xf, ty = fy - yf;
          const double dist = pt_sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
          for (int j = 0; j < 2; ++j) {
            const int qyi = y0 + j;
            if (qyi < 0 || qyi >= H) continue;
            for (int i = 0; i < 2; ++i) {
              const int qxi = x0 + i;
              if (qxi < 0 || qxi >= W) continue;
              const double2* rec = (const double2*)(hist_prev + ((long long)qyi * W + qxi) * 12);
              const double2 r3 = rec[3]; /* {N, hf} */
              if (!(r3.x > 0.0)) continue;
              if (h > 0.0) {
                if (!(r3.y > 0.0)) continue;
                const double2 r4 = rec[4], r5 = rec[5]; /* {n.x, n.y}, {n.z, zc} */
                if (!((n.x * r4.x + n.y * r4.y) + n.z * r5.x >= tp.normal_threshold)) continue;
                if (!(pt_fabs(dist - r5.y) <= tp.depth_tolerance * dist)) continue;
              } else if (!(r3.y == 0.0)) {
                continue;
              }
              const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2]; /* {M1.r, M1.g}, {M1.b, M2.r}, {M2.g, M2.b} */
              const double w = (i ? tx : 1.0 - tx) * (j ? ty : 1.0 - ty);
              sw = sw + w;
              a1[0] = a1[0] + w * r0.x;
              a1[1] = a1[1] + w * r0.y;
              a1[2] = a1[2] + w * r1.x;
              a2[0] = a2[0] + w * r1.y;
              a2[1] = a2[1] + w * r2.x;
              a2[2] = a2[2] + w * r2.y;
              aN = aN + w * r3.x;
            }
          }
          history = sw > tp.min_weight;
        }
      }
    }
    double M1[3], M2[3], N = kd;
    if (history) {
      double NH = aN / sw;
      if (NH > tp.cap) NH = tp.cap;
      const double al = kd / (NH + kd);
      for (int c = 0; c < 3; ++c) {
        const double H1 = a1[c] / sw, H2 = a2[c] / sw;
        M1[c] = H1 * (1.0 - al) + mu[c] * al;
        M2[c] = H2 * (1.0 - al) + nu[c] * al;
      }
      N = NH + kd;
    } else {
      for (int c = 0; c < 3; ++c) {
        M1[c] = mu[c];
        M2[c] = nu[c];
      }
    }
    double2* out = (double2*)(hist_out + p * 12);
    out[0] = make_double2(M1[0], M1[1]);
    out[1] = make_double2(M1[2], M2[0]);
    out[2] = make_double2(M2[1], M2[2]);
    out[3] = make_double2(N, hf);
    out[4] = make_double2(n.x, n.y);
    out[5] = make_double2(n.z, z);
    for (int c = 0; c < 3; ++c) {
      raw_out[3 * p + c] = M1[c] * kd;
      double var = M2[c] - M1[c] * M1[c];
      if (!(var > 0.0)) var = 0.0;
      err_out[3 * p + c] = pt_sqrt(var / (N - 1.0));
    }
    if (motion_out) {
      motion_out[3 * p] = history ? fx - (double)x : 0.0;
      motion_out[3 * p + 1] = history ? fy - (double)y : 0.0;
      motion_out[3 * p + 2] = history ? sw : 0.0;
    }
  }
  /* every lane of the wave arrives here (the lanes outside the image with history = false) */
  const unsigned long long took = __ballot(history);
  if ((threadIdx.x & (PT_WAVE - 1)) == 0 && took != 0ull) atomicAdd(count, (unsigned long long)__popcll(took));
}
