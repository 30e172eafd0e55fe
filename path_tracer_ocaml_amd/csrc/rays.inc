/* rays.inc -- radiance along rays the caller owns (included from kernels.hip; the rule: include/ptx.h, ptx_render_rays_device).
 * The lens and the pose reach the integrator by writing camera rays into a path queue that run_bounces bounces walk-first; that route
 * takes any ray, and the three kernels here are all that an entry point for explicit rays needs beside it: a check of the caller's
 * arrays, a generator that copies one batch of them into the queue, and a fold of the batch's contributions into the caller's bins.
 * No kernel of another path is touched. */

/* Ray i of the caller's arrays is refused if a component of its origin or direction is not finite, if its direction is (+-0, +-0, +-0),
 * or if its offset lies outside [0, 2^31 - 2] (pt_lds_get forms 1 + offset in 32 bits).  *lowest = the lowest refused index (an integer
 * minimum: the same answer whatever order the waves run in), left as it was (0xffffffff) where every ray is accepted. */
__device__ __forceinline__ bool pt_rays_finite(double a) { return (__double2hiint(a) & 0x7ff00000) != 0x7ff00000; }
__global__ __launch_bounds__(256) void k_rays_check(long long n, const double* __restrict__ o3, const double* __restrict__ d3,
                                                    const int32_t* __restrict__ offsets, uint32_t* __restrict__ lowest) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double ox = o3[3 * i], oy = o3[3 * i + 1], oz = o3[3 * i + 2];
  const double dx = d3[3 * i], dy = d3[3 * i + 1], dz = d3[3 * i + 2];
  bool bad = !(pt_rays_finite(ox) && pt_rays_finite(oy) && pt_rays_finite(oz) && pt_rays_finite(dx) && pt_rays_finite(dy) && pt_rays_finite(dz));
  bad = bad || (dx == 0.0 && dy == 0.0 && dz == 0.0);
  if (offsets) {
    const int32_t off = offsets[i];
    bad = bad || off < 0 || off > 0x7ffffffe;
  }
  if (bad) atomicMin(lowest, (uint32_t)i);
}

/* One batch: rays [first, first + n) of the caller's arrays become entries [0, n) of the queue, entry = id = the ray's index in the
 * batch (every thread owns its slot: no append, the queue's order is the caller's).  Consecutive lanes read consecutive 24-byte
 * triples of both arrays (a wave: two contiguous 1.5 KiB stretches) and write consecutive records through pt_q_store_fresh, so a lit
 * scene gets its emission record.  NORMALIZE: V3.normalize of the direction first; otherwise the direction as it was given. */
template <bool NORMALIZE>
__global__ __launch_bounds__(256) void k_generate_rays(PtSceneDev sc, long long first, uint32_t n, const double* __restrict__ o3,
                                                       const double* __restrict__ d3, const int32_t* __restrict__ offsets, PtQueue q) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *q.count = n;
  if (i >= n) return;
  const long long r = first + (long long)i;
  const V3 o = v3(o3[3 * r], o3[3 * r + 1], o3[3 * r + 2]);
  V3 d = v3(d3[3 * r], d3[3 * r + 1], d3[3 * r + 2]);
  if (NORMALIZE) d = v3_normalize(d);
  const int offset = offsets ? offsets[r] : (int)r;
  pt_q_store_fresh(sc, q, i, o, d, i, offset);
}

/* The batch's contributions folded into the caller's bins: bin b is rays [b m, (b + 1) m), one thread per bin that the batch
 * [first, first + n) touches, sum = sum + c and sq = sq + c * c in ray order onto what the buffers hold (the product is rounded
 * before the add: -ffp-contract=off).  A bin that straddles two batches is continued by the later batch's launch from where the
 * earlier one left it, so the fold is the same left fold whatever the batch size.  No atomics: a bin has one writer per launch and
 * the launches of a call run in order. */
template <bool SQ>
__global__ __launch_bounds__(256) void k_accum_rays(PtContrib contrib, long long first, long long n, long long m, double* __restrict__ sum,
                                                    double* __restrict__ sq) {
  const long long b0 = first / m, b1 = (first + n - 1) / m; /* the bins of this batch, both ends included */
  const long long b = b0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > b1) return;
  const long long r0 = b * m > first ? b * m : first;
  const long long r1 = (b + 1) * m < first + n ? (b + 1) * m : first + n;
  double r = sum[3 * b], g = sum[3 * b + 1], bl = sum[3 * b + 2];
  double sr = 0.0, sg = 0.0, sb = 0.0;
  if (SQ) {
    sr = sq[3 * b];
    sg = sq[3 * b + 1];
    sb = sq[3 * b + 2];
  }
  for (long long k = r0; k < r1; ++k) {
    const double4 c = contrib.rgbx[k - first];
    r = r + c.x;
    g = g + c.y;
    bl = bl + c.z;
    if (SQ) {
      sr = sr + c.x * c.x;
      sg = sg + c.y * c.y;
      sb = sb + c.z * c.z;
    }
  }
  sum[3 * b] = r;
  sum[3 * b + 1] = g;
  sum[3 * b + 2] = bl;
  if (SQ) {
    sq[3 * b] = sr;
    sq[3 * b + 1] = sg;
    sq[3 * b + 2] = sb;
  }
}
