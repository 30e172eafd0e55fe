/* bvh_build_gpu.inc -- binned-SAH BVH build on the GPU, level by level, producing EXACTLY the tree of
 * Shape_tree.Make(Leaf).create (path_tracer/src/shape_tree.ml:72-196,252-263): same splits, same leaf
 * decisions, same element order inside every leaf.  (SURVEY.md section 8 F3.)  Included by kernels.hip.
 *
 * Every pending node ("segment" = a slice order[lo, hi) plus its bbox) of the current level goes through
 *   1. Bshape.centroid_bbox: min/max of the centroids;
 *   2. Proposal.propose_split_one_axis for X, Y, Z: bins kept as order-preserving u64 images of the f64 bounds
 *      (integer atomic min/max -- exact and order-independent, with ONE exception: the images order -0.0 below
 *      +0.0, while the reference's Float.min / Float.max keep the second of two equal arguments, so among zeros of
 *      both signs ITS result depends on the slice order and no order-independent reduction can follow it.  The
 *      prefix and suffix unions below have the same limit: on a tie they keep `mine`, the reference the neighbour.
 *      bvh_build_gpu (ptx_api.inc) therefore refuses boxes of which one bound column holds both zeros; the photon
 *      map's device-resident boxes are not checked, see DESIGN F3), then one thread per axis builds the prefix
 *      boxes and evaluates the candidate costs with the reference's arithmetic and tie rules (List.min_elt = first
 *      minimum of a consed list);
 *   3. the leaf test of Tree.create;
 *   4. Slice.partition_in_place, reproduced exactly: the Hoare scan swaps the q-th misplaced element from the
 *      left with the q-th misplaced element from the right, so two prefix scans give every element's final
 *      position and the permutation is applied in parallel;
 *   5. pushes the two children onto the next level's work lists.
 * Three implementations of the same steps, chosen by segment size (a level's segments differ 1 : 10^6):
 *   small  (n <= 64)          one WAVE per segment, one element per lane, no workgroup barriers  -- k_bvh_small
 *   medium                    one 256-thread workgroup per segment, bins in LDS                  -- k_bvh_level
 *   big    (n >= BVH_BIG_MIN) many workgroups per segment (tiles of BVH_TILE elements), bins and
 *                             scan offsets in global memory, seven short kernels                 -- k_big_*
 * Afterwards the tree is numbered in pre-order (node, lhs subtree, rhs subtree) and the leaf slots are laid out,
 * also level by level on the device (k_fin_*): subtree sizes bottom-up, indices top-down.
 */

struct BvhSeg { /* one pending node */
  int lo, hi;
  int node; /* index in the temporary node array */
  int pad;
  double box[6];
};
struct BvhTmpNode {
  double box[6];
  int lo, hi;
  int leaf;
  int axis;
  int lhs, rhs; /* temporary indices */
};

__device__ __forceinline__ unsigned long long bvh_enc(double x) { /* order-preserving f64 -> u64 */
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double bvh_dec(unsigned long long u) {
  const unsigned long long b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
  return __longlong_as_double((long long)b);
}

#define BVH_MAX_BINS 64
#define BVH_BLOCK 256
#define BVH_SMALL_MAX 64   /* <= one wave of elements */
#define BVH_BIG_MIN 8192   /* from here on a segment is spread over several workgroups */
#define BVH_TILE 2048      /* elements of a big segment per workgroup */

struct BvhSplit {
  int valid;
  int axis, index;
  double cost, scale, origin;
  double lhs[6], rhs[6];
};

/* next level's work lists by size class + the node allocator */
struct BvhLists {
  BvhSeg* seg[3]; /* small, medium, big */
  int* count;     /* [0..2] list lengths, [3] nodes allocated so far */
};

/* OCaml Float.compare: nan = nan, nan below everything */
__device__ __forceinline__ int bvh_compare(double a, double b) {
  if (a != a) return (b != b) ? 0 : -1;
  if (b != b) return 1;
  return a < b ? -1 : (a > b ? 1 : 0);
}
__device__ __forceinline__ double bvh_area(const double* b) { /* Bbox.surface_area, bbox.ml:33-38 */
  const double x = b[3] - b[0], y = b[4] - b[1], z = b[5] - b[2];
  return 2.0 * pt_fma(x, y, pt_fma(y, z, z * x));
}

/* Proposal candidates of ONE axis (shape_tree.ml:91-119), run by one thread.  bin[j][0..5] = encoded bounds of
 * bin j, cnt[j] its element count; lbox / lhas = scratch for Bin.populate_bbox_l (:62-69).  bbox_r (:53-60) is
 * kept as a running box while p walks DOWN: the reference conses candidates for p = 0.. and List.min_elt keeps
 * the first minimum, i.e. the HIGHEST p among equal costs -- walking down and replacing only on `<` is the same. */
template <class BinT, class CntT>
__device__ __forceinline__ BvhSplit bvh_axis_candidates(int a, int n, int num_bins, double scale, double origin, bool axis_ok,
                                                        const BinT* bin /* [num_bins][6] */, const CntT* cnt,
                                                        double (*lbox)[6], unsigned char* lhas) {
  BvhSplit best;
  best.valid = 0;
  if (!axis_ok) return best;
  for (int j = 0; j < num_bins; ++j) {
    const bool has = cnt[j] > 0;
    const bool nb = j > 0 && lhas[j - 1];
    for (int k = 0; k < 6; ++k) {
      const double mine = has ? bvh_dec(bin[j * 6 + k]) : 0.0;
      double v = mine;
      if (has && nb) v = (k < 3) ? (lbox[j - 1][k] < mine ? lbox[j - 1][k] : mine) : (lbox[j - 1][k] > mine ? lbox[j - 1][k] : mine);
      else if (!has && nb) v = lbox[j - 1][k];
      lbox[j][k] = v;
    }
    lhas[j] = (has || nb) ? 1 : 0;
  }
  const double total_area = bvh_area(lbox[num_bins - 1]);
  double rb[6] = {0, 0, 0, 0, 0, 0};
  bool rhas = false;
  int n_right = 0;
  for (int p = num_bins - 2; p >= 0; --p) {
    const int j = p + 1;
    const bool has = cnt[j] > 0;
    for (int k = 0; k < 6; ++k) {
      const double mine = has ? bvh_dec(bin[j * 6 + k]) : 0.0;
      if (has && rhas) rb[k] = (k < 3) ? (rb[k] < mine ? rb[k] : mine) : (rb[k] > mine ? rb[k] : mine);
      else if (has) rb[k] = mine;
    }
    rhas = has || rhas;
    n_right += (int)cnt[j];
    if (!lhas[p] || !rhas) continue;
    const int n_left = n - n_right;
    const double lhs_area = (double)n_left * bvh_area(lbox[p]);
    const double rhs_area = (double)n_right * bvh_area(rb);
    const double cost = 0.25 + ((lhs_area + rhs_area) * 1.0 / total_area);
    if (!best.valid || bvh_compare(cost, best.cost) < 0) {
      best.valid = 1;
      best.cost = cost;
      best.axis = a;
      best.index = p;
      best.scale = scale;
      best.origin = origin;
      for (int k = 0; k < 6; ++k) {
        best.lhs[k] = lbox[p][k];
        best.rhs[k] = rb[k];
      }
    }
  }
  return best;
}

/* Proposal.create (:141-146: X, Y, Z, first minimum), the leaf test of Tree.create (:177-196), the node record and
 * the allocation of the two children.  Returns the split to apply (valid = 0 for a leaf); *children = temp index
 * of the lhs child. */
__device__ __forceinline__ BvhSplit bvh_decide(const BvhSplit* axis3, const BvhSeg& seg, int cutoff, BvhTmpNode* nodes,
                                               int* node_count, int* children) {
  BvhSplit best;
  best.valid = 0;
  for (int a = 0; a < 3; ++a) {
    if (!axis3[a].valid) continue;
    if (!best.valid || bvh_compare(axis3[a].cost, best.cost) < 0) best = axis3[a];
  }
  const int n = seg.hi - seg.lo;
  const double leaf_cost = 1.0 * (double)n;
  const bool leaf = !best.valid || (best.cost >= leaf_cost && n <= cutoff) || n <= 4;
  BvhTmpNode nd;
  for (int k = 0; k < 6; ++k) nd.box[k] = seg.box[k];
  nd.lo = seg.lo;
  nd.hi = seg.hi;
  nd.leaf = leaf ? 1 : 0;
  nd.axis = leaf ? -1 : best.axis;
  nd.lhs = nd.rhs = -1;
  if (!leaf) {
    const int c = atomicAdd(node_count, 2);
    nd.lhs = c;
    nd.rhs = c + 1;
    *children = c;
  } else {
    best.valid = 0;
  }
  nodes[seg.node] = nd;
  return best;
}

__device__ __forceinline__ void bvh_push_child(const BvhLists& out, int lo, int hi, int node, const double* box) {
  const int n = hi - lo;
  const int cls = n <= BVH_SMALL_MAX ? 0 : (n >= BVH_BIG_MIN ? 2 : 1);
  const int at = atomicAdd(out.count + cls, 1);
  BvhSeg s;
  s.lo = lo; s.hi = hi; s.node = node; s.pad = 0;
  for (int k = 0; k < 6; ++k) s.box[k] = box[k];
  out.seg[cls][at] = s;
}

__device__ __forceinline__ bool bvh_goes_left(const double* prim_box, int elt, const BvhSplit& sp) {
  const double* b = prim_box + (size_t)elt * 6;
  const double c = 0.5 * (b[sp.axis] + b[sp.axis + 3]);
  return (int)(sp.scale * (c - sp.origin)) <= sp.index; /* Float.to_int truncates */
}

/* ------------------------------------------------------------------ medium: one workgroup per segment */
__global__ __launch_bounds__(BVH_BLOCK) void k_bvh_level(const double* __restrict__ prim_box /* n x 6 */,
                                                         int* __restrict__ order, int* __restrict__ scratch /* 2n */,
                                                         const BvhSeg* __restrict__ segs, int n_segs, BvhLists out,
                                                         BvhTmpNode* __restrict__ nodes, int n_total, int num_bins,
                                                         int cutoff) {
  __shared__ unsigned long long s_cb[6];                       /* centroid bbox, encoded */
  __shared__ unsigned long long s_bin[3][BVH_MAX_BINS * 6];     /* per-bin bounds, encoded */
  __shared__ int s_cnt[3][BVH_MAX_BINS];
  /* private copies for waves 1..3 (wave 0 uses s_bin / s_cnt directly): 4x less LDS-atomic contention */
  __shared__ unsigned long long s_pbin[BVH_BLOCK / 64 - 1][3][BVH_MAX_BINS * 6];
  __shared__ int s_pcnt[BVH_BLOCK / 64 - 1][3][BVH_MAX_BINS];
  __shared__ double s_lbox[3][BVH_MAX_BINS][6]; /* Bin.bbox_l */
  __shared__ unsigned char s_lhas[3][BVH_MAX_BINS];
  __shared__ BvhSplit s_axis[3];
  __shared__ BvhSplit s_best;
  __shared__ int s_wave[BVH_BLOCK / 64];
  __shared__ int s_carry;
  __shared__ int s_children;
  const int tid = (int)threadIdx.x;
  const int seg_i = (int)blockIdx.x;
  if (seg_i >= n_segs) return;
  const BvhSeg seg = segs[seg_i];
  const int lo = seg.lo, n = seg.hi - seg.lo;

  /* ---- 1. centroid bbox (Bshape.centroid_bbox, shape_tree.ml:21-24; centroid = Bbox.center, bbox.ml:12) ---- */
  if (tid < 6) s_cb[tid] = (tid < 3) ? ~0ull : 0ull;
  const bool private_bins = n >= 2048; /* small nodes: too few elements per bin to contend */
  for (int a = tid; a < 3 * BVH_MAX_BINS; a += BVH_BLOCK) {
    const int ax = a / BVH_MAX_BINS, bn = a % BVH_MAX_BINS;
    s_cnt[ax][bn] = 0;
    for (int k = 0; k < 6; ++k) s_bin[ax][bn * 6 + k] = (k < 3) ? ~0ull : 0ull;
    if (private_bins)
      for (int w = 0; w < BVH_BLOCK / 64 - 1; ++w) {
        s_pcnt[w][ax][bn] = 0;
        for (int k = 0; k < 6; ++k) s_pbin[w][ax][bn * 6 + k] = (k < 3) ? ~0ull : 0ull;
      }
  }
  __syncthreads();
  {
    unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    for (int k = tid; k < n; k += BVH_BLOCK) {
      const double* b = prim_box + (size_t)order[lo + k] * 6;
      for (int a = 0; a < 3; ++a) {
        const unsigned long long e = bvh_enc(0.5 * (b[a] + b[a + 3]));
        mn[a] = e < mn[a] ? e : mn[a];
        mx[a] = e > mx[a] ? e : mx[a];
      }
    }
    for (int a = 0; a < 3; ++a) { /* wave reduction, then one LDS atomic per wave */
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o1 = __shfl_xor(mn[a], off, 64), o2 = __shfl_xor(mx[a], off, 64);
        mn[a] = o1 < mn[a] ? o1 : mn[a];
        mx[a] = o2 > mx[a] ? o2 : mx[a];
      }
      if ((tid & 63) == 0) {
        atomicMin(&s_cb[a], mn[a]);
        atomicMax(&s_cb[a + 3], mx[a]);
      }
    }
  }
  __syncthreads();

  /* ---- 2. bins for the three axes (propose_split_one_axis, shape_tree.ml:123-139; Bin.insert :41-51) ---- */
  const double epsilon = 1e-6;
  double scale[3], origin[3];
  bool axis_ok[3];
  for (int a = 0; a < 3; ++a) {
    const double cb_min = bvh_dec(s_cb[a]), cb_max = bvh_dec(s_cb[a + 3]);
    origin[a] = cb_min;
    scale[a] = (double)num_bins * (1.0 - epsilon) / (cb_max - cb_min);
    axis_ok[a] = pt_isfinite(scale[a]) != 0;
  }
  for (int k = tid; k < n; k += BVH_BLOCK) {
    const double* b = prim_box + (size_t)order[lo + k] * 6;
    for (int a = 0; a < 3; ++a) {
      if (!axis_ok[a]) continue;
      const double c = 0.5 * (b[a] + b[a + 3]);
      const int bin = (int)(scale[a] * (c - origin[a])); /* Float.to_int truncates */
      const int pw = (tid >> 6) - 1;
      int* cnt = (private_bins && pw >= 0) ? &s_pcnt[pw][a][bin] : &s_cnt[a][bin];
      unsigned long long* bb = (private_bins && pw >= 0) ? &s_pbin[pw][a][bin * 6] : &s_bin[a][bin * 6];
      atomicAdd(cnt, 1);
      for (int j = 0; j < 3; ++j) {
        atomicMin(&bb[j], bvh_enc(b[j]));
        atomicMax(&bb[j + 3], bvh_enc(b[j + 3]));
      }
    }
  }
  __syncthreads();
  if (private_bins) { /* merge the private copies (min/max and counts are order-independent) */
    for (int a = tid; a < 3 * BVH_MAX_BINS; a += BVH_BLOCK) {
      const int ax = a / BVH_MAX_BINS, bn = a % BVH_MAX_BINS;
      for (int w = 0; w < BVH_BLOCK / 64 - 1; ++w) {
        s_cnt[ax][bn] += s_pcnt[w][ax][bn];
        for (int k = 0; k < 3; ++k) {
          if (s_pbin[w][ax][bn * 6 + k] < s_bin[ax][bn * 6 + k]) s_bin[ax][bn * 6 + k] = s_pbin[w][ax][bn * 6 + k];
          if (s_pbin[w][ax][bn * 6 + k + 3] > s_bin[ax][bn * 6 + k + 3]) s_bin[ax][bn * 6 + k + 3] = s_pbin[w][ax][bn * 6 + k + 3];
        }
      }
    }
    __syncthreads();
  }
  if (tid < 3)
    s_axis[tid] = bvh_axis_candidates(tid, n, num_bins, scale[tid], origin[tid], axis_ok[tid], s_bin[tid], s_cnt[tid],
                                      s_lbox[tid], s_lhas[tid]);
  __syncthreads();

  /* ---- 3. choose, leaf test, node record ---- */
  if (tid == 0) {
    int children = -1;
    s_best = bvh_decide(s_axis, seg, cutoff, nodes, out.count + 3, &children);
    s_children = children;
    s_carry = 0;
  }
  __syncthreads();
  if (!s_best.valid) return;
  const BvhSplit sp = s_best;

  /* ---- 4. Slice.partition_in_place (slice.ml:67-80) ---- */
  int L = 0; /* number of lhs elements = the split position */
  for (int p = 0; p <= sp.index; ++p) L += s_cnt[sp.axis][p];
  int* ml = scratch + lo;           /* q-th misplaced (rhs) element among the first L positions, from the left */
  int* mr = scratch + n_total + lo; /* q-th misplaced (lhs) element among the last n-L positions, from the right */
  const int lane = tid & 63, wave = tid >> 6;
  for (int base = 0; base < L; base += BVH_BLOCK) { /* forward scan over [0, L) */
    const int k = base + tid;
    const bool mis = k < L && !bvh_goes_left(prim_box, order[lo + k], sp);
    const unsigned long long m = __ballot(mis);
    if (lane == 0) s_wave[wave] = (int)__popcll(m);
    __syncthreads();
    int before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (mis) ml[before + (int)__popcll(m & ((1ull << lane) - 1ull))] = k;
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < BVH_BLOCK / 64; ++w) t += s_wave[w];
      s_carry += t;
    }
    __syncthreads();
  }
  const int n_mis = s_carry;
  __syncthreads();
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n - L; base += BVH_BLOCK) { /* backward scan over [L, n): position n-1-j for j = 0.. */
    const int j = base + tid;
    const int k = n - 1 - j;
    const bool mis = j < n - L && bvh_goes_left(prim_box, order[lo + k], sp);
    const unsigned long long m = __ballot(mis);
    if (lane == 0) s_wave[wave] = (int)__popcll(m);
    __syncthreads();
    int before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (mis) mr[before + (int)__popcll(m & ((1ull << lane) - 1ull))] = k;
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < BVH_BLOCK / 64; ++w) t += s_wave[w];
      s_carry += t;
    }
    __syncthreads();
  }
  __syncthreads();
  for (int q = tid; q < n_mis; q += BVH_BLOCK) { /* the q-th pair is swapped */
    const int a = lo + ml[q], b = lo + mr[q];
    const int t = order[a];
    order[a] = order[b];
    order[b] = t;
  }

  /* ---- 5. children ---- */
  if (tid == 0) {
    bvh_push_child(out, lo, lo + L, s_children, sp.lhs);
    bvh_push_child(out, lo + L, seg.hi, s_children + 1, sp.rhs);
  }
}

/* ------------------------------------------------------------------ small: one wave per segment */
/* LDS written by some lanes of a wave is read by others: keep the compiler from moving accesses across this point
 * (the hardware executes a wave's LDS instructions in order) */
__device__ __forceinline__ void bvh_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
/* dynamic LDS per wave: bins u64[3][nb*6], counts int[3][nb], lbox double[3][nb][6], lhas u8[3][nb] (+ pad) */
__host__ __device__ inline size_t bvh_small_lds_per_wave(int num_bins) {
  const size_t b = (size_t)3 * num_bins * (6 * 8 + 4 + 6 * 8 + 1) + 3 * sizeof(BvhSplit) + 64;
  return (b + 15) & ~(size_t)15;
}
/* Proposal.create + the leaf test only (no allocation): valid = 0 for a leaf */
__device__ __forceinline__ BvhSplit bvh_choose(const BvhSplit* axis3, int n, int cutoff) {
  BvhSplit best;
  best.valid = 0;
  for (int a = 0; a < 3; ++a) {
    if (!axis3[a].valid) continue;
    if (!best.valid || bvh_compare(axis3[a].cost, best.cost) < 0) best = axis3[a];
  }
  const double leaf_cost = 1.0 * (double)n;
  const bool leaf = !best.valid || (best.cost >= leaf_cost && n <= cutoff) || n <= 4;
  if (leaf) best.valid = 0;
  return best;
}

/* Up to BVH_SMALL_WAVES segments per workgroup, one per wave.  Node ids and work-list slots are allocated ONCE PER
 * WORKGROUP (the deep levels hold 100 k+ segments: one atomic per segment on the same two counters ran the level at
 * the chip's same-address atomic rate, ~2.6 ms; per workgroup it is ~0.3 ms). */
#define BVH_SMALL_WAVES 16
__global__ __launch_bounds__(BVH_SMALL_WAVES * 64) void k_bvh_small(const double* __restrict__ prim_box, int* __restrict__ order,
                                                                    const BvhSeg* __restrict__ segs, int n_segs, BvhLists out,
                                                                    BvhTmpNode* __restrict__ nodes, int num_bins, int cutoff) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bvh_lds[];
  __shared__ int s_split[BVH_SMALL_WAVES];      /* 1: this wave's segment splits */
  __shared__ int s_cls[BVH_SMALL_WAVES][2];     /* work-list class of its two children */
  __shared__ int s_node0[BVH_SMALL_WAVES];      /* temp id of its lhs child */
  __shared__ int s_slot[BVH_SMALL_WAVES][2];    /* positions of its children in their lists */
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
  const int seg_i = (int)blockIdx.x * n_waves + wave;
  const bool have = seg_i < n_segs;
  unsigned char* base = bvh_lds + (size_t)wave * bvh_small_lds_per_wave(num_bins);
  unsigned long long* w_bin = (unsigned long long*)base;                       /* [3][nb*6] */
  double* w_lbox = (double*)(base + (size_t)3 * num_bins * 48);                 /* [3][nb][6] */
  BvhSplit* w_axis = (BvhSplit*)(base + (size_t)3 * num_bins * 96);             /* [3] */
  int* w_cnt = (int*)(base + (size_t)3 * num_bins * 96 + 3 * sizeof(BvhSplit)); /* [3][nb] */
  unsigned char* w_lhas = (unsigned char*)(w_cnt + 3 * num_bins);               /* [3][nb] */
  BvhSeg seg;
  seg.lo = seg.hi = 0;
  seg.node = 0;
  if (have) seg = segs[seg_i];
  const int lo = seg.lo, n = seg.hi - seg.lo; /* 1 <= n <= 64 when have */
  const bool mine = have && lane < n;
  const int elt = mine ? order[lo + lane] : 0;
  double b[6] = {0, 0, 0, 0, 0, 0};
  if (mine)
    for (int k = 0; k < 6; ++k) b[k] = prim_box[(size_t)elt * 6 + k];
  BvhSplit sp;
  sp.valid = 0;
  int L = 0;
  if (have) { /* wave-uniform */
    /* 1. centroid bbox */
    unsigned long long mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
      const unsigned long long e = bvh_enc(0.5 * (b[a] + b[a + 3]));
      mn[a] = mine ? e : ~0ull;
      mx[a] = mine ? e : 0ull;
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o1 = __shfl_xor(mn[a], off, 64), o2 = __shfl_xor(mx[a], off, 64);
        mn[a] = o1 < mn[a] ? o1 : mn[a];
        mx[a] = o2 > mx[a] ? o2 : mx[a];
      }
    }
    /* 2. bins */
    const double epsilon = 1e-6;
    double scale[3], origin[3];
    bool axis_ok[3];
    for (int a = 0; a < 3; ++a) {
      const double cb_min = bvh_dec(mn[a]), cb_max = bvh_dec(mx[a]);
      origin[a] = cb_min;
      scale[a] = (double)num_bins * (1.0 - epsilon) / (cb_max - cb_min);
      axis_ok[a] = pt_isfinite(scale[a]) != 0;
    }
    for (int j = lane; j < 3 * num_bins; j += 64) {
      w_cnt[j] = 0;
      for (int k = 0; k < 6; ++k) w_bin[(size_t)j * 6 + k] = (k < 3) ? ~0ull : 0ull;
    }
    bvh_wave_sync();
    if (mine) {
      for (int a = 0; a < 3; ++a) {
        if (!axis_ok[a]) continue;
        const double c = 0.5 * (b[a] + b[a + 3]);
        const int bin = (int)(scale[a] * (c - origin[a]));
        atomicAdd(&w_cnt[a * num_bins + bin], 1);
        unsigned long long* bb = w_bin + ((size_t)a * num_bins + bin) * 6;
        for (int j = 0; j < 3; ++j) {
          atomicMin(&bb[j], bvh_enc(b[j]));
          atomicMax(&bb[j + 3], bvh_enc(b[j + 3]));
        }
      }
    }
    bvh_wave_sync();
    if (lane < 3)
      w_axis[lane] = bvh_axis_candidates(lane, n, num_bins, scale[lane], origin[lane], axis_ok[lane],
                                         w_bin + (size_t)lane * num_bins * 6, w_cnt + lane * num_bins,
                                         (double(*)[6])(w_lbox + (size_t)lane * num_bins * 6), w_lhas + lane * num_bins);
    bvh_wave_sync();
    /* 3. choose (lane 0), broadcast through LDS */
    if (lane == 0) w_axis[0] = bvh_choose(w_axis, n, cutoff);
    bvh_wave_sync();
    sp = w_axis[0];
    /* 4. partition: lane k holds position k */
    if (sp.valid) {
      const bool left = mine && bvh_goes_left(prim_box, elt, sp);
      const unsigned long long lm = __ballot(left);
      L = (int)__popcll(lm);
      const bool mis_l = mine && lane < L && !left; /* rhs element among the first L positions */
      const bool mis_r = mine && lane >= L && left; /* lhs element among the last n - L positions */
      const unsigned long long ml_m = __ballot(mis_l), mr_m = __ballot(mis_r);
      int new_elt = elt;
      if (ml_m != 0) {
        /* rank from the left among ml, from the right among mr; partner = the lane with the same rank */
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long above = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);
        const int my_rank = mis_l ? (int)__popcll(ml_m & below) : (mis_r ? (int)__popcll(mr_m & above) : -1);
        int partner = lane;
        if (mis_l) { /* my_rank-th highest set bit of mr_m */
          unsigned long long m = mr_m;
          for (int r = 0; r < my_rank; ++r) m &= ~(1ull << (63 - __clzll((long long)m)));
          partner = 63 - __clzll((long long)m);
        } else if (mis_r) { /* my_rank-th lowest set bit of ml_m */
          unsigned long long m = ml_m;
          for (int r = 0; r < my_rank; ++r) m &= m - 1ull;
          partner = __ffsll((long long)m) - 1;
        }
        new_elt = __shfl(elt, partner, 64);
      }
      if (mine && new_elt != elt) order[lo + lane] = new_elt;
    }
  }
  /* 5. one allocation per workgroup: node ids (two per split) and work-list slots (one per child, by class) */
  if (lane == 0) {
    s_split[wave] = sp.valid ? 1 : 0;
    const int nl = L, nr = n - L;
    s_cls[wave][0] = nl <= BVH_SMALL_MAX ? 0 : (nl >= BVH_BIG_MIN ? 2 : 1);
    s_cls[wave][1] = nr <= BVH_SMALL_MAX ? 0 : (nr >= BVH_BIG_MIN ? 2 : 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int splits = 0, per_cls[3] = {0, 0, 0};
    for (int w = 0; w < n_waves; ++w)
      if (s_split[w]) {
        s_node0[w] = 2 * splits++;
        for (int c = 0; c < 2; ++c) s_slot[w][c] = per_cls[s_cls[w][c]]++;
      }
    if (splits > 0) {
      const int node_base = atomicAdd(out.count + 3, 2 * splits);
      int cls_base[3] = {0, 0, 0};
      for (int k = 0; k < 3; ++k)
        if (per_cls[k] > 0) cls_base[k] = atomicAdd(out.count + k, per_cls[k]);
      for (int w = 0; w < n_waves; ++w)
        if (s_split[w]) {
          s_node0[w] += node_base;
          for (int c = 0; c < 2; ++c) s_slot[w][c] += cls_base[s_cls[w][c]];
        }
    }
  }
  __syncthreads();
  if (have && lane == 0) {
    BvhTmpNode nd;
    for (int k = 0; k < 6; ++k) nd.box[k] = seg.box[k];
    nd.lo = seg.lo;
    nd.hi = seg.hi;
    nd.leaf = sp.valid ? 0 : 1;
    nd.axis = sp.valid ? sp.axis : -1;
    nd.lhs = sp.valid ? s_node0[wave] : -1;
    nd.rhs = sp.valid ? s_node0[wave] + 1 : -1;
    nodes[seg.node] = nd;
    if (sp.valid) {
      BvhSeg l, r;
      l.lo = lo; l.hi = lo + L; l.node = s_node0[wave]; l.pad = 0;
      r.lo = lo + L; r.hi = seg.hi; r.node = s_node0[wave] + 1; r.pad = 0;
      for (int k = 0; k < 6; ++k) {
        l.box[k] = sp.lhs[k];
        r.box[k] = sp.rhs[k];
      }
      out.seg[s_cls[wave][0]][s_slot[wave][0]] = l;
      out.seg[s_cls[wave][1]][s_slot[wave][1]] = r;
    }
  }
}

/* ------------------------------------------------------------------ big: many workgroups per segment */
struct BvhBigSeg {
  BvhSeg seg;
  int tile0, n_tiles; /* this segment's tiles are [tile0, tile0 + n_tiles) of the level's tile table */
  int pad0, pad1;
};
struct BvhBigState { /* per big segment, in global memory */
  unsigned long long cb[6];
  unsigned long long bin[3][BVH_MAX_BINS * 6];
  int cnt[3][BVH_MAX_BINS];
  BvhSplit split;
  int L, n_mis, children, pad;
};

__global__ __launch_bounds__(BVH_BLOCK) void k_big_init(BvhBigState* __restrict__ st, int n_big) {
  const int i = (int)blockIdx.x;
  if (i >= n_big) return;
  BvhBigState& s = st[i];
  const int tid = (int)threadIdx.x;
  if (tid < 6) s.cb[tid] = (tid < 3) ? ~0ull : 0ull;
  for (int a = tid; a < 3 * BVH_MAX_BINS; a += BVH_BLOCK) {
    const int ax = a / BVH_MAX_BINS, bn = a % BVH_MAX_BINS;
    s.cnt[ax][bn] = 0;
    for (int k = 0; k < 6; ++k) s.bin[ax][bn * 6 + k] = (k < 3) ? ~0ull : 0ull;
  }
  if (tid == 0) {
    s.split.valid = 0;
    s.L = 0;
    s.n_mis = 0;
    s.children = -1;
  }
}

/* tile t of the level: tiles[t] = {big segment index, tile index inside it} */
__global__ __launch_bounds__(BVH_BLOCK) void k_big_centroid(const double* __restrict__ prim_box, const int* __restrict__ order,
                                                            const BvhBigSeg* __restrict__ big, const int2* __restrict__ tiles,
                                                            BvhBigState* __restrict__ st) {
  const int2 tl = tiles[blockIdx.x];
  const BvhBigSeg& bs = big[tl.x];
  const int lo = bs.seg.lo, n = bs.seg.hi - bs.seg.lo;
  const int k0 = tl.y * BVH_TILE, k1 = min(n, k0 + BVH_TILE);
  unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
  for (int k = k0 + (int)threadIdx.x; k < k1; k += BVH_BLOCK) {
    const double* b = prim_box + (size_t)order[lo + k] * 6;
    for (int a = 0; a < 3; ++a) {
      const unsigned long long e = bvh_enc(0.5 * (b[a] + b[a + 3]));
      mn[a] = e < mn[a] ? e : mn[a];
      mx[a] = e > mx[a] ? e : mx[a];
    }
  }
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o1 = __shfl_xor(mn[a], off, 64), o2 = __shfl_xor(mx[a], off, 64);
      mn[a] = o1 < mn[a] ? o1 : mn[a];
      mx[a] = o2 > mx[a] ? o2 : mx[a];
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&st[tl.x].cb[a], mn[a]);
      atomicMax(&st[tl.x].cb[a + 3], mx[a]);
    }
  }
}

__device__ __forceinline__ void bvh_big_axes(const BvhBigState& s, int num_bins, double* scale, double* origin, bool* axis_ok) {
  const double epsilon = 1e-6;
  for (int a = 0; a < 3; ++a) {
    const double cb_min = bvh_dec(s.cb[a]), cb_max = bvh_dec(s.cb[a + 3]);
    origin[a] = cb_min;
    scale[a] = (double)num_bins * (1.0 - epsilon) / (cb_max - cb_min);
    axis_ok[a] = pt_isfinite(scale[a]) != 0;
  }
}

__global__ __launch_bounds__(BVH_BLOCK) void k_big_bins(const double* __restrict__ prim_box, const int* __restrict__ order,
                                                        const BvhBigSeg* __restrict__ big, const int2* __restrict__ tiles,
                                                        BvhBigState* __restrict__ st, int num_bins) {
  __shared__ unsigned long long s_bin[BVH_BLOCK / 64][3][BVH_MAX_BINS * 6]; /* one copy per wave */
  __shared__ int s_cnt[BVH_BLOCK / 64][3][BVH_MAX_BINS];
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  const int2 tl = tiles[blockIdx.x];
  const BvhBigSeg& bs = big[tl.x];
  BvhBigState& s = st[tl.x];
  const int lo = bs.seg.lo, n = bs.seg.hi - bs.seg.lo;
  const int k0 = tl.y * BVH_TILE, k1 = min(n, k0 + BVH_TILE);
  for (int a = tid; a < 3 * BVH_MAX_BINS; a += BVH_BLOCK) {
    const int ax = a / BVH_MAX_BINS, bn = a % BVH_MAX_BINS;
    for (int w = 0; w < BVH_BLOCK / 64; ++w) {
      s_cnt[w][ax][bn] = 0;
      for (int k = 0; k < 6; ++k) s_bin[w][ax][bn * 6 + k] = (k < 3) ? ~0ull : 0ull;
    }
  }
  __syncthreads();
  double scale[3], origin[3];
  bool axis_ok[3];
  bvh_big_axes(s, num_bins, scale, origin, axis_ok);
  for (int k = k0 + tid; k < k1; k += BVH_BLOCK) {
    const double* b = prim_box + (size_t)order[lo + k] * 6;
    for (int a = 0; a < 3; ++a) {
      if (!axis_ok[a]) continue;
      const double c = 0.5 * (b[a] + b[a + 3]);
      const int bin = (int)(scale[a] * (c - origin[a]));
      atomicAdd(&s_cnt[wave][a][bin], 1);
      unsigned long long* bb = &s_bin[wave][a][bin * 6];
      for (int j = 0; j < 3; ++j) {
        atomicMin(&bb[j], bvh_enc(b[j]));
        atomicMax(&bb[j + 3], bvh_enc(b[j + 3]));
      }
    }
  }
  __syncthreads();
  for (int a = tid; a < 3 * num_bins; a += BVH_BLOCK) {
    const int ax = a / num_bins, bn = a % num_bins;
    int c = 0;
    unsigned long long m[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    for (int w = 0; w < BVH_BLOCK / 64; ++w) {
      c += s_cnt[w][ax][bn];
      for (int k = 0; k < 3; ++k) {
        m[k] = s_bin[w][ax][bn * 6 + k] < m[k] ? s_bin[w][ax][bn * 6 + k] : m[k];
        m[k + 3] = s_bin[w][ax][bn * 6 + k + 3] > m[k + 3] ? s_bin[w][ax][bn * 6 + k + 3] : m[k + 3];
      }
    }
    if (c > 0) {
      atomicAdd(&s.cnt[ax][bn], c);
      for (int k = 0; k < 3; ++k) {
        atomicMin(&s.bin[ax][bn * 6 + k], m[k]);
        atomicMax(&s.bin[ax][bn * 6 + k + 3], m[k + 3]);
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_big_split(const BvhBigSeg* __restrict__ big, int n_big, BvhBigState* __restrict__ st,
                                                  BvhLists out, BvhTmpNode* __restrict__ nodes, int num_bins, int cutoff) {
  __shared__ double s_lbox[3][BVH_MAX_BINS][6];
  __shared__ unsigned char s_lhas[3][BVH_MAX_BINS];
  __shared__ BvhSplit s_axis[3];
  const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (i >= n_big) return;
  BvhBigState& s = st[i];
  const BvhSeg seg = big[i].seg;
  const int n = seg.hi - seg.lo;
  double scale[3], origin[3];
  bool axis_ok[3];
  bvh_big_axes(s, num_bins, scale, origin, axis_ok);
  if (tid < 3)
    s_axis[tid] = bvh_axis_candidates(tid, n, num_bins, scale[tid], origin[tid], axis_ok[tid], s.bin[tid], s.cnt[tid],
                                      s_lbox[tid], s_lhas[tid]);
  __syncthreads();
  if (tid == 0) {
    int children = -1;
    const BvhSplit best = bvh_decide(s_axis, seg, cutoff, nodes, out.count + 3, &children);
    int L = 0;
    if (best.valid) {
      for (int p = 0; p <= best.index; ++p) L += s.cnt[best.axis][p];
      bvh_push_child(out, seg.lo, seg.lo + L, children, best.lhs);
      bvh_push_child(out, seg.lo + L, seg.hi, children + 1, best.rhs);
    }
    s.split = best;
    s.L = L;
    s.children = children;
  }
}

/* per tile: how many misplaced elements it holds on each side of the split position */
__global__ __launch_bounds__(BVH_BLOCK) void k_big_count(const double* __restrict__ prim_box, const int* __restrict__ order,
                                                         const BvhBigSeg* __restrict__ big, const int2* __restrict__ tiles,
                                                         const BvhBigState* __restrict__ st, int* __restrict__ tile_cl,
                                                         int* __restrict__ tile_cr) {
  __shared__ int s_l, s_r;
  const int tid = (int)threadIdx.x;
  const int2 tl = tiles[blockIdx.x];
  const BvhBigState& s = st[tl.x];
  if (tid == 0) s_l = s_r = 0;
  __syncthreads();
  if (s.split.valid) {
    const BvhSplit sp = s.split;
    const int lo = big[tl.x].seg.lo, n = big[tl.x].seg.hi - lo, L = s.L;
    const int k0 = tl.y * BVH_TILE, k1 = min(n, k0 + BVH_TILE);
    int cl = 0, cr = 0;
    for (int k = k0 + tid; k < k1; k += BVH_BLOCK) {
      const bool left = bvh_goes_left(prim_box, order[lo + k], sp);
      cl += (k < L && !left) ? 1 : 0;
      cr += (k >= L && left) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
      cl += __shfl_xor(cl, off, 64);
      cr += __shfl_xor(cr, off, 64);
    }
    if ((tid & 63) == 0) {
      atomicAdd(&s_l, cl);
      atomicAdd(&s_r, cr);
    }
  }
  __syncthreads();
  if (tid == 0) {
    tile_cl[blockIdx.x] = s_l;
    tile_cr[blockIdx.x] = s_r;
  }
}

/* per big segment: exclusive offsets of its tiles -- ascending tiles for the left side, descending for the right */
__global__ void k_big_offsets(const BvhBigSeg* __restrict__ big, int n_big, BvhBigState* __restrict__ st,
                              int* __restrict__ tile_cl, int* __restrict__ tile_cr) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n_big) return;
  const int t0 = big[i].tile0, nt = big[i].n_tiles;
  int acc = 0;
  for (int t = 0; t < nt; ++t) {
    const int c = tile_cl[t0 + t];
    tile_cl[t0 + t] = acc;
    acc += c;
  }
  st[i].n_mis = acc;
  acc = 0;
  for (int t = nt - 1; t >= 0; --t) {
    const int c = tile_cr[t0 + t];
    tile_cr[t0 + t] = acc;
    acc += c;
  }
}

/* per tile: write the positions of its misplaced elements at their ranks (ml ascending, mr descending) */
__global__ __launch_bounds__(BVH_BLOCK) void k_big_scatter(const double* __restrict__ prim_box, const int* __restrict__ order,
                                                           int* __restrict__ scratch, int n_total,
                                                           const BvhBigSeg* __restrict__ big, const int2* __restrict__ tiles,
                                                           const BvhBigState* __restrict__ st, const int* __restrict__ tile_offl,
                                                           const int* __restrict__ tile_offr) {
  __shared__ int s_wave[BVH_BLOCK / 64];
  __shared__ int s_carry;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int2 tl = tiles[blockIdx.x];
  const BvhBigState& s = st[tl.x];
  if (!s.split.valid) return;
  const BvhSplit sp = s.split;
  const int lo = big[tl.x].seg.lo, n = big[tl.x].seg.hi - lo, L = s.L;
  const int k0 = tl.y * BVH_TILE, k1 = min(n, k0 + BVH_TILE);
  int* ml = scratch + lo;
  int* mr = scratch + n_total + lo;
  for (int side = 0; side < 2; ++side) {
    if (tid == 0) s_carry = side == 0 ? tile_offl[blockIdx.x] : tile_offr[blockIdx.x];
    __syncthreads();
    for (int base = 0; base < k1 - k0; base += BVH_BLOCK) {
      const int j = base + tid;
      const int k = side == 0 ? k0 + j : k1 - 1 - j; /* ascending for ml, descending for mr */
      bool mis = false;
      if (j < k1 - k0) {
        const bool left = bvh_goes_left(prim_box, order[lo + k], sp);
        mis = side == 0 ? (k < L && !left) : (k >= L && left);
      }
      const unsigned long long m = __ballot(mis);
      if (lane == 0) s_wave[wave] = (int)__popcll(m);
      __syncthreads();
      int before = s_carry;
      for (int w = 0; w < wave; ++w) before += s_wave[w];
      if (mis) (side == 0 ? ml : mr)[before + (int)__popcll(m & ((1ull << lane) - 1ull))] = k;
      __syncthreads();
      if (tid == 0) {
        int t = 0;
        for (int w = 0; w < BVH_BLOCK / 64; ++w) t += s_wave[w];
        s_carry += t;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(BVH_BLOCK) void k_big_swap(int* __restrict__ order, const int* __restrict__ scratch, int n_total,
                                                        const BvhBigSeg* __restrict__ big, const int2* __restrict__ tiles,
                                                        const BvhBigState* __restrict__ st) {
  const int2 tl = tiles[blockIdx.x];
  const BvhBigState& s = st[tl.x];
  if (!s.split.valid) return;
  const int lo = big[tl.x].seg.lo;
  const int* ml = scratch + lo;
  const int* mr = scratch + n_total + lo;
  const int q0 = tl.y * BVH_TILE, q1 = min(s.n_mis, q0 + BVH_TILE);
  for (int q = q0 + (int)threadIdx.x; q < q1; q += BVH_BLOCK) {
    const int a = lo + ml[q], b = lo + mr[q];
    const int t = order[a];
    order[a] = order[b];
    order[b] = t;
  }
}

/* ------------------------------------------------------------------ finalisation: pre-order numbering */
/* Temp node ids are handed out level by level (a level's children are allocated while it is processed), so level l
 * owns the contiguous id range [level_start[l], level_start[l + 1]).  sizes: bottom-up; indices: top-down. */
struct BvhFin {
  int n_nodes; /* subtree node count */
  int n_slots; /* subtree leaf slots (after padding) */
  int depth;   /* Shape_tree.depth: leaf = 0 */
  int index;   /* final (pre-order) index */
  int slot0;   /* first leaf slot of the subtree */
  int n_leaves;
};
__global__ void k_fin_sizes(const BvhTmpNode* __restrict__ nodes, BvhFin* __restrict__ fin, int first, int count, int pad4) {
  const int i = first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= first + count) return;
  const BvhTmpNode& t = nodes[i];
  BvhFin f;
  f.index = 0;
  f.slot0 = 0;
  if (t.leaf) {
    const int cnt = t.hi - t.lo;
    f.n_nodes = 1;
    f.n_slots = pad4 ? ((cnt + 3) & ~3) : cnt;
    f.depth = 0;
    f.n_leaves = 1;
  } else {
    const BvhFin a = fin[t.lhs], b = fin[t.rhs];
    f.n_nodes = 1 + a.n_nodes + b.n_nodes;
    f.n_slots = a.n_slots + b.n_slots;
    f.depth = 1 + (a.depth > b.depth ? a.depth : b.depth);
    f.n_leaves = a.n_leaves + b.n_leaves;
  }
  fin[i] = f;
}
__global__ void k_fin_index(const BvhTmpNode* __restrict__ nodes, BvhFin* __restrict__ fin, int first, int count) {
  const int i = first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= first + count) return;
  const BvhTmpNode& t = nodes[i];
  if (t.leaf) return;
  const int me = fin[i].index, s0 = fin[i].slot0;
  fin[t.lhs].index = me + 1;
  fin[t.lhs].slot0 = s0;
  fin[t.rhs].index = me + 1 + fin[t.lhs].n_nodes;
  fin[t.rhs].slot0 = s0 + fin[t.lhs].n_slots;
}
/* one thread per temp node: writes the final PtNode and, for a leaf, its slots */
__global__ void k_fin_emit(const BvhTmpNode* __restrict__ nodes, const BvhFin* __restrict__ fin, int n_nodes,
                           const int* __restrict__ order, PtNode* __restrict__ out_nodes, int* __restrict__ slot_prim) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n_nodes) return;
  const BvhTmpNode& t = nodes[i];
  const BvhFin f = fin[i];
  PtNode nd;
  for (int k = 0; k < 3; ++k) {
    nd.mn[k] = t.box[k];
    nd.mx[k] = t.box[k + 3];
  }
  nd.pad[0] = 0;
  nd.pad[1] = 0;
  if (t.leaf) {
    const int cnt = t.hi - t.lo;
    nd.a = (uint32_t)f.slot0;
    nd.b = (uint32_t)f.n_slots | (PT_NODE_LEAF_AXIS << 30);
    nd.pad[0] = (uint32_t)cnt; /* real elements: the NaN padding slots can never be selected */
    for (int k = 0; k < f.n_slots; ++k) slot_prim[f.slot0 + k] = k < cnt ? order[t.lo + k] : -1;
  } else {
    nd.a = (uint32_t)fin[t.lhs].index;
    nd.b = (uint32_t)fin[t.rhs].index | ((uint32_t)t.axis << 30);
  }
  out_nodes[f.index] = nd;
}

/* Tree root box (shape_tree.ml:257-260): union of all element boxes -- min/max are exact in any order, except that a
 * bound that is +0.0 in one box and -0.0 in another comes out as -0.0 (minima) / +0.0 (maxima) here and as the LAST
 * of them in the reference (see the head of this file).  Only the photon map comes this way. */
__global__ __launch_bounds__(BVH_BLOCK) void k_bvh_root_box(const double* __restrict__ prim_box, int n,
                                                            unsigned long long* __restrict__ enc /* 6, initialised */) {
  unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
  for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < n; k += (int)(gridDim.x * blockDim.x)) {
    const double* b = prim_box + (size_t)k * 6;
    for (int a = 0; a < 3; ++a) {
      const unsigned long long e0 = bvh_enc(b[a]), e1 = bvh_enc(b[a + 3]);
      mn[a] = e0 < mn[a] ? e0 : mn[a];
      mx[a] = e1 > mx[a] ? e1 : mx[a];
    }
  }
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o1 = __shfl_xor(mn[a], off, 64), o2 = __shfl_xor(mx[a], off, 64);
      mn[a] = o1 < mn[a] ? o1 : mn[a];
      mx[a] = o2 > mx[a] ? o2 : mx[a];
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&enc[a], mn[a]);
      atomicMax(&enc[a + 3], mx[a]);
    }
  }
}
__global__ void k_bvh_iota(int* __restrict__ order, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) order[i] = i;
}
__global__ void k_bvh_root_seg(const unsigned long long* __restrict__ enc, int n, BvhSeg* __restrict__ seg) {
  BvhSeg s;
  s.lo = 0; s.hi = n; s.node = 0; s.pad = 0;
  for (int k = 0; k < 6; ++k) s.box[k] = bvh_dec(enc[k]);
  *seg = s;
}
