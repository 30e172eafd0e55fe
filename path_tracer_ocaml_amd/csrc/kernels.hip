/* kernels.hip -- the wavefront path integrator for gfx950 (MI355X), binary64 throughout.
 *
 * Stages (one kernel each, connected by path queues -- a 48-byte ray record + a 32-byte path-state record per entry -- that stay
 * resident in HBM):
 *   generate : sampler dims 0,1 + Camera.ray            (integrator.ml:96-105, camera.ml:93-102); fused into the bounce-0
 *              launches of trace and shade (PRIMARY), a kernel of its own only for explicit sample lists
 *   trace    : Scene.intersect = ordered BVH walk + leaf packets (shape_tree.ml:198-220, lib.rs:102-178,
 *              sphere.ml:35-54, triangle.ml:74-98, ganesha floor pre-test main.ml:286-298)
 *   shade    : Sphere.hit / Triangle.Hit.to_hit, Material.scatter, the body of Integrator's path loop
 *              (integrator.ml:30-66), background on a miss; survivors are compacted into the next queue
 *   accum    : per-pixel radiance sums in pass order
 *   film     : 3x3 binomial reconstruction + gamma (filter_kernel.ml, film_tile.ml, integrator.ml:114-128,152-154)
 * A render runs trace + shade of a bounce as ONE kernel (k_bounce: a wave walks 64 rays, files them in per-category pools, shades
 * a pool when it holds 64) -- around an LDS copy of the scene where tree and packets fit one, over the per-octant node image in
 * HBM / L2 otherwise; k_trace + k_shade_pool remain for what k_bounce does not cover (ptx_intersect_rays, scenes too large for
 * LDS beside the pools, PTX_FUSED = 0).  LDS-resident scenes binned by elevation run its steps in the other order (k_bounce_carry:
 * an entry carries its hit; a launch shades its input first and walks the new rays second, nothing is gathered or read twice).
 * Both walks are stackless and their links TAGGED: a visit ends with one select between "what a hit leads to" and "what a miss leads
 * to", and the walk's control state -- wants a node, holds a leaf, over -- lives in the link's spare bits (PT_SWZ_TAG_* on the LDS
 * image, the top two bits of a word on the per-octant record).  On Simd_leaf scenes in LDS the node loop itself is gfx950 assembly
 * (PtTraverser::walk_asm); everything else is HIP C++.  What lies where in a kernel's dynamic LDS buffer -- stacks, the scene image,
 * pools, parked walks -- and which scenes get an LDS copy at all is stated once, in pt_lds_layout.h, for these kernels and the host.
 *
 * Compiled with -ffp-contract=off; every fused multiply-add below is written out exactly where the
 * reference writes Float.fma / _mm256_fmadd_pd.  No MFMA: there is no dense contraction on this path.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pt_lds_layout.h"
#include "pt_scene.h"
#include "pt_vec.h"
#include "pt_tile_scan.h"

#define PT_WAVE 64

/* ------------------------------------------------------------------ path queue (records in HBM) */
/* A queue entry is two records: the ray (what k_trace reads, densely) and the rest of the path's state (what only the shade
 * stage reads, entry by entry in the order its category pools dictate -- one 32-byte sector instead of five 8-byte fields in
 * five different sectors).  Both are multiples of 16 bytes: every access is a 16-byte load or store. */
struct PtRayRec { double ox, oy, oz, dx, dy, dz; };                  /* 48 B: ray origin, direction (padded to one 64-byte line
                                                                         per ray: shade +20 % -- partial-line writes) */
struct PtPathRec { double ar, ag, ab; uint32_t id; int32_t offset; }; /* 32 B: attn0 (integrator.ml:30); slot in the batch's
                                                                         contribution buffer; sampler offset = gy*W + gx + pass*spp
                                                                         (integrator.ml:98) */
struct PtEmitRec { double er, eg, eb, pad; };                         /* 32 B: emit0; scenes with emitters only */
/* Scenes with emitters keep an entry's path state and its carried emission in ONE 64-byte line: `path` then holds
 * {PtPathRec, PtEmitRec} pairs (entry i at path + 2 i).  The shade stage gathers an entry's records sparsely and memory moves
 * 64-byte lines: two 32-byte records in two arrays cost two lines per segment (cornell: 315 B fetched per segment against 144
 * of records), the pair costs one. */
struct PtQueue {
  PtRayRec* ray;
  PtPathRec* path;
  uint32_t* count; /* number of live entries (device) */
};

struct PtHits {
  double* t;     /* scenes without triangles: t_hit per entry */
  int32_t* slot; /* leaf slot index, -1 = miss; >= n_slots = floor triangle */
  /* scenes with triangles: ONE 32-byte record {t_hit, u, v, -} per entry (triangle barycentrics, triangle.ml:14-20), `t` is
   * then unused (NULL).  Round 4: only ptx_intersect_rays asks for these records (tuv != NULL).  A render does not keep them
   * at all: the shade step RECOMPUTES (t, u, v) from the ray and the one primitive that was hit (PT_RECOMPUTE_HIT) -- the
   * same function on the same operands, so the same bits -- because the record cost a 32-byte write per segment and, gathered
   * again one or two chunks later when the L2 no longer holds it, a whole 128-byte line of fabric traffic per segment
   * (cornell's bounce launches, TCC counters: 2.7 line requests per segment reach the L2, 2.4 miss): ~60 vector instructions
   * against a third of the kernel's memory traffic. */
  double4* tuv;
  /* k_bounce running the remaining bounces of a batch in one launch (PtSolo): its workgroups are at DIFFERENT bounces at the same
   * time, and entry i of the even queue and entry i of the odd queue would share t[i] -- bounce b keeps its distances at
   * t + (b & 1) * t_parity_stride there (0: `t` holds one array only and no launch runs solo). */
  size_t t_parity_stride;
};
__device__ __forceinline__ void pt_hit_store(const PtHits& hits, uint32_t i, double t, int slot, double u, double v, bool with_uv) {
  hits.slot[i] = slot;
  if (with_uv) {
    if (hits.tuv) hits.tuv[i] = make_double4(t, u, v, 0.0);
  } else hits.t[i] = t;
}

/* A queue written by k_shade_pool has HOLES (unused entries of its last blocks): direction x = a NaN whose payload no
 * arithmetic produces.  k_trace skips a hole and records PT_SLOT_HOLE for it. */
#define PT_HOLE_HI 0x7ff8dead
#define PT_SLOT_HOLE (-2)
__device__ __forceinline__ bool pt_is_hole(double dx) { return __double2hiint(dx) == (int)PT_HOLE_HI; }

__device__ __forceinline__ void pt_q_load_ray(const PtQueue& q, uint32_t i, V3& o, V3& d) {
  const double2* r = (const double2*)(q.ray + i);
  const double2 a = r[0], b = r[1], c = r[2];
  o = v3(a.x, a.y, b.x);
  d = v3(b.y, c.x, c.y);
}
template <bool EMIT>
__device__ __forceinline__ void pt_q_load_path(const PtQueue& q, uint32_t i, V3& attn, uint32_t& id, int& offset, V3& emit) {
  const double2* r = (const double2*)(q.path + (EMIT ? 2 * (size_t)i : (size_t)i));
  const double2 a = r[0], b = r[1];
  attn = v3(a.x, a.y, b.x);
  id = (uint32_t)__double2loint(b.y);
  offset = __double2hiint(b.y);
  if (EMIT) {
    const double2 c = r[2], e = r[3];
    emit = v3(c.x, c.y, e.x);
  }
}
__device__ __forceinline__ void pt_q_store_ray(const PtQueue& q, uint32_t i, V3 o, V3 d) {
  /* a real ray's NaN that happens to carry the hole payload (it can only come in through the caller's data: arithmetic
   * produces the canonical NaN or hands an operand's payload on) is stored as the canonical NaN: any NaN walks alike */
  if (pt_is_hole(d.x)) d.x = __hiloint2double(0x7ff80000, 0);
  double2* r = (double2*)(q.ray + i);
  r[0] = make_double2(o.x, o.y);
  r[1] = make_double2(o.z, d.x);
  r[2] = make_double2(d.y, d.z);
}
template <bool EMIT>
__device__ __forceinline__ void pt_q_store(const PtQueue& q, uint32_t i, V3 o, V3 d, V3 attn, V3 emit, uint32_t id, int offset) {
  pt_q_store_ray(q, i, o, d);
  double2* r = (double2*)(q.path + (EMIT ? 2 * (size_t)i : (size_t)i));
  r[0] = make_double2(attn.x, attn.y);
  r[1] = make_double2(attn.z, __hiloint2double(offset, (int)id));
  if (EMIT) {
    r[2] = make_double2(emit.x, emit.y);
    r[3] = make_double2(emit.z, 0.0);
  }
}

struct PtCounters { /* device-side work counters (count_work) */
  unsigned long long segments, nodes, prims, floor;
  unsigned long long undecided, fallback_steps; /* binary32 filter: lane tests handed to the binary64 code, wave steps that ran it */
  unsigned long long solo;                      /* k_bounce launches that ran their batch's remaining bounces by themselves (PtSolo) */
  unsigned long long carry;                     /* k_bounce_carry launches */
  unsigned long long lane_walks;                /* camera launches of k_bounce / k_bounce_carry that walked one ray per lane (LANE_WALK) */
  unsigned long long tile_fallbacks;            /* k_bounce_carry<..., TILE>: chunks of camera rays a guard of the list scan sent back to the walk (non-counting renders) */
};

/* ------------------------------------------------------------------ small device helpers */
__device__ __forceinline__ int pt_lane() { return (int)(threadIdx.x & 63); }

/* popcount of a wave mask as a 32-bit scalar: `(int)__popcll(m) < K` is turned into a 64-bit comparison, for which the scalar
 * unit has no instruction -- it lands on the VECTOR pipe, once per turn of the walk */
__device__ __forceinline__ int pt_popc_mask(unsigned long long m) { return __builtin_popcount((unsigned)m) + __builtin_popcount((unsigned)(m >> 32)); }

/* wave-aggregated append: returns the destination index for lanes with keep != 0 */
__device__ __forceinline__ uint32_t pt_wave_append(uint32_t* counter, bool keep) {
  const unsigned long long mask = __ballot(keep);
  const uint32_t total = (uint32_t)__popcll(mask);
  uint32_t base = 0;
  const int lane = pt_lane();
  const int leader = mask ? (int)__ffsll((unsigned long long)mask) - 1 : 0;
  if (lane == leader && total) base = atomicAdd(counter, total);
  base = (uint32_t)__shfl((int)base, leader, 64);
  const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  return base + rank;
}

__device__ __forceinline__ unsigned long long pt_wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

/* Low_discrepancy_sequence.get (low_discrepancy_sequence.ml:19-20,33-36) */
__device__ __forceinline__ double pt_lds_get(const double* __restrict__ alpha, int offset, int dimension) {
  const double a = alpha[dimension];
  const double x = 0.5 + (a * (double)(1 + offset));
  return x - pt_trunc(x);
}

/* ------------------------------------------------------------------ generate */
struct PtGenParams {
  int32_t width, height;   /* full image */
  int32_t spp;
  int32_t local_rows;      /* rows this rank renders */
  int32_t band_rows, band_first, band_step;
  int32_t first_pass, n_pass; /* passes in this batch */
  int32_t tiles_x, tiles_y;   /* 8x8 pixel tiles over (width x local_rows) */
};

__device__ __forceinline__ int pt_global_row(const PtGenParams& g, int local_row) {
  if (g.band_step <= 1) return local_row;
  const int band_local = local_row / g.band_rows;
  const int within = local_row - band_local * g.band_rows;
  return (g.band_first + band_local * g.band_step) * g.band_rows + within;
}

/* Camera.ray (camera.ml:93-102): direction only; the origin is P3.origin */
__device__ __forceinline__ V3 pt_camera_dir(const PtSceneDev& sc, double cx, double cy) {
  return v3_normalize(v3(sc.cam_llx + (sc.cam_vx * cx), sc.cam_lly + (sc.cam_vy * cy), -1.0));
}

/* ------------------------------------------------------------------ trace */
/* Bbox.is_hit (bbox.ml:40-56) with Base's NaN-propagating min/max */
__device__ __forceinline__ bool pt_slab_hit(const PtNode& n, V3 o, V3 inv, double t_min, double t_max) {
  const double t0x = (n.mn[0] - o.x) * inv.x, t0y = (n.mn[1] - o.y) * inv.y, t0z = (n.mn[2] - o.z) * inv.z;
  const double t1x = (n.mx[0] - o.x) * inv.x, t1y = (n.mx[1] - o.y) * inv.y, t1z = (n.mx[2] - o.z) * inv.z;
  const double a = pt_base_max(pt_base_min(t0x, t1x), pt_base_max(pt_base_min(t0y, t1y), pt_base_min(t0z, t1z)));
  const double b = pt_base_min(pt_base_max(t0x, t1x), pt_base_min(pt_base_max(t0y, t1y), pt_base_max(t0z, t1z)));
  const double lo = pt_base_max(t_min, a);
  const double hi = pt_base_min(t_max, b);
  return lo <= hi;
}

/* Triangle.intersect (triangle.ml:74-98) */
__device__ __forceinline__ bool pt_triangle_intersect(V3 a, V3 b, V3 c, V3 o, V3 dir, double t_min, double t_max,
                                                      double* t_out, double* u_out, double* v_out) {
  const double epsilon = 1e-6;
  const V3 e1 = v3_sub(b, a);
  const V3 e2 = v3_sub(c, a);
  const V3 pvec = v3_cross(dir, e2);
  const double det = v3_dot(e1, pvec);
  if (pt_fabs(det) < epsilon) return false;
  const double det_inv = 1.0 / det;
  const V3 tvec = v3_sub(o, a);
  const double u = det_inv * v3_dot(tvec, pvec);
  const V3 qvec = v3_cross(tvec, e1);
  const double v = det_inv * v3_dot(dir, qvec);
  if (0.0 <= u && u <= 1.0 && 0.0 <= v && u + v <= 1.0) {
    const double t_hit = det_inv * v3_dot(e2, qvec);
    if (t_min <= t_hit && t_hit <= t_max) {
      *t_out = t_hit;
      *u_out = u;
      *v_out = v;
      return true;
    }
  }
  return false;
}

__device__ __forceinline__ V3 pt_load_v3(const double* p) { return v3(p[0], p[1], p[2]); }

/* Sphere.intersect, scalar (--no-simd / Array_leaf) form, sphere.ml:35-54 */
__device__ __forceinline__ bool pt_sphere_intersect_scalar(V3 center, double radius, V3 o, V3 d, double t_min,
                                                           double t_max, double* t_out) {
  const double r2 = radius * radius;
  const V3 f = v3_sub(center, o);
  const double bp = v3_dot(f, d);
  const double a = v3_quadrance(d);
  const double discrim = r2 - v3_quadrance(v3_sub(v3_scale(d, bp / a), f));
  if (discrim < 0.0) return false;
  const double sign_bp = (bp >= 0.0) ? 1.0 : -1.0;
  const double q = pt_fma(sign_bp, pt_sqrt(a * discrim), bp);
  const double c = v3_quadrance(f) - r2;
  const double t_hit = (c > 0.0) ? c / q : q / a;
  if (t_min <= t_hit && t_hit <= t_max) {
    *t_out = t_hit;
    return true;
  }
  return false;
}

/* Decodes entry i of a PRIMARY (bounce 0) launch: the queue is virtual -- entry i IS sample
 * (pass_in_batch, tile, lane) -- so camera rays are never written to or read from HBM. */
struct PtPrimarySample {
  int x, y, gy, pass_in_batch, offset;
  uint32_t id;
  bool valid;
};
__device__ __forceinline__ PtPrimarySample pt_primary_decode(const PtGenParams& g, uint32_t i) {
  PtPrimarySample s;
  const uint32_t per_pass = (uint32_t)(g.tiles_x * g.tiles_y) * 64u;
  const uint32_t pass_in_batch = i / per_pass;
  const uint32_t rem = i - pass_in_batch * per_pass;
  const int tile = (int)(rem >> 6), lane = (int)(rem & 63);
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  s.x = tx * 8 + (lane & 7);
  s.y = ty * 8 + (lane >> 3);
  s.pass_in_batch = (int)pass_in_batch;
  s.valid = (int)pass_in_batch < g.n_pass && s.x < g.width && s.y < g.local_rows;
  s.gy = pt_global_row(g, s.y);
  s.offset = (s.gy * g.width) + s.x + ((g.first_pass + (int)pass_in_batch) * g.spp); /* integrator.ml:98 */
  s.id = (uint32_t)((long long)pass_in_batch * g.width * g.local_rows + (long long)s.y * g.width + s.x);
  return s;
}

/* camera rays written into a queue: the film coordinates, the camera kinds and the three generators */
#include "camera_rays.inc"

/* render_tile (integrator.ml:98-105) + Camera.ray (camera.ml:93-102) */
__device__ __forceinline__ V3 pt_primary_dir(const PtSceneDev& sc, const PtGenParams& g, const PtPrimarySample& s,
                                             const double* __restrict__ alpha) {
  double cx, cy;
  pt_film_coords(alpha, s.x, s.gy, g.width, g.height, s.offset, &cx, &cy);
  return pt_camera_dir(sc, cx, cy);
}

/* Bbox.is_hit when no 0 * inf can occur (every 1/d component finite): no NaN is ever produced, so Base's
 * NaN-propagating min/max coincide with the hardware v_min_f64 / v_max_f64 -- same boolean, 4x fewer
 * instructions.  (The values may differ in the sign of a zero, which no comparison can see.) */
template <bool ORIGIN_ZERO>
__device__ __forceinline__ bool pt_slab_hit_fast(const double* nb, V3 o, V3 inv, double t_min, double t_max) {
  /* camera rays start at P3.origin = (+0, +0, +0): x - (+0.0) == x bit for bit (also for x = -0.0), so the six
   * subtractions can be dropped for them */
  const double t0x = (ORIGIN_ZERO ? nb[0] : nb[0] - o.x) * inv.x, t0y = (ORIGIN_ZERO ? nb[1] : nb[1] - o.y) * inv.y,
               t0z = (ORIGIN_ZERO ? nb[2] : nb[2] - o.z) * inv.z;
  const double t1x = (ORIGIN_ZERO ? nb[3] : nb[3] - o.x) * inv.x, t1y = (ORIGIN_ZERO ? nb[4] : nb[4] - o.y) * inv.y,
               t1z = (ORIGIN_ZERO ? nb[5] : nb[5] - o.z) * inv.z;
  const double a = __builtin_fmax(__builtin_fmin(t0x, t1x), __builtin_fmax(__builtin_fmin(t0y, t1y), __builtin_fmin(t0z, t1z)));
  const double b = __builtin_fmin(__builtin_fmax(t0x, t1x), __builtin_fmin(__builtin_fmax(t0y, t1y), __builtin_fmax(t0z, t1z)));
  return __builtin_fmax(t_min, a) <= __builtin_fmin(t_max, b);
}
__device__ __forceinline__ bool pt_slab_hit_exact(const double* nb, V3 o, V3 inv, double t_min, double t_max) {
  PtNode n;
  n.mn[0] = nb[0]; n.mn[1] = nb[1]; n.mn[2] = nb[2];
  n.mx[0] = nb[3]; n.mx[1] = nb[4]; n.mx[2] = nb[5];
  return pt_slab_hit(n, o, inv, t_min, t_max);
}

/* LDS image of a node for LDS-resident scenes: 48 bytes -- a binary32 FILTER in front of the binary64 slab test, and the
 * tree THREADED per direction octant so that the walk needs no stack.
 *   words 0..5  mn.x mn.y mn.z mx.x mx.y mx.z rounded to binary32
 *   word 6      branch: lhs | rhs << 16 (node BYTE offsets into this image);  leaf: first slot | real slot count << 16
 *   word 7      bits of `mag` = max |bound| of the node (binary32, rounded up), low 2 bits replaced by the axis (3 = leaf)
 *   words 8..11 skip[8], u16 each: for a ray whose direction signs are octant o (shape_tree.ml:201), the node the
 *               reference's recursion visits next once this node's subtree is done (box missed, leaf taken, or both
 *               children searched) = the far sibling of the nearest ancestor entered through its near child; 0xffff = none.
 *               Same visiting order as the recursion (near subtree completely, then the far child, tested on arrival against
 *               the closest hit so far: shape_tree.ml:209-216), hence the same tests and counters, but no push, no pop, no
 *               stack pointer and no per-lane stack in LDS: ~12 fewer vector instructions and 1 LDS access less per visit.
 * Bbox.is_hit (bbox.ml:40-56) is a boolean of binary64 quantities; the image decides it in binary32 with a rigorous
 * error bound and hands the (rare) undecided lanes to the binary64 code, so the boolean -- and with it every hit, every
 * work counter and every pixel -- is the reference's.  For a ray with (root_mag + max|o|) max|1/d| < 2^100 and
 * max|1/d| > 2^-60 (else: always binary64):
 *   t~ = fma32(bound32, inv32, -(o * inv)32) differs from the reference's fl64((bound - o) * inv) by at most
 *        3.2 * 2^-24 * (|bound| + |o|) * |inv|  <=  M := 3.2 * 2^-24 * (mag + max|o|) * max|inv|
 *   (three binary32 roundings of the inputs, one of the fma, the reference's own two binary64 roundings; as built,
 *   with inv32 and (o inv)32 computed in binary32 from the start: 6 instead of 3.2, see PtTraverser::begin);
 *   max / min are 1-Lipschitz, so lo~ = max(0, a~) and hi~ = min(b~, t32) are within M (+ 2^-24 t for the rounded
 *   closest-hit distance) of the reference's lo, hi, and u = hi~ - lo~ (one more rounding) within 8.4 * 2^-24 * (..)
 *   + 2^-24 t of hi - lo.  With m2 = 2^-19 * (mag + max|o|) * max|inv| + 2^-21 * t32  (twice that bound):
 *        u >= m2  =>  lo <= hi (hit)        u <= -m2  =>  lo > hi (miss)        otherwise (|u| < m2 or unordered): binary64.
 * The undecided share is ~4 m2 / (hi - lo spread) ~ 1e-5 per test, scale-free because mag is the node's own. */
/* Layout 3 (layouts 1 and 2 -- 48-byte nodes, 64-byte nodes with the near-child table -- were its A/B partners and are gone from
 * the source).  The vector pipe is what the walk is bound by, so the image is arranged to take instructions out of a
 * visit:
 *   bytes  0..35  per axis a: mn_a, mx_a, mn_a (binary32).  A ray reads the PAIR at 12 a + (d_a >= 0 ? 0 : 4): (near, far)
 *                 bound of that axis for its direction sign, so t_near = fma(near, inv, n), t_far = fma(far, inv, n) need no
 *                 min / max per axis (an fma with a fixed second and third operand is monotone in the first, so these are
 *                 bit for bit the min and max the unselected form computes): 4 min / max per visit instead of 10
 *   bytes 36..39  word 6 as before: branch lhs | rhs << 16, leaf first slot | real count << 16
 *   bytes 40..43  word 7 as before: mag | axis
 *   bytes 44..59  skip[8] u16          bytes 60..75  near[8] u16          bytes 76..83  unused (see PT_SWZ_NODE_BYTES)
 * and every node reference (lhs, rhs, skip, near, the walk's `node`) is the node's ABSOLUTE LDS byte address, so a visit
 * starts reading at `node` itself (PT_SWZ_END / PT_SWZ_LEAF stay out of range: the image ends below 0xfffe). */
/* (PT_SWZ_NODE_BYTES of this layout: pt_scene.h) */
#define PT_SWZ_OFF_LINKS 36
#define PT_SWZ_OFF_SKIP 44
#define PT_SWZ_OFF_NEAR 60
typedef const __attribute__((address_space(3))) unsigned char* PtLdsPtr;
/* native vectors (HIP's float2 class cannot be read through an address-space-qualified pointer), 4-byte aligned: the pairs
 * start at 12 a + {0, 4} */
typedef float pt_f2 __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned int pt_u2 __attribute__((ext_vector_type(2), aligned(4)));
#define PT_LDS_AT(addr) ((PtLdsPtr)(uintptr_t)(uint32_t)(addr))
#define PT_SWZ_LEAF 0xfffeu
/* Layout 3: TAGGED links (round 5).  Node addresses are multiples of 4, so the two low bits of a 16-bit link are free:
 *   tag 0  a node to visit                       tag 1  "this lane holds a leaf; afterwards continue at link & ~3"
 *   tag 2  PT_SWZ_END: the walk is over          tag 3  "holds a leaf; afterwards the walk is over" (PT_SWZ_END | 1)
 * A leaf's near[o] entry is its skip[o] entry with bit 0 set, so a visit ends with ONE select, `node = hit ? near[o] : skip[o]`,
 * and the walk's whole control state is that register: wants a node step <=> (node & 3) == 0, holds a leaf <=> node & 1,
 * finished <=> node == PT_SWZ_END.  The leaf's (first slot, real count) word stays in the register the visit loaded it into
 * (`lkx`) until the leaf phase decodes it.  Before: a leaf compare, two conditional updates of (leaf_first, leaf_n), the END
 * compare, the conditional update of `node` and the (walking > leaf_n) compare -- 9 of a visit's 27 vector instructions. */
#define PT_SWZ_TAG_LEAF 1u
#define PT_SWZ_TAG_END 2u
#define PT_SWZ_END 0xfffeu /* tag 2 (see PT_SWZ_TAG_*) */
/* (A sphere slot is 4 doubles, {x, y, z, r}, in the LDS copy as in global memory: padding it to 6 -- a slot then starts in 16 of the
 * 64 banks instead of 8 -- was measured, no gain: profiles/r05_ab_sphere_stride.txt.) */
/* (what lies where in the dynamic LDS buffer -- the per-wave stacks, the scene image, pools, parked walks: pt_lds_layout.h) */

/* where the traversal data of this launch lives: HBM/L2 (large scenes) or an LDS copy (small scenes) */
/* StackT of a walk that needs no stack: scenes traversed from HBM / L2 follow per-octant skip links like the LDS image
 * does (PtSceneDev.node_skip32), which frees the LDS the per-lane stacks took (depth x 256 bytes per wave: it capped
 * the ganesha-like scene at 3 waves per SIMD where its registers allow 4) */
struct PtThreadTag {};
/* ... and the same walk on the PER-OCTANT node image (PtSceneDev.nodes32o): one 32-byte record per (direction octant, node) that
 * carries the six binary32 bounds, ONE link word and the skip link of that octant -- a visit is two 16-byte loads instead of
 * two + the skip table's entry.  The texture-address unit that binds the walk from HBM / L2 works per load instruction and
 * lane (profiles/r03c_ganesha_ta_tcp.txt: three per node test); the price is eight copies of the bounds (23 MB for 92 k nodes
 * instead of 6 MB of image + table).  A pre-order tree needs no lhs link (the lhs child of node k is k + 1), which is what
 * frees the word: inner nodes keep `rhs | axis << 30`, leaves pack `tag << 30 | real slots << 22 | first slot`. */
struct PtThreadOctTag {};
/* ... and the LDS walk on ITS per-octant image (PtSceneDev.lds_oct, PT_LOCT_* in pt_scene.h; non-counting k_bounce_carry launches of
 * Simd_leaf scenes that fit with it, pt_lds_oct_layout): what the per-octant record did for the walk from HBM / L2, for the loop every
 * segment of the headline goes through.  The shared LDS record serves all eight octants with per-lane offsets: four address adds, two
 * 16-bit link reads, three 8-byte bound reads and the link pair per visit.  Here a visit is ONE address (record number << 5 beside the
 * image's LDS address), two 16-byte reads, and a select that takes the hit or the miss half of word 6; "wants a node" is one unsigned
 * comparison (link < PT_LOCT_LEAF_TAG).  A leaf's hit link is its own record under PT_LOCT_LEAF_TAG: the leaf phase reads the
 * leaf table's word (first slot | real slots << 16) and goes on at the record's miss link -- two reads per leaf held, 2.3 leaves
 * a ray against 21 visits.  Same bounds (rounded the same way), same magnitude word, same margin, same binary64 fallback: the
 * undecided visit is performed in C++ (node_step) on binary64 node `record - octant * n_nodes`. */
struct PtLdsOctTag {};
typedef unsigned int pt_u4 __attribute__((ext_vector_type(4)));
/* Round 5, second layout of the per-octant record: what the tagged links did for the LDS image, for the walk from
 * HBM / L2 -- where four fifths of the visits are answered by the L1 in ~120 clocks and the ~45 vector + ~40 scalar instructions
 * the old record cost per visit were as long a chain as the load.  An octant fixes the sign of every direction component, so
 *   words 0..2  the NEAR bound of each axis for this octant (mn where the direction component is >= 0, else mx), words 3..5 the
 *               FAR one: t_near = fma(near, inv, n), t_far = fma(far, inv, n) -- the six min / max per visit are gone (an fma with
 *               fixed second and third operand is monotone in the first: the same bits);
 *   word 6      what a HIT leads to: an inner node -> its near child for this octant (an index < 2^30: tag 00 in the top bits);
 *               a leaf -> 01 << 30 | real slots << 22 | first slot: "this lane holds a leaf", the leaf's packet in the same word;
 *   word 7      what a MISS -- or the end of the leaf -- leads to: the octant's skip link, or PT_OCT_END (1 << 31: nothing).
 * A visit ends with one select, node = hit ? word 6 : word 7, and the walk's control state is that register: wants a node step
 * <=> node < 2^30, holds a leaf <=> node >> 30 == 1, over <=> node >= 2^31; after the leaf phase the walk continues at the word 7
 * the leaf's visit loaded (oct_skip).  The node's magnitude for the filter's margin comes from the bounds themselves (three
 * v_max3 with |.| modifiers); its 1.000001 lives in the ray's k2. */
/* (The record of round 4 -- six bounds as stored, `rhs | axis << 30` / packed leaf word, skip link -- and the first tagged record with
 * un-offset links were this layout's A/B partners: profiles/r05_ab_oct_tagged.txt, r05_ab_oct_preoffset.txt; removed from the source
 * once measured; commit afabea1 is the last whose source holds both alternates.) */
#ifndef PT_FILTER_DEBUG
#define PT_FILTER_DEBUG 0 /* diagnostic builds only (tools/filter_error_study.py): the traverser keeps the u and the margin of its last box test on the
                             per-octant record, and the library gains ptx_debug_filter_error -- not in the product build */
#endif
/* Links are PRE-OFFSET: the links of octant o's records are record numbers in the whole image (o * n_nodes + k) and so is the walk's
 * `node`: a visit's address is one 32-bit shift beside the image's scalar base (the image is smaller than 4 GiB: the host builds it
 * only then) instead of add, 64-bit shift, 64-bit add at the head of its chain; the binary64 fallback subtracts the octant's base. */
#ifndef PT_OCT_BATCH_FALLBACK
#define PT_OCT_BATCH_FALLBACK 1 /* (0: evaluated there and then, as until round 5's last change) a lane whose box test the binary32 filter leaves undecided does not stop its
                                   wave for the ~100 instructions of the binary64 test there and then (22 % of the mesh's wave steps did, for a handful of
                                   lanes): it leaves the node loop like a lane that holds a leaf, its node tagged PT_OCT_PENDING, and all such lanes take
                                   the binary64 test TOGETHER after the loop (resolve_pending), before the leaf phase.  Same tests per ray, same order */
#endif
#define PT_OCT_PENDING 0xc0000000u /* top bits 11: "the test of node (low 30 bits) awaits its binary64 evaluation"; oct_link / oct_skip hold its links */
/* (PT_OCT_LEAF_FIRST_BITS, PT_OCT_LEAF_REAL_MAX, PT_OCT_END, PT_OCT_LEAF_TAG: pt_scene.h, the host builds the image) */

struct PtSceneView {
  const PtNode* nodes;
  const uint32_t* skip32; /* threaded global walk: n_nodes x 8, 0xffffffff = none */
  const unsigned char* nodes32; /* 32-byte binary32 image of the nodes for the walk from HBM / L2 */
  const unsigned char* nodes32o; /* ... per direction octant (PtThreadOctTag), 8 x n_nodes x 32 bytes, or null */
  uint32_t n_nodes;
  const unsigned char* swz_nodes; /* LDS-resident scenes: the binary32 filter image, PT_SWZ_NODE_BYTES per node */
  uint32_t swz_root;              /* what the walk's `node` is for node 0: the image's absolute LDS address (node references are
                                     absolute LDS addresses) */
  const unsigned char* top;       /* scenes walked from HBM / L2: the LDS copy of PtSceneDev.top_nodes if has_top (else never dereferenced:
                                     no node reference carries PT_TOP_FLAG) */
  bool has_top;
  const double* sph;
  const double* tri;
  const uint8_t* kind;
  const double* nodes64; /* LDS-resident scenes with PtSceneDev.lds_nodes64: six binary64 bounds per node in LDS, else null */
  uint32_t oct_base, oct_leaf; /* PtLdsOctTag: the LDS addresses of the per-octant image's records and of its leaf table */
  const uint8_t* cat; /* the slots' shading categories: the LDS copy on LDS-resident scenes (k_bounce files a finished ray by it right
                         after the walk: from global memory that one byte was a ~1 us round trip in every chunk's chain) */
  /* scenes walked from HBM / L2: the first n_floor_lds floor triangles (ganesha's Floor, tested before the tree for EVERY ray,
   * main.ml:247-256) as 10-double records in LDS.  Read from global memory their 2 x 5 loads per ray were a fifth of the
   * walk's vector-memory instructions -- all lanes at the same address, but the texture-address unit that binds this kernel
   * still processes every one of them; an LDS read of one address is a broadcast on a pipe the kernel does not use. */
  const __attribute__((address_space(3))) double* floor_lds;
  int n_floor_lds;
};
#define PT_FLOOR_LDS 4

struct PtTraceResult {
  double t, u, v;
  int slot;
};

/* Scene.intersect for ONE ray held by this lane.  The traversal stack (far children only) lives in LDS,
 * one column per lane (conflict-free ds_write_b32 / ds_read_b32).  A far child's bbox is tested when it
 * is POPPED, against the closest hit so far -- exactly the t_max the reference's recursion passes
 * (shape_tree.ml:210-216). */
template <class T> __device__ __forceinline__ void pt_stack_push(T* stk, int sp, uint32_t val) { stk[sp * PT_WAVE] = (T)val; }
template <class T> __device__ __forceinline__ uint32_t pt_stack_pop(const T* stk, int sp) { return (uint32_t)stk[sp * PT_WAVE]; }
__device__ __forceinline__ void pt_stack_push(PtThreadTag*, int, uint32_t) {}
__device__ __forceinline__ uint32_t pt_stack_pop(const PtThreadTag*, int) { return 0u; }
__device__ __forceinline__ void pt_stack_push(PtThreadOctTag*, int, uint32_t) {}
__device__ __forceinline__ uint32_t pt_stack_pop(const PtThreadOctTag*, int) { return 0u; }
__device__ __forceinline__ void pt_stack_push(PtLdsOctTag*, int, uint32_t) {}
__device__ __forceinline__ uint32_t pt_stack_pop(const PtLdsOctTag*, int) { return 0u; }
#define PT_STACK_PUSH(stk, sp, val) pt_stack_push((stk), (sp), (uint32_t)(val))
#define PT_STACK_POP(stk, sp) pt_stack_pop((stk), (sp))

#ifndef PT_WALK_MIN
#define PT_WALK_MIN 8
#endif
#ifndef PT_WALK_MIN_GLOBAL
#define PT_WALK_MIN_GLOBAL 16 /* the same threshold for the walk from HBM / L2, where a node step is a round trip to the L2 and the leaf phase's
                                 first loads are the longest waits of the walk: leaves are taken up sooner (ganesha-like frame 4: 28.1, 8: 26.4, 16: 25.8 ms) */
#endif
#ifndef PT_MARGIN_K2
#define PT_MARGIN_K2 0x1.000002p-19f /* the filter's margin m2 = PT_MARGIN_K2 (mag + max|o|) max|1/d| + PT_MARGIN_T t (header comment) */
#define PT_MARGIN_T 0x1p-21f
#endif
/* PT_DIAG (diagnostic builds only, tools/diag_utilisation.sh): re-purposes the COUNT counters of SECONDARY launches
 * to measure lane utilisation per traversal phase: nodes = useful lane steps, floor = lane slots the wave spent.
 * 1: node walk   2: node walk if only the per-chunk tail were lost   3: packet scan   4: packet heavy part
 * 5 / 6 (k_bounce only, tools/diag_phases.py): a wave's life in 100 MHz ticks per phase -- walk / shade steps / rest, or walk / its leaf phases */
#ifndef PT_DIAG
#define PT_DIAG 0
#endif
#ifndef PT_DIAG_EXTRA_LOADS
#define PT_DIAG_EXTRA_LOADS 0
#endif
/* diagnostic builds only (tools/README.md, "what binds the node loop"): PT_DIAG_VISIT_VALU = n more vector instructions per
 * visit of the LDS walk, PT_DIAG_VISIT_LDS = n more 16-bit LDS reads (+ one vector add each), PT_DIAG_VISIT_SALU = n more scalar ones */
#ifndef PT_DIAG_VISIT_VALU
#define PT_DIAG_VISIT_VALU 0
#endif
#ifndef PT_DIAG_VISIT_LDS
#define PT_DIAG_VISIT_LDS 0
#endif
#ifndef PT_DIAG_VISIT_SALU
#define PT_DIAG_VISIT_SALU 0
#endif
#ifndef PT_WALK_ASM
#define PT_WALK_ASM 1 /* k_bounce on LDS scenes: the node loop in assembly (PtTraverser::walk_asm); 0: the compiler's loop */
#endif
#define PT_DIAG_WAVE_SLOTS(c) do { if (pt_lane() == __ffsll((long long)__ballot(1)) - 1) (c) += 64; } while (0)

/* One ray's traversal state.  begin() = Ray.create + the per-ray constants; node_step() = one visit of
 * Tree.intersect's recursion (shape_tree.ml:203-221); packet() = Leaf.intersect on the leaf the lane holds.
 * Driven by pt_trace_ray (one ray per lane; a chunk may stop early and its unfinished walks be resumed later, PtTailCtl) and by
 * pt_trace_packet (camera rays of LDS-resident scenes). */
template <int MODE, bool COUNT, bool ORIGIN_ZERO, typename StackT, bool SWZ>
struct PtTraverser {
  /* the binary32 filter runs wherever the walk is threaded: on the LDS image (SWZ) and on the 32-byte global image */
  static constexpr bool OCT = !SWZ && std::is_same<StackT, PtThreadOctTag>::value; /* the per-octant image (PtThreadOctTag) */
  static constexpr bool G32 = !SWZ && (std::is_same<StackT, PtThreadTag>::value || OCT);
  static constexpr bool FILT = SWZ || G32;
  V3 o, d, inv; /* SWZ: inv is not kept (the binary64 fallback recomputes 1 / d, the same three divisions) */
  uint32_t dirs;
  bool exact_slab; /* SWZ: also set when the binary32 filter does not apply to this ray (|1/d| >= 2^100) */
  /* binary32 filter constants of the ray (SWZ only): inv32, -(o * inv)32, k2 = 2^-19 max|inv|, c2 = max|o| k2 + 2^-21 t32 */
  float fix, fiy, fiz, fnx, fny, fnz, k2, c2base, c2, t32;
  uint32_t skip_off; /* SWZ: byte offset of this ray's octant entry in a node's skip table; OCT: index of the octant's node 0 */
  mutable uint32_t oct_skip; /* OCT: the visited node's skip link, out of its record (test_box) */
  mutable uint32_t oct_link; /* OTAG: word 6 of the visited node's record (what a hit leads to) */
#if PT_FILTER_DEBUG
  mutable float dbg_u, dbg_m2; /* the binary32 filter's u = hi~ - lo~ and margin m2 of the last box test (OTAG branch) */
#endif
  uint32_t sel_x, sel_y, sel_z; /* SWZ: byte offsets of the ray's (near, far) bound pairs */
  mutable unsigned long long n_undecided = 0, n_wave_fallbacks = 0; /* COUNT only (ptx_stats.filter_*) */
  double qa, one_over_a;
  PtTraceResult r;
  int sp;
  /* TAGGED (the LDS image, layout 3): `node` carries the walk's control state in its two low bits (PT_SWZ_TAG_*), `walking` and
   * `leaf_n` are not used between the leaf phases; `lkx` = word 6 of the node visited last (a leaf's first slot | real count << 16) */
  static constexpr bool LOCT = SWZ && std::is_same<StackT, PtLdsOctTag>::value; /* the per-octant LDS image: `node` is a PT_LOCT_* link */
  static constexpr bool TAGGED = SWZ && !LOCT;
  static constexpr bool OTAG = OCT; /* the per-octant record: tagged, pre-offset links */
  static constexpr bool TAGS = TAGGED || OTAG || LOCT;
  uint32_t node;
  mutable uint32_t lkx;
  uint32_t lkx_diag = 0u, sdiag = 0u; /* (PT_DIAG_VISIT_*) */
  uint32_t walking; /* 0 / 1: an integer, so that "wants a node step" is ONE unsigned comparison (walking > leaf_n) */
  int leaf_first, leaf_n;
  __device__ __forceinline__ bool wants_node() const { return LOCT ? node < PT_LOCT_LEAF_TAG : OTAG ? node < PT_OCT_LEAF_TAG : (TAGGED ? (node & 3u) == 0u : walking > (uint32_t)leaf_n); }
  /* the same as a wave mask, straight from the comparison: the ballot builtin of the very expression the branch tests lets the
   * compiler use ONE v_cmp for both (HIP's __ballot of a boolean that is also branched on costs two more vector instructions
   * per turn; __builtin_amdgcn_uicmp a second compare); 38 = signed greater than, 33 = not equal */
  __device__ __forceinline__ unsigned long long wants_node_mask() const { return __builtin_amdgcn_ballot_w64(wants_node()); }
  __device__ __forceinline__ bool holds_leaf() const { return LOCT ? (node & PT_LOCT_LEAF_TAG) != 0u : OTAG ? (node >> 30) == 1u : (TAGGED ? (node & PT_SWZ_TAG_LEAF) != 0u : leaf_n > 0); }
  __device__ __forceinline__ unsigned long long holds_leaf_mask() const { return TAGS ? __builtin_amdgcn_ballot_w64(holds_leaf()) : __builtin_amdgcn_sicmp(leaf_n, 0, 38); }
  /* the ray's walk is not over (it wants a node step or holds a leaf) */
  __device__ __forceinline__ bool alive() const {
    if (LOCT) return node != PT_LOCT_END;
    return OTAG ? (PT_OCT_BATCH_FALLBACK ? (node & PT_OCT_PENDING) != PT_OCT_END : node < PT_OCT_END) : (TAGGED ? node != PT_SWZ_END : (walking != 0u || leaf_n > 0));
  }
  __device__ __forceinline__ bool pending() const { return OTAG && PT_OCT_BATCH_FALLBACK && node >= PT_OCT_PENDING; }
  /* ... as a wave mask, where no lane holds a leaf (after the leaf phase: the chunk cut) */
  __device__ __forceinline__ unsigned long long walking_mask() const { return TAGS ? __builtin_amdgcn_ballot_w64(alive()) : __builtin_amdgcn_uicmp(walking, 0u, 33); }

  __device__ __forceinline__ void begin(const PtSceneDev& sc, const PtSceneView& sv, V3 o_, V3 d_,
                                        unsigned long long& c_floor) {
    o = o_;
    d = d_;
    /* dirs, shape_tree.ml:201 */
    dirs = (d.x >= 0.0 ? 1u : 0u) | (d.y >= 0.0 ? 2u : 0u) | (d.z >= 0.0 ? 4u : 0u);
    if (!FILT) {
      inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z); /* Ray.create, ray.ml:7-10 */
      exact_slab = !(pt_isfinite(inv.x) && pt_isfinite(inv.y) && pt_isfinite(inv.z));
    } else {
      inv = v3(0.0, 0.0, 0.0); /* the filter takes its reciprocals in binary32 (below); the binary64 fallback divides for itself */
      exact_slab = false;
    }
    if (FILT) {
      skip_off = 2u * dirs;
      if (SWZ) { /* where this ray's (near, far) pair of each axis starts inside a node */
        sel_x = (dirs & 1u) ? 0u : 4u;
        sel_y = 12u + ((dirs & 2u) ? 0u : 4u);
        sel_z = 24u + ((dirs & 4u) ? 0u : 4u);
      }
      const double omax = __builtin_fmax(pt_fabs(o.x), __builtin_fmax(pt_fabs(o.y), pt_fabs(o.z)));
      /* The filter's constants straight in binary32: inv32 = v_rcp_f32(fl32(d)) (1 ulp) is within 3 * 2^-24 of 1 / d and
       * (o inv)32 = fl32(fl32(o) inv32) within 5 * 2^-24 of o / d, instead of one rounding each from Ray.create's binary64
       * quotients -- three binary64 divisions per ray (~40 vector instructions of a walk's ~1000) that only the filter used.
       * The bound above becomes 6 (t~) and 13 (u) units of 2^-24 (..) against m2 = 32 of them: still more than twice.  A zero,
       * subnormal or NaN component gives inf / NaN here and fails the guard below (binary64 throughout, as before); a
       * component beyond binary32 gives inv32 = 0 for a true |1 / d| < 2^-127, the flush case the guard's comment covers. */
      fix = __builtin_amdgcn_rcpf((float)d.x);
      fiy = __builtin_amdgcn_rcpf((float)d.y);
      fiz = __builtin_amdgcn_rcpf((float)d.z);
      const float fimax = __builtin_fmaxf(__builtin_fabsf(fix), __builtin_fmaxf(__builtin_fabsf(fiy), __builtin_fabsf(fiz)));
      const float fisum = __builtin_fabsf(fix) + __builtin_fabsf(fiy) + __builtin_fabsf(fiz); /* (fmax drops a NaN, a sum keeps it) */
      /* every binary32 intermediate stays far inside the format: (mag + |o|) |inv| < 2^100 for every node, because every
       * node lies inside the root box (root_mag = its largest |coordinate|, +inf when that exceeds binary32: such a scene
       * is walked in binary64 throughout), so no product, sum or margin of the filter can overflow, whatever the scene's
       * scale.  And max|1/d| is kept far above the binary32 subnormals (>= 2^-60): components of inv32 / (o inv)32 that
       * are subnormal -- or flushed to zero, whatever the f32 denormal mode of the code object -- are then wrong by
       * < 2^-126 (mag + |o|) absolute, which m2 >= 2^-19 (mag + |o|) 2^-60 + 1e-30 covers with room to spare. */
      const float fomax = (float)omax; /* (a magnitude beyond binary32 becomes +inf and fails the guard) */
      if (!((sc.root_mag + fomax) * fisum < 0x1p100f) || !(fimax > 0x1p-60f)) exact_slab = true;
      fnx = ORIGIN_ZERO ? 0.0f : -((float)o.x * fix);
      fny = ORIGIN_ZERO ? 0.0f : -((float)o.y * fiy);
      fnz = ORIGIN_ZERO ? 0.0f : -((float)o.z * fiz);
      k2 = fimax * PT_MARGIN_K2;
      if (OTAG) k2 *= 1.000002f; /* (the node's magnitude is taken from its bounds as they are: test_box) */
      c2base = __builtin_fmaf(fomax * 1.000001f, k2, 1e-30f);
      /* exact_slab folded into the margin: with m2 = NaN neither `u >= m2` nor `u < -m2` holds, so every test of such a ray
       * is undecided and takes the binary64 code -- no per-visit instruction for the flag itself */
      if (exact_slab) c2base = __builtin_nanf("");
    }
    r.t = PT_MAX_FINITE;
    r.slot = -1;
    r.u = 0.0;
    r.v = 0.0;
    /* ganesha Floor.intersect (main.ml:247-256): f1 then f2, the first hit clips t_max for the tree */
    if (MODE == PT_MODE_ARRAY && sc.n_floor > 0) {
      for (int f = 0; f < sc.n_floor; ++f) {
        V3 fa, fb, fc;
        if (f < sv.n_floor_lds) { /* (wave-uniform) */
          const __attribute__((address_space(3))) double* tv = sv.floor_lds + f * 10;
          fa = v3(tv[0], tv[1], tv[2]);
          fb = v3(tv[3], tv[4], tv[5]);
          fc = v3(tv[6], tv[7], tv[8]);
        } else {
          const double* tv = sv.tri + (size_t)(sc.n_slots + f) * 10;
          fa = pt_load_v3(tv);
          fb = pt_load_v3(tv + 3);
          fc = pt_load_v3(tv + 6);
        }
        double t, u, v;
        if (COUNT) c_floor++;
        if (pt_triangle_intersect(fa, fb, fc, o, d, 0.0, PT_MAX_FINITE, &t, &u, &v)) {
          r.t = t;
          r.u = u;
          r.v = v;
          r.slot = sc.n_slots + f;
          break;
        }
      }
    }
    /* packet constants of spheres_intersect_aux (lib.rs:115-117): a is the UNFUSED scalar dot */
    qa = 0.0;
    one_over_a = 0.0;
    if (MODE == PT_MODE_SIMD) {
      qa = d.x * d.x + d.y * d.y + d.z * d.z;
      one_over_a = 1.0 / qa;
    }
    sp = 0;
    if (OCT) skip_off = dirs * sv.n_nodes;
    node = SWZ ? sv.swz_root : ((G32 && !OCT && sv.has_top) ? PT_TOP_FLAG : 0u); /* the root (slot 0 of the top image) */
    walking = sc.n_nodes > 0;
    if (TAGGED && sc.n_nodes <= 0) node = PT_SWZ_END;
    if (OTAG) node = skip_off; /* the root's record of this ray's octant */
    if (OTAG && sc.n_nodes <= 0) node = PT_OCT_END;
    if (LOCT) { /* the root's record of this ray's octant; skip_off = the octant's first record */
      skip_off = dirs * sv.n_nodes;
      node = sc.n_nodes > 0 ? skip_off : PT_LOCT_END;
    }
    lkx = 0u;
    leaf_first = 0;
    leaf_n = 0;
    if (FILT) update_t32();
  }
  /* the closest hit so far as the filter sees it; called whenever r.t may have changed */
  __device__ __forceinline__ void update_t32() {
    t32 = (float)r.t; /* PT_MAX_FINITE -> +inf */
    c2 = c2base + (t32 < 0x1p120f ? t32 * PT_MARGIN_T : 0.0f);
  }

#if PT_WALK_ASM
  /* The node loop of the LDS walk (TAGGED), written out in gfx950 assembly.  Measured (tools/README.md "what binds the node
   * loop", profiles/r05_visit_sensitivity.txt): three more vector instructions per visit cost the headline frame 0.5 %, six more
   * SCALAR ones 1.6 % -- with four waves per SIMD, each issuing at most one instruction per turn, the walk is bound by the number
   * of instructions a wave issues per visit, of whatever kind, and of the compiler's 56 (21 vector + 6 LDS + 4 waits + ~25 scalar
   * of exec-mask algebra for a loop with a divergent and a uniform exit and a divergent branch inside) the scalar ones are
   * bookkeeping.  Here a visit is 21 vector + 6 LDS + 4 waits + 6 ... 9 scalar instructions: the exec mask IS the set of lanes
   * that still want a node step, a lane leaves by one s_and of exec, and the filter's undecided case is a wave-uniform exit.
   * Same loads, same arithmetic, same select as node_step (read the two side by side).
   * Runs visits until no lane wants one, or -- once a lane has left -- fewer than `wmin` are still walking.  Returns nonzero if it
   * stopped BEFORE the select of a visit because the binary32 filter left a lane undecided: the caller performs that visit with
   * node_step (the binary64 arithmetic lives there) and calls again.  Temporaries live in v120..v127 (the halves of a
   * ds_read2_b32 result cannot be named through an operand): 128-VGPR kernels only (k_bounce). */
  __device__ __forceinline__ unsigned long long walk_asm(int wmin) {
    register uint32_t bx0 asm("v120"), bx1 asm("v121"), by0 asm("v122"), by1 asm("v123"), bz0 asm("v124"), bz1 asm("v125"), lk0 asm("v126"), lk1 asm("v127");
    lk0 = lkx;
    unsigned long long und, sv_, ent_, hit_;
    uint32_t a_, sk_, nr_, tg_, n_;
    float tn_, tf_, p_, q_, r_, s_, m2_;
    asm volatile(
        "s_mov_b64 %[sv], exec\n"
        "s_mov_b64 %[und], 0\n"
        "v_and_b32 %[tg], 3, %[node]\n"
        "v_cmp_eq_u32 vcc, 0, %[tg]\n"
        "s_and_b64 exec, exec, vcc\n"
        "s_cbranch_execz .Ldone%=\n"
        "s_mov_b64 %[ent], exec\n"
        "s_waitcnt lgkmcnt(0)\n" /* (scalar loads return out of order: nothing of the compiler's may be outstanding) */
        ".Lloop%=:\n"
        "v_add_u32 %[a], %[node], %[so]\n"
        "ds_read_u16 %[sk], %[a] offset:44\n"
        "ds_read_u16 %[nr], %[a] offset:60\n"
        "v_add_u32 %[a], %[node], %[sx]\n"
        "ds_read2_b32 v[120:121], %[a] offset1:1\n"
        "v_add_u32 %[a], %[node], %[sy]\n"
        "ds_read2_b32 v[122:123], %[a] offset1:1\n"
        "v_add_u32 %[a], %[node], %[sz]\n"
        "ds_read2_b32 v[124:125], %[a] offset1:1\n"
        "ds_read2_b32 v[126:127], %[node] offset0:9 offset1:10\n"
        "s_waitcnt lgkmcnt(3)\n"
        "v_fma_f32 %[tn], %[bx0], %[fix], %[fnx]\n"
        "v_fma_f32 %[tf], %[bx1], %[fix], %[fnx]\n"
        "s_waitcnt lgkmcnt(2)\n"
        "v_fma_f32 %[p], %[by0], %[fiy], %[fny]\n"
        "v_fma_f32 %[q], %[by1], %[fiy], %[fny]\n"
        "s_waitcnt lgkmcnt(1)\n"
        "v_fma_f32 %[r], %[bz0], %[fiz], %[fnz]\n"
        "v_fma_f32 %[s], %[bz1], %[fiz], %[fnz]\n"
        "v_max_f32 %[tn], %[tn], %[p]\n"
        "v_min_f32 %[tf], %[tf], %[q]\n"
        "v_max3_f32 %[tn], %[tn], %[r], 0\n"
        "v_min3_f32 %[tf], %[tf], %[s], %[t32]\n"
        "s_waitcnt lgkmcnt(0)\n"
        "v_fma_f32 %[m2], %[lk1], %[k2], %[c2]\n"
        "v_sub_f32 %[tf], %[tf], %[tn]\n"
        "v_cmp_ge_f32_e64 %[hit], %[tf], %[m2]\n"
        "v_cmp_nge_f32_e64 vcc, |%[tf]|, %[m2]\n"
        "s_cbranch_vccnz .Lund%=\n"
        "v_cndmask_b32_e64 %[node], %[sk], %[nr], %[hit]\n"
        "v_and_b32 %[tg], 3, %[node]\n"
        "v_cmp_eq_u32 vcc, 0, %[tg]\n"
        "s_and_b64 exec, exec, vcc\n"
        "s_cbranch_execz .Ldone%=\n"
        "s_cmp_eq_u64 exec, %[ent]\n"
        "s_cbranch_scc1 .Lloop%=\n"
        "s_bcnt1_i32_b64 %[n], exec\n"
        "s_cmp_ge_u32 %[n], %[wmin]\n"
        "s_cbranch_scc1 .Lloop%=\n"
        "s_branch .Ldone%=\n"
        ".Lund%=:\n"
        "s_mov_b64 %[und], vcc\n"
        ".Ldone%=:\n"
        "s_mov_b64 exec, %[sv]\n"
        : [node] "+v"(node), [lk0] "+v"(lk0), [lk1] "=&v"(lk1), [bx0] "=&v"(bx0), [bx1] "=&v"(bx1), [by0] "=&v"(by0), [by1] "=&v"(by1),
          [bz0] "=&v"(bz0), [bz1] "=&v"(bz1), [und] "=&s"(und), [sv] "=&s"(sv_), [ent] "=&s"(ent_), [hit] "=&s"(hit_), [n] "=&s"(n_),
          [a] "=&v"(a_), [sk] "=&v"(sk_), [nr] "=&v"(nr_), [tg] "=&v"(tg_), [tn] "=&v"(tn_), [tf] "=&v"(tf_), [p] "=&v"(p_), [q] "=&v"(q_),
          [r] "=&v"(r_), [s] "=&v"(s_), [m2] "=&v"(m2_)
        : [so] "v"(skip_off), [sx] "v"(sel_x), [sy] "v"(sel_y), [sz] "v"(sel_z), [fix] "v"(fix), [fiy] "v"(fiy), [fiz] "v"(fiz), [fnx] "v"(fnx),
          [fny] "v"(fny), [fnz] "v"(fnz), [t32] "v"(t32), [k2] "v"(k2), [c2] "v"(c2), [wmin] "s"(wmin)
        : "vcc", "scc");
    lkx = lk0;
    return und;
  }
  /* The same loop on the per-octant LDS image (LOCT): 17 vector + 2 LDS + 2 waits + 4 scalar instructions per visit, 25 issued
   * against 37..40 (profiles/pr_lds_oct_isa.txt).  `node` is a record number; the record's address is one shift-add beside the
   * image's LDS address (a scalar).  The undecided test comes first and leaves through vcc as above; the hit test then sets vcc for
   * the select, which takes word 6's low half (the hit link) or its high half (the miss link) in one instruction; the tag test
   * writes exec itself (v_cmpx: the lanes that still want a node).  The exits are one comparison: thr = min(lanes entered, wmin),
   * go on while the lanes left are >= thr -- while nobody has left that holds, once somebody has it is "fewer than wmin", and an
   * empty exec is below any thr >= 1: walk_asm's rule, three scalar instructions whether or not a lane has left.
   * Same arithmetic as node_step's LOCT branch.  (Measured and not kept, DESIGN.md Appendix A: the records as two arrays of
   * 16-byte words against bank conflicts, one s_waitcnt instead of two.) */
  __device__ __forceinline__ unsigned long long walk_asm_oct(uint32_t base, int wmin) {
    register uint32_t nx asm("v120"), ny asm("v121"), nz asm("v122"), fx asm("v123"), fy asm("v124"), fz asm("v125"), lk asm("v126"), mg asm("v127");
    unsigned long long und, sv_;
    uint32_t a_, n_, thr_;
    float tn_, tf_, p_, q_, r_, s_, m2_;
    asm volatile(
        "s_mov_b64 %[sv], exec\n"
        "s_mov_b64 %[und], 0\n"
        "v_cmpx_gt_u32 vcc, %[lt], %[node]\n"
        "s_cbranch_execz .Ldone%=\n"
        "s_bcnt1_i32_b64 %[thr], exec\n"
        "s_min_u32 %[thr], %[thr], %[wmin]\n"
        "s_waitcnt lgkmcnt(0)\n" /* (scalar loads return out of order: nothing of the compiler's may be outstanding) */
        ".Lloop%=:\n"
        "v_lshl_add_u32 %[a], %[node], 5, %[base]\n"
        "ds_read_b128 v[120:123], %[a]\n"
        "ds_read_b128 v[124:127], %[a] offset:16\n"
        "s_waitcnt lgkmcnt(1)\n"
        "v_fma_f32 %[tn], %[nx], %[fix], %[fnx]\n"
        "v_fma_f32 %[p], %[ny], %[fiy], %[fny]\n"
        "v_fma_f32 %[r], %[nz], %[fiz], %[fnz]\n"
        "v_fma_f32 %[tf], %[fx], %[fix], %[fnx]\n"
        "v_max_f32 %[tn], %[tn], %[p]\n"
        "v_max3_f32 %[tn], %[tn], %[r], 0\n"
        "s_waitcnt lgkmcnt(0)\n"
        "v_fma_f32 %[q], %[fy], %[fiy], %[fny]\n"
        "v_fma_f32 %[s], %[fz], %[fiz], %[fnz]\n"
        "v_fma_f32 %[m2], %[mg], %[k2], %[c2]\n"
        "v_min_f32 %[tf], %[tf], %[q]\n"
        "v_min3_f32 %[tf], %[tf], %[s], %[t32]\n"
        "v_sub_f32 %[tf], %[tf], %[tn]\n"
        "v_cmp_nge_f32_e64 vcc, |%[tf]|, %[m2]\n"
        "s_cbranch_vccnz .Lund%=\n"
        "v_cmp_ge_f32 vcc, %[tf], %[m2]\n"
        "v_cndmask_b32_sdwa %[node], %[lk], %[lk], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0\n"
        "v_cmpx_gt_u32 vcc, %[lt], %[node]\n"
        "s_bcnt1_i32_b64 %[n], exec\n"
        "s_cmp_ge_u32 %[n], %[thr]\n"
        "s_cbranch_scc1 .Lloop%=\n"
        "s_branch .Ldone%=\n"
        ".Lund%=:\n"
        "s_mov_b64 %[und], vcc\n"
        ".Ldone%=:\n"
        "s_mov_b64 exec, %[sv]\n"
        : [node] "+v"(node), [nx] "=&v"(nx), [ny] "=&v"(ny), [nz] "=&v"(nz), [fx] "=&v"(fx), [fy] "=&v"(fy), [fz] "=&v"(fz), [lk] "=&v"(lk),
          [mg] "=&v"(mg), [und] "=&s"(und), [sv] "=&s"(sv_), [thr] "=&s"(thr_), [n] "=&s"(n_), [a] "=&v"(a_), [tn] "=&v"(tn_),
          [tf] "=&v"(tf_), [p] "=&v"(p_), [q] "=&v"(q_), [r] "=&v"(r_), [s] "=&v"(s_), [m2] "=&v"(m2_)
        : [base] "s"(base), [lt] "s"((uint32_t)PT_LOCT_LEAF_TAG), [fix] "v"(fix), [fiy] "v"(fiy), [fiz] "v"(fiz), [fnx] "v"(fnx), [fny] "v"(fny),
          [fnz] "v"(fnz), [t32] "v"(t32), [k2] "v"(k2), [c2] "v"(c2), [wmin] "s"(wmin)
        : "vcc", "scc");
    return und;
  }
#endif
  /* Visit `node`: bbox test against the closest hit so far, then descend / hold the leaf / pop.  The traversal
   * stack (far children only) lives in LDS, one column per lane (conflict-free ds_write / ds_read).  A far child's
   * bbox is tested when it is POPPED, against the closest hit so far -- exactly the t_max the reference's recursion
   * passes (shape_tree.ml:210-216). */
  /* the reference's own arithmetic on the binary64 node `np` (the filter could not decide): 1 / d again -- the same three
   * divisions as Ray.create, opaque to the optimiser, or it hoists them out of the walk and keeps six more registers live
   * across the hot loop */
  __device__ __forceinline__ bool slab64(const double* nb /* mn.xyz, mx.xyz */) const {
    double qx = d.x, qy = d.y, qz = d.z;
    asm volatile("" : "+v"(qx), "+v"(qy), "+v"(qz));
    const V3 inv64 = v3(1.0 / qx, 1.0 / qy, 1.0 / qz);
    return (!(pt_isfinite(inv64.x) && pt_isfinite(inv64.y) && pt_isfinite(inv64.z))) ? pt_slab_hit_exact(nb, o, inv64, 0.0, r.t)
                                                                                     : pt_slab_hit_fast<ORIGIN_ZERO>(nb, o, inv64, 0.0, r.t);
  }
  __device__ __forceinline__ bool slab64(const PtNode* np) const { return slab64(np->mn); }
  /* What the generic u = hi - lo cannot decide although it is certain: ONE axis k whose slab interval [near_k, far_k] lies
   * inside the other two axes' intervals and inside [0, t_max] by the margin.  Then the reference's lo IS near_k and its hi IS
   * far_k, and near_k <= far_k holds by construction (the min and the max of the same two products): a hit, however small
   * far_k - near_k is -- and it is exactly 0 for a box that is flat along k (an axis-aligned wall's triangles: cornell's whole
   * room -- 4.7 % of its box tests were undecided and 31 % of its wave steps ran the binary64 fallback), tiny for thin boxes.
   * Each one-sided gap carries the same error bound as u, so the same margin decides it.  false = still undecided (near-ties
   * between DIFFERENT axes, NaNs): binary64. */
  __device__ __forceinline__ bool nested_hit(float tnx, float tfx, float tny, float tfy, float tnz, float tfz, float m2) const {
    const float lx = __builtin_fmaxf(__builtin_fmaxf(tny, tnz), 0.0f), hx = __builtin_fminf(__builtin_fminf(tfy, tfz), t32);
    const float ly = __builtin_fmaxf(__builtin_fmaxf(tnx, tnz), 0.0f), hy = __builtin_fminf(__builtin_fminf(tfx, tfz), t32);
    const float lz = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), 0.0f), hz = __builtin_fminf(__builtin_fminf(tfx, tfy), t32);
    return (tnx - lx >= m2 && hx - tfx >= m2) || (tny - ly >= m2 && hy - tfy >= m2) || (tnz - lz >= m2 && hz - tfz >= m2);
  }
  /* Bbox.is_hit of `nd` against the closest hit so far + the node's links (a, b, real slot count) */
  __device__ __forceinline__ bool test_box(const PtSceneView& sv, uint32_t nd, uint32_t& na, uint32_t& nb, uint32_t& n_real, bool active = true,
                                           bool* defer_undecided = nullptr /* OTAG: set instead of evaluating the binary64 test here */) const {
    const double t_min = 0.0;
    bool hit;
    if (FILT) {
      uint4 w0, w1;
      float mag;
      if (OTAG) { /* nd is the record's number in the whole image; the octant's tagged record: near xyz, far xyz, hit link, miss link */
        const uint4* p = (const uint4*)(sv.nodes32o + (uint32_t)(nd << 5)); /* (a 32-bit offset beside the scalar base: one shift ahead of the loads) */
        const uint4 r0 = p[0];
        uint4 r1 = p[1];
#if PT_DIAG_EXTRA_LOADS /* diagnostic builds only: what one / two more 16-byte loads per node visit cost (the record's own line: no new misses) */
        {
          const uint4 x0 = p[(nd & 1u) ? -1 : 2];
          if (x0.x == 0x7fc12345u && x0.w == 0x12345u) r1.x ^= 1u; /* (never true: keeps the load) */
#if PT_DIAG_EXTRA_LOADS > 1
          const uint4 x1 = p[(nd & 1u) ? -2 : 3];
          if (x1.x == 0x7fc12345u && x1.w == 0x12345u) r1.y ^= 1u;
#endif
        }
#endif
        oct_link = r1.z;
        oct_skip = r1.w;
        n_real = (r1.z >> PT_OCT_LEAF_FIRST_BITS) & PT_OCT_LEAF_REAL_MAX; /* (meaningful for a leaf; na / nb are not used by this walk) */
        na = r1.z & ((1u << PT_OCT_LEAF_FIRST_BITS) - 1u);
        nb = 0u;
        const float nx_ = __uint_as_float(r0.x), ny_ = __uint_as_float(r0.y), nz_ = __uint_as_float(r0.z);
        const float fx_ = __uint_as_float(r0.w), fy_ = __uint_as_float(r1.x), fz_ = __uint_as_float(r1.y);
        const float tnx = __builtin_fmaf(nx_, fix, fnx), tny = __builtin_fmaf(ny_, fiy, fny), tnz = __builtin_fmaf(nz_, fiz, fnz);
        const float tfx = __builtin_fmaf(fx_, fix, fnx), tfy = __builtin_fmaf(fy_, fiy, fny), tfz = __builtin_fmaf(fz_, fiz, fnz);
        const float a = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz);
        const float b = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
        const float u = __builtin_fminf(b, t32) - __builtin_fmaxf(a, 0.0f);
        const float mg = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(nx_), __builtin_fabsf(ny_)), __builtin_fabsf(nz_)),
                                         __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(fx_), __builtin_fabsf(fy_)), __builtin_fabsf(fz_)));
        const float m2 = __builtin_fmaf(mg, k2, c2);
#if PT_FILTER_DEBUG
        dbg_u = u;
        dbg_m2 = m2;
#endif
        hit = u >= m2;
        if (defer_undecided) { /* PT_OCT_BATCH_FALLBACK: no branch here at all -- the caller tags the lane (node_step) */
          *defer_undecided = active && !(__builtin_fabsf(u) >= m2);
          if (COUNT && *defer_undecided) n_undecided++;
          return hit;
        }
        if (active && !(__builtin_fabsf(u) >= m2)) { /* (as below: one divergent branch; a ray the filter does not apply to carries m2 = NaN) */
          if (COUNT) {
            n_undecided++;
            if (pt_lane() == __ffsll((long long)__ballot(1)) - 1) n_wave_fallbacks++;
          }
          hit = slab64(sv.nodes + (nd - skip_off)); /* (the canonical node: the octant's base off again) */
        }
        return hit;
      }
      if (SWZ) { /* nd is the node's absolute LDS address; the ray's sign-selected (near, far) bounds: see the layout */
        const pt_f2 bx = *(const __attribute__((address_space(3))) pt_f2*)PT_LDS_AT(nd + sel_x);
        const pt_f2 by = *(const __attribute__((address_space(3))) pt_f2*)PT_LDS_AT(nd + sel_y);
        const pt_f2 bz = *(const __attribute__((address_space(3))) pt_f2*)PT_LDS_AT(nd + sel_z);
        const pt_u2 lk = *(const __attribute__((address_space(3))) pt_u2*)PT_LDS_AT(nd + PT_SWZ_OFF_LINKS);
        lkx = lk.x;
        na = lk.x & 0xffffu;
        nb = (lk.x >> 16) | ((lk.y & 3u) << 30);
        n_real = lk.x >> 16;
        const float tnx = __builtin_fmaf(bx.x, fix, fnx), tfx = __builtin_fmaf(bx.y, fix, fnx);
        const float tny = __builtin_fmaf(by.x, fiy, fny), tfy = __builtin_fmaf(by.y, fiy, fny);
        const float tnz = __builtin_fmaf(bz.x, fiz, fnz), tfz = __builtin_fmaf(bz.y, fiz, fnz);
        const float a = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz);
        const float b = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
        const float u = __builtin_fminf(b, t32) - __builtin_fmaxf(a, 0.0f);
        const float m2 = __builtin_fmaf(__uint_as_float(lk.y), k2, c2);
        hit = u >= m2;
        /* one divergent branch, no wave-uniform pre-check: two scalar instructions per visit instead of five (at 4 waves per
         * SIMD the scalar instructions of a visit -- 27 against 22 vector ones -- are no longer free) */
        if (active && !(__builtin_fabsf(u) >= m2)) {
          const bool nested = nested_hit(tnx, tfx, tny, tfy, tnz, tfz, m2);
          if (nested) hit = true;
          else {
            if (COUNT) n_undecided++;
            const uint32_t k64 = (nd - sv.swz_root) / PT_SWZ_NODE_BYTES;
            hit = sv.nodes64 ? slab64(sv.nodes64 + (size_t)k64 * 6u) : slab64(sv.nodes + k64); /* (wave-uniform choice) */
          }
          if (COUNT && __ballot(!nested) != 0 && pt_lane() == __ffsll((long long)__ballot(1)) - 1) n_wave_fallbacks++;
        }
        return hit;
      }
      { /* nd is the node's index; 32-byte global image: six binary32 bounds, a, b (leaf b: count | real << 15 | tag) */
        if (nd & PT_TOP_FLAG) { /* ... or PT_TOP_FLAG | byte offset into the LDS copy of the tree's top: same words */
          const uint4* p = (const uint4*)(sv.top + (nd & (PT_TOP_FLAG - 1u)));
          w0 = p[0];
          w1 = p[1];
        } else {
          const uint4* p = (const uint4*)(sv.nodes32 + (size_t)nd * 32u);
          w0 = p[0];
          w1 = p[1];
        }
        na = w1.z;
        const bool leaf = (w1.w >> 30) == PT_NODE_LEAF_AXIS;
        n_real = (w1.w >> 15) & 0x7fffu;
        nb = leaf ? ((w1.w & 0x7fffu) | (PT_NODE_LEAF_AXIS << 30)) : w1.w;
        /* the node's own magnitude, from the bounds just loaded (the LDS image stores it) */
        mag = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(__uint_as_float(w0.x)), __builtin_fabsf(__uint_as_float(w0.y))),
                                              __builtin_fmaxf(__builtin_fabsf(__uint_as_float(w0.z)), __builtin_fabsf(__uint_as_float(w0.w)))),
                              __builtin_fmaxf(__builtin_fabsf(__uint_as_float(w1.x)), __builtin_fabsf(__uint_as_float(w1.y)))) * 1.000001f;
      }
      const float t0x = __builtin_fmaf(__uint_as_float(w0.x), fix, fnx), t1x = __builtin_fmaf(__uint_as_float(w0.w), fix, fnx);
      const float t0y = __builtin_fmaf(__uint_as_float(w0.y), fiy, fny), t1y = __builtin_fmaf(__uint_as_float(w1.x), fiy, fny);
      const float t0z = __builtin_fmaf(__uint_as_float(w0.z), fiz, fnz), t1z = __builtin_fmaf(__uint_as_float(w1.y), fiz, fnz);
      const float a = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t0x, t1x), __builtin_fminf(t0y, t1y)), __builtin_fminf(t0z, t1z));
      const float b = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t0x, t1x), __builtin_fmaxf(t0y, t1y)), __builtin_fmaxf(t0z, t1z));
      const float u = __builtin_fminf(b, t32) - __builtin_fmaxf(a, 0.0f);
      const float m2 = __builtin_fmaf(mag, k2, c2);
      hit = u >= m2;
      /* (a ray the filter does not apply to carries m2 = NaN: neither comparison holds, every test of it is undecided.)
       * One comparison |u| >= m2 (u == -m2 exactly counts as a decided miss: it is one, m2 is twice the error bound) and one
       * divergent branch, no wave-uniform pre-check -- see the layout-3 branch above */
      if (active && !(__builtin_fabsf(u) >= m2)) {
        /* (no nested_hit here: on a mesh walked from HBM / L2 it settles 7 % of the undecided tests and its twenty
         * instructions in 22 % of the wave steps cost 3 % of the frame) */
        if (COUNT) {
          n_undecided++;
          if (pt_lane() == __ffsll((long long)__ballot(1)) - 1) n_wave_fallbacks++;
        }
        /* the reference's arithmetic, on the binary64 node (global memory: L2-resident, rarely read) */
        hit = slab64(sv.nodes + ((nd & PT_TOP_FLAG) ? *(const uint32_t*)(sv.top + (nd & (PT_TOP_FLAG - 1u)) + 48) : nd));
      }
    } else {
      const PtNode* np = sv.nodes + nd;
      hit = exact_slab ? pt_slab_hit_exact(np->mn, o, inv, t_min, r.t) : pt_slab_hit_fast<ORIGIN_ZERO>(np->mn, o, inv, t_min, r.t);
      na = np->a;
      nb = np->b;
      n_real = np->pad[0];
    }
    return hit;
  }

  __device__ __forceinline__ void node_step(const PtSceneView& sv, StackT* stack, unsigned long long& c_nodes,
                                            unsigned long long& c_prims) {
    if (COUNT && (PT_DIAG == 0 || (PT_DIAG <= 2 && !ORIGIN_ZERO))) c_nodes++;
    bool descend = false;
    uint32_t na, nb, n_real;
    if (OTAG) { /* the tagged per-octant record: a hit leads to word 6 (near child, or "holds a leaf"), a miss to word 7 */
      if (PT_OCT_BATCH_FALLBACK) { /* an undecided test: the lane steps out of the walk with its node tagged (resolve_pending) */
        bool und = false;
        const bool hit = test_box(sv, node, na, nb, n_real, true, &und);
        if (COUNT && PT_DIAG == 0 && !und && hit && (oct_link >> 30) == 1u) c_prims += (unsigned long long)(MODE == PT_MODE_SIMD ? ((n_real + 3u) & ~3u) : n_real);
        node = und ? (node | PT_OCT_PENDING) : (hit ? oct_link : oct_skip);
        return;
      }
      const bool hit = test_box(sv, node, na, nb, n_real);
      if (COUNT && PT_DIAG == 0 && hit && (oct_link >> 30) == 1u) c_prims += (unsigned long long)(MODE == PT_MODE_SIMD ? ((n_real + 3u) & ~3u) : n_real);
      node = hit ? oct_link : oct_skip;
      return;
    }
    if (LOCT) { /* the per-octant LDS record: near xyz, far xyz, hit | miss << 16, magnitude (walk_asm_oct: the same visit) */
      const uint32_t ad = sv.oct_base + (node << 5), ad1 = ad + 16u;
      const pt_u4 r0 = *(const __attribute__((address_space(3))) pt_u4*)PT_LDS_AT(ad);
      const pt_u4 r1 = *(const __attribute__((address_space(3))) pt_u4*)PT_LDS_AT(ad1);
      const float tnx = __builtin_fmaf(__uint_as_float(r0.x), fix, fnx), tny = __builtin_fmaf(__uint_as_float(r0.y), fiy, fny),
                  tnz = __builtin_fmaf(__uint_as_float(r0.z), fiz, fnz);
      const float tfx = __builtin_fmaf(__uint_as_float(r0.w), fix, fnx), tfy = __builtin_fmaf(__uint_as_float(r1.x), fiy, fny),
                  tfz = __builtin_fmaf(__uint_as_float(r1.y), fiz, fnz);
      const float a = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz);
      const float b = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
      const float u = __builtin_fminf(b, t32) - __builtin_fmaxf(a, 0.0f);
      const float m2 = __builtin_fmaf(__uint_as_float(r1.w), k2, c2);
      bool hit = u >= m2;
      if (!(__builtin_fabsf(u) >= m2)) { /* (as on the shared image: the nested-interval rule, then binary64) */
        if (nested_hit(tnx, tfx, tny, tfy, tnz, tfz, m2)) hit = true;
        else {
          const uint32_t k64 = node - skip_off; /* the canonical node: the octant's base off again */
          hit = sv.nodes64 ? slab64(sv.nodes64 + (size_t)k64 * 6u) : slab64(sv.nodes + k64); /* (wave-uniform choice) */
        }
      }
      static_assert(!(LOCT && COUNT), "the per-octant LDS image has no counting walk: counting launches keep the shared image");
      node = hit ? (r1.z & 0xffffu) : (r1.z >> 16);
      return;
    }
    /* threaded image: where to go once this subtree is done (issued beside the node's own reads) */
    constexpr bool THREAD32 = G32;
    uint32_t skip;
    if (SWZ) {
      skip = (uint32_t)*(const __attribute__((address_space(3))) uint16_t*)PT_LDS_AT(node + skip_off + PT_SWZ_OFF_SKIP);
      asm("" : "+v"(skip)); /* (a zero-extended 16-bit load the select below need not mask again) */
    }
    else if (!THREAD32) skip = 0u;
    else if (node & PT_TOP_FLAG) { /* top image: 16-bit byte offsets, a top node's successor is a top node */
      const uint32_t s16 = (uint32_t)*(const uint16_t*)(sv.top + (node & (PT_TOP_FLAG - 1u)) + 32u + 2u * dirs);
      skip = s16 == 0xffffu ? 0xffffffffu : (PT_TOP_FLAG | s16);
    } else skip = sv.skip32[(size_t)node * 8u + dirs];
    if (SWZ) { /* (TAGGED) */
      uint32_t near_c = (uint32_t)*(const __attribute__((address_space(3))) uint16_t*)PT_LDS_AT(node + skip_off + PT_SWZ_OFF_NEAR);
      asm("" : "+v"(near_c));
      const bool hit = test_box(sv, node, na, nb, n_real);
#if PT_DIAG_VISIT_VALU || PT_DIAG_VISIT_LDS || PT_DIAG_VISIT_SALU
      for (int k_ = 0; k_ < PT_DIAG_VISIT_VALU; ++k_) asm volatile("v_add_u32 %0, 1, %0" : "+v"(lkx_diag));
      for (int k_ = 0; k_ < PT_DIAG_VISIT_LDS; ++k_) lkx_diag += (uint32_t)*(const __attribute__((address_space(3))) uint16_t*)PT_LDS_AT(node + skip_off + PT_SWZ_OFF_SKIP + 2u * (uint32_t)(k_ + 1));
      for (int k_ = 0; k_ < PT_DIAG_VISIT_SALU; ++k_) { uint32_t t_; asm volatile("s_mov_b32 %0, 1" : "=s"(t_)); }
#endif
      /* an inner node that was hit: its near child; a leaf that was hit: what follows it, tagged "holds a leaf"; a miss: what
       * follows this subtree (PT_SWZ_END: nothing) */
      if (COUNT && PT_DIAG == 0 && hit && (near_c & PT_SWZ_TAG_LEAF)) c_prims += (unsigned long long)(MODE == PT_MODE_SIMD ? ((n_real + 3u) & ~3u) : n_real);
      node = hit ? near_c : skip;
      return;
    }
    const bool hit = test_box(sv, node, na, nb, n_real);
    if (hit) {
      const uint32_t axis = nb >> 30;
      if (axis == PT_NODE_LEAF_AXIS) {
        leaf_first = (int)na;
        leaf_n = (int)n_real; /* real slots; the NaN padding (main.ml:185) can never be selected */
        /* Leaf.length incl. padding: Simd_leaf pads to a multiple of 4 (main.ml:179-186); the filter image keeps the real count */
        if (COUNT && PT_DIAG == 0) c_prims += (unsigned long long)(nb & 0x3fffffffu);
      } else {
        /* Branch: near child first (shape_tree.ml:209), far child deferred */
        const uint32_t lhs = na, rhs = nb & 0x3fffffffu;
        const bool lhs_first = (dirs >> axis) & 1u;
        if (!THREAD32) {
          PT_STACK_PUSH(stack, sp, lhs_first ? rhs : lhs);
          ++sp;
        }
        node = lhs_first ? lhs : rhs;
        descend = true;
      }
    }
    if (!descend) {
      /* the next node's bbox is tested on the NEXT visit, i.e. after this leaf's packet has been
       * intersected and r.t shrunk -- the t_max the reference passes to the far child */
      if (THREAD32) {
        if (skip == 0xffffffffu) walking = false;
        else node = skip;
      } else if (sp == 0) walking = false;
      else {
        --sp;
        node = PT_STACK_POP(stack, sp);
      }
    }
  }

  /* PT_OCT_BATCH_FALLBACK: the binary64 box test of every lane of the wave whose walk stepped out on an undecided filter test, together;
   * then the visit's select, as node_step would have made it (oct_link / oct_skip are still that visit's words) */
  __device__ __forceinline__ void resolve_pending(const PtSceneView& sv, unsigned long long& c_prims) {
    if (pending()) {
      const uint32_t nd = node & ~PT_OCT_PENDING;
      if (COUNT && pt_lane() == __ffsll((long long)__ballot(1)) - 1) n_wave_fallbacks++;
      const bool hit = slab64(sv.nodes + (nd - skip_off)); /* (the canonical node: the octant's base off again) */
      if (COUNT && PT_DIAG == 0 && hit && (oct_link >> 30) == 1u) {
        const uint32_t n_real = (oct_link >> PT_OCT_LEAF_FIRST_BITS) & PT_OCT_LEAF_REAL_MAX;
        c_prims += (unsigned long long)(MODE == PT_MODE_SIMD ? ((n_real + 3u) & ~3u) : n_real);
      }
      node = hit ? oct_link : oct_skip;
    }
  }
  /* the first slot of the leaf this lane holds (holds_leaf(), the LDS images), read where packet() reads it and nothing of the walk
   * touched: k_next_leaf_eval, which reports the leaf and never enters it */
  __device__ __forceinline__ int held_leaf_first(const PtSceneView& sv) const {
    static_assert(TAGGED || LOCT, "the LDS images' walks");
    if (LOCT) {
      const uint32_t rec = node & (PT_LOCT_LEAF_TAG - 1u);
      return (int)(*(const __attribute__((address_space(3))) uint32_t*)PT_LDS_AT(sv.oct_leaf + ((rec - skip_off) << 2)) & 0xffffu);
    }
    return (int)(lkx & 0xffffu);
  }
  /* Leaf.intersect on the held leaf (caller checks leaf_n > 0) */
  __device__ __forceinline__ void packet(const PtSceneView& sv, unsigned long long& c_nodes, unsigned long long& c_floor) {
    const double t_min = 0.0;
    if (TAGGED) { /* the leaf's word, as the visit that took it loaded it */
      leaf_first = (int)(lkx & 0xffffu);
      leaf_n = (int)(lkx >> 16);
      node &= ~PT_SWZ_TAG_LEAF; /* -> the node that follows the leaf, or PT_SWZ_END */
    }
    if (LOCT) { /* `node` names the leaf's own record: its packet from the leaf table, then on at the record's miss link */
      const uint32_t rec = node & (PT_LOCT_LEAF_TAG - 1u);
      const uint32_t lw = *(const __attribute__((address_space(3))) uint32_t*)PT_LDS_AT(sv.oct_leaf + ((rec - skip_off) << 2));
      leaf_first = (int)(lw & 0xffffu);
      leaf_n = (int)(lw >> 16);
      node = (uint32_t)*(const __attribute__((address_space(3))) uint16_t*)PT_LDS_AT(sv.oct_base + (rec << 5) + 26u);
    }
    if (OTAG) { /* `node` IS the leaf's word; the walk goes on where the leaf's miss link points */
      leaf_first = (int)(node & ((1u << PT_OCT_LEAF_FIRST_BITS) - 1u));
      leaf_n = (int)((node >> PT_OCT_LEAF_FIRST_BITS) & PT_OCT_LEAF_REAL_MAX);
      node = oct_skip;
    }
    if (MODE == PT_MODE_SIMD) {
      /* spheres_intersect_aux, lib.rs:102-178, one packet lane per step, split in two so the wave stays
       * dense: SCAN (cheap, every lane: f, c, b', discriminant) runs until the lane meets a slot whose
       * discriminant is >= +0; only then do the lanes that found one run the HEAVY part (sqrt, divide)
       * together.  Testing slot after slot in lockstep would execute ~50 sqrt/div instructions per slot with
       * one lane in eight active.  Slots are still visited in order, so `t <= t_found` ties resolve alike. */
      /* pass 1, lockstep over the slots: only the discriminant's sign; pass 2: the roots of the candidates, in slot
       * order.  The discriminant does not depend on the closest hit so far, so deferring the roots changes nothing. */
      for (int base = 0; base < leaf_n; base += 32) {
        const int m = (leaf_n - base) < 32 ? (leaf_n - base) : 32;
        uint32_t cand = 0;
        for (int k = 0; k < m; ++k) {
          if (COUNT && PT_DIAG == 3 && !ORIGIN_ZERO) {
            c_nodes++;
            PT_DIAG_WAVE_SLOTS(c_floor);
          }
          const double* s = sv.sph + (size_t)(leaf_first + base + k) * 4;
          const double fx = ORIGIN_ZERO ? s[0] : s[0] - o.x, fy = ORIGIN_ZERO ? s[1] : s[1] - o.y,
                       fz = ORIGIN_ZERO ? s[2] : s[2] - o.z;
          const double bp_over_a = pt_fma(fx, d.x, pt_fma(fy, d.y, fz * d.z)) * one_over_a;
          const double wx = pt_fma(d.x, bp_over_a, -fx);
          const double wy = pt_fma(d.y, bp_over_a, -fy);
          const double wz = pt_fma(d.z, bp_over_a, -fz);
          const double disc = (s[3] * s[3]) - pt_fma(wx, wx, pt_fma(wy, wy, wz * wz));
          /* "neither NaN nor sign bit set" (lib.rs:162-166) is ONE unsigned comparison of the bit pattern (+0 ... +inf), and the
           * candidate mask takes the outcome as the carry of cand + cand: two vector instructions instead of five; the mask
           * comes out in reverse order and is turned round once per leaf */
          {
            const unsigned long long fm = __builtin_amdgcn_ballot_w64((unsigned long long)__double_as_longlong(disc) <= 0x7ff0000000000000ull);
            unsigned long long co_;
            asm("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(cand), "=s"(co_) : "s"(fm));
          }
        }
        cand = __brev(cand) >> (32 - m); /* slot k -> bit k (m >= 1) */
        while (cand != 0) {
          if (COUNT && PT_DIAG == 4 && !ORIGIN_ZERO) {
            c_nodes++;
            PT_DIAG_WAVE_SLOTS(c_floor);
          }
          const int k = __ffs((int)cand) - 1;
          cand &= cand - 1u;
          const double* s = sv.sph + (size_t)(leaf_first + base + k) * 4;
          const double fx = ORIGIN_ZERO ? s[0] : s[0] - o.x, fy = ORIGIN_ZERO ? s[1] : s[1] - o.y,
                       fz = ORIGIN_ZERO ? s[2] : s[2] - o.z;
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
          if (!(t < t_min) && t <= r.t) {
            r.t = t;
            r.slot = leaf_first + base + k;
          }
        }
      }
    } else {
      /* Array_leaf.intersect, shape_tree.ml:299-311: shrinking t_max, later element wins ties */
      if (!SWZ && sv.kind == nullptr) {
        /* a triangle-only scene walked from HBM / L2 (a mesh): the leaf's triangles are 80-byte records that mostly miss
         * every cache level above L2, and testing them one after the other made a leaf visit a chain of up to
         * length_cutoff dependent round trips -- the longest waits of the whole walk.  The next triangle's nine
         * coordinates are requested before the current one is tested; same tests, same order. */
        const double* tv = sv.tri + (size_t)leaf_first * 10;
        V3 a = pt_load_v3(tv), b = pt_load_v3(tv + 3), c = pt_load_v3(tv + 6);
        for (int k = 0; k < leaf_n; ++k) {
          const double* nx = sv.tri + (size_t)(leaf_first + (k + 1 < leaf_n ? k + 1 : k)) * 10;
          const V3 na = pt_load_v3(nx), nb = pt_load_v3(nx + 3), nc = pt_load_v3(nx + 6);
          double t, u, v;
          if (pt_triangle_intersect(a, b, c, o, d, t_min, r.t, &t, &u, &v)) {
            r.t = t;
            r.u = u;
            r.v = v;
            r.slot = leaf_first + k;
          }
          a = na; b = nb; c = nc;
        }
        leaf_n = 0;
        if (FILT) update_t32();
        return;
      }
      for (int k = 0; k < leaf_n; ++k) {
        if (COUNT && PT_DIAG == 3 && !ORIGIN_ZERO) {
          c_nodes++;
          PT_DIAG_WAVE_SLOTS(c_floor);
        }
        const int slot = leaf_first + k;
        if (sv.kind[slot] == PT_SLOT_SPHERE) {
          const double* s = sv.sph + (size_t)slot * 4;
          double t;
          if (pt_sphere_intersect_scalar(v3(s[0], s[1], s[2]), s[3], o, d, t_min, r.t, &t)) {
            r.t = t;
            r.slot = slot;
          }
        } else {
          const double* tv = sv.tri + (size_t)slot * 10;
          double t, u, v;
          if (pt_triangle_intersect(pt_load_v3(tv), pt_load_v3(tv + 3), pt_load_v3(tv + 6), o, d, t_min, r.t, &t, &u,
                                    &v)) {
            r.t = t;
            r.u = u;
            r.v = v;
            r.slot = slot;
          }
        }
      }
    }
    leaf_n = 0;
    if (FILT) update_t32();
  }
};

/* Scene.intersect for ONE ray held by this lane, start to finish.
 * "while-while" traversal: every lane walks nodes until it reaches a leaf (or runs out of nodes); only then do the
 * lanes that hold a leaf test its packet TOGETHER.  Interleaving the two, as the recursive reference does, would
 * run the packet loop for one or two lanes at a time.  The order of node tests and packet tests of each individual
 * ray is unchanged. */
/* Tail cut (threaded LDS scenes only: the whole state of a walk in progress is the node it stands on, the closest hit so
 * far and its slot).  The wave stops a chunk once fewer than `min_active` of its rays are still walking; those rays are
 * not finished: the caller parks their state and resumes them later TOGETHER with the stragglers of its other chunks
 * (k_trace).  A resumed ray continues at `node` with `t` / `slot` restored, i.e. it performs exactly the box and packet
 * tests it had left, in the same order. */
struct PtTailCtl {
  int min_active;   /* in: stop when fewer rays than this are walking (0 = run to completion) */
  bool resume;      /* in: this lane continues a parked walk */
  uint32_t node;    /* in (resume) / out (unfinished): byte offset of the node to visit next */
  double t;         /* in (resume): closest hit so far */
  double u, v;      /* in (resume): its barycentrics (triangle scenes) */
  int slot;
  bool unfinished;  /* out: the ray is still walking */
};
template <int MODE, bool COUNT, bool ORIGIN_ZERO, typename StackT, bool SWZ = false, bool DIV_LOOP = false, bool ASM_WALK = false>
__device__ __forceinline__ PtTraceResult pt_trace_ray(const PtSceneDev& sc, const PtSceneView& sv, StackT* stack,
                                                      V3 o, V3 d, unsigned long long& c_nodes,
                                                      unsigned long long& c_prims, unsigned long long& c_floor,
                                                      bool valid = true, PtTailCtl* tc = nullptr,
                                                      unsigned long long* c_filter = nullptr) {
  PtTraverser<MODE, COUNT, ORIGIN_ZERO, StackT, SWZ> tr;
  constexpr int WALK_MIN = SWZ ? PT_WALK_MIN : PT_WALK_MIN_GLOBAL;
  unsigned long long no_count = 0; /* lanes without a ray run begin() on a dummy ray: keep them out of the counters */
  /* a resumed walk has had its floor pre-test (its outcome is part of the parked state): not counted again */
  tr.begin(sc, sv, o, d, (valid && !(tc && tc->resume)) ? c_floor : no_count);
  if (tc && tc->resume) {
    tr.node = tc->node;
    tr.r.t = tc->t;
    tr.r.u = tc->u;
    tr.r.v = tc->v;
    tr.r.slot = tc->slot;
    if (tr.FILT) tr.update_t32(); /* the filter's copy of t: stale, it would pass boxes beyond the restored hit */
  }
  while (valid && tr.alive()) {
    /* DIV_LOOP: the node walk as ONE divergent loop: a lane stays in it while it wants node steps, so the lanes still walking
     * are simply the loop's exec mask (no per-turn ballot of a `want` flag, no `continue`, no exit-reason bookkeeping: the
     * first version of this loop spent ~19 of its ~80 instructions per turn on that).  Same rule as below: once fewer than
     * PT_WALK_MIN lanes are walking and some lane holds a leaf, the pending packets are intersected first.  Half the SCALAR
     * instructions per turn: +3 % time in k_trace at 8 waves per SIMD (scalar issue is not what binds there), -1 % in k_bounce
     * at 4 (with half the waves, a wave busy with scalar bookkeeping is more often the one the vector pipe is waiting for). */
    if constexpr (ASM_WALK && (PT_WALK_ASM != 0) && (PT_DIAG == 0) && !COUNT && PtTraverser<MODE, COUNT, ORIGIN_ZERO, StackT, SWZ>::LOCT) {
#if PT_WALK_ASM
      while (tr.walk_asm_oct(sv.oct_base, WALK_MIN) != 0ull)
        if (tr.wants_node()) tr.node_step(sv, stack, c_nodes, c_prims);
#endif
    } else if constexpr (ASM_WALK && (PT_WALK_ASM != 0) && (PT_DIAG == 0) && !COUNT && PtTraverser<MODE, COUNT, ORIGIN_ZERO, StackT, SWZ>::TAGGED) {
#if PT_WALK_ASM
      /* the node loop in assembly; a visit the binary32 filter cannot decide for some lane is performed here, in binary64 */
      while (tr.walk_asm(WALK_MIN) != 0ull)
        if (tr.wants_node()) tr.node_step(sv, stack, c_nodes, c_prims);
#endif
    } else if constexpr (DIV_LOOP) {
     if (tr.wants_node()) {
      bool leaf_waiting = false; /* wave-uniform: a lane of this wave left the walk holding a leaf */
      /* TAGGED: "a lane has left the walk" instead (scalar: the loop's exec mask against the one it was entered with) -- a lane
       * leaves with a leaf or because its walk is over; when the few that are left come out and no leaf is waiting, the chunk cut
       * below looks at them a little earlier than it used to.  A change of schedule only: which tests a ray performs is its own affair */
      const unsigned long long entered = tr.TAGS ? __builtin_amdgcn_ballot_w64(true) : 0ull;
      for (;;) {
        if (COUNT && PT_DIAG == 1 && !ORIGIN_ZERO) PT_DIAG_WAVE_SLOTS(c_floor);
        tr.node_step(sv, stack, c_nodes, c_prims);
        if (!tr.TAGS && __ballot(tr.leaf_n > 0) != 0) leaf_waiting = true;
        if (!tr.wants_node()) break;
        const unsigned long long now = __builtin_amdgcn_ballot_w64(true);
        if (tr.TAGS) leaf_waiting = now != entered;
        if (leaf_waiting && pt_popc_mask(now) < WALK_MIN) break;
      }
     }
    } else {
    for (;;) {
      /* keep walking while enough lanes still want a node step; once fewer than PT_WALK_MIN do and some lane
       * already holds a leaf, intersect the pending packets first (the stragglers resume afterwards) */
      const unsigned long long wm = tr.wants_node_mask();
      if (wm == 0) break;
      if (pt_popc_mask(wm) < WALK_MIN && tr.holds_leaf_mask() != 0) break;
      if (COUNT && PT_DIAG == 1 && !ORIGIN_ZERO) PT_DIAG_WAVE_SLOTS(c_floor);
      if (!tr.wants_node()) continue;
      tr.node_step(sv, stack, c_nodes, c_prims);
    }
    }
    if (tr.OTAG && PT_OCT_BATCH_FALLBACK) tr.resolve_pending(sv, c_prims); /* (a lane it lets into a leaf takes part in the leaf phase below) */
    if (COUNT && PT_DIAG == 6 && !ORIGIN_ZERO) { /* (diagnostic build: ticks the wave spends in the leaf phase, into c_prims; lane 0's copy is kept) */
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long t0_ = __builtin_readcyclecounter();
      if (tr.holds_leaf()) tr.packet(sv, c_nodes, c_floor);
      __builtin_amdgcn_sched_barrier(0);
      c_prims += __builtin_readcyclecounter() - t0_;
    } else
    if (tr.holds_leaf()) tr.packet(sv, c_nodes, c_floor);
    /* nobody holds a leaf here: a safe place to stop.  The ballot sees the rays that are still walking (finished
     * lanes have left the loop), and every one of them sees the same count. */
    if (tc && pt_popc_mask(tr.walking_mask()) < tc->min_active) break;
  }
  if (tc) {
    tc->unfinished = valid && tr.alive(); /* (no lane holds a leaf here) */
    tc->node = tr.node;
  }
  if (COUNT && c_filter) {
    c_filter[0] += tr.n_undecided;
    c_filter[1] += tr.n_wave_fallbacks;
  }
#if PT_DIAG_VISIT_VALU || PT_DIAG_VISIT_LDS || PT_DIAG_VISIT_SALU
  if (tr.lkx_diag + tr.sdiag == 0xfffffff3u) tr.r.t = 0.0; /* (keeps the diagnostic's loads alive) */
#endif
  return tr.r;
}

/* (Round 5, measured and not kept -- profiles/r05_ab_packet_stack.txt: the shared stack below held in the LANES of three registers,
 * v_writelane on a push and v_readlane on a pop instead of the LDS round trip behind a fence and a wave barrier: bit-exact, and
 * +1.5 % on the headline and on cornell -- the camera rays' launches are bound by vector issue (0.85 busy) and the LDS pipe they
 * leave idle carried the stack for nothing; the node's words 6 / 7 handed to the lanes' box test instead of read again per lane: +-0.) */
/* Camera rays: the 64 rays of a wave are one 8x8 pixel tile of one pass, so they walk the tree TOGETHER -- one
 * shared stack of (node, lane mask) instead of 64 private ones.  A ray's own sequence of box tests and packet tests
 * is exactly pt_trace_ray's: its child order depends only on the signs of its direction (shape_tree.ml:201,209), the
 * wave is split into groups of equal signs (almost always one), a ray takes part in a node only if it hit the parent,
 * and a far child is tested when popped, against each ray's own closest hit.  What changes is the cost: node and
 * packet addresses are wave-uniform (LDS broadcasts, scalar control flow), no per-lane stack traffic, and the
 * packet loop runs in lockstep.  wstack: 3 words per level, shared by the wave. */
template <int MODE, bool COUNT, bool ORIGIN_ZERO, bool SWZ>
__device__ __forceinline__ PtTraceResult pt_trace_packet(const PtSceneDev& sc, const PtSceneView& sv, uint32_t* wstack,
                                                         bool valid, V3 o, V3 d, unsigned long long& c_nodes,
                                                         unsigned long long& c_prims, unsigned long long& c_floor,
                                                         unsigned long long* c_filter = nullptr) {
  const int lane = pt_lane();
  PtTraverser<MODE, COUNT, ORIGIN_ZERO, uint32_t, SWZ> tr;
  unsigned long long no_count = 0; /* lanes without a sample run begin() on a dummy ray: keep them out of the counters */
  tr.begin(sc, sv, valid ? o : v3(0.0, 0.0, 0.0), valid ? d : v3(0.0, 0.0, -1.0), valid ? c_floor : no_count);
  unsigned long long remaining = __ballot(valid && tr.alive());
  while (remaining != 0) {
    /* the lanes that share the first remaining lane's direction signs */
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)tr.dirs, __ffsll((long long)remaining) - 1);
    unsigned long long m = __ballot(tr.dirs == d0) & remaining;
    remaining &= ~m;
    uint32_t node = SWZ ? sv.swz_root : 0u;
    int sp = 0;
    bool act = (m >> lane) & 1ull; /* this lane takes part in `node` */
    for (;;) {
      /* the node's links: one address for the whole wave */
      uint32_t ua, ub, n_real;
      if (SWZ) { /* node = the node's absolute LDS address */
        const pt_u2 lk = *(const __attribute__((address_space(3))) pt_u2*)PT_LDS_AT(node + PT_SWZ_OFF_LINKS);
        const uint32_t w6 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lk.x);
        const uint32_t w7 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lk.y);
        ua = w6 & 0xffffu;
        ub = (w6 >> 16) | ((w7 & 3u) << 30);
        n_real = w6 >> 16;
      } else {
        const PtNode* np = sv.nodes + node;
        ua = (uint32_t)__builtin_amdgcn_readfirstlane((int)np->a);
        ub = (uint32_t)__builtin_amdgcn_readfirstlane((int)np->b);
        n_real = (uint32_t)__builtin_amdgcn_readfirstlane((int)np->pad[0]);
      }
      bool hit = false;
      if (act) {
        if (COUNT) c_nodes++;
        uint32_t x0, x1, x2;
        hit = tr.test_box(sv, node, x0, x1, x2);
      }
      const unsigned long long hm = __ballot(hit);
      bool descended = false;
      if (hm != 0) {
        const uint32_t axis = ub >> 30;
        if (axis == PT_NODE_LEAF_AXIS) {
          if (COUNT && hit) c_prims += (unsigned long long)(SWZ ? (MODE == PT_MODE_SIMD ? ((n_real + 3u) & ~3u) : n_real) : (ub & 0x3fffffffu));
          if (MODE == PT_MODE_SIMD) {
            /* spheres_intersect_aux (lib.rs:102-178) in lockstep: slot k of the packet for every ray that hit the
             * leaf's box; the roots only where a ray's discriminant is >= +0 (same order per ray as packet()) */
            const double t_min = 0.0;
            for (uint32_t k = 0; k < n_real; ++k) {
              const double* sp4 = sv.sph + (size_t)(ua + k) * 4;
              /* f = center - origin; for camera rays the origin is (+0, +0, +0) and x - (+0) == x bit for bit */
              const double fx = ORIGIN_ZERO ? sp4[0] : sp4[0] - tr.o.x, fy = ORIGIN_ZERO ? sp4[1] : sp4[1] - tr.o.y,
                           fz = ORIGIN_ZERO ? sp4[2] : sp4[2] - tr.o.z;
              const double r2 = sp4[3] * sp4[3];
              const double bp = pt_fma(fx, tr.d.x, pt_fma(fy, tr.d.y, fz * tr.d.z));
              const double bp_over_a = bp * tr.one_over_a;
              const double wx = pt_fma(tr.d.x, bp_over_a, -fx);
              const double wy = pt_fma(tr.d.y, bp_over_a, -fy);
              const double wz = pt_fma(tr.d.z, bp_over_a, -fz);
              const double disc = r2 - pt_fma(wx, wx, pt_fma(wy, wy, wz * wz));
              const bool found = hit && (disc == disc) && !pt_signbit(disc);
              if (__ballot(found) != 0) {
                if (found) {
                  const double c = pt_fma(fx, fx, pt_fma(fy, fy, fz * fz)) - r2;
                  const double q_rhs = pt_sqrt(tr.qa * disc);
                  const double qq = pt_signbit(bp) ? (bp - q_rhs) : (bp + q_rhs);
                  const double t = pt_signbit(c) ? (qq * tr.one_over_a) : (c / qq);
                  if (!(t < t_min) && t <= tr.r.t) {
                    tr.r.t = t;
                    tr.r.slot = (int)(ua + k);
                  }
                }
              }
            }
            if (SWZ) tr.update_t32();
          } else if (hit) {
            tr.leaf_first = (int)ua;
            tr.leaf_n = (int)n_real;
            tr.lkx = ua | (n_real << 16); /* (TAGGED: packet() decodes the leaf's word itself) */
            tr.packet(sv, c_nodes, c_floor);
          }
        } else {
          const uint32_t lhs = ua, rhs = ub & 0x3fffffffu;
          const bool lhs_first = (d0 >> axis) & 1u;
          if (lane == 0) {
            wstack[3 * sp] = lhs_first ? rhs : lhs;
            wstack[3 * sp + 1] = (uint32_t)hm;
            wstack[3 * sp + 2] = (uint32_t)(hm >> 32);
          }
          ++sp;
          node = lhs_first ? lhs : rhs;
          act = hit;
          descended = true;
        }
      }
      if (!descended) {
        if (sp == 0) break;
        --sp;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        node = (uint32_t)__builtin_amdgcn_readfirstlane((int)wstack[3 * sp]);
        const unsigned long long pm = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)wstack[3 * sp + 1]) |
                                      ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)wstack[3 * sp + 2]) << 32);
        act = (pm >> lane) & 1ull;
      }
    }
  }
  if (COUNT && c_filter) {
    c_filter[0] += tr.n_undecided;
    c_filter[1] += tr.n_wave_fallbacks;
  }
  return tr.r;
}

/* Where this workgroup traverses from.  LDS_SCENE: the whole tree and every leaf packet are first copied into LDS
 * behind the traversal stacks (nodes expanded to the swizzled image on the way); ends with a __syncthreads(). */
template <int MODE, bool LDS_SCENE, bool LOCT = false /* LDS_SCENE with the per-octant image in place of stacks + shared node image (PtLdsOctTag) */>
__device__ __forceinline__ PtSceneView pt_scene_view(const PtSceneDev& sc, unsigned char* lds_raw, int stack_depth, bool want_top = false) {
  const uint32_t waves_per_block = blockDim.x >> 6;
  PtSceneView sv;
  sv.nodes = sc.nodes;
  sv.skip32 = sc.node_skip32;
  sv.nodes32 = (const unsigned char*)sc.nodes32;
  sv.nodes32o = (const unsigned char*)sc.nodes32o;
  sv.n_nodes = (uint32_t)sc.n_nodes;
  sv.swz_nodes = nullptr;
  sv.swz_root = 0u;
  sv.top = lds_raw;
  sv.has_top = false;
  sv.floor_lds = nullptr;
  sv.n_floor_lds = 0;
  if (!LDS_SCENE && want_top && sc.n_top > 0) { /* the tree's top into LDS (the caller's barrier follows) */
    const uint4* src = (const uint4*)sc.top_nodes;
    uint4* dst = (uint4*)lds_raw;
    for (int k = threadIdx.x; k < sc.n_top * (PT_TOP_NODE_BYTES / 16); k += blockDim.x) dst[k] = src[k];
    sv.has_top = true;
    sv.skip32 = sc.node_skip32_top;
  }
  sv.sph = sc.sph;
  sv.tri = sc.tri;
  sv.kind = sc.slot_kind;
  sv.cat = sc.slot_cat;
  sv.nodes64 = nullptr;
  sv.oct_base = sv.oct_leaf = 0u;
  if (!LDS_SCENE && sc.all_triangles) sv.kind = nullptr; /* PtTraverser::packet: the pipelined triangle loop */
  if constexpr (LDS_SCENE && LOCT) {
    unsigned char *l_oct, *l_leaf, *l_sph, *l_cat, *l_nodes64, *l_end; /* pt_lds_layout.h, PT_LDS_OCT_REGIONS */
    const int total_slots = sc.n_slots + sc.n_floor;
#define PT_VIEW_AT(region, off_) l_##region = lds_raw + (off_)
    PT_LDS_OCT_REGIONS(PT_VIEW_AT, sc.n_nodes, total_slots, sc.lds_nodes64);
#undef PT_VIEW_AT
    (void)l_end;
    { /* records and leaf table as the host built them: one run of 16-byte words */
      const uint4* src = (const uint4*)sc.lds_oct;
      uint4* dst = (uint4*)l_oct;
      const int n16 = sc.n_nodes * 16 + (int)(PT_LOCT_LEAF_WORDS(sc.n_nodes) / 4u);
      for (int k = threadIdx.x; k < n16; k += blockDim.x) dst[k] = src[k];
    }
    {
      const uint4* src = (const uint4*)sc.sph;
      uint4* dst = (uint4*)l_sph;
      for (int k = threadIdx.x; k < total_slots * 2; k += blockDim.x) dst[k] = src[k];
    }
    for (int k = threadIdx.x; k < total_slots; k += blockDim.x) l_cat[k] = sc.slot_cat[k];
    if (sc.lds_nodes64)
      for (int k = threadIdx.x; k < sc.n_nodes * 3; k += blockDim.x)
        ((double2*)l_nodes64)[k] = ((const double2*)(sc.nodes + k / 3))[k % 3];
    __syncthreads();
    sv.oct_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)l_oct;
    sv.oct_leaf = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)l_leaf;
    sv.sph = (const double*)l_sph;
    sv.cat = l_cat;
    if (sc.lds_nodes64) sv.nodes64 = (const double*)l_nodes64;
  } else
  if (LDS_SCENE) {
    unsigned char *l_nodes, *l_sph, *l_tri, *l_kind, *l_cat, *l_nodes64, *l_end; /* the regions of the image: pt_lds_layout.h */
#define PT_VIEW_AT(region, off_) l_##region = lds_raw + (off_)
    PT_LDS_IMAGE_REGIONS(PT_VIEW_AT, MODE, waves_per_block, stack_depth, sc.n_nodes, sc.n_slots + sc.n_floor, sc.has_triangles, sc.lds_nodes64);
#undef PT_VIEW_AT
    (void)l_end;
    const int total_slots = sc.n_slots + sc.n_floor;
    /* nodes: the binary32 filter image (PT_SWZ_NODE_BYTES each); links become absolute LDS
     * addresses (layout 3 above) */
    const uint32_t nbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)l_nodes;
    for (int k = threadIdx.x; k < sc.n_nodes; k += blockDim.x) {
      const PtNode* src = sc.nodes + k;
      uint32_t* w = (uint32_t*)(l_nodes + (size_t)k * PT_SWZ_NODE_BYTES);
      float mag = 0.0f;
      for (int ax = 0; ax < 3; ++ax) {
        const float lo = (float)src->mn[ax], hi = (float)src->mx[ax];
        w[3 * ax] = __float_as_uint(lo);
        w[3 * ax + 1] = __float_as_uint(hi);
        w[3 * ax + 2] = __float_as_uint(lo);
        mag = __builtin_fmaxf(mag, __builtin_fmaxf(__builtin_fabsf(lo), __builtin_fabsf(hi)));
      }
      const uint32_t axis = src->b >> 30;
      const bool leaf = axis == PT_NODE_LEAF_AXIS;
      uint32_t* lk = w + PT_SWZ_OFF_LINKS / 4;
      lk[0] = leaf ? ((src->a & 0xffffu) | ((src->pad[0] & 0xffffu) << 16))
                   : ((nbase + src->a * PT_SWZ_NODE_BYTES) | ((nbase + (src->b & 0x3fffffffu) * PT_SWZ_NODE_BYTES) << 16));
      /* rounded up, then the two lowest mantissa bits carry the axis (a relative change below 2^-21, inside the slack) */
      lk[1] = ((__float_as_uint(mag * 1.000001f) + 4u) & ~3u) | axis;
      uint16_t* sk = (uint16_t*)((unsigned char*)w + PT_SWZ_OFF_SKIP);
      for (int o = 0; o < 8; ++o) {
        const uint32_t nx = sc.node_skip[(size_t)k * 8 + o];
        sk[o] = nx == 0xffffu ? (uint16_t)PT_SWZ_END : (uint16_t)(nbase + nx * PT_SWZ_NODE_BYTES);
        uint16_t* nr = (uint16_t*)((unsigned char*)w + PT_SWZ_OFF_NEAR);
        /* tagged links (PT_SWZ_TAG_*): a leaf's entry is what follows it, with "holds a leaf" set */
        nr[o] = leaf ? (uint16_t)(sk[o] | PT_SWZ_TAG_LEAF) : (uint16_t)(nbase + (((o >> axis) & 1) ? src->a : (src->b & 0x3fffffffu)) * PT_SWZ_NODE_BYTES);
      }
    }
    {
      const uint4* src = (const uint4*)sc.sph;
      uint4* dst = (uint4*)l_sph;
      for (int k = threadIdx.x; k < total_slots * 2; k += blockDim.x) dst[k] = src[k];
    }
    if (MODE == PT_MODE_ARRAY) {
      if (sc.has_triangles) {
        const uint4* src = (const uint4*)sc.tri;
        uint4* dst = (uint4*)l_tri;
        for (int k = threadIdx.x; k < total_slots * 5; k += blockDim.x) dst[k] = src[k];
      }
      for (int k = threadIdx.x; k < total_slots; k += blockDim.x) l_kind[k] = sc.slot_kind[k];
    }
    for (int k = threadIdx.x; k < total_slots; k += blockDim.x) l_cat[k] = sc.slot_cat[k];
    if (sc.lds_nodes64) /* (workgroup-uniform) mn.xyz, mx.xyz: the first 48 bytes of a PtNode */
      for (int k = threadIdx.x; k < sc.n_nodes * 3; k += blockDim.x)
        ((double2*)l_nodes64)[k] = ((const double2*)(sc.nodes + k / 3))[k % 3];
    __syncthreads();
    sv.swz_nodes = l_nodes;
    sv.swz_root = nbase;
    sv.sph = (const double*)l_sph;
    sv.tri = (const double*)l_tri;
    sv.kind = l_kind;
    sv.cat = l_cat;
    if (sc.lds_nodes64) sv.nodes64 = (const double*)l_nodes64;
  }
  return sv;
}

/* Dynamic hand-out of a launch's work units (64-ray chunks for trace, workgroup windows for shade).  A static
 * stride (unit = wave + k * n_waves) gave every wave ~28 units per launch whose costs differ several-fold (sky
 * against ground rows, 1 against 8 live bounces): the slowest wave ran ~1.7x the mean and a resident wave was alive
 * for only 62 % (trace) / 47 % (shade) of its kernel's duration (rocprofv3 SQ_WAVE_CYCLES against the kernel time,
 * profiles/r02a_sq.json).  The workgroup keeps its static share (chunks blockIdx, blockIdx + gridDim, ...) and its waves
 * take them from a counter in LDS: no global atomic (units dealt from up to 8 sharded global counters were this scheme's A/B
 * partner), and a workgroup's total is the sum of ~450 chunk costs instead of a wave's ~28, so the spread between
 * workgroups is a quarter of the spread between waves.  Wave-uniform. */
struct PtChunkFeed {
  uint32_t* ctr;
  uint32_t nc, c, limit, next, end;
  __device__ __forceinline__ void init(uint32_t total_units, uint32_t* lds_ctr) {
    nc = gridDim.x;
    c = blockIdx.x;
    limit = c < total_units ? (total_units - c + nc - 1u) / nc : 0u;
    next = end = 0u;
    ctr = lds_ctr; /* zeroed by the caller before a workgroup barrier */
  }
  __device__ __forceinline__ bool take(uint32_t& unit) {
    if (next >= end) {
      uint32_t k = 0u;
      if (pt_lane() == 0) k = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const uint32_t got = 1u;
      k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
      if (k >= limit) {
        next = end = limit;
        return false;
      }
      next = k;
      end = (k + got < limit) ? k + got : limit;
    }
    unit = next * nc + c;
    ++next;
    return true;
  }
};

/* ------------------------------------------------------------------ steps the walking kernels share
 * (k_trace, k_bounce, k_bounce_carry, k_walk_eval: each step is written here once; DESIGN.md section 4, "Shared protocols") */
/* two doubles <-> one 16-byte word {lo a, hi a, lo b, hi b} */
__device__ __forceinline__ uint4 pt_pack2(double a, double b) {
  return make_uint4((uint32_t)__double2loint(a), (uint32_t)__double2hiint(a), (uint32_t)__double2loint(b), (uint32_t)__double2hiint(b));
}
__device__ __forceinline__ double pt_unpack_lo(uint4 w) { return __hiloint2double((int)w.y, (int)w.x); }
__device__ __forceinline__ double pt_unpack_hi(uint4 w) { return __hiloint2double((int)w.w, (int)w.z); }
/* {x, y, t} and {t, x, y}: one double and two plain words */
__device__ __forceinline__ uint4 pt_pack_xy_t(uint32_t x, uint32_t y, double t) { return make_uint4(x, y, (uint32_t)__double2loint(t), (uint32_t)__double2hiint(t)); }
__device__ __forceinline__ uint4 pt_pack_t_xy(double t, uint32_t x, uint32_t y) { return make_uint4((uint32_t)__double2loint(t), (uint32_t)__double2hiint(t), x, y); }

/* A parked walk (PtTailCtl, and the closest hit so far) as 16-byte words:
 *   head {queue index, node | slot << 16, t}   an LDS image has < 65536 nodes and slots; slot 0xffff = none yet
 *   uv   {u, v}                                Array_leaf scenes: the triangle hit's barycentrics
 *   w    {node, slot, -, -}                    the walk from HBM / L2 (WIDE): both as 32-bit words, head's packed word then unused
 * k_bounce_carry's record has the same packed word in front of its own fields (its ray is nowhere in memory). */
__device__ __forceinline__ uint32_t pt_tail_node_slot(uint32_t node, int slot) { return node | ((uint32_t)(slot < 0 ? 0xffff : slot) << 16); }
__device__ __forceinline__ uint32_t pt_tail_node_of(uint32_t w) { return w & 0xffffu; }
__device__ __forceinline__ int pt_tail_slot_of(uint32_t w) { return (int)(w >> 16) == 0xffff ? -1 : (int)(w >> 16); }
__device__ __forceinline__ uint4 pt_tail_head(uint32_t i, uint32_t node, int slot, double t) { return pt_pack_xy_t(i, pt_tail_node_slot(node, slot), t); }
__device__ __forceinline__ uint4 pt_tail_wide(uint32_t node, int slot) { return make_uint4(node, (uint32_t)slot, 0u, 0u); }
/* (the way back is spelled field by field at its three users, tc.node = WIDE ? w.x : pt_tail_node_of(head.y) ...: one function that
 * fills a PtTailCtl compiles the non-counting k_trace and k_walk_eval to other code than the same statements in place) */

/* The lane's ray for entry i of a chunk: declares o and d, the camera sample's ray (PRIMARY) or the queue's, and clears `valid` where
 * the lane has none; such a lane holds P3.origin and -z.  A hole of the queue (pt_is_hole) is no ray: ON_HOLE is what the kernel
 * does about it besides (k_trace notes PT_SLOT_HOLE for the shade launch to drop; k_bounce nothing).
 * A macro like PT_STAGE_FLOOR below, for the same reason as PT_SHARE_*: as an inlined function (reference outputs, or a struct
 * returned) the non-counting k_trace instantiations come out with other code and up to 8 more bytes of scratch. */
#define PT_CHUNK_RAY(PRIMARY, sc, g, alpha, q, i, valid, o, d, ON_HOLE) \
  V3 o = v3(0.0, 0.0, 0.0), d = v3(0.0, 0.0, -1.0); /* P3.origin */ \
  if (valid) { \
    if (PRIMARY) { \
      const PtPrimarySample ps = pt_primary_decode(g, i); \
      valid = ps.valid; \
      if (valid) d = pt_primary_dir(sc, g, ps, alpha); \
    } else { \
      pt_q_load_ray(q, i, o, d); \
      if (pt_is_hole(d.x)) { /* never parked, so never seen on resume */ \
        valid = false; \
        ON_HOLE; \
        o = v3(0.0, 0.0, 0.0); \
        d = v3(0.0, 0.0, -1.0); \
      } \
    } \
  }

/* Scenes walked from HBM / L2: the pre-tested floor triangles (PtSceneView.floor_lds) into the workgroup's `lds_floor`, then the
 * barrier pt_scene_view leaves out when it copies nothing. */
#define PT_STAGE_FLOOR(MODE, sc, sv, lds_floor) do { \
    if (MODE == PT_MODE_ARRAY && sc.n_floor > 0) { \
      sv.n_floor_lds = sc.n_floor < PT_FLOOR_LDS ? sc.n_floor : PT_FLOOR_LDS; \
      sv.floor_lds = (const __attribute__((address_space(3))) double*)lds_floor; \
      for (int k = threadIdx.x; k < sv.n_floor_lds * 10; k += blockDim.x) lds_floor[k] = sc.tri[(size_t)sc.n_slots * 10 + k]; \
    } \
    __syncthreads(); \
  } while (0)

/* A wave's work counters (count_work) into the launch's: one sum over the wave and one atomic per counter. */
__device__ __forceinline__ void pt_counters_flush(PtCounters* counters, unsigned long long c_nodes, unsigned long long c_prims, unsigned long long c_floor,
                                                  unsigned long long c_seg, const unsigned long long* c_filter) {
  c_nodes = pt_wave_sum(c_nodes);
  c_prims = pt_wave_sum(c_prims);
  c_floor = pt_wave_sum(c_floor);
  c_seg = pt_wave_sum(c_seg);
  const unsigned long long f0 = pt_wave_sum(c_filter[0]), f1 = pt_wave_sum(c_filter[1]);
  if (pt_lane() == 0) {
    atomicAdd(&counters->nodes, c_nodes);
    atomicAdd(&counters->prims, c_prims);
    atomicAdd(&counters->floor, c_floor);
    atomicAdd(&counters->segments, c_seg);
    atomicAdd(&counters->undecided, f0);
    atomicAdd(&counters->fallback_steps, f1);
  }
}

/* Where a wave's life goes (diagnostic builds, tools/diag_phases.py): tick(var) adds the time since the last tick to var, in ticks
 * of the 100 MHz clock.  ON = false (every default build): nothing. */
template <bool ON>
struct PtPhaseClock {
  unsigned long long last, begin;
  __device__ __forceinline__ void start() { last = begin = ON ? __builtin_readcyclecounter() : 0ull; }
  __device__ __forceinline__ void tick(unsigned long long& var) {
    if (ON) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long now = __builtin_readcyclecounter();
      var += now - last;
      last = now;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __device__ __forceinline__ unsigned long long life() const { return last - begin; }
};

/* The traverse + intersect stage.  PRIMARY: bounce 0, rays come from the sampler + camera, not from a queue.
 * LDS_SCENE: the whole tree and every leaf packet are first copied into LDS (small scenes: Shirley is
 * 22 KB of nodes + 22 KB of packets), so node / packet reads are ds_read_b128 instead of L1 traffic.
 * LDS layout: [traversal stacks: waves x depth x 64 u32][nodes][sphere slots][triangle slots][slot kinds] */
#ifndef PT_TRACE_GLOBAL_WAVES
#define PT_TRACE_GLOBAL_WAVES 4
#endif
/* (PT_TAIL_CUT, PT_TAIL_CUT_GLOBAL: pt_lds_layout.h -- the parked walks' room depends on them) */
#ifndef PT_TRACE_BLOCK_LDS
#define PT_TRACE_BLOCK_LDS 1024 /* workgroup size when the scene is copied to LDS (one copy per workgroup) */
#endif
#ifndef PT_TRACE_BLOCK_LDS_ARRAY
#define PT_TRACE_BLOCK_LDS_ARRAY 512 /* Array_leaf kernels need ~106 VGPRs (4 waves per SIMD either way): cornell +6.6 % over 1024 */
#endif
#define PT_TRACE_BLOCK_OF(MODE, LDS_SCENE) \
  ((LDS_SCENE) ? ((MODE) == PT_MODE_SIMD ? PT_TRACE_BLOCK_LDS : PT_TRACE_BLOCK_LDS_ARRAY) : PT_TRACE_BLOCK_GLOBAL)
#ifndef PT_TRACE_LDS_WAVES
#define PT_TRACE_LDS_WAVES 8 /* Simd_leaf only: waves per SIMD asked of the register allocator */
#endif
#ifndef PT_TRACE_BLOCK_GLOBAL
#define PT_TRACE_BLOCK_GLOBAL 256 /* workgroup size when the scene is traversed from HBM/L2 (512: -6 % on ganesha-like) */
#endif
template <int MODE, bool COUNT, bool PRIMARY, bool LDS_SCENE, bool PACKET>
/* Simd_leaf + LDS scene fits 64 VGPRs without spilling: ask for 2 x 1024-thread workgroups per CU.  The Array_leaf
 * variants (triangle / scalar-sphere code) need ~100 VGPRs: forcing 64 would spill to scratch (1.5 GB of HBM
 * writes per launch on cornell). */
__global__ __launch_bounds__(PT_TRACE_BLOCK_OF(MODE, LDS_SCENE), (LDS_SCENE && MODE == PT_MODE_SIMD) ? PT_TRACE_LDS_WAVES : PT_TRACE_GLOBAL_WAVES) void k_trace(PtSceneDev sc, PtQueue q, PtHits hits, int stack_depth,
                                               PtCounters* counters, PtGenParams g, const double* __restrict__ alpha,
                                               uint32_t n_primary, uint32_t* work, uint4* susp, int top_in_lds) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  const int lane = pt_lane();
  const int wave_in_block = (int)(threadIdx.x >> 6);
  /* LDS-resident scenes have < 65536 nodes: 16-bit stack entries halve the stack footprint */
  /* no per-lane stack anywhere: both walks are threaded.  PACKET on a scene walked from HBM / L2 (where wave packets do not
   * pay) selects the per-octant node image instead (PtThreadOctTag; the host launches it when PtSceneDev.nodes32o exists) */
  typedef typename std::conditional<LDS_SCENE, uint16_t, typename std::conditional<PACKET, PtThreadOctTag, PtThreadTag>::type>::type StackT;
  StackT* stack = (StackT*)(lds_raw + (size_t)wave_in_block * PT_WAVE_STACK_BYTES(LDS_SCENE, stack_depth));
  __shared__ uint32_t lds_chunk_ctr;
  if (threadIdx.x == 0) lds_chunk_ctr = 0u;
  PtSceneView sv = pt_scene_view<MODE, LDS_SCENE>(sc, lds_raw, stack_depth, top_in_lds != 0);
  if (!LDS_SCENE) {
    __shared__ double lds_floor[PT_FLOOR_LDS * 10];
    PT_STAGE_FLOOR(MODE, sc, sv, lds_floor);
  }
  const uint32_t n = PRIMARY ? n_primary : *q.count;
  PtChunkFeed feed;
  feed.init((uint32_t)(((unsigned long long)n + PT_WAVE - 1) / PT_WAVE), &lds_chunk_ctr);
  uint32_t chunk;
  unsigned long long c_nodes = 0, c_prims = 0, c_floor = 0, c_seg = 0, c_filter[2] = {0, 0};

  if (PACKET && LDS_SCENE) { /* the 64 rays of the wave walk the tree together (pt_trace_packet) */
    /* the wave's private stack area (stack_depth x 64 entries) holds the shared (node, mask) stack: 12 B per level */
    uint32_t* wstack = (uint32_t*)(lds_raw + (size_t)wave_in_block * PT_WAVE_STACK_BYTES(LDS_SCENE, stack_depth));
    while (feed.take(chunk)) {
      const uint32_t i = chunk * PT_WAVE + lane;
      bool valid = i < n;
      PT_CHUNK_RAY(PRIMARY, sc, g, alpha, q, i, valid, o, d, hits.slot[i] = PT_SLOT_HOLE);
      if (COUNT && valid) c_seg++;
      const PtTraceResult r = pt_trace_packet<MODE, COUNT, PRIMARY, LDS_SCENE>(sc, sv, wstack, valid, o, d, c_nodes, c_prims, c_floor, c_filter);
      if (valid) {
        pt_hit_store(hits, i, r.t, r.slot, r.u, r.v, MODE == PT_MODE_ARRAY && sc.has_triangles);
      }
    }
  } else {
    /* One ray per lane; on LDS scenes the wave-level node loop with a `want` ballot per turn (the divergent loop has fewer scalar
     * instructions per turn, but k_trace is bound by VECTOR issue there: measured 3 % slower).
     * TAIL: see PtTailCtl -- a chunk ends when fewer than PT_TAIL_CUT of its rays are still walking;
     * their states (16 bytes each) go to this wave's list in `susp` and once 64 - PT_TAIL_CUT have gathered the wave walks
     * them as a chunk of their own.  tools/sim_coherence.py: 0.527 -> 0.435 wave steps per ray at 16. */
    constexpr int CUT = LDS_SCENE ? PT_TAIL_CUT : PT_TAIL_CUT_GLOBAL;
    constexpr bool TAIL = CUT > 0 && PT_DIAG == 0; /* both walks are threaded (LDS image, HBM / L2); a parked camera ray is recomputed from its index */
    constexpr bool TAIL_UV = TAIL && MODE == PT_MODE_ARRAY; /* triangle hits carry barycentrics: a second 16 bytes per state */
    constexpr bool TAIL_W = TAIL && !LDS_SCENE;            /* 32-bit node index and slot: a third 16 bytes */
    uint4* my_susp = TAIL ? susp + ((size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block) * (PT_WAVE * 3) : nullptr;
    uint32_t n_susp = 0; /* wave-uniform */
    bool more = true;
    for (;;) { /* no `continue` past a point where lanes have diverged: take() is wave-uniform */
      bool resume = false, valid = false;
      uint32_t i = 0;
      uint4 parked = make_uint4(0, 0, 0, 0), parked_uv = make_uint4(0, 0, 0, 0), parked_w = make_uint4(0, 0, 0, 0);
      if (TAIL && (n_susp > (uint32_t)(PT_WAVE - CUT) || (!more && n_susp > 0))) {
        resume = true;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); /* this wave's own parked states, written below */
        valid = (uint32_t)lane < n_susp;
        if (valid) parked = my_susp[lane];
        if (TAIL_UV && valid) parked_uv = my_susp[PT_WAVE + lane];
        if (TAIL_W && valid) parked_w = my_susp[2 * PT_WAVE + lane];
        i = parked.x;
        n_susp = 0;
      } else {
        if (!more) break;
        more = feed.take(chunk);
        if (more) {
          i = chunk * PT_WAVE + lane;
          valid = i < n;
        }
      }
      PT_CHUNK_RAY(PRIMARY, sc, g, alpha, q, i, valid, o, d, hits.slot[i] = PT_SLOT_HOLE);
      if (COUNT && valid && !resume) c_seg++;
      const unsigned long long diag_n0 = c_nodes;
      PtTailCtl tc;
      tc.min_active = (TAIL && more) ? CUT : 0; /* the last chunks of a wave run to completion */
      tc.resume = resume && valid;
      tc.node = TAIL_W ? parked_w.x : pt_tail_node_of(parked.y);
      tc.slot = TAIL_W ? (int)parked_w.y : pt_tail_slot_of(parked.y);
      tc.t = pt_unpack_hi(parked);
      tc.u = pt_unpack_lo(parked_uv);
      tc.v = pt_unpack_hi(parked_uv);
      tc.unfinished = false;
      /* every lane goes in (wave-level ballots inside); lanes without a ray commit nothing */
      /* (the node loop as one divergent loop where the kernel runs at 4 waves per SIMD: the walk from HBM / L2 -- ganesha-like
       * frame 35.4 -> 33.6 ms; the LDS walk at 8 waves per SIMD loses 3 % with it) */
      const PtTraceResult r = pt_trace_ray<MODE, COUNT, PRIMARY, StackT, LDS_SCENE, /* DIV_LOOP */ !LDS_SCENE>(sc, sv, stack, o, d, c_nodes, c_prims, c_floor, valid, TAIL ? &tc : nullptr, c_filter);
      if (COUNT && PT_DIAG == 2 && !PRIMARY && valid) {
        unsigned long long m = c_nodes - diag_n0;
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long other = __shfl_xor(m, off);
          m = other > m ? other : m;
        }
        PT_DIAG_WAVE_SLOTS(c_floor);
        if (lane == 0) c_floor += m * 64 - 64;
      }
      const bool park = TAIL && tc.unfinished;
      if (valid && !park) {
        pt_hit_store(hits, i, r.t, r.slot, r.u, r.v, MODE == PT_MODE_ARRAY && sc.has_triangles);
      }
      if (TAIL) {
        const unsigned long long pm = __ballot(park);
        if (pm != 0) {
          if (park) {
            const uint32_t k = n_susp + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
            my_susp[k] = pt_tail_head(i, tc.node, r.slot, r.t);
            if (TAIL_W) my_susp[2 * PT_WAVE + k] = pt_tail_wide(tc.node, r.slot);
            if (TAIL_UV) my_susp[PT_WAVE + k] = pt_pack2(r.u, r.v);
          }
          n_susp += (uint32_t)__popcll(pm);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
      }
    }
  }
  if (COUNT) pt_counters_flush(counters, c_nodes, c_prims, c_floor, c_seg, c_filter);
}

/* ------------------------------------------------------------------ shade */
/* (Quat, pt_shader_rotation and pt_tri_normal: pt_vec.h -- the host computes tri_frame and the light table with them) */
/* Quaternion.mul (quaternion.ml:25-32) */
__device__ __forceinline__ Quat pt_quat_mul(Quat a, Quat b) {
  Quat o;
  o.r = (a.r * b.r) - v3_dot(a.v, b.v);
  o.v = v3_add(v3_add(v3_cross(a.v, b.v), v3_scale(b.v, a.r)), v3_scale(a.v, b.r));
  return o;
}
/* Quaternion.transform t v = ((t * (0, v)) * conj t).v (quaternion.ml:34-42) */
__device__ __forceinline__ V3 pt_quat_transform(Quat t, V3 v) {
  Quat p;
  p.r = 0.0;
  p.v = v;
  Quat c;
  c.r = t.r;
  c.v = v3_neg(t.v);
  return pt_quat_mul(pt_quat_mul(t, p), c).v;
}
__device__ __forceinline__ Quat pt_quat_conj(Quat q) {
  Quat c;
  c.r = q.r;
  c.v = v3_neg(q.v);
  return c;
}

/* What a segment needs of its slot's shading record (PtShadeRec), in registers: every address is known the moment the segment
 * starts (queue index and hit slot), so everything is requested in one round (pt_shade_entry) instead of field by field where
 * the code needs it.  Which fields are read is fixed by the category when the kernel is specialised for one. */
struct PtMatRegs {
  int kind, tex_kind, tex_w, tex_h;
  double index;
  V3 even, odd, emit;
};
/* IMG (scenes with an image or an environment only): a slot of the textured-Lambertian category may carry an image (PT_TEX_IMAGE),
 * so its texture kind is read, not known */
template <int CAT, bool EMIT, bool IMG = false>
__device__ __forceinline__ PtMatRegs pt_mat_load(const PtShadeRec* m) {
  PtMatRegs r;
  r.kind = (CAT == PT_CAT_LAMBERT_SOLID || CAT == PT_CAT_LAMBERT_CHECKER) ? 0 : (CAT == PT_CAT_METAL ? 1 : (CAT == PT_CAT_DIELECTRIC ? 2 : m->kind));
  r.tex_kind = CAT == PT_CAT_LAMBERT_SOLID ? 0 : ((CAT == PT_CAT_LAMBERT_CHECKER && !IMG) ? 1 : (CAT == PT_CAT_DIELECTRIC ? 0 : m->tex_kind));
  const bool tex = CAT != PT_CAT_DIELECTRIC;
  const bool checker = CAT != PT_CAT_DIELECTRIC && CAT != PT_CAT_LAMBERT_SOLID;
  r.tex_w = checker ? m->tex_w : 1;
  r.tex_h = checker ? m->tex_h : 1;
  r.index = (CAT == PT_CAT_DIELECTRIC || CAT == PT_CAT_NONE) ? m->index : 1.0;
  r.even = tex ? v3(m->even[0], m->even[1], m->even[2]) : v3(0.0, 0.0, 0.0);
  r.odd = checker ? v3(m->odd[0], m->odd[1], m->odd[2]) : v3(0.0, 0.0, 0.0);
  r.emit = EMIT ? v3(m->emit[0], m->emit[1], m->emit[2]) : v3(0.0, 0.0, 0.0);
  return r;
}

/* ------------------------------------------------------------------ image textures (include/ptx.h states the rule; every expression
 * below keeps its grouping, and the build has -ffp-contract=off) */
/* p = u * W of the rule: a product that is NaN or reaches 2^62 in magnitude counts as 0 */
__device__ __forceinline__ double pt_image_scale(double u, int n) {
  const double p = u * (double)n;
  return pt_fabs(p) < 0x1p62 ? p : 0.0;
}
/* wrap of the rule for an index given as the integer-valued double i (|i| <= 2^62), 1 <= n <= 16384, without a 64-bit division (the
 * GPU has no integer divide: a 64-bit one is ~100 instructions and a dozen registers, in kernels held to 128 VGPRs).
 *   clamp   min(max(i, 0), n - 1), taken on the double: exact.
 *   repeat  ((i % n) + n) % n with C's truncating % is m for i >= 0 and (n - m) % n for i < 0, m = |i| mod n.  |i| < 2^32 -- every
 *           coordinate a scene produces -- is one 32-bit remainder; beyond it (a rare, cold branch) |i| = hi 2^32 + lo and
 *           m = ((hi mod n) (2^32 mod n) + lo mod n) mod n, every product below 2^28. */
__device__ __forceinline__ int pt_image_wrap(double i, int n, bool repeat) {
  if (!repeat) {
    const double last = (double)(n - 1);
    return (int)(i < 0.0 ? 0.0 : (i > last ? last : i));
  }
  const double a = pt_fabs(i);
  const uint32_t un = (uint32_t)n;
  uint32_t m;
  if (__builtin_expect(a < 0x1p32, 1)) {
    m = (uint32_t)a % un;
  } else {
    const unsigned long long big = (unsigned long long)a;
    const uint32_t hi = (uint32_t)(big >> 32), lo = (uint32_t)big;
    const uint32_t two32 = (0xffffffffu % un + 1u) % un; /* 2^32 mod n */
    m = ((hi % un) * two32 + lo % un) % un;
  }
  return (int)((i < 0.0 && m != 0u) ? un - m : m);
}
/* wrap(i + 1) from i0 = wrap(i): repeat steps round the axis; clamp stays at 0 for i < 0 (then i + 1 <= 0) and stops at n - 1 */
__device__ __forceinline__ int pt_image_next(double i, int i0, int n, bool repeat) {
  if (repeat) return i0 + 1 == n ? 0 : i0 + 1;
  return i < 0.0 ? 0 : (i0 + 1 > n - 1 ? n - 1 : i0 + 1);
}
/* texels: 32-byte records {r, g, b, -}.  All loads of a lookup are issued together, before the first use: two 16-byte loads for
 * nearest, eight for bilinear -- the texel address depends on the tex coords, so this is the shade step's second dependent round
 * trip, and its last. */
__device__ __forceinline__ V3 pt_image_eval(const double* __restrict__ texels, int w, int h, int flags, double u, double v) {
  const bool rep_u = (flags & PT_IMAGE_REPEAT_U) != 0, rep_v = (flags & PT_IMAGE_REPEAT_V) != 0;
  const double p = pt_image_scale(u, w), q = pt_image_scale(v, h);
  const double2* t = (const double2*)texels;
  if (!(flags & PT_IMAGE_BILINEAR)) {
    const int ix = pt_image_wrap(__builtin_trunc(p), w, rep_u), iy = pt_image_wrap(__builtin_trunc(q), h, rep_v); /* (long long)p */
    const double2* c = t + 2u * (uint32_t)(iy * w + ix);
    const double2 c0 = c[0], c1 = c[1];
    return v3(c0.x, c0.y, c1.x);
  }
  const double x = p - 0.5, y = q - 0.5;
  const double x0 = __builtin_floor(x), y0 = __builtin_floor(y);
  const double fx = x - x0, fy = y - y0;
  const int ix0 = pt_image_wrap(x0, w, rep_u), iy0 = pt_image_wrap(y0, h, rep_v);
  const int ix1 = pt_image_next(x0, ix0, w, rep_u), iy1 = pt_image_next(y0, iy0, h, rep_v);
  const uint32_t row0 = (uint32_t)(iy0 * w), row1 = (uint32_t)(iy1 * w);
  const double2 *p00 = t + 2u * (row0 + (uint32_t)ix0), *p10 = t + 2u * (row0 + (uint32_t)ix1);
  const double2 *p01 = t + 2u * (row1 + (uint32_t)ix0), *p11 = t + 2u * (row1 + (uint32_t)ix1);
  const double2 a0 = p00[0], a1 = p00[1], b0 = p10[0], b1 = p10[1], c0 = p01[0], c1 = p01[1], d0 = p11[0], d1 = p11[1];
  const V3 c00 = v3(a0.x, a0.y, a1.x), c10 = v3(b0.x, b0.y, b1.x), c01 = v3(c0.x, c0.y, c1.x), c11 = v3(d0.x, d0.y, d1.x);
  const V3 top = v3_lerp(fx, c00, c10), bot = v3_lerp(fx, c01, c11);
  return v3_lerp(fy, top, bot);
}

/* Texture.eval (texture.ml:16-31); IMG: and the image arm (PtShadeRec: the texels' address and the flags in the bits of `even`) */
template <bool IMG = false>
__device__ __forceinline__ V3 pt_texture_eval(const PtMatRegs& t, double u, double v) {
  if (IMG && t.tex_kind == PT_TEX_IMAGE)
    return pt_image_eval((const double*)(uintptr_t)__double_as_longlong(t.even.x), t.tex_w, t.tex_h, (int)__double_as_longlong(t.even.y), u, v);
  if (t.tex_kind == 0) return t.even;
  const double width = (double)(t.tex_w - 1), height = (double)(t.tex_h - 1);
  const double xp = u * width, yp = v * height;
  const long long px = ((long long)xp) & 1, py = ((long long)yp) & 1; /* Float.to_int a land 1 */
  if (px == py) return t.even;
  return t.odd;
}

/* schlick_reflectance (material.ml:16-20) */
__device__ __forceinline__ double pt_schlick(double cos_theta, double index) {
  const double qd = (1.0 - index) / (1.0 + index);
  const double r0 = qd * qd;
  return r0 + ((1.0 - r0) * pt_pow5(1.0 - cos_theta));
}

/* the environment (include/ptx.h): Sphere.tex_coord of the rotated unit direction, then the image rule, repeat in u, clamp in v */
__device__ __forceinline__ V3 pt_environment(const PtSceneDev& sc, V3 dir) {
  const double pi = 3.14159265358979323846;
  const V3 e = v3_normalize(dir);
  const double* R = sc.env_rot;
  const double mx = (R[0] * e.x + R[1] * e.y) + R[2] * e.z;
  const double my = (R[3] * e.x + R[4] * e.y) + R[5] * e.z;
  const double mz = (R[6] * e.x + R[7] * e.y) + R[8] * e.z;
  const double one_over_pi = 1.0 / pi, one_over_two_pi = 1.0 / (2.0 * pi);
  const double cy = my < -1.0 ? -1.0 : (my > 1.0 ? 1.0 : my); /* min(max(m.y, -1), 1); a NaN stays (acos gives NaN, which counts as v = 0) */
  const double u = (pi + pt_atan2(-mz, mx)) * one_over_two_pi;
  const double v = pt_acos(-cy) * one_over_pi;
  return pt_image_eval(sc.env, sc.env_w, sc.env_h, (sc.env_flags & PT_IMAGE_BILINEAR) | PT_IMAGE_REPEAT_U, u, v);
}
/* Scene.background (shirley_spheres/bin/main.ml:104-110); IMG: and the environment arm */
template <bool IMG = false>
__device__ __forceinline__ V3 pt_background(const PtSceneDev& sc, V3 dir) {
  if (IMG && sc.bg_kind == PT_BG_ENV) return pt_environment(sc, dir);
  if (sc.bg_kind == 0) return v3(0.0, 0.0, 0.0);
  const V3 d = v3_normalize(dir);
  const double t = 0.5 * (v3_dot(d, v3(0.0, 1.0, 0.0)) + 1.0);
  return v3_lerp(t, v3(sc.bg_horizon[0], sc.bg_horizon[1], sc.bg_horizon[2]),
                 v3(sc.bg_zenith[0], sc.bg_zenith[1], sc.bg_zenith[2]));
}

/* What Sphere.hit (sphere.ml:56-69) / Triangle.Hit.to_hit (triangle.ml:43-64) build: the local geometry of a hit
 * and what Material.scatter's partial application captures. */
struct PtSurface {
  V3 point, normal; /* Shader_space.world_origin / world_normal */
  Quat rot;         /* Shader_space.rotation */
  V3 omega_i;       /* Shader_space.omega_i */
  double tu, tv;    /* Texture.Coord */
  bool hit_front;
};
/* geometry of the hit slot requested together with the rest of the segment's inputs (pt_shade_entry): the sphere's record on
 * scenes without triangles; with triangles the slot's kind, which decides what to fetch in a second round */
struct PtSlotGeom {
  double cx, cy, cz;
  int kind; /* PT_SLOT_* */
};
/* (the photon passes' form: one ray at a time, nothing to batch the loads with) */
__device__ __forceinline__ PtSlotGeom pt_slot_geom(const PtSceneDev& sc, int slot) {
  PtSlotGeom g;
  g.cx = g.cy = g.cz = 0.0;
  g.kind = sc.has_triangles ? (int)sc.slot_kind[slot] : PT_SLOT_SPHERE;
  if (!sc.has_triangles) {
    const double* s = sc.sph + (size_t)slot * 4;
    g.cx = s[0];
    g.cy = s[1];
    g.cz = s[2];
  }
  return g;
}
/* CAT: the shading category when the caller knows it at compile time (per-category shade kernels), PT_CAT_NONE when it
 * has to be read from the slot's record */
template <int CAT = PT_CAT_NONE>
__device__ __forceinline__ PtSurface pt_surface_hit(const PtSceneDev& sc, V3 o, V3 d, int slot, double t_hit, double bu,
                                                    double bv, const PtMatRegs& m, const PtSlotGeom& geom) {
  const double pi = 3.14159265358979323846;
  PtSurface sf;
  sf.tu = 0.0;
  sf.tv = 0.0;
  /* tex_coord feeds Texture.eval only, and only a checker reads it */
  const bool need_uv = CAT == PT_CAT_LAMBERT_SOLID || CAT == PT_CAT_DIELECTRIC ? false
                       : (CAT == PT_CAT_LAMBERT_CHECKER ? true : ((m.kind != 2) && (m.tex_kind != 0)));
  if (geom.kind == PT_SLOT_SPHERE) {
    /* Sphere.hit (sphere.ml:56-69) */
    V3 center = v3(geom.cx, geom.cy, geom.cz);
    if (sc.has_triangles) { /* (mixed scenes learn the slot's kind in the first round and fetch its geometry in a second) */
      const double* s = sc.sph + (size_t)slot * 4;
      center = v3(s[0], s[1], s[2]);
    }
    sf.point = v3_add(o, v3_scale(d, t_hit)); /* Ray.point_at, ray.ml:15 */
    V3 normal = v3_normalize(v3_sub(sf.point, center));
    sf.hit_front = v3_dot(d, normal) < 0.0;
    if (!sf.hit_front) normal = v3_neg(normal);
    sf.normal = normal;
    if (need_uv) { /* tex_coord (sphere.ml:25-33) feeds Texture.eval only */
      const double one_over_pi = 1.0 / pi, one_over_two_pi = 1.0 / (2.0 * pi);
      const double theta = pt_acos(-normal.y);
      const double phi = pi + pt_atan2(-normal.z, normal.x);
      sf.tu = phi * one_over_two_pi;
      sf.tv = theta * one_over_pi;
    }
  } else {
    /* Triangle.Hit.to_hit (triangle.ml:43-64) */
    const double* tvx = sc.tri + (size_t)slot * 10;
    const V3 a = pt_load_v3(tvx), b = pt_load_v3(tvx + 3), c = pt_load_v3(tvx + 6);
    const bool framed = sc.tri_frame != nullptr; /* (wave-uniform) */
    V3 g_normal;
    if (framed) g_normal = pt_load_v3(sc.tri_frame + (size_t)slot * PT_TRI_FRAME_DOUBLES);
    else g_normal = pt_tri_normal(a, b, c);
    const double u = bu, v = bv;
    const double w = 1.0 - u - v;
    sf.point = v3_add(v3_add(v3_scale(a, w), v3_scale(b, u)), v3_scale(c, v));
    const double* uv = sc.tri_uv + (size_t)slot * 6;
    sf.tu = (uv[0] * w) + (uv[2] * u) + (uv[4] * v);
    sf.tv = (uv[1] * w) + (uv[3] * u) + (uv[5] * v);
    sf.hit_front = v3_dot(d, g_normal) < 0.0;
    sf.normal = sf.hit_front ? g_normal : v3_neg(g_normal);
    if (framed) { /* Shader_space.create of that normal: one of the slot's two precomputed rotations (PtSceneDev.tri_frame); both are
                     requested with the normal -- a load that depends on hit_front would be one more round trip in the step's chain */
      const double2* r = (const double2*)(sc.tri_frame + (size_t)slot * PT_TRI_FRAME_DOUBLES + 4);
      const double2 f0 = r[0], f1 = r[1], b0 = r[2], b1 = r[3];
      sf.rot.r = sf.hit_front ? f0.x : b0.x;
      sf.rot.v = v3(sf.hit_front ? f0.y : b0.y, sf.hit_front ? f1.x : b1.x, sf.hit_front ? f1.y : b1.y);
      sf.omega_i = pt_quat_transform(sf.rot, v3_neg(d));
      return sf;
    }
  }
  sf.rot = pt_shader_rotation(sf.normal);
  sf.omega_i = pt_quat_transform(sf.rot, v3_neg(d)); /* Shader_space.omega_i */
  return sf;
}

/* Material.scatter applied to u (material.ml:22-57): kind 0 Absorb | 1 Specular (wo = shader-space direction of the
 * scattered ray, attenuation) | 2 Diffuse (attenuation = the texture colour) */
struct PtScatter {
  int kind;
  V3 attenuation, wo;
};
template <int CAT = PT_CAT_NONE, bool IMG = false>
__device__ __forceinline__ PtScatter pt_material_scatter(const PtSceneDev& sc, const PtSurface& sf, const PtMatRegs& m, double su) {
  const V3 omega_i = sf.omega_i;
  PtScatter r;
  r.attenuation = v3(1.0, 1.0, 1.0);
  r.wo = v3(0.0, 0.0, 0.0);
  const int mkind = (CAT == PT_CAT_LAMBERT_SOLID || CAT == PT_CAT_LAMBERT_CHECKER) ? 0
                    : (CAT == PT_CAT_METAL ? 1 : (CAT == PT_CAT_DIELECTRIC ? 2 : m.kind));
  if (mkind == 0) {
    r.kind = 2;
    r.attenuation = pt_texture_eval<IMG>(m, sf.tu, sf.tv);
  } else if (mkind == 1) {
    const V3 omega_r = v3(-omega_i.x, -omega_i.y, omega_i.z); /* Shader_space.reflect */
    if (omega_r.z <= 0.0) {
      r.kind = 0;
    } else {
      r.kind = 1;
      const V3 a = pt_texture_eval<IMG>(m, sf.tu, sf.tv);
      const double sp5 = pt_pow5(1.0 - omega_i.z);
      const V3 c = v3_scale(v3_sub(v3(1.0, 1.0, 1.0), a), sp5);
      r.attenuation = v3_add(a, c);
      r.wo = omega_r;
    }
  } else {
    r.kind = 1;
    const double index = m.index, index_inv = 1.0 / m.index;
    const double wi_z = omega_i.z;
    const double c = wi_z < 0.0 ? 0.0 : (1.0 < wi_z ? 1.0 : wi_z); /* Float.clamp_exn */
    const double sn = pt_sqrt_nonneg(1.0 - c * c);
    const double refract_ratio = sf.hit_front ? index_inv : index;
    /* Both candidate directions are cheap: evaluate them unconditionally and select.  (A divergent
     * `a || f(x) > u` branch here was miscompiled by hipcc -O3 -- caught by the bit-exact sample test.) */
    const bool reflect = (refract_ratio * sn > 1.0) || (pt_schlick(c, refract_ratio) > su);
    /* Shader_space.refract (shader_space.ml:41-49) */
    const double cc = pt_base_min(omega_i.z, 1.0);
    const V3 perp = v3_scale(v3_sub(v3(0.0, 0.0, cc), omega_i), refract_ratio);
    const V3 para = v3(0.0, 0.0, -pt_sqrt_nonneg(pt_fabs(1.0 - v3_quadrance(perp))));
    const V3 refr = v3_add(perp, para);
    r.wo.x = reflect ? -omega_i.x : refr.x; /* Shader_space.reflect (shader_space.ml:34-39) */
    r.wo.y = reflect ? -omega_i.y : refr.y;
    r.wo.z = reflect ? omega_i.z : refr.z;
  }
  return r;
}

/* per-path final colours, one 32-byte record {r, g, b, -} per contribution id: a path ends in an arbitrary lane of an
 * arbitrary wave, so its three doubles go out as ONE 32-byte sector instead of three 8-byte writes to three arrays
 * (each its own sector: 96 B of HBM traffic for 24 B of data) */
struct PtContrib {
  double4* rgbx;
};

/* The bin a survivor is appended under.  Scenes whose primitives lie in a slab (Shirley: spheres on a ground plane;
 * PtSceneDev.sort_by_elevation, decided at scene creation): the ELEVATION of the new direction above that plane in 8 steps --
 * a predictor of the LENGTH of the next walk: rays that climb leave the slab after a few node tests, grazing rays cross the
 * whole scene, and what a wave of one-ray-per-lane walks loses is the spread of its rays' lengths.  tools/sim_coherence.py on
 * bounce-1 rays, 512-entry windows: wave steps per ray 0.656 (octant) -> 0.584 (elevation); sorting by the true length would give
 * 0.485.  Measured: frame 36.96 -> 35.87 ms.  Other scenes (cornell's closed box, a mesh): the direction OCTANT (rays of a
 * wave share the child order), which measured 1.5-2 % better there. */
template <int BINS = 8>
__device__ __forceinline__ int pt_bin_key(const PtSceneDev& sc, V3 o, V3 d) {
  if (sc.sort_by_elevation) {
    const float e = (float)d.x * (float)sc.sort_axis[0] + (float)d.y * (float)sc.sort_axis[1] + (float)d.z * (float)sc.sort_axis[2];
    const int b = (int)((e + 1.0f) * (0.5f * (float)BINS));
    return b < 0 ? 0 : (b > BINS - 1 ? BINS - 1 : b);
  }
  if (sc.sort_by_root) {
    const float ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
    const float ix = 1.0f / (float)d.x, iy = 1.0f / (float)d.y, iz = 1.0f / (float)d.z;
    const float ax = (sc.root_mn[0] - ox) * ix, bx = (sc.root_mx[0] - ox) * ix;
    const float ay = (sc.root_mn[1] - oy) * iy, by = (sc.root_mx[1] - oy) * iy;
    const float az = (sc.root_mn[2] - oz) * iz, bz = (sc.root_mx[2] - oz) * iz;
    const float t_in = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
    const float t_out = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    const bool reaches = !(t_out < t_in); /* a NaN (0 * inf) counts as reaching */
    return (reaches ? 4 : 0) | (d.x >= 0.0 ? 1 : 0) | (d.z >= 0.0 ? 2 : 0);
  }
  return (d.x >= 0.0 ? 1 : 0) | (d.y >= 0.0 ? 2 : 0) | (d.z >= 0.0 ? 4 : 0);
}
/* What one segment leaves behind: either the path's final colour (written to `contrib` inside) or the next ray. */
struct PtShadeOut {
  bool keep;
  V3 n_o, n_d, n_attn, n_emit;
  uint32_t id;
  int offset;
};
/* ------------------------------------------------------------------ light sampling (PTX_LIGHTING_SAMPLED)
 * Pdf.sample of the light half of diffuse_plus_light: a point on the emissive triangles, uniform by area, from the hit's two sampler
 * dimensions (u < 0.5 chose this half); returns the world-space unit direction from p towards it.  The scan of the running sums is
 * wave-uniform (scalar loads); the chosen record is a per-lane gather from a table of at most 64 x 112 bytes. */
/* (the table through the constant address space: it is never written while a kernel runs, and a load whose address is wave-uniform
 * is then a scalar load whatever the kernel has stored before it -- from the global address space the compiler keeps vector loads) */
typedef const double __attribute__((address_space(4))) PtConstDouble;
/* ptx_scene_set_sphere_light_sampling (include/ptx.h states the rule).  The sphere lights' records lie behind the triangles' in the
 * light table (pt_scene.h, PT_SLIGHT_*).  The two sphere arms are inlined.  Measured both ways (tools/kernel_resources.py against the
 * parent): inline, the 22 LIT kernels without IMG (128 VGPRs, 4 waves) go from 14..28 spilled VGPRs and 28..128 bytes of scratch to
 * 17..45 and 48..168, and the 22 LIT && IMG ones (168 VGPRs) keep theirs; as __noinline__ functions all 44 are worse (26..60 spilled
 * VGPRs, 112..240 bytes; the IMG ones 0 -> 32..64 bytes), one arm inlined and one not lies between, and marking the branch unlikely
 * changes nothing.  No kernel loses a wave per SIMD.  DESIGN.md section 7 has the cost with the option off.
 * 1 - cos(theta_max) of the cone a sphere of squared radius r2 spans from a point at squared distance d2 > r2 of its centre, without
 * the cancellation: */
__device__ __forceinline__ double pt_sphere_cone_q(double r2, double d2) {
  const double s2 = r2 / d2;
  return s2 / (1.0 + pt_sqrt_nonneg(1.0 - s2));
}
/* the sphere arm of Pdf.sample's light half: sphere light record S (a per-lane gather), (u2, v) in [0, 1]^2; the world-space unit
 * direction -- uniform over the cone the sphere spans from p, over the whole sphere of directions for a p inside or on it */
__device__ __forceinline__ V3 pt_sphere_light_sample(const double* __restrict__ S, V3 p, double u2, double v) {
  const double pi = 3.14159265358979323846;
  const double r2 = S[PT_SLIGHT_R2];
  const V3 f = v3_sub(v3(S[0], S[1], S[2]), p);
  const double d2 = v3_dot(f, f);
  const double phi = (v * 2.0) * pi;
  double sn, cs;
  pt_sincos(phi, &sn, &cs);
  if (d2 <= r2) {
    const double z = 1.0 - 2.0 * u2;
    const double m = 1.0 - z * z;
    const double s = pt_sqrt_nonneg(m > 0.0 ? m : 0.0);
    return v3(s * cs, s * sn, z);
  }
  const double t = u2 * pt_sphere_cone_q(r2, d2);
  const double ct = 1.0 - t, st = pt_sqrt_nonneg(t * (2.0 - t));
  return pt_quat_transform(pt_quat_conj(pt_shader_rotation(v3_normalize(f))), v3(st * cs, st * sn, ct));
}
/* the sphere lights' part of Pdf.eval's light half: to pd, the triangles' running sum, every sphere light whose cone holds w adds, in
 * list order, its share W_k / W_total of the draws over the cone's solid angle.  The table is indexed uniformly: scalar loads. */
__device__ __forceinline__ double pt_sphere_light_pd(const PtConstDouble* __restrict__ stable, int ns, double total, V3 p, V3 w, double pd) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < ns; ++k) {
    const PtConstDouble* S = stable + k * PT_SLIGHT_DOUBLES;
    const double r2 = S[PT_SLIGHT_R2], share = S[PT_SLIGHT_W] / total;
    const V3 f = v3_sub(v3(S[0], S[1], S[2]), p);
    const double d2 = v3_dot(f, f);
    if (d2 <= r2) {
      pd = pd + share / (4.0 * pi);
    } else {
      const double bp = v3_dot(f, w);
      const V3 g = v3_sub(f, v3_scale(w, bp));
      if (bp > 0.0 && r2 - v3_dot(g, g) >= 0.0) pd = pd + share / ((2.0 * pi) * pt_sphere_cone_q(r2, d2));
    }
  }
  return pd;
}
/* Pdf.sample of the light half over the joined table, triangles first and the sphere lights behind them (none unless
 * ptx_scene_set_sphere_light_sampling is on: the branch on their count is wave-uniform).  k_out: the index of the light drawn. */
__device__ __forceinline__ V3 pt_light_sample(const PtSceneDev& sc, V3 p, double u, double v, int* k_out = nullptr) {
  const double x = (2.0 * u) * sc.light_area;
  const PtConstDouble* table = (const PtConstDouble*)sc.lights;
  const int nt = sc.n_lights, ns = sc.n_sphere_lights;
  int k = nt + ns - 1;
  if (ns > 0) { /* (wave-uniform) */
    const PtConstDouble* stable = table + nt * PT_LIGHT_DOUBLES;
    for (int j = ns - 2; j >= 0; --j)
      if (x < stable[j * PT_SLIGHT_DOUBLES + PT_SLIGHT_CUM]) k = nt + j;
  }
  for (int j = ns > 0 ? nt - 1 : nt - 2; j >= 0; --j)
    if (x < table[j * PT_LIGHT_DOUBLES + PT_LIGHT_CUM]) k = j; /* ends at the FIRST k with x < cum_k (the last if none) */
  if (k_out) *k_out = k;
  if (ns > 0 && k >= nt) {
    const double* S = sc.lights + (size_t)nt * PT_LIGHT_DOUBLES + (size_t)(k - nt) * PT_SLIGHT_DOUBLES;
    const double before = k > nt ? S[PT_SLIGHT_CUM - PT_SLIGHT_DOUBLES] : (nt > 0 ? S[PT_LIGHT_CUM - PT_LIGHT_DOUBLES] : 0.0);
    return pt_sphere_light_sample(S, p, pt_base_min((x - before) / S[PT_SLIGHT_W], 1.0), v);
  }
  const double* L = sc.lights + (size_t)k * PT_LIGHT_DOUBLES;
  const double before = k > 0 ? L[PT_LIGHT_CUM - PT_LIGHT_DOUBLES] : 0.0;
  const double u2 = pt_base_min((x - before) / L[PT_LIGHT_AREA], 1.0);
  const double s = pt_sqrt_nonneg(u2);
  const double b1 = 1.0 - s, b2 = v * s;
  const double w = 1.0 - b1 - b2;
  const V3 q = v3_add(v3_add(v3_scale(pt_load_v3(L), w), v3_scale(pt_load_v3(L + 3), b1)), v3_scale(pt_load_v3(L + 6), b2)); /* Triangle point */
  return v3_normalize(v3_sub(q, p));
}
/* Pdf.eval of the light half for the world direction w at p: every light the ray (p, w) meets, by the walk's own element test,
 * contributes its solid-angle density t^2 / (A_total |n . w|), and the sphere lights theirs.  The table is indexed uniformly: scalar
 * loads. */
__device__ __forceinline__ double pt_light_pd(const PtSceneDev& sc, V3 p, V3 w) {
  double pd = 0.0;
  const PtConstDouble* table = (const PtConstDouble*)sc.lights;
  for (int k = 0; k < sc.n_lights; ++k) {
    const PtConstDouble* L = table + k * PT_LIGHT_DOUBLES;
    double t = 0.0, bu, bv;
    if (pt_triangle_intersect(v3(L[0], L[1], L[2]), v3(L[3], L[4], L[5]), v3(L[6], L[7], L[8]), p, w, 0.0, PT_MAX_FINITE, &t, &bu, &bv))
      pd = pd + (t * t) / (sc.light_area * pt_fabs(v3_dot(v3(L[9], L[10], L[11]), w)));
  }
  if (sc.n_sphere_lights > 0) /* (wave-uniform) */
    pd = pt_sphere_light_pd(table + sc.n_lights * PT_LIGHT_DOUBLES, sc.n_sphere_lights, sc.light_area, p, w, pd);
  return pd;
}

/* ------------------------------------------------------------------ environment sampling (ptx_scene_set_environment_sampling;
 * include/ptx.h states the rule, DESIGN.md section 7 the mixture).  The table lies behind the environment's texels: PT_ENVD_* of
 * pt_scene.h; its two scalars (T, the last row) are read through the constant address space, at a wave-uniform address: scalar loads.
 * Pdf.sample of the environment half: a texel drawn with probability w / T, a point uniform inside it, the world-space unit direction
 * that the environment rule maps there.  Two binary searches, log2 H + log2 W dependent loads a lane: the row sums are one small table
 * every lane reads (H doubles: L1 / L2 resident), the row's running sums are the lane's own.  Each search ends at the first entry above
 * the target, as the linear scan of the rule does (the sums never decrease).  What a search's result decides -- the sum before it, the
 * row's total, the texel's weight -- is requested in one round behind it.  Every index is in range whatever (a, b) are: a target that
 * no entry exceeds (a NaN included) takes the row or column the host found. */
__device__ __forceinline__ const double* pt_env_table(const PtSceneDev& sc) {
  return sc.env + 4 * ((size_t)sc.env_w * (size_t)sc.env_h);
}
__device__ __forceinline__ V3 pt_env_sample(const PtSceneDev& sc, double a, double b, int* ix_out, int* iy_out) {
  const double pi = 3.14159265358979323846;
  const int W = sc.env_w, H = sc.env_h;
  const double* __restrict__ table = pt_env_table(sc);
  const double* __restrict__ m = table + PT_ENVD_ROWS;
  const double total = ((const PtConstDouble*)table)[PT_ENVD_TOTAL];
  const int last_row = (int)((const PtConstDouble*)table)[PT_ENVD_LAST_ROW];
  const double x = a * total;
  int lo = 0, hi = H;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x < m[mid]) hi = mid;
    else lo = mid + 1;
  }
  const int iy = lo < H ? lo : last_row;
  const double* __restrict__ c = table + PT_ENVD_COND(H) + (size_t)iy * (size_t)W;
  const double before_y = m[iy > 0 ? iy - 1 : 0], r = c[W - 1], last_x = table[PT_ENVD_LASTX(H) + (size_t)iy];
  const double fy = pt_base_min((x - (iy > 0 ? before_y : 0.0)) / r, 1.0);
  const double y = b * r;
  lo = 0;
  hi = W;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (y < c[mid]) hi = mid;
    else lo = mid + 1;
  }
  const int ix = lo < W ? lo : (int)last_x;
  const double before_x = c[ix > 0 ? ix - 1 : 0], wt = c[(size_t)W * (size_t)H + (size_t)ix]; /* (the weights lie W x H behind the sums) */
  const double fx = pt_base_min((y - (ix > 0 ? before_x : 0.0)) / wt, 1.0);
  *ix_out = ix;
  *iy_out = iy;
  const double u = ((double)ix + fx) / (double)W, v = ((double)iy + fy) / (double)H;
  const double al = u * (2.0 * pi) - pi, th = v * pi;
  double sa, ca, st, ct;
  pt_sincos(al, &sa, &ca);
  pt_sincos(th, &st, &ct);
  const V3 mm = v3(st * ca, -ct, -(st * sa));
  const double* R = sc.env_rot;
  return v3_normalize(v3((R[0] * mm.x + R[3] * mm.y) + R[6] * mm.z, (R[1] * mm.x + R[4] * mm.y) + R[7] * mm.z,
                         (R[2] * mm.x + R[5] * mm.y) + R[8] * mm.z));
}
/* Pdf.eval of the environment half for the world direction w: the texel the environment rule's tex coords fall in (nearest, whatever
 * the image's filter), its share w / T of the draws over its solid angle (2 pi / W) (pi / H) sin(theta).  One load, its address known
 * once the tex coords are. */
__device__ __forceinline__ double pt_env_pd(const PtSceneDev& sc, V3 w) {
  const double pi = 3.14159265358979323846;
  const int W = sc.env_w, H = sc.env_h;
  const double* __restrict__ table = pt_env_table(sc);
  const double total = ((const PtConstDouble*)table)[PT_ENVD_TOTAL];
  /* (u, v) of the environment rule, as pt_environment computes them */
  const V3 e = v3_normalize(w);
  const double* R = sc.env_rot;
  const double mx = (R[0] * e.x + R[1] * e.y) + R[2] * e.z;
  const double my = (R[3] * e.x + R[4] * e.y) + R[5] * e.z;
  const double mz = (R[6] * e.x + R[7] * e.y) + R[8] * e.z;
  const double one_over_pi = 1.0 / pi, one_over_two_pi = 1.0 / (2.0 * pi);
  const double cy = my < -1.0 ? -1.0 : (my > 1.0 ? 1.0 : my);
  const double u = (pi + pt_atan2(-mz, mx)) * one_over_two_pi;
  const double v = pt_acos(-cy) * one_over_pi;
  const int ix = pt_image_wrap(__builtin_trunc(pt_image_scale(u, W)), W, false), iy = pt_image_wrap(__builtin_trunc(pt_image_scale(v, H)), H, false);
  const double wt = table[PT_ENVD_WEIGHT(W, H) + (size_t)iy * (size_t)W + (size_t)ix];
  const double st = pt_sin(v * pi);
  return st > 0.0 ? ((wt / total) * ((double)W * (double)H)) / ((2.0 * (pi * pi)) * st) : 0.0;
}

/* The camera launches of k_bounce_carry hand shade 0 the decoded sample, the camera direction and the hit distance the same lane held
 * a few instructions earlier (PtCameraCarry), instead of storing hits.t[i] behind a pair of fences and having every category step
 * decode the index, derive the direction and load the distance again.  The same values, so the same arithmetic on them.  The TILE
 * launches request their chunk's tile record before the camera direction is derived instead of where it is used.  (The camera branch
 * without either was this one's A/B partner: profiles/pr_ab_camera_carry.txt, profiles/pr_camera_carry_isa.txt.) */
/* of ps only id, offset and valid are read after the walk: the caller leaves the rest zero and the registers go */
struct PtCameraCarry {
  PtPrimarySample ps;
  V3 d;
  double t; /* sphere scenes; with triangles in the scene the shade step recomputes it as for a queued ray */
};
__device__ __forceinline__ PtCameraCarry pt_camera_carry(uint32_t id, int offset, bool valid, V3 d, double t) {
  PtCameraCarry c;
  c.ps.x = c.ps.y = c.ps.gy = c.ps.pass_in_batch = 0;
  c.ps.id = id;
  c.ps.offset = offset;
  c.ps.valid = valid;
  c.d = d;
  c.t = t;
  return c;
}

/* The body of `loop` in Integrator.path_tracer (integrator.ml:30-66) for entry i of the queue (PRIMARY: virtual
 * entry i = a camera sample).  CAT = the entry's shading category if the kernel is specialised for one.
 * LIT (emissive scenes in lighting modes 1 and 2 only; mode 0 never launches it): emission is summed in path order,
 * emit0' = fma(attn0, emit, emit0), and in mode 2 (a wave-uniform branch) a Diffuse scatter samples and divides by
 * diffuse_plus_light = 1/2 cosine + 1/2 emissive triangles.
 * IMG (scenes with an image texture or an environment only; no other scene launches it): pt_texture_eval's image arm and
 * pt_background's environment arm.
 * LIT && IMG, in mode 2 with PtSceneDev.env_sample (wave-uniform as well): the light half is shared with, or is, the environment's
 * density (include/ptx.h, ptx_scene_set_environment_sampling). */
template <bool EMIT, bool PRIMARY, int CAT, bool LIT = false, bool IMG = false>
__device__ __forceinline__ void pt_shade_entry(const PtSceneDev& sc, const PtQueue& q, const PtHits& hits, const PtContrib& contrib,
                                               const double* __restrict__ alpha, int bounce, int last_bounce,
                                               const PtGenParams& g, uint32_t i, bool live, PtShadeOut& so,
                                               int known_slot = PT_SLOT_HOLE /* the entry's hit slot if the caller holds it */,
                                               const PtCameraCarry* cam = nullptr /* PRIMARY: the sample, its ray and its hit distance if the caller's lane holds them */) {
    const double pi = 3.14159265358979323846;
    bool keep = false;
    V3 n_o = v3(0, 0, 0), n_d = v3(0, 0, 0), n_attn = v3(0, 0, 0), n_emit = v3(0, 0, 0);
    uint32_t id = 0;
    int offset = 0;
    PtPrimarySample ps;
    if (PRIMARY && live) {
      ps = cam ? cam->ps : pt_primary_decode(g, i);
      live = ps.valid;
    }
    if (live) {
      V3 o, d, attn0, emit0 = v3(0.0, 0.0, 0.0);
      if (PRIMARY) {
        o = v3(0.0, 0.0, 0.0);
        /* derived again for a ray that another lane or an earlier launch walked (k_shade_pool, k_bounce's pool steps): handing it over
         * through memory as a 32-byte {t, direction} record measured headline +-0, cornell +2 %, mesh +3 % (profiles/r05_ab_primary_dir.txt).
         * k_bounce_carry's camera launch shades in the lane that walked, and no byte moves: cam (profiles/pr_ab_camera_carry.txt) */
        d = cam ? cam->d : pt_primary_dir(sc, g, ps, alpha);
        attn0 = v3(1.0, 1.0, 1.0); /* Color.white, integrator.ml:68 */
        id = ps.id;
        offset = ps.offset;
      } else {
        pt_q_load_ray(q, i, o, d);
        pt_q_load_path<EMIT>(q, i, attn0, id, offset, emit0);
      }
      const int slot = CAT == PT_CAT_MISS ? -1 : (known_slot != PT_SLOT_HOLE ? known_slot : hits.slot[i]);
      V3 result = v3(0, 0, 0);
      bool done = true;
      if (CAT == PT_CAT_MISS || (CAT == PT_CAT_NONE && slot < 0)) {
        /* None -> add_mul emit0 attn0 (background ray), integrator.ml:36 */
        result = v3_fma(attn0, pt_background<IMG>(sc, d), emit0);
      } else {
        /* the rest of the segment's inputs, requested in the same round as the queue records above (PtMatRegs): the hit
         * distance, the slot's shading record, and its geometry (or, with triangles in the scene, its kind) */
        double t_hit, bu = 0.0, bv = 0.0;
        PtSlotGeom geom;
        geom.cx = geom.cy = geom.cz = 0.0;
        geom.kind = PT_SLOT_SPHERE;
        if (sc.has_triangles) {
          geom.kind = (int)sc.slot_kind[slot];
          /* (t, u, v) of the hit again, from the ray and the primitive the walk settled on: Array_leaf's own element tests
           * (PtTraverser::packet, begin's floor test) on the same operands.  Their acceptance range only ever decided WHICH
           * primitive won; the values do not depend on it. */
          t_hit = 0.0;
          if (geom.kind == PT_SLOT_SPHERE) {
            const double* sp = sc.sph + (size_t)slot * 4;
            (void)pt_sphere_intersect_scalar(v3(sp[0], sp[1], sp[2]), sp[3], o, d, 0.0, PT_MAX_FINITE, &t_hit);
          } else {
            const double* tvx = sc.tri + (size_t)slot * 10;
            (void)pt_triangle_intersect(pt_load_v3(tvx), pt_load_v3(tvx + 3), pt_load_v3(tvx + 6), o, d, 0.0, PT_MAX_FINITE, &t_hit, &bu, &bv);
          }
        } else {
          t_hit = (PRIMARY && cam) ? cam->t : hits.t[i];
          const double2* sp = (const double2*)(sc.sph + (size_t)slot * 4);
          const double2 s0 = sp[0], s1 = sp[1];
          geom.cx = s0.x;
          geom.cy = s0.y;
          geom.cz = s1.x;
        }
        const PtMatRegs m = pt_mat_load<CAT, EMIT, IMG>(sc.slot_shade + slot);
        const bool is_tri = geom.kind != PT_SLOT_SPHERE;
        const PtSurface sf = pt_surface_hit<CAT>(sc, o, d, slot, t_hit, is_tri ? bu : 0.0, is_tri ? bv : 0.0, m, geom);
        const V3 point = sf.point;
        const Quat rot_inv = pt_quat_conj(sf.rot);
        const V3 emit = m.emit;
        /* take_2d (), integrator.ml:20-28,39: dims 2+2k, 3+2k for the k-th hit */
        const double su = pt_lds_get(alpha, offset, 2 + 2 * bounce);
        const double sv = pt_lds_get(alpha, offset, 3 + 2 * bounce);
        const PtScatter scat = pt_material_scatter<CAT, IMG>(sc, sf, m, su);
        const int sc_kind = scat.kind;
        V3 attenuation = scat.attenuation;
        V3 wo = scat.wo;

        if (sc_kind == 0) {
          result = v3_fma(attn0, emit, emit0); /* Absorb, integrator.ml:41 */
        } else {
          bool scatter_ok = true;
          if (sc_kind == 2) {
            /* Pdf.sample / Pdf.eval (pdf.ml:5-15, shader_space.ml:56-64) */
            /* mode 2: Pdf.sample diffuse_plus_light -- u < 0.5 the light half, else the cosine half on (2u - 1, v) */
            const bool sampled = LIT && sc.lighting == PT_LIGHTING_SAMPLED; /* (wave-uniform) */
            /* ... with environment sampling: su < 0.25 the triangles on 2u := 4 su, su < 0.5 the environment on (4 su - 1, v); without
             * light triangles su < 0.5 the environment on (2 su, v) (both wave-uniform) */
            const bool env_on = LIT && IMG && sampled && sc.env_sample != 0;
            const bool tri_on = sampled && !(env_on && sc.n_lights + sc.n_sphere_lights == 0);
            const double hu = sampled ? 2.0 * su - 1.0 : su;
            if (tri_on && su < (env_on ? 0.25 : 0.5)) {
              wo = pt_quat_transform(sf.rot, pt_light_sample(sc, point, env_on ? 2.0 * su : su, sv)); /* Pdf.sample returns a shader-space direction */
            } else if (env_on && su < 0.5) {
              int tx, ty;
              wo = pt_quat_transform(sf.rot, pt_env_sample(sc, tri_on ? 4.0 * su - 1.0 : 2.0 * su, sv, &tx, &ty));
            } else {
              const double r = pt_sqrt_nonneg(hu);
              const double theta = sv * 2.0 * pi;
              double sn, cs;
              pt_sincos(theta, &sn, &cs);
              wo = v3(r * cs, r * sn, pt_sqrt_nonneg(1.0 - hu));
            }
            const double diffuse_pd = (wo.z < 0.0) ? 0.0 : wo.z / pi;
            if (diffuse_pd == 0.0) {
              scatter_ok = false;
            } else {
              double divisor = diffuse_pd; /* modes 0 and 1: divisor = Pdf.eval diffuse_plus_light = the same */
              if (sampled && !env_on) divisor = 0.5 * diffuse_pd + 0.5 * pt_light_pd(sc, point, pt_quat_transform(rot_inv, wo));
              if (env_on) {
                const V3 wdir = pt_quat_transform(rot_inv, wo); /* the direction world_ray will trace */
                const double env_pd = pt_env_pd(sc, wdir);
                if (tri_on) divisor = (0.5 * diffuse_pd + 0.25 * pt_light_pd(sc, point, wdir)) + 0.25 * env_pd;
                else divisor = 0.5 * diffuse_pd + 0.5 * env_pd;
              }
              const double pd = diffuse_pd / divisor;
              if (!pt_isfinite(pd)) scatter_ok = false;
              else attenuation = v3_scale(attenuation, pd);
            }
          }
          if (!scatter_ok) {
            result = v3_fma(attn0, emit, emit0); /* integrator.ml:53,58 */
          } else {
            /* Shader_space.world_ray (shader_space.ml:51-54) */
            const V3 dir = pt_quat_transform(rot_inv, wo);
            n_o = v3_add(point, v3_scale(dir, 1e-3));
            n_d = dir;
            if (LIT) n_emit = v3_fma(attn0, emit, emit0); /* path order: add_mul emit0 attn0 emit, the old attn0 */
            else n_emit = v3_fma(attenuation, emit0, emit); /* add_mul emit attenuation emit0 */
            n_attn = v3_mul(attenuation, attn0);
            if (last_bounce) {
              /* the recursive call sees max_bounces <= 0: add_mul emit0 attn0 Color.black (integrator.ml:31-32) */
              result = v3_fma(n_attn, v3(0.0, 0.0, 0.0), n_emit);
            } else {
              done = false;
            }
          }
        }
      }
      if (done) {
        contrib.rgbx[id] = make_double4(result.x, result.y, result.z, 0.0);
      } else {
        keep = true;
      }
    }
    so.keep = keep;
    so.n_o = n_o; so.n_d = n_d; so.n_attn = n_attn; so.n_emit = n_emit;
    so.id = id;
    so.offset = offset;
}

#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 4
#endif
/* The IMG instantiations of k_bounce and k_shade_pool (scenes with an image texture or an environment) get 3 waves per SIMD instead of
 * 4, i.e. 168 VGPRs instead of 128: at 128 the image arm's live values -- the texel address, the two fractions, and for bilinear 32
 * registers of texels in flight -- went to scratch in 64 of the 71 kernels; at 168 none of them spills a register (DESIGN.md section
 * 4).  Their workgroups are sized to match: 768 threads of k_bounce (12 waves: 3 per SIMD), 256 of k_shade_pool (3 per CU). */
#define PT_IMG_WAVES 3
#define PT_BOUNCE_THREADS_IMG 768
#define PT_POOL_THREADS_IMG 256
#ifndef PT_SHADE_TIMING
#define PT_SHADE_TIMING 0
#endif

/* ------------------------------------------------------------------ the shade stage without workgroup barriers
 * Rounds 1-2 shaded category-sorted 512-entry windows (workgroup barriers around a sort and an append): between two barriers the
 * window's waves ran materials of very different length (a miss is ~150 instructions, a checker Lambertian ~1200), and the
 * kernel's own clock showed 33 % of a wave's life at the append's first barrier waiting for the window's slowest wave, 10 %
 * behind the append's atomic, 12 % in the sort, 39 % in the segment's arithmetic (removed in round 5).
 *
 * Here a wave never waits for another one (except while a full output block is being replaced, below):
 *  - POOLS.  Every wave owns one list of queue indices per category in LDS (128 entries each).  It classifies raw chunks of 64
 *    entries (hit slot -> category) into its lists and, whenever a list holds 64, shades those 64 together: one category per
 *    wave step by construction, no sort.  When the input is exhausted the lists are drained (the only partly filled steps).
 *  - BLOCKED OUTPUT.  The workgroup owns one output block of PT_POOL_BLOCK entries per bin (pt_bin_key: elevation / octant);
 *    a wave reserves room for its survivors of a bin with ONE LDS atomic on a word that holds (block, cursor) together, so the
 *    block it writes to is the one its reservation belongs to.  The wave whose reservation crosses the end of the block fills
 *    it up, gets the next block from the queue's global counter (one device atomic per PT_POOL_BLOCK survivors, as few as the
 *    windowed append) and publishes it; waves that arrive in between spin on the LDS word.  A block is single-bin, so every
 *    wave of the next trace launch walks rays of one bin.
 *  - HOLES.  When the kernel ends the blocks in use are partly filled.  The last wave of the workgroup marks the unused
 *    entries by a direction whose x is a NaN with a payload no arithmetic produces (PT_HOLE_HI); k_trace skips such an entry and
 *    records slot PT_SLOT_HOLE for it, which the next launch of this kernel drops when it classifies.  The queue's count
 *    is then a number of ENTRIES (a multiple of the block), not of rays; the segment counters count rays.
 * Every ray still gets exactly pt_shade_entry's arithmetic; the order of the queue changes, which no result depends on
 * (contributions are stored per path id and summed in pass order). */
#ifndef PT_POOL_BLOCK
#define PT_POOL_BLOCK 256 /* < 4096 - 16 * 64: the cursor field must hold a full block plus one stray reservation per wave */
#endif
#ifndef PT_POOL_THREADS
#define PT_POOL_THREADS 512 /* largest workgroup of k_shade_pool (the pools live in dynamic LDS, sized by blockDim).  Nothing in it is
                               workgroup-wide but the output blocks: when two batches share every CU it runs 256-thread workgroups,
                               which interleave with the other batch's trace workgroups at a finer grain (headline frame 27.6 ms
                               against 29.6 ms with 512, 29.0 ms with 128); alone on the chip 512 is 2-6 % faster (fewer
                               part-filled blocks, larger shares) */
#endif
#ifndef PT_POOL_BINS
#define PT_POOL_BINS 8 /* output bins per workgroup (<= 64: one lane each in pt_pool_push); octant-keyed scenes use the first 8 */
#endif
#ifndef PT_POOL_RUN
#define PT_POOL_RUN 32 /* a workgroup's share of the input: runs of this many consecutive chunks, dealt round-robin; its waves take
                          the chunks of a run one by one (LDS counter), so they shade neighbouring chunks at the same time and a block of
                          survivors holds rays that were neighbours -- the next trace launch walks them together (single chunks dealt
                          round-robin cost that launch 8 %).  Runs handed to single waves from device counters: shade +18 %. */
#endif
#ifndef PT_POOL_MIN_CHUNKS
#define PT_POOL_MIN_CHUNKS 16 /* raw chunks per wave below which fewer workgroups take part (the drain costs up to 5 part-filled steps) */
#endif
#define PT_POOL_NO_BLOCK 0xfffffu

/* blk_list / blk_n (LDS, or null): every block this workgroup takes from the output queue is also noted there (PtSolo: the workgroup
 * reads its own survivors back in the next bounce of the same launch) */
/* The reservation: room for the wave's entries (`keep` lanes, each under its `bin`) in the workgroup's output blocks.  Returns the
 * lane's entry of `out` (meaningful where `keep`); at least one lane must keep. */
__device__ __forceinline__ uint32_t pt_pool_reserve(const PtQueue& out, bool keep, int bin, uint32_t* lds_out,
                                                    uint32_t* blk_list = nullptr, uint32_t* blk_n = nullptr) {
  const int lane = pt_lane();
  /* all bins at once: lane b < 8 holds bin b's survivor count and makes its reservation -- one LDS atomic instruction */
  uint32_t rank = 0, kk = 0;
#pragma unroll
  for (int b = 0; b < PT_POOL_BINS; ++b) {
    const unsigned long long m = __ballot(keep && bin == b);
    if (bin == b) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == b) kk = (uint32_t)__popcll(m);
  }
  uint32_t st = 0;
  if (kk != 0) st = __hip_atomic_fetch_add(lds_out + lane, kk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  /* a reservation that does not fit its block (pos + k > PT_POOL_BLOCK): rare, one bin at a time, wave-uniform */
  unsigned long long slow = __ballot(kk != 0 && (st & 0xfffu) + kk > (uint32_t)PT_POOL_BLOCK);
  uint32_t blk2 = 0, head = 0xffffffffu; /* lane b: the second block of a reservation that crossed into it, and how much went to the first */
  while (slow != 0) {
    const int b = __ffsll((long long)slow) - 1;
    slow &= slow - 1;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)kk, b);
    uint32_t sb = (uint32_t)__builtin_amdgcn_readlane((int)st, b);
    for (;;) {
      const uint32_t pos = sb & 0xfffu, blk = sb >> 12;
      if (pos + k <= (uint32_t)PT_POOL_BLOCK) break; /* a retry that fits */
      if (pos <= (uint32_t)PT_POOL_BLOCK) {
        /* this reservation crosses the end of the block (or finds it exactly full, or finds no block yet): fill it up and
         * bring the next one.  Everybody else sees pos > PT_POOL_BLOCK until the new word is stored. */
        uint32_t nb = 0;
        if (lane == 0) {
          nb = atomicAdd(out.count, (uint32_t)PT_POOL_BLOCK) / (uint32_t)PT_POOL_BLOCK;
          if (blk_list) blk_list[__hip_atomic_fetch_add(blk_n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)] = nb;
        }
        nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)nb);
        const uint32_t h = (uint32_t)PT_POOL_BLOCK - pos;
        if (lane == 0) __hip_atomic_store(lds_out + b, (nb << 12) | (k - h), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (lane == b) { blk2 = nb; head = h; }
        break;
      }
      /* the block is being replaced by another wave: wait for the new one, reserve again */
      uint32_t cur;
      do {
        __builtin_amdgcn_s_sleep(2);
        cur = __hip_atomic_load(lds_out + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } while ((cur >> 12) == blk);
      uint32_t again = 0;
      if (lane == 0) again = __hip_atomic_fetch_add(lds_out + b, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      sb = (uint32_t)__builtin_amdgcn_readfirstlane((int)again);
    }
    if (lane == b) st = sb;
  }
  /* every lane picks up its bin's reservation */
  const uint32_t my_st = (uint32_t)__shfl((int)st, bin, 64);
  const uint32_t my_head = (uint32_t)__shfl((int)head, bin, 64);
  const uint32_t my_blk2 = (uint32_t)__shfl((int)blk2, bin, 64);
  return rank < my_head ? (my_st >> 12) * (uint32_t)PT_POOL_BLOCK + (my_st & 0xfffu) + rank
                        : my_blk2 * (uint32_t)PT_POOL_BLOCK + (rank - my_head);
}
template <bool EMIT>
__device__ __forceinline__ void pt_pool_push(const PtSceneDev& sc, const PtQueue& out, const PtShadeOut& so, uint32_t* lds_out,
                                             uint32_t* blk_list = nullptr, uint32_t* blk_n = nullptr, bool one_bin = false) {
  /* one_bin (wave-uniform): a workgroup whose rays would not fill a block does not spread them over eight (PtSolo) */
  const int bin = one_bin ? 0 : pt_bin_key<PT_POOL_BINS>(sc, so.n_o, so.n_d);
  if (__ballot(so.keep) == 0) return;
  const uint32_t dst = pt_pool_reserve(out, so.keep, bin, lds_out, blk_list, blk_n);
  if (so.keep) pt_q_store<EMIT>(out, dst, so.n_o, so.n_d, so.n_attn, so.n_emit, so.id, so.offset);
}

/* The workgroup's share of a launch's chunks (k_shade_pool, k_bounce, k_bounce_carry).  PT_SHARE_WGS declares n_wg, how many
 * workgroups take part -- fewer than the grid when a wave would get less than min_chunks (workgroup-uniform; the others return at
 * once).  Those deal the chunks among themselves in runs of PT_POOL_RUN, round-robin; a workgroup's waves take the chunks of its runs
 * one by one from a counter in LDS: PT_SHARE_NEXT declares k, the wave's next count (wave-uniform), PT_SHARE_CHUNK is that count's
 * chunk of the launch (>= total_chunks: the share is exhausted).
 * Macros, not functions: as inlined functions the same statements compile every instantiation of k_shade_pool to other code (+-300
 * of ~10000 instructions, other SGPR spill counts), and that kernel is held to the parent's instructions. */
#define PT_SHARE_WGS(n_wg, total_chunks, min_chunks, nw) \
  uint32_t n_wg = (total_chunks) / (uint32_t)((min_chunks) * (nw)); \
  n_wg = n_wg < 1u ? 1u : (n_wg > gridDim.x ? gridDim.x : n_wg)
#define PT_SHARE_NEXT(k, lds_ctr, lane) \
  uint32_t k = 0u; \
  if ((lane) == 0) k = __hip_atomic_fetch_add(&(lds_ctr), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
  k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k)
#define PT_SHARE_CHUNK(k, n_wg) (((k) / PT_POOL_RUN) * ((n_wg) * PT_POOL_RUN) + blockIdx.x * PT_POOL_RUN + ((k) % PT_POOL_RUN))

/* HOLES (above): the last of the workgroup's nw waves to arrive marks what is left of the workgroup's part-filled output blocks;
 * mark(e) makes entry e of the output queue a hole, the way the kernel's reader looks for one. */
template <typename Mark>
__device__ __forceinline__ void pt_blocks_close(uint32_t* lds_done, const uint32_t* lds_out, int nw, Mark mark) {
  const int lane = pt_lane();
  uint32_t done = 0u;
  if (lane == 0) done = __hip_atomic_fetch_add(lds_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
  done = (uint32_t)__builtin_amdgcn_readfirstlane((int)done);
  if (done != (uint32_t)(nw - 1)) return;
  for (int b = 0; b < PT_POOL_BINS; ++b) {
    const uint32_t st = __hip_atomic_load(lds_out + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t blk = st >> 12, pos = st & 0xfffu;
    if (blk == PT_POOL_NO_BLOCK) continue;
    for (uint32_t e = pos + (uint32_t)lane; e < (uint32_t)PT_POOL_BLOCK; e += PT_WAVE) mark((size_t)blk * PT_POOL_BLOCK + e);
  }
}
/* a queue whose reader looks at the rays (k_trace, k_bounce): direction x = the hole NaN */
__device__ __forceinline__ void pt_blocks_close_rays(uint32_t* lds_done, const uint32_t* lds_out, int nw, const PtQueue& out) {
  pt_blocks_close(lds_done, lds_out, nw, [&](size_t e) { out.ray[e].dx = __hiloint2double((int)PT_HOLE_HI, 0); });
}

template <bool EMIT, bool PRIMARY, bool LIT = false, bool IMG = false>
__global__ __launch_bounds__(IMG ? PT_POOL_THREADS_IMG : PT_POOL_THREADS, IMG ? PT_IMG_WAVES : PT_SHADE_WAVES) void k_shade_pool(PtSceneDev sc, PtQueue q, PtHits hits, PtQueue out, PtContrib contrib,
                                                const double* __restrict__ alpha, int bounce, int last_bounce,
                                                PtGenParams g, uint32_t n_primary, uint32_t* work) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_pool_raw[]; /* [waves][PT_N_SHADE_CAT][128] x (queue index, hit slot) */
  __shared__ uint32_t lds_out[PT_POOL_BINS];
  __shared__ uint32_t lds_chunk_ctr, lds_done;
  const int lane = pt_lane(), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
  const uint32_t n = PRIMARY ? n_primary : *q.count;
  const uint32_t total_chunks = (uint32_t)(((unsigned long long)n + PT_WAVE - 1) / PT_WAVE);
  PT_SHARE_WGS(n_wg, total_chunks, PT_POOL_MIN_CHUNKS, nw);
  if (blockIdx.x >= n_wg) return; /* workgroup-uniform */
  if (threadIdx.x == 0) { lds_chunk_ctr = 0u; lds_done = 0u; }
  if (threadIdx.x < PT_POOL_BINS) lds_out[threadIdx.x] = (PT_POOL_NO_BLOCK << 12) | (uint32_t)PT_POOL_BLOCK; /* "full": the first push brings a block */
  __syncthreads(); /* the only workgroup barrier */
  uint2 (*pool)[128] = (uint2 (*)[128])lds_pool_raw + (size_t)wave * PT_N_SHADE_CAT;
  uint32_t cnt[PT_N_SHADE_CAT];
#pragma unroll
  for (int k = 0; k < PT_N_SHADE_CAT; ++k) cnt[k] = 0u;
  /* raw chunks are classified through a two-stage pipeline, so that neither of the two dependent loads (hit slot, then the
   * slot's category) is waited for: stage B holds a chunk whose slots are on their way, stage C one whose categories are */
  uint32_t iB = 0u, iC = 0u;
  int slotB = PT_SLOT_HOLE, slotC = PT_SLOT_HOLE, catC = PT_CAT_NONE;
  bool haveB = false, haveC = false; /* wave-uniform */
#define PT_POOL_TAKE_B() do { \
    PT_SHARE_NEXT(unit_, lds_chunk_ctr, lane); \
    unit_ = PT_SHARE_CHUNK(unit_, n_wg); \
    haveB = unit_ < total_chunks; \
    iB = unit_ * PT_WAVE + (uint32_t)lane; \
    slotB = PT_SLOT_HOLE; \
    if (haveB) { \
      bool valid_ = iB < n; \
      if (PRIMARY && valid_) valid_ = pt_primary_decode(g, iB).valid; \
      if (valid_) slotB = hits.slot[iB]; \
    } \
  } while (0)
#define PT_POOL_ADVANCE() do { \
    iC = iB; haveC = haveB; slotC = slotB; \
    catC = slotB == PT_SLOT_HOLE ? PT_CAT_NONE : (slotB < 0 ? PT_CAT_MISS : (int)sc.slot_cat[slotB]); \
    PT_POOL_TAKE_B(); \
  } while (0)
  PT_POOL_TAKE_B();
  PT_POOL_ADVANCE();
  bool more = haveC;
#if PT_SHADE_TIMING
  unsigned long long tm_refill = 0, tm_entry = 0, tm_push = 0, tm_steps = 0, tm_live = 0;
  const unsigned long long tm_begin = __builtin_readcyclecounter();
  unsigned long long tm_t = tm_begin;
#define PT_TM(var, since) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_readcyclecounter(); var += now_ - since; since = now_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PT_TM(var, since) do { } while (0)
#endif
  for (;;) {
    /* the fullest list that holds a whole step; once the input is exhausted, the fullest list */
    int c = -1;
    uint32_t best = more ? (uint32_t)(PT_WAVE - 1) : 0u;
#pragma unroll
    for (int k = 0; k < PT_N_SHADE_CAT; ++k)
      if (cnt[k] > best) { best = cnt[k]; c = k; }
    if (c >= 0) {
      const uint32_t take = best < (uint32_t)PT_WAVE ? best : (uint32_t)PT_WAVE;
      const uint32_t start = best - take;
      const bool live = (uint32_t)lane < take;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); /* this wave's own pushes below */
      uint32_t i = 0u;
      int sl = -1;
      PtShadeOut so;
      so.keep = false;
      /* one category per step (wave-uniform `c`): each case reads its own list and runs its own specialisation */
#define PT_POOL_STEP(K, ...)                                                                                               \
  case K: {                                                                                                                \
    cnt[K] = start;                                                                                                        \
    if (live) {                                                                                                            \
      const uint2 e = pool[K][start + lane];                                                                               \
      i = e.x;                                                                                                             \
      sl = (int)e.y;                                                                                                       \
    }                                                                                                                      \
    pt_shade_entry<EMIT, PRIMARY, K, LIT, IMG>(sc, q, hits, contrib, alpha, bounce, last_bounce, g, i, live, so, ##__VA_ARGS__); \
  } break;
      switch (c) {
        PT_POOL_STEP(PT_CAT_MISS)
        PT_POOL_STEP(PT_CAT_LAMBERT_SOLID, sl)
        PT_POOL_STEP(PT_CAT_LAMBERT_CHECKER, sl)
        PT_POOL_STEP(PT_CAT_METAL, sl)
        PT_POOL_STEP(PT_CAT_DIELECTRIC, sl)
        default: break;
      }
#undef PT_POOL_STEP
      PT_TM(tm_entry, tm_t);
      if (c != PT_CAT_MISS && !last_bounce) pt_pool_push<EMIT>(sc, out, so, lds_out);
      PT_TM(tm_push, tm_t);
#if PT_SHADE_TIMING
      tm_steps++;
      tm_live += take;
#endif
      continue;
    }
    if (!more) break;
#pragma unroll
    for (int k = 0; k < PT_N_SHADE_CAT; ++k) {
      const unsigned long long m = __ballot(catC == k);
      if (catC == k) pool[k][cnt[k] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = make_uint2(iC, (uint32_t)slotC);
      cnt[k] += (uint32_t)__popcll(m);
    }
    PT_POOL_ADVANCE();
    more = haveC;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    PT_TM(tm_refill, tm_t);
  }
#if PT_SHADE_TIMING
  if (lane == 0) {
    uint32_t* tw = work + 16; /* diagnostic build only */
    const unsigned long long life = __builtin_readcyclecounter() - tm_begin;
    atomicAdd(tw + 0, (uint32_t)(tm_refill >> 8));
    atomicAdd(tw + 1, (uint32_t)(tm_entry >> 8));
    atomicAdd(tw + 2, (uint32_t)(tm_push >> 8));
    atomicAdd(tw + 3, (uint32_t)tm_steps);
    atomicAdd(tw + 4, (uint32_t)(life >> 8));
    atomicAdd(tw + 5, 1u);
    atomicAdd(tw + 6, (uint32_t)tm_live);
    atomicMax(tw + 7, (uint32_t)(life >> 8));
  }
#endif
#undef PT_TM
#undef PT_POOL_TAKE_B
#undef PT_POOL_ADVANCE
  if (last_bounce) return;
  pt_blocks_close_rays(&lds_done, lds_out, nw, out);
}

/* ------------------------------------------------------------------ one kernel per bounce
 * k_trace and k_shade_pool of two batches share every CU so that one batch's vector-bound walk fills the other's waits for
 * memory -- but a 128-VGPR shade wave that waits two thirds of its life holds its quarter of the register file while it
 * does, and the split 4 trace + 2 shade waves per SIMD halves the shade stage's own latency hiding (the frame gained 6 % over
 * running the two kernels one after the other).  k_bounce is both stages in ONE wave: it walks a chunk of
 * 64 queued rays (pt_trace_ray with k_trace's tail cut; the walks it cuts short are pooled per workgroup in LDS), files the finished rays in its
 * per-category pools, and whenever a pool holds 64 entries shades them (pt_shade_entry, pt_pool_push exactly as in
 * k_shade_pool).  Every wave of the CU then spends most of its life walking, the waits of a wave that shades are covered by
 * the three others on its SIMD, the hit slot never goes through memory, and a bounce is one launch.  One 1024-thread
 * workgroup per CU: [stacks][scene image][16 waves x 5 pools][parked walks] in LDS.  Same tests in the same order per ray, same
 * arithmetic per segment: the results are those of the two-kernel path bit for bit. */
#ifndef PT_BOUNCE_THREADS
#define PT_BOUNCE_THREADS 1024
#endif
#ifndef PT_BOUNCE_THREADS_GLOBAL
#define PT_BOUNCE_THREADS_GLOBAL 1024 /* k_bounce workgroup on scenes walked from HBM / L2: nothing is shared but the output blocks and the chunk
                                         hand-out, and the larger the group that shares them the better -- ganesha-like frame 28.4 (256) / 28.0 (512) /
                                         26.1 ms (1024) against 28.95 ms for k_trace + k_shade_pool */
#endif
#ifndef PT_BOUNCE_WAVES
#define PT_BOUNCE_WAVES 4 /* waves per SIMD asked of the register allocator (PT_BOUNCE_THREADS / 256); 768 threads / 3 waves: +16 % */
#endif
/* The walk phase's node loop on LDS scenes is one divergent loop (pt_trace_ray DIV_LOOP) in both leaf modes: headline -0.7 ... -1.1 %;
 * cornell (Array_leaf) +1 % with the untagged links of round 4, -1.5 % with tagged ones (no ballot of "a lane holds a leaf" per turn
 * any more: profiles/r05_ab_divloop_array_and_global_thresholds.txt) */
#ifndef PT_BOUNCE_MIN_CHUNKS
#define PT_BOUNCE_MIN_CHUNKS 2 /* chunks per wave below which fewer workgroups take part (k_shade_pool: 16 -- there a chunk is a few microseconds) */
#endif
/* (k_bounce's shade steps read slot kinds / spheres / triangles, and a finished ray's shading category (PtSceneView.cat), from the LDS
 * image instead of global memory.) */
#ifndef PT_DIAG_FLOOR
#define PT_DIAG_FLOOR 0 /* diagnostic builds only: 1 = k_bounce returns once the scene image is in LDS, 2 = at once (the launch floor) */
#endif
#ifndef PT_BOUNCE_FENCE_WG
#define PT_BOUNCE_FENCE_WG 0 /* 1: always workgroup-scope fences (s_waitcnt vmcnt(0)) around the wave's own hit / parked records instead of wavefront
                                scope; at run time: PTX_BOUNCE_FENCE_WG=1 (k_bounce's fence_wg argument) */
#endif
/* LDS_SCENE = false (round 5): the same kernel for scenes walked from HBM / L2 over the per-octant node image (PtThreadOctTag; the
 * host launches it when PtSceneDev.nodes32o exists): the walk is k_trace's (threaded, binary32 filter, chunk cut at
 * PT_TAIL_CUT_GLOBAL with the third parked word for 32-bit node indices and slots, camera rays walked one per lane and parked like
 * any other), the pools and shade steps are the ones above, nothing of the scene is copied to LDS but the pre-tested floor
 * triangles, and the hit slot no longer travels through memory between two launches. */
/* SOLO (round 5): the small launches at the end of a batch.  Once a bounce's input has shrunk to PtSolo.max_entries queue entries, a
 * launch is a fixed cost -- the gap to the previous launch, the scene image built in LDS again, a handful of waves with one chunk
 * each and their drain -- and a frame of few pixels (one rank's share of an 8-rank job, the reference's 600 x 300 command) consists
 * of little else: 14 of its 16 launches per batch sat on that floor.  Paths are independent, so nothing requires the bounces of
 * DIFFERENT workgroups to stay in step: the first launch that finds its input that small runs ALL remaining bounces -- every
 * workgroup keeps its static share, notes the output blocks it takes (pt_pool_push), and after a workgroup barrier reads exactly
 * those blocks back as the next bounce's input, the scene image still in LDS.  It leaves its bounce number + 1 in PtSolo.flag; the
 * batch's later launches find it and return at once.  Workgroups drift apart in bounce number, so nothing written during the
 * launch may be overwritten during it: each of the two queue buffers hands out blocks from ONE cursor for the whole launch (the
 * buffer that holds the launch's input starts behind it), and the launch runs solo only if the buffers are large enough for
 * every remaining bounce's survivors and holes in the worst case.  Same walks, same shade steps, same sampler dimensions per bounce: the
 * results do not depend on the order of a queue, so they are the step-by-step launches' bit for bit. */
/* a workgroup-wide lock in LDS for the few-instruction critical sections of the parked-walk pool (every lane of the wave calls both) */
__device__ __forceinline__ void pt_lds_lock(uint32_t* l) {
  if (pt_lane() == 0)
    while (__hip_atomic_exchange(l, 1u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u) __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void pt_lds_unlock(uint32_t* l) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (pt_lane() == 0) __hip_atomic_store(l, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
/* The workgroup's parked walks (PtTailCtl): a stack of records in LDS under a count and a lock.  A wave that parks walks, or takes up to
 * 64 up again, brackets its own record stores / loads with a begin, which takes the lock and says where they go, and an end, which
 * leaves the new count and the lock.  Every lane of the wave calls both; what they return is wave-uniform. */
struct PtParkSpan {
  uint32_t base, take; /* records base .. base + take - 1 */
};
/* the most recently parked 64, or what is left once this wave's share of the input is exhausted (!more); take == 0: another wave was faster */
__device__ __forceinline__ PtParkSpan pt_park_take_begin(uint32_t* park_n, uint32_t* park_lock, bool more) {
  pt_lds_lock(park_lock);
  const uint32_t np = __hip_atomic_load(park_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  PtParkSpan s;
  s.take = (np >= (uint32_t)PT_WAVE || !more) ? (np < (uint32_t)PT_WAVE ? np : (uint32_t)PT_WAVE) : 0u;
  s.base = np - s.take;
  return s;
}
__device__ __forceinline__ void pt_park_take_end(uint32_t* park_n, uint32_t* park_lock, PtParkSpan s) {
  if (pt_lane() == 0 && s.take) __hip_atomic_store(park_n, s.base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  pt_lds_unlock(park_lock);
}
/* the lanes of mask pm (not empty) park: the lane's record is base + its rank among them */
__device__ __forceinline__ uint32_t pt_park_put_begin(uint32_t* park_n, uint32_t* park_lock) {
  pt_lds_lock(park_lock);
  return __hip_atomic_load(park_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void pt_park_put_end(uint32_t* park_n, uint32_t* park_lock, uint32_t base, unsigned long long pm) {
  if (pt_lane() == 0) __hip_atomic_store(park_n, base + (uint32_t)__popcll(pm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  pt_lds_unlock(park_lock);
}
/* A wave's own stores (hit records, parked states, pool entries) before its own later loads of them: program order is enough for
 * that (one wave's vector memory instructions reach the L1 / L2 in order), the compiler must not move them -- wavefront scope.
 * wg (PT_BOUNCE_FENCE_WG, or PTX_BOUNCE_FENCE_WG=1 at run time; wave-uniform): workgroup-scope fences instead -- every store of the
 * turn is waited for (s_waitcnt vmcnt(0)) before the wave goes on.  The safety net should the in-order assumption ever fail on some
 * part; the parity tests run both (tests/test_gpu_parity.py). */
__device__ __forceinline__ void pt_own_fence(bool wg) {
  if (wg) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}
struct PtSolo {
  uint32_t* flag;       /* per batch, zero at its start; null = never run solo */
  uint32_t max_entries; /* run solo when the input queue holds at most this many entries (0 = never) */
  int32_t max_bounces;
  uint32_t cap_entries; /* capacity of each of the two queues, in entries */
};
#ifndef PT_SOLO_ONE_BIN_CHUNKS
#define PT_SOLO_ONE_BIN_CHUNKS 2 /* a workgroup whose input of a solo turn is at most this many chunks per wave puts all survivors into one bin */
#endif
/* (PT_SOLO_MAX_BLOCKS: pt_lds_layout.h) */
template <int MODE, bool COUNT, bool EMIT, bool PRIMARY, bool LDS_SCENE = true, bool SOLO_T = false, bool LIT = false, bool LANE_WALK = false /* (PRIMARY && LDS_SCENE: k_bounce_carry) */, bool IMG = false>
__global__ __launch_bounds__(IMG ? PT_BOUNCE_THREADS_IMG : PT_BOUNCE_THREADS, IMG ? PT_IMG_WAVES : PT_BOUNCE_WAVES) void k_bounce(PtSceneDev sc, PtQueue q, PtHits hits, PtQueue out, PtContrib contrib,
                                                                 const double* __restrict__ alpha, int bounce, int last_bounce, PtGenParams g,
                                                                 uint32_t n_primary, int stack_depth, uint32_t pool_off,
                                                                 PtCounters* counters, int fence_wg, PtSolo solo) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  __shared__ uint32_t lds_out[PT_POOL_BINS];
  __shared__ uint32_t lds_chunk_ctr, lds_done;
  __shared__ uint32_t lds_park_n, lds_park_lock; /* the workgroup's parked walks (below) */
  /* (a template switch, launched only when PTX_SOLO_ENTRIES asks for it: the loop around the bounces costs the kernel 6 - 11 VGPRs it does
   * not have -- the instantiations without it keep 0 spilled registers) */
  constexpr bool SOLO = SOLO_T && !PRIMARY && PT_DIAG == 0 && PT_DIAG_FLOOR == 0;
  __shared__ uint32_t lds_blk[SOLO ? 2 : 1][SOLO ? PT_SOLO_MAX_BLOCKS : 1]; /* the blocks this workgroup wrote in the bounce before / is writing now */
  __shared__ uint32_t lds_nblk[2];
  const int lane = pt_lane(), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
  typedef typename std::conditional<LDS_SCENE, uint16_t, PtThreadOctTag>::type StackT;
  StackT* stack = (StackT*)(lds_raw + (size_t)wave * PT_WAVE_STACK_BYTES(LDS_SCENE, stack_depth));
  const uint32_t n = PRIMARY ? n_primary : *q.count;
  const uint32_t total_chunks = (uint32_t)(((unsigned long long)n + PT_WAVE - 1) / PT_WAVE);
  PT_SHARE_WGS(n_wg, total_chunks, PT_BOUNCE_MIN_CHUNKS, nw);
  bool solo_on = false; /* launch-uniform */
  if (SOLO && solo.flag != nullptr) {
    const uint32_t f = __hip_atomic_load(solo.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (f != 0u && f != (uint32_t)bounce + 1u) return; /* an earlier launch of this batch ran (or is the one running) this bounce */
    /* the largest share of this launch in output blocks: runs of PT_POOL_RUN chunks dealt round-robin, every entry a survivor, one
     * part-filled block per bin */
    const uint32_t runs = (total_chunks + PT_POOL_RUN - 1u) / PT_POOL_RUN;
    const uint32_t share_blocks = ((runs + n_wg - 1u) / n_wg) * PT_POOL_RUN * PT_WAVE / PT_POOL_BLOCK + PT_POOL_BINS;
    /* each buffer takes the output of every second remaining bounce: at most the launch's input + one part-filled block per
     * (workgroup, bin) each time, the input's buffer behind the input */
    const unsigned long long per_bounce = (unsigned long long)n + (unsigned long long)n_wg * PT_POOL_BINS * PT_POOL_BLOCK;
    const unsigned long long worst = (unsigned long long)((solo.max_bounces - bounce) / 2 + 1) * per_bounce + (unsigned long long)n + PT_POOL_BLOCK;
    solo_on = !last_bounce && n <= solo.max_entries && share_blocks <= (uint32_t)PT_SOLO_MAX_BLOCKS && worst <= (unsigned long long)solo.cap_entries;
    if (solo_on && blockIdx.x == 0 && threadIdx.x == 0) {
      __hip_atomic_store(solo.flag, (uint32_t)bounce + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (COUNT) atomicAdd(&counters->solo, 1ull);
    }
  }
  if (COUNT && PRIMARY && LDS_SCENE && LANE_WALK && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters->lane_walks, 1ull);
  if (blockIdx.x >= n_wg) return; /* workgroup-uniform */
#if PT_DIAG_FLOOR == 2
  if (gridDim.x > 0) return; /* diagnostic build (tools/README.md): what a launch costs before it does anything */
#endif
  if (threadIdx.x == 0) { lds_chunk_ctr = 0u; lds_done = 0u; lds_nblk[0] = lds_nblk[1] = 0u; lds_park_n = 0u; lds_park_lock = 0u; }
  if (threadIdx.x < PT_POOL_BINS) lds_out[threadIdx.x] = (PT_POOL_NO_BLOCK << 12) | (uint32_t)PT_POOL_BLOCK; /* "full": the first push brings a block */
  PtSceneView sv = pt_scene_view<MODE, LDS_SCENE>(sc, lds_raw, stack_depth); /* LDS_SCENE: ends with the workgroup's only barrier (SOLO: per bounce, two more) */
  if (!LDS_SCENE) {
    __shared__ double lds_floor[PT_FLOOR_LDS * 10];
    PT_STAGE_FLOOR(MODE, sc, sv, lds_floor); /* ends with the workgroup's only barrier */
  }
#if PT_DIAG_FLOOR == 1
  if (gridDim.x > 0) return; /* diagnostic build: launch + the scene image in LDS, nothing else */
#endif
  /* the shade steps read the slots' kinds and geometry where the walk reads them: the LDS image (generic pointers: flat loads) */
  PtSceneDev scl = sc;
  if (LDS_SCENE) {
    scl.slot_kind = sv.kind;
    scl.sph = sv.sph;
    scl.tri = sv.tri;
  }
  /* the wave's five pools: queue indices (32 bits) and hit slots apart -- an LDS-resident scene has fewer than 65536 slots, so
   * its slots take 16 bits: 6 bytes per entry instead of 8, 20 KB of a 1024-thread workgroup's LDS for the scene image */
  typedef typename std::conditional<LDS_SCENE, uint16_t, uint32_t>::type PoolSlotT;
  constexpr int CUT = LDS_SCENE ? PT_TAIL_CUT : PT_TAIL_CUT_GLOBAL;
  constexpr bool TAIL = CUT > 0 && !(PRIMARY && LDS_SCENE); /* LDS scenes: camera rays walk as a packet (pt_trace_packet), or one per lane without a cut (LANE_WALK), and finish together */
  constexpr bool TAIL_UV = TAIL && MODE == PT_MODE_ARRAY;
  constexpr bool TAIL_W = TAIL && !LDS_SCENE; /* 32-bit node index and slot: a third 16 bytes (as in k_trace) */
  /* (the regions behind pool_off: pt_lds_layout.h; of the workgroup's pools a wave's five are its own) */
  uint32_t (*pool_i)[128];
  PoolSlotT (*pool_s)[128];
#define PT_POOL_AT(region, off_) region = (decltype(region))(lds_raw + off_) + (size_t)wave * PT_N_SHADE_CAT
  PT_LDS_BOUNCE_POOLS(PT_POOL_AT, pool_off, nw);
#undef PT_POOL_AT
  uint32_t cnt[PT_N_SHADE_CAT];
#pragma unroll
  for (int k = 0; k < PT_N_SHADE_CAT; ++k) cnt[k] = 0u;
  /* Parked walks (PtTailCtl) are pooled per WORKGROUP in LDS, behind the shade pools: whichever wave next looks for work and finds
   * 64 of them walks them as a dense chunk.  (Round 4 kept them per wave, in global memory: a wave had to collect 48 of its own
   * stragglers -- three or four cut chunks -- before it could resume any, which is what held the cut at 16 rays.)  An entry's
   * 16-byte words: pt_tail_head; the pool's lock and count: pt_park_take_begin. */
  const uint32_t park_cap = (uint32_t)PT_PARK_CAP(nw, CUT);
  uint4 *park0, *park_uv, *park_w, *park_end;
#define PT_PARK_AT(region, off_) region = (uint4*)(lds_raw + off_)
#define PT_PARK_AFTER(region, prev, words_) region = prev + (words_)
  PT_LDS_BOUNCE_PARK(PT_PARK_AT, PT_PARK_AFTER, pool_off, nw, LDS_SCENE, TAIL_UV, park_cap);
#undef PT_PARK_AT
#undef PT_PARK_AFTER
  (void)park_end;
  bool more = true;    /* wave-uniform: the workgroup's share of the queue is not exhausted */
  unsigned long long c_nodes = 0, c_prims = 0, c_floor = 0, c_seg = 0, c_filter[2] = {0, 0}; /* COUNT: as in k_trace */
  /* SOLO: the bounce this workgroup is at, its queues, and whether its input is the block list it noted in the bounce before */
  uint32_t own_chunks = 0u, cur_list = 0u; /* own_blocks: chunks of lds_blk[cur_list]; pushes note into lds_blk[cur_list ^ 1] */
  bool own_blocks = false;
  uint32_t* const solo_cursor[2] = {out.count, out.count + 1}; /* the block cursors of the buffer written first / of the input's buffer */
  uint32_t solo_turn = 0u;
  if (SOLO && solo_on) hits.t += (size_t)(bounce & 1) * hits.t_parity_stride;
  /* PT_DIAG == 5 (tools/diag_phases.py; counting renders of diagnostic builds, queued rays' launches): where a wave's life goes,
   * in ticks of the 100 MHz clock summed over waves -- nodes = walks, prims = shade steps (with their pushes), floor = everything
   * else in the loop (chunk hand-out, ray loads, filing, parking), segments = the whole loop; undecided / fallback_steps = the
   * number of shade steps / walks */
  constexpr bool DIAG_T = COUNT && (((PT_DIAG == 5 || PT_DIAG == 6 || PT_DIAG == 7) && !PRIMARY) || (PT_DIAG == 8 && PRIMARY)); /* 8: as 5, the camera rays' launches */ /* 6: prims = the walks' leaf phases instead of the shade steps; 7: prims = the pushes alone */
  PtPhaseClock<DIAG_T> clk;
  clk.start();
 for (;;) { /* (one turn per bounce; a launch that does not run solo leaves after the first) */
  for (;;) {
    clk.tick(c_floor);
    const uint32_t park_hint = TAIL ? __hip_atomic_load(&lds_park_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u; /* (wave-uniform: one LDS word) */
    const bool input_left = more || park_hint > 0;
    /* the fullest pool that holds a whole step; once nothing is left to walk, the fullest pool */
    int c = -1;
    uint32_t best = input_left ? (uint32_t)(PT_WAVE - 1) : 0u;
#pragma unroll
    for (int k = 0; k < PT_N_SHADE_CAT; ++k)
      if (cnt[k] > best) { best = cnt[k]; c = k; }
    if (c >= 0) {
      const uint32_t take = best < (uint32_t)PT_WAVE ? best : (uint32_t)PT_WAVE;
      const uint32_t start = best - take;
      const bool live = (uint32_t)lane < take;
      uint32_t i = 0u;
      int sl = -1;
      PtShadeOut so;
      so.keep = false;
#define PT_POOL_STEP(K, ...)                                                                                               \
  case K: {                                                                                                                \
    cnt[K] = start;                                                                                                        \
    if (live) {                                                                                                            \
      i = pool_i[K][start + lane];                                                                                         \
      sl = (int)pool_s[K][start + lane];                                                                                   \
      if (LDS_SCENE && sl == 0xffff) sl = -1; /* (misses are filed with slot -1) */                                        \
    }                                                                                                                      \
    pt_shade_entry<EMIT, PRIMARY, K, LIT, IMG>(LDS_SCENE ? scl : sc, q, hits, contrib, alpha, bounce, last_bounce, g, i, live, so, ##__VA_ARGS__); \
  } break;
      switch (c) {
        PT_POOL_STEP(PT_CAT_MISS)
        PT_POOL_STEP(PT_CAT_LAMBERT_SOLID, sl)
        PT_POOL_STEP(PT_CAT_LAMBERT_CHECKER, sl)
        PT_POOL_STEP(PT_CAT_METAL, sl)
        PT_POOL_STEP(PT_CAT_DIELECTRIC, sl)
        default: break;
      }
#undef PT_POOL_STEP
      if (PT_DIAG == 7) clk.tick(c_floor);
      if (c != PT_CAT_MISS && !last_bounce) {
        if (SOLO && solo_on) pt_pool_push<EMIT>(sc, out, so, lds_out, lds_blk[SOLO ? (cur_list ^ 1u) : 0u], &lds_nblk[cur_list ^ 1u],
                                                own_blocks && own_chunks <= (uint32_t)(PT_SOLO_ONE_BIN_CHUNKS * nw));
        else pt_pool_push<EMIT>(sc, out, so, lds_out);
      }
      if (PT_DIAG == 6) clk.tick(c_floor);
      else clk.tick(c_prims);
      if (DIAG_T) c_filter[0] += (lane == 0);
      continue;
    }
    if (!input_left) break;
    /* walk: 64 parked rays once enough have gathered (or nothing else is left), else the next chunk of the share */
    bool resume = false, valid = false;
    uint32_t i = 0;
    uint4 parked = make_uint4(0, 0, 0, 0), parked_uv = make_uint4(0, 0, 0, 0), parked_w = make_uint4(0, 0, 0, 0);
    if (TAIL && (park_hint >= (uint32_t)PT_WAVE || (!more && park_hint > 0))) {
      /* 64 parked walks (the most recently parked: a stack), or what is left once this wave's share of the input is exhausted */
      const PtParkSpan s = pt_park_take_begin(&lds_park_n, &lds_park_lock, more);
      if ((uint32_t)lane < s.take) {
        parked = park0[s.base + lane];
        if (TAIL_UV) parked_uv = park_uv[s.base + lane];
        if (TAIL_W) parked_w = park_w[s.base + lane];
      }
      pt_park_take_end(&lds_park_n, &lds_park_lock, s);
      if (s.take == 0u) continue; /* (another wave was faster) */
      resume = true;
      valid = (uint32_t)lane < s.take;
      i = parked.x;
    } else {
      if (!more) continue; /* (only here when the hint and the pool disagreed a moment ago) */
      /* the next chunk of the workgroup's share (PT_SHARE_NEXT;
       * taking a chunk one turn ahead and touching its ray records cost 2 % in round 3 and 3.5 % (cornell 5 %) in round 4: a line
       * touched ~10 us early is evicted from the L2 again before the wave comes back for it, and is then fetched twice) */
      PT_SHARE_NEXT(unit, lds_chunk_ctr, lane);
      if (SOLO && own_blocks) { /* the workgroup's own blocks of the bounce before (block | entries written << 20), PT_POOL_BLOCK / 64 chunks each */
        more = unit < own_chunks;
        if (more) {
          const uint32_t e = lds_blk[SOLO ? cur_list : 0u][unit / (PT_POOL_BLOCK / PT_WAVE)];
          const uint32_t fill = e >> 20, off = (unit % (PT_POOL_BLOCK / PT_WAVE)) * PT_WAVE;
          if (off >= fill) continue; /* (wave-uniform) the unwritten part of a bin's last block: nothing to read, nothing was marked */
          i = (e & 0xfffffu) * (uint32_t)PT_POOL_BLOCK + off + (uint32_t)lane;
          valid = off + (uint32_t)lane < fill;
        }
      } else {
        unit = PT_SHARE_CHUNK(unit, n_wg);
        more = unit < total_chunks;
        if (more) {
          i = unit * PT_WAVE + (uint32_t)lane;
          valid = i < n;
        }
      }
    }
    PT_CHUNK_RAY(PRIMARY, sc, g, alpha, q, i, valid, o, d, (void)0);
    if (COUNT && !DIAG_T && valid && !resume) c_seg++;
    PtTailCtl tc;
    tc.min_active = (TAIL && more) ? CUT : 0; /* the last chunks of a wave run to completion */
    tc.resume = resume && valid;
    tc.node = TAIL_W ? parked_w.x : pt_tail_node_of(parked.y);
    tc.slot = TAIL_W ? (int)parked_w.y : pt_tail_slot_of(parked.y);
    tc.t = pt_unpack_hi(parked);
    tc.u = pt_unpack_lo(parked_uv);
    tc.v = pt_unpack_hi(parked_uv);
    tc.unfinished = false;
    PtTraceResult r;
    clk.tick(c_floor);
    unsigned long long dg_n = 0, dg_p = 0, dg_f = 0; /* (diagnostic builds: the walk's own counters go nowhere) */
    if constexpr (PRIMARY && LDS_SCENE && !LANE_WALK) r = pt_trace_packet<MODE, COUNT, true, true>(sc, sv, (uint32_t*)stack, valid, o, d, DIAG_T ? dg_n : c_nodes, DIAG_T ? dg_p : c_prims, DIAG_T ? dg_f : c_floor, DIAG_T ? nullptr : c_filter);
    else r = pt_trace_ray<MODE, COUNT, PRIMARY, StackT, LDS_SCENE, true, LDS_SCENE && !COUNT && MODE == PT_MODE_SIMD /* (Array_leaf kernels have no registers to pin: cornell +0.5 %; the walk from HBM / L2 in assembly: +1.9 %, profiles/r05_ab_oct_asm.txt) */>(sc, sv, stack, o, d, DIAG_T ? dg_n : c_nodes, DIAG_T ? dg_p : c_prims, DIAG_T ? dg_f : c_floor, valid, TAIL ? &tc : nullptr, DIAG_T ? nullptr : c_filter);
    clk.tick(c_nodes);
    if (DIAG_T) c_filter[1] += (lane == 0);
    const bool park = TAIL && tc.unfinished;
    const bool done = valid && !park;
    int cat = PT_CAT_NONE;
    if (done) {
      /* the hit distance (and a triangle's barycentrics) reach the shade step through memory -- this wave's own L1 / L2
       * lines; the slot travels in the pool entry */
      if (!(MODE == PT_MODE_ARRAY && sc.has_triangles)) hits.t[i] = r.t; /* (else the shade step recomputes it: PtHits) */
      cat = r.slot < 0 ? PT_CAT_MISS : (int)sv.cat[r.slot]; /* (walks from HBM / L2: sv.cat is sc.slot_cat) */
    }
#pragma unroll
    for (int k = 0; k < PT_N_SHADE_CAT; ++k) {
      const unsigned long long m = __ballot(cat == k);
      if (cat == k) {
        const uint32_t at = cnt[k] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        pool_i[k][at] = i;
        pool_s[k][at] = (PoolSlotT)r.slot;
      }
      cnt[k] += (uint32_t)__popcll(m);
    }
    if (TAIL) {
      const unsigned long long pm = __ballot(park);
      if (pm != 0) {
        const uint32_t base = pt_park_put_begin(&lds_park_n, &lds_park_lock);
        if (park) {
          const uint32_t k = base + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
          park0[k] = pt_tail_head(i, tc.node, r.slot, r.t);
          if (TAIL_W) park_w[k] = pt_tail_wide(tc.node, r.slot);
          if (TAIL_UV) park_uv[k] = pt_pack2(r.u, r.v);
        }
        pt_park_put_end(&lds_park_n, &lds_park_lock, base, pm);
      }
    }
    pt_own_fence(PT_BOUNCE_FENCE_WG || fence_wg); /* this turn's hit records, parked states and pool entries */
  }
  if (!(SOLO && solo_on) || last_bounce) break;
  /* SOLO: this workgroup's next bounce.  Every wave has filed, shaded and pushed its last ray of this one when the barrier
   * opens; the unused tails of the part-filled blocks become holes, the blocks noted by the pushes become the input. */
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); /* the survivors' records, for the other waves of this workgroup */
  __syncthreads();
  {
    /* how far each noted block was written: a bin's last block up to its cursor, every other one completely.  The next turn reads
     * exactly that much -- no holes are marked, none are looked for */
    const uint32_t nb = lds_nblk[cur_list ^ 1u];
    for (uint32_t t = threadIdx.x; t < nb; t += blockDim.x) {
      const uint32_t blk = lds_blk[SOLO ? (cur_list ^ 1u) : 0u][t];
      uint32_t fill = (uint32_t)PT_POOL_BLOCK;
      for (int b = 0; b < PT_POOL_BINS; ++b) {
        const uint32_t st = lds_out[b];
        if ((st >> 12) == blk) fill = st & 0xfffu;
      }
      lds_blk[SOLO ? (cur_list ^ 1u) : 0u][t] = blk | (fill << 20);
    }
    own_chunks = nb * (uint32_t)(PT_POOL_BLOCK / PT_WAVE);
  }
  __syncthreads(); /* everybody has read the bins and the list's length */
  if (threadIdx.x == 0) {
    lds_chunk_ctr = 0u;
    lds_nblk[cur_list] = 0u;
    /* the input's buffer is written from the second turn on: its cursor starts behind the launch's input (idempotent) */
    if (solo_turn == 0u) atomicMax(solo_cursor[1], ((n + (uint32_t)PT_POOL_BLOCK - 1u) / (uint32_t)PT_POOL_BLOCK) * (uint32_t)PT_POOL_BLOCK);
  }
  if (threadIdx.x < PT_POOL_BINS) lds_out[threadIdx.x] = (PT_POOL_NO_BLOCK << 12) | (uint32_t)PT_POOL_BLOCK;
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (own_chunks == 0u) break; /* (workgroup-uniform) none of this workgroup's paths is left */
  cur_list ^= 1u;
  own_blocks = true;
  more = true;
  ++bounce;
  last_bounce = bounce == solo.max_bounces - 1;
  { const PtQueue t_ = q; q = out; out = t_; }
  ++solo_turn;
  out.count = solo_cursor[solo_turn & 1u];
  hits.t += (bounce & 1) ? (ptrdiff_t)hits.t_parity_stride : -(ptrdiff_t)hits.t_parity_stride;
 }
  if (DIAG_T) {
    clk.tick(c_floor);
    c_seg = (lane == 0) ? clk.life() : 0ull;
    if (lane != 0) c_nodes = c_prims = c_floor = 0ull; /* wave-uniform quantities: one lane's copy */
  }
  if (COUNT && !(PT_DIAG != 0 && (PRIMARY != (PT_DIAG == 8)))) /* (diagnostic builds measure the queued rays' launches only; 8: the camera rays') */
    pt_counters_flush(counters, c_nodes, c_prims, c_floor, c_seg, c_filter);
  if (last_bounce || (SOLO && solo_on)) return; /* (a solo launch leaves no queue behind: its paths have all ended) */
  pt_blocks_close_rays(&lds_done, lds_out, nw, out);
}

/* ------------------------------------------------------------------ a bounce launch that shades first and walks second
 * k_bounce above is walk(b) -> pools -> shade(b) -> push: the shade step gathers by pool index, one to several chunks after the
 * walk read them densely, the ray it walked, the path record and the hit distance -- and the L2 has let go of them by then: 190 B
 * of fabric reads per segment against 88 B of records.  k_bounce_carry turns the loop round.  A queue ENTRY CARRIES ITS HIT: the
 * ray, the path record, and in PtHits at the entry's own index the slot and the distance of the hit the ray has already found.
 * Survivors are binned by the shading category of that hit, a block is single-bin, so a chunk of 64 entries is one category by
 * construction, as a pool step is.  A wave's turn in launch b:
 *     read a chunk densely, once -> pt_shade_entry<CAT> of bounce b on the lane's own entry -> the new ray is in registers ->
 *     walk it at once (bounce b + 1) -> a miss ends the path on the spot, a hit is pushed as {new ray,
 *     path record, slot, t} under its category.
 * (The key of the next walk's length that pt_bin_key takes from the new direction is gone: that direction does not exist until the
 * next launch has shaded.  Predicting it for the checker category from the sampler value the scatter will use, two and four levels,
 * measured slower than no key: DESIGN.md Appendix A.)
 * Nothing is gathered, nothing is read twice, no pools.  Launches per batch stay max_bounces:
 *     launch 0 (PRIMARY)         camera rays as a packet walk -> shade 0 in place, category by category -> walk 1 -> push
 *     launch b, 0 < b < last     shade b -> walk b + 1 -> push
 *     the last launch            shade only: nothing survives it.
 * A walk the tail cut stops has its ray nowhere in memory, so the parked record is the whole entry (ray, path record, node, slot,
 * t [, emission] [, u, v]); the workgroup-level pool, its lock and "resume 64 at a time" are k_bounce's.  Holes are marked in the
 * slot array (PT_SLOT_HOLE) and skipped before they are shaded.  Same arithmetic, same tests per ray in the same order; which wave
 * does what when, and the order of a queue, change -- which no result depends on.  `hits` belongs to the input queue (launch 0:
 * to the camera samples), `hout` to the output queue. */
static_assert(PT_POOL_BINS >= PT_N_SHADE_CAT, "k_bounce_carry: one output bin per shading category");

/* LANE_WALK (PRIMARY launches, PTX_PRIMARY_WALK): the camera rays walk one per lane through pt_trace_ray -- on Simd_leaf scenes the
 * assembly node loop the queued rays use -- instead of as a wave packet.  A ray's tests and their order are the same in both. */
/* LOCT (Schedule::lds_oct; Simd_leaf, not counting, camera rays one per lane): the workgroup holds the per-octant LDS image (PtLdsOctTag)
 * in place of the stacks and the shared node image; pool_off is then pt_lds_oct_layout's. */
/* TILE (Schedule::tile_lists; LOCT camera launches): sc.tile_lists holds the image's camera tile lists (scene_host.h, PtTileRec); a chunk
 * whose tile has a list scans it (pt_tile_scan.h) instead of walking the tree, unless the record says "walk", a live ray's octant is not
 * the record's, or a guard of the scan fires -- then the chunk walks as without the flag. */
template <int MODE, bool COUNT, bool EMIT, bool PRIMARY, bool LANE_WALK = false, bool LOCT = false, bool TILE = false>
__global__ __launch_bounds__(PT_BOUNCE_THREADS, PT_BOUNCE_WAVES) void k_bounce_carry(PtSceneDev sc, PtQueue q, PtHits hits, PtQueue out, PtHits hout, PtContrib contrib,
                                                                 const double* __restrict__ alpha, int bounce, int last_bounce, PtGenParams g,
                                                                 uint32_t n_primary, int stack_depth, uint32_t pool_off,
                                                                 PtCounters* counters, int fence_wg) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  __shared__ uint32_t lds_out[PT_POOL_BINS];
  __shared__ uint32_t lds_chunk_ctr, lds_done;
  __shared__ uint32_t lds_park_n, lds_park_lock;
  const int lane = pt_lane(), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
  static_assert(!LOCT || (MODE == PT_MODE_SIMD && !COUNT && (!PRIMARY || LANE_WALK)), "the per-octant LDS image: Simd_leaf, not counting, no packet walk");
  static_assert(!TILE || (LOCT && PRIMARY), "camera tile lists: the camera launch on the per-octant LDS image");
  typedef typename std::conditional<LOCT, PtLdsOctTag, uint16_t>::type StackT;
  StackT* stack = LOCT ? nullptr : (StackT*)(lds_raw + (size_t)wave * PT_WAVE_STACK_BYTES(true, stack_depth));
  const uint32_t n = PRIMARY ? n_primary : *q.count;
  const uint32_t total_chunks = (uint32_t)(((unsigned long long)n + PT_WAVE - 1) / PT_WAVE);
  PT_SHARE_WGS(n_wg, total_chunks, PT_BOUNCE_MIN_CHUNKS, nw);
  if (COUNT && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters->carry, 1ull);
  if (COUNT && PRIMARY && LANE_WALK && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counters->lane_walks, 1ull);
  if (blockIdx.x >= n_wg) return; /* workgroup-uniform */
  if (threadIdx.x == 0) { lds_chunk_ctr = 0u; lds_done = 0u; lds_park_n = 0u; lds_park_lock = 0u; }
  if (threadIdx.x < PT_POOL_BINS) lds_out[threadIdx.x] = (PT_POOL_NO_BLOCK << 12) | (uint32_t)PT_POOL_BLOCK; /* "full": the first push brings a block */
  PtSceneView sv = pt_scene_view<MODE, true, LOCT>(sc, lds_raw, stack_depth); /* ends with the workgroup's only barrier */
  PtSceneDev scl = sc; /* the shade steps read the slots' kinds and geometry where the walk reads them (k_bounce) */
  scl.slot_kind = sv.kind;
  scl.sph = sv.sph;
  scl.tri = sv.tri;
  constexpr int CUT = PT_TAIL_CUT;
  constexpr bool TAIL = CUT > 0;
  constexpr bool TAIL_UV = TAIL && MODE == PT_MODE_ARRAY;
  /* the workgroup's parked walks behind the scene image (there are no pools): one array of 16-byte words per field (PT_CARRY_PARK_WORDS) */
  const uint32_t park_cap = (uint32_t)PT_PARK_CAP(nw, CUT);
  uint4 *park0, *park_emit, *park_uv, *park_end;
#define PT_PARK_AT(region, off_) region = (uint4*)(lds_raw + off_)
#define PT_PARK_AFTER(region, prev, words_) region = prev + (words_)
  PT_LDS_CARRY_REGIONS(PT_PARK_AT, PT_PARK_AFTER, pool_off, EMIT, TAIL_UV, park_cap);
#undef PT_PARK_AT
#undef PT_PARK_AFTER
  (void)park_end;
  bool more = true; /* wave-uniform: the workgroup's share of the input (launch 0: of the camera samples) is not exhausted */
  unsigned long long c_nodes = 0, c_prims = 0, c_floor = 0, c_seg = 0, c_filter[2] = {0, 0}; /* COUNT: as in k_trace */
  /* PT_DIAG == 8 (tools/diag_phases.py; counting renders of diagnostic builds, the camera launch): where a wave's life goes, in ticks
   * of the 100 MHz clock summed over waves -- nodes = chunk hand-out + ray set-up + the camera walk, prims = shade 0, floor = bounce 1's
   * walk (resumed walks included), undecided = pushes + parking, segments = the whole loop; fallback_steps = the number of tile turns.
   * The queued rays' launches add nothing */
  constexpr bool DIAG_T = COUNT && PT_DIAG == 8 && PRIMARY;
  PtPhaseClock<DIAG_T> clk;
  clk.start();
  unsigned long long dg_n = 0, dg_p = 0, dg_f = 0; /* (diagnostic builds: the walks' own counters go nowhere) */
  for (;;) {
    clk.tick(c_filter[0]);
    const uint32_t park_hint = TAIL ? __hip_atomic_load(&lds_park_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u; /* (wave-uniform: one LDS word) */
    /* what this turn walks: the lane's ray, and the rest of the entry it will push */
    bool resume = false, valid = false;
    V3 o = v3(0.0, 0.0, 0.0), d = v3(0.0, 0.0, -1.0), attn = v3(0.0, 0.0, 0.0), emit = v3(0.0, 0.0, 0.0);
    uint32_t id = 0u;
    int offset = 0;
    PtTailCtl tc;
    tc.node = 0u;
    tc.slot = -1;
    tc.t = tc.u = tc.v = 0.0;
    if (TAIL && (park_hint >= (uint32_t)PT_WAVE || (!more && park_hint > 0))) {
      /* 64 parked walks (the most recently parked: a stack), or what is left once this wave's share of the input is exhausted */
      const PtParkSpan s = pt_park_take_begin(&lds_park_n, &lds_park_lock, more);
      if ((uint32_t)lane < s.take) {
        const uint32_t base = s.base;
        const uint4* p = park0 + base + lane;
        const uint4 h = p[0], r0 = p[park_cap], r1 = p[2u * park_cap], r2 = p[3u * park_cap], a0 = p[4u * park_cap], a1 = p[5u * park_cap];
        tc.node = pt_tail_node_of(h.x);
        tc.slot = pt_tail_slot_of(h.x);
        offset = (int)h.y;
        tc.t = pt_unpack_hi(h);
        o = v3(pt_unpack_lo(r0), pt_unpack_hi(r0), pt_unpack_lo(r1));
        d = v3(pt_unpack_hi(r1), pt_unpack_lo(r2), pt_unpack_hi(r2));
        attn = v3(pt_unpack_lo(a0), pt_unpack_hi(a0), pt_unpack_lo(a1));
        id = a1.z;
        if (EMIT) {
          const uint4 e0 = park_emit[base + lane], e1 = park_emit[park_cap + base + lane];
          emit = v3(pt_unpack_lo(e0), pt_unpack_hi(e0), pt_unpack_lo(e1));
        }
        if (TAIL_UV) {
          const uint4 w = park_uv[base + lane];
          tc.u = pt_unpack_lo(w);
          tc.v = pt_unpack_hi(w);
        }
      }
      pt_park_take_end(&lds_park_n, &lds_park_lock, s);
      if (s.take == 0u) continue; /* (another wave was faster) */
      resume = true;
      valid = (uint32_t)lane < s.take;
    } else {
      /* a shade step on the next chunk of the share: 64 entries of one category by construction (launch 0: 64 camera samples) */
      int c = -1;
      uint32_t i = 0u;
      int sl = -1;
      bool live = false;
      int my_cat = PT_CAT_NONE; /* PRIMARY: the lane's own category (a chunk of camera samples may hold several) */
      if (!more) {
        if (park_hint > 0) continue;
        break;
      }
      PT_SHARE_NEXT(unit, lds_chunk_ctr, lane); /* the next chunk of the workgroup's share */
      unit = PT_SHARE_CHUNK(unit, n_wg);
      more = unit < total_chunks;
      if (!more) continue;
      i = unit * PT_WAVE + (uint32_t)lane;
      if (PRIMARY) {
        /* camera samples: generate, walk as a packet or one ray per lane (LANE_WALK; k_bounce's front half).  The hit goes straight to the shade steps below:
         * a chunk is one 8 x 8 tile of one pass, mostly one category, so there are no pools -- each category present is shaded
         * in turn, its lanes live */
        live = i < n;
        int tile_x = 0, tile_gy = 0; /* TILE: the lane's pixel column and GLOBAL row (lane 0: the tile's first) */
        PtPrimarySample ps;
        ps.x = ps.y = ps.gy = ps.pass_in_batch = ps.offset = 0;
        ps.id = 0u;
        ps.valid = false;
        if (live) {
          ps = pt_primary_decode(g, i);
          live = ps.valid;
          tile_x = ps.x;
          tile_gy = ps.gy;
        }
        /* TILE: the chunk's record is requested here, as soon as lane 0's tile is known, so that the camera direction's arithmetic
         * covers the load (lane 0 holds the tile's first pixel, inside the image whenever any lane is live; the record's index is
         * checked against the grid before it forms an address) */
        int recv = 0;
        bool rec_ok = false; /* wave-uniform */
        if constexpr (TILE) {
          const uint32_t gtx = (uint32_t)(g.width + 7) >> 3, gty = (uint32_t)(g.height + 7) >> 3;
          const uint32_t tx = (uint32_t)__builtin_amdgcn_readfirstlane(tile_x) >> 3, ty = (uint32_t)__builtin_amdgcn_readfirstlane(tile_gy) >> 3;
          rec_ok = __ballot(live) != 0ull && tx < gtx && ty < gty;
          if (rec_ok) {
            /* the 32-byte record: lane k < 16 reads halfword k, the header and the slot numbers come out of it by readlane and stay scalar */
            const uint16_t* rec = (const uint16_t*)sc.tile_lists + ((size_t)ty * gtx + tx) * 16u;
            recv = (int)rec[lane & 15];
          }
        }
        if (live) {
          d = pt_primary_dir(sc, g, ps, alpha);
          id = ps.id; /* (what a survivor of shade 0 is pushed with: the step leaves them alone) */
          offset = ps.offset;
        }
        if (COUNT && !DIAG_T && live) c_seg++;
        PtTraceResult r;
        bool scanned = false; /* wave-uniform */
        if constexpr (TILE) {
          if (rec_ok) {
            const uint32_t head = (uint32_t)__builtin_amdgcn_readlane(recv, 0);
            const uint32_t n_list = head & 0xffu, oct = head >> 8;
            const uint32_t dirs = (d.x >= 0.0 ? 1u : 0u) | (d.y >= 0.0 ? 2u : 0u) | (d.z >= 0.0 ? 4u : 0u); /* PtTraverser::begin */
            if (n_list != PT_TILE_WALK && __ballot(live && dirs != oct) == 0ull) {
              const PtTileHit th = pt_tile_scan<true>(sv.sph, [&](int k) { return (uint32_t)__builtin_amdgcn_readlane(recv, k + 1); },
                                                      [](bool b) { return __builtin_amdgcn_ballot_w64(b) != 0ull; }, (int)n_list, live, d, PT_MAX_FINITE);
              if (__ballot(th.guard) == 0ull) {
                scanned = true;
                r.t = th.t;
                r.slot = th.slot;
                r.u = 0.0;
                r.v = 0.0;
              } else if (lane == 0) {
                atomicAdd(&counters->tile_fallbacks, 1ull);
              }
            }
          }
        }
        if (scanned) {
        } else if constexpr (LANE_WALK) /* no tail cut: the tile runs to completion */
          r = pt_trace_ray<MODE, COUNT, true, StackT, true, true, !COUNT && MODE == PT_MODE_SIMD>(sc, sv, stack, o, d, DIAG_T ? dg_n : c_nodes, DIAG_T ? dg_p : c_prims, DIAG_T ? dg_f : c_floor, live, nullptr, DIAG_T ? nullptr : c_filter);
        else r = pt_trace_packet<MODE, COUNT, true, true>(sc, sv, (uint32_t*)stack, live, o, d, DIAG_T ? dg_n : c_nodes, DIAG_T ? dg_p : c_prims, DIAG_T ? dg_f : c_floor, DIAG_T ? nullptr : c_filter);
        /* shade 0 runs in this lane on what it holds: the sample, the direction and the hit distance stay in registers; nothing is
         * stored to hits.t and there is nothing to fence (fence_wg: the queued launches never used it either).  They stay in the
         * registers of what the turn walks next, which a lane does not need before its own category step has run: the path id and the
         * sampler offset where a survivor's are, the camera direction in d, the hit distance in o.x (a camera ray's origin is zero) */
        if (live) {
          sl = r.slot;
          my_cat = r.slot < 0 ? PT_CAT_MISS : (int)sv.cat[r.slot];
        }
        o = v3(r.t, 0.0, 0.0);
        (void)fence_wg;
        clk.tick(c_nodes);
        if (DIAG_T) c_filter[1] += (lane == 0);
      } else {
        sl = i < n ? hits.slot[i] : PT_SLOT_HOLE;
        live = sl != PT_SLOT_HOLE;
        /* the chunk's category: its first entry's (a block holds one bin, a bin one category) */
        const unsigned long long lm = __ballot(live);
        if (lm == 0ull) continue; /* the unwritten part of a bin's last block */
        my_cat = !live ? PT_CAT_NONE : (sl < 0 ? PT_CAT_MISS : (int)sv.cat[sl]);
        c = __builtin_amdgcn_readlane(my_cat, __ffsll((long long)lm) - 1);
      }
      /* (PRIMARY: every category some lane holds, in turn; else the chunk's one) */
#define PT_CARRY_STEP(K, SLOT)                                                                                         \
  if (PRIMARY ? __ballot(my_cat == K) != 0ull : c == K) {                                                              \
    PtShadeOut so;                                                                                                     \
    const PtCameraCarry cam = pt_camera_carry(id, offset, live, d, o.x);                                               \
    pt_shade_entry<EMIT, PRIMARY, K>(scl, q, hits, contrib, alpha, bounce, last_bounce, g, i, live && my_cat == K, so, SLOT, PRIMARY ? &cam : nullptr); \
    if (so.keep) {                                                                                                     \
      valid = true;                                                                                                    \
      o = so.n_o;                                                                                                      \
      d = so.n_d;                                                                                                      \
      attn = so.n_attn;                                                                                                \
      emit = so.n_emit;                                                                                                \
      if (!PRIMARY) { /* (the camera launch holds them since the sample was decoded) */                               \
        id = so.id;                                                                                                    \
        offset = so.offset;                                                                                            \
      }                                                                                                                \
    }                                                                                                                  \
  }
      PT_CARRY_STEP(PT_CAT_MISS, PT_SLOT_HOLE)
      PT_CARRY_STEP(PT_CAT_LAMBERT_SOLID, sl)
      PT_CARRY_STEP(PT_CAT_LAMBERT_CHECKER, sl)
      PT_CARRY_STEP(PT_CAT_METAL, sl)
      PT_CARRY_STEP(PT_CAT_DIELECTRIC, sl)
#undef PT_CARRY_STEP
      if (PRIMARY && !valid) { /* no ray to walk: the lane's registers as every other turn leaves them */
        o = v3(0.0, 0.0, 0.0);
        d = v3(0.0, 0.0, -1.0);
      }
      clk.tick(c_prims);
      if (last_bounce || __ballot(valid) == 0ull) continue; /* nothing survives the step */
      if (COUNT && !DIAG_T && valid) c_seg++;
    }
    /* walk the new rays (or go on with the parked ones); the last chunks of a wave run to completion */
    tc.min_active = (TAIL && more) ? CUT : 0;
    tc.resume = resume && valid;
    tc.unfinished = false;
    const PtTraceResult r = pt_trace_ray<MODE, COUNT, false, StackT, true, true, !COUNT && MODE == PT_MODE_SIMD>(sc, sv, stack, o, d, DIAG_T ? dg_n : c_nodes, DIAG_T ? dg_p : c_prims, DIAG_T ? dg_f : c_floor, valid, TAIL ? &tc : nullptr, DIAG_T ? nullptr : c_filter);
    clk.tick(c_floor);
    const bool park = TAIL && tc.unfinished;
    const bool done = valid && !park;
    const int cat = !done ? PT_CAT_NONE : (r.slot < 0 ? PT_CAT_MISS : (int)sv.cat[r.slot]);
    /* a ray that left the scene ends its path here: pt_shade_entry<PT_CAT_MISS>'s one line on the registers that hold its operands
     * (None -> add_mul emit0 attn0 background, integrator.ml:36), instead of an entry for the next launch to read back */
    if (cat == PT_CAT_MISS) {
      const V3 result = v3_fma(attn, pt_background(sc, d), EMIT ? emit : v3(0.0, 0.0, 0.0));
      contrib.rgbx[id] = make_double4(result.x, result.y, result.z, 0.0);
    }
    const bool push = done && !(cat == PT_CAT_MISS); /* (written `cat != PT_CAT_MISS` the compiler merges the two tests of `cat` another way: other bytes, profiles/pr_lds_layout_identity.txt) */
    if (__ballot(push) != 0ull) {
      const uint32_t dst = pt_pool_reserve(out, push, push ? cat : 0, lds_out); /* the bin: the category, so that a chunk is one category */
      if (push) {
        pt_q_store<EMIT>(out, dst, o, d, attn, emit, id, offset);
        hout.slot[dst] = r.slot;
        if (!(MODE == PT_MODE_ARRAY && sc.has_triangles)) hout.t[dst] = r.t; /* (else the shade step recomputes it: PtHits) */
      }
    }
    if (TAIL) {
      const unsigned long long pm = __ballot(park);
      if (pm != 0) {
        const uint32_t base = pt_park_put_begin(&lds_park_n, &lds_park_lock);
        if (park) {
          uint4* p = park0 + base + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
          p[0] = pt_pack_xy_t(pt_tail_node_slot(tc.node, r.slot), (uint32_t)offset, r.t);
          p[park_cap] = pt_pack2(o.x, o.y);
          p[2u * park_cap] = pt_pack2(o.z, d.x);
          p[3u * park_cap] = pt_pack2(d.y, d.z);
          p[4u * park_cap] = pt_pack2(attn.x, attn.y);
          p[5u * park_cap] = pt_pack_t_xy(attn.z, id, 0u);
          if (EMIT) {
            p[6u * park_cap] = pt_pack2(emit.x, emit.y);
            p[7u * park_cap] = pt_pack_t_xy(emit.z, 0u, 0u);
          }
          if (TAIL_UV) p[(EMIT ? 8u : 6u) * park_cap] = pt_pack2(r.u, r.v);
        }
        pt_park_put_end(&lds_park_n, &lds_park_lock, base, pm);
      }
    }
  }
  if (DIAG_T) {
    clk.tick(c_filter[0]);
    c_seg = (lane == 0) ? clk.life() : 0ull;
    if (lane != 0) c_nodes = c_prims = c_floor = c_filter[0] = 0ull; /* wave-uniform quantities: one lane's copy */
  }
  if (COUNT && !(PT_DIAG == 8 && !PRIMARY)) /* (that diagnostic build measures the camera launch only) */
    pt_counters_flush(counters, c_nodes, c_prims, c_floor, c_seg, c_filter);
  if (last_bounce) return;
  pt_blocks_close(&lds_done, lds_out, nw, [&](size_t e) { hout.slot[e] = PT_SLOT_HOLE; }); /* (holes of a carried queue: in the slot array) */
}

/* ------------------------------------------------------------------ accumulate + film */
/* raw[pix] += contributions of this batch's passes, in pass order (the order render_tile's pass loop
 * feeds the film, integrator.ml:96) */
/* The sample-sum core of k_accum, k_accum_sq and k_accum_list: pixel p's sums += contributions j, j + stride, ... of n_pass passes.
 * SQ: sq also gets each channel's squared contribution in the same pass order, s = s + c * c (the build has -ffp-contract=off, so
 * the product is rounded before the add, as numpy's s + c * c does) */
template <bool SQ>
__device__ __forceinline__ void pt_accum_pixel(const PtContrib& contrib, long long j, long long stride, int n_pass, long long p,
                                               double* __restrict__ raw, double* __restrict__ sq) {
  double r = raw[3 * p], g = raw[3 * p + 1], b = raw[3 * p + 2];
  double sr = 0.0, sg = 0.0, sb = 0.0;
  if (SQ) {
    sr = sq[3 * p];
    sg = sq[3 * p + 1];
    sb = sq[3 * p + 2];
  }
  for (int k = 0; k < n_pass; ++k) {
    const double4 c = contrib.rgbx[(long long)k * stride + j];
    r = r + c.x;
    g = g + c.y;
    b = b + c.z;
    if (SQ) {
      sr = sr + c.x * c.x;
      sg = sg + c.y * c.y;
      sb = sb + c.z * c.z;
    }
  }
  raw[3 * p] = r;
  raw[3 * p + 1] = g;
  raw[3 * p + 2] = b;
  if (SQ) {
    sq[3 * p] = sr;
    sq[3 * p + 1] = sg;
    sq[3 * p + 2] = sb;
  }
}
/* [p0, p1): the pixels of this launch -- the whole image, or one row slab of the frame's last batch (ptx_render: the film and the
 * copy of slab k to the host run while slab k + 1 is still being summed) */
__global__ __launch_bounds__(256) void k_accum(PtContrib contrib, long long npix, int n_pass, double* __restrict__ raw, long long p0, long long p1) {
  const long long p = p0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= p1) return;
  pt_accum_pixel<false>(contrib, p, npix, n_pass, p, raw, nullptr);
}

struct PtFilm3 {
  double w[9];
};
/* Where image row y lives in the raw-sum buffer the film reads.  world <= 1: row y of a (height x width) image.
 * world > 1: the buffer is the GATHERED multi-rank layout [rank][pad_rows][width][3] -- rank r's compact rows exactly
 * as ptx_render_raw_device left them (interleaved bands r, r + world, ... of band_rows rows) -- so the film reads the
 * bands in place and rank 0 never un-permutes them. */
struct PtBandMap {
  int world, band_rows, pad_rows;
};
__device__ __forceinline__ long long pt_band_row(const PtBandMap& m, int y) {
  if (m.world <= 1) return y;
  const int band = y / m.band_rows;
  const int rank = band % m.world;
  const int local = (band / m.world) * m.band_rows + (y - band * m.band_rows);
  return (long long)rank * m.pad_rows + local;
}
/* Film_tile.write_pixel splats sample s at its own pixel q to q + (dx, dy) with weight k[dy][dx]
 * (film_tile.ml:23-45); stitch_tile drops what falls outside the image (integrator.ml:114-128).  As a
 * gather: P = sum_taps k[dy][dx] * S(P - (dx, dy)) over in-image neighbours, then sqrt(v * (1/spp)). */
__global__ __launch_bounds__(256) void k_film(const double* __restrict__ raw, int width, int height, double spp_inv,
                                              PtFilm3 kern, PtBandMap map, double* __restrict__ out, int row0, int row1) {
  const long long p = (long long)row0 * width + (long long)blockIdx.x * blockDim.x + threadIdx.x; /* rows [row0, row1) of the image */
  if (p >= (long long)width * row1) return;
  const int x = (int)(p % width), y = (int)(p / width);
  double r = 0.0, g = 0.0, b = 0.0;
  int k = 0;
  for (int dy = -1; dy <= 1; ++dy) {
    const int sy = y - dy;
    const long long srow = (sy >= 0 && sy < height) ? pt_band_row(map, sy) : 0;
    for (int dx = -1; dx <= 1; ++dx, ++k) {
      const int sx = x - dx;
      if (sx < 0 || sx >= width || sy < 0 || sy >= height) continue;
      const double* s = raw + (srow * width + sx) * 3;
      const double wgt = kern.w[k];
      r = pt_fma(wgt, s[0], r);
      g = pt_fma(wgt, s[1], g);
      b = pt_fma(wgt, s[2], b);
    }
  }
  out[3 * p] = pt_sqrt(r * spp_inv);
  out[3 * p + 1] = pt_sqrt(g * spp_inv);
  out[3 * p + 2] = pt_sqrt(b * spp_inv);
}

/* ------------------------------------------------------------------ progressive rendering: second moments + per-pixel error */
/* k_accum that also sums each channel's squared contribution into sq (pt_accum_pixel<true>) */
__global__ __launch_bounds__(256) void k_accum_sq(PtContrib contrib, long long npix, int n_pass, double* __restrict__ raw,
                                                  double* __restrict__ sq, long long p0, long long p1) {
  const long long p = p0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= p1) return;
  pt_accum_pixel<true>(contrib, p, npix, n_pass, p, raw, sq);
}

/* Standard error of a pixel channel's sample mean after k passes, from S1 = sum c and S2 = sum c^2:
 * se = sqrt(max(0, S2 - S1 * S1 / k) / (k (k - 1))) for k >= 2, +inf below.  This is the estimate for INDEPENDENT samples; the
 * sampler is a low-discrepancy sequence, so it usually overestimates the error of the rendered mean. */
__device__ __forceinline__ double pt_pixel_se(double s1, double s2, double kd) {
  if (!(kd >= 2.0)) return __builtin_inf();
  const double v = s2 - s1 * s1 / kd;
  return pt_sqrt((v > 0.0 ? v : 0.0) / (kd * (kd - 1.0)));
}

constexpr int PT_ERR_THREADS = 256;
/* The workgroup's (se^2, mean^2) pairs summed in a fixed tree order (no atomics: the same sums give the same bits on every run);
 * thread 0 finds the totals in lds_se[0] and lds_mean[0] */
__device__ __forceinline__ void pt_error_block_sum(double se2, double mean2, double* lds_se, double* lds_mean) {
  lds_se[threadIdx.x] = se2;
  lds_mean[threadIdx.x] = mean2;
  for (int off = PT_ERR_THREADS / 2; off > 0; off >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < off) {
      lds_se[threadIdx.x] = lds_se[threadIdx.x] + lds_se[threadIdx.x + off];
      lds_mean[threadIdx.x] = lds_mean[threadIdx.x] + lds_mean[threadIdx.x + off];
    }
  }
}
/* The body of k_pixel_error and k_pixel_error_counts.  One pixel per thread, after k passes (COUNTS: the pixel's own passes[p]):
 * err (optional, 3 per pixel) and, per workgroup, partials[2 block] = sum of se^2 and partials[2 block + 1] = sum of
 * (S1 / k)^2 over its pixels and channels (pt_error_block_sum) */
template <bool COUNTS>
__device__ __forceinline__ void pt_pixel_error_block(const double* __restrict__ raw, const double* __restrict__ sq,
                                                     const int32_t* __restrict__ passes, int k, long long npix, double* __restrict__ err,
                                                     double* __restrict__ partials) {
  __shared__ double lds_se[PT_ERR_THREADS], lds_mean[PT_ERR_THREADS];
  const long long p = (long long)blockIdx.x * PT_ERR_THREADS + threadIdx.x;
  double se2 = 0.0, mean2 = 0.0;
  if (p < npix) {
    const double kd = (double)(COUNTS ? passes[p] : k);
    for (int c = 0; c < 3; ++c) {
      const double s1 = raw[3 * p + c], se = pt_pixel_se(s1, sq[3 * p + c], kd), m = s1 / kd;
      if (err) err[3 * p + c] = se;
      se2 = se2 + se * se;
      mean2 = mean2 + m * m;
    }
  }
  pt_error_block_sum(se2, mean2, lds_se, lds_mean);
  if (threadIdx.x == 0) {
    partials[2 * (long long)blockIdx.x] = lds_se[0];
    partials[2 * (long long)blockIdx.x + 1] = lds_mean[0];
  }
}
__global__ __launch_bounds__(PT_ERR_THREADS) void k_pixel_error(const double* __restrict__ raw, const double* __restrict__ sq,
                                                                long long npix, int k, double* __restrict__ err,
                                                                double* __restrict__ partials) {
  pt_pixel_error_block<false>(raw, sq, nullptr, k, npix, err, partials);
}

/* One workgroup: the frame summary rel_err = sqrt(sum se^2) / sqrt(sum mean^2) from k_pixel_error's n_blocks partial pairs, in a
 * fixed order (thread t sums blocks t, t + 256, ... in turn, then a tree); 0 when both sums are 0, +inf for k < 2 */
__global__ __launch_bounds__(PT_ERR_THREADS) void k_error_summary(const double* __restrict__ partials, long long n_blocks, int k,
                                                                  double* __restrict__ rel_err) {
  __shared__ double lds_se[PT_ERR_THREADS], lds_mean[PT_ERR_THREADS];
  double se2 = 0.0, mean2 = 0.0;
  for (long long b = threadIdx.x; b < n_blocks; b += PT_ERR_THREADS) {
    se2 = se2 + partials[2 * b];
    mean2 = mean2 + partials[2 * b + 1];
  }
  pt_error_block_sum(se2, mean2, lds_se, lds_mean);
  if (threadIdx.x == 0) {
    const double a = lds_se[0], m = lds_mean[0];
    *rel_err = k < 2 ? __builtin_inf() : (a == 0.0 && m == 0.0) ? 0.0 : pt_sqrt(a) / pt_sqrt(m);
  }
}

/* ------------------------------------------------------------------ adaptive sampling: pixel lists and per-pixel pass counts */
/* Every listed index lies in [0, npix): *bad (zeroed by the caller) is set to 1 otherwise.  Runs before anything else is queued. */
__global__ __launch_bounds__(256) void k_list_check(const int32_t* __restrict__ pix, long long n, long long npix, int32_t* __restrict__ bad) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t p = pix[j];
  if (p < 0 || (long long)p >= npix) *bad = 1;
}

/* k_accum / k_accum_sq over a pixel list: raw[pix[j]] += contributions pass_in_batch * n_list + j in pass order, sq (nullable) the
 * squares, as those kernels add them; passes (nullable: the count map) [pix[j]] = pass_end */
__global__ __launch_bounds__(256) void k_accum_list(PtContrib contrib, long long n_list, int n_pass, const int32_t* __restrict__ pix,
                                                    double* __restrict__ raw, double* __restrict__ sq, int32_t* __restrict__ passes,
                                                    int pass_end) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_list) return;
  const long long p = pix[j];
  if (sq) pt_accum_pixel<true>(contrib, j, n_list, n_pass, p, raw, sq);
  else pt_accum_pixel<false>(contrib, j, n_list, n_pass, p, raw, nullptr);
  if (passes) passes[p] = pass_end;
}

/* The stopping rule for a pixel after k passes, evaluated as written (the build has -ffp-contract=off):
 * se_c = pt_pixel_se(S1_c, S2_c, k), m_c = S1_c / k, e = sqrt((se_r^2 + se_g^2) + se_b^2), d = max(sqrt((m_r^2 + m_g^2) + m_b^2), F);
 * converged <=> T > 0 and e <= T * d */
__device__ __forceinline__ bool pt_adaptive_converged(const double* __restrict__ raw, const double* __restrict__ sq, long long p, double kd,
                                                      double target, double floor_) {
  const double s1r = raw[3 * p], s1g = raw[3 * p + 1], s1b = raw[3 * p + 2];
  const double ser = pt_pixel_se(s1r, sq[3 * p], kd), seg = pt_pixel_se(s1g, sq[3 * p + 1], kd), seb = pt_pixel_se(s1b, sq[3 * p + 2], kd);
  const double mr = s1r / kd, mg = s1g / kd, mb = s1b / kd;
  const double e = pt_sqrt((ser * ser + seg * seg) + seb * seb);
  const double m = pt_sqrt((mr * mr + mg * mg) + mb * mb);
  const double d = m > floor_ ? m : floor_;
  return target > 0.0 && e <= target * d;
}

constexpr int PT_SEL_THREADS = 256;
/* Entry j of the last round's list: pix[j], or with pix == nullptr the whole image in pt_primary_decode's 8x8-tile order (entry j is
 * tile j / 64, lane j % 64; lanes off the image are never kept) */
__device__ __forceinline__ long long pt_select_pixel(const int32_t* __restrict__ pix, long long j, int width, int height, int tiles_x) {
  if (pix) return pix[j];
  const int tile = (int)(j >> 6), lane = (int)(j & 63);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
  return (x < width && y < height) ? (long long)y * width + x : -1;
}
/* rank of this lane among the workgroup's kept lanes, and the workgroup's kept count (waves in order: no atomics) */
__device__ __forceinline__ uint32_t pt_select_rank(bool keep, uint32_t* lds_wave, uint32_t* total) {
  const unsigned long long m = __ballot(keep);
  const int lane = pt_lane(), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) lds_wave[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < PT_SEL_THREADS / 64; ++w) {
    if (w < wave) before += lds_wave[w];
    all += lds_wave[w];
  }
  *total = all;
  return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
/* select, step 1: keep[j] = the pixel has not converged after k passes; block_counts[block] = kept entries of the workgroup */
__global__ __launch_bounds__(PT_SEL_THREADS) void k_select_count(const int32_t* __restrict__ pix, long long n, int width, int height,
                                                                 int tiles_x, const double* __restrict__ raw, const double* __restrict__ sq,
                                                                 int k, double target, double floor_, uint8_t* __restrict__ keep,
                                                                 uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t lds_wave[PT_SEL_THREADS / 64];
  const long long j = (long long)blockIdx.x * PT_SEL_THREADS + threadIdx.x;
  bool kp = false;
  if (j < n) {
    const long long p = pt_select_pixel(pix, j, width, height, tiles_x);
    kp = p >= 0 && !pt_adaptive_converged(raw, sq, p, (double)k, target, floor_);
    keep[j] = kp ? 1 : 0;
  }
  uint32_t total = 0;
  (void)pt_select_rank(kp, lds_wave, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}
/* select, step 2 (one workgroup): block_offsets = the exclusive prefix sums of block_counts in block order, *n_next their total.
 * Thread t scans the blocks [t c, (t + 1) c) of a contiguous chunk, the chunks' totals are scanned in LDS. */
__global__ __launch_bounds__(PT_SEL_THREADS) void k_select_scan(const uint32_t* __restrict__ block_counts, long long n_blocks,
                                                                uint32_t* __restrict__ block_offsets, int32_t* __restrict__ n_next) {
  __shared__ uint32_t lds[PT_SEL_THREADS];
  const long long chunk = (n_blocks + PT_SEL_THREADS - 1) / PT_SEL_THREADS;
  const long long b0 = (long long)threadIdx.x * chunk, b1 = b0 + chunk < n_blocks ? b0 + chunk : n_blocks;
  uint32_t s = 0;
  for (long long b = b0; b < b1; ++b) s += block_counts[b];
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < PT_SEL_THREADS; off <<= 1) { /* inclusive Hillis-Steele scan of the chunk totals */
    const uint32_t v = (int)threadIdx.x >= off ? lds[threadIdx.x - off] : 0u;
    __syncthreads();
    lds[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = threadIdx.x > 0 ? lds[threadIdx.x - 1] : 0u;
  for (long long b = b0; b < b1; ++b) {
    block_offsets[b] = run;
    run += block_counts[b];
  }
  if (threadIdx.x == PT_SEL_THREADS - 1) *n_next = (int32_t)lds[PT_SEL_THREADS - 1];
}
/* select, step 3: the kept entries' pixels written to out in entry order (the next round's list) */
__global__ __launch_bounds__(PT_SEL_THREADS) void k_select_scatter(const int32_t* __restrict__ pix, long long n, int width, int height,
                                                                   int tiles_x, const uint8_t* __restrict__ keep,
                                                                   const uint32_t* __restrict__ block_offsets, int32_t* __restrict__ out) {
  __shared__ uint32_t lds_wave[PT_SEL_THREADS / 64];
  const long long j = (long long)blockIdx.x * PT_SEL_THREADS + threadIdx.x;
  const bool kp = j < n && keep[j] != 0;
  uint32_t total = 0;
  const uint32_t rank = pt_select_rank(kp, lds_wave, &total);
  if (kp) out[block_offsets[blockIdx.x] + rank] = (int32_t)pt_select_pixel(pix, j, width, height, tiles_x);
}

/* k_film with a per-pixel pass count n(q) (the count map).  Where every in-image tap has the same count n it is k_film with
 * spp_inv = 1.0 / n, bit for bit; elsewhere each tap contributes its own mean: sqrt(fma-sum(w * (S(q) * (1.0 / n(q))))). */
__global__ __launch_bounds__(256) void k_film_counts(const double* __restrict__ raw, const int32_t* __restrict__ passes, int width,
                                                     int height, PtFilm3 kern, double* __restrict__ out) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long long)width * height) return;
  const int x = (int)(p % width), y = (int)(p / width);
  const int n0 = passes[p];
  bool same = true;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int sx = x - dx, sy = y - dy;
      if (sx < 0 || sx >= width || sy < 0 || sy >= height) continue;
      if (passes[(long long)sy * width + sx] != n0) same = false;
    }
  double r = 0.0, g = 0.0, b = 0.0;
  int k = 0;
  for (int dy = -1; dy <= 1; ++dy) {
    const int sy = y - dy;
    for (int dx = -1; dx <= 1; ++dx, ++k) {
      const int sx = x - dx;
      if (sx < 0 || sx >= width || sy < 0 || sy >= height) continue;
      const long long q = (long long)sy * width + sx;
      const double* s = raw + q * 3;
      const double wgt = kern.w[k];
      if (same) {
        r = pt_fma(wgt, s[0], r);
        g = pt_fma(wgt, s[1], g);
        b = pt_fma(wgt, s[2], b);
      } else {
        const double inv = 1.0 / (double)passes[q];
        r = pt_fma(wgt, s[0] * inv, r);
        g = pt_fma(wgt, s[1] * inv, g);
        b = pt_fma(wgt, s[2] * inv, b);
      }
    }
  }
  if (same) {
    const double spp_inv = 1.0 / (double)n0;
    r = r * spp_inv;
    g = g * spp_inv;
    b = b * spp_inv;
  }
  out[3 * p] = pt_sqrt(r);
  out[3 * p + 1] = pt_sqrt(g);
  out[3 * p + 2] = pt_sqrt(b);
}

/* ------------------------------------------------------------------ the film at any order and radius (ptx_film_params) */
/* Binomial.create ~order ~pixel_radius for a run-time radius r in 0 .. 7: the rule of include/ptx.h, operation for operation.  A
 * 256-thread workgroup owns a 32 x 8 tile of output pixels.  It copies the tile and a halo of r pixels into LDS as three planes, one
 * per channel (the 24-byte pixel stride of the sums would put a wave's reads two to a bank; a plane's row is 32 consecutive doubles
 * per half wave, one per bank pair), 46 x 22 x 3 doubles = 24288 bytes at r = 7, then runs the (2r + 1)^2 taps from LDS in the rule's
 * order: dy outer, dx inner, one fma per channel.  Not separable: two 1-D passes would round differently.
 * The taps outside the image are skipped by clamping the two loop ranges (in-image is a range of dx and a range of dy), so the
 * interior runs without a per-tap test and the halo cells outside the image are never read (nor written).
 * COUNTS: a fourth plane holds the per-pixel pass counts n(q) (k_film_counts with a wider window). */
constexpr int PT_FILM_MAX_R = 7; /* PTX_FILM_MAX_RADIUS */
constexpr int PT_FILM_TX = 32, PT_FILM_TY = 8;
constexpr int PT_FILM_LW = PT_FILM_TX + 2 * PT_FILM_MAX_R, PT_FILM_LH = PT_FILM_TY + 2 * PT_FILM_MAX_R; /* the LDS tile: 46 x 22 */
constexpr int PT_FILM_PLANE = PT_FILM_LW * PT_FILM_LH;
struct PtFilmWide {
  int r;
  double w[2 * PT_FILM_MAX_R + 1]; /* the normalised 1-D weights, 2r + 1 of them */
};
/* image rows [row0, row1) (the tiles start at row0); passes != nullptr exactly when COUNTS */
template <bool COUNTS, bool RENORM>
__device__ __forceinline__ void pt_film_wide_tile(const double* __restrict__ raw, const int32_t* __restrict__ passes, int width, int height,
                                                  double spp_inv, const PtFilmWide& kern, const PtBandMap& map, double* __restrict__ out,
                                                  int row0, int row1, double* lds_s, int32_t* lds_n, double* lds_w) {
  const int r = kern.r, tid = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * PT_FILM_TX, y0 = row0 + (int)blockIdx.y * PT_FILM_TY;
  const int tw = PT_FILM_TX + 2 * r, th = PT_FILM_TY + 2 * r;
  if (tid <= 2 * r) lds_w[tid] = kern.w[tid];
  /* a tile row is 3 * tw consecutive doubles of the sums: consecutive lanes read consecutive doubles */
  const int row_d = 3 * tw;
  for (int i = tid; i < th * row_d; i += PT_FILM_TX * PT_FILM_TY) {
    const int ly = i / row_d, j = i - ly * row_d, lx = j / 3, c = j - 3 * lx;
    const int sx = x0 - r + lx, sy = y0 - r + ly;
    if (sx < 0 || sx >= width || sy < 0 || sy >= height) continue;
    lds_s[c * PT_FILM_PLANE + ly * PT_FILM_LW + lx] = raw[(pt_band_row(map, sy) * width + sx) * 3 + c];
  }
  if (COUNTS) {
    for (int i = tid; i < th * tw; i += PT_FILM_TX * PT_FILM_TY) {
      const int ly = i / tw, lx = i - ly * tw;
      const int sx = x0 - r + lx, sy = y0 - r + ly;
      if (sx < 0 || sx >= width || sy < 0 || sy >= height) continue;
      lds_n[ly * PT_FILM_LW + lx] = passes[(long long)sy * width + sx];
    }
  }
  __syncthreads();
  const int tx = tid % PT_FILM_TX, ty = tid / PT_FILM_TX;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= width || y >= row1) return;
  /* (x - dx, y - dy) is inside the image for dx in [dx_lo, dx_hi], dy in [dy_lo, dy_hi] */
  const int dx_lo = x - (width - 1) > -r ? x - (width - 1) : -r, dx_hi = x < r ? x : r;
  const int dy_lo = y - (height - 1) > -r ? y - (height - 1) : -r, dy_hi = y < r ? y : r;
  const bool clipped = dx_lo > -r || dx_hi < r || dy_lo > -r || dy_hi < r;
  const int centre = (ty + r) * PT_FILM_LW + tx + r;
  bool same = true;
  int n0 = 1;
  if (COUNTS) {
    n0 = lds_n[centre];
    for (int dy = dy_lo; dy <= dy_hi; ++dy)
      for (int dx = dx_lo; dx <= dx_hi; ++dx)
        if (lds_n[centre - dy * PT_FILM_LW - dx] != n0) same = false;
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, ws = 0.0;
  for (int dy = dy_lo; dy <= dy_hi; ++dy) {
    const double wy = lds_w[dy + r];
    const int qrow = centre - dy * PT_FILM_LW;
    for (int dx = dx_lo; dx <= dx_hi; ++dx) {
      const double wgt = wy * lds_w[dx + r];
      const int q = qrow - dx;
      double s0 = lds_s[q], s1 = lds_s[PT_FILM_PLANE + q], s2 = lds_s[2 * PT_FILM_PLANE + q];
      if (COUNTS && !same) {
        const double inv = 1.0 / (double)lds_n[q];
        s0 = s0 * inv;
        s1 = s1 * inv;
        s2 = s2 * inv;
      }
      a0 = pt_fma(wgt, s0, a0);
      a1 = pt_fma(wgt, s1, a1);
      a2 = pt_fma(wgt, s2, a2);
      if (RENORM) ws = ws + wgt;
    }
  }
  if (RENORM && clipped) {
    a0 = a0 / ws;
    a1 = a1 / ws;
    a2 = a2 / ws;
  }
  if (same) {
    const double inv = COUNTS ? 1.0 / (double)n0 : spp_inv;
    a0 = a0 * inv;
    a1 = a1 * inv;
    a2 = a2 * inv;
  }
  const long long p = (long long)y * width + x;
  out[3 * p] = pt_sqrt(a0);
  out[3 * p + 1] = pt_sqrt(a1);
  out[3 * p + 2] = pt_sqrt(a2);
}
/* k_film at any radius: grid (ceil(width / 32), ceil((row1 - row0) / 8)) */
template <bool RENORM>
__global__ __launch_bounds__(PT_FILM_TX * PT_FILM_TY) void k_film_wide(const double* __restrict__ raw, int width, int height, double spp_inv,
                                                                        PtFilmWide kern, PtBandMap map, double* __restrict__ out, int row0, int row1) {
  __shared__ double lds_s[3 * PT_FILM_PLANE];
  __shared__ double lds_w[2 * PT_FILM_MAX_R + 1];
  pt_film_wide_tile<false, RENORM>(raw, nullptr, width, height, spp_inv, kern, map, out, row0, row1, lds_s, nullptr, lds_w);
}
/* k_film_counts at any radius, over the whole image */
template <bool RENORM>
__global__ __launch_bounds__(PT_FILM_TX * PT_FILM_TY) void k_film_wide_counts(const double* __restrict__ raw, const int32_t* __restrict__ passes,
                                                                               int width, int height, PtFilmWide kern, double* __restrict__ out) {
  __shared__ double lds_s[3 * PT_FILM_PLANE];
  __shared__ int32_t lds_n[PT_FILM_PLANE];
  __shared__ double lds_w[2 * PT_FILM_MAX_R + 1];
  pt_film_wide_tile<true, RENORM>(raw, passes, width, height, 1.0, kern, PtBandMap{1, 1, 0}, out, 0, height, lds_s, lds_n, lds_w);
}

/* k_pixel_error with the pixel's own pass count k = passes[p]; the partials are k_error_summary's (called with k = 2: a pixel with
 * fewer than 2 passes has se = +inf, which the sums carry) */
__global__ __launch_bounds__(PT_ERR_THREADS) void k_pixel_error_counts(const double* __restrict__ raw, const double* __restrict__ sq,
                                                                       const int32_t* __restrict__ passes, long long npix,
                                                                       double* __restrict__ err, double* __restrict__ partials) {
  pt_pixel_error_block<true>(raw, sq, passes, 0, npix, err, partials);
}

/* ------------------------------------------------------------------ unit entry points */
__global__ void k_lds_sample(const double* __restrict__ alpha, long long n, const int32_t* __restrict__ offsets,
                             const int32_t* __restrict__ dims, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = pt_lds_get(alpha, offsets[i], dims[i]);
}

__global__ void k_math_eval(int fn, long long n, const double* __restrict__ a, const double* __restrict__ b,
                            double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], y = b ? b[i] : 0.0;
  double r;
  switch (fn) {
    case 0: r = pt_hypot(x, y); break;
    case 1: r = pt_sin(x); break;
    case 2: r = pt_cos(x); break;
    case 3: r = pt_acos(x); break;
    case 4: r = pt_atan2(x, y); break;
    case 5: r = pt_pow5(x); break;
    case 6: r = pt_sqrt(x); break;
    case 7: r = x / y; break;
    case 8: r = pt_fma(x, y, y); break;
    case 9: r = pt_rnorm3(x, y, x - y); break;             /* the fused forms against the oracle's nested literal ones */
    case 10: r = pt_rnorm_frame(1.0 + x, y, x - y); break;
    case 11: r = pt_sqrt_nonneg(x); break;
    case 12: r = pt_rcp_mid(x); break;                     /* mid-range operands only (pt_math.h) */
    case 13: r = pt_div_mid(x, y); break;
    case 14: r = pt_sqrt_mid(x); break;
    default: r = pt_nan(); break;
  }
  out[i] = r;
}

/* ptx_texture_eval / ptx_environment_eval: the shade step's own evaluation functions (the IMG arms) on explicit inputs */
__global__ void k_texture_eval(PtShadeRec rec, long long n, const double* __restrict__ uv, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PtMatRegs m = pt_mat_load<PT_CAT_NONE, false, true>(&rec);
  const V3 c = pt_texture_eval<true>(m, uv[2 * i], uv[2 * i + 1]);
  out[3 * i] = c.x;
  out[3 * i + 1] = c.y;
  out[3 * i + 2] = c.z;
}
__global__ void k_environment_eval(PtSceneDev sc, long long n, const double* __restrict__ dirs, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 c = pt_background<true>(sc, v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
  out[3 * i] = c.x;
  out[3 * i + 1] = c.y;
  out[3 * i + 2] = c.z;
}
/* ptx_environment_sample / ptx_environment_pdf: the shade step's two environment-sampling functions on explicit inputs */
__global__ void k_environment_sample(PtSceneDev sc, long long n, const double* __restrict__ ab, double* __restrict__ dirs, int32_t* __restrict__ texel) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int ix, iy;
  const V3 d = pt_env_sample(sc, ab[2 * i], ab[2 * i + 1], &ix, &iy);
  dirs[3 * i] = d.x;
  dirs[3 * i + 1] = d.y;
  dirs[3 * i + 2] = d.z;
  if (texel) {
    texel[2 * i] = ix;
    texel[2 * i + 1] = iy;
  }
}
__global__ void k_environment_pdf(PtSceneDev sc, long long n, const double* __restrict__ dirs, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = pt_env_pd(sc, v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
}

/* ptx_light_sample / ptx_light_pdf: the shade step's two light-half functions, triangles and spheres together, on explicit inputs */
__global__ void k_light_sample(PtSceneDev sc, long long n, const double* __restrict__ points, const double* __restrict__ uv,
                               double* __restrict__ dirs, int32_t* __restrict__ index) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int k;
  const V3 d = pt_light_sample(sc, v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), uv[2 * i], uv[2 * i + 1], &k);
  dirs[3 * i] = d.x;
  dirs[3 * i + 1] = d.y;
  dirs[3 * i + 2] = d.z;
  if (index) index[i] = k;
}
__global__ void k_light_pdf(PtSceneDev sc, long long n, const double* __restrict__ points, const double* __restrict__ dirs, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = pt_light_pd(sc, v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
}

/* copies explicit rays into a queue (ptx_intersect_rays) */
__global__ void k_load_rays(long long n, const double* __restrict__ o, const double* __restrict__ d, PtQueue q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pt_q_store_ray(q, (uint32_t)i, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
}

/* ptx_walk_rays: the walks of k_bounce / k_bounce_carry on LDS-resident scenes, on explicit rays.  Nothing of a walk is restated here:
 * the workgroup builds the scene image k_bounce_carry builds (pt_scene_view: the shared image behind the stacks, or the per-octant
 * one with LOCT) in a dynamic buffer of that kernel's size, and every wave hands 64 consecutive rays at a time to the instantiation of
 * pt_trace_ray / pt_trace_packet the bounce kernels use -- MODE == PT_MODE_SIMD: the assembly node loops (walk_asm, LOCT: walk_asm_oct),
 * else the divergent loop; ZERO: the camera launch's ORIGIN_ZERO forms (the origins are +0.0, the host has checked); PACKET: the
 * camera rays' wave packet.  Same launch bounds as k_bounce_carry: the assembly loops name v120..v127.
 * TAIL: a chunk stops where k_bounce_carry's would (PtTailCtl, min_active = PT_TAIL_CUT) and the walks it cut short go in again, with
 * the finished lanes idle, until none is left.  In between a walk is what k_bounce_carry's parked record keeps of it (word 0 of the
 * entry, written after its walk and read back before it: the node in 16 bits, the slot in 16 with 0xffff for none; t, and u, v on
 * Array_leaf scenes, as they are) -- through the kernel's own pair (pt_tail_node_slot); its pool, lock and ray words are not needed
 * for 64 lanes that keep their rays in registers. */
template <int MODE, bool PACKET, bool LOCT, bool ZERO, bool TAIL>
__global__ __launch_bounds__(PT_BOUNCE_THREADS, PT_BOUNCE_WAVES) void k_walk_eval(PtSceneDev sc, long long n, const double* __restrict__ o3,
                                                                                    const double* __restrict__ d3, double* __restrict__ t_out,
                                                                                    int32_t* __restrict__ slot_out, int stack_depth) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  static_assert(!LOCT || (MODE == PT_MODE_SIMD && !PACKET), "the per-octant LDS image: Simd_leaf, no packet walk");
  static_assert(!PACKET || (ZERO && !TAIL), "the packet walk is the camera rays': origin zero, no tail cut");
  static_assert(!(ZERO && TAIL), "the camera launch has no tail cut");
  typedef typename std::conditional<LOCT, PtLdsOctTag, uint16_t>::type StackT;
  const int lane = pt_lane(), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
  StackT* stack = LOCT ? nullptr : (StackT*)(lds_raw + (size_t)wave * PT_WAVE_STACK_BYTES(true, stack_depth));
  PtSceneView sv = pt_scene_view<MODE, true, LOCT>(sc, lds_raw, stack_depth); /* ends with the workgroup's only barrier */
  const long long chunks = (n + PT_WAVE - 1) / PT_WAVE;
  unsigned long long c_nodes = 0, c_prims = 0, c_floor = 0; /* (not counting: the walks leave them alone) */
  for (long long c = (long long)blockIdx.x * nw + wave; c < chunks; c += (long long)gridDim.x * nw) { /* wave-uniform */
    const long long i = c * PT_WAVE + lane;
    const bool valid = i < n;
    V3 o = v3(0.0, 0.0, 0.0), d = v3(0.0, 0.0, -1.0);
    if (valid) {
      if (!ZERO) o = v3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]);
      d = v3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
    }
    PtTraceResult r;
    if constexpr (PACKET) {
      r = pt_trace_packet<MODE, false, true, true>(sc, sv, (uint32_t*)stack, valid, o, d, c_nodes, c_prims, c_floor);
    } else if constexpr (!TAIL) {
      r = pt_trace_ray<MODE, false, ZERO, StackT, true, true, MODE == PT_MODE_SIMD>(sc, sv, stack, o, d, c_nodes, c_prims, c_floor, valid);
    } else {
      bool todo = valid; /* this lane's walk is not finished */
      PtTailCtl tc;
      tc.min_active = PT_TAIL_CUT;
      tc.resume = false;
      tc.node = 0u;
      tc.slot = -1;
      tc.t = tc.u = tc.v = 0.0;
      r.t = PT_MAX_FINITE;
      r.u = r.v = 0.0;
      r.slot = -1;
      for (;;) {
        tc.unfinished = false;
        const PtTraceResult rr = pt_trace_ray<MODE, false, false, StackT, true, true, MODE == PT_MODE_SIMD>(sc, sv, stack, o, d, c_nodes, c_prims, c_floor, todo, &tc);
        if (todo && !tc.unfinished) {
          r = rr;
          todo = false;
        }
        if (todo) { /* through the parked record's packed word, as k_bounce_carry parks a walk and takes it up again */
          const uint32_t w = pt_tail_node_slot(tc.node, rr.slot);
          tc.node = pt_tail_node_of(w);
          tc.slot = pt_tail_slot_of(w);
          tc.t = rr.t;
          tc.u = MODE == PT_MODE_ARRAY ? rr.u : 0.0; /* (park_uv: Array_leaf scenes only) */
          tc.v = MODE == PT_MODE_ARRAY ? rr.v : 0.0;
        }
        tc.resume = todo;
        if (__ballot(todo) == 0ull) break;
      }
    }
    if (valid) {
      t_out[i] = r.t;
      slot_out[i] = r.slot;
    }
  }
}

/* ptx_walk_next_leaf: the BOX DECISIONS of the same walks, one at a time.  Per (ray, node, closest hit so far) the first slot of the
 * next leaf whose box test the walk passes, starting with the visit of `node`; -1 when the walk runs off the tree first.  k_walk_eval's
 * shape (launch bounds, image, 64 triples per wave).  A lane is put where a resumed parked walk is put (pt_trace_ray, the
 * `tc->resume` block): begin(), then the node as the image's own link, r.t and update_t32().  Then the production node phase and
 * nothing else -- packet() is never called, so the closest hit stays the caller's and what comes out depends on box decisions alone.
 * Nothing of a visit is restated: the filter, nested_hit and slab64 are PtTraverser's.
 * The dispatch below is pt_trace_ray's node phase (its three `if constexpr` branches), spelled again: taking it out of pt_trace_ray
 * into a function of its own would hand the compiler other code for every kernel that inlines it.  Keep the two alike. */
template <int MODE, bool LOCT, bool ZERO>
__global__ __launch_bounds__(PT_BOUNCE_THREADS, PT_BOUNCE_WAVES) void k_next_leaf_eval(PtSceneDev sc, long long n, const double* __restrict__ o3,
                                                                                         const double* __restrict__ d3, const int32_t* __restrict__ node_in,
                                                                                         const double* __restrict__ t_max, int32_t* __restrict__ leaf_out,
                                                                                         int stack_depth) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  static_assert(!LOCT || MODE == PT_MODE_SIMD, "the per-octant LDS image: Simd_leaf");
  typedef typename std::conditional<LOCT, PtLdsOctTag, uint16_t>::type StackT;
  typedef PtTraverser<MODE, false, ZERO, StackT, true> Walk;
  constexpr int WALK_MIN = PT_WALK_MIN;
  const int lane = pt_lane(), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
  StackT* stack = LOCT ? nullptr : (StackT*)(lds_raw + (size_t)wave * PT_WAVE_STACK_BYTES(true, stack_depth));
  PtSceneView sv = pt_scene_view<MODE, true, LOCT>(sc, lds_raw, stack_depth); /* ends with the workgroup's only barrier */
  const long long chunks = (n + PT_WAVE - 1) / PT_WAVE;
  unsigned long long c_nodes = 0, c_prims = 0, no_count = 0; /* (not counting: the walk leaves them alone) */
  for (long long c = (long long)blockIdx.x * nw + wave; c < chunks; c += (long long)gridDim.x * nw) { /* wave-uniform */
    const long long i = c * PT_WAVE + lane;
    const bool valid = i < n;
    V3 o = v3(0.0, 0.0, 0.0), d = v3(0.0, 0.0, -1.0);
    uint32_t k = 0u;
    double tm = 0.0;
    if (valid) {
      if (!ZERO) o = v3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]);
      d = v3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
      k = (uint32_t)node_in[i]; /* 0 .. n_nodes - 1: the host has checked */
      tm = t_max[i];
    }
    Walk tr;
    tr.begin(sc, sv, o, d, no_count);
    /* a lane without a triple has ended; the others stand on node k of ptx_scene_tree's numbering: its record of the ray's octant
     * (LOCT: begin() left the octant's first record in skip_off), or its absolute LDS address in the shared image */
    if (LOCT) tr.node = valid ? tr.skip_off + k : (uint32_t)PT_LOCT_END;
    else tr.node = valid ? sv.swz_root + k * (uint32_t)PT_SWZ_NODE_BYTES : (uint32_t)PT_SWZ_END;
    tr.r.t = tm;
    tr.update_t32();
    while (tr.wants_node_mask() != 0ull) { /* wave-uniform: the node phase again until every lane holds a leaf or has ended */
      if constexpr ((PT_WALK_ASM != 0) && (PT_DIAG == 0) && MODE == PT_MODE_SIMD && LOCT) {
#if PT_WALK_ASM
        while (tr.walk_asm_oct(sv.oct_base, WALK_MIN) != 0ull)
          if (tr.wants_node()) tr.node_step(sv, stack, c_nodes, c_prims);
#endif
      } else if constexpr ((PT_WALK_ASM != 0) && (PT_DIAG == 0) && MODE == PT_MODE_SIMD) {
#if PT_WALK_ASM
        while (tr.walk_asm(WALK_MIN) != 0ull)
          if (tr.wants_node()) tr.node_step(sv, stack, c_nodes, c_prims);
#endif
      } else {
        if (tr.wants_node()) { /* pt_trace_ray's DIV_LOOP on a tagged image */
          const unsigned long long entered = __builtin_amdgcn_ballot_w64(true);
          for (;;) {
            tr.node_step(sv, stack, c_nodes, c_prims);
            if (!tr.wants_node()) break;
            const unsigned long long now = __builtin_amdgcn_ballot_w64(true);
            if (now != entered && pt_popc_mask(now) < WALK_MIN) break;
          }
        }
      }
    }
    if (valid) leaf_out[i] = tr.holds_leaf() ? tr.held_leaf_first(sv) : -1;
  }
}

#if PT_FILTER_DEBUG
/* Diagnostic builds only: the PRODUCTION box test of the walk from HBM / L2 (PtTraverser::begin + test_box on the tagged per-octant
 * record) on a list of (ray, node, closest hit so far) triples, and beside it the reference's binary64 quantities of the same test
 * (Bbox.is_hit, bbox.ml:40-56, the arithmetic of pt_slab_hit_fast: finite 1 / d only).  out[6 i ..] = u32, m2, lo64, hi64,
 * the filter's outcome (1 hit / 0 miss decided, -1 undecided), the outcome test_box returns (its fallback included). */
__global__ __launch_bounds__(256) void k_filter_error(PtSceneDev sc, long long n, const double* __restrict__ o3, const double* __restrict__ d3,
                                                      const int32_t* __restrict__ nodes, const double* __restrict__ tmax, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PtSceneView sv;
  sv.nodes = sc.nodes; sv.skip32 = sc.node_skip32; sv.nodes32 = (const unsigned char*)sc.nodes32; sv.nodes32o = (const unsigned char*)sc.nodes32o;
  sv.n_nodes = (uint32_t)sc.n_nodes; sv.swz_nodes = nullptr; sv.swz_root = 0u; sv.top = nullptr; sv.has_top = false; sv.sph = sc.sph; sv.tri = sc.tri;
  sv.kind = sc.slot_kind; sv.cat = sc.slot_cat; sv.nodes64 = nullptr; sv.floor_lds = nullptr; sv.n_floor_lds = 0;
  PtSceneDev scn = sc;
  scn.n_floor = 0; /* (no floor pre-test: the closest hit so far is the caller's) */
  const V3 o = v3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = v3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
  PtTraverser<PT_MODE_ARRAY, false, false, PtThreadOctTag, false> tr;
  unsigned long long cf = 0;
  tr.begin(scn, sv, o, d, cf);
  tr.r.t = tmax[i];
  tr.update_t32();
  const uint32_t k = (uint32_t)nodes[i];
  uint32_t na, nb, nr;
  const bool final_hit = tr.test_box(sv, tr.skip_off + k, na, nb, nr);
  const float u = tr.dbg_u, m2 = tr.dbg_m2;
  const PtNode* np = sc.nodes + k;
  const V3 inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
  const double t0x = (np->mn[0] - o.x) * inv.x, t0y = (np->mn[1] - o.y) * inv.y, t0z = (np->mn[2] - o.z) * inv.z;
  const double t1x = (np->mx[0] - o.x) * inv.x, t1y = (np->mx[1] - o.y) * inv.y, t1z = (np->mx[2] - o.z) * inv.z;
  const double a = __builtin_fmax(__builtin_fmin(t0x, t1x), __builtin_fmax(__builtin_fmin(t0y, t1y), __builtin_fmin(t0z, t1z)));
  const double b = __builtin_fmin(__builtin_fmax(t0x, t1x), __builtin_fmin(__builtin_fmax(t0y, t1y), __builtin_fmax(t0z, t1z)));
  double* r = out + 6 * i;
  r[0] = (double)u;
  r[1] = (double)m2;
  r[2] = __builtin_fmax(0.0, a);
  r[3] = __builtin_fmin(tmax[i], b);
  r[4] = (__builtin_fabsf(u) >= m2) ? (u >= m2 ? 1.0 : 0.0) : -1.0;
  r[5] = final_hit ? 1.0 : 0.0;
}
#endif

#ifndef PT_KERNELS_ONLY /* (tools/quick_kernel.sh instantiates single kernels of this file for register / ISA studies) */
#include "bvh_build_gpu.inc"
#include "ppm.inc"
#include "denoise.inc"
#include "temporal.inc"
#include "rays.inc"
#include "display.inc"
#include "ptx_api.inc"
#include "probes.inc"
#endif
