/* pt_lds_layout.h -- the ONE statement of what lies where in the dynamic LDS buffer of k_trace, k_bounce, k_bounce_carry and
 * k_shade_pool, and of which scenes are walked from an LDS copy at all.  Plain C++ (no HIP types): the kernels take their
 * pointers from these functions, the host (ptx_api.inc) sizes its launches with them, scene_host.cpp decides with them which node
 * images to build, and tests/c/asan_host_driver.cpp prints them (`layout` mode, tests/test_lds_layout.py).
 *
 * The buffer, in this order (a region a kernel does not have is empty):
 *   [per-wave stacks]   waves x stack_depth x 16 bytes (the camera rays' shared (node, mask) stack: 12 bytes per level), to 64
 *   [scene image]       nodes (PT_SWZ_NODE_BYTES each, to 64) | sphere slots (32 B) | triangle slots (80 B: Array_leaf scenes with
 *                       triangles) | slot kinds (Array_leaf, to 16) | shading categories (to 16) | binary64 bounds (48 B per node,
 *                       PtSceneDev.lds_nodes64)
 *   [k_bounce, at pool_off = the above to 64]   pool queue indices (waves x 5 x 128 x u32) | pool slots (u16; u32 from HBM / L2) |
 *                       parked walks: one array of park_cap 16-byte words each for {index, node | slot << 16, t} | {u, v}
 *                       (Array_leaf) | {node, slot} (walks from HBM / L2)
 *   [k_bounce_carry, at pool_off]   parked entries, one array of park_cap 16-byte words per field: 6 (PT_CARRY_PARK_WORDS) |
 *                       2 x emission (scenes with emitters) | {u, v} (Array_leaf)
 * A walk from HBM / L2 has no stacks and no image: k_bounce's pools start at 0, k_trace holds the tree's top (n_top x 64 bytes).
 * k_bounce_carry's non-counting launches on a Simd_leaf scene that fits with it hold the per-octant node image instead of stacks and
 * shared image: a region list and an admit decision of their own, PT_LDS_OCT_REGIONS / pt_lds_oct_layout below. */
#ifndef PT_LDS_LAYOUT_H
#define PT_LDS_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include "pt_scene.h"

#if defined(__HIPCC__)
#define PT_LDS_HD static __host__ __device__ __forceinline__
#else
#define PT_LDS_HD static inline
#endif

#define PT_N_SHADE_CAT 5 /* PT_CAT_MISS .. PT_CAT_DIELECTRIC */
#ifndef PT_TAIL_CUT
#define PT_TAIL_CUT 16 /* 0 = off */
#endif
#ifndef PT_TAIL_CUT_GLOBAL
/* scenes walked from HBM / L2 (k_trace): a step of the walk is a round trip to the L2, so lanes that idle while a chunk's long
 * rays finish cost more there, and a chunk is cut earlier.  Ganesha-like, per-octant node image: trace 23.7 (cut at 16) ->
 * 22.8 ms (24, 32); round 3 measured 24 / 32 within noise on the three-load walk. */
#define PT_TAIL_CUT_GLOBAL 32
#endif
#ifndef PT_SOLO_MAX_BLOCKS
#define PT_SOLO_MAX_BLOCKS 256 /* output blocks a workgroup can note per bounce; a launch whose shares could need more does not run solo */
#endif
#define PT_LDS_MAX_WAVES 16 /* the largest workgroup of any of these kernels: 1024 threads */

/* bytes of LDS a wave keeps for traversal stacks: LDS-resident scenes walk the threaded image (no per-lane stack) and
 * only the camera-ray packet walk keeps its shared (node, mask) stack there: 12 bytes per level, rounded to 16.  The walks from
 * HBM / L2 are threaded too and keep nothing. */
#define PT_WAVE_STACK_BYTES(LDS_SCENE, depth) ((LDS_SCENE) ? (size_t)(depth) * 16u : (size_t)0)
/* entries the parked-walk pool of a k_bounce workgroup of nw waves must hold: a wave takes a fresh chunk only while fewer than 64
 * walks are parked and parks fewer than the cut when it ends; a resumed chunk takes 64 out before it can put any back */
#define PT_PARK_CAP(nw, cut) (64 + (nw) * (cut))
#define PT_BOUNCE_POOL_ENTRY_BYTES(LDS_SCENE_) ((LDS_SCENE_) ? 6u : 8u) /* k_bounce's pool entries: 32-bit queue index + 16- / 32-bit slot */
/* 16-byte words of a parked entry: {node | slot << 16, offset, t}, 3 x ray, {attn.x, attn.y}, {attn.z, id} [, 2 x emission] [, {u, v}] */
#define PT_CARRY_PARK_WORDS(EMIT_, UV_) (6 + ((EMIT_) ? 2 : 0) + ((UV_) ? 1 : 0))

#define PT_LDS_CU_BYTES ((size_t)160 * 1024)
#define PT_LDS_SCENE_LIMIT ((size_t)80 * 1024) /* stacks + image of k_trace: 2 workgroups per CU */
/* dynamic LDS a k_bounce / k_bounce_carry launch may ask for: a CU's LDS less the kernel's own static words -- bins, counters, the floor
 * triangles, and in the instantiation that can run solo its two block lists.  A request beyond what the CU has does not fail
 * politely: the queue aborts, so the launchers also check the kernel's real static size once per instantiation. */
#define PT_LDS_BOUNCE_LIMIT (PT_LDS_CU_BYTES - (2 * PT_SOLO_MAX_BLOCKS * sizeof(uint32_t) + 512))
/* The 16-bit node references of the image are ABSOLUTE LDS addresses, multiples of 4 below PT_SWZ_END (0xfffe): the START of
 * every node must lie at or below 0xfffc.  Node k starts at base + stacks + k * PT_SWZ_NODE_BYTES, where base is the kernel's
 * static LDS rounded up to the dynamic array's alignment (64) and stacks <= PT_LDS_MAX_WAVES x stack_depth x 16 (a multiple of
 * 64).  pt_lds_placement admits a tree when 2048 + that + n_nodes * PT_SWZ_NODE_BYTES <= 65533, i.e. the last node starts at
 * or below base - 2048 + 65533 - PT_SWZ_NODE_BYTES, which is <= 0xfffc for every base <= 2048 + PT_SWZ_NODE_BYTES - 1 = 2139:
 * the test is sufficient for any kernel whose static LDS is at most that, rounded down to 64.  The launchers compare every
 * LDS-scene instantiation's real static size with it on first launch (k_bounce's solo instantiation holds exactly this much). */
#define PT_LDS_STATIC_MAX ((size_t)((2048 + PT_SWZ_NODE_BYTES - 1) & ~63)) /* 2112 */

/* ---- where a scene is walked from ---- */
enum {
  PT_PLACE_LDS = 0,        /* the whole tree and every slot in LDS */
  PT_PLACE_HBM_OCT = 1,    /* HBM / L2: scene_host builds the per-octant image (and the top image) */
  PT_PLACE_HBM_SHARED = 2  /* HBM / L2 on the shared 32-byte image + skip table, k_trace + k_shade_pool */
};
enum { PT_LDS_K_TRACE = 0, PT_LDS_K_BOUNCE = 1, PT_LDS_K_BOUNCE_CARRY = 2 };

struct PtLdsIn {
  int mode;                  /* PT_MODE_* */
  int n_nodes, total_slots;  /* total_slots = n_slots + n_floor */
  int has_triangles, has_emit, lds_nodes64;
  int stack_depth;           /* max(1, tree depth + 1) */
  int waves;                 /* waves of the workgroup (pt_lds_placement: of k_trace's) */
  int kernel;                /* PT_LDS_K_* */
  int from_hbm;              /* the launch walks from HBM / L2 */
  int n_top;                 /* k_trace from HBM / L2: nodes of the tree's top held in LDS (0: none) */
};

/* The scene image's regions behind the stacks of `waves_` waves, as ONE list of statements: AT(region, off) is handed every region
 * with its byte offset, in order; the last, `end`, is where the image ends.  pt_lds_image below makes offsets of it for the host;
 * pt_scene_view (kernels.hip) expands the same list into its pointers, so that the compiler is handed the very arithmetic the
 * kernels have always had -- a function's result, inlined, came out as different (no worse, but different) machine code in
 * every kernel with a scene in LDS. */
#define PT_LDS_IMAGE_REGIONS(AT, mode_, waves_, depth_, n_nodes_, total_slots_, has_triangles_, lds_nodes64_)           \
  size_t off = ((size_t)(waves_) * PT_WAVE_STACK_BYTES(true, depth_) + 63) & ~(size_t)63;                                \
  AT(nodes, off);                                                                                                        \
  off += ((size_t)(n_nodes_) * PT_SWZ_NODE_BYTES + 63) & ~(size_t)63; /* (the packets behind it are read 16 bytes at a time) */ \
  const int lds_slots_ = (total_slots_);                                                                                 \
  AT(sph, off);                                                                                                          \
  off += (size_t)lds_slots_ * 4 * sizeof(double);                                                                        \
  AT(tri, off);                                                                                                          \
  if ((mode_) == PT_MODE_ARRAY && (has_triangles_)) off += (size_t)lds_slots_ * 10 * sizeof(double);                     \
  AT(kind, off);                                                                                                         \
  if ((mode_) == PT_MODE_ARRAY) off += ((size_t)lds_slots_ + 15) & ~(size_t)15;                                          \
  AT(cat, off);                                                                                                          \
  off += ((size_t)lds_slots_ + 15) & ~(size_t)15;                                                                        \
  AT(nodes64, off);                                                                                                      \
  if (lds_nodes64_) off += (size_t)(n_nodes_) * 48;                                                                      \
  AT(end, off)
struct PtLdsImage { size_t nodes, sph, tri, kind, cat, nodes64, end; };
PT_LDS_HD PtLdsImage pt_lds_image(int mode, uint32_t waves, int stack_depth, int n_nodes, int total_slots, bool has_triangles, bool lds_nodes64) {
  PtLdsImage m;
#define PT_LDS_AT_OFFSET(region, off_) m.region = (off_)
  PT_LDS_IMAGE_REGIONS(PT_LDS_AT_OFFSET, mode, waves, stack_depth, n_nodes, total_slots, has_triangles, lds_nodes64);
#undef PT_LDS_AT_OFFSET
  return m;
}

/* The one "where does this scene live" decision.  A tree of n_nodes * PT_SWZ_NODE_BYTES >= 65535 bytes is beyond LDS whatever
 * else holds, and gets the per-octant image.  A smaller tree is LDS-resident if its node addresses fit 16 bits (PT_LDS_STATIC_MAX
 * above: 2048 + the largest workgroup's stacks + the nodes < 65534), its slot indices do (< 65536 slots) and stacks + image fit
 * PT_LDS_SCENE_LIMIT at k_trace's workgroup size.  THE GAP between the two: a tree the first test calls small that the address
 * bound, the slot count or the limit sends to HBM / L2 has no per-octant and no top image; it keeps the shared image and the
 * two-kernel schedule (k_trace + k_shade_pool).  That is behaviour, not an oversight to tidy away: scenes would change sides. */
PT_LDS_HD int pt_lds_placement(const PtLdsIn& in) {
  if ((size_t)in.n_nodes * PT_SWZ_NODE_BYTES >= 65535) return PT_PLACE_HBM_OCT;
  if (2048 + (size_t)PT_LDS_MAX_WAVES * PT_WAVE_STACK_BYTES(true, in.stack_depth) + (size_t)in.n_nodes * PT_SWZ_NODE_BYTES >= 65534 ||
      (size_t)in.total_slots >= 65536)
    return PT_PLACE_HBM_SHARED;
  const PtLdsImage m = pt_lds_image(in.mode, (uint32_t)in.waves, in.stack_depth, in.n_nodes, in.total_slots, in.has_triangles != 0, in.lds_nodes64 != 0);
  return m.end <= PT_LDS_SCENE_LIMIT ? PT_PLACE_LDS : PT_PLACE_HBM_SHARED;
}

/* k_bounce's pools and parked walks / k_bounce_carry's parked entries, from pool_off on, as lists of statements like the image's:
 * AT(region, off) places a region at a byte offset, AFTER(region, prev, words) places it `words` 16-byte words behind the start
 * of `prev`; cap_ = PT_PARK_CAP of the workgroup.  (pool_off_ comes first in each sum and unparenthesised: a kernel adds the
 * terms to its buffer from left to right, as it always has.) */
#define PT_LDS_BOUNCE_POOLS(AT, pool_off_, nw_)                                                                          \
  AT(pool_i, pool_off_);                                                                                                  \
  AT(pool_s, pool_off_ + (size_t)(nw_) * PT_N_SHADE_CAT * 128 * sizeof(uint32_t))
#define PT_LDS_BOUNCE_PARK(AT, AFTER, pool_off_, nw_, lds_scene_, uv_, cap_)                                             \
  AT(park0, pool_off_ + (size_t)(nw_) * PT_N_SHADE_CAT * 128 * PT_BOUNCE_POOL_ENTRY_BYTES(lds_scene_));                  \
  AFTER(park_uv, park0, cap_);                                                                                            \
  AFTER(park_w, park_uv, (uv_) ? (cap_) : 0u);                                                                            \
  AFTER(park_end, park_w, (lds_scene_) ? 0u : (cap_))
#define PT_LDS_CARRY_REGIONS(AT, AFTER, pool_off_, emit_, uv_, cap_)                                                     \
  AT(park0, pool_off_);                                                                                                   \
  AFTER(park_emit, park0, 6u * (cap_));                                                                                   \
  AFTER(park_uv, park_emit, (emit_) ? 2u * (cap_) : 0u);                                                                  \
  AFTER(park_end, park_uv, (uv_) ? (cap_) : 0u)
struct PtLdsWork { size_t pool_i, pool_s, park0, park_emit, park_uv, park_w, park_end; };
#define PT_LDS_AT_OFFSET(region, off_) w.region = (off_)
#define PT_LDS_AFTER_OFFSET(region, prev, words_) w.region = w.prev + (size_t)(words_) * 16
PT_LDS_HD PtLdsWork pt_lds_bounce_work(size_t pool_off, int nw, bool lds_scene, bool uv) {
  const uint32_t park_cap = (uint32_t)PT_PARK_CAP(nw, lds_scene ? PT_TAIL_CUT : PT_TAIL_CUT_GLOBAL);
  PtLdsWork w;
  PT_LDS_BOUNCE_POOLS(PT_LDS_AT_OFFSET, pool_off, nw);
  PT_LDS_BOUNCE_PARK(PT_LDS_AT_OFFSET, PT_LDS_AFTER_OFFSET, pool_off, nw, lds_scene, uv, park_cap);
  w.park_emit = w.park_uv; /* (no emission words: k_bounce_carry's) */
  return w;
}
PT_LDS_HD PtLdsWork pt_lds_carry_work(size_t pool_off, int nw, bool emit, bool uv) {
  const uint32_t park_cap = (uint32_t)PT_PARK_CAP(nw, PT_TAIL_CUT);
  PtLdsWork w;
  PT_LDS_CARRY_REGIONS(PT_LDS_AT_OFFSET, PT_LDS_AFTER_OFFSET, pool_off, emit, uv, park_cap);
  w.pool_i = w.pool_s = w.park0; /* (no pools: its parked entries start where they would) */
  w.park_w = w.park_end;
  return w;
}
#undef PT_LDS_AT_OFFSET
#undef PT_LDS_AFTER_OFFSET
/* k_shade_pool: [waves][PT_N_SHADE_CAT][128] x (queue index, hit slot), nothing else */
PT_LDS_HD size_t pt_lds_shade_pool_bytes(int waves) { return (size_t)waves * PT_N_SHADE_CAT * 128 * 8; }

/* The whole buffer of one launch.  pool_off is what the host passes to k_bounce / k_bounce_carry; fits: the launch may be made
 * (k_trace: always -- pt_lds_placement has decided; the k_bounce family: total within PT_LDS_BOUNCE_LIMIT). */
struct PtLdsLayout {
  size_t stacks;  /* always 0: the stacks open the buffer; they end at image.nodes */
  PtLdsImage image;
  size_t top;     /* k_trace from HBM / L2: the tree's top, at 0 */
  size_t pool_off;
  PtLdsWork work;
  size_t total;
  int fits;
};
PT_LDS_HD PtLdsLayout pt_lds_layout(const PtLdsIn& in) {
  PtLdsLayout l;
  l.stacks = l.top = 0;
  if (in.from_hbm) l.image.nodes = l.image.sph = l.image.tri = l.image.kind = l.image.cat = l.image.nodes64 = l.image.end = 0;
  else l.image = pt_lds_image(in.mode, (uint32_t)in.waves, in.stack_depth, in.n_nodes, in.total_slots, in.has_triangles != 0, in.lds_nodes64 != 0);
  l.pool_off = in.from_hbm ? 0 : ((l.image.end + 63) & ~(size_t)63);
  const bool uv = in.mode == PT_MODE_ARRAY;
  if (in.kernel == PT_LDS_K_BOUNCE) l.work = pt_lds_bounce_work(l.pool_off, in.waves, !in.from_hbm, uv);
  else if (in.kernel == PT_LDS_K_BOUNCE_CARRY) l.work = pt_lds_carry_work(l.pool_off, in.waves, in.has_emit != 0, uv);
  else {
    l.pool_off = in.from_hbm ? (size_t)in.n_top * PT_TOP_NODE_BYTES : l.image.end; /* (k_trace: nothing behind the image / the top) */
    l.work.pool_i = l.work.pool_s = l.work.park0 = l.work.park_emit = l.work.park_uv = l.work.park_w = l.work.park_end = l.pool_off;
  }
  l.total = l.work.park_end;
  l.fits = in.kernel == PT_LDS_K_TRACE || l.total <= PT_LDS_BOUNCE_LIMIT;
  return l;
}

/* ---- the per-octant LDS image (PtSceneDev.lds_oct, PT_LOCT_* in pt_scene.h): k_bounce_carry's non-counting launches on Simd_leaf scenes ----
 * The buffer of such a launch: NO per-wave stacks (its walks are threaded and its camera rays walk one per lane: nothing reads a
 * stack), then
 *   records (8 x n_nodes x 32 B, a multiple of 64) | leaf table (one word per node, to 16) | sphere slots (32 B) | shading categories
 *   (to 16) | binary64 bounds (48 B per node, in.lds_nodes64)
 * and, at pool_off = the above to 64, k_bounce_carry's parked entries as in every launch of that kernel. */
#define PT_LDS_OCT_REGIONS(AT, n_nodes_, total_slots_, lds_nodes64_)                                                     \
  size_t off = 0;                                                                                                        \
  AT(oct, off);                                                                                                          \
  off += (size_t)(n_nodes_) * 8 * PT_LOCT_RECORD_BYTES;                                                                  \
  AT(leaf, off);                                                                                                         \
  off += (size_t)PT_LOCT_LEAF_WORDS(n_nodes_) * 4;                                                                       \
  AT(sph, off);                                                                                                          \
  off += (size_t)(total_slots_) * 4 * sizeof(double);                                                                    \
  AT(cat, off);                                                                                                          \
  off += ((size_t)(total_slots_) + 15) & ~(size_t)15;                                                                    \
  AT(nodes64, off);                                                                                                      \
  if (lds_nodes64_) off += (size_t)(n_nodes_) * 48;                                                                      \
  AT(end, off)
struct PtLdsOctLayout {
  size_t oct, leaf, sph, cat, nodes64, end;
  size_t pool_off;
  PtLdsWork work;
  size_t total;
  int fits; /* the scene is admitted: a Simd_leaf tree of 1 .. PT_LOCT_MAX_NODES nodes whose whole buffer is within PT_LDS_BOUNCE_LIMIT */
};
/* in.kernel is taken as PT_LDS_K_BOUNCE_CARRY, in.waves as that launch's; in.stack_depth, in.from_hbm and in.n_top play no part */
PT_LDS_HD PtLdsOctLayout pt_lds_oct_layout(const PtLdsIn& in) {
  PtLdsOctLayout l;
#define PT_LDS_AT_OFFSET(region, off_) l.region = (off_)
  PT_LDS_OCT_REGIONS(PT_LDS_AT_OFFSET, in.n_nodes, in.total_slots, in.lds_nodes64 != 0);
#undef PT_LDS_AT_OFFSET
  l.pool_off = (l.end + 63) & ~(size_t)63;
  l.work = pt_lds_carry_work(l.pool_off, in.waves, in.has_emit != 0, false);
  l.total = l.work.park_end;
  l.fits = in.mode == PT_MODE_SIMD && in.n_nodes >= 1 && in.n_nodes <= PT_LOCT_MAX_NODES && (size_t)in.total_slots < 65536 &&
           l.total <= PT_LDS_BOUNCE_LIMIT;
  return l;
}

/* PtSceneDev.lds_nodes64: the binary64 bounds join the image only if the scene is LDS-resident without them and stays so, in both
 * schedules (k_trace at in.waves, k_bounce at bounce_waves), with them */
PT_LDS_HD int pt_lds_keep_nodes64(PtLdsIn in, int bounce_waves) {
  in.lds_nodes64 = 0;
  if (pt_lds_placement(in) != PT_PLACE_LDS) return 0;
  in.lds_nodes64 = 1;
  if (pt_lds_placement(in) != PT_PLACE_LDS) return 0;
  in.kernel = PT_LDS_K_BOUNCE;
  in.waves = bounce_waves;
  in.from_hbm = 0;
  return pt_lds_layout(in).fits;
}

#endif /* PT_LDS_LAYOUT_H */
