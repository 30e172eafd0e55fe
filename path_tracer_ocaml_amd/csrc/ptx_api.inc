/* ptx_api.inc -- host side of libptx_hip.so: the C ABI declared in include/ptx.h.
 * Included at the end of kernels.hip (one translation unit, so the launches see the templates), in front of probes.inc, which holds
 * the point-probe entry points (ptx_camera_rays, ptx_walk_rays, ptx_trace_samples, ptx_math_eval and their kin). */
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <tuple>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ptx.h"
#include "bvh_build.h"
#include "scene_host.h"

namespace {

thread_local std::string g_last_error;
thread_local int g_last_code = 0; /* the code fail() last returned on this thread (for entry points that return a handle) */

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  g_last_code = code;
  return code;
}

/* (PTX_ERR_ARG / PTX_ERR_HIP / PTX_ERR_STATE: scene_host.h) */
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(PTX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

double wall_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

/* Low_discrepancy_sequence.create (low_discrepancy_sequence.ml:8-31): host-side table, like the
 * reference builds it once per tile with libm's pow */
std::vector<double> lds_alpha(int dimension) {
  const double dp = 1.0 / ((double)dimension + 1.0);
  double x = 2.0;
  for (int it = 0; it < 100000; ++it) {
    const double xp = std::pow(1.0 + x, dp);
    if (x == xp) break;
    x = xp;
  }
  std::vector<double> a((size_t)dimension);
  for (int i = 0; i < dimension; ++i) a[(size_t)i] = 1.0 / std::pow(x, (double)(i + 1));
  return a;
}

/* Filter_kernel.Binomial.create ~order:5 ~pixel_radius:1 (filter_kernel.ml:49-85) evaluated with exact
 * integer rationals: the three resampled taps are 11/3, 26/3, 11/3 */
void binomial_3x3(double out[9]) {
  /* order 5 -> coefficients C(4,k) = 1 4 6 4 1; ratio = 5/3.
   * tap i covers [i*5/3, (i+1)*5/3): partial first/last source cells weighted by their overlap. */
  const int order = 5, width = 3;
  long long num[3];
  const long long coeff[5] = {1, 4, 6, 4, 1};
  for (int i = 0; i < width; ++i) {
    /* work in thirds: source cell k spans [3k, 3k+3), tap i spans [5i, 5i+5) */
    long long acc = 0; /* in thirds */
    for (int k = 0; k < order; ++k) {
      const long long lo = std::max<long long>(3 * k, 5 * i), hi = std::min<long long>(3 * k + 3, 5 * i + 5);
      if (hi > lo) acc += (hi - lo) * coeff[k];
    }
    num[i] = acc; /* weight = acc / 3 */
  }
  double w[3];
  for (int i = 0; i < 3; ++i) w[i] = (double)num[i] / 3.0; /* float_of_num */
  double total = 0.0;
  for (int i = 0; i < 3; ++i) total = total + w[i];
  for (int i = 0; i < 3; ++i) w[i] = w[i] / total;
  for (int j = 0; j < 9; ++j) out[j] = w[j / 3] * w[j % 3]; /* outer_product */
}

/* Filter_kernel.Binomial.create ~order ~pixel_radius (filter_kernel.ml:49-85) restated literally, Num as reduced 64-bit rationals
 * (order <= 16: C(15, k) <= 6435 and 15! < 2^41, the denominators divide 2r + 1 <= 15).  w: the 2r + 1 normalised 1-D weights.
 * binomial_3x3 above is the (5, 1) instance written out by hand; the default film keeps using it. */
struct FilmRat {
  long long n, d; /* d > 0, gcd(n, d) = 1 */
};
long long film_gcd(long long a, long long b) {
  if (a < 0) a = -a;
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a ? a : 1;
}
FilmRat film_rat(long long n, long long d) {
  const long long g = film_gcd(n, d);
  return FilmRat{n / g, d / g};
}
FilmRat film_add(FilmRat a, FilmRat b) { return film_rat(a.n * b.d + b.n * a.d, a.d * b.d); }
FilmRat film_sub(FilmRat a, FilmRat b) { return film_rat(a.n * b.d - b.n * a.d, a.d * b.d); }
FilmRat film_mul(FilmRat a, FilmRat b) { return film_rat(a.n * b.n, a.d * b.d); }
long long film_floor(FilmRat a) { return a.n >= 0 ? a.n / a.d : -((-a.n + a.d - 1) / a.d); }
long long film_ceil(FilmRat a) { return -film_floor(FilmRat{-a.n, a.d}); }
long long film_pow_falling(long long n, long long k) { return k == 0 ? 1 : n * film_pow_falling(n - 1, k - 1); } /* :27 */
long long film_binomial(long long n, long long k) { return film_pow_falling(n, k) / film_pow_falling(k, k); }    /* :28-29 */
void film_weights_1d(int order, int pixel_radius, double* w) {
  const int f_width = 1 + 2 * pixel_radius;
  const FilmRat ratio = film_rat(order, f_width), one = film_rat(1, 1);
  long long coeffs[PTX_FILM_MAX_ORDER];
  for (int k = 0; k < order; ++k) coeffs[k] = film_binomial(order - 1, k);
  for (int i = 0; i < f_width; ++i) {
    const FilmRat ip = film_mul(film_rat(i, 1), ratio); /* i' */
    const FilmRat jp = film_add(ip, ratio);             /* j' */
    const long long beg = film_floor(ip), end_ = film_ceil(jp), len = end_ - beg;
    FilmRat sum = film_rat(0, 1);
    for (long long k = 0; k < len; ++k) {
      FilmRat weight = one;
      if (k == 0) weight = film_sub(one, film_sub(ip, film_rat(film_floor(ip), 1))); /* one -/ fractional_part i' */
      else if (k == len - 1) weight = film_sub(one, film_sub(film_rat(end_, 1), jp));
      sum = film_add(sum, film_mul(weight, film_rat(coeffs[k + beg], 1)));
    }
    w[i] = (double)sum.n / (double)sum.d; /* float_of_num: both are exact in binary64, the quotient rounds to nearest */
  }
  double total = 0.0;
  for (int i = 0; i < f_width; ++i) total = total + w[i]; /* fold_left ( +. ) ~init:0.0, :82 */
  for (int i = 0; i < f_width; ++i) w[i] = w[i] / total;  /* :83 */
}

/* the accepted ptx_film_params (include/ptx.h); the message names the rule that refused */
int film_check(const ptx_film_params* f) {
  if (f->order < 1 || f->order > PTX_FILM_MAX_ORDER) return fail(PTX_ERR_ARG, "film: order %d is outside 1 .. %d", f->order, PTX_FILM_MAX_ORDER);
  if (f->pixel_radius < 0 || f->pixel_radius > PTX_FILM_MAX_RADIUS)
    return fail(PTX_ERR_ARG, "film: pixel_radius %d is outside 0 .. %d", f->pixel_radius, PTX_FILM_MAX_RADIUS);
  if (f->order < 2 * f->pixel_radius + 1)
    return fail(PTX_ERR_ARG, "film: order %d is smaller than 2 * pixel_radius + 1 = %d (the reference's kernel is lopsided there)", f->order,
                2 * f->pixel_radius + 1);
  if (f->flags & ~PTX_FILM_RENORMALISE) return fail(PTX_ERR_ARG, "film: unknown bits in flags (%d): only PTX_FILM_RENORMALISE is defined", f->flags);
  if (f->reserved != 0) return fail(PTX_ERR_ARG, "film: reserved must be 0 (got %d)", f->reserved);
  return 0;
}
constexpr ptx_film_params kFilmDefault = {5, 1, 0, 0};
/* the film the existing kernels apply (k_film, k_film_counts) */
bool film_is_default(const ptx_film_params& f) { return f.order == 5 && f.pixel_radius == 1 && f.flags == 0; }

/* A device allocation that frees itself: a member of ptx_scene (or a local) cannot be forgotten by a hand-kept release list.
 * hipFree needs the owning device current only for the ordering the runtime gives it; ptx_scene_destroy sets it before the
 * handle's members go. */
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p; n = o.n;
      o.p = nullptr; o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t want) {
    if (want <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(want, 1) * sizeof(T));
    if (e == hipSuccess) n = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

/* A buffer of a per-thread workspace that lives until the thread (usually the process) ends: by then the HIP runtime may be
 * gone, so it is released explicitly (ptx_release_workspaces) or handed back to the runtime's own teardown -- never freed
 * from a static destructor. */
template <class T>
struct ThreadLifeBuf : DevBuf<T> {
  ~ThreadLifeBuf() { this->p = nullptr; this->n = 0; }
};

/* Staging for the calls that take host arrays: `count` items into a buffer made large enough, `count` items back out.  Each fails
 * as HIP_TRY does and adds no synchronisation of its own. */
template <class T>
int upload(DevBuf<T>& d, const T* host, size_t count) {
  HIP_TRY(d.ensure(count));
  HIP_TRY(hipMemcpy(d.p, host, sizeof(T) * count, hipMemcpyHostToDevice));
  return 0;
}
template <class T>
int download(T* host, const DevBuf<T>& d, size_t count) {
  HIP_TRY(hipMemcpy(host, d.p, sizeof(T) * count, hipMemcpyDeviceToHost));
  return 0;
}
/* the grid of a launch with one thread per item on 256-thread blocks */
inline dim3 grid256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

struct QueueMem {
  DevBuf<PtRayRec> ray;
  DevBuf<PtPathRec> path; /* emissive scenes: {PtPathRec, PtEmitRec} pairs, one 64-byte line per entry (PtQueue) */
  size_t cap = 0;
  bool with_emit = false;
  hipError_t ensure(size_t c, bool want_emit) {
    hipError_t e;
    with_emit = want_emit;
    if ((e = ray.ensure(c)) != hipSuccess) return e;
    if ((e = path.ensure(want_emit ? 2 * c : c)) != hipSuccess) return e;
    cap = c;
    return hipSuccess;
  }
  PtQueue view(uint32_t* count) const {
    PtQueue q;
    q.ray = ray.p;
    q.path = path.p;
    q.count = count;
    return q;
  }
  void release() { ray.release(); path.release(); cap = 0; }
};

struct TimedLaunch {
  int kind;
  hipEvent_t a, b;
};

}  // namespace

/* Raise a kernel's dynamic-LDS limit towards the CU's 160 KB.  A refusal (static + dynamic beyond the limit) must not linger as
 * the thread's "last error": a later, unrelated hipGetLastError() would report it against the wrong call (seen in round 4, when a
 * kernel gained 320 bytes of static LDS and every later launch check failed with "invalid argument"). */
static void raise_dynamic_lds_limit(const void* kern, int bytes) {
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) (void)hipGetLastError();
}

/* tuning switches read from the environment (documented in DESIGN.md); absent = the default */
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

constexpr int kMaxSets = 4; /* batches in flight (one HIP stream and one workspace set each) */
/* the per-batch control words, zeroed together: counts[b] = live paths entering bounce b (130 words), then per
 * bounce kWorkPerBounce work-distribution words (PtChunkFeed counters, per-category list lengths) */
/* per bounce kWorkPerBounce words: [0..7] trace feed, [16 + 8 c ..] shade feed of category c (5), [56..60] category list lengths */
constexpr size_t kSoloFlagWord = 130; /* (counts[0 .. 127] are the bounces' queue counts) k_bounce's PtSolo.flag */
constexpr size_t kWorkBase = 136, kWorkPerBounce = 64, kCountsWords = kWorkBase + 128 * kWorkPerBounce;
/* block numbers are 20 bits next to a 12-bit cursor (pt_pool_push); 0xfffff = "no block yet" */
constexpr size_t kPoolMaxEntries = (size_t)(PT_POOL_NO_BLOCK - 1) * PT_POOL_BLOCK;

/* How a scene's bounces are launched while `sets_in_flight` batches share the chip: every answer the launch path needs.  Computed in one
 * place (make_schedule) where sets_in_flight, the lighting mode or the uploaded scene changes, and only read in between: by the
 * workspace's sizes, the bounce loop and the four launch functions, which therefore cannot disagree within a render. */
struct Schedule {
  int placement = PT_PLACE_HBM_SHARED; /* where k_trace walks the scene from (pt_lds_placement at k_trace's workgroup size) */
  bool from_hbm = false;       /* the fused kernel runs as k_bounce<..., LDS_SCENE = false> over the per-octant image in HBM / L2 */
  bool share_cus = false;      /* two batches in flight on a Simd_leaf scene held in LDS: every kernel takes half a CU */
  bool lit = false;            /* emitters under lighting mode 1 or 2: the LIT instantiations */
  bool img = false;            /* an image texture or an environment: the IMG instantiations */
  bool lens = false;           /* a thin lens (ptx_scene_set_lens): camera rays are generated into a queue, never a PRIMARY launch; the walk-first order */
  bool pose = false;           /* a camera pose (ptx_scene_set_camera_pose): like a lens, camera rays are generated into a queue (k_generate_tiles) and bounced walk-first */
  bool shutter = false;        /* a camera shutter (ptx_scene_set_camera_shutter): the posed route (pose is set with it), the _SHUTTER kinds of the generators */
  bool latlong = false;        /* the lat-long projection (ptx_scene_set_camera_projection): the posed route (pose is set with it), the PT_CAM_LATLONG kind of the generators */
  bool fused_possible = false; /* a bounce can be one k_bounce launch (PTX_FUSED, the placement, the layout fits) ... */
  bool carry_ok = false;       /* the shade-first order (k_bounce_carry) can be taken */
  bool lane_walk = false;      /* camera launches of k_bounce / k_bounce_carry walk one ray per lane */
  bool lds_oct = false;        /* non-counting k_bounce_carry launches hold the per-octant LDS image (PtSceneDev.lds_oct) and walk it */
  bool tile_lists = false;     /* ... and their camera launch scans the image's camera tile lists where it has them (PTX_TILE_LISTS; tile_lists_for) */
  int top_in_lds = 0;          /* k_trace from HBM / L2 keeps the tree's top in LDS */
  int trace_threads = 0, bounce_threads = 0; /* workgroups of k_trace; of k_bounce and k_bounce_carry */
  size_t trace_lds = 0;        /* dynamic LDS of a k_trace launch */
  PtLdsLayout bounce{}, carry{}; /* dynamic LDS of a k_bounce, of a k_bounce_carry launch */
  PtLdsOctLayout carry_oct{};  /* ... of a k_bounce_carry launch on the per-octant LDS image */
  bool in_lds() const { return placement == PT_PLACE_LDS; }
  bool fused_ok(size_t cap_entries) const { return fused_possible && cap_entries < kPoolMaxEntries; } /* ... with queues of this capacity */
};

/* The camera tile lists of a scene (scene_host.h, scene_tile_lists), one grid per image size, built at the first render of that size and
 * kept: the host copies are shared by a scene and its replicas, every device gets its own upload. */
struct TileListCache {
  std::mutex mu;
  std::vector<std::shared_ptr<const PtTileGrid>> grids;
};
constexpr size_t kMaxTileGrids = 8;
const unsigned long long kZero64 = 0ull;
struct TileListsDev {
  std::shared_ptr<const PtTileGrid> grid;
  DevBuf<uint32_t> buf;
};

struct ptx_scene {
  int device = 0;
  PtSceneDev dev{};
  std::shared_ptr<const PtHostArrays> host; /* scene_host.h; shared by a scene and its replicas; a host-only scene's holds the tree only */
  std::vector<ptx_scene*> replicas;         /* ptx_render with n_gpus > 1: owned, destroyed with the scene */
  std::set<const void*> attr_done;          /* kernels whose dynamic-LDS limit was raised on THIS scene's device */
  int peer_root = -1;                       /* ptx_render_multi: the root device peer access was last set up with ... */
  bool peer_ok = false;                     /* ... and whether both directions were granted */
  DevBuf<double> gather;                    /* multi-GPU root: [rank][pad_rows][W][3] raw sums */
  double* pinned = nullptr;                 /* host staging for the framebuffer's way back (hipHostMalloc) */
  size_t pinned_n = 0;
  hipStream_t copy_stream = nullptr;        /* ptx_render into a pinned image: film + copy of the row slabs */
  hipEvent_t ev_slab[8] = {};
  char* reg_ptr = nullptr;                  /* the caller's framebuffer while it is pinned (ptx_image_pin, ptx_image_pin_bytes) */
  size_t reg_bytes = 0;
  bool holds_pinned(const void* ptr, size_t bytes) const {
    return reg_ptr && (const char*)ptr >= reg_ptr && (const char*)ptr + bytes <= reg_ptr + reg_bytes;
  }
  DevBuf<uint8_t> disp;                     /* the display image of ptx_render_display / ptx_render_progressive_display (display.inc) */
  /* Lighting (ptx_scene_set_lighting): the mode asked for; the light table made of host->emissive_tris when mode 2 is first set
   * (PT_LIGHT_DOUBLES per record) and its device copy, which lives as long as the handle (queued frames keep reading it);
   * the number of calls that are rendering with this handle right now */
  int lighting = 0;
  ptx_film_params film = kFilmDefault;      /* ptx_scene_set_film: what every entry point that films through this handle applies */
  double lens_radius = 0.0, lens_focus = 1.0; /* ptx_scene_set_lens: radius 0 = off, the pinhole */
  /* ptx_scene_set_camera_pose: off = the state of a scene that never called it.  While on: where the camera stands, its rotation
   * (row-major) and, with pose_has_view, its own four view fields */
  bool pose_on = false, pose_has_view = false;
  double pose_origin[3] = {0.0, 0.0, 0.0}, pose_rotation[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  ptx_camera pose_view = {0.0, 0.0, 0.0, 0.0};
  /* ptx_scene_set_camera_shutter: off = the state of a scene that never called it.  While on: how far the camera moves and about
   * which unit axis, by what angle, it turns while the shutter is open */
  bool shutter_on = false;
  double shutter_translation[3] = {0.0, 0.0, 0.0}, shutter_axis[3] = {0.0, 0.0, 0.0}, shutter_angle = 0.0;
  /* ptx_scene_set_camera_projection: PTX_PROJECTION_PERSPECTIVE = the state of a scene that never called it */
  int32_t projection = PTX_PROJECTION_PERSPECTIVE;
  ptx_camera own_view = {0.0, 0.0, 0.0, 0.0}; /* the descriptor's camera (a host-only scene keeps no PtSceneDev scalars) */
  std::vector<double> light_table;
  DevBuf<double> d_lights;
  /* Sphere light sampling (ptx_scene_set_sphere_light_sampling): the flag; the sphere light table made when it is first set
   * (PT_SLIGHT_DOUBLES per record, its running sums continuing the triangles') and the device copy of the JOINED table -- the
   * triangles' records as light_table_build gives them, then the spheres' -- which like d_lights is never freed or rewritten before the
   * handle goes (queued frames keep reading it) */
  bool sphere_sampling = false;
  std::vector<double> sphere_table;
  DevBuf<double> d_joined_lights;
  /* Images (ptx_scene_set_texture_image / _set_environment): per entry of the texture table and for the environment, the host copy of
   * the texel records (shared with the replicas) and this device's upload; the slot categories and shading records with the images in
   * place (scene_image_overrides) and their uploads, which dev.slot_cat / dev.slot_shade point at while any entry carries an image */
  struct ImageHost {
    int32_t width = 0, height = 0, flags = 0;
    std::vector<double> rec; /* 4 doubles per texel */
  };
  struct ImageSlot {
    std::shared_ptr<const ImageHost> host;
    DevBuf<double> dev;
  };
  std::vector<std::unique_ptr<ImageSlot>> images; /* one per texture entry once any was set; host == nullptr: none */
  ImageSlot env;
  double env_rot[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  /* Environment sampling (ptx_scene_set_environment_sampling): the flag; while it is on the density of env.host (shared with the
   * replicas), and env.dev holds its table behind the texels (pt_scene.h, PT_ENVD_*) */
  bool env_sampling = false;
  std::shared_ptr<const PtEnvDensity> env_density;
  DevBuf<uint8_t> slot_cat_img;
  DevBuf<PtShadeRec> slot_shade_img;
  std::atomic<int> busy{0};
  /* owned device memory */
  DevBuf<PtNode> nodes;
  DevBuf<double> sph, tri, tri_uv, tri_frame;
  DevBuf<uint8_t> slot_kind, slot_cat;
  DevBuf<int32_t> slot_material, slot_prim;
  DevBuf<PtMaterial> materials;
  DevBuf<PtTexture> textures;
  DevBuf<PtShadeRec> slot_shade;
  DevBuf<uint16_t> node_skip;
  DevBuf<uint32_t> node_skip32, nodes32, nodes32o, lds_oct, top_nodes, node_skip32_top;
  std::shared_ptr<TileListCache> tile_cache;             /* shared with the replicas, like `host` */
  std::vector<std::unique_ptr<TileListsDev>> tile_dev;   /* this device's uploads: they live as long as the handle (queued frames keep reading them) */
  const TileListsDev* tile_cur = nullptr;                /* the lists of the render in progress, or none (render_raw) */
  const TileListsDev* tile_last = nullptr;               /* ptx_tile_list_stats: the lists the last render scanned, and how many launches did */
  int64_t tile_launches = 0;
  bool tile_fallbacks_zeroed = false;                    /* PtCounters::tile_fallbacks was zeroed once, before the handle's first list launch */
  bool lds_oct_launched = false; /* the render in progress has launched a kernel on the per-octant LDS image (ptx_stats.lds_oct_launches) */
  int n_prims = 0;
  int tree_depth = 0, tree_leaves = 0;
  double build_ms = 0.0;
  /* render workspace, grown on demand and kept */
  /* two independent sets: consecutive batches run on two HIP streams so that one batch's HBM-bound shade
   * overlaps the other's VALU-bound trace */
  struct WorkBufs {
    QueueMem qa, qb;
    DevBuf<double> hit_t, hit_tuv, contrib; /* hit_t: scenes without triangles; hit_tuv: 4 doubles per entry with (PtHits) */
    DevBuf<int32_t> hit_slot;
    DevBuf<uint32_t> counts; /* counts[b] = live paths entering bounce b */
    DevBuf<uint4> susp;       /* k_trace tail cut: 64 parked walk states per wave of the largest grid */
    void release() { qa.release(); qb.release(); hit_t.release(); hit_tuv.release(); contrib.release(); hit_slot.release(); counts.release(); susp.release(); }
  } wb[kMaxSets];
  hipStream_t streams[kMaxSets] = {};
  hipEvent_t ev_fork = nullptr, ev_accum[kMaxSets] = {}, ev_join[kMaxSets] = {};
  /* The sampler's alpha table (L.create, low_discrepancy_sequence.ml:8-31) depends on the dimension only (sampler_dimension).
   * One device copy per distinct dimension, uploaded the first time it is asked for and never written again: frames queued
   * with PTX_RENDER_ASYNC (possibly with different max_bounces, on any stream) keep reading the table they were launched
   * with, and a render call no longer copies anything on the NULL stream. */
  struct AlphaRef { double* p = nullptr; } alpha;      /* the current render's table (a view into alpha_tables) */
  std::vector<std::pair<int, double*>> alpha_tables;   /* (dimension, device copy) */
  DevBuf<double> raw, rgb;
  DevBuf<double> sq, err, err_partials;     /* ptx_render_progressive: square sums, per-pixel error, k_pixel_error partials + rel_err */
  hipEvent_t ev_update = nullptr;           /* ptx_render_progressive: update j filmed (its copy waits for this) */
  /* ptx_render_adaptive: the count map and its copy for round j's callback, the two pixel lists (this round's, the next one's), the
   * select scratch (keep flags, per-workgroup counts and offsets, the next list's length) and the event behind the select */
  DevBuf<int32_t> passes, passes_img, list[2], sel_n;
  DevBuf<uint8_t> sel_keep;
  DevBuf<uint32_t> sel_blocks, sel_offsets;
  hipEvent_t ev_select = nullptr;
  DevBuf<uint32_t> rays_lowest; /* ptx_render_rays_device: k_rays_check's lowest refused index */
  /* ptx_render_features_device: the hit records of one batch of camera rays (slot; t on scenes without triangles), k_trace's
   * hand-out words and parked walks -- its own, because a queued slice of a render may be running on the workspace sets meanwhile;
   * ptx_render_denoised: the feature sums, their means for the host, the filter's guide and {c, V} pair, the denoised sums */
  DevBuf<int32_t> feat_slot;
  DevBuf<PtRayRec> feat_ray; /* a lens's feature slices: the camera rays k_trace walks (k_generate_tiles<CAM, false>) */
  DevBuf<double> feat_t;
  DevBuf<uint32_t> feat_work;
  DevBuf<uint4> feat_susp;
  DevBuf<double> feat, feat_mean, den_raw, den_guide, den_cv[2];
  /* ptx_render_temporal: the two history buffers (hist[hist_cur] holds the last frame's records while hist_valid), the size and
   * camera of the frame that wrote them, the accumulated sums, the motion and the history count */
  DevBuf<double> hist[2], temporal_raw, temporal_motion;
  DevBuf<unsigned long long> temporal_count;
  int hist_cur = 0, hist_w = 0, hist_h = 0;
  bool hist_valid = false;
  ptx_temporal_camera hist_camera{};
  DevBuf<PtCounters> counters;
  std::vector<TimedLaunch> timed;
  std::vector<hipEvent_t> event_pool;
  size_t event_next = 0;
  int n_cu = 256;
  bool built_on_gpu = false;
  int grid_div = 1; /* 2 while two batches run concurrently on two streams */
  /* LDS-resident scenes: queued rays of bounces 1 .. bounce_packet also walk the tree as wave packets (0 = camera rays only) */
  int bounce_packet = env_int("PTX_BOUNCE_PACKET", 0);
  int sets_in_flight = 1;                            /* batches sharing the chip during the current render ... */
  Schedule sched;                                    /* ... and how its bounces are launched: written together, by reschedule() */
  /* the last render_raw ran its batch(es) on the caller's stream with workspace set 0 (one set): the lanes of the next one must not
   * start before that stream (slices of different lengths, ptx_render_passes_device, can alternate between one set and two) */
  bool single_set_last = false;
  int trace_block = env_int("PTX_TRACE_BLOCK", 0); /* 0 = by schedule (make_schedule) */
  int fused = env_int("PTX_FUSED", 2);             /* LDS-resident scenes: one kernel per bounce (k_bounce: walk + shade in the same wave) -- 2: every bounce, 1: all but the camera rays', 0: k_trace + k_shade_pool */
  int bounce_fence_wg = env_int("PTX_BOUNCE_FENCE_WG", 0); /* k_bounce: 1 = workgroup-scope fences around a wave's own records (the safety net; tests run both) */
  int solo_entries = env_int("PTX_SOLO_ENTRIES", 0); /* k_bounce: a launch whose input queue holds at most this many entries runs the batch's remaining bounces by itself (0 = off) */
  int fused_global = env_int("PTX_FUSED_GLOBAL", 1); /* scenes walked from HBM / L2: 1 = k_bounce<..., LDS_SCENE = false> instead of k_trace + k_shade_pool */
  int bounce_order = env_int("PTX_BOUNCE_ORDER", 2); /* LDS-resident scenes, PTX_FUSED=2: 1 = a bounce launch shades its input's carried hits first and walks the new rays second (k_bounce_carry), 0 = walk first (k_bounce), 2 = by scene (Schedule::carry_ok) */
  int primary_walk = env_int("PTX_PRIMARY_WALK", 2); /* LDS-resident scenes, the camera launch of k_bounce / k_bounce_carry: 0 = the tile walks as a wave packet (pt_trace_packet), 1 = one ray per lane (pt_trace_ray), 2 = by scene (Schedule::lane_walk) */
  int bounce_threads = env_int("PTX_BOUNCE_THREADS", 0); /* k_bounce workgroup size (0 = PT_BOUNCE_THREADS; tests: 64 .. 1024) */
  int bounce_wgs = env_int("PTX_BOUNCE_WGS", 0);         /* k_bounce workgroups per launch (0 = one per CU; tests: a few, so that every wave walks hundreds of chunks) */
  int trace_top = env_int("PTX_TRACE_TOP", 0);     /* scenes walked from HBM / L2: 1 = keep the tree's top in LDS (measured: no gain, the top of the tree is hot in L1 anyway; DESIGN.md section 4) */
  int trace_wgs_per_cu = env_int("PTX_TRACE_WGS", 0); /* 0 = as many as fit */
  int shade_wgs_per_cu = env_int("PTX_SHADE_WGS", 0); /* k_shade_pool workgroups per CU; 0 = what the registers admit */
};

namespace {

hipEvent_t scene_event(ptx_scene* s) {
  if (s->event_next == s->event_pool.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    s->event_pool.push_back(e);
  }
  return s->event_pool[s->event_next++];
}

/* Held by every call that shades with a handle, for as long as it does: ptx_scene_set_lighting refuses meanwhile (a progress or
 * update callback that tries gets PTX_ERR_STATE).  Calls nest (ptx_render_progressive around its slices). */
struct RenderBusy {
  ptx_scene* s;
  explicit RenderBusy(ptx_scene* s_) : s(s_) { s->busy.fetch_add(1); }
  ~RenderBusy() { s->busy.fetch_sub(1); }
  RenderBusy(const RenderBusy&) = delete;
  RenderBusy& operator=(const RenderBusy&) = delete;
};

struct LaunchTimer {
  ptx_scene* s;
  hipStream_t st;
  bool on;
  TimedLaunch t{};
  LaunchTimer(ptx_scene* s_, hipStream_t st_, bool on_, int kind) : s(s_), st(st_), on(on_) {
    if (on) {
      t.kind = kind;
      t.a = scene_event(s);
      t.b = scene_event(s);
      (void)hipEventRecord(t.a, st);
    }
  }
  ~LaunchTimer() {
    if (on) {
      (void)hipEventRecord(t.b, st);
      s->timed.push_back(t);
    }
  }
};

int local_rows(const ptx_render_params* p) {
  if (p->band_step <= 1) return p->height;
  const int br = p->band_rows > 0 ? p->band_rows : 32;
  const int n_bands = (p->height + br - 1) / br;
  int rows = 0;
  for (int b = p->band_first; b < n_bands; b += p->band_step) rows += std::min(br, p->height - b * br);
  return rows;
}

int global_row(const ptx_render_params* p, int local_row) {
  if (local_row < 0 || local_row >= local_rows(p)) return -1;
  if (p->band_step <= 1) return local_row;
  const int br = p->band_rows > 0 ? p->band_rows : 32;
  const int band_local = local_row / br;
  return (p->band_first + band_local * p->band_step) * br + (local_row - band_local * br);
}

int check_params(const ptx_render_params* p) {
  if (!p) return fail(PTX_ERR_ARG, "params is NULL");
  if (p->width <= 0 || p->height <= 0) return fail(PTX_ERR_ARG, "image dimensions must be positive (got %d x %d)", p->width, p->height);
  if (p->samples_per_pixel <= 0) return fail(PTX_ERR_ARG, "samples_per_pixel must be >= 1 (got %d)", p->samples_per_pixel);
  if (p->max_bounces < 0 || p->max_bounces > 126) return fail(PTX_ERR_ARG, "max_bounces must be in [0, 126] (got %d)", p->max_bounces);
  if (p->band_step > 1 && (p->band_first < 0 || p->band_first >= p->band_step)) return fail(PTX_ERR_ARG, "band_first %d out of range for band_step %d", p->band_first, p->band_step);
  /* sampler offset = gy*W + gx + pass*spp must fit an int32 (OCaml ints are 63-bit; we carry i32) */
  const long long max_off = (long long)(p->height - 1) * p->width + (p->width - 1) + (long long)(p->samples_per_pixel - 1) * p->samples_per_pixel;
  if (max_off >= 2147483647LL) return fail(PTX_ERR_ARG, "sampler offset %lld does not fit 32 bits", max_off);
  if (p->flags & ~PTX_RENDER_ASYNC) return fail(PTX_ERR_ARG, "unknown bits in flags (0x%x): the field replaced `reserved` and must be initialised", (unsigned)p->flags);
  return 0;
}

/* grid for the persistent-style (strided) kernels */
int strided_grid(const ptx_scene* s, size_t n, int block, int blocks_per_cu) {
  const size_t need = (n + (size_t)block - 1) / (size_t)block;
  const size_t cap = std::max<size_t>(1, (size_t)s->n_cu * (size_t)blocks_per_cu / (size_t)s->grid_div);
  return (int)std::max<size_t>(1, std::min(need, cap));
}

constexpr int kTraceBlockGlobal = PT_TRACE_BLOCK_GLOBAL; /* traversal data in HBM/L2: u32 stacks */
static_assert(PT_TRACE_BLOCK_LDS <= 64 * PT_LDS_MAX_WAVES && PT_BOUNCE_THREADS <= 64 * PT_LDS_MAX_WAVES, "pt_lds_layout.h bounds node addresses for workgroups of PT_LDS_MAX_WAVES waves");

/* Once per instantiation: a kernel's real static LDS must leave the room the layout counts on -- `reserve` bytes beside the largest
 * dynamic request, and on an LDS scene no more than PT_LDS_STATIC_MAX in front of the image (the 16-bit node addresses) */
void check_static_lds(const void* kern, const char* name, bool lds_scene, size_t reserve) {
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, kern) != hipSuccess) return;
  if ((size_t)fa.sharedSizeBytes > reserve || (lds_scene && (size_t)fa.sharedSizeBytes > PT_LDS_STATIC_MAX)) {
    fprintf(stderr, "ptx: %s holds %zu bytes of static LDS, more than pt_lds_layout.h leaves room for (%zu%s)\n", name, (size_t)fa.sharedSizeBytes, reserve,
            lds_scene ? ", PT_LDS_STATIC_MAX in front of the scene image" : "");
    abort(); /* a build error (a new __shared__ array), caught on the first launch of any test */
  }
}
/* A kernel's first launch on this scene's device: its dynamic-LDS limit goes up to the family's `dynamic_limit` (the rest of the
 * CU's 160 KB is the kernels' static words: chunk counters, bins, the floor triangles) and its static LDS is checked against the
 * family's `reserve`.  The limit is a property of (kernel, device): remembered per scene, which is bound to one device */
void prepare_kernel(ptx_scene* s, const void* kern, const char* name, bool lds_scene, size_t dynamic_limit, size_t reserve) {
  if (!s->attr_done.insert(kern).second) return;
  raise_dynamic_lds_limit(kern, (int)dynamic_limit);
  check_static_lds(kern, name, lds_scene, reserve);
}

/* what pt_lds_layout.h needs to know of a launch of `kernel` (PT_LDS_K_*) with workgroups of `waves` waves */
PtLdsIn lds_in(const ptx_scene* s, int kernel, int waves, bool from_hbm = false, int n_top = 0) {
  PtLdsIn in{};
  in.mode = s->dev.mode;
  in.n_nodes = s->dev.n_nodes;
  in.total_slots = s->dev.n_slots + s->dev.n_floor;
  in.has_triangles = s->dev.has_triangles;
  in.has_emit = s->dev.has_emit;
  in.lds_nodes64 = s->dev.lds_nodes64;
  in.stack_depth = std::max(1, s->tree_depth + 1);
  in.waves = waves;
  in.kernel = kernel;
  in.from_hbm = from_hbm;
  in.n_top = n_top;
  return in;
}

/* The one place that decides how a scene's bounces are launched while `sets` batches share the chip: every answer is a function of
 * the scene (s->dev, the tree's depth), its PTX_* knobs and `sets`, and holds still for as long as none of them changes.  reschedule()
 * below is the only writer of ptx_scene::sets_in_flight and ptx_scene::sched. */
Schedule make_schedule(const ptx_scene* s, int sets) {
  Schedule c;
  const bool simd = s->dev.mode == PT_MODE_SIMD;
  /* k_trace with the traversal data copied to LDS once per workgroup (u16 stacks): workgroup size by leaf kind */
  /* Simd_leaf scenes: 1024-thread workgroups when one batch runs alone (one LDS scene copy and one chunk counter per 16
   * waves: trace 22.4 ms against 24.4 ms with 512), 512-thread workgroups when two batches share the chip on two streams (the
   * dispatcher interleaves them with the other batch's shade workgroups at a finer grain: frame 37.3 ms against 38.6 ms).
   * The kernel is compiled for up to PT_TRACE_BLOCK_LDS threads and sizes everything from blockDim. */
  int trace_block_lds = PT_TRACE_BLOCK_LDS_ARRAY;
  if (simd) {
    const int b = s->trace_block > 0 ? s->trace_block : (sets >= 2 ? 512 : PT_TRACE_BLOCK_LDS);
    trace_block_lds = std::min(PT_TRACE_BLOCK_LDS, std::max(64, b & ~63));
  }
  /* the traversal data fits an LDS copy (else: traverse from HBM/L2).  8 or 16 waves of stacks can decide it: a one-set and a two-set
   * render of the same scene may be placed differently */
  c.placement = pt_lds_placement(lds_in(s, PT_LDS_K_TRACE, trace_block_lds / 64));
  const bool in_lds = c.in_lds();
  /* Two batches in flight on a Simd_leaf scene held in LDS: every kernel takes half of what a CU holds (launch_shade_pool).
   * Measured: headline frame 29.7 -> 27.4 ms, 4K spp 256 468 -> 429 ms.  Array_leaf scenes (cornell: the trace kernel needs
   * ~106 VGPRs, one workgroup would be left) and scenes walked from HBM / L2 lose 1-2 % and keep whole-CU grids. */
  c.share_cus = sets >= 2 && simd && in_lds;
  /* An emissive scene in lighting mode 1 or 2 (PtSceneDev.lighting holds the mode in effect: mode 1 without emitters is mode 0): the
   * instantiations flagged LIT.  Such a scene takes the walk-first kernel and never runs solo. */
  c.lit = s->dev.lighting != 0 && s->dev.has_emit != 0;
  /* A scene with an image on a texture entry or an environment (ptx_scene_set_texture_image / _set_environment): the instantiations
   * flagged IMG, which only the walk-first k_bounce, k_shade_pool, the feature kernel and the photon passes have.  Like a lit scene
   * it never takes the shade-first order -- hence no per-octant LDS image and no tile lists either -- and never runs solo. */
  c.img = s->dev.n_images != 0 || s->dev.env != nullptr;
  /* A scene with a lens: its camera rays have an origin, which no fused camera launch can take, so they are written into a queue
   * (k_generate_tiles) and bounced like a list's.  The shade-first order starts at a camera launch: a lens scene keeps the walk-first
   * order, and with it has no per-octant LDS image and no tile lists. */
  c.lens = s->lens_radius > 0.0;
  /* A posed camera (ptx_scene_set_camera_pose), the identity pose included: its rays start at the pose's origin, so they take the
   * lens's route -- a queue (k_generate_tiles) and the walk-first order; no per-octant LDS image, no tile lists (both are made for
   * rays from the origin of the scene's own space), no solo run. */
  /* The lat-long projection: rays in every direction from the pose's origin (origin 0 and the identity while the pose is off) -- the
   * posed route with a camera kind of its own (camera_rays.inc), and everything a posed scene gives up. */
  c.latlong = s->projection == PTX_PROJECTION_LATLONG;
  /* A camera shutter: the posed route too (origin 0 and the identity while the pose is off), with camera kinds of its own. */
  c.shutter = s->shutter_on;
  c.pose = s->pose_on || c.latlong || c.shutter;
  /* scenes walked from HBM / L2: the top of the tree goes to LDS (PtSceneDev.top_nodes), PTX_TRACE_TOP=0 switches it off */
  c.top_in_lds = (!in_lds && s->dev.n_top > 0 && s->trace_top) ? 1 : 0;
  c.trace_threads = in_lds ? trace_block_lds : kTraceBlockGlobal;
  c.trace_lds = pt_lds_layout(lds_in(s, PT_LDS_K_TRACE, c.trace_threads / 64, !in_lds, c.top_in_lds ? s->dev.n_top : 0)).total;
  /* k_bounce: a bounce of an LDS-resident scene as ONE launch (walk + pooled shade in the same wave), counting renders
   * included (its COUNT instantiations); the scenes walked from HBM / L2 keep the two kernels */
  /* scenes walked from HBM / L2 run k_bounce<..., LDS_SCENE = false> over the per-octant node image (PTX_FUSED_GLOBAL=0: k_trace + k_shade_pool) */
  c.from_hbm = !in_lds && s->dev.nodes32o != nullptr && s->fused_global != 0 && !(s->dev.n_top > 0 && s->trace_top);
  /* (the IMG instantiations are compiled for 3 waves per SIMD: at most PT_BOUNCE_THREADS_IMG threads a workgroup) */
  const int bounce_max = c.img ? PT_BOUNCE_THREADS_IMG : PT_BOUNCE_THREADS;
  c.bounce_threads = s->bounce_threads > 0 ? std::min(bounce_max, std::max(64, s->bounce_threads & ~63))
                                           : std::min(bounce_max, c.from_hbm ? PT_BOUNCE_THREADS_GLOBAL : PT_BOUNCE_THREADS);
  /* the dynamic LDS of a k_bounce and of a k_bounce_carry launch: total, pool_off and whether it fits (PT_LDS_BOUNCE_LIMIT) */
  c.bounce = pt_lds_layout(lds_in(s, PT_LDS_K_BOUNCE, c.bounce_threads / 64, c.from_hbm));
  c.carry = pt_lds_layout(lds_in(s, PT_LDS_K_BOUNCE_CARRY, c.bounce_threads / 64, c.from_hbm));
  c.fused_possible = s->fused && (in_lds || c.from_hbm) && c.bounce.fits;
  /* the shade-first order (k_bounce_carry) is for LDS-resident scenes whose larger parked record still fits, with every bounce a
   * k_bounce launch and no solo run configured.  By default (PTX_BOUNCE_ORDER=2) the scenes binned by elevation take it -- open
   * scenes, where two paths in five leave per bounce and end where their walk ends (Shirley: frame -8 %) -- and the others keep the
   * walk-first order: a closed box has no misses to save, loses its octant key and carries its emission through the walk (cornell:
   * +4.8 %; DESIGN.md Appendix A).  1 = wherever possible, 0 = nowhere (the A/B, the tests) */
  c.carry_ok = (s->bounce_order == 1 || (s->bounce_order >= 2 && s->dev.sort_by_elevation)) && !c.lit && !c.img && !c.lens && !c.pose && s->fused >= 2 && s->solo_entries <= 0 &&
               in_lds && !c.from_hbm && c.carry.fits;
  /* how the camera rays of an LDS-resident scene walk the tree in k_bounce / k_bounce_carry.  By default (PTX_PRIMARY_WALK=2) the
   * Simd_leaf scenes walk one ray per lane -- not counting, that is the assembly node loop of the queued rays -- and the Array_leaf
   * scenes, which have no such loop, keep the wave packet (DESIGN.md Appendix A).  1 = per lane everywhere, 0 = the packet everywhere */
  c.lane_walk = s->primary_walk == 1 || (s->primary_walk >= 2 && simd);
  /* the per-octant LDS image (PTX_LDS_OCT, read at scene creation: scene_host.cpp builds it or not): wherever the shade-first order
   * runs with the camera rays one per lane and the whole buffer of such a launch fits with it.  Counting launches keep the shared image */
  c.carry_oct = pt_lds_oct_layout(lds_in(s, PT_LDS_K_BOUNCE_CARRY, c.bounce_threads / 64));
  c.lds_oct = s->dev.lds_oct != nullptr && simd && c.carry_ok && c.lane_walk && c.carry_oct.fits;
  /* camera tile lists (PTX_TILE_LISTS, read at scene creation like PTX_LDS_OCT): wherever the camera launch runs on the per-octant LDS image
   * and the scene can have lists at all (Simd_leaf spheres, no floor) */
  c.tile_lists = c.lds_oct && s->host && s->host->tile_lists != 0 && scene_tile_lists_possible(*s->host);
  return c;
}
void reschedule(ptx_scene* s, int sets) {
  s->sets_in_flight = sets;
  s->sched = make_schedule(s, sets);
}

struct PrimaryLaunch {
  bool on = false;
  PtGenParams g{};
  uint32_t n = 0;
};

/* ---- one selector per kernel family: the runtime facts of a launch -> the instantiation, as a pointer of the family's one function
 * type.  Each instantiation is named exactly once, in its selector, so the text below IS the set the library is built with; a name
 * more is a kernel more (minutes of build, megabytes of code object).  The order of the names is the order of the kernels in the code
 * object (a kernel is emitted where it is first named; profiles/pr_launch_schedule_identity.txt): moving one moves code, nothing else. ---- */
using TraceKernel = decltype(&k_trace<PT_MODE_SIMD, false, false, false, false>);
using ShadePoolKernel = decltype(&k_shade_pool<false, false>);
using CarryKernel = decltype(&k_bounce_carry<PT_MODE_SIMD, false, false, false>);
using BounceKernel = decltype(&k_bounce<PT_MODE_SIMD, false, false, false>);
enum class Shading { none, emit, lit };          /* no emitters; emitters summed as the reference does; emitters under lighting mode 1 or 2 (LIT implies EMIT) */
enum class Variant { plain, solo, lane_walk };   /* k_bounce: with the loop over a batch's remaining bounces (PtSolo); camera rays one per lane */

/* k_trace: 32 = MODE 2 x COUNT 2 x PRIMARY 2 x LDS_SCENE 2 x PACKET 2, the whole cube.  PACKET is the wave-packet walk on an LDS scene
 * and the per-octant node image on a walk from HBM / L2, so both values occur on both sides. */
template <int MODE, bool COUNT>
TraceKernel trace_kernel_of(bool primary, bool lds_scene, bool packet) {
  if (primary && lds_scene) return packet ? k_trace<MODE, COUNT, true, true, true> : k_trace<MODE, COUNT, true, true, false>;
  if (primary) return packet ? k_trace<MODE, COUNT, true, false, true> : k_trace<MODE, COUNT, true, false, false>;
  if (lds_scene) return packet ? k_trace<MODE, COUNT, false, true, true> : k_trace<MODE, COUNT, false, true, false>;
  return packet ? k_trace<MODE, COUNT, false, false, true> : k_trace<MODE, COUNT, false, false, false>;
}
TraceKernel trace_kernel(int mode, bool count, bool primary, bool lds_scene, bool packet) {
  if (mode == PT_MODE_SIMD) return count ? trace_kernel_of<PT_MODE_SIMD, true>(primary, lds_scene, packet) : trace_kernel_of<PT_MODE_SIMD, false>(primary, lds_scene, packet);
  return count ? trace_kernel_of<PT_MODE_ARRAY, true>(primary, lds_scene, packet) : trace_kernel_of<PT_MODE_ARRAY, false>(primary, lds_scene, packet);
}

/* k_shade_pool: 12 = (EMIT, LIT) in {00, 10, 11} x PRIMARY 2 x IMG 2 */
ShadePoolKernel shade_pool_kernel(Shading shading, bool primary, bool img) {
  if (img) {
    if (shading == Shading::lit) return primary ? k_shade_pool<true, true, true, true> : k_shade_pool<true, false, true, true>;
    if (shading == Shading::emit) return primary ? k_shade_pool<true, true, false, true> : k_shade_pool<true, false, false, true>;
    return primary ? k_shade_pool<false, true, false, true> : k_shade_pool<false, false, false, true>;
  }
  if (shading == Shading::lit) return primary ? k_shade_pool<true, true, true> : k_shade_pool<true, false, true>;
  if (shading == Shading::emit) return primary ? k_shade_pool<true, true> : k_shade_pool<true, false>;
  return primary ? k_shade_pool<false, true> : k_shade_pool<false, false>;
}

/* k_bounce_carry: 24 = MODE 2 x COUNT 2 x EMIT 2 x (PRIMARY, LANE_WALK) in {00, 10, 11}: only camera rays walk one per lane (a
 * lane walk asked of a queued launch is the plain kernel), and a lit scene never takes this kernel (Schedule::carry_ok);
 * + 6 on the per-octant LDS image (LOCT; Simd_leaf, not counting): EMIT 2 x {queued, camera with lane walk, camera with lane walk
 * over tile lists} */
CarryKernel carry_kernel_oct(bool emit, bool primary, bool tile) {
  if (primary && tile) return emit ? k_bounce_carry<PT_MODE_SIMD, false, true, true, true, true, true> : k_bounce_carry<PT_MODE_SIMD, false, false, true, true, true, true>;
  if (emit) return primary ? k_bounce_carry<PT_MODE_SIMD, false, true, true, true, true> : k_bounce_carry<PT_MODE_SIMD, false, true, false, false, true>;
  return primary ? k_bounce_carry<PT_MODE_SIMD, false, false, true, true, true> : k_bounce_carry<PT_MODE_SIMD, false, false, false, false, true>;
}
template <int MODE, bool COUNT>
CarryKernel carry_kernel_of(bool emit, bool primary, bool lane_walk) {
  if (emit) {
    if (primary) return lane_walk ? k_bounce_carry<MODE, COUNT, true, true, true> : k_bounce_carry<MODE, COUNT, true, true>;
    return k_bounce_carry<MODE, COUNT, true, false>;
  }
  if (primary) return lane_walk ? k_bounce_carry<MODE, COUNT, false, true, true> : k_bounce_carry<MODE, COUNT, false, true>;
  return k_bounce_carry<MODE, COUNT, false, false>;
}
CarryKernel carry_kernel(int mode, bool count, bool emit, bool primary, bool lane_walk) {
  if (mode == PT_MODE_SIMD) return count ? carry_kernel_of<PT_MODE_SIMD, true>(emit, primary, lane_walk) : carry_kernel_of<PT_MODE_SIMD, false>(emit, primary, lane_walk);
  return count ? carry_kernel_of<PT_MODE_ARRAY, true>(emit, primary, lane_walk) : carry_kernel_of<PT_MODE_ARRAY, false>(emit, primary, lane_walk);
}

/* k_bounce: 76 = MODE 2 x COUNT 2 x 19, the 19 being 7 + 7 + 5 by shading.
 *   none, emit: 7 = a camera launch {plain, lane walk} on an LDS scene and {plain} from HBM / L2, a queued launch {plain, solo} x {LDS, HBM}
 *   lit:        5 = the same without the two solo kernels (a lit scene never runs solo)
 * A variant the family does not have is the plain kernel: a lane walk off a camera launch or off LDS, solo on a camera launch or a
 * lit scene.  Template arguments: <MODE, COUNT, EMIT, PRIMARY, LDS_SCENE, SOLO_T, LIT, LANE_WALK>.  (With emitters the lit kernels stand
 * beside the unlit plain ones, row by row, and the unlit variants behind them: the order these kernels have always been emitted in.) */
template <int MODE, bool COUNT>
BounceKernel bounce_kernel_of(Shading shading, bool primary, bool lds_scene, Variant variant) {
  const bool lit = shading == Shading::lit;
  const bool lane_walk = variant == Variant::lane_walk && primary && lds_scene, solo = variant == Variant::solo && !primary && !lit;
  if (shading != Shading::none) {
    if (lit || !(lane_walk || solo)) { /* what a lit scene can get, beside the unlit plain kernel of the same launch */
      if (primary && !lds_scene) return !lit ? k_bounce<MODE, COUNT, true, true, false> : k_bounce<MODE, COUNT, true, true, false, false, true>;
      if (primary && !lane_walk) return !lit ? k_bounce<MODE, COUNT, true, true, true> : k_bounce<MODE, COUNT, true, true, true, false, true>;
      if (primary) return k_bounce<MODE, COUNT, true, true, true, false, true, true>;
      if (!lds_scene) return !lit ? k_bounce<MODE, COUNT, true, false, false> : k_bounce<MODE, COUNT, true, false, false, false, true>;
      return !lit ? k_bounce<MODE, COUNT, true, false, true> : k_bounce<MODE, COUNT, true, false, true, false, true>;
    }
    if (lane_walk) return k_bounce<MODE, COUNT, true, true, true, false, false, true>;
    return !lds_scene ? k_bounce<MODE, COUNT, true, false, false, true> : k_bounce<MODE, COUNT, true, false, true, true>;
  }
  if (primary && !lds_scene) return k_bounce<MODE, COUNT, false, true, false>;
  if (primary) return !lane_walk ? k_bounce<MODE, COUNT, false, true, true> : k_bounce<MODE, COUNT, false, true, true, false, false, true>;
  if (!lds_scene) return solo ? k_bounce<MODE, COUNT, false, false, false, true> : k_bounce<MODE, COUNT, false, false, false>;
  return solo ? k_bounce<MODE, COUNT, false, false, true, true> : k_bounce<MODE, COUNT, false, false, true>;
}
/* + 60 with an image texture or an environment (IMG) = MODE 2 x COUNT 2 x shading 3 x 5, the lit scene's five: such a scene never runs solo */
template <int MODE, bool COUNT, bool EMIT, bool LIT>
BounceKernel bounce_kernel_img_of(bool primary, bool lds_scene, bool lane_walk) {
  if (primary && !lds_scene) return k_bounce<MODE, COUNT, EMIT, true, false, false, LIT, false, true>;
  if (primary) return lane_walk ? k_bounce<MODE, COUNT, EMIT, true, true, false, LIT, true, true> : k_bounce<MODE, COUNT, EMIT, true, true, false, LIT, false, true>;
  return lds_scene ? k_bounce<MODE, COUNT, EMIT, false, true, false, LIT, false, true> : k_bounce<MODE, COUNT, EMIT, false, false, false, LIT, false, true>;
}
template <int MODE, bool COUNT>
BounceKernel bounce_kernel_img(Shading shading, bool primary, bool lds_scene, Variant variant) {
  const bool lane_walk = variant == Variant::lane_walk && primary && lds_scene;
  if (shading == Shading::lit) return bounce_kernel_img_of<MODE, COUNT, true, true>(primary, lds_scene, lane_walk);
  if (shading == Shading::emit) return bounce_kernel_img_of<MODE, COUNT, true, false>(primary, lds_scene, lane_walk);
  return bounce_kernel_img_of<MODE, COUNT, false, false>(primary, lds_scene, lane_walk);
}
BounceKernel bounce_kernel(int mode, bool count, Shading shading, bool primary, bool lds_scene, Variant variant, bool img) {
  if (img) {
    if (mode == PT_MODE_SIMD) return count ? bounce_kernel_img<PT_MODE_SIMD, true>(shading, primary, lds_scene, variant) : bounce_kernel_img<PT_MODE_SIMD, false>(shading, primary, lds_scene, variant);
    return count ? bounce_kernel_img<PT_MODE_ARRAY, true>(shading, primary, lds_scene, variant) : bounce_kernel_img<PT_MODE_ARRAY, false>(shading, primary, lds_scene, variant);
  }
  if (mode == PT_MODE_SIMD) return count ? bounce_kernel_of<PT_MODE_SIMD, true>(shading, primary, lds_scene, variant) : bounce_kernel_of<PT_MODE_SIMD, false>(shading, primary, lds_scene, variant);
  return count ? bounce_kernel_of<PT_MODE_ARRAY, true>(shading, primary, lds_scene, variant) : bounce_kernel_of<PT_MODE_ARRAY, false>(shading, primary, lds_scene, variant);
}
Shading scene_shading(const ptx_scene* s) { return s->sched.lit ? Shading::lit : (s->dev.has_emit ? Shading::emit : Shading::none); }

/* ---- the kernel table (ptx_kernel_table): every selector above walked over the whole cube of its arguments, in the fixed order below;
 * a pointer is entered the first time a selector returns it, under the name of the arguments that did.  Host code only: the selectors
 * are pure and the pointers are the host stubs that hipLaunchKernelGGL takes, which is what ptx_scene::attr_done holds. ---- */
struct KernelEntry {
  const void* kern;
  std::string name;
};
const std::vector<KernelEntry>& kernel_table() {
  static const std::vector<KernelEntry> table = [] {
    std::vector<KernelEntry> t;
    std::set<const void*> seen;
    const auto add = [&](const void* k, std::string name) {
      if (seen.insert(k).second) t.push_back(KernelEntry{k, std::move(name)});
    };
    const int modes[2] = {PT_MODE_SIMD, PT_MODE_ARRAY};
    const char* const mode_n[2] = {"simd", "array"};
    const char* const count_n[2] = {"nocount", "count"};
    const char* const shading_n[3] = {"none", "emit", "lit"};
    const char* const primary_n[2] = {"queued", "camera"};
    const char* const lds_n[2] = {"hbm", "lds"};
    const char* const variant_n[3] = {"plain", "solo", "lanewalk"};
    const char* const img_n[2] = {"noimg", "img"};
    const auto join = [](std::initializer_list<const char*> parts) {
      std::string s;
      for (const char* p : parts) {
        if (!s.empty()) s += '/';
        s += p;
      }
      return s;
    };
    for (int m = 0; m < 2; ++m)
      for (int c = 0; c < 2; ++c)
        for (int p = 0; p < 2; ++p)
          for (int l = 0; l < 2; ++l)
            for (int k = 0; k < 2; ++k)
              add((const void*)trace_kernel(modes[m], c != 0, p != 0, l != 0, k != 0),
                  join({"k_trace", mode_n[m], count_n[c], primary_n[p], lds_n[l], k ? "packet" : "nopacket"}));
    for (int sh = 0; sh < 3; ++sh)
      for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 2; ++i)
          add((const void*)shade_pool_kernel((Shading)sh, p != 0, i != 0), join({"k_shade_pool", shading_n[sh], primary_n[p], img_n[i]}));
    for (int m = 0; m < 2; ++m)
      for (int c = 0; c < 2; ++c)
        for (int e = 0; e < 2; ++e)
          for (int p = 0; p < 2; ++p)
            for (int w = 0; w < 2; ++w)
              add((const void*)carry_kernel(modes[m], c != 0, e != 0, p != 0, w != 0),
                  join({"k_bounce_carry", mode_n[m], count_n[c], shading_n[e], primary_n[p], w ? "lanewalk" : "plain"}));
    for (int e = 0; e < 2; ++e)
      for (int p = 0; p < 2; ++p)
        for (int tl = 0; tl < 2; ++tl)
          add((const void*)carry_kernel_oct(e != 0, p != 0, tl != 0),
              join({"k_bounce_carry", "simd", "nocount", shading_n[e], primary_n[p], p ? "lanewalk" : "plain", tl ? "oct-tiles" : "oct"}));
    for (int i = 0; i < 2; ++i)
      for (int m = 0; m < 2; ++m)
        for (int c = 0; c < 2; ++c)
          for (int sh = 0; sh < 3; ++sh)
            for (int p = 0; p < 2; ++p)
              for (int l = 0; l < 2; ++l)
                for (int v = 0; v < 3; ++v)
                  add((const void*)bounce_kernel(modes[m], c != 0, (Shading)sh, p != 0, l != 0, (Variant)v, i != 0),
                      join({"k_bounce", mode_n[m], count_n[c], shading_n[sh], primary_n[p], lds_n[l], variant_n[v], img_n[i]}));
    return t;
  }();
  return table;
}

/* ---- one launch function per family: the kernel by its selector, prepared once, then grid, block and LDS from the schedule ---- */
constexpr int kNoBounce = -1; /* launch_trace: the rays are not a numbered bounce of a render (ptx_intersect_rays) */
/* work: 8 zeroed hand-out counters of this launch (PtChunkFeed); susp: the parked-walk buffer of the launching workspace set; bounce:
 * 0 for camera rays, b >= 1 for the queued rays of bounce b, kNoBounce */
void launch_trace(ptx_scene* s, hipStream_t st, const PtQueue& q, const PtHits& h, size_t n_upper, bool count, uint32_t* work,
                  uint4* susp, int bounce, const PrimaryLaunch& pl = PrimaryLaunch()) {
  const Schedule& sc = s->sched;
  const bool lds_scene = sc.in_lds();
  const int stack_depth = std::max(1, s->tree_depth + 1);
  const int kTraceBlock = sc.trace_threads;
  const size_t lds = sc.trace_lds;
  /* from HBM/L2 one shared node fetch per step serialises the latency (-3 %): packets only on LDS-resident scenes */
  /* (the same template switch selects the per-octant node image on scenes walked from HBM / L2: k_trace) */
  const bool packet = lds_scene ? (pl.on ? true : (bounce >= 1 && bounce <= s->bounce_packet))
                                : (s->dev.nodes32o != nullptr && !sc.top_in_lds);
  const TraceKernel kern = trace_kernel(s->dev.mode, count, pl.on, lds_scene, packet);
  prepare_kernel(s, (const void*)kern, "k_trace", lds_scene, 160 * 1024 - 1024, 1024);
  int blocks_per_cu = lds_scene ? std::min(4, std::max<int>(1, (int)((160 * 1024) / std::max<size_t>(lds, 1)))) : (PT_TRACE_GLOBAL_WAVES * 256) / kTraceBlockGlobal; /* what the registers admit: no stack in LDS any more */
  if (s->trace_wgs_per_cu > 0) blocks_per_cu = std::min(4, s->trace_wgs_per_cu); /* `susp` is sized for 4 */
  else if (sc.share_cus) {
    /* half of the CU's wave slots (see launch_shade_pool): two 512-thread workgroups, as long as their scene copies fit
     * beside the pools of the shade stage's two 256-thread workgroups (20.5 KB each).  Measured (round 3): the two-stream
     * frame is flat in the size of the scene copy up to that limit and 3-5 ms slower beyond it (108-byte nodes, or 48-byte
     * sphere slots: two trace and two shade workgroups no longer fit a CU together). */
    const size_t shade_lds = 2 * ((size_t)(256 / 64) * PT_N_SHADE_CAT * 128 * sizeof(uint2) + 256);
    const int by_lds = std::max<int>(1, (int)((160 * 1024 - shade_lds) / std::max<size_t>(lds, 1)));
    blocks_per_cu = std::max(1, std::min(std::min(blocks_per_cu, by_lds), 2 * (512 / std::max(64, kTraceBlock))));
  }
  const int grid = strided_grid(s, n_upper, kTraceBlock, blocks_per_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kTraceBlock), lds, st, s->dev, q, h, stack_depth, s->counters.p, pl.g, s->alpha.p, pl.n, work, susp, sc.top_in_lds);
}

/* k_shade_pool leaves holes in its output queue (part-filled blocks): at most one block per (workgroup, bin) */
size_t shade_pool_slack(const ptx_scene* s) { return (size_t)s->n_cu * (1024 / 256) * PT_POOL_BINS * PT_POOL_BLOCK; }
void launch_shade_pool(ptx_scene* s, hipStream_t st, const PtQueue& q, const PtHits& h, const PtQueue& out,
                       const PtContrib& c, size_t n_upper, int bounce, int last, uint32_t* work, const PrimaryLaunch& pl) {
  const Schedule& sc = s->sched;
  /* 128 VGPRs: 16 waves per CU.  With two batches in flight each kernel takes HALF of what a CU holds, so that one batch's
   * trace workgroups (vector-issue-bound) and the other's shade workgroups (bound by the memory system) are resident on every
   * CU together instead of taking turns at the chip */
  const int threads = (sc.share_cus || sc.img) ? 256 : PT_POOL_THREADS; /* 256 threads when two batches share every CU and for the IMG kernels, else 512 */
  const int most = (sc.img ? PT_IMG_WAVES * 256 : 1024) / threads;
  const int per_cu = s->shade_wgs_per_cu > 0 ? std::min(s->shade_wgs_per_cu, most) : (sc.share_cus ? std::max(1, most / 2) : most);
  const int grid = strided_grid(s, n_upper, threads, per_cu);
  const size_t lds = pt_lds_shade_pool_bytes(threads / 64);
  const ShadePoolKernel kern = shade_pool_kernel(scene_shading(s), pl.on, sc.img);
  s->attr_done.insert((const void*)kern); /* the launch record (ptx_scene_launched_kernels); its dynamic LDS needs no raised limit */
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, s->dev, q, h, out, c, s->alpha.p, bounce, last, pl.g, pl.n, work);
}

void launch_bounce_carry(ptx_scene* s, hipStream_t st, const PtQueue& q, const PtHits& h, const PtQueue& out, const PtHits& hout,
                         const PtContrib& c, size_t n_upper, int bounce, int last, bool count, const PrimaryLaunch& pl) {
  const Schedule& sc = s->sched;
  const int stack_depth = std::max(1, s->tree_depth + 1);
  const bool oct = sc.lds_oct && !count;
  /* the camera launch scans tile lists where the render has them (render_raw: s->tile_cur) */
  const bool tile = oct && pl.on && sc.tile_lists && s->tile_cur != nullptr;
  PtSceneDev dev = s->dev;
  dev.tile_lists = tile ? s->tile_cur->buf.p : nullptr;
  if (tile) {
    s->tile_launches++;
    s->tile_last = s->tile_cur;
  }
  const CarryKernel kern = oct ? carry_kernel_oct(s->dev.has_emit != 0, pl.on, tile) : carry_kernel(s->dev.mode, count, s->dev.has_emit != 0, pl.on, sc.lane_walk);
  prepare_kernel(s, (const void*)kern, "k_bounce_carry", !oct /* (record numbers, not 16-bit addresses) */, 160 * 1024 - 256, PT_LDS_CU_BYTES - PT_LDS_BOUNCE_LIMIT);
  const int threads = sc.bounce_threads;
  int grid = strided_grid(s, n_upper, threads, 1); /* one workgroup (one scene image) per CU */
  if (s->bounce_wgs > 0) grid = std::max(1, std::min(grid, s->bounce_wgs));
  if (oct) s->lds_oct_launched = true;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), oct ? sc.carry_oct.total : sc.carry.total, st, dev, q, h, out, hout, c, s->alpha.p, bounce, last, pl.g, pl.n,
                     stack_depth, (uint32_t)(oct ? sc.carry_oct.pool_off : sc.carry.pool_off), s->counters.p, s->bounce_fence_wg);
}

void launch_bounce(ptx_scene* s, hipStream_t st, const PtQueue& q, const PtHits& h, const PtQueue& out, const PtContrib& c,
                   size_t n_upper, int bounce, int last, bool count, const PrimaryLaunch& pl, const PtSolo& solo) {
  const Schedule& sc = s->sched;
  const bool lds_scene = !sc.from_hbm;
  const int stack_depth = std::max(1, s->tree_depth + 1);
  /* the instantiation with the loop over a batch's remaining bounces (PtSolo) only where it can be taken */
  /* (LIT: the walk-first kernel without the solo loop, whatever PTX_SOLO_ENTRIES says -- run_bounces hands it no flag) */
  /* (camera rays of an LDS-resident scene: the packet walk or one ray per lane, Schedule::lane_walk) */
  const Variant variant = pl.on ? (sc.lane_walk ? Variant::lane_walk : Variant::plain) : (solo.flag != nullptr ? Variant::solo : Variant::plain);
  const BounceKernel kern = bounce_kernel(s->dev.mode, count, scene_shading(s), pl.on, lds_scene, variant, sc.img);
  prepare_kernel(s, (const void*)kern, "k_bounce", lds_scene, 160 * 1024 - 256, PT_LDS_CU_BYTES - PT_LDS_BOUNCE_LIMIT);
  const int threads = sc.bounce_threads;
  /* LDS scenes: one workgroup (one scene image) per CU; walks from HBM / L2: what the registers admit (PT_BOUNCE_WAVES per SIMD) --
   * shade_pool_slack and the parked-walk buffer are sized for 4 workgroups per CU */
  const int per_cu = lds_scene ? 1 : std::max(1, std::min(4, ((sc.img ? PT_IMG_WAVES : PT_BOUNCE_WAVES) * 256) / threads));
  int grid = strided_grid(s, n_upper, threads, per_cu);
  if (s->bounce_wgs > 0) grid = std::max(1, std::min(grid, s->bounce_wgs));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), sc.bounce.total, st, s->dev, q, h, out, c, s->alpha.p, bounce, last, pl.g, pl.n, stack_depth,
                     (uint32_t)sc.bounce.pool_off, s->counters.p, s->bounce_fence_wg, solo);
}

struct Workspace {
  PtQueue q[2];
  PtHits hits;
  PtContrib contrib;
  uint32_t* counts; /* counts[b] = live paths entering bounce b (b >= 1; counts[0] for list-mode generation) */
  uint4* susp = nullptr;
  size_t cap_entries = 0; /* queue / hit-record capacity */
  size_t carry_stride = 0; /* k_bounce_carry: the hit arrays hold a second half of this many entries (0: they do not) */
  double* contrib_all = nullptr;
  size_t contrib_n = 0;
};

/* The sampler's dimension for renders of this depth: 2 + 2 max_bounces, two more -- the lens pair -- while the scene has a lens and
 * one more -- the last, the sample's time -- while it has a shutter (include/ptx.h: every alpha of the table then differs from the
 * pinhole's) */
int sampler_dimension(const ptx_scene* s, int max_bounces) {
  return 2 + 2 * std::max(max_bounces, 0) + (s->lens_radius > 0.0 ? 2 : 0) + (s->shutter_on ? 1 : 0);
}
/* the lens of a launch (Schedule::lens): its pair is the sampler's last two dimensions, or the two before a shutter's time */
PtLens scene_lens(const ptx_scene* s, int max_bounces) {
  return PtLens{s->lens_radius, s->lens_focus, sampler_dimension(s, max_bounces) - (s->shutter_on ? 1 : 0)};
}
/* the shutter of a launch (Schedule::shutter) */
PtShutter scene_shutter(const ptx_scene* s, int max_bounces) {
  PtShutter sh;
  std::memcpy(sh.tr, s->shutter_translation, sizeof sh.tr);
  std::memcpy(sh.k, s->shutter_axis, sizeof sh.k);
  sh.angle = s->shutter_angle;
  sh.dim = sampler_dimension(s, max_bounces);
  return sh;
}
/* the pose of a launch (Schedule::pose): the view is the pose's own or the scene's */
PtCameraPose scene_pose(const ptx_scene* s) {
  PtCameraPose cp;
  std::memcpy(cp.o, s->pose_origin, sizeof cp.o);
  std::memcpy(cp.r, s->pose_rotation, sizeof cp.r);
  const ptx_camera& view = s->pose_has_view ? s->pose_view : s->own_view;
  cp.llx = view.lower_left_x; cp.lly = view.lower_left_y; cp.vx = view.view_x; cp.vy = view.view_y;
  return cp;
}

/* ---- the camera of a launch: which generator instantiation writes a scene's camera rays (camera_rays.inc) ---- */
/* the one place that maps a scene's state to a camera kind */
PtCameraKind camera_kind(const Schedule& c) {
  if (c.shutter) return c.latlong ? PT_CAM_LATLONG_SHUTTER : c.lens ? PT_CAM_POSE_LENS_SHUTTER : PT_CAM_POSE_SHUTTER;
  if (c.latlong) return PT_CAM_LATLONG;
  if (c.pose) return c.lens ? PT_CAM_POSE_LENS : PT_CAM_POSE;
  return c.lens ? PT_CAM_LENS : PT_CAM_PINHOLE;
}
/* what the kinds read, for renders of this depth (a kind reads its own fields and no other) */
PtCameraArg scene_camera(const ptx_scene* s, int max_bounces) {
  return PtCameraArg{scene_pose(s), scene_lens(s, max_bounces), scene_shutter(s, max_bounces)};
}
/* the one switch over kinds: f(std::integral_constant<int, kind>) with the run-time kind made a compile-time constant */
template <class F>
void with_camera_kind(PtCameraKind kind, F&& f) {
  switch (kind) {
    case PT_CAM_PINHOLE: return f(std::integral_constant<int, PT_CAM_PINHOLE>());
    case PT_CAM_LENS: return f(std::integral_constant<int, PT_CAM_LENS>());
    case PT_CAM_POSE: return f(std::integral_constant<int, PT_CAM_POSE>());
    case PT_CAM_POSE_LENS: return f(std::integral_constant<int, PT_CAM_POSE_LENS>());
    case PT_CAM_LATLONG: return f(std::integral_constant<int, PT_CAM_LATLONG>());
    case PT_CAM_POSE_SHUTTER: return f(std::integral_constant<int, PT_CAM_POSE_SHUTTER>());
    case PT_CAM_POSE_LENS_SHUTTER: return f(std::integral_constant<int, PT_CAM_POSE_LENS_SHUTTER>());
    case PT_CAM_LATLONG_SHUTTER: return f(std::integral_constant<int, PT_CAM_LATLONG_SHUTTER>());
  }
}
/* The camera rays of a whole batch in the fused camera launch's order, written to q (pl.n entries, holes included).  path = false: the
 * rays alone (the feature slices).  Not for the pinhole, whose whole batch IS the fused camera launch: callers ask sched.lens || pose. */
void launch_generate_tiles(const ptx_scene* s, const ptx_render_params* p, const PrimaryLaunch& pl, bool path, const PtQueue& q, hipStream_t st) {
  const PtCameraArg cam = scene_camera(s, p->max_bounces);
  with_camera_kind(camera_kind(s->sched), [&](auto kind) {
    constexpr int CAM = decltype(kind)::value;
    if constexpr (CAM != PT_CAM_PINHOLE)
      hipLaunchKernelGGL((path ? k_generate_tiles<CAM, true> : k_generate_tiles<CAM, false>), grid256(pl.n), dim3(256), 0, st, s->dev, pl.g,
                         cam, (const double*)s->alpha.p, q);
  });
}
/* the camera rays of n_pass passes of a pixel list, dense and pass-major in q */
void launch_generate_pixels(const ptx_scene* s, const ptx_render_params* p, int first, int n_pass, const int32_t* d_list, long long n_list,
                            const PtQueue& q, hipStream_t st) {
  const PtCameraArg cam = scene_camera(s, p->max_bounces);
  const size_t n_paths = (size_t)n_pass * (size_t)n_list;
  with_camera_kind(camera_kind(s->sched), [&](auto kind) {
    hipLaunchKernelGGL(k_generate_pixels<decltype(kind)::value>, grid256(n_paths), dim3(256), 0, st, s->dev, p->width,
                       p->height, p->samples_per_pixel, first, n_pass, d_list, n_list, cam, (const double*)s->alpha.p, q);
  });
}

/* The sampler's alpha table of this dimension becomes the scene's current one (ptx_scene.alpha): looked up, or made and
 * uploaded the first time the dimension is asked for */
int use_alpha_table(ptx_scene* s, int dim) {
  double* table = nullptr;
  for (const auto& t : s->alpha_tables)
    if (t.first == dim) table = t.second;
  if (!table) {
    const std::vector<double> alpha = lds_alpha(dim); /* create_sampler, integrator.ml:89 */
    HIP_TRY(hipMalloc((void**)&table, sizeof(double) * (size_t)dim));
    /* uploaded first, cached on success only: a table whose upload failed must not be found by the next render of this depth */
    if (hipMemcpy(table, alpha.data(), sizeof(double) * (size_t)dim, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(table);
      return fail(PTX_ERR_HIP, "uploading the sampler's alpha table (%d dimensions) failed", dim);
    }
    s->alpha_tables.emplace_back(dim, table); /* owned from here on (freed by ptx_scene_destroy) */
  }
  s->alpha.p = table;
  return 0;
}

int ensure_workspace(ptx_scene* s, size_t cap, int max_bounces, Workspace* w, int set = 0, bool want_hit_records = false) {
  ptx_scene::WorkBufs& b = s->wb[set];
  const size_t cap_paths = cap;
  cap += shade_pool_slack(s); /* queue entries, not rays: room for the holes */
  if (s->solo_entries > 0 && max_bounces > 2) {
    /* a launch runs solo (k_bounce, PtSolo) only if each queue could hold the worst case of every remaining bounce, and on a small
     * frame -- where it matters -- that is more than the paths themselves: room for a solo run from the first queued bounce on,
     * as far as 16 M extra entries go */
    const size_t holes = (size_t)s->n_cu * (s->sched.from_hbm ? 4 : 1) * PT_POOL_BINS * PT_POOL_BLOCK;
    const size_t n1 = std::min(cap_paths + holes, (size_t)s->solo_entries);
    const size_t worst = (size_t)((std::min(max_bounces, 16) - 1) / 2 + 1) * (n1 + holes) + n1 + PT_POOL_BLOCK;
    cap = std::max(cap, std::min(worst, cap + ((size_t)16 << 20)));
  }
  HIP_TRY(b.qa.ensure(cap, s->dev.has_emit != 0));
  HIP_TRY(b.qb.ensure(cap, s->dev.has_emit != 0));
  /* {t, u, v, -} records (barycentrics exist for triangle hits only): kept for ptx_intersect_rays, which hands t back; a render's
   * shade step recomputes them (PtHits) and the buffer is not even allocated */
  const bool hit_records = s->dev.has_triangles && want_hit_records;
  if (hit_records) HIP_TRY(b.hit_tuv.ensure(cap * 4));
  /* k_bounce_carry reads its input's hits while it writes its output's: entries of even and odd bounces in two halves */
  const bool carry = s->sched.carry_ok && !hit_records;
  if (!hit_records) HIP_TRY(b.hit_t.ensure(((s->solo_entries > 0 || carry) && !s->dev.has_triangles) ? 2 * cap : cap)); /* (PtHits.t_parity_stride: a solo launch keeps the distances of even and odd bounces apart) */
  HIP_TRY(b.hit_slot.ensure(carry ? 2 * cap : cap));
  HIP_TRY(b.contrib.ensure(cap * 4));
  HIP_TRY(b.counts.ensure(kCountsWords));
  /* parked walks of k_trace: <= 4 workgroups of <= 16 waves per CU with 64 states (3 x 16 bytes) per wave (k_bounce keeps its own in LDS) */
  HIP_TRY(b.susp.ensure((size_t)s->n_cu * 4 * 16 * PT_WAVE * 3));
  HIP_TRY(s->counters.ensure(1));
  { /* (every set: a cached lookup) */
    const int rc = use_alpha_table(s, sampler_dimension(s, max_bounces));
    if (rc) return rc;
  }
  /* views must use the capacity the buffers were SIZED with */
  b.qa.cap = b.qa.ray.n;
  b.qb.cap = b.qb.ray.n;
  w->counts = b.counts.p;
  w->susp = b.susp.p;
  w->cap_entries = cap;
  w->carry_stride = carry ? cap : 0;
  w->q[0] = b.qa.view(nullptr);
  w->q[1] = b.qb.view(nullptr);
  w->hits.t = s->dev.has_triangles ? nullptr : b.hit_t.p;
  w->hits.slot = b.hit_slot.p;
  w->hits.tuv = hit_records ? (double4*)b.hit_tuv.p : nullptr;
  w->hits.t_parity_stride = (!hit_records && !s->dev.has_triangles && s->solo_entries > 0) ? cap : 0;
  w->contrib.rgbx = (double4*)b.contrib.p;
  w->contrib_all = b.contrib.p;
  w->contrib_n = b.contrib.n;
  return 0;
}

/* The bounce loop.  Bounce b reads queue (b & 1) whose live count is counts[b] and appends survivors to
 * queue ((b + 1) & 1), count counts[b + 1]; counts[] must be zero on entry (one memset per batch).
 * With pl.on, bounce 0 is a PRIMARY launch (no input queue).  n_upper bounds every live count. */
void run_bounces(ptx_scene* s, hipStream_t st, Workspace& w, size_t n_upper, int max_bounces, bool count, bool timed,
                 const PrimaryLaunch& pl, int run_only = -1) {
  const int n_run = run_only >= 0 ? run_only : max_bounces;
  const Schedule& sc = s->sched;
  const bool fused = sc.fused_ok(w.cap_entries);
  /* the shade-first order: a whole batch from its camera launch on (its launch b shades bounce b and walks bounce b + 1) */
  /* (w.carry_stride > 0: ensure_workspace sized the hit arrays for it, from the same Schedule) */
  const bool carry = pl.on && run_only < 0 && max_bounces >= 2 && w.carry_stride > 0 && sc.carry_ok && fused;
  for (int b = 0; b < n_run; ++b) {
    PtQueue in = w.q[b & 1], out = w.q[(b + 1) & 1];
    in.count = w.counts + b;
    out.count = w.counts + b + 1;
    const PrimaryLaunch here = (b == 0) ? pl : PrimaryLaunch();
    const int last = (b == max_bounces - 1) ? 1 : 0;
    if (carry) {
      LaunchTimer t(s, st, timed, PTX_KERNEL_BOUNCE);
      PtHits h_in = w.hits, h_out = w.hits;
      h_in.slot += (size_t)(b & 1) * w.carry_stride;
      h_out.slot += (size_t)((b + 1) & 1) * w.carry_stride;
      if (w.hits.t) {
        h_in.t += (size_t)(b & 1) * w.carry_stride;
        h_out.t += (size_t)((b + 1) & 1) * w.carry_stride;
      }
      launch_bounce_carry(s, st, in, h_in, out, h_out, w.contrib, n_upper, b, last, count, here);
      continue;
    }
    if ((!here.on || s->fused >= 2) && fused) { /* PTX_FUSED=2: the camera rays' bounce too */
      LaunchTimer t(s, st, timed, PTX_KERNEL_BOUNCE);
      /* PtSolo: the first launch whose input has shrunk to s->solo_entries runs the batch's remaining bounces by itself, the
       * later ones return at once (the flag: a word of the batch's counts, zeroed with them).  A partial run (run_only) and a
       * hit-distance array without its second half never run solo. */
      PtSolo solo;
      solo.flag = (run_only < 0 && s->solo_entries > 0 && !sc.lit && !sc.img && !sc.pose && (s->dev.has_triangles || w.hits.t_parity_stride > 0)) ? w.counts + kSoloFlagWord : nullptr;
      solo.max_entries = (uint32_t)std::max(0, s->solo_entries);
      solo.max_bounces = max_bounces;
      solo.cap_entries = (uint32_t)std::min<size_t>(w.cap_entries, 0xffffffffu);
      launch_bounce(s, st, in, w.hits, out, w.contrib, n_upper, b, last, count, here, solo);
      continue;
    }
    {
      LaunchTimer t(s, st, timed, PTX_KERNEL_TRACE);
      /* (list-mode bounce 0, explicit samples, reads a queue like any bounce) */
      launch_trace(s, st, in, w.hits, n_upper, count, w.counts + kWorkBase + (size_t)b * kWorkPerBounce, w.susp, here.on ? 0 : std::max(b, 1), here);
    }
    {
      LaunchTimer t(s, st, timed, PTX_KERNEL_SHADE);
      uint32_t* wk = w.counts + kWorkBase + (size_t)b * kWorkPerBounce;
      launch_shade_pool(s, st, in, w.hits, out, w.contrib, n_upper, b, last, wk + 8, here);
    }
  }
}

void collect_timing(ptx_scene* s, ptx_stats* stats) {
  for (const TimedLaunch& t : s->timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess && stats) {
      stats->kernel_ms[t.kind] += (double)ms;
      stats->kernel_launches[t.kind] += 1;
    }
  }
  s->timed.clear();
  s->event_next = 0;
}

int collect_counters(ptx_scene* s, ptx_stats* stats) {
  PtCounters c;
  HIP_TRY(hipMemcpy(&c, s->counters.p, sizeof c, hipMemcpyDeviceToHost));
  stats->segments = (int64_t)c.segments;
  stats->nodes_tested = (int64_t)c.nodes;
  stats->prims_tested = (int64_t)c.prims;
  stats->floor_tested = (int64_t)c.floor;
  stats->filter_undecided = (int64_t)c.undecided;
  stats->filter_fallback_steps = (int64_t)c.fallback_steps;
  stats->solo_launches = (int32_t)c.solo;
  stats->carry_launches = (int32_t)c.carry;
  stats->primary_lane_walks = (int32_t)c.lane_walks;
  return 0;
}

void fill_tree_stats(const ptx_scene* s, ptx_stats* st) {
  st->tree_nodes = (int32_t)s->host->nodes.size();
  st->tree_depth = s->tree_depth;
  st->tree_leaves = s->tree_leaves;
  st->leaf_slots = s->dev.n_slots;
  st->build_ms = s->build_ms;
  st->traversal_in_lds = (s->device >= 0 && s->sched.in_lds()) ? 1 : 0;
  st->bvh_built_on_gpu = s->built_on_gpu ? 1 : 0;
}

/* How many sampling passes (one sample of every pixel each) are traced together.  Large batches amortise the
 * per-launch tail and the per-workgroup LDS scene load: on the headline frame 2 batches of 32 passes (66M paths,
 * ~13 GB of queues per batch) render 9 % faster than 8 batches of 8.  The count is made even so the two streams
 * get the same number of batches, and a job that would fit one batch is still split in two for them. */
int choose_passes_per_batch(const ptx_render_params* p, long long npix, long long padded, int n_passes) {
  const long long spp = n_passes; /* the passes this call renders: the whole frame, or a slice of it */
  long long k = std::min<long long>(p->passes_per_batch, spp);
  if (k <= 0) {
  long long target = 80ll << 20; /* paths in flight per batch */
  if (const char* e = getenv("PTX_BATCH_PATHS")) target = std::max(1ll, atoll(e));
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    /* two workspace sets of ~204 B per path; stay below a quarter of what is free */
    const long long fit = (long long)(free_b / 4 / 408);
    target = std::max(1ll << 20, std::min(target, fit));
  }
  k = std::max(1ll, std::min(spp, target / std::max<long long>(npix, 1)));
  long long n_batches = (spp + k - 1) / k;
  if (n_batches == 1 && spp >= 2 && npix * spp >= (4ll << 20)) n_batches = 2;
  else if (n_batches > 1 && (n_batches & 1)) ++n_batches;
  k = (spp + n_batches - 1) / n_batches;
  }
  /* queue / hit-record indices and contribution ids are 32-bit */
  while (k > 1 && k * padded >= 0xffffffffll) --k;
  return (int)k;
}

/* the whole integrator for this rank's rows -> raw per-pixel sums at d_raw (rows*W*3) */
/* A slice of the frame (ptx_render_passes_device, render_updates): passes [pass_first, pass_first + pass_count) of the
 * frame of p->samples_per_pixel passes (the sampler offsets depend on that total), ADDED to d_raw when zero is false; d_sq, if
 * given, receives the sums of the squared contributions in the same order (k_accum_sq) */
struct PassRange {
  int first = 0, count = -1; /* count < 0: the whole frame [0, samples_per_pixel) */
  bool zero = true;
  double* d_sq = nullptr;
  /* list mode (ptx_render_pixels_device, ptx_render_adaptive): only the n_list pixels of the DEVICE list d_list (whole image,
   * y * W + x), their camera rays written by k_generate_pixels and bounced from a queue; d_passes (nullable), the count map, gets
   * the range's end for every listed pixel */
  const int32_t* d_list = nullptr;
  long long n_list = 0;
  int32_t* d_passes = nullptr;
  PassRange() = default;
  PassRange(int first_, int count_, bool zero_, double* d_sq_) : first(first_), count(count_), zero(zero_), d_sq(d_sq_) {}
  PassRange listed(const int32_t* list, long long n, int32_t* passes) const { /* list == nullptr: the whole image */
    PassRange r = *this;
    r.d_list = list;
    r.n_list = list ? n : 0;
    r.d_passes = passes;
    return r;
  }
};
/* ptx_render's tail (below): row slabs of the frame's last accumulate, an event recorded behind each */
constexpr int kMaxFinalSlabs = 8;
constexpr int kMinSlabImageRows = 64; /* ptx_render cuts the tail of a pinned image into slabs from this height on */
/* render_into_pinned films slab k once slab k + 1 has been summed; the film reads pixel_radius rows beyond a slab on both sides, so
 * every slab must hold at least the largest radius in rows */
static_assert(kMinSlabImageRows / kMaxFinalSlabs >= PTX_FILM_MAX_RADIUS, "a row slab of a pinned image must be at least PTX_FILM_MAX_RADIUS rows high");
struct FinalSlabs {
  int n = 0;
  int row[kMaxFinalSlabs + 1] = {};   /* slab k = image rows [row[k], row[k + 1]) */
  hipEvent_t done[kMaxFinalSlabs] = {};
  bool used = false;                  /* out: the last batch was accumulated in slabs and the events were recorded */
};

/* render_raw, piece 1: how the range's passes are cut into batches and how many of them are in flight */
struct BatchPlan {
  int rows = 0, pass_first = 0, pass_count = 0, pass_end = 0;
  long long npix = 0, per_pass = 0; /* pixels of this rank; samples of one pass (the list's length in list mode) */
  bool list = false;
  size_t padded = 0, cap = 0;       /* entries of one pass in a queue; of one batch */
  int ppb = 0, n_batches = 0, n_sets = 0;
};
int plan_batches(ptx_scene* s, const ptx_render_params* p, const PassRange& range, BatchPlan* out) {
  BatchPlan& b = *out = BatchPlan();
  b.rows = local_rows(p);
  b.pass_first = range.count < 0 ? 0 : range.first;
  b.pass_count = range.count < 0 ? p->samples_per_pixel : range.count;
  b.pass_end = b.pass_first + b.pass_count;
  b.npix = (long long)b.rows * p->width;
  b.list = range.d_list != nullptr;
  if (b.npix == 0 || (b.list && range.n_list == 0)) return 0; /* n_batches stays 0: nothing to render */
  if (b.npix >= 0xffffffffll) return fail(PTX_ERR_ARG, "too many pixels for one rank");
  /* bounce-0 hit records are indexed by the VIRTUAL primary index (8x8 tiles, ragged edges padded); a list's queue is dense */
  b.padded = b.list ? (size_t)range.n_list : (size_t)((p->width + 7) / 8) * (size_t)((b.rows + 7) / 8) * 64;
  b.per_pass = b.list ? range.n_list : b.npix;
  b.ppb = choose_passes_per_batch(p, b.per_pass, (long long)b.padded, b.pass_count);
  /* the blocked output queue of k_shade_pool numbers its blocks in 20 bits: 268 M entries per batch */
  while (b.ppb > 1 && (size_t)b.ppb * b.padded + shade_pool_slack(s) >= kPoolMaxEntries) --b.ppb;
  if ((size_t)b.ppb * b.padded + shade_pool_slack(s) >= kPoolMaxEntries)
    return fail(PTX_ERR_ARG, "one pass over %lld pixels exceeds the %zu entries a path queue can number (block numbers are 20 bits): render the image in bands", b.per_pass, kPoolMaxEntries);
  b.cap = (size_t)b.ppb * b.padded;
  b.n_batches = (b.pass_count + b.ppb - 1) / b.ppb;
  /* Two batches in flight on two streams: trace is f64-VALU-bound, shade streams ~170 B per segment through
   * HBM; run side by side, one batch's shade fills the memory pipes while the other's trace fills the SIMDs. */
  b.n_sets = (b.n_batches >= 2 && p->max_bounces > 0) ? 2 : 1;
  if (const char* e = getenv("PTX_STREAMS")) b.n_sets = std::max(1, std::min(kMaxSets, atoi(e)));
  b.n_sets = std::min(b.n_sets, b.n_batches);
  reschedule(s, b.n_sets);
  return 0;
}

/* render_raw, piece 2: the lanes the batches run on (batch k on lane k % n_sets; one set: the caller's stream itself) */
struct Lanes {
  hipStream_t lane[kMaxSets] = {};
  bool overlap_frames = false;
};
/* fork: the lanes start after everything already queued on the caller's stream (a queued frame: only its k_accum does) */
int fork_lanes(ptx_scene* s, const ptx_render_params* p, const BatchPlan& b, hipStream_t st, bool has_progress, Lanes* l) {
  /* A QUEUED frame's bounces (PTX_RENDER_ASYNC) read the scene and this handle's workspace only, both ordered by the lanes
   * themselves, so they do not wait for what the caller's stream still carries -- the previous frame's join, band exchange and
   * film: a lane that has finished its batch of frame k starts frame k + 1 while the other lane still runs frame k's last
   * bounces (a few thousand rays per launch, most of the chip idle).  Only k_accum, the first kernel that touches the
   * caller's buffer, waits for the fork event.  One rank's share of an 8-rank job: 3.53 -> 3.44 ms per step.  (Two frames in
   * flight on two PAIRS of lanes, so that a frame's whole tail overlaps the next frame's head: 3.64 ms, and the full
   * frame 22.9 -> 23.5 ms -- four kernels sharing the CUs cost more than the idle tail they fill; measured, dropped.) */
  /* (a list is the caller's buffer, read by the first kernel of every batch: list mode always waits for the fork) */
  l->overlap_frames = (p->flags & PTX_RENDER_ASYNC) && !p->count_work && !p->time_kernels && !has_progress && !PT_SHADE_TIMING &&
                      b.n_sets >= 2 && !s->single_set_last && !b.list && env_int("PTX_OVERLAP_FRAMES", 1);
  s->single_set_last = b.n_sets < 2; /* (crosses calls: the next frame's overlap rule reads it) */
  for (int k = 0; k < kMaxSets; ++k) l->lane[k] = st;
  if (b.n_sets < 2) return 0;
  for (int k = 0; k < b.n_sets; ++k) {
    if (!s->streams[k]) HIP_TRY(hipStreamCreateWithFlags(&s->streams[k], hipStreamNonBlocking));
    if (!s->ev_accum[k]) HIP_TRY(hipEventCreateWithFlags(&s->ev_accum[k], hipEventDisableTiming));
    if (!s->ev_join[k]) HIP_TRY(hipEventCreateWithFlags(&s->ev_join[k], hipEventDisableTiming));
    l->lane[k] = s->streams[k];
  }
  if (!s->ev_fork) HIP_TRY(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(s->ev_fork, st));
  if (!l->overlap_frames)
    for (int k = 0; k < b.n_sets; ++k) HIP_TRY(hipStreamWaitEvent(l->lane[k], s->ev_fork, 0));
  return 0;
}
/* join: the caller's stream continues after every lane */
int join_lanes(ptx_scene* s, const BatchPlan& b, const Lanes& l, hipStream_t st) {
  for (int k = 0; k < b.n_sets && b.n_sets >= 2; ++k) {
    HIP_TRY(hipEventRecord(s->ev_join[k], l.lane[k]));
    HIP_TRY(hipStreamWaitEvent(st, s->ev_join[k], 0));
  }
  return 0;
}

/* render_raw, piece 3: one batch's camera rays and bounces on its lane -> the batch's contributions in w.contrib */
int queue_batch_paths(ptx_scene* s, const ptx_render_params* p, const BatchPlan& b, const PassRange& range, Workspace& w, hipStream_t ls,
                      int first, int n_pass) {
  const bool count = p->count_work != 0, timed = p->time_kernels != 0;
  const size_t n_paths = (size_t)n_pass * (size_t)b.per_pass;
  HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * kCountsWords, ls));
  if (p->max_bounces <= 0) {
    /* loop returns add_mul emit0 attn0 black = 0 for every sample (integrator.ml:31-32) */
    HIP_TRY(hipMemsetAsync(w.contrib_all, 0, sizeof(double) * w.contrib_n, ls));
  } else if (b.list) {
    PtQueue q0 = w.q[0];
    q0.count = w.counts;
    {
      LaunchTimer t(s, ls, timed, PTX_KERNEL_GENERATE);
      launch_generate_pixels(s, p, first, n_pass, range.d_list, range.n_list, q0, ls);
    }
    run_bounces(s, ls, w, n_paths, p->max_bounces, count, timed, PrimaryLaunch());
  } else {
    PrimaryLaunch pl;
    pl.on = true;
    PtGenParams& g = pl.g;
    g.width = p->width; g.height = p->height; g.spp = p->samples_per_pixel; g.local_rows = b.rows;
    g.band_rows = p->band_rows > 0 ? p->band_rows : 32; g.band_first = p->band_first; g.band_step = p->band_step;
    g.tiles_x = (p->width + 7) / 8; g.tiles_y = (b.rows + 7) / 8;
    g.first_pass = first; g.n_pass = n_pass;
    pl.n = (uint32_t)((size_t)n_pass * (size_t)g.tiles_x * (size_t)g.tiles_y * 64u);
    if (s->sched.lens || s->sched.pose) {
      /* the fused camera launch's virtual queue made real: pl.n entries in its order (b.cap is sized for them), then queued bounces */
      PtQueue q0 = w.q[0];
      q0.count = w.counts;
      {
        LaunchTimer t(s, ls, timed, PTX_KERNEL_GENERATE);
        launch_generate_tiles(s, p, pl, true, q0, ls);
      }
      run_bounces(s, ls, w, (size_t)pl.n, p->max_bounces, count, timed, PrimaryLaunch());
    } else {
      run_bounces(s, ls, w, std::max<size_t>(n_paths, pl.n), p->max_bounces, count, timed, pl);
    }
  }
  return 0;
}

/* render_raw, piece 4: one batch's contributions added to the caller's sums -- the only place that knows about squares, lists,
 * count maps and row slabs */
int queue_batch_accumulate(ptx_scene* s, const ptx_render_params* p, const BatchPlan& b, const PassRange& range, FinalSlabs* slabs,
                           const Workspace& w, hipStream_t ls, double* d_raw, int first, int n_pass) {
  const bool timed = p->time_kernels != 0, last_batch = first + b.ppb >= b.pass_end;
  LaunchTimer t(s, ls, timed, PTX_KERNEL_ACCUM);
  const dim3 grid(grid256(b.per_pass)), block(256);
  if (b.list) {
    hipLaunchKernelGGL(k_accum_list, grid, block, 0, ls, w.contrib, range.n_list, n_pass, range.d_list, d_raw, range.d_sq, range.d_passes,
                       first + n_pass);
  } else if (range.d_sq) {
    hipLaunchKernelGGL(k_accum_sq, grid, block, 0, ls, w.contrib, b.npix, n_pass, d_raw, range.d_sq, 0ll, b.npix);
  } else if (slabs && slabs->n > 1 && last_batch && !timed) {
    /* the frame's last accumulate in row slabs, an event behind each: the caller films and copies slab k while k + 1 is summed */
    for (int k = 0; k < slabs->n; ++k) {
      const long long q0 = (long long)slabs->row[k] * p->width, q1 = (long long)slabs->row[k + 1] * p->width;
      if (q1 > q0) hipLaunchKernelGGL(k_accum, grid256(q1 - q0), block, 0, ls, w.contrib, b.npix, n_pass, d_raw, q0, q1);
      HIP_TRY(hipEventRecord(slabs->done[k], ls));
    }
    slabs->used = true;
  } else {
    hipLaunchKernelGGL(k_accum, grid, block, 0, ls, w.contrib, b.npix, n_pass, d_raw, 0ll, b.npix);
  }
  return 0;
}

/* render_raw, piece 5: update_progress gets pixel areas summing to W*H (integrator.ml:150, render_command.ml:87-103).  The batches
 * keep running on both streams; the host only waits for their accumulate steps in order, on the calling thread. */
int wait_progress(const BatchPlan& b, const std::vector<hipEvent_t>& batch_done, ptx_progress_fn progress, void* user) {
  long long done_pixels_reported = 0;
  int k = 0;
  for (int first = b.pass_first; first < b.pass_end; first += b.ppb, ++k) {
    HIP_TRY(hipEventSynchronize(batch_done[(size_t)k]));
    const int n_pass = std::min(b.ppb, b.pass_end - first);
    const long long upto = (long long)((double)(first - b.pass_first + n_pass) / b.pass_count * (double)b.npix);
    progress(user, upto - done_pixels_reported);
    done_pixels_reported = upto;
  }
  return 0;
}

/* The camera tile lists of a width x height image on this scene's device: the host grid out of the cache shared with the replicas (built
 * the first time any of them renders that size), uploaded once per device.  nullptr: no lists (the launch walks the tree). */
const TileListsDev* tile_lists_for(ptx_scene* s, int width, int height) {
  for (const auto& t : s->tile_dev)
    if (t->grid->width == width && t->grid->height == height) return t.get();
  /* at most kMaxTileGrids image sizes per handle: nothing is evicted (a queued frame may still be reading an upload), a further size walks */
  if (!s->tile_cache || s->tile_dev.size() >= kMaxTileGrids) return nullptr;
  std::shared_ptr<const PtTileGrid> grid;
  {
    std::lock_guard<std::mutex> lock(s->tile_cache->mu);
    for (const auto& g : s->tile_cache->grids)
      if (g->width == width && g->height == height) grid = g;
    if (!grid) {
      if (s->tile_cache->grids.size() >= kMaxTileGrids) return nullptr;
      grid = std::make_shared<const PtTileGrid>(scene_tile_lists(*s->host, width, height));
      s->tile_cache->grids.push_back(grid);
    }
  }
  if (grid->rec.empty()) return nullptr;
  auto t = std::make_unique<TileListsDev>();
  t->grid = grid;
  const size_t words = grid->rec.size() * (sizeof(PtTileRec) / sizeof(uint32_t));
  if (t->buf.ensure(words) != hipSuccess || hipMemcpy(t->buf.p, grid->rec.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  s->tile_dev.push_back(std::move(t));
  return s->tile_dev.back().get();
}

int render_raw(ptx_scene* s, const ptx_render_params* p, double* d_raw, hipStream_t st, ptx_stats* stats,
               ptx_progress_fn progress, void* user, FinalSlabs* slabs = nullptr, const PassRange& range = PassRange()) {
  RenderBusy busy(s);
  s->event_next = 0; /* an earlier call that failed half-way may have left these behind */
  s->timed.clear();
  s->lds_oct_launched = false;
  s->tile_cur = s->tile_last = nullptr;
  s->tile_launches = 0;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    fill_tree_stats(s, stats);
  }
  struct GridDivGuard { /* every exit path, also the HIP_TRY ones, leaves later launches on this scene with whole grids */
    ptx_scene* s;
    ~GridDivGuard() { s->grid_div = 1; reschedule(s, 1); }
  } grid_div_guard{s};
  BatchPlan b;
  int rc = plan_batches(s, p, range, &b);
  if (rc || b.n_batches == 0) return rc;
  const bool count = p->count_work != 0, timed = p->time_kernels != 0;
  Workspace ws[kMaxSets];
  for (int k = 0; k < b.n_sets; ++k) {
    rc = ensure_workspace(s, b.cap, p->max_bounces, &ws[k], k);
    if (rc) return rc;
  }
  if (range.zero) {
    HIP_TRY(hipMemsetAsync(d_raw, 0, sizeof(double) * (size_t)b.npix * 3, st));
    if (range.d_sq) HIP_TRY(hipMemsetAsync(range.d_sq, 0, sizeof(double) * (size_t)b.npix * 3, st));
  }
  if (count) HIP_TRY(hipMemsetAsync(s->counters.p, 0, sizeof(PtCounters), st));
  /* camera tile lists: non-counting renders of whole images, or of bands the global tile grid can be indexed with (a band = whole tile
   * rows: pt_global_row(g, 8 ty) >> 3); a list render (adaptive rounds) has no camera launch */
  if (s->sched.tile_lists && !count && !b.list && p->max_bounces >= 2 && (p->band_step <= 1 || (p->band_rows > 0 ? p->band_rows : 32) % 8 == 0)) {
    s->tile_cur = tile_lists_for(s, p->width, p->height);
    /* the fallback counter runs on from the handle's first list render (or its last counting render, whose memset above covers it):
     * zeroing it per render would race with the lanes' camera launches and with a frame still queued */
    if (s->tile_cur && !s->tile_fallbacks_zeroed) {
      HIP_TRY(hipMemcpy(&s->counters.p->tile_fallbacks, &kZero64, sizeof kZero64, hipMemcpyHostToDevice));
      s->tile_fallbacks_zeroed = true;
    }
  }
  Lanes l;
  rc = fork_lanes(s, p, b, st, progress != nullptr, &l);
  if (rc) return rc;
  /* Grids cover the whole chip for every batch in flight; how many workgroups a CU takes of each kernel is decided per launch
   * (Schedule::share_cus: half a CU each on Simd_leaf LDS scenes). */
  s->grid_div = std::max(1, env_int("PTX_GRID_DIV", 1));
  std::vector<hipEvent_t> batch_done; /* progress: one event per batch, waited for in order after everything is queued */
  int batch = 0;
  for (int first = b.pass_first; first < b.pass_end; first += b.ppb, ++batch) {
    const int set = batch % b.n_sets;
    hipStream_t ls = l.lane[set];
    const int n_pass = std::min(b.ppb, b.pass_end - first);
    rc = queue_batch_paths(s, p, b, range, ws[set], ls, first, n_pass);
    if (rc) return rc;
    /* raw sums are accumulated in PASS order: batch k's accumulate runs after batch k-1's */
    if (b.n_sets >= 2 && batch > 0) HIP_TRY(hipStreamWaitEvent(ls, s->ev_accum[(batch - 1) % b.n_sets], 0));
    if (b.n_sets >= 2 && l.overlap_frames && batch < b.n_sets) HIP_TRY(hipStreamWaitEvent(ls, s->ev_fork, 0)); /* the caller's buffer: see the fork */
    rc = queue_batch_accumulate(s, p, b, range, slabs, ws[set], ls, d_raw, first, n_pass);
    if (rc) return rc;
    if (b.n_sets >= 2) HIP_TRY(hipEventRecord(s->ev_accum[set], ls));
    HIP_TRY(hipGetLastError());
    if (progress) {
      const hipEvent_t ev = scene_event(s);
      HIP_TRY(hipEventRecord(ev, ls));
      batch_done.push_back(ev);
    }
  }
  if (progress) {
    rc = wait_progress(b, batch_done, progress, user);
    if (rc) return rc;
  }
  rc = join_lanes(s, b, l, st);
  if (rc) return rc;
  /* PTX_RENDER_ASYNC: the frame is queued, the caller's stream carries the order (everything above is stream-ordered: the
   * lanes fork from `st` and join it, the workspace is reused in stream order, a reallocation synchronises by itself) */
  const bool wait = !(p->flags & PTX_RENDER_ASYNC) || count || timed || progress || PT_SHADE_TIMING;
  if (wait) HIP_TRY(hipStreamSynchronize(st));
#if PT_SHADE_TIMING
  { /* diagnostic build: the last batch of each workspace set, per bounce (units of 256 shader clocks, summed over waves) */
    std::vector<uint32_t> h(kCountsWords);
    for (int k = 0; k < b.n_sets; ++k) {
      HIP_TRY(hipMemcpy(h.data(), ws[k].counts, sizeof(uint32_t) * kCountsWords, hipMemcpyDeviceToHost));
      for (int bo = 0; bo < p->max_bounces; ++bo) {
        const uint32_t* t = h.data() + kWorkBase + (size_t)bo * kWorkPerBounce + 8 + 16;
        if (t[5]) fprintf(stderr, "shade_timing set %d bounce %d rays %u waves %u sort/refill %u entry %u append/push %u (first barrier/live lanes %u) store/steps %u life %u (longest wave %u, mean %u)\n", k, bo, h[bo], t[5], t[0], t[1], t[2], t[6], t[3], t[4], t[7], t[4] / t[5]);
      }
    }
  }
#endif
  if (stats) {
    stats->samples = (int64_t)b.per_pass * b.pass_count;
    stats->lds_oct_launches = s->lds_oct_launched ? 1 : 0;
    if (count) {
      rc = collect_counters(s, stats);
      if (rc) return rc;
    }
  }
  collect_timing(s, stats);
  return 0;
}


/* Level-synchronous GPU build (bvh_build_gpu.inc): the same tree as the host builder (csrc/bvh_build.cpp), left
 * on the device in its final layout.  The buffers belong to a per-thread, per-device workspace and stay valid
 * until the next build on the same thread (the photon mapper builds a tree per iteration; hipMalloc / hipFree of
 * a dozen buffers cost more than the build itself). */
struct BvhDeviceTree {
  const PtNode* nodes = nullptr;
  const int* slot_prim = nullptr; /* per leaf slot: index into the input boxes, -1 = padding */
  int n_nodes = 0, n_slots = 0, depth = 0, leaves = 0;
};
struct BvhGpuWorkspace {
  int device = -1;
  ThreadLifeBuf<double> d_box;
  ThreadLifeBuf<int> d_order, d_scratch, d_counts, d_tile_cl, d_tile_cr, d_slot;
  ThreadLifeBuf<BvhSeg> d_seg[2][3];
  ThreadLifeBuf<BvhTmpNode> d_tmp;
  ThreadLifeBuf<BvhFin> d_fin;
  ThreadLifeBuf<PtNode> d_nodes;
  ThreadLifeBuf<BvhBigSeg> d_big;
  ThreadLifeBuf<BvhBigState> d_bigstate;
  ThreadLifeBuf<int2> d_tiles;
  ThreadLifeBuf<unsigned long long> d_rootenc;
  void release() {
    d_box.release(); d_order.release(); d_scratch.release(); d_counts.release(); d_tile_cl.release(); d_tile_cr.release();
    d_slot.release(); d_tmp.release(); d_fin.release(); d_nodes.release(); d_big.release(); d_bigstate.release();
    d_tiles.release(); d_rootenc.release();
    for (int c = 0; c < 2; ++c) for (int k = 0; k < 3; ++k) d_seg[c][k].release();
  }
};
BvhGpuWorkspace& bvh_gpu_workspace() {
  static thread_local BvhGpuWorkspace ws;
  int cur_dev = 0;
  (void)hipGetDevice(&cur_dev);
  if (ws.device != cur_dev) {
    ws.release();
    ws.device = cur_dev;
  }
  return ws;
}

/* d_boxes: n x 6 doubles on the device (may be ws.d_box).  root: the tree's bbox if the caller has it (host
 * builds compute it while flattening), else it is reduced on the device. */
bool bvh_build_device(const double* d_boxes, int n, const Box* root, int num_bins, int length_cutoff, bool pad4,
                      BvhDeviceTree* out) {
  if (n <= 0 || num_bins > BVH_MAX_BINS || num_bins < 2) return false;
  BvhGpuWorkspace& ws = bvh_gpu_workspace();
  const bool dbg = getenv("PTX_DBG_BUILD") != nullptr;
  const double t_start = wall_ms();
  bool ok = true;
  auto chk = [&](hipError_t e) { if (e != hipSuccess) ok = false; return e == hipSuccess; };
  const size_t cap[3] = {(size_t)n + 2, (size_t)n / (BVH_SMALL_MAX + 1) + 2, (size_t)n / BVH_BIG_MIN + 2};
  if (!chk(ws.d_order.ensure((size_t)n)) || !chk(ws.d_scratch.ensure((size_t)n * 2)) || !chk(ws.d_counts.ensure(4)) ||
      !chk(ws.d_tmp.ensure((size_t)n * 2 + 2)) || !chk(ws.d_fin.ensure((size_t)n * 2 + 2)) ||
      !chk(ws.d_nodes.ensure((size_t)n * 2 + 2)) || !chk(ws.d_slot.ensure(pad4 ? (size_t)n * 4 : (size_t)n)) ||
      !chk(ws.d_rootenc.ensure(6)))
    return false;
  for (int c = 0; c < 2; ++c)
    for (int k = 0; k < 3; ++k)
      if (!chk(ws.d_seg[c][k].ensure(cap[k]))) return false;
  const int root_cls = n <= BVH_SMALL_MAX ? 0 : (n >= BVH_BIG_MIN ? 2 : 1);
  hipLaunchKernelGGL(k_bvh_iota, grid256(n), dim3(256), 0, nullptr, ws.d_order.p, n);
  if (root) {
    BvhSeg rs;
    rs.lo = 0; rs.hi = n; rs.node = 0; rs.pad = 0;
    rs.box[0] = root->mn.x; rs.box[1] = root->mn.y; rs.box[2] = root->mn.z;
    rs.box[3] = root->mx.x; rs.box[4] = root->mx.y; rs.box[5] = root->mx.z;
    if (!chk(hipMemcpy(ws.d_seg[0][root_cls].p, &rs, sizeof rs, hipMemcpyHostToDevice))) return false;
  } else {
    const unsigned long long init[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    if (!chk(hipMemcpy(ws.d_rootenc.p, init, sizeof init, hipMemcpyHostToDevice))) return false;
    hipLaunchKernelGGL(k_bvh_root_box, dim3((unsigned)std::min(1024, (n + 255) / 256)), dim3(BVH_BLOCK), 0, nullptr, d_boxes, n, ws.d_rootenc.p);
    hipLaunchKernelGGL(k_bvh_root_seg, dim3(1), dim3(1), 0, nullptr, ws.d_rootenc.p, n, ws.d_seg[0][root_cls].p);
  }
  int counts[4] = {0, 0, 0, 1}; /* next level's small / medium / big segments, nodes allocated */
  int n_cls[3] = {0, 0, 0};
  n_cls[root_cls] = 1;
  if (!chk(hipMemcpy(ws.d_counts.p, counts, sizeof counts, hipMemcpyHostToDevice))) return false;
  std::vector<int> level_start; /* temp ids of level l = [level_start[l], level_start[l + 1]) */
  level_start.push_back(0);
  std::vector<BvhSeg> h_big;
  std::vector<BvhBigSeg> h_bigseg;
  std::vector<int2> h_tiles;
  const double t_alloc = wall_ms();
  double t_prev = t_alloc;
  int cur = 0;
  /* small segments: as many waves (segments) per workgroup as fit ~48 KB of bins, so that two workgroups share a CU */
  const int small_waves = (int)std::max<size_t>(1, std::min<size_t>(BVH_SMALL_WAVES, (48 * 1024) / bvh_small_lds_per_wave(num_bins)));
  const size_t small_lds = bvh_small_lds_per_wave(num_bins) * (size_t)small_waves;
  if (small_lds > 64 * 1024) raise_dynamic_lds_limit((const void*)k_bvh_small, (int)(160 * 1024 - 1024)); /* the kernels also hold static words (chunk counters, the floor triangles) */
  for (int level = 0; n_cls[0] + n_cls[1] + n_cls[2] > 0 && level < 4096; ++level) {
    level_start.push_back(counts[3]);
    if (!chk(hipMemsetAsync(ws.d_counts.p, 0, sizeof(int) * 3, nullptr))) break;
    BvhLists lists;
    for (int k = 0; k < 3; ++k) lists.seg[k] = ws.d_seg[1 - cur][k].p;
    lists.count = ws.d_counts.p;
    if (n_cls[0] > 0)
      hipLaunchKernelGGL(k_bvh_small, dim3((unsigned)((n_cls[0] + small_waves - 1) / small_waves)), dim3((unsigned)small_waves * 64), small_lds,
                         nullptr, d_boxes, ws.d_order.p, ws.d_seg[cur][0].p, n_cls[0], lists, ws.d_tmp.p, num_bins, length_cutoff);
    if (n_cls[1] > 0)
      hipLaunchKernelGGL(k_bvh_level, dim3((unsigned)n_cls[1]), dim3(BVH_BLOCK), 0, nullptr, d_boxes, ws.d_order.p, ws.d_scratch.p,
                         ws.d_seg[cur][1].p, n_cls[1], lists, ws.d_tmp.p, n, num_bins, length_cutoff);
    if (n_cls[2] > 0) {
      /* the few big segments: their sizes decide the tile table */
      const int nb = n_cls[2];
      h_big.resize((size_t)nb);
      if (!chk(hipMemcpy(h_big.data(), ws.d_seg[cur][2].p, sizeof(BvhSeg) * (size_t)nb, hipMemcpyDeviceToHost))) break;
      h_bigseg.resize((size_t)nb);
      h_tiles.clear();
      for (int i = 0; i < nb; ++i) {
        BvhBigSeg& bs = h_bigseg[(size_t)i];
        bs.seg = h_big[(size_t)i];
        bs.tile0 = (int)h_tiles.size();
        bs.n_tiles = (bs.seg.hi - bs.seg.lo + BVH_TILE - 1) / BVH_TILE;
        bs.pad0 = bs.pad1 = 0;
        for (int t = 0; t < bs.n_tiles; ++t) h_tiles.push_back(make_int2(i, t));
      }
      const unsigned nt = (unsigned)h_tiles.size();
      if (!chk(ws.d_big.ensure((size_t)nb)) || !chk(ws.d_bigstate.ensure((size_t)nb)) || !chk(ws.d_tiles.ensure(nt)) ||
          !chk(ws.d_tile_cl.ensure(nt)) || !chk(ws.d_tile_cr.ensure(nt)))
        break;
      if (!chk(hipMemcpy(ws.d_big.p, h_bigseg.data(), sizeof(BvhBigSeg) * (size_t)nb, hipMemcpyHostToDevice))) break;
      if (!chk(hipMemcpy(ws.d_tiles.p, h_tiles.data(), sizeof(int2) * nt, hipMemcpyHostToDevice))) break;
      hipLaunchKernelGGL(k_big_init, dim3((unsigned)nb), dim3(BVH_BLOCK), 0, nullptr, ws.d_bigstate.p, nb);
      hipLaunchKernelGGL(k_big_centroid, dim3(nt), dim3(BVH_BLOCK), 0, nullptr, d_boxes, ws.d_order.p, ws.d_big.p, ws.d_tiles.p, ws.d_bigstate.p);
      hipLaunchKernelGGL(k_big_bins, dim3(nt), dim3(BVH_BLOCK), 0, nullptr, d_boxes, ws.d_order.p, ws.d_big.p, ws.d_tiles.p, ws.d_bigstate.p, num_bins);
      hipLaunchKernelGGL(k_big_split, dim3((unsigned)nb), dim3(64), 0, nullptr, ws.d_big.p, nb, ws.d_bigstate.p, lists, ws.d_tmp.p, num_bins, length_cutoff);
      hipLaunchKernelGGL(k_big_count, dim3(nt), dim3(BVH_BLOCK), 0, nullptr, d_boxes, ws.d_order.p, ws.d_big.p, ws.d_tiles.p, ws.d_bigstate.p, ws.d_tile_cl.p, ws.d_tile_cr.p);
      hipLaunchKernelGGL(k_big_offsets, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, nullptr, ws.d_big.p, nb, ws.d_bigstate.p, ws.d_tile_cl.p, ws.d_tile_cr.p);
      hipLaunchKernelGGL(k_big_scatter, dim3(nt), dim3(BVH_BLOCK), 0, nullptr, d_boxes, ws.d_order.p, ws.d_scratch.p, n, ws.d_big.p, ws.d_tiles.p, ws.d_bigstate.p, ws.d_tile_cl.p, ws.d_tile_cr.p);
      hipLaunchKernelGGL(k_big_swap, dim3(nt), dim3(BVH_BLOCK), 0, nullptr, ws.d_order.p, ws.d_scratch.p, n, ws.d_big.p, ws.d_tiles.p, ws.d_bigstate.p);
    }
    if (!chk(hipGetLastError())) break;
    if (!chk(hipMemcpy(counts, ws.d_counts.p, sizeof counts, hipMemcpyDeviceToHost))) break;
    if (dbg) {
      const double now = wall_ms();
      fprintf(stderr, "  level %d: %d small %d medium %d big -> %d %d %d, %.3f ms\n", level, n_cls[0], n_cls[1], n_cls[2], counts[0], counts[1], counts[2], now - t_prev);
      t_prev = now;
    }
    if ((size_t)counts[0] > cap[0] || (size_t)counts[1] > cap[1] || (size_t)counts[2] > cap[2]) { ok = false; break; } /* cannot happen */
    for (int k = 0; k < 3; ++k) n_cls[k] = counts[k];
    cur = 1 - cur;
  }
  if (!ok) return false;
  const double t_levels = wall_ms();
  /* pre-order numbering + leaf slots: subtree sizes bottom-up, indices top-down, one emit pass */
  const int n_tmp = counts[3];
  const int n_levels = (int)level_start.size() - 1;
  level_start.back() = std::min(level_start.back(), n_tmp);
  auto level_count = [&](int l) { return (l + 1 < (int)level_start.size() ? level_start[(size_t)l + 1] : n_tmp) - level_start[(size_t)l]; };
  for (int l = n_levels - 1; l >= 0; --l) {
    const int c = level_count(l);
    if (c > 0) hipLaunchKernelGGL(k_fin_sizes, grid256(c), dim3(256), 0, nullptr, ws.d_tmp.p, ws.d_fin.p, level_start[(size_t)l], c, pad4 ? 1 : 0);
  }
  for (int l = 0; l < n_levels; ++l) {
    const int c = level_count(l);
    if (c > 0) hipLaunchKernelGGL(k_fin_index, grid256(c), dim3(256), 0, nullptr, ws.d_tmp.p, ws.d_fin.p, level_start[(size_t)l], c);
  }
  hipLaunchKernelGGL(k_fin_emit, grid256(n_tmp), dim3(256), 0, nullptr, ws.d_tmp.p, ws.d_fin.p, n_tmp, ws.d_order.p, ws.d_nodes.p, ws.d_slot.p);
  if (!chk(hipGetLastError())) return false;
  BvhFin rootfin;
  if (!chk(hipMemcpy(&rootfin, ws.d_fin.p, sizeof rootfin, hipMemcpyDeviceToHost))) return false;
  if (rootfin.n_nodes != n_tmp) return false; /* cannot happen */
  out->nodes = ws.d_nodes.p;
  out->slot_prim = ws.d_slot.p;
  out->n_nodes = n_tmp;
  out->n_slots = rootfin.n_slots;
  out->depth = rootfin.depth;
  out->leaves = rootfin.n_leaves;
  if (dbg) fprintf(stderr, "bvh_build_device n=%d: alloc %.2f ms, %d levels %.2f ms, finalize %.2f ms\n", n, t_alloc - t_start, n_levels, t_levels - t_alloc, wall_ms() - t_levels);
  return true;
}

/* host boxes in, host BvhResult out (scene creation).
 * The kernels reduce bounds as integers, where -0.0 < +0.0; the host builder's box_union keeps whichever of two equal
 * bounds Float.min / Float.max meet second, so among zeros of both signs its result depends on the slice order.  One
 * of the six bound columns holding both zeros is therefore refused before the device is touched (*mixed_zeros says so)
 * and the caller builds on the host; with one kind of zero per column every order gives the same bits. */
bool bvh_build_gpu(const std::vector<Box>& boxes, int num_bins, int length_cutoff, bool pad4, BvhResult* out, bool* mixed_zeros = nullptr) {
  const int n = (int)boxes.size();
  if (mixed_zeros) *mixed_zeros = false;
  if (n == 0 || num_bins > BVH_MAX_BINS) return false;
  std::vector<double> flat((size_t)n * 6);
  Box root = boxes[0];
  unsigned zeros[6] = {0, 0, 0, 0, 0, 0}; /* per bound column: bit 0 = holds a +0.0, bit 1 = holds a -0.0 */
  for (int i = 0; i < n; ++i) {
    const Box& b = boxes[(size_t)i];
    double* f = &flat[(size_t)i * 6];
    f[0] = b.mn.x; f[1] = b.mn.y; f[2] = b.mn.z; f[3] = b.mx.x; f[4] = b.mx.y; f[5] = b.mx.z;
    for (int k = 0; k < 6; ++k)
      if (f[k] == 0.0) zeros[k] |= std::signbit(f[k]) ? 2u : 1u;
    if (i) root = box_union(root, b); /* shape_tree.ml:257-260 */
  }
  for (int k = 0; k < 6; ++k)
    if (zeros[k] == 3u) {
      if (mixed_zeros) *mixed_zeros = true;
      return false;
    }
  BvhGpuWorkspace& ws = bvh_gpu_workspace();
  if (ws.d_box.ensure(flat.size()) != hipSuccess) return false;
  if (hipMemcpy(ws.d_box.p, flat.data(), sizeof(double) * flat.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
  BvhDeviceTree t;
  if (!bvh_build_device(ws.d_box.p, n, &root, num_bins, length_cutoff, pad4, &t)) return false;
  BvhResult r;
  r.nodes.resize((size_t)t.n_nodes);
  r.slot_prim.resize((size_t)t.n_slots);
  if (hipMemcpy(r.nodes.data(), t.nodes, sizeof(PtNode) * r.nodes.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (t.n_slots > 0 && hipMemcpy(r.slot_prim.data(), t.slot_prim, sizeof(int) * r.slot_prim.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
  r.depth = t.depth;
  r.leaves = t.leaves;
  *out = std::move(r);
  return true;
}

/* a checked, non-default film as the k_film_wide kernels take it */
PtFilmWide film_wide_arg(const ptx_film_params& f) {
  PtFilmWide k{};
  k.r = f.pixel_radius;
  film_weights_1d(f.order, f.pixel_radius, k.w);
  return k;
}
/* PTX_FILM_WIDE=1: the default film runs k_film_wide too (tools/film_cost.py measures it against k_film; same bits) */
bool film_wide_forced() { return env_int("PTX_FILM_WIDE", 0) != 0; }
dim3 film_wide_grid(int width, int rows) { return dim3((unsigned)((width + PT_FILM_TX - 1) / PT_FILM_TX), (unsigned)((rows + PT_FILM_TY - 1) / PT_FILM_TY)); }

/* rows [row0, row1) of the image (reads raw rows row0 - r .. row1 - 1 + r, r = the film's radius); row1 < 0: the whole image.
 * film: checked parameters; the default film runs k_film, every other one k_film_wide */
int film_resolve(int width, int height, int spp, const double* d_raw, double* d_out, hipStream_t st,
                 PtBandMap map = PtBandMap{1, 1, 0}, int row0 = 0, int row1 = -1, const ptx_film_params& film = kFilmDefault) {
  const double spp_inv = 1.0 / (double)spp; /* 1 // samples_per_pixel */
  if (row1 < 0) row1 = height;
  if (!film_is_default(film) || film_wide_forced()) {
    if (row1 <= row0) return 0;
    const PtFilmWide kw = film_wide_arg(film);
    const dim3 grid = film_wide_grid(width, row1 - row0);
    if (film.flags & PTX_FILM_RENORMALISE)
      hipLaunchKernelGGL(k_film_wide<true>, grid, dim3(PT_FILM_TX * PT_FILM_TY), 0, st, d_raw, width, height, spp_inv, kw, map, d_out, row0, row1);
    else
      hipLaunchKernelGGL(k_film_wide<false>, grid, dim3(PT_FILM_TX * PT_FILM_TY), 0, st, d_raw, width, height, spp_inv, kw, map, d_out, row0, row1);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  PtFilm3 k;
  binomial_3x3(k.w);
  const long long n = (long long)width * (row1 - row0);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_film, grid256(n), dim3(256), 0, st, d_raw, width, height, spp_inv, k, map, d_out, row0, row1);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* k_pixel_error (d_passes == nullptr: k passes for every pixel) or k_pixel_error_counts (the pixel's own d_passes[p]), then
 * k_error_summary, queued on st: d_partials holds pixel_error_partials(npix) doubles, the last of them rel_err */
size_t pixel_error_blocks(long long npix) { return (size_t)((npix + PT_ERR_THREADS - 1) / PT_ERR_THREADS); }
size_t pixel_error_partials(long long npix) { return 2 * pixel_error_blocks(npix) + 1; }
int pixel_error_queue(long long npix, int k, const int32_t* d_passes, const double* d_raw, const double* d_sq, double* d_err,
                      double* d_partials, hipStream_t st) {
  const size_t n_blocks = pixel_error_blocks(npix);
  if (d_passes) hipLaunchKernelGGL(k_pixel_error_counts, dim3((unsigned)n_blocks), dim3(PT_ERR_THREADS), 0, st, d_raw, d_sq, d_passes, npix, d_err, d_partials);
  else hipLaunchKernelGGL(k_pixel_error, dim3((unsigned)n_blocks), dim3(PT_ERR_THREADS), 0, st, d_raw, d_sq, npix, k, d_err, d_partials);
  /* (a count map's summary is called with k = 2: a pixel with fewer than 2 passes has se = +inf, which the sums carry) */
  hipLaunchKernelGGL(k_error_summary, dim3(1), dim3(PT_ERR_THREADS), 0, st, (const double*)d_partials, (long long)n_blocks, d_passes ? 2 : k,
                     d_partials + 2 * n_blocks);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* adaptive sampling: k_film_counts queued on st */
int film_counts_queue(int width, int height, const double* d_raw, const int32_t* d_passes, double* d_out, hipStream_t st,
                      const ptx_film_params& film = kFilmDefault) {
  if (!film_is_default(film) || film_wide_forced()) {
    const PtFilmWide kw = film_wide_arg(film);
    const dim3 grid = film_wide_grid(width, height);
    if (film.flags & PTX_FILM_RENORMALISE)
      hipLaunchKernelGGL(k_film_wide_counts<true>, grid, dim3(PT_FILM_TX * PT_FILM_TY), 0, st, d_raw, d_passes, width, height, kw, d_out);
    else
      hipLaunchKernelGGL(k_film_wide_counts<false>, grid, dim3(PT_FILM_TX * PT_FILM_TY), 0, st, d_raw, d_passes, width, height, kw, d_out);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  PtFilm3 k;
  binomial_3x3(k.w);
  const long long n = (long long)width * height;
  hipLaunchKernelGGL(k_film_counts, grid256(n), dim3(256), 0, st, d_raw, d_passes, width, height, k, d_out);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* the sampler's tables hold 256 dimensions: a lens and a shutter together leave room for 125 bounces (2 + 2 * 125 + 2 + 1 = 255);
 * a depth past 126 is check_params' to refuse */
int check_shutter_depth(const ptx_scene* s, const ptx_render_params* p) {
  if (p && s->shutter_on && s->lens_radius > 0.0 && p->max_bounces == 126)
    return fail(PTX_ERR_ARG, "camera shutter: the sampler has 256 dimensions, which is at most 125 bounces with a lens (got max_bounces %d)", p->max_bounces);
  return 0;
}

/* What the render entry points check first, in this order: the scene handle, the depth a lens and a shutter leave (a host-only scene
 * gets this answer too), a device behind it, the caller's other pointers (missing: the message when one of them is NULL, else
 * nullptr), the params */
int check_render_args(const ptx_scene* s, const ptx_render_params* p, const char* missing) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (const int rc = check_shutter_depth(s, p)) return rc;
  if (s->device < 0) return fail(PTX_ERR_STATE, "scene was created host-only (device -1): no CPU fallback exists");
  if (missing) return fail(PTX_ERR_ARG, "%s", missing);
  return check_params(p);
}

int check_device(int32_t device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    (void)hipGetLastError();
    return fail(PTX_ERR_ARG, "device %d out of range (have %d HIP devices): this library has no CPU fallback", device, ndev);
  }
  return 0;
}

/* the second stream and the events of the pipelines that film and copy out behind a queued frame, made once per scene */
int ensure_event(hipEvent_t* ev) {
  if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  return 0;
}
int ensure_copy_stream(ptx_scene* s) {
  if (!s->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
  return 0;
}
/* Every exit of a call that queues a frame and works behind it (render_updates, render_into_pinned): nothing the call queued is
 * still running when it returns (an error half-way may leave lanes that were never joined, and a copy into the caller's image in
 * flight, hence the whole device).  Disarmed once the null stream and copy_stream have been waited for. */
struct DrainOnExit {
  bool armed = true;
  ~DrainOnExit() {
    if (armed) (void)hipDeviceSynchronize();
  }
};

}  // namespace

/* ================================================================== C ABI */
extern "C" {

int32_t ptx_version(void) { return PTX_ABI_VERSION; }
int32_t ptx_leaf_size(void) { return 16; } /* LEAF_SIZE, sphere-intersect-rs/src/lib.rs:13 */
const char* ptx_last_error(void) { return g_last_error.c_str(); }

int32_t ptx_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(PTX_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  return n;
}

int32_t ptx_local_rows(const ptx_render_params* p) { return p ? local_rows(p) : -1; }
int32_t ptx_global_row(const ptx_render_params* p, int32_t r) { return p ? global_row(p, r) : -1; }

/* Copies s->host to the scene's device (the current device) and points s->dev at the copies. */
static int scene_upload(ptx_scene* s) {
  const PtHostArrays& h = *s->host;
  auto up = [](auto& buf, const auto& vec) -> hipError_t {
    hipError_t e = buf.ensure(vec.size());
    if (e != hipSuccess || vec.empty()) return e;
    return hipMemcpy(buf.p, vec.data(), sizeof(vec[0]) * vec.size(), hipMemcpyHostToDevice);
  };
  HIP_TRY(up(s->nodes, h.nodes));
  HIP_TRY(up(s->sph, h.sph));
  const bool any_tri = h.dev.has_triangles != 0;
  if (any_tri) {
    HIP_TRY(up(s->tri, h.tri));
    HIP_TRY(up(s->tri_uv, h.tri_uv));
    HIP_TRY(up(s->tri_frame, h.tri_frame));
  }
  HIP_TRY(up(s->slot_kind, h.kind));
  HIP_TRY(up(s->slot_cat, h.cat));
  HIP_TRY(up(s->slot_material, h.slot_mat));
  HIP_TRY(up(s->slot_prim, h.slot_prim));
  HIP_TRY(up(s->materials, h.mats));
  HIP_TRY(up(s->textures, h.texs));
  HIP_TRY(up(s->slot_shade, h.shade));
  HIP_TRY(up(s->node_skip, h.skip));
  HIP_TRY(up(s->node_skip32, h.skip32));
  HIP_TRY(up(s->nodes32, h.nodes32));
  HIP_TRY(up(s->nodes32o, h.nodes32o));
  HIP_TRY(up(s->lds_oct, h.lds_oct));
  HIP_TRY(up(s->top_nodes, h.top_nodes));
  HIP_TRY(up(s->node_skip32_top, h.skip32_top));
  PtSceneDev& dv = s->dev;
  dv = h.dev;
  dv.nodes = s->nodes.p;
  dv.sph = s->sph.p; dv.tri = any_tri ? s->tri.p : nullptr; dv.tri_uv = any_tri ? s->tri_uv.p : nullptr;
  dv.tri_frame = (any_tri && !h.tri_frame.empty()) ? s->tri_frame.p : nullptr;
  dv.slot_kind = s->slot_kind.p; dv.slot_cat = s->slot_cat.p; dv.slot_material = s->slot_material.p; dv.slot_prim = s->slot_prim.p;
  dv.materials = s->materials.p; dv.textures = s->textures.p; dv.slot_shade = s->slot_shade.p;
  dv.node_skip = h.skip.empty() ? nullptr : s->node_skip.p;
  dv.node_skip32 = s->node_skip32.p;
  dv.nodes32 = s->nodes32.p;
  dv.nodes32o = h.nodes32o.empty() ? nullptr : s->nodes32o.p;
  dv.lds_oct = h.lds_oct.empty() ? nullptr : s->lds_oct.p;
  dv.top_nodes = h.top_nodes.empty() ? nullptr : s->top_nodes.p;
  dv.node_skip32_top = h.skip32_top.empty() ? nullptr : s->node_skip32_top.p;
  dv.n_top = (int32_t)(h.top_nodes.size() / 16);
  /* lds_nodes64 is decided once, here, by the schedule of the image without them; the schedule the scene leaves with counts them in */
  dv.lds_nodes64 = 0;
  reschedule(s, s->sets_in_flight);
  if (s->sched.in_lds() && env_int("PTX_LDS_NODES64", 1)) {
    dv.lds_nodes64 = pt_lds_keep_nodes64(lds_in(s, PT_LDS_K_TRACE, s->sched.trace_threads / 64), s->sched.bounce_threads / 64);
    reschedule(s, s->sets_in_flight);
  }
  return 0;
}

/* descriptor -> boxes -> tree -> host arrays (scene_host.cpp) -> upload; a host-only scene stops after the tree */
static int scene_build(ptx_scene* s, const ptx_scene_desc* d) {
  const double t0 = wall_ms();
  std::string msg;
  if (const int rc = scene_check_desc(d, &msg)) return fail(rc, "%s", msg.c_str());
  const std::vector<Box> boxes = scene_boxes(d);
  const int n = (int)boxes.size(), num_bins = scene_num_bins(d);
  const bool simd = d->leaf_kind == PTX_LEAF_SIMD;
  /* builder: desc->reserved 0 = auto (GPU for large scenes on a device, host otherwise), 1 = host, 2 = GPU */
  BvhResult tree;
  bool built = false;
  const bool want_gpu = s->device >= 0 && (d->reserved == 2 || (d->reserved == 0 && n >= 4096)) && num_bins <= BVH_MAX_BINS;
  if (d->reserved == 2 && !want_gpu) return fail(PTX_ERR_ARG, "GPU BVH build requested but unavailable (host-only scene or num_bins > %d)", BVH_MAX_BINS);
  if (want_gpu) {
    bool mixed_zeros = false;
    built = bvh_build_gpu(boxes, num_bins, d->length_cutoff, simd, &tree, &mixed_zeros);
    if (mixed_zeros && d->reserved == 2)
      return fail(PTX_ERR_ARG, "GPU BVH build requested but unavailable (a bound of the primitives' boxes is +0.0 and -0.0 among them: "
                               "the host builder's result depends on their order)");
    if (!built && d->reserved == 2) return fail(PTX_ERR_HIP, "GPU BVH build failed: %s", hipGetErrorString(hipGetLastError()));
  }
  if (!built) tree = bvh_build(boxes, num_bins, d->length_cutoff, simd);
  s->built_on_gpu = built;
  s->n_prims = n;
  s->own_view = d->camera;
  s->tree_depth = tree.depth;
  s->tree_leaves = tree.leaves;
  auto ha = std::make_shared<PtHostArrays>();
  if (const int rc = scene_set_tree(d, std::move(tree), ha.get(), &msg)) return fail(rc, "%s", msg.c_str());
  s->host = ha;
  s->tile_cache = std::make_shared<TileListCache>();
  int rc = 0;
  if (s->device < 0) {
    s->dev.n_slots = ha->dev.n_slots;
    s->dev.n_nodes = ha->dev.n_nodes;
  } else {
    scene_assemble(d, boxes, scene_options_from_env(), ha.get());
    rc = scene_upload(s);
  }
  s->build_ms = wall_ms() - t0;
  return rc;
}

ptx_scene* ptx_scene_create(const ptx_scene_desc* desc, int32_t device) {
  if (!desc) {
    fail(PTX_ERR_ARG, "desc is NULL");
    return nullptr;
  }
  if (device == -1) {
    /* host-only scene: BVH built and flattened for inspection (ptx_scene_tree / ptx_scene_stats);
     * nothing is uploaded and every compute entry point refuses it */
    ptx_scene* hs = new ptx_scene();
    hs->device = -1;
    if (scene_build(hs, desc) != 0) {
      delete hs;
      return nullptr;
    }
    return hs;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    fail(PTX_ERR_HIP, "no HIP device available (%s): this library has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= ndev) {
    fail(PTX_ERR_ARG, "device %d out of range (have %d)", device, ndev);
    return nullptr;
  }
  if ((e = hipSetDevice(device)) != hipSuccess) {
    fail(PTX_ERR_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
    return nullptr;
  }
  ptx_scene* s = new ptx_scene();
  s->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
  if (scene_build(s, desc) != 0) {
    ptx_scene_destroy(s);
    return nullptr;
  }
  return s;
}

int32_t ptx_image_unpin(ptx_scene* s) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (s->reg_ptr) {
    (void)hipSetDevice(s->device);
    (void)hipHostUnregister(s->reg_ptr);
    (void)hipGetLastError();
    s->reg_ptr = nullptr;
    s->reg_bytes = 0;
  }
  return 0;
}

int32_t ptx_image_pin_bytes(ptx_scene* s, void* image, int64_t n_bytes) {
  if (!s || !image || n_bytes <= 0) return fail(PTX_ERR_ARG, "NULL argument or empty image");
  if (s->device < 0) return fail(PTX_ERR_STATE, "scene was created host-only (device -1)");
  (void)ptx_image_unpin(s);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipHostRegister(image, (size_t)n_bytes, hipHostRegisterDefault));
  s->reg_ptr = (char*)image;
  s->reg_bytes = (size_t)n_bytes;
  return 0;
}

int32_t ptx_image_pin(ptx_scene* s, double* image, int64_t n_doubles) {
  if (n_doubles > (int64_t)(INT64_MAX / sizeof(double))) return fail(PTX_ERR_ARG, "n_doubles %lld is out of range", (long long)n_doubles);
  return ptx_image_pin_bytes(s, image, n_doubles > 0 ? n_doubles * (int64_t)sizeof(double) : 0);
}

void ptx_scene_destroy(ptx_scene* s) {
  if (!s) return;
  if (s->device < 0) {
    delete s;
    return;
  }
  for (ptx_scene* r : s->replicas) ptx_scene_destroy(r);
  s->replicas.clear();
  (void)hipSetDevice(s->device);
  if (s->pinned) (void)hipHostFree(s->pinned);
  s->pinned = nullptr;
  (void)ptx_image_unpin(s);
  if (s->built_on_gpu) ptx_release_workspaces(); /* the GPU builder's thread-local buffers (largest build so far) */
  for (auto& t : s->alpha_tables) (void)hipFree(t.second);
  s->alpha_tables.clear();
  s->alpha.p = nullptr;
  /* every DevBuf member (scene arrays, workspaces, gather / raw / rgb) frees itself when the handle is deleted below */
  for (int k = 0; k < kMaxSets; ++k) {
    if (s->streams[k]) (void)hipStreamDestroy(s->streams[k]);
    if (s->ev_accum[k]) (void)hipEventDestroy(s->ev_accum[k]);
    if (s->ev_join[k]) (void)hipEventDestroy(s->ev_join[k]);
  }
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->ev_update) (void)hipEventDestroy(s->ev_update);
  if (s->ev_select) (void)hipEventDestroy(s->ev_select);
  if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
  for (hipEvent_t ev : s->ev_slab)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : s->event_pool) (void)hipEventDestroy(ev);
  delete s;
}

/* The one place that writes what the kernels read of the lighting state -- PtSceneDev.lighting, the light table, env_sample and the
 * density, has_emit -- from the handle's own (lighting, light_table, env_sampling, env_density), then reschedules.  A scene in mode 2
 * with environment sampling on is a lit scene whether or not anything in it emits: has_emit = 1 gives it the queue's emission record
 * (which stays zero without emitters), and Schedule::lit and every size taken from has_emit follow from the same field. */
static void apply_lighting(ptx_scene* s) {
  if (s->device < 0) return;
  const int mode = s->lighting;
  const bool sampled = mode == PTX_LIGHTING_SAMPLED, env_on = s->env_sampling && s->env_density && s->env.dev.p;
  s->dev.has_emit = (s->host->dev.has_emit || (sampled && env_on)) ? 1 : 0;
  /* the mode in effect: without emitters there is no emission to order, and mode 1 is mode 0 */
  s->dev.lighting = s->dev.has_emit ? mode : PTX_LIGHTING_REFERENCE;
  const bool lights = sampled && !s->light_table.empty();
  s->dev.lights = lights ? s->d_lights.p : nullptr;
  s->dev.n_lights = lights ? s->host->n_emissive_tris : 0;
  s->dev.light_area = lights ? s->light_table[s->light_table.size() - PT_LIGHT_DOUBLES + PT_LIGHT_CUM] : 0.0;
  const bool spheres = sampled && s->sphere_sampling && !s->sphere_table.empty();
  s->dev.n_sphere_lights = spheres ? (int32_t)(s->sphere_table.size() / PT_SLIGHT_DOUBLES) : 0; /* (0 is pad_f's 0.0f) */
  if (spheres) { /* the joined table: the triangles' records again, the spheres' behind them */
    s->dev.lights = s->d_joined_lights.p;
    s->dev.n_lights = s->host->n_emissive_tris >= 1 && s->host->n_emissive_tris <= PTX_MAX_LIGHT_TRIANGLES ? s->host->n_emissive_tris : 0;
    s->dev.light_area = s->sphere_table[s->sphere_table.size() - PT_SLIGHT_DOUBLES + PT_SLIGHT_CUM]; /* W_total */
  }
  s->dev.env_sample = env_on ? 1 : 0;
  reschedule(s, s->sets_in_flight); /* (Schedule::lit, and what follows from it) */
}

int32_t ptx_scene_set_lighting(ptx_scene* s, int32_t mode) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (mode != PTX_LIGHTING_REFERENCE && mode != PTX_LIGHTING_PATH_ORDER && mode != PTX_LIGHTING_SAMPLED) return fail(PTX_ERR_ARG, "unknown lighting mode %d", mode);
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the lighting mode cannot change while a render runs on the scene");
  if (mode == PTX_LIGHTING_SAMPLED) {
    if (s->host->n_emissive_tris == 0 && !s->env_sampling && !s->sphere_sampling) return fail(PTX_ERR_ARG, "sampled lighting needs an emissive triangle in the tree (emissive spheres and floor triangles are not sampled)");
    if (s->host->n_emissive_tris > PTX_MAX_LIGHT_TRIANGLES) return fail(PTX_ERR_ARG, "%d emissive tree triangles, more than PTX_MAX_LIGHT_TRIANGLES = %d (no light hierarchy)", s->host->n_emissive_tris, PTX_MAX_LIGHT_TRIANGLES);
    if (s->light_table.empty()) s->light_table = light_table_build(*s->host);
    if (s->device >= 0 && !s->d_lights.p && !s->light_table.empty()) {
      HIP_TRY(hipSetDevice(s->device));
      HIP_TRY(s->d_lights.ensure(s->light_table.size()));
      HIP_TRY(hipMemcpy(s->d_lights.p, s->light_table.data(), sizeof(double) * s->light_table.size(), hipMemcpyHostToDevice));
    }
  }
  s->lighting = mode;
  apply_lighting(s);
  for (ptx_scene* r : s->replicas) {
    const int rc = ptx_scene_set_lighting(r, mode);
    if (rc) return rc;
  }
  return 0;
}

/* the records the sphere lights' running sums continue: the triangles' as light_table_build gives them, none for a scene whose
 * triangles mode 2 would not take */
static std::vector<double> light_triangle_records(const ptx_scene* s) {
  if (s->host->n_emissive_tris < 1 || s->host->n_emissive_tris > PTX_MAX_LIGHT_TRIANGLES) return {};
  return s->light_table.empty() ? light_table_build(*s->host) : s->light_table;
}
/* one scene takes the flag: everything that can fail comes before anything changes */
static int take_sphere_sampling(ptx_scene* s, bool on) {
  if (on && s->sphere_table.empty()) {
    std::vector<double> joined = light_triangle_records(s);
    std::vector<double> table = sphere_light_table_build(*s->host, joined.empty() ? 0.0 : joined[joined.size() - PT_LIGHT_DOUBLES + PT_LIGHT_CUM]);
    if (s->device >= 0) {
      joined.insert(joined.end(), table.begin(), table.end());
      HIP_TRY(hipSetDevice(s->device));
      HIP_TRY(s->d_joined_lights.ensure(joined.size()));
      HIP_TRY(hipMemcpy(s->d_joined_lights.p, joined.data(), sizeof(double) * joined.size(), hipMemcpyHostToDevice));
    }
    s->sphere_table = std::move(table);
  }
  s->sphere_sampling = on;
  apply_lighting(s);
  return 0;
}

int32_t ptx_scene_set_sphere_light_sampling(ptx_scene* s, int32_t on) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "sphere light sampling cannot change while a render runs on the scene");
  if (on) {
    const int n = s->host->n_emissive_spheres;
    if (n == 0) return fail(PTX_ERR_ARG, "sphere light sampling needs an emissive sphere in the tree: the scene has 0");
    if (n > PTX_MAX_LIGHT_SPHERES) return fail(PTX_ERR_ARG, "%d emissive tree spheres, more than PTX_MAX_LIGHT_SPHERES = %d (no light hierarchy)", n, PTX_MAX_LIGHT_SPHERES);
  } else {
    if (!s->sphere_sampling) return 0;
    if (s->lighting == PTX_LIGHTING_SAMPLED && s->host->n_emissive_tris == 0 && !s->env_sampling)
      return fail(PTX_ERR_STATE, "sampled lighting has nothing but the sphere lights to sample: set another lighting mode first");
  }
  if (const int rc = take_sphere_sampling(s, on != 0)) return rc;
  for (ptx_scene* r : s->replicas)
    if (const int rc = take_sphere_sampling(r, on != 0)) return rc;
  return 0;
}

int32_t ptx_scene_sphere_lights(const ptx_scene* s, int32_t* on_out, int32_t* n_out, double* weight_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  const bool on = s->sphere_sampling && !s->sphere_table.empty();
  if (on_out) *on_out = s->sphere_sampling ? 1 : 0;
  if (n_out) *n_out = on ? (int32_t)(s->sphere_table.size() / PT_SLIGHT_DOUBLES) : 0;
  if (weight_out) *weight_out = on ? s->sphere_table[s->sphere_table.size() - PT_SLIGHT_DOUBLES + PT_SLIGHT_CUM] : 0.0;
  return 0;
}

int32_t ptx_light_table(const ptx_scene* s, double* triangles_out, double* spheres_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (triangles_out && !s->light_table.empty()) std::memcpy(triangles_out, s->light_table.data(), sizeof(double) * s->light_table.size());
  if (spheres_out && s->sphere_sampling && !s->sphere_table.empty())
    std::memcpy(spheres_out, s->sphere_table.data(), sizeof(double) * s->sphere_table.size());
  return 0;
}

int32_t ptx_scene_lighting(const ptx_scene* s, int32_t* mode_out, int32_t* n_light_triangles_out, double* light_area_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (mode_out) *mode_out = s->lighting;
  /* the light list exists once mode 2 has been set */
  if (n_light_triangles_out) *n_light_triangles_out = (int32_t)(s->light_table.size() / PT_LIGHT_DOUBLES);
  if (light_area_out) *light_area_out = s->light_table.empty() ? 0.0 : s->light_table[s->light_table.size() - PT_LIGHT_DOUBLES + PT_LIGHT_CUM];
  return 0;
}

int32_t ptx_film_defaults(ptx_film_params* out) {
  if (!out) return fail(PTX_ERR_ARG, "NULL argument");
  *out = kFilmDefault;
  return 0;
}

int32_t ptx_film_weights(const ptx_film_params* film, double* w1d_out, double* w2d_out) {
  if (!film || !w1d_out) return fail(PTX_ERR_ARG, "NULL argument");
  const int rc = film_check(film);
  if (rc) return rc;
  const int f_width = 2 * film->pixel_radius + 1;
  double w[2 * PTX_FILM_MAX_RADIUS + 1];
  film_weights_1d(film->order, film->pixel_radius, w);
  for (int i = 0; i < f_width; ++i) w1d_out[i] = w[i];
  if (w2d_out)
    for (int j = 0; j < f_width * f_width; ++j) w2d_out[j] = w[j / f_width] * w[j % f_width]; /* outer_product, :40-47 */
  return 0;
}

int32_t ptx_scene_set_film(ptx_scene* s, const ptx_film_params* film) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  const ptx_film_params f = film ? *film : kFilmDefault;
  int rc = film_check(&f);
  if (rc) return rc;
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the film cannot change while a render runs on the scene");
  s->film = f;
  for (ptx_scene* r : s->replicas) {
    rc = ptx_scene_set_film(r, &f);
    if (rc) return rc;
  }
  return 0;
}

int32_t ptx_scene_film(const ptx_scene* s, ptx_film_params* out) {
  if (!s || !out) return fail(PTX_ERR_ARG, "NULL argument");
  *out = s->film;
  return 0;
}

int32_t ptx_scene_set_lens(ptx_scene* s, double radius, double focus_distance) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (!std::isfinite(radius) || !(radius >= 0.0)) return fail(PTX_ERR_ARG, "lens: radius must be finite and >= 0 (got %g); 0 switches the lens off", radius);
  if (!std::isfinite(focus_distance) || !(focus_distance > 0.0)) return fail(PTX_ERR_ARG, "lens: focus_distance must be finite and > 0 (got %g)", focus_distance);
  if (radius > 0.0 && s->projection == PTX_PROJECTION_LATLONG)
    return fail(PTX_ERR_STATE, "lens: the lat-long projection has no lens: ptx_scene_set_camera_projection(scene, PTX_PROJECTION_PERSPECTIVE) first");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the lens cannot change while a render runs on the scene");
  s->lens_radius = radius;
  s->lens_focus = focus_distance;
  if (s->device >= 0) reschedule(s, s->sets_in_flight); /* (Schedule::lens, and what follows from it) */
  for (ptx_scene* r : s->replicas) {
    const int rc = ptx_scene_set_lens(r, radius, focus_distance);
    if (rc) return rc;
  }
  return 0;
}

int32_t ptx_scene_lens(const ptx_scene* s, double* radius_out, double* focus_distance_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (radius_out) *radius_out = s->lens_radius;
  if (focus_distance_out) *focus_distance_out = s->lens_focus;
  return 0;
}

/* ---- camera projection ---- */
int32_t ptx_scene_set_camera_projection(ptx_scene* s, int32_t projection) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (projection != PTX_PROJECTION_PERSPECTIVE && projection != PTX_PROJECTION_LATLONG)
    return fail(PTX_ERR_ARG, "camera projection: %d is neither PTX_PROJECTION_PERSPECTIVE (0) nor PTX_PROJECTION_LATLONG (1)", projection);
  if (projection == PTX_PROJECTION_LATLONG && s->lens_radius > 0.0)
    return fail(PTX_ERR_STATE, "camera projection: the lat-long projection has no lens: switch the lens off with ptx_scene_set_lens(scene, 0, 1) first");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the camera projection cannot change while a render runs on the scene");
  s->projection = projection;
  if (s->device >= 0) reschedule(s, s->sets_in_flight); /* (Schedule::latlong and ::pose, and what follows from them) */
  for (ptx_scene* r : s->replicas) {
    const int rr = ptx_scene_set_camera_projection(r, projection);
    if (rr) return rr;
  }
  return 0;
}

int32_t ptx_scene_camera_projection(const ptx_scene* s) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  return s->projection;
}

/* ---- camera pose ---- */
namespace {
const double kPoseIdentity[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
/* the setter's conditions on (origin, rotation, view); each refusal names its rule */
int check_camera_pose(const double* origin, const double* R, const ptx_camera* view) {
  if ((origin == nullptr) != (R == nullptr))
    return fail(PTX_ERR_ARG, "camera pose: origin and rotation are given together or not at all (%s is NULL)", origin ? "rotation" : "origin");
  if (origin) {
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(origin[i])) return fail(PTX_ERR_ARG, "camera pose: origin must be finite (component %d is %g)", i, origin[i]);
    for (int i = 0; i < 9; ++i)
      if (!std::isfinite(R[i])) return fail(PTX_ERR_ARG, "camera pose: rotation must be finite (entry %d is %g)", i, R[i]);
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double g = (R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2];
        worst = std::max(worst, std::fabs(g - (i == j ? 1.0 : 0.0)));
      }
    if (!(worst <= 1e-9)) return fail(PTX_ERR_ARG, "camera pose: rotation must be orthonormal: max |R R^T - I| = %g exceeds 1e-9", worst);
    const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(det > 0.0)) return fail(PTX_ERR_ARG, "camera pose: rotation must have det R > 0 (got %g): a reflection is not a rotation", det);
  }
  /* ptx_scene_create reads the descriptor's camera as it is; a view given here must at least be finite */
  if (view && !(std::isfinite(view->lower_left_x) && std::isfinite(view->lower_left_y) && std::isfinite(view->view_x) && std::isfinite(view->view_y)))
    return fail(PTX_ERR_ARG, "camera pose: view must be finite (got lower_left %g, %g, view %g, %g)", view->lower_left_x, view->lower_left_y, view->view_x, view->view_y);
  return 0;
}
bool same_camera_pose(const ptx_scene* a, const ptx_scene* b) {
  if (a->pose_on != b->pose_on) return false;
  if (!a->pose_on) return true;
  if (std::memcmp(a->pose_origin, b->pose_origin, sizeof a->pose_origin) || std::memcmp(a->pose_rotation, b->pose_rotation, sizeof a->pose_rotation)) return false;
  if (a->pose_has_view != b->pose_has_view) return false;
  return !a->pose_has_view || std::memcmp(&a->pose_view, &b->pose_view, sizeof a->pose_view) == 0;
}
void copy_camera_pose(ptx_scene* dst, const ptx_scene* src) {
  dst->pose_on = src->pose_on;
  dst->pose_has_view = src->pose_has_view;
  std::memcpy(dst->pose_origin, src->pose_origin, sizeof dst->pose_origin);
  std::memcpy(dst->pose_rotation, src->pose_rotation, sizeof dst->pose_rotation);
  dst->pose_view = src->pose_view;
}
}  // namespace

int32_t ptx_scene_set_camera_pose(ptx_scene* s, const double origin[3], const double rotation[9], const ptx_camera* view) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  const int rc = check_camera_pose(origin, rotation, view);
  if (rc) return rc;
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the camera pose cannot change while a render runs on the scene");
  s->pose_on = origin || view;
  s->pose_has_view = view != nullptr;
  for (int i = 0; i < 3; ++i) s->pose_origin[i] = origin ? origin[i] : 0.0;
  std::memcpy(s->pose_rotation, rotation ? rotation : kPoseIdentity, sizeof s->pose_rotation);
  s->pose_view = view ? *view : ptx_camera{0.0, 0.0, 0.0, 0.0};
  if (s->device >= 0) reschedule(s, s->sets_in_flight); /* (Schedule::pose, and what follows from it) */
  for (ptx_scene* r : s->replicas) {
    const int rr = ptx_scene_set_camera_pose(r, origin, rotation, view);
    if (rr) return rr;
  }
  return 0;
}

int32_t ptx_scene_camera_pose(const ptx_scene* s, double origin_out[3], double rotation_out[9], ptx_camera* view_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (origin_out) std::memcpy(origin_out, s->pose_origin, sizeof s->pose_origin);
  if (rotation_out) std::memcpy(rotation_out, s->pose_rotation, sizeof s->pose_rotation);
  if (view_out) *view_out = s->pose_has_view ? s->pose_view : s->own_view;
  return s->pose_on ? 1 : 0;
}

/* ---- camera shutter ---- */
namespace {
bool same_camera_shutter(const ptx_scene* a, const ptx_scene* b) {
  if (a->shutter_on != b->shutter_on) return false;
  return !a->shutter_on || (std::memcmp(a->shutter_translation, b->shutter_translation, sizeof a->shutter_translation) == 0 &&
                            std::memcmp(a->shutter_axis, b->shutter_axis, sizeof a->shutter_axis) == 0 &&
                            std::memcmp(&a->shutter_angle, &b->shutter_angle, sizeof a->shutter_angle) == 0);
}
void copy_camera_shutter(ptx_scene* dst, const ptx_scene* src) {
  dst->shutter_on = src->shutter_on;
  std::memcpy(dst->shutter_translation, src->shutter_translation, sizeof dst->shutter_translation);
  std::memcpy(dst->shutter_axis, src->shutter_axis, sizeof dst->shutter_axis);
  dst->shutter_angle = src->shutter_angle;
}
}  // namespace

int32_t ptx_scene_set_camera_shutter(ptx_scene* s, const double translation[3], const double axis[3], double angle) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if ((translation == nullptr) != (axis == nullptr))
    return fail(PTX_ERR_ARG, "camera shutter: translation and axis are given together or not at all (%s is NULL)", translation ? "axis" : "translation");
  if (!std::isfinite(angle)) return fail(PTX_ERR_ARG, "camera shutter: angle must be finite (got %g)", angle);
  if (!translation && angle != 0.0)
    return fail(PTX_ERR_ARG, "camera shutter: translation and axis are given together with an angle (both are NULL, angle is %g); NULL, NULL, 0 switches the shutter off", angle);
  if (translation) {
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(translation[i])) return fail(PTX_ERR_ARG, "camera shutter: translation must be finite (component %d is %g)", i, translation[i]);
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(axis[i])) return fail(PTX_ERR_ARG, "camera shutter: axis must be finite (component %d is %g)", i, axis[i]);
    const double pi = 3.14159265358979323846;
    if (!(std::fabs(angle) <= pi)) return fail(PTX_ERR_ARG, "camera shutter: |angle| must be at most pi (got %g)", angle);
    const double len = std::sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    if (angle != 0.0 && !(std::fabs(len - 1.0) <= 1e-9))
      return fail(PTX_ERR_ARG, "camera shutter: axis must be a unit vector while angle != 0: | |axis| - 1 | = %g exceeds 1e-9", std::fabs(len - 1.0));
  }
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the camera shutter cannot change while a render runs on the scene");
  s->shutter_on = translation != nullptr;
  for (int i = 0; i < 3; ++i) {
    s->shutter_translation[i] = translation ? translation[i] : 0.0;
    s->shutter_axis[i] = axis ? axis[i] : 0.0;
  }
  s->shutter_angle = translation ? angle : 0.0;
  if (s->device >= 0) reschedule(s, s->sets_in_flight); /* (Schedule::shutter and ::pose, and what follows from them) */
  for (ptx_scene* r : s->replicas) {
    const int rr = ptx_scene_set_camera_shutter(r, translation, axis, angle);
    if (rr) return rr;
  }
  return 0;
}

int32_t ptx_scene_camera_shutter(const ptx_scene* s, double translation_out[3], double axis_out[3], double* angle_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (translation_out) std::memcpy(translation_out, s->shutter_translation, sizeof s->shutter_translation);
  if (axis_out) std::memcpy(axis_out, s->shutter_axis, sizeof s->shutter_axis);
  if (angle_out) *angle_out = s->shutter_angle;
  return s->shutter_on ? 1 : 0;
}

/* ---- image textures and the environment ---- */
/* A setter changes a scene and its replicas together or not at all: everything that can fail -- the uploads of the texels and of
 * the slot categories and shading records made of them -- goes into fresh buffers first, for every scene (stage); only when all of
 * them stand are the buffers swapped in (commit: moves and assignments, nothing that fails).  The caller has checked the arguments. */
struct ImageStage {
  using Host = std::shared_ptr<const ptx_scene::ImageHost>;
  ptx_scene* s = nullptr;
  DevBuf<double> texels;
  DevBuf<uint8_t> cat;
  DevBuf<PtShadeRec> shade;
  int n_images = 0;
};
using EnvDensityRef = std::shared_ptr<const PtEnvDensity>;
/* the density of an environment under a matrix, or why it has none */
static int env_density_make(const ptx_scene::ImageHost& host, const double* rot, EnvDensityRef* out) {
  std::string msg;
  int rc = scene_check_env_rotation(rot, &msg);
  if (rc) return fail(rc, "%s", msg.c_str());
  auto d = std::make_shared<PtEnvDensity>();
  if ((rc = scene_env_density(host.rec.data(), host.width, host.height, d.get(), &msg)) != 0) return fail(rc, "%s", msg.c_str());
  *out = d;
  return 0;
}
/* density (an environment that is sampled only): its table goes behind the texels, in the same buffer (pt_scene.h, PT_ENVD_*) */
static int stage_texels(ptx_scene* s, const ImageStage::Host& host, ImageStage* st, const PtEnvDensity* density = nullptr) {
  st->s = s;
  if (s->device < 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize()); /* frames queued with PTX_RENDER_ASYNC still read the buffers the commit replaces */
  if (host) {
    HIP_TRY(st->texels.ensure(host->rec.size() + (density ? density->table.size() : 0)));
    HIP_TRY(hipMemcpy(st->texels.p, host->rec.data(), sizeof(double) * host->rec.size(), hipMemcpyHostToDevice));
    if (density)
      HIP_TRY(hipMemcpy(st->texels.p + host->rec.size(), density->table.data(), sizeof(double) * density->table.size(), hipMemcpyHostToDevice));
  }
  return 0;
}
/* the image for entry `index` of one scene's texture table (host == nullptr: none), and the slot categories and shading records with
 * every image in place (scene_image_overrides) */
static int stage_texture_image(ptx_scene* s, int32_t index, const ImageStage::Host& host, ImageStage* st) {
  const int rc = stage_texels(s, host, st);
  if (rc || s->device < 0) return rc;
  std::vector<PtImageEntry> entries((size_t)s->host->n_textures);
  for (size_t i = 0; i < entries.size(); ++i) {
    const bool mine = i == (size_t)index;
    const ptx_scene::ImageHost* h = mine ? host.get() : (s->images.empty() ? nullptr : s->images[i]->host.get());
    if (!h) continue;
    entries[i].width = h->width;
    entries[i].height = h->height;
    entries[i].flags = h->flags;
    entries[i].texels = (uint64_t)(uintptr_t)(mine ? st->texels.p : s->images[i]->dev.p);
    ++st->n_images;
  }
  if (st->n_images) {
    std::vector<uint8_t> cat;
    std::vector<PtShadeRec> shade;
    scene_image_overrides(*s->host, entries, &cat, &shade);
    HIP_TRY(st->cat.ensure(cat.size()));
    HIP_TRY(st->shade.ensure(shade.size()));
    HIP_TRY(hipMemcpy(st->cat.p, cat.data(), cat.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st->shade.p, shade.data(), sizeof(PtShadeRec) * shade.size(), hipMemcpyHostToDevice));
  }
  return 0;
}
static void commit_texture_image(ImageStage* st, int32_t index, const ImageStage::Host& host) {
  ptx_scene* s = st->s;
  if (s->images.empty()) {
    s->images.resize((size_t)s->host->n_textures);
    for (auto& e : s->images) e = std::make_unique<ptx_scene::ImageSlot>();
  }
  if (s->device >= 0) (void)hipSetDevice(s->device); /* (the buffers the moves below release are this device's) */
  ptx_scene::ImageSlot& slot = *s->images[(size_t)index];
  slot.dev = std::move(st->texels);
  slot.host = host;
  if (s->device < 0) return;
  s->slot_cat_img = std::move(st->cat);
  s->slot_shade_img = std::move(st->shade);
  s->dev.n_images = st->n_images;
  s->dev.slot_cat = st->n_images ? s->slot_cat_img.p : s->slot_cat.p;
  s->dev.slot_shade = st->n_images ? s->slot_shade_img.p : s->slot_shade.p;
  reschedule(s, s->sets_in_flight); /* (Schedule::img, and what follows from it) */
}
static void commit_environment(ImageStage* st, const ImageStage::Host& host, const double* rot) {
  ptx_scene* s = st->s;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  s->env.dev = std::move(st->texels);
  s->env.host = host;
  std::memcpy(s->env_rot, rot, sizeof s->env_rot);
  if (s->device < 0) return;
  const ptx_scene::ImageHost* e = host.get();
  s->dev.env = e ? s->env.dev.p : nullptr;
  s->dev.env_w = e ? e->width : 0;
  s->dev.env_h = e ? e->height : 0;
  s->dev.env_flags = e ? e->flags : 0;
  std::memcpy(s->dev.env_rot, s->env_rot, sizeof s->env_rot);
  s->dev.bg_kind = e ? PT_BG_ENV : s->host->dev.bg_kind;
  reschedule(s, s->sets_in_flight);
}
/* the scene, then its replicas */
static std::vector<ptx_scene*> scene_family(ptx_scene* s) {
  std::vector<ptx_scene*> all{s};
  all.insert(all.end(), s->replicas.begin(), s->replicas.end());
  return all;
}
static int family_take_texture_image(const std::vector<ptx_scene*>& all, int32_t index, const ImageStage::Host& host) {
  std::vector<ImageStage> stages(all.size());
  for (size_t k = 0; k < all.size(); ++k)
    if (const int rc = stage_texture_image(all[k], index, host, &stages[k])) return rc; /* nothing has changed yet */
  for (ImageStage& st : stages) commit_texture_image(&st, index, host);
  return 0;
}
/* density: the new environment's, where the family samples it (the flag stays as it is) */
static int family_take_environment(const std::vector<ptx_scene*>& all, const ImageStage::Host& host, const double* rot,
                                   const EnvDensityRef& density = nullptr) {
  std::vector<ImageStage> stages(all.size());
  for (size_t k = 0; k < all.size(); ++k)
    if (const int rc = stage_texels(all[k], host, &stages[k], density.get())) return rc;
  for (ImageStage& st : stages) {
    st.s->env_density = density;
    commit_environment(&st, host, rot);
    apply_lighting(st.s);
  }
  return 0;
}
/* the environment's texels again, with (on) or without the density table behind them */
static int family_take_env_sampling(const std::vector<ptx_scene*>& all, bool on, const EnvDensityRef& density) {
  std::vector<ImageStage> stages(all.size());
  for (size_t k = 0; k < all.size(); ++k)
    if (const int rc = stage_texels(all[k], all[k]->env.host, &stages[k], density.get())) return rc;
  for (ImageStage& st : stages) {
    ptx_scene* s = st.s;
    s->env_sampling = on;
    s->env_density = density;
    if (s->device >= 0) {
      (void)hipSetDevice(s->device);
      s->env.dev = std::move(st.texels);
      s->dev.env = s->env.host ? s->env.dev.p : nullptr;
    }
    apply_lighting(s);
  }
  return 0;
}
static std::shared_ptr<const ptx_scene::ImageHost> image_host_copy(const ptx_image* img) {
  auto h = std::make_shared<ptx_scene::ImageHost>();
  h->width = img->width;
  h->height = img->height;
  h->flags = img->flags;
  h->rec = scene_image_records(img);
  return h;
}
static int check_texture_index(const ptx_scene* s, int32_t index) {
  if (index < 0 || index >= s->host->n_textures) return fail(PTX_ERR_ARG, "texture index %d out of range (the scene's texture table has %d entries)", index, s->host->n_textures);
  return 0;
}
static const double kIdentity3[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};

int32_t ptx_scene_set_texture_image(ptx_scene* s, int32_t index, const ptx_image* img) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  int rc = check_texture_index(s, index);
  if (rc) return rc;
  if (img) {
    std::string msg;
    if ((rc = scene_check_image(img, false, &msg)) != 0) return fail(rc, "%s", msg.c_str());
  }
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "a texture image cannot change while a render runs on the scene");
  if (!img && s->images.empty()) return 0; /* nothing was ever set */
  std::shared_ptr<const ptx_scene::ImageHost> host = img ? image_host_copy(img) : nullptr;
  return family_take_texture_image(scene_family(s), index, host);
}

int32_t ptx_scene_set_environment(ptx_scene* s, const ptx_image* img, const double* R) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  int rc = 0;
  if (img) {
    std::string msg;
    if ((rc = scene_check_image(img, true, &msg)) != 0) return fail(rc, "%s", msg.c_str());
  }
  if (R)
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(R[k])) return fail(PTX_ERR_ARG, "environment: R[%d] is not finite", k);
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the environment cannot change while a render runs on the scene");
  const double* rot = (img && R) ? R : kIdentity3;
  if (s->env_sampling && !img) return fail(PTX_ERR_STATE, "the environment is being sampled: turn environment sampling off first");
  std::shared_ptr<const ptx_scene::ImageHost> host = img ? image_host_copy(img) : nullptr;
  EnvDensityRef density;
  if (s->env_sampling && (rc = env_density_make(*host, rot, &density)) != 0) return rc; /* (refused: the old state stays) */
  return family_take_environment(scene_family(s), host, rot, density);
}

int32_t ptx_scene_set_environment_sampling(ptx_scene* s, int32_t on) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "environment sampling cannot change while a render runs on the scene");
  EnvDensityRef density;
  if (on) {
    if (!s->env.host) return fail(PTX_ERR_ARG, "environment sampling needs an environment (ptx_scene_set_environment with an image)");
    if (const int rc = env_density_make(*s->env.host, s->env_rot, &density)) return rc;
  } else {
    if (!s->env_sampling) return 0;
    if (s->lighting == PTX_LIGHTING_SAMPLED && s->host->n_emissive_tris == 0 && !s->sphere_sampling)
      return fail(PTX_ERR_STATE, "sampled lighting has nothing but the environment to sample: set another lighting mode first");
  }
  return family_take_env_sampling(scene_family(s), on != 0, density);
}

int32_t ptx_scene_environment_sampling(const ptx_scene* s, int32_t* on_out, double* total_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (on_out) *on_out = s->env_sampling ? 1 : 0;
  if (total_out) *total_out = (s->env_sampling && s->env_density) ? s->env_density->total : 0.0;
  return 0;
}

int32_t ptx_environment_distribution(const ptx_scene* s, double* marginal_out, double* conditional_out) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (!s->env_sampling || !s->env_density) return fail(PTX_ERR_STATE, "environment sampling is off: there is no density to inspect");
  const PtEnvDensity& d = *s->env_density;
  const size_t W = (size_t)d.width, H = (size_t)d.height;
  if (marginal_out) std::memcpy(marginal_out, d.table.data() + PT_ENVD_ROWS, sizeof(double) * H);
  if (conditional_out) std::memcpy(conditional_out, d.table.data() + PT_ENVD_COND(H), sizeof(double) * W * H);
  return 0;
}

static void image_describe(const ptx_scene::ImageHost* h, ptx_image* out) {
  std::memset(out, 0, sizeof *out);
  if (!h) return;
  out->width = h->width;
  out->height = h->height;
  out->flags = h->flags;
}
int32_t ptx_scene_texture_image(const ptx_scene* s, int32_t index, ptx_image* out) {
  if (!s || !out) return fail(PTX_ERR_ARG, "NULL argument");
  const int rc = check_texture_index(s, index);
  if (rc) return rc;
  image_describe(s->images.empty() ? nullptr : s->images[(size_t)index]->host.get(), out);
  return 0;
}
int32_t ptx_scene_environment(const ptx_scene* s, ptx_image* out, double* R_out) {
  if (!s || !out) return fail(PTX_ERR_ARG, "NULL argument");
  image_describe(s->env.host.get(), out);
  if (R_out) std::memcpy(R_out, s->env_rot, sizeof s->env_rot);
  return 0;
}

int32_t ptx_scene_stats(const ptx_scene* s, ptx_stats* out) {
  if (!s || !out) return fail(PTX_ERR_ARG, "NULL argument");
  std::memset(out, 0, sizeof *out);
  fill_tree_stats(s, out);
  return 0;
}

int32_t ptx_tile_list_stats(const ptx_scene* s, int64_t out[5]) {
  if (!s || !out) return fail(PTX_ERR_ARG, "NULL argument");
  for (int k = 0; k < 5; ++k) out[k] = 0;
  if (s->device < 0 || !s->tile_last) return 0;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize()); /* (a frame queued with PTX_RENDER_ASYNC may still be counting) */
  unsigned long long fb = 0;
  HIP_TRY(hipMemcpy(&fb, &s->counters.p->tile_fallbacks, sizeof fb, hipMemcpyDeviceToHost));
  const PtTileGrid& g = *s->tile_last->grid;
  out[0] = s->tile_launches;
  out[1] = (int64_t)g.rec.size();
  out[2] = g.n_walk;
  out[3] = g.longest;
  out[4] = (int64_t)fb;
  return 0;
}

int32_t ptx_render_raw_device(ptx_scene* s, const ptx_render_params* p, double* d_raw_out, void* stream, ptx_stats* stats) {
  if (!s || !d_raw_out) return fail(PTX_ERR_ARG, "NULL argument");
  int rc = check_render_args(s, p, nullptr);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const double t0 = wall_ms();
  rc = render_raw(s, p, d_raw_out, (hipStream_t)stream, stats, nullptr, nullptr);
  if (rc) return rc;
  if (stats) stats->render_ms = wall_ms() - t0;
  return 0;
}

int32_t ptx_film_resolve_device(int32_t device, int32_t width, int32_t height, int32_t spp, const double* d_raw_full,
                                double* d_rgb_out, void* stream) {
  if (!d_raw_full || !d_rgb_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || height <= 0 || spp <= 0) return fail(PTX_ERR_ARG, "bad dimensions");
  HIP_TRY(hipSetDevice(device));
  int rc = film_resolve(width, height, spp, d_raw_full, d_rgb_out, (hipStream_t)stream);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int32_t ptx_film_resolve_ex_device(int32_t device, int32_t width, int32_t height, int32_t spp, const ptx_film_params* film,
                                   const double* d_raw_full, double* d_rgb_out, void* stream) {
  if (!d_raw_full || !d_rgb_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || height <= 0 || spp <= 0) return fail(PTX_ERR_ARG, "bad dimensions");
  const ptx_film_params f = film ? *film : kFilmDefault;
  int rc = film_check(&f);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  rc = film_resolve(width, height, spp, d_raw_full, d_rgb_out, (hipStream_t)stream, PtBandMap{1, 1, 0}, 0, -1, f);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

static int32_t film_resolve_banded(int32_t device, int32_t width, int32_t height, int32_t spp, const double* d_gathered,
                                   int32_t n_ranks, int32_t band_rows, int32_t pad_rows, double* d_rgb_out, void* stream, bool wait,
                                   const ptx_film_params& film = kFilmDefault) {
  if (!d_gathered || !d_rgb_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || height <= 0 || spp <= 0) return fail(PTX_ERR_ARG, "bad dimensions");
  if (n_ranks < 1 || band_rows < 1) return fail(PTX_ERR_ARG, "need n_ranks >= 1 and band_rows >= 1");
  ptx_render_params q;
  std::memset(&q, 0, sizeof q);
  q.width = width; q.height = height; q.band_rows = band_rows; q.band_step = n_ranks;
  for (int r = 0; r < n_ranks; ++r) {
    q.band_first = r;
    if (local_rows(&q) > pad_rows) return fail(PTX_ERR_ARG, "pad_rows %d is smaller than rank %d's %d rows", pad_rows, r, local_rows(&q));
  }
  HIP_TRY(hipSetDevice(device));
  int rc = film_resolve(width, height, spp, d_gathered, d_rgb_out, (hipStream_t)stream, PtBandMap{n_ranks, band_rows, pad_rows}, 0, -1, film);
  if (rc) return rc;
  if (wait) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
int32_t ptx_film_resolve_banded_device(int32_t device, int32_t width, int32_t height, int32_t spp, const double* d_gathered,
                                       int32_t n_ranks, int32_t band_rows, int32_t pad_rows, double* d_rgb_out, void* stream) {
  return film_resolve_banded(device, width, height, spp, d_gathered, n_ranks, band_rows, pad_rows, d_rgb_out, stream, true);
}
int32_t ptx_film_resolve_banded_ex_device(int32_t device, int32_t width, int32_t height, int32_t spp, const ptx_film_params* film,
                                          const double* d_gathered, int32_t n_ranks, int32_t band_rows, int32_t pad_rows, double* d_rgb_out,
                                          void* stream) {
  const ptx_film_params f = film ? *film : kFilmDefault;
  const int rc = film_check(&f);
  if (rc) return rc;
  return film_resolve_banded(device, width, height, spp, d_gathered, n_ranks, band_rows, pad_rows, d_rgb_out, stream, true, f);
}
int32_t ptx_film_resolve_banded_queue(int32_t device, int32_t width, int32_t height, int32_t spp, const double* d_gathered,
                                      int32_t n_ranks, int32_t band_rows, int32_t pad_rows, double* d_rgb_out, void* stream) {
  return film_resolve_banded(device, width, height, spp, d_gathered, n_ranks, band_rows, pad_rows, d_rgb_out, stream, false);
}

void ptx_release_workspaces(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  BvhGpuWorkspace& ws = bvh_gpu_workspace(); /* follows the current device; buffers of another device were freed on the switch */
  ws.release();
}

ptx_scene* ptx_scene_replicate(const ptx_scene* src, int32_t device) {
  if (!src) {
    fail(PTX_ERR_ARG, "NULL scene");
    return nullptr;
  }
  if (src->device < 0 || !src->host) {
    fail(PTX_ERR_STATE, "a host-only scene (device -1) cannot be replicated");
    return nullptr;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || device < 0 || device >= ndev) {
    fail(PTX_ERR_ARG, "device %d out of range (have %d)", device, ndev);
    return nullptr;
  }
  if ((e = hipSetDevice(device)) != hipSuccess) {
    fail(PTX_ERR_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
    return nullptr;
  }
  const double t0 = wall_ms();
  ptx_scene* s = new ptx_scene();
  s->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
  s->host = src->host;
  s->tile_cache = src->tile_cache;
  s->n_prims = src->n_prims;
  s->tree_depth = src->tree_depth;
  s->tree_leaves = src->tree_leaves;
  s->film = src->film;
  s->lens_radius = src->lens_radius; /* (scene_upload schedules, like every setter) */
  s->lens_focus = src->lens_focus;
  s->own_view = src->own_view;
  copy_camera_pose(s, src);
  copy_camera_shutter(s, src);
  s->projection = src->projection;
  if (scene_upload(s) != 0) {
    ptx_scene_destroy(s);
    return nullptr;
  }
  /* the images and the environment: the host copies are shared, this device gets its own uploads */
  for (size_t i = 0; i < src->images.size(); ++i)
    if (src->images[i]->host && family_take_texture_image({s}, (int32_t)i, src->images[i]->host) != 0) {
      ptx_scene_destroy(s);
      return nullptr;
    }
  if (src->env.host && family_take_environment({s}, src->env.host, src->env_rot) != 0) {
    ptx_scene_destroy(s);
    return nullptr;
  }
  /* environment sampling (the density is shared too), then the lighting mode, which may need it */
  if ((src->env_sampling && family_take_env_sampling({s}, true, src->env_density) != 0) ||
      (src->sphere_sampling && take_sphere_sampling(s, true) != 0) ||
      (src->lighting != 0 && ptx_scene_set_lighting(s, src->lighting) != 0)) {
    ptx_scene_destroy(s);
    return nullptr;
  }
  s->build_ms = wall_ms() - t0; /* upload only: the tree came with the original */
  return s;
}

/* RAII pair of timing events (ptx_render's film pass): destroyed on every exit path */
namespace {
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

int timed_film(const ptx_render_params& p, const double* d_raw, double* d_rgb, PtBandMap map, ptx_stats* stats, const ptx_film_params& film) {
  EventPair ev;
  if (p.time_kernels) {
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, nullptr));
  }
  int rc = film_resolve(p.width, p.height, p.samples_per_pixel, d_raw, d_rgb, nullptr, map, 0, -1, film);
  if (rc) return rc;
  if (p.time_kernels) {
    HIP_TRY(hipEventRecord(ev.b, nullptr));
    HIP_TRY(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    if (stats) {
      stats->kernel_ms[PTX_KERNEL_FILM] += ms;
      stats->kernel_launches[PTX_KERNEL_FILM] += 1;
    }
  }
  return 0;
}

/* The post-gamma framebuffer back to the caller's (pageable) memory.  A plain hipMemcpy of 50 MB into pageable memory
 * runs at ~7 GB/s (6.8 ms at 1080p, a fifth of the render).  Here the device copies 4 MB chunks into a pinned staging
 * buffer with asynchronous DMA while a few host threads move finished chunks on to the caller's buffer: ~2 ms. */
/* cs: the stream the copies are ordered on (NULL: the null stream, and the call waits for the whole device at the end);
 * ptx_render_progressive copies update j on its copy stream while the next slice is already queued on the others */
int copy_to_host_on(hipStream_t cs, const char* d_src, char* dst, size_t n_bytes) {
  if (!cs) {
    HIP_TRY(hipMemcpy(dst, d_src, n_bytes, hipMemcpyDeviceToHost));
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(dst, d_src, n_bytes, hipMemcpyDeviceToHost, cs));
  HIP_TRY(hipStreamSynchronize(cs));
  return 0;
}
/* (in bytes: an f64 image through framebuffer_to_host below, a display image as it is) */
int image_bytes_to_host(ptx_scene* s, const char* d_src, char* dst, size_t n_bytes, hipStream_t cs = nullptr) {
  if (env_int("PTX_PLAIN_D2H", 0) || n_bytes < ((size_t)8 << 20)) return copy_to_host_on(cs, d_src, dst, n_bytes);
  /* an image the caller has pinned (ptx_image_pin): one DMA straight into it */
  if (s->holds_pinned(dst, n_bytes)) {
    HIP_TRY(hipMemcpyAsync(dst, d_src, n_bytes, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    return 0;
  }
  const size_t n_doubles = (n_bytes + sizeof(double) - 1) / sizeof(double); /* the staging buffer is counted in doubles */
  if (s->pinned_n < n_doubles) {
    if (s->pinned) (void)hipHostFree(s->pinned);
    s->pinned = nullptr;
    s->pinned_n = 0;
    if (hipHostMalloc((void**)&s->pinned, sizeof(double) * n_doubles, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return copy_to_host_on(cs, d_src, dst, n_bytes); /* no pinned memory to be had */
    }
    s->pinned_n = n_doubles;
  }
  char* const stage = (char*)s->pinned;
  const size_t chunk = (size_t)4 << 20; /* 4 MB */
  const size_t n_chunks = (n_bytes + chunk - 1) / chunk;
  std::vector<hipEvent_t> done(n_chunks, nullptr);
  int rc = 0;
  for (size_t k = 0; k < n_chunks && rc == 0; ++k) {
    const size_t off = k * chunk, len = std::min(chunk, n_bytes - off);
    if (hipEventCreateWithFlags(&done[k], hipEventDisableTiming) != hipSuccess ||
        hipMemcpyAsync(stage + off, d_src + off, len, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipEventRecord(done[k], cs) != hipSuccess)
      rc = fail(PTX_ERR_HIP, "framebuffer copy failed: %s", hipGetErrorString(hipGetLastError()));
  }
  if (rc == 0) {
    const int n_threads = (int)std::min<size_t>(4, n_chunks);
    std::atomic<int> bad{0};
    const int dev = s->device;
    auto mover = [&](int tid) {
      (void)hipSetDevice(dev);
      for (size_t k = (size_t)tid; k < n_chunks; k += (size_t)n_threads) {
        if (hipEventSynchronize(done[k]) != hipSuccess) { bad = 1; return; }
        const size_t off = k * chunk, len = std::min(chunk, n_bytes - off);
        std::memcpy(dst + off, stage + off, len);
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < n_threads; ++t) th.emplace_back(mover, t);
    mover(0);
    for (std::thread& t : th) t.join();
    if (bad) rc = fail(PTX_ERR_HIP, "framebuffer copy failed: %s", hipGetErrorString(hipGetLastError()));
  }
  if (cs) (void)hipStreamSynchronize(cs);
  else (void)hipDeviceSynchronize();
  for (hipEvent_t e : done)
    if (e) (void)hipEventDestroy(e);
  return rc;
}
int framebuffer_to_host(ptx_scene* s, const double* d_src, double* dst, size_t n_doubles, hipStream_t cs = nullptr) {
  return image_bytes_to_host(s, (const char*)d_src, (char*)dst, sizeof(double) * n_doubles, cs);
}

/* ---- display outputs (display.inc; the rule: include/ptx.h) ---- */
/* one display call as the render entry points carry it: the checked settings, the caller's image and its size */
struct DisplayJob {
  ptx_display_params d;
  void* out;
  size_t pixel_bytes;
};

int check_display(const ptx_display_params* d) {
  if (!d) return fail(PTX_ERR_ARG, "display: NULL ptx_display_params");
  std::string msg;
  const int rc = display_check(d, &msg);
  return rc ? fail(rc, "%s", msg.c_str()) : 0;
}

/* the sRGB thresholds on the current device: copied into the module's table the first time the device displays.  The flag is the
 * process's, like the dynamic-LDS limits the handles remember: an embedding application that calls hipDeviceReset re-zeroes the
 * module's table behind it (every sRGB code would then read 255) and has to restart the process, as it has to for every handle it
 * made before the reset. */
constexpr int kMaxDisplayDevices = 64;
int display_thresholds_device() {
  static std::mutex mu;
  static bool done[kMaxDisplayDevices] = {};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDisplayDevices) return fail(PTX_ERR_ARG, "display: device %d is beyond the %d the threshold table is kept for", dev, kMaxDisplayDevices);
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev]) return 0;
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_display_thresholds), display_thresholds(), sizeof(double) * PT_DISPLAY_THRESHOLDS));
  done[dev] = true;
  return 0;
}

/* k_display_image over pixels [p0, p1) of the image at d_rgb into the display image at d_out, queued on st (the device is current
 * and has its thresholds -- display_thresholds_device, a blocking copy, is called by every entry point before it queues anything --
 * d has passed check_display, both images are 16-byte aligned) */
int display_queue(const ptx_display_params& d, long long p0, long long p1, const double* d_rgb, void* d_out, hipStream_t st) {
  if (p1 <= p0) return 0;
  const long long quads = (p1 + 3) / 4 - p0 / 4;
  const dim3 grid(grid256(quads)), block(256);
  const PtDisplay pd{d.transfer, d.tone, d.exposure};
  switch (d.format) {
    case PTX_PIXEL_RGB8: hipLaunchKernelGGL(k_display_image<PTX_PIXEL_RGB8>, grid, block, 0, st, d_rgb, p0, p1, pd, d_out); break;
    case PTX_PIXEL_RGBA8: hipLaunchKernelGGL(k_display_image<PTX_PIXEL_RGBA8>, grid, block, 0, st, d_rgb, p0, p1, pd, d_out); break;
    case PTX_PIXEL_RGB32F: hipLaunchKernelGGL(k_display_image<PTX_PIXEL_RGB32F>, grid, block, 0, st, d_rgb, p0, p1, pd, d_out); break;
    default: hipLaunchKernelGGL(k_display_image<PTX_PIXEL_RGBA32F>, grid, block, 0, st, d_rgb, p0, p1, pd, d_out); break;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
constexpr long long kMaxDisplayPixels = 1ll << 40; /* the grid: a quad a thread, 256 a workgroup, fewer than 2^31 workgroups */

/* the display image of the handle's filmed image s->rgb, whole, queued on st */
int display_scene_image(ptx_scene* s, const DisplayJob& job, long long npix, hipStream_t st) {
  return display_queue(job.d, 0, npix, s->rgb.p, s->disp.p, st);
}

/* progress sink of the worker threads: pixel counts are only ADDED here; the calling thread hands them on */
void progress_to_counter(void* user, int64_t pixels) { ((std::atomic<long long>*)user)->fetch_add(pixels); }
}  // namespace

/* ptx_render and ptx_render_multi with the image they hand back chosen by `job`: NULL = the f64 image into rgb_out; otherwise the
 * display image into job->out (ptx_render_display), and rgb_out is not read */
static int32_t render_one(ptx_scene* s, const ptx_render_params* p_in, double* rgb_out, const DisplayJob* job, ptx_stats* stats,
                          ptx_progress_fn progress, void* user);

static int32_t render_many(ptx_scene* const* scenes, int32_t n, const ptx_render_params* p_in, double* rgb_out, const DisplayJob* job,
                           ptx_stats* stats, ptx_progress_fn progress, void* user) {
  if (!scenes || !(job ? job->out : (void*)rgb_out) || n < 1) return fail(PTX_ERR_ARG, "NULL argument or no scenes");
  if (n > 64) return fail(PTX_ERR_ARG, "at most 64 scenes");
  for (int k = 0; k < n; ++k) {
    if (!scenes[k]) return fail(PTX_ERR_ARG, "scene %d is NULL", k);
    if (scenes[k]->device < 0) return fail(PTX_ERR_STATE, "scene %d was created host-only (device -1): no CPU fallback exists", k);
    for (int j = 0; j < k; ++j)
      if (scenes[j] == scenes[k]) return fail(PTX_ERR_ARG, "scene %d is the same handle as scene %d (one render per handle at a time)", k, j);
    if (scenes[k]->host != scenes[0]->host && (scenes[k]->dev.n_nodes != scenes[0]->dev.n_nodes || scenes[k]->dev.n_slots != scenes[0]->dev.n_slots))
      return fail(PTX_ERR_ARG, "scene %d is not a replica of scene 0", k);
    if (scenes[k]->lens_radius != scenes[0]->lens_radius || (scenes[0]->lens_radius > 0.0 && scenes[k]->lens_focus != scenes[0]->lens_focus))
      return fail(PTX_ERR_ARG, "scene %d does not carry the lens of scene 0 (ptx_scene_set_lens): the bands would not be one image", k);
    if (scenes[k]->projection != scenes[0]->projection)
      return fail(PTX_ERR_ARG, "scene %d does not carry the camera projection of scene 0 (ptx_scene_set_camera_projection): the bands would not be one image", k);
    if (!same_camera_pose(scenes[k], scenes[0]))
      return fail(PTX_ERR_ARG, "scene %d does not carry the camera pose of scene 0 (ptx_scene_set_camera_pose): the bands would not be one image", k);
    if (!same_camera_shutter(scenes[k], scenes[0]))
      return fail(PTX_ERR_ARG, "scene %d does not carry the camera shutter of scene 0 (ptx_scene_set_camera_shutter): the bands would not be one image", k);
  }
  int rc = check_params(p_in);
  if (rc) return rc;
  rc = check_shutter_depth(scenes[0], p_in);
  if (rc) return rc;
  if (n == 1) {
    ptx_render_params p1 = *p_in;
    p1.n_gpus = 0;
    return render_one(scenes[0], &p1, rgb_out, job, stats, progress, user);
  }
  ptx_render_params p = *p_in;
  p.n_gpus = 0;
  p.flags = 0; /* PTX_RENDER_ASYNC is ptx_render_raw_device's: this entry point hands back a host framebuffer */
  p.band_rows = p.band_rows > 0 ? p.band_rows : 8; /* 8 rows = the 8x8 pixel tile a wave covers; finer bands balance better */
  p.band_step = n;
  int pad_rows = 0;
  for (int k = 0; k < n; ++k) {
    p.band_first = k;
    pad_rows = std::max(pad_rows, local_rows(&p));
  }
  ptx_scene* root = scenes[0];
  const double t0 = wall_ms();
  HIP_TRY(hipSetDevice(root->device));
  const size_t slice = (size_t)pad_rows * p.width * 3;
  HIP_TRY(root->gather.ensure(slice * (size_t)n));
  HIP_TRY(root->rgb.ensure((size_t)p.width * p.height * 3));
  if (job) {
    HIP_TRY(root->disp.ensure((size_t)p.width * p.height * job->pixel_bytes));
    rc = display_thresholds_device();
    if (rc) return rc;
  }

  /* Peer access root <-> replica, once per pair (kept with the replica's handle): with it hipMemcpyPeer moves the bands
   * device to device over xGMI; without it the runtime stages them through host memory.  Either way the bytes are the same. */
  for (int k = 1; k < n; ++k) {
    ptx_scene* s = scenes[k];
    if (s->device == root->device || s->peer_root == root->device) continue;
    int can_rs = 0, can_sr = 0;
    (void)hipDeviceCanAccessPeer(&can_rs, root->device, s->device);
    (void)hipDeviceCanAccessPeer(&can_sr, s->device, root->device);
    bool ok = can_rs && can_sr;
    if (ok) {
      hipError_t e1 = hipSetDevice(root->device) == hipSuccess ? hipDeviceEnablePeerAccess(s->device, 0) : hipErrorInvalidDevice;
      hipError_t e2 = hipSetDevice(s->device) == hipSuccess ? hipDeviceEnablePeerAccess(root->device, 0) : hipErrorInvalidDevice;
      ok = (e1 == hipSuccess || e1 == hipErrorPeerAccessAlreadyEnabled) && (e2 == hipSuccess || e2 == hipErrorPeerAccessAlreadyEnabled);
      (void)hipGetLastError(); /* "already enabled" is not an error of this call */
    }
    /* only SUCCESS is remembered: a transient failure (another process holding the mapping, a driver hiccup) is retried by the
     * next call instead of pinning this replica to staged host copies for the handle's life */
    s->peer_root = ok ? root->device : -1;
    s->peer_ok = ok;
  }
  HIP_TRY(hipSetDevice(root->device));

  struct Worker {
    int rc = 0;
    std::string err;
    ptx_stats st;
  };
  std::vector<Worker> work((size_t)n);
  std::atomic<long long> done_pixels{0};
  std::atomic<int> running{n};
  auto body = [&](int k) {
    Worker& w = work[(size_t)k];
    ptx_scene* s = scenes[k];
    ptx_render_params pk = p;
    pk.band_first = k;
    auto run = [&]() -> int {
      HIP_TRY(hipSetDevice(s->device));
      double* dst = root->gather.p + slice * (size_t)k;
      const size_t bytes = sizeof(double) * (size_t)local_rows(&pk) * pk.width * 3;
      if (s->device == root->device) /* same device: the bands land in the gathered layout directly */
        return render_raw(s, &pk, dst, nullptr, &w.st, progress ? progress_to_counter : nullptr, &done_pixels);
      HIP_TRY(s->raw.ensure((size_t)pad_rows * pk.width * 3));
      int r = render_raw(s, &pk, s->raw.p, nullptr, &w.st, progress ? progress_to_counter : nullptr, &done_pixels);
      if (r) return r;
      /* the one exchange of the path: this replica's raw sums to the root device, peer to peer over xGMI */
      if (bytes) HIP_TRY(hipMemcpyPeer(dst, root->device, s->raw.p, s->device, bytes));
      return 0;
    };
    w.rc = run();
    if (w.rc) w.err = g_last_error; /* thread-local: carried to the calling thread below */
    running.fetch_sub(1);
  };
  std::vector<std::thread> threads;
  threads.reserve((size_t)n);
  for (int k = 0; k < n; ++k) threads.emplace_back(body, k);
  if (progress) { /* update_progress stays on the calling thread (the OCaml runtime lock is never needed elsewhere) */
    long long reported = 0;
    for (;;) {
      const bool finished = running.load() == 0;
      const long long now = done_pixels.load();
      if (now > reported) {
        progress(user, now - reported);
        reported = now;
      }
      if (finished) break;
      std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
  }
  for (std::thread& t : threads) t.join();
  for (int k = 0; k < n; ++k)
    if (work[(size_t)k].rc) return fail(work[(size_t)k].rc, "device %d (rank %d of %d): %s", scenes[k]->device, k, n, work[(size_t)k].err.c_str());
  HIP_TRY(hipSetDevice(root->device));
  if (stats) {
    *stats = work[0].st;
    for (int k = 1; k < n; ++k) {
      const ptx_stats& o = work[(size_t)k].st;
      stats->samples += o.samples; stats->segments += o.segments; stats->nodes_tested += o.nodes_tested;
      stats->prims_tested += o.prims_tested; stats->floor_tested += o.floor_tested;
      stats->filter_undecided += o.filter_undecided; stats->filter_fallback_steps += o.filter_fallback_steps;
      for (int i = 0; i < PTX_N_KERNELS; ++i) { /* the slowest device bounds the frame */
        stats->kernel_ms[i] = std::max(stats->kernel_ms[i], o.kernel_ms[i]);
        stats->kernel_launches[i] = std::max(stats->kernel_launches[i], o.kernel_launches[i]);
      }
    }
  }
  if (stats)
    for (int k = 1; k < n; ++k)
      if (scenes[k]->device != root->device) (scenes[k]->peer_ok ? stats->peer_copies : stats->staged_copies) += 1;
  rc = timed_film(p, root->gather.p, root->rgb.p, PtBandMap{n, p.band_rows, pad_rows}, stats, root->film); /* the film runs on scenes[0]: its film governs */
  if (rc) return rc;
  if (job) { /* the display kernel runs over the filmed image: it needs no band map of its own */
    rc = display_scene_image(root, *job, (long long)p.width * p.height, nullptr);
    if (!rc) rc = image_bytes_to_host(root, (const char*)root->disp.p, (char*)job->out, (size_t)p.width * p.height * job->pixel_bytes);
  } else {
    rc = framebuffer_to_host(root, root->rgb.p, rgb_out, (size_t)p.width * p.height * 3);
  }
  if (rc) return rc;
  if (stats) stats->render_ms = wall_ms() - t0;
  return 0;
}

int32_t ptx_render_multi(ptx_scene* const* scenes, int32_t n, const ptx_render_params* p_in, double* rgb_out, ptx_stats* stats,
                         ptx_progress_fn progress, void* user) {
  return render_many(scenes, n, p_in, rgb_out, nullptr, stats, progress, user);
}

/* ptx_render's tail into an image the caller has pinned, as a pipeline: the last batch's accumulate runs in row slabs, and on a
 * second stream slab k is filmed (once slab k + 1 has been summed: the 3 x 3 filter reads one row beyond) and copied into the
 * image while the later slabs are still being summed.  49.8 MB at the 55.6 GB/s the PCIe link gives (tools/d2h_rate.py: 0.89 ms,
 * whatever the number of pieces or streams) is the floor of this entry point over the device-resident one; what the
 * pipeline hides is the last accumulate (0.37 ms at 1080p).
 * *copied = false: the frame had no last batch to cut into slabs (one pass per batch); the raw sums are complete in s->raw and
 * the caller films and copies them the plain way. */
namespace {
int render_into_pinned(ptx_scene* s, const ptx_render_params& p, int n_slabs, double* rgb_out, const DisplayJob* job, ptx_stats* stats, bool* copied) {
  FinalSlabs fs;
  fs.n = std::min(n_slabs, kMaxFinalSlabs);
  for (int k = 0; k <= fs.n; ++k) fs.row[k] = (int)((long long)p.height * k / fs.n);
  /* Invariant of the wait below: slab k's film reads s->film.pixel_radius rows beyond it, and "slab k + 1 has been summed" covers
   * them only if slab k + 1 is at least that high (the slabs before k are behind earlier events of the same stream).  At most
   * kMaxFinalSlabs slabs over at least kMinSlabImageRows rows gives >= 8 rows >= PTX_FILM_MAX_RADIUS (the static_assert beside the
   * constants); this refuses, instead of misreading, a caller that breaks it some other way. */
  for (int k = 0; k < fs.n; ++k)
    if (fs.row[k + 1] - fs.row[k] < s->film.pixel_radius)
      return fail(PTX_ERR_STATE, "row slab %d of %d has %d rows, fewer than the film's pixel_radius %d", k, fs.n, fs.row[k + 1] - fs.row[k], s->film.pixel_radius);
  int rc = ensure_copy_stream(s);
  for (int k = 0; k < fs.n && !rc; ++k) {
    rc = ensure_event(&s->ev_slab[k]);
    fs.done[k] = s->ev_slab[k];
  }
  if (rc) return rc;
  DrainOnExit drain; /* from the queued frame to the last wait, every return drains the lanes, the film and the copy into rgb_out */
  ptx_render_params pq = p;
  pq.flags = PTX_RENDER_ASYNC; /* queued: this thread goes on to queue the tail behind the slabs' events */
  rc = render_raw(s, &pq, s->raw.p, nullptr, stats, nullptr, nullptr, &fs);
  if (rc) return rc;
  for (int k = 0; k < fs.n && fs.used; ++k) {
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, fs.done[std::min(k + 1, fs.n - 1)], 0));
    rc = film_resolve(p.width, p.height, p.samples_per_pixel, s->raw.p, s->rgb.p, s->copy_stream, PtBandMap{1, 1, 0}, fs.row[k], fs.row[k + 1], s->film);
    if (rc) return rc;
    const size_t off = (size_t)fs.row[k] * p.width * 3, len = (size_t)(fs.row[k + 1] - fs.row[k]) * p.width * 3;
    if (job) { /* the display kernel over the slab's rows, then the slab's display bytes */
      const long long p0 = (long long)fs.row[k] * p.width, p1 = (long long)fs.row[k + 1] * p.width;
      rc = display_queue(job->d, p0, p1, s->rgb.p, s->disp.p, s->copy_stream);
      if (rc) return rc;
#ifdef PT_DISPLAY_MUTANT_SLAB
      const size_t boff = (size_t)p0 * 3, blen = (size_t)(p1 - p0) * job->pixel_bytes; /* the offset counted in doubles */
#else
      const size_t boff = (size_t)p0 * job->pixel_bytes, blen = (size_t)(p1 - p0) * job->pixel_bytes;
#endif
      if (blen) HIP_TRY(hipMemcpyAsync((char*)job->out + boff, (const char*)s->disp.p + boff, blen, hipMemcpyDeviceToHost, s->copy_stream));
    } else if (len) HIP_TRY(hipMemcpyAsync(rgb_out + off, s->rgb.p + off, sizeof(double) * len, hipMemcpyDeviceToHost, s->copy_stream));
  }
  if (fs.used) HIP_TRY(hipStreamSynchronize(s->copy_stream));
  HIP_TRY(hipStreamSynchronize(nullptr));
  drain.armed = false;
  *copied = fs.used;
  return 0;
}
}  // namespace

static int32_t render_one(ptx_scene* s, const ptx_render_params* p_in, double* rgb_out, const DisplayJob* job, ptx_stats* stats,
                          ptx_progress_fn progress, void* user) {
  if (!s || !(job ? job->out : (void*)rgb_out)) return fail(PTX_ERR_ARG, "NULL argument");
  int rc = check_render_args(s, p_in, nullptr);
  if (rc) return rc;
  if (p_in->n_gpus > 1) {
    /* replicas on the following device ordinals, made once and kept with the handle */
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    const bool alias = env_int("PTX_MULTI_ALIAS", 0) != 0; /* test hook for one-GPU boxes: replicas share devices */
    if (p_in->n_gpus > ndev && !alias) return fail(PTX_ERR_ARG, "n_gpus %d but only %d HIP device(s) visible", p_in->n_gpus, ndev);
    while ((int)s->replicas.size() < p_in->n_gpus - 1) {
      ptx_scene* r = ptx_scene_replicate(s, (s->device + 1 + (int)s->replicas.size()) % ndev);
      if (!r) return g_last_code ? g_last_code : PTX_ERR_HIP; /* code and message set by ptx_scene_replicate */
      s->replicas.push_back(r);
    }
    std::vector<ptx_scene*> all;
    all.push_back(s);
    for (int k = 0; k + 1 < p_in->n_gpus; ++k) all.push_back(s->replicas[(size_t)k]);
    return render_many(all.data(), (int32_t)all.size(), p_in, rgb_out, job, stats, progress, user);
  }
  ptx_render_params p = *p_in;
  p.band_step = 0; /* whole image on this GPU */
  p.flags = 0;     /* PTX_RENDER_ASYNC is ptx_render_raw_device's: this entry point hands back a host framebuffer */
  HIP_TRY(hipSetDevice(s->device));
  const double t0 = wall_ms();
  const size_t n = (size_t)p.width * p.height * 3;
  HIP_TRY(s->raw.ensure(n));
  HIP_TRY(s->rgb.ensure(n));
  const size_t out_bytes = job ? (size_t)p.width * p.height * job->pixel_bytes : sizeof(double) * n;
  if (job) {
    HIP_TRY(s->disp.ensure(out_bytes));
    rc = display_thresholds_device();
    if (rc) return rc;
  }
  /* an image the caller has pinned takes the frame's tail as a pipeline (render_into_pinned) */
  const bool pinned = s->holds_pinned(job ? job->out : (void*)rgb_out, out_bytes);
  const int n_slabs = (pinned && !p.count_work && !p.time_kernels && !progress && p.height >= kMinSlabImageRows && p.max_bounces > 0) ? env_int("PTX_FINAL_SLABS", 4) : 1;
  bool copied = false;
  if (n_slabs > 1) rc = render_into_pinned(s, p, n_slabs, rgb_out, job, stats, &copied);
  else rc = render_raw(s, &p, s->raw.p, nullptr, stats, progress, user);
  if (rc) return rc;
  if (copied) {
    if (stats) stats->render_ms = wall_ms() - t0;
    return 0;
  }
  rc = timed_film(p, s->raw.p, s->rgb.p, PtBandMap{1, 1, 0}, stats, s->film);
  if (rc) return rc;
  if (job) {
    rc = display_scene_image(s, *job, (long long)p.width * p.height, nullptr);
    if (!rc) rc = image_bytes_to_host(s, (const char*)s->disp.p, (char*)job->out, out_bytes);
  } else {
    rc = framebuffer_to_host(s, s->rgb.p, rgb_out, n);
  }
  if (rc) return rc;
  if (stats) stats->render_ms = wall_ms() - t0;
  return 0;
}

int32_t ptx_render(ptx_scene* s, const ptx_render_params* p_in, double* rgb_out, ptx_stats* stats, ptx_progress_fn progress, void* user) {
  return render_one(s, p_in, rgb_out, nullptr, stats, progress, user);
}

int32_t ptx_render_display(ptx_scene* s, const ptx_render_params* p_in, const ptx_display_params* display, void* out, ptx_stats* stats,
                           ptx_progress_fn progress, void* user) {
  const int rc = check_display(display);
  if (rc) return rc;
  const DisplayJob job{*display, out, (size_t)display_pixel_bytes(display->format)};
  return render_one(s, p_in, nullptr, &job, stats, progress, user);
}

/* ---- progressive rendering: a frame rendered as consecutive pass slices into the same raw sums ---- */
namespace {
int check_pass_range(const ptx_render_params* p, int32_t pass_first, int32_t pass_count) {
  if (pass_count < 1) return fail(PTX_ERR_ARG, "pass_count must be >= 1 (got %d)", pass_count);
  if (pass_first < 0 || (long long)pass_first + pass_count > p->samples_per_pixel)
    return fail(PTX_ERR_ARG, "pass range [%d, %lld) is outside the frame's passes [0, %d)", pass_first,
                (long long)pass_first + pass_count, p->samples_per_pixel);
  return 0;
}

int check_one_gpu(const ptx_render_params* p, const char* what) {
  if (p->n_gpus > 1 || p->band_step > 1)
    return fail(PTX_ERR_ARG, "%s runs on one GPU over the whole image (n_gpus %d, band_step %d)", what, p->n_gpus, p->band_step);
  return 0;
}

void add_slice_stats(ptx_stats* acc, const ptx_stats& o) {
  acc->segments += o.segments; acc->nodes_tested += o.nodes_tested; acc->prims_tested += o.prims_tested;
  acc->floor_tested += o.floor_tested; acc->filter_undecided += o.filter_undecided;
  acc->filter_fallback_steps += o.filter_fallback_steps; acc->solo_launches += o.solo_launches; acc->carry_launches += o.carry_launches;
  acc->lds_oct_launches += o.lds_oct_launches;
  acc->primary_lane_walks += o.primary_lane_walks;
  for (int i = 0; i < PTX_N_KERNELS; ++i) {
    acc->kernel_ms[i] += o.kernel_ms[i];
    acc->kernel_launches[i] += o.kernel_launches[i];
  }
}

/* The update loop of ptx_render_progressive and ptx_render_adaptive: a frame rendered as slices, an update (the image, its error,
 * a callback) after each.
 * Slices are queued on the null stream (PTX_RENDER_ASYNC: render_raw returns once they are queued).  Update j is filmed there
 * behind slice j's accumulate; slice j + 1 is queued next, so its bounces run while update j is copied out on copy_stream and
 * handed to the callback -- its accumulate waits for the film (render_raw's fork event, recorded behind it).  The copy of update
 * j + 1 is queued only after callback j has returned.  A render that counts work or times kernels waits for every slice and
 * queues the next one only after the callback.
 * The policy says what a slice and an update are: prepare() makes its own buffers and events; first() is the frame's first slice;
 * queue_update(cur) queues, on the null stream behind slice cur, the film into s->rgb, the error (s->err if asked for, rel_err at
 * the end of s->err_partials) and whatever else follows an update; next_slice(cur, &next) gives the slice after cur, count 0 when
 * the frame is complete (it may wait for what queue_update queued, and for nothing else); copy_extras(cs) queues further copies of
 * the update to the host on cs; call_back(update, cur, next, samples, rel) is the caller's callback and the stopping rule. */
extern "C++" template <class Policy>
int render_updates(ptx_scene* s, const ptx_render_params& p, Policy& pol, bool want_err, double* rgb_out, double* err_out, ptx_stats* stats,
                   const DisplayJob* job = nullptr) {
  RenderBusy busy(s);
  const double t0 = wall_ms();
  const long long npix = (long long)p.width * p.height;
  const size_t n = (size_t)npix * 3;
  HIP_TRY(s->raw.ensure(n));
  HIP_TRY(s->rgb.ensure(n));
  if (job) { /* the updates' images leave as display pixels (ptx_render_progressive_display): rgb_out is not read */
    HIP_TRY(s->disp.ensure((size_t)npix * job->pixel_bytes));
    const int rd = display_thresholds_device();
    if (rd) return rd;
  }
  if (want_err) {
    HIP_TRY(s->sq.ensure(n));
    HIP_TRY(s->err_partials.ensure(pixel_error_partials(npix)));
    if (err_out) HIP_TRY(s->err.ensure(n));
  }
  int rc = pol.prepare();
  if (!rc) rc = ensure_copy_stream(s);
  if (!rc) rc = ensure_event(&s->ev_update);
  if (rc) return rc;
  DrainOnExit drain;
  ptx_stats acc, one;
  std::memset(&acc, 0, sizeof acc);
  fill_tree_stats(s, &acc);
  int64_t samples = 0, samples_done = 0; /* queued so far; in the sums the last update was made from */
  const bool ahead = !p.count_work && !p.time_kernels;
  auto queue_slice = [&](const PassRange& r) -> int {
    ptx_render_params pq = p;
    pq.flags = PTX_RENDER_ASYNC;
    const int r2 = render_raw(s, &pq, s->raw.p, nullptr, &one, nullptr, nullptr, nullptr, r);
    if (r2) return r2;
    add_slice_stats(&acc, one);
    samples += one.samples;
    /* a slice over the whole image sets the whole count map */
    if (r.d_passes && !r.d_list) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)r.d_passes, r.first + r.count, (size_t)npix, nullptr));
    return 0;
  };
  PassRange cur = pol.first(), next;
  rc = queue_slice(cur);
  if (rc) return rc;
  double rel = std::nan("");
  for (int update = 1;; ++update) {
    rc = pol.queue_update(cur);
    if (!rc && job) rc = display_scene_image(s, *job, npix, nullptr);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s->ev_update, nullptr));
    rc = pol.next_slice(cur, &next);
    if (rc) return rc;
    samples_done = samples;
    if (next.count > 0 && ahead) {
      rc = queue_slice(next);
      if (rc) return rc;
    }
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_update, 0));
    if (job) rc = image_bytes_to_host(s, (const char*)s->disp.p, (char*)job->out, (size_t)npix * job->pixel_bytes, s->copy_stream);
    else rc = framebuffer_to_host(s, s->rgb.p, rgb_out, n, s->copy_stream);
    if (rc) return rc;
    if (err_out) {
      rc = framebuffer_to_host(s, s->err.p, err_out, n, s->copy_stream);
      if (rc) return rc;
    }
    rc = pol.copy_extras(s->copy_stream);
    if (rc) return rc;
    if (want_err) {
      HIP_TRY(hipMemcpyAsync(&rel, s->err_partials.p + 2 * pixel_error_blocks(npix), sizeof rel, hipMemcpyDeviceToHost, s->copy_stream));
      HIP_TRY(hipStreamSynchronize(s->copy_stream));
    }
    if (pol.call_back(update, cur, next, samples_done, rel) || next.count <= 0) break;
    if (!ahead) {
      rc = queue_slice(next);
      if (rc) return rc;
    }
    cur = next;
  }
  /* (after an early stop the slice queued ahead finishes here; its passes are in the raw sums only, never in rgb_out) */
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipStreamSynchronize(s->copy_stream));
  drain.armed = false;
  if (stats) {
    *stats = acc;
    stats->samples = samples_done; /* W*H*k; with a count map, its sum */
    stats->render_ms = wall_ms() - t0;
  }
  return 0;
}

/* every index of the DEVICE list in [0, npix), checked on the device before anything else is queued (waits for st) */
int check_list_device(ptx_scene* s, const int32_t* d_list, long long n, long long npix, hipStream_t st) {
  HIP_TRY(s->sel_n.ensure(2)); /* [1]: the flag */
  HIP_TRY(hipMemsetAsync(s->sel_n.p + 1, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_list_check, grid256(n), dim3(256), 0, st, d_list, n, npix, s->sel_n.p + 1);
  HIP_TRY(hipGetLastError());
  int32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, s->sel_n.p + 1, sizeof bad, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) return fail(PTX_ERR_ARG, "the pixel list holds an index outside [0, %lld)", npix);
  return 0;
}

/* ptx_pixel_error_device and ptx_pixel_error_counts_device (d_passes == nullptr: passes_done for every pixel); the caller has
 * checked its own arguments */
int pixel_error_device(int32_t device, int32_t width, int32_t rows, int32_t passes_done, const int32_t* d_passes, const double* d_raw,
                       const double* d_sq, double* d_err_out, double* rel_err_out, hipStream_t st) {
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  const long long npix = (long long)width * rows;
  DevBuf<double> part;
  HIP_TRY(part.ensure(pixel_error_partials(npix)));
  rc = pixel_error_queue(npix, passes_done, d_passes, d_raw, d_sq, d_err_out, part.p, st);
  if (rc) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  double rel = 0.0;
  HIP_TRY(hipMemcpyAsync(&rel, part.p + 2 * pixel_error_blocks(npix), sizeof rel, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (rel_err_out) *rel_err_out = rel;
  return 0;
}
}  // namespace

int32_t ptx_render_passes_device(ptx_scene* s, const ptx_render_params* p, int32_t pass_first, int32_t pass_count,
                                 double* d_raw_inout, double* d_sq_inout, void* stream, ptx_stats* stats) {
  int rc = check_render_args(s, p, d_raw_inout ? nullptr : "d_raw_inout is NULL");
  if (rc) return rc;
  rc = check_pass_range(p, pass_first, pass_count);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const double t0 = wall_ms();
  rc = render_raw(s, p, d_raw_inout, (hipStream_t)stream, stats, nullptr, nullptr, nullptr, PassRange(pass_first, pass_count, false, d_sq_inout));
  if (rc) return rc;
  if (stats) stats->render_ms = wall_ms() - t0;
  return 0;
}

int32_t ptx_pixel_error_device(int32_t device, int32_t width, int32_t rows, int32_t passes_done, const double* d_raw,
                               const double* d_sq, double* d_err_out, double* rel_err_out, void* stream) {
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: the error kernels run on a HIP device only, no CPU fallback exists", device);
  if (!d_raw || !d_sq) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || rows <= 0) return fail(PTX_ERR_ARG, "bad dimensions (%d x %d)", width, rows);
  if (passes_done < 1) return fail(PTX_ERR_ARG, "passes_done must be >= 1 (got %d)", passes_done);
  return pixel_error_device(device, width, rows, passes_done, nullptr, d_raw, d_sq, d_err_out, rel_err_out, (hipStream_t)stream);
}

namespace {
/* ptx_render_progressive as render_updates sees it: slices of K passes over the whole image, k_film with spp = the passes done */
struct ProgressivePolicy {
  ptx_scene* s;
  const ptx_render_params& p;
  const ptx_progressive_params& pp;
  double *rgb_out, *err_out;
  int32_t* passes_done_out;
  ptx_update_fn on_update;
  void* user;
  bool want_err() const { return pp.want_error != 0; }
  PassRange slice(int first) const {
    return PassRange(first, std::min(pp.passes_per_update, p.samples_per_pixel - first), first == 0, want_err() ? s->sq.p : nullptr);
  }
  int prepare() { return 0; }
  PassRange first() const { return slice(0); }
  int queue_update(const PassRange& cur) {
    const int k = cur.first + cur.count;
    const int rc = film_resolve(p.width, p.height, k, s->raw.p, s->rgb.p, nullptr, PtBandMap{1, 1, 0}, 0, -1, s->film);
    if (rc || !want_err()) return rc;
    return pixel_error_queue((long long)p.width * p.height, k, nullptr, s->raw.p, s->sq.p, err_out ? s->err.p : nullptr, s->err_partials.p, nullptr);
  }
  int next_slice(const PassRange& cur, PassRange* next) {
    *next = slice(cur.first + cur.count);
    return 0;
  }
  int copy_extras(hipStream_t) { return 0; }
  bool call_back(int, const PassRange& cur, const PassRange&, int64_t, double rel) {
    const int k = cur.first + cur.count;
    if (passes_done_out) *passes_done_out = k;
    const bool stop = on_update && on_update(user, k, rel, rgb_out, err_out) != 0;
    return stop || (want_err() && pp.target_rel_err > 0.0 && rel <= pp.target_rel_err);
  }
};
}  // namespace

namespace {
/* The callback of a display render behind the f64 policies' ptx_update_fn: the policies hand it their rgb_out (NULL under a display
 * job); the caller's function gets the display image instead. */
struct DisplayUpdate {
  ptx_update_display_fn fn;
  void* user;
  const void* pixels;
  static int32_t call(void* self, int32_t passes_done, double rel_err, const double*, const double* err) {
    const DisplayUpdate* u = (const DisplayUpdate*)self;
    return u->fn(u->user, passes_done, rel_err, u->pixels, err);
  }
};
}  // namespace

/* ptx_render_progressive, and with `job` ptx_render_progressive_display without denoise (rgb_out is then not read) */
static int32_t render_progressive(ptx_scene* s, const ptx_render_params* p_in, const ptx_progressive_params* pp, double* rgb_out,
                                  const DisplayJob* job, double* err_out, int32_t* passes_done_out, ptx_stats* stats, ptx_update_fn on_update,
                                  void* user) {
  int rc = check_render_args(s, p_in, (pp && (job ? job->out : (void*)rgb_out)) ? nullptr : "NULL argument");
  if (rc) return rc;
  if (p_in->n_gpus > 1) return fail(PTX_ERR_ARG, "progressive rendering runs on one GPU (n_gpus %d)", p_in->n_gpus);
  if (pp->passes_per_update < 1) return fail(PTX_ERR_ARG, "passes_per_update must be >= 1 (got %d)", pp->passes_per_update);
  if (!(pp->target_rel_err >= 0.0)) return fail(PTX_ERR_ARG, "target_rel_err must be >= 0 (got %g)", pp->target_rel_err);
  if (!pp->want_error && (pp->target_rel_err > 0.0 || err_out))
    return fail(PTX_ERR_ARG, "target_rel_err and err_out need want_error");
  if (passes_done_out) *passes_done_out = 0;
  ptx_render_params p = *p_in;
  p.band_step = 0; /* whole image on this GPU */
  p.n_gpus = 0;
  HIP_TRY(hipSetDevice(s->device));
  ProgressivePolicy pol{s, p, *pp, rgb_out, err_out, passes_done_out, on_update, user};
  return render_updates(s, p, pol, pol.want_err(), rgb_out, err_out, stats, job);
}

int32_t ptx_render_progressive(ptx_scene* s, const ptx_render_params* p_in, const ptx_progressive_params* pp, double* rgb_out,
                               double* err_out, int32_t* passes_done_out, ptx_stats* stats, ptx_update_fn on_update, void* user) {
  return render_progressive(s, p_in, pp, rgb_out, nullptr, err_out, passes_done_out, stats, on_update, user);
}

/* ---- adaptive sampling: rounds of passes for the pixels that have not converged yet ---- */
int32_t ptx_render_pixels_device(ptx_scene* s, const ptx_render_params* p, int32_t pass_first, int32_t pass_count,
                                 const int32_t* d_pixels, int64_t n_pixels, double* d_raw_inout, double* d_sq_inout, void* stream,
                                 ptx_stats* stats) {
  int rc = check_render_args(s, p, d_raw_inout ? nullptr : "d_raw_inout is NULL");
  if (rc) return rc;
  rc = check_one_gpu(p, "a pixel list");
  if (rc) return rc;
  rc = check_pass_range(p, pass_first, pass_count);
  if (rc) return rc;
  const long long npix = (long long)p->width * p->height;
  if (n_pixels < 0 || n_pixels > npix) return fail(PTX_ERR_ARG, "n_pixels %lld is outside [0, %lld]", (long long)n_pixels, npix);
  if (n_pixels > 0 && !d_pixels) return fail(PTX_ERR_ARG, "d_pixels is NULL");
  HIP_TRY(hipSetDevice(s->device));
  const double t0 = wall_ms();
  if (n_pixels == 0) {
    if (stats) {
      std::memset(stats, 0, sizeof *stats);
      fill_tree_stats(s, stats);
    }
    return 0;
  }
  rc = check_list_device(s, d_pixels, n_pixels, npix, (hipStream_t)stream);
  if (rc) return rc;
  rc = render_raw(s, p, d_raw_inout, (hipStream_t)stream, stats, nullptr, nullptr, nullptr,
                  PassRange(pass_first, pass_count, false, d_sq_inout).listed(d_pixels, n_pixels, nullptr));
  if (rc) return rc;
  if (stats) stats->render_ms = wall_ms() - t0;
  return 0;
}

int32_t ptx_film_resolve_counts_device(int32_t device, int32_t width, int32_t height, const double* d_raw, const int32_t* d_passes,
                                       double* d_rgb_out, void* stream) {
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: the film runs on a HIP device only, no CPU fallback exists", device);
  if (!d_raw || !d_passes || !d_rgb_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || height <= 0) return fail(PTX_ERR_ARG, "bad dimensions (%d x %d)", width, height);
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  rc = film_counts_queue(width, height, d_raw, d_passes, d_rgb_out, (hipStream_t)stream);
  (void)hipStreamSynchronize((hipStream_t)stream);
  return rc;
}

int32_t ptx_film_resolve_counts_ex_device(int32_t device, int32_t width, int32_t height, const ptx_film_params* film, const double* d_raw,
                                          const int32_t* d_passes, double* d_rgb_out, void* stream) {
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: the film runs on a HIP device only, no CPU fallback exists", device);
  if (!d_raw || !d_passes || !d_rgb_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || height <= 0) return fail(PTX_ERR_ARG, "bad dimensions (%d x %d)", width, height);
  const ptx_film_params f = film ? *film : kFilmDefault;
  int rc = film_check(&f);
  if (rc) return rc;
  rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  rc = film_counts_queue(width, height, d_raw, d_passes, d_rgb_out, (hipStream_t)stream, f);
  (void)hipStreamSynchronize((hipStream_t)stream);
  return rc;
}

int32_t ptx_pixel_error_counts_device(int32_t device, int32_t width, int32_t rows, const int32_t* d_passes, const double* d_raw,
                                      const double* d_sq, double* d_err_out, double* rel_err_out, void* stream) {
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: the error kernels run on a HIP device only, no CPU fallback exists", device);
  if (!d_passes || !d_raw || !d_sq) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || rows <= 0) return fail(PTX_ERR_ARG, "bad dimensions (%d x %d)", width, rows);
  return pixel_error_device(device, width, rows, 0, d_passes, d_raw, d_sq, d_err_out, rel_err_out, (hipStream_t)stream);
}

namespace {
/* ptx_render_adaptive as render_updates sees it.  A round over the whole image is a plain slice (camera rays decoded in k_bounce), a
 * partial one runs in list mode.  After round j: the film, the error and a copy of the count map, then the select of round j + 1's
 * list.  The host waits for the select only (it needs the list's length to size the next round); render_updates then queues round
 * j + 1, and copies update j out on copy_stream and calls back while round j + 1's bounces run. */
struct AdaptivePolicy {
  ptx_scene* s;
  const ptx_render_params& p;
  const ptx_adaptive_params& ap;
  double *rgb_out, *err_out;
  int32_t* passes_out;
  ptx_round_fn on_round;
  void* user;
  bool selecting = false; /* queue_update queued a select: next_slice waits for it */
  long long npix() const { return (long long)p.width * p.height; }
  int tiles_x() const { return (p.width + 7) / 8; }
  long long padded() const { return (long long)tiles_x() * ((p.height + 7) / 8) * 64; } /* the whole image in 8x8-tile order */
  PassRange round(int first, int count, const int32_t* list, long long n_list) const {
    return PassRange(first, count, first == 0, s->sq.p).listed(list, n_list, s->passes.p);
  }
  /* the list the round after cur is selected into: the buffer that does not hold cur's */
  int32_t* next_list(const PassRange& cur) const { return s->list[cur.d_list == s->list[0].p ? 1 : 0].p; }
  int prepare() {
    const size_t max_blocks = (size_t)((padded() + PT_SEL_THREADS - 1) / PT_SEL_THREADS);
    HIP_TRY(s->passes.ensure((size_t)npix()));
    HIP_TRY(s->passes_img.ensure((size_t)npix()));
    HIP_TRY(s->list[0].ensure((size_t)npix()));
    HIP_TRY(s->list[1].ensure((size_t)npix()));
    HIP_TRY(s->sel_n.ensure(2));
    HIP_TRY(s->sel_keep.ensure((size_t)padded()));
    HIP_TRY(s->sel_blocks.ensure(max_blocks));
    HIP_TRY(s->sel_offsets.ensure(max_blocks));
    return ensure_event(&s->ev_select);
  }
  PassRange first() const { return round(0, std::min(ap.min_passes, p.samples_per_pixel), nullptr, 0); }
  int queue_update(const PassRange& cur) {
    const int W = p.width, H = p.height, b = cur.first + cur.count;
    int rc = film_counts_queue(W, H, s->raw.p, s->passes.p, s->rgb.p, nullptr, s->film);
    if (rc) return rc;
    rc = pixel_error_queue(npix(), 0, s->passes.p, s->raw.p, s->sq.p, err_out ? s->err.p : nullptr, s->err_partials.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s->passes_img.p, s->passes.p, sizeof(int32_t) * (size_t)npix(), hipMemcpyDeviceToDevice, nullptr));
    selecting = b < p.samples_per_pixel && ap.target_rel_err > 0.0; /* T = 0: no pixel converges */
    if (!selecting) return 0;
    const long long n_sel = cur.d_list ? cur.n_list : padded();
    const unsigned nb = (unsigned)((n_sel + PT_SEL_THREADS - 1) / PT_SEL_THREADS);
    hipLaunchKernelGGL(k_select_count, dim3(nb), dim3(PT_SEL_THREADS), 0, nullptr, cur.d_list, n_sel, W, H, tiles_x(), (const double*)s->raw.p,
                       (const double*)s->sq.p, b, ap.target_rel_err, ap.radiance_floor, s->sel_keep.p, s->sel_blocks.p);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(PT_SEL_THREADS), 0, nullptr, (const uint32_t*)s->sel_blocks.p, (long long)nb,
                       s->sel_offsets.p, s->sel_n.p);
    hipLaunchKernelGGL(k_select_scatter, dim3(nb), dim3(PT_SEL_THREADS), 0, nullptr, cur.d_list, n_sel, W, H, tiles_x(),
                       (const uint8_t*)s->sel_keep.p, (const uint32_t*)s->sel_offsets.p, next_list(cur));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev_select, nullptr));
    return 0;
  }
  int next_slice(const PassRange& cur, PassRange* next) {
    const int b = cur.first + cur.count, count = std::min(ap.passes_per_round, p.samples_per_pixel - b);
    long long n_next = cur.d_list ? cur.n_list : npix();
    if (selecting) {
      int32_t got = 0;
      HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_select, 0));
      HIP_TRY(hipMemcpyAsync(&got, s->sel_n.p, sizeof got, hipMemcpyDeviceToHost, s->copy_stream));
      HIP_TRY(hipStreamSynchronize(s->copy_stream));
      n_next = got;
    }
    /* a list that holds the whole image runs as a plain slice; an empty one ends the render */
    const bool whole = !selecting || n_next == npix();
    *next = round(b, n_next > 0 ? count : 0, whole ? nullptr : next_list(cur), n_next);
    return 0;
  }
  int copy_extras(hipStream_t cs) {
    if (passes_out) HIP_TRY(hipMemcpyAsync(passes_out, s->passes_img.p, sizeof(int32_t) * (size_t)npix(), hipMemcpyDeviceToHost, cs));
    return 0;
  }
  bool call_back(int update, const PassRange& cur, const PassRange& next, int64_t samples, double rel) {
    const long long active_next = next.count <= 0 ? 0 : next.d_list ? next.n_list : npix();
    return on_round && on_round(user, update, cur.first + cur.count, active_next, samples, rel, rgb_out, err_out, passes_out) != 0;
  }
};
}  // namespace

int32_t ptx_render_adaptive(ptx_scene* s, const ptx_render_params* p_in, const ptx_adaptive_params* ap, double* rgb_out,
                            double* err_out, int32_t* passes_out, ptx_stats* stats, ptx_round_fn on_round, void* user) {
  int rc = check_render_args(s, p_in, (ap && rgb_out) ? nullptr : "NULL argument");
  if (rc) return rc;
  rc = check_one_gpu(p_in, "adaptive rendering");
  if (rc) return rc;
  if (ap->min_passes < 2) return fail(PTX_ERR_ARG, "min_passes must be >= 2 (got %d)", ap->min_passes);
  if (ap->passes_per_round < 1) return fail(PTX_ERR_ARG, "passes_per_round must be >= 1 (got %d)", ap->passes_per_round);
  if (!(ap->target_rel_err >= 0.0)) return fail(PTX_ERR_ARG, "target_rel_err must be >= 0 (got %g)", ap->target_rel_err);
  if (!(ap->radiance_floor >= 0.0)) return fail(PTX_ERR_ARG, "radiance_floor must be >= 0 (got %g)", ap->radiance_floor);
  ptx_render_params p = *p_in;
  p.band_step = 0;
  p.n_gpus = 0;
  HIP_TRY(hipSetDevice(s->device));
  AdaptivePolicy pol{s, p, *ap, rgb_out, err_out, passes_out, on_round, user};
  return render_updates(s, p, pol, true, rgb_out, err_out, stats);
}

/* ---- first-hit feature sums and the a-trous denoiser (kernels: denoise.inc; the rule: include/ptx.h) ---- */
namespace {
/* Passes [pass_first, pass_first + pass_count) of the frame's camera rays -> d_feat, queued on st.  A batch of passes is one PRIMARY
 * launch of the unchanged k_trace (launch_trace: LDS-resident scenes and scenes walked from HBM / L2 alike; the camera rays are
 * never written anywhere) that keeps slot and distance per entry, then k_features, which computes every ray again and adds the
 * batch's records per pixel in pass order.  12 bytes per sample in flight; the batches of a call run one after the other. */
int features_queue(ptx_scene* s, const ptx_render_params* p, int pass_first, int pass_count, double* d_feat, hipStream_t st) {
  const int tiles_x = (p->width + 7) / 8, tiles_y = (p->height + 7) / 8;
  const unsigned long long padded = (unsigned long long)tiles_x * (unsigned long long)tiles_y * 64ull; /* entries of one pass */
  if (padded >= 0xffffffffull) return fail(PTX_ERR_ARG, "too many pixels for one feature pass");
  long long ppb = p->passes_per_batch > 0 ? p->passes_per_batch : std::max<long long>(1, (16ll << 20) / (long long)padded);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) /* 12 bytes of hit record per entry: below a quarter of what is free */
    ppb = std::min<long long>(ppb, std::max<long long>(1, (long long)(free_b / 4 / 12 / padded)));
  ppb = std::max<long long>(1, std::min<long long>(ppb, pass_count));
  while (ppb > 1 && (unsigned long long)ppb * padded >= 0xffffffffull) --ppb; /* entry indices are 32-bit */
  const size_t cap = (size_t)ppb * (size_t)padded;
  HIP_TRY(s->feat_slot.ensure(cap));
  if (!s->dev.has_triangles) HIP_TRY(s->feat_t.ensure(cap));
  const bool lens = s->sched.lens || s->sched.pose; /* (rays with an origin: generated into a queue of their own) */
  if (lens) HIP_TRY(s->feat_ray.ensure(cap));
  HIP_TRY(s->feat_work.ensure(16)); /* [0..7] k_trace's hand-out words, [8] the entry count of a lens's ray queue */
  HIP_TRY(s->feat_susp.ensure((size_t)s->n_cu * 4 * 16 * PT_WAVE * 3)); /* as a workspace set's (ensure_workspace) */
  HIP_TRY(s->counters.ensure(1));
  int rc = use_alpha_table(s, sampler_dimension(s, p->max_bounces));
  if (rc) return rc;
  const double* alpha = s->alpha.p;
  PtHits h{};
  h.t = s->dev.has_triangles ? nullptr : s->feat_t.p; /* with triangles k_features recomputes (t, u, v), as a render's shade step does */
  h.slot = s->feat_slot.p;
  for (int first = pass_first; first < pass_first + pass_count; first += (int)ppb) {
    const int n_pass = std::min<int>((int)ppb, pass_first + pass_count - first);
    PrimaryLaunch pl;
    pl.on = true;
    PtGenParams& g = pl.g;
    g.width = p->width; g.height = p->height; g.spp = p->samples_per_pixel; g.local_rows = p->height;
    g.band_rows = 32; g.band_first = 0; g.band_step = 0;
    g.tiles_x = tiles_x; g.tiles_y = tiles_y;
    g.first_pass = first; g.n_pass = n_pass;
    pl.n = (uint32_t)((unsigned long long)n_pass * padded);
    HIP_TRY(hipMemsetAsync(s->feat_work.p, 0, sizeof(uint32_t) * 8, st));
    if (lens) {
      /* the same entries as rays in a queue of their own (48 bytes per entry more), walked as ptx_intersect_rays' are */
      PtQueue q{s->feat_ray.p, nullptr, s->feat_work.p + 8};
      launch_generate_tiles(s, p, pl, false, q, st);
      launch_trace(s, st, q, h, (size_t)pl.n, false, s->feat_work.p, s->feat_susp.p, kNoBounce);
      hipLaunchKernelGGL(s->sched.img ? k_features_queue<true> : k_features_queue<false>, grid256(padded), dim3(256), 0, st, s->dev, g, q, h, d_feat);
      HIP_TRY(hipGetLastError());
      continue;
    }
    launch_trace(s, st, PtQueue{}, h, (size_t)pl.n, false, s->feat_work.p, s->feat_susp.p, 0, pl);
    hipLaunchKernelGGL(s->sched.img ? k_features<true> : k_features<false>, grid256(padded), dim3(256), 0, st, s->dev, g, h, alpha, d_feat);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int check_denoise_params(const ptx_denoise_params* d) {
  if (d->levels < 0 || d->levels > 8) return fail(PTX_ERR_ARG, "levels must be in [0, 8] (got %d)", d->levels);
  if (d->normal_power_log2 < 0 || d->normal_power_log2 > 8)
    return fail(PTX_ERR_ARG, "normal_power_log2 must be in [0, 8] (got %d)", d->normal_power_log2);
  if (d->feature_passes < 0) return fail(PTX_ERR_ARG, "feature_passes must be >= 0 (got %d)", d->feature_passes);
  if (d->flags & ~PTX_DENOISE_DEMODULATE) return fail(PTX_ERR_ARG, "unknown bits in the denoiser's flags (0x%x)", (unsigned)d->flags);
  const double sg[3] = {d->sigma_luminance, d->sigma_depth, d->sigma_albedo};
  for (double v : sg)
    if (!(v > 0.0) || !std::isfinite(v)) return fail(PTX_ERR_ARG, "sigma_luminance, sigma_depth and sigma_albedo must be > 0 and finite (got %g)", v);
  return 0;
}

/* prepare, one k_atrous per level, finish, queued on st; guide holds W*H*8 doubles, cv0 and cv1 W*H*4 each (the levels' ping-pong) */
int denoise_queue(int width, int height, const ptx_denoise_params& d, int k, const int32_t* d_passes, int kf, const double* d_raw,
                  const double* d_err, const double* d_feat, double* guide, double* cv0, double* cv1, double* d_out, hipStream_t st) {
  const long long npix = (long long)width * height;
  if (d.levels == 0) {
    HIP_TRY(hipMemcpyAsync(d_out, d_raw, sizeof(double) * (size_t)npix * 3, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  PtDenoise dn;
  dn.width = width; dn.height = height; dn.m = d.normal_power_log2; dn.demodulate = (d.flags & PTX_DENOISE_DEMODULATE) ? 1 : 0;
  dn.sl2 = d.sigma_luminance * d.sigma_luminance; dn.sz = d.sigma_depth; dn.sa2 = d.sigma_albedo * d.sigma_albedo;
  const dim3 lin(grid256(npix)), tiles((unsigned)((width + PT_ATROUS_TX - 1) / PT_ATROUS_TX), (unsigned)((height + PT_ATROUS_TY - 1) / PT_ATROUS_TY));
  double4* cv[2] = {(double4*)cv0, (double4*)cv1};
  hipLaunchKernelGGL(k_denoise_prepare, lin, dim3(256), 0, st, dn, k, d_passes, (double)kf, d_raw, d_err, d_feat, (PtGuide*)guide, cv[0]);
  /* how a level fetches its taps: the tile and its halo through LDS at steps <= PTX_ATROUS_LDS (0 .. PT_ATROUS_LDS_STEP), gathers
   * through L1 / L2 above -- the same bits either way.  Default 1: measured, the LDS copy wins at step 1 and ties at step 2
   * (DESIGN.md section 8, tools/denoise_cost.py) */
  const int lds_steps = std::max(0, std::min(PT_ATROUS_LDS_STEP, env_int("PTX_ATROUS_LDS", 1)));
  for (int l = 0; l < d.levels; ++l) {
    const int step = 1 << l;
    auto kern = step <= lds_steps ? k_atrous<true> : k_atrous<false>;
    hipLaunchKernelGGL(kern, tiles, dim3(PT_ATROUS_TX * PT_ATROUS_TY), 0, st, dn, step, (const PtGuide*)guide, (const double4*)cv[l & 1], cv[(l + 1) & 1]);
  }
  hipLaunchKernelGGL(k_denoise_finish, lin, dim3(256), 0, st, dn, k, d_passes, (const PtGuide*)guide, (const double4*)cv[d.levels & 1], d_out);
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace

int32_t ptx_render_features_device(ptx_scene* s, const ptx_render_params* p, int32_t pass_first, int32_t pass_count,
                                   double* d_feat_inout, void* stream, ptx_stats* stats) {
  int rc = check_render_args(s, p, d_feat_inout ? nullptr : "d_feat_inout is NULL");
  if (rc) return rc;
  rc = check_one_gpu(p, "a feature pass");
  if (rc) return rc;
  rc = check_pass_range(p, pass_first, pass_count);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  RenderBusy busy(s);
  const double t0 = wall_ms();
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    fill_tree_stats(s, stats);
  }
  rc = features_queue(s, p, pass_first, pass_count, d_feat_inout, (hipStream_t)stream);
  if (rc) {
    (void)hipStreamSynchronize((hipStream_t)stream);
    return rc;
  }
  if (!(p->flags & PTX_RENDER_ASYNC)) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (stats) {
    stats->samples = (int64_t)p->width * p->height * pass_count;
    stats->render_ms = wall_ms() - t0;
  }
  return 0;
}

int32_t ptx_denoise_defaults(ptx_denoise_params* out) {
  if (!out) return fail(PTX_ERR_ARG, "NULL argument");
  out->levels = 5;
  out->normal_power_log2 = 5;
  out->feature_passes = 8;
  out->flags = PTX_DENOISE_DEMODULATE;
  out->sigma_luminance = 4.0;
  out->sigma_depth = 0.05;
  out->sigma_albedo = 0.2;
  return 0;
}

int32_t ptx_denoise_device(int32_t device, int32_t width, int32_t height, const ptx_denoise_params* d, int32_t passes_done,
                           const int32_t* d_passes, int32_t feature_passes_done, const double* d_raw, const double* d_err,
                           const double* d_feat, double* d_raw_out, void* stream) {
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: the denoiser runs on a HIP device only, no CPU fallback exists", device);
  if (!d || !d_raw || !d_err || !d_feat || !d_raw_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (d_raw_out == d_raw) return fail(PTX_ERR_ARG, "d_raw_out must not be d_raw");
  if (width <= 0 || height <= 0) return fail(PTX_ERR_ARG, "bad dimensions (%d x %d)", width, height);
  int rc = check_denoise_params(d);
  if (rc) return rc;
  if (!d_passes && passes_done < 2) return fail(PTX_ERR_ARG, "passes_done must be >= 2 (got %d): the error of fewer passes is infinite", passes_done);
  if (feature_passes_done < 1) return fail(PTX_ERR_ARG, "feature_passes_done must be >= 1 (got %d)", feature_passes_done);
  rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t npix = (size_t)width * (size_t)height;
  DevBuf<double> guide, cv0, cv1;
  if (d->levels > 0) {
    HIP_TRY(guide.ensure(npix * 8));
    HIP_TRY(cv0.ensure(npix * 4));
    HIP_TRY(cv1.ensure(npix * 4));
  }
  rc = denoise_queue(width, height, *d, passes_done, d_passes, feature_passes_done, d_raw, d_err, d_feat, guide.p, cv0.p, cv1.p, d_raw_out,
                     (hipStream_t)stream);
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream); /* (also on an error: the scratch buffers go with this frame) */
  if (rc) return rc;
  HIP_TRY(e);
  return 0;
}

namespace {
/* ptx_render_denoised as render_updates sees it: ProgressivePolicy with the squares always kept, a feature slice beside every slice
 * while it starts below F, and an update that films the DENOISED sums */
struct DenoisePolicy {
  ptx_scene* s;
  const ptx_render_params& p;
  const ptx_progressive_params& pp;
  const ptx_denoise_params& dp;
  double *rgb_out, *err_out, *feat_out;
  int32_t* passes_done_out;
  ptx_update_fn on_update;
  void* user;
  long long npix() const { return (long long)p.width * p.height; }
  int feature_end() const { return dp.feature_passes > 0 ? std::min(dp.feature_passes, p.samples_per_pixel) : p.samples_per_pixel; }
  PassRange slice(int first) const {
    return PassRange(first, std::min(pp.passes_per_update, p.samples_per_pixel - first), first == 0, s->sq.p);
  }
  int prepare() {
    const size_t n = (size_t)npix();
    HIP_TRY(s->err.ensure(n * 3)); /* the filter's input, whether the caller wants it or not */
    HIP_TRY(s->feat.ensure(n * 8));
    if (feat_out) HIP_TRY(s->feat_mean.ensure(n * 8));
    HIP_TRY(s->den_raw.ensure(n * 3));
    HIP_TRY(s->den_guide.ensure(n * 8));
    HIP_TRY(s->den_cv[0].ensure(n * 4));
    HIP_TRY(s->den_cv[1].ensure(n * 4));
    HIP_TRY(hipMemsetAsync(s->feat.p, 0, sizeof(double) * n * 8, nullptr));
    return 0;
  }
  PassRange first() const { return slice(0); }
  int queue_update(const PassRange& cur) {
    const int k = cur.first + cur.count, F = feature_end(), kf = std::min(F, k);
    int rc = 0;
    if (cur.first < F) rc = features_queue(s, &p, cur.first, kf - cur.first, s->feat.p, nullptr);
    if (!rc) rc = pixel_error_queue(npix(), k, nullptr, s->raw.p, s->sq.p, s->err.p, s->err_partials.p, nullptr);
    if (!rc) rc = denoise_queue(p.width, p.height, dp, k, nullptr, kf, s->raw.p, s->err.p, s->feat.p, s->den_guide.p, s->den_cv[0].p, s->den_cv[1].p,
                                s->den_raw.p, nullptr);
    if (!rc) rc = film_resolve(p.width, p.height, k, s->den_raw.p, s->rgb.p, nullptr, PtBandMap{1, 1, 0}, 0, -1, s->film);
    if (rc || !feat_out) return rc;
    const long long n = npix() * 8;
    hipLaunchKernelGGL(k_feature_means, grid256(n), dim3(256), 0, nullptr, (const double*)s->feat.p, n, (double)kf, s->feat_mean.p);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  int next_slice(const PassRange& cur, PassRange* next) {
    *next = slice(cur.first + cur.count);
    return 0;
  }
  int copy_extras(hipStream_t cs) {
    if (feat_out) HIP_TRY(hipMemcpyAsync(feat_out, s->feat_mean.p, sizeof(double) * (size_t)npix() * 8, hipMemcpyDeviceToHost, cs));
    return 0;
  }
  bool call_back(int, const PassRange& cur, const PassRange&, int64_t, double rel) {
    const int k = cur.first + cur.count;
    if (passes_done_out) *passes_done_out = k;
    const bool stop = on_update && on_update(user, k, rel, rgb_out, err_out) != 0;
    return stop || (pp.target_rel_err > 0.0 && rel <= pp.target_rel_err);
  }
};
}  // namespace

/* ptx_render_denoised, and with `job` ptx_render_progressive_display with denoise (rgb_out is then not read) */
static int32_t render_denoised(ptx_scene* s, const ptx_render_params* p_in, const ptx_progressive_params* pp, const ptx_denoise_params* dp,
                               double* rgb_out, const DisplayJob* job, double* err_out, double* feat_out, int32_t* passes_done_out,
                               ptx_stats* stats, ptx_update_fn on_update, void* user) {
  int rc = check_render_args(s, p_in, (pp && dp && (job ? job->out : (void*)rgb_out)) ? nullptr : "NULL argument");
  if (rc) return rc;
  rc = check_one_gpu(p_in, "denoised rendering");
  if (rc) return rc;
  if (pp->passes_per_update < 2) return fail(PTX_ERR_ARG, "passes_per_update must be >= 2 (got %d): the filter needs the error of every update", pp->passes_per_update);
  if (p_in->samples_per_pixel < 2) return fail(PTX_ERR_ARG, "samples_per_pixel must be >= 2 (got %d): the error of one pass is infinite", p_in->samples_per_pixel);
  if (!(pp->target_rel_err >= 0.0)) return fail(PTX_ERR_ARG, "target_rel_err must be >= 0 (got %g)", pp->target_rel_err);
  rc = check_denoise_params(dp);
  if (rc) return rc;
  if (passes_done_out) *passes_done_out = 0;
  ptx_render_params p = *p_in;
  p.band_step = 0; /* whole image on this GPU */
  p.n_gpus = 0;
  HIP_TRY(hipSetDevice(s->device));
  DenoisePolicy pol{s, p, *pp, *dp, rgb_out, err_out, feat_out, passes_done_out, on_update, user};
  return render_updates(s, p, pol, true, rgb_out, err_out, stats, job);
}

int32_t ptx_render_denoised(ptx_scene* s, const ptx_render_params* p_in, const ptx_progressive_params* pp, const ptx_denoise_params* dp,
                            double* rgb_out, double* err_out, double* feat_out, int32_t* passes_done_out, ptx_stats* stats,
                            ptx_update_fn on_update, void* user) {
  return render_denoised(s, p_in, pp, dp, rgb_out, nullptr, err_out, feat_out, passes_done_out, stats, on_update, user);
}

int32_t ptx_render_progressive_display(ptx_scene* s, const ptx_render_params* p_in, const ptx_progressive_params* pp,
                                       const ptx_denoise_params* dp, const ptx_display_params* display, void* out, double* err_out,
                                       int32_t* passes_done_out, ptx_stats* stats, ptx_update_display_fn on_update, void* user) {
  const int rc = check_display(display);
  if (rc) return rc;
  const DisplayJob job{*display, out, (size_t)display_pixel_bytes(display->format)};
  DisplayUpdate du{on_update, user, out};
  const ptx_update_fn fn = on_update ? DisplayUpdate::call : nullptr;
  if (dp) return render_denoised(s, p_in, pp, dp, nullptr, &job, err_out, nullptr, passes_done_out, stats, fn, &du);
  return render_progressive(s, p_in, pp, nullptr, &job, err_out, passes_done_out, stats, fn, &du);
}

/* ---- display outputs without a scene: the defaults, the table, the rule on the host and on a device ---- */
int32_t ptx_display_defaults(ptx_display_params* out) {
  if (!out) return fail(PTX_ERR_ARG, "NULL argument");
  std::memset(out, 0, sizeof *out);
  out->format = PTX_PIXEL_RGB8;
  out->transfer = PTX_TRANSFER_REFERENCE;
  out->tone = PTX_TONE_NONE;
  out->exposure = 1.0;
  return 0;
}

int32_t ptx_display_check(const ptx_display_params* display) { return check_display(display); }

int32_t ptx_display_pixel_bytes(int32_t format) {
  const int b = display_pixel_bytes(format);
  return b ? b : fail(PTX_ERR_ARG, "display: unknown format %d (PTX_PIXEL_RGB8 0, RGBA8 1, RGB32F 2, RGBA32F 3)", format);
}

int32_t ptx_display_thresholds(double out[255]) {
  if (!out) return fail(PTX_ERR_ARG, "NULL argument");
  std::memcpy(out, display_thresholds(), sizeof(double) * PT_DISPLAY_THRESHOLDS);
  return 0;
}

int32_t ptx_display_apply(const ptx_display_params* display, int64_t n_pixels, const double* rgb, void* out) {
  const int rc = check_display(display);
  if (rc) return rc;
  if (n_pixels < 0) return fail(PTX_ERR_ARG, "display: n_pixels must be >= 0 (got %lld)", (long long)n_pixels);
  if (n_pixels == 0) return 0;
  if (!rgb || !out) return fail(PTX_ERR_ARG, "NULL argument");
  display_apply_host(*display, n_pixels, rgb, out);
  return 0;
}

int32_t ptx_display_image_device(int32_t device, const ptx_display_params* display, int64_t n_pixels, const double* d_rgb, void* d_out,
                                 void* stream) {
  return ptx_display_range_device(device, display, 0, n_pixels, d_rgb, d_out, stream);
}

int32_t ptx_display_range_device(int32_t device, const ptx_display_params* display, int64_t pixel_first, int64_t n_pixels,
                                 const double* d_rgb, void* d_out, void* stream) {
  int rc = check_display(display);
  if (rc) return rc;
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: the display kernel runs on a HIP device only (the host has ptx_display_apply)", device);
  if (n_pixels < 0 || n_pixels > kMaxDisplayPixels) return fail(PTX_ERR_ARG, "display: n_pixels %lld is outside [0, 2^40]", (long long)n_pixels);
  if (pixel_first < 0 || pixel_first > kMaxDisplayPixels) return fail(PTX_ERR_ARG, "display: pixel_first %lld is outside [0, 2^40]", (long long)pixel_first);
  if (n_pixels == 0) return 0;
  if (!d_rgb || !d_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (((uintptr_t)d_rgb | (uintptr_t)d_out) & 15) return fail(PTX_ERR_ARG, "display: d_rgb and d_out must be 16-byte aligned (the kernel moves 16-byte pieces)");
  rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  rc = display_thresholds_device();
  if (rc) return rc;
  rc = display_queue(*display, pixel_first, pixel_first + n_pixels, d_rgb, d_out, (hipStream_t)stream);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

/* ---- temporal accumulation (temporal.inc; the rule: include/ptx.h) ---- */
namespace {
int check_temporal_params(const ptx_temporal_params* t) {
  const double v[4] = {t->max_history_passes, t->normal_threshold, t->depth_tolerance, t->min_weight};
  for (double a : v)
    if (!std::isfinite(a)) return fail(PTX_ERR_ARG, "temporal: max_history_passes, normal_threshold, depth_tolerance and min_weight must be finite (got %g)", a);
  if (!(t->max_history_passes >= 0.0)) return fail(PTX_ERR_ARG, "temporal: max_history_passes must be >= 0 (got %g)", t->max_history_passes);
  if (!(t->normal_threshold >= -1.0 && t->normal_threshold <= 1.0)) return fail(PTX_ERR_ARG, "temporal: normal_threshold must be in [-1, 1] (got %g)", t->normal_threshold);
  if (!(t->depth_tolerance >= 0.0)) return fail(PTX_ERR_ARG, "temporal: depth_tolerance must be >= 0 (got %g)", t->depth_tolerance);
  if (!(t->min_weight >= 0.0 && t->min_weight < 1.0)) return fail(PTX_ERR_ARG, "temporal: min_weight must be in [0, 1) (got %g)", t->min_weight);
  return 0;
}
/* a camera of the temporal rule: a pose's conditions, and a view the reprojection can divide by */
int check_temporal_camera(const ptx_temporal_camera* c, const char* which) {
  const int rc = check_camera_pose(c->origin, c->rotation, &c->view);
  if (rc) return rc;
  if (c->view.view_x == 0.0 || c->view.view_y == 0.0)
    return fail(PTX_ERR_ARG, "temporal: view_x and view_y of the %s camera must be non-zero (got %g, %g)", which, c->view.view_x, c->view.view_y);
  return 0;
}
PtCameraPose temporal_pose(const ptx_temporal_camera& c) {
  PtCameraPose cp;
  std::memcpy(cp.o, c.origin, sizeof cp.o);
  std::memcpy(cp.r, c.rotation, sizeof cp.r);
  cp.llx = c.view.lower_left_x; cp.lly = c.view.lower_left_y; cp.vx = c.view.view_x; cp.vy = c.view.view_y;
  return cp;
}
/* the camera a scene's renders launch their rays from: the pose, or origin 0, the identity and the scene's own view */
ptx_temporal_camera scene_temporal_camera(const ptx_scene* s) {
  ptx_temporal_camera c;
  std::memcpy(c.origin, s->pose_origin, sizeof c.origin);
  std::memcpy(c.rotation, s->pose_rotation, sizeof c.rotation);
  c.view = s->pose_has_view ? s->pose_view : s->own_view;
  return c;
}
/* k_temporal_accumulate queued on st behind the zeroing of d_count; checked arguments (prev == nullptr exactly when d_hist_prev is) */
int temporal_queue(int width, int height, const ptx_temporal_params& t, int k, int kf, const ptx_temporal_camera& cur,
                   const ptx_temporal_camera* prev, const double* d_raw, const double* d_sq, const double* d_feat, const double* d_hist_prev,
                   double* d_hist_out, double* d_raw_out, double* d_err_out, double* d_motion_out, unsigned long long* d_count, hipStream_t st) {
  PtTemporal tp{};
  tp.width = width; tp.height = height; tp.has_prev = d_hist_prev ? 1 : 0;
  tp.kd = (double)k; tp.kfd = (double)kf;
  tp.cap = t.max_history_passes; tp.normal_threshold = t.normal_threshold; tp.depth_tolerance = t.depth_tolerance; tp.min_weight = t.min_weight;
  tp.cur = temporal_pose(cur);
  tp.prev = temporal_pose(prev ? *prev : cur);
  HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
  const dim3 grid((unsigned)((width + PT_TEMPORAL_TX - 1) / PT_TEMPORAL_TX), (unsigned)((height + PT_TEMPORAL_TY - 1) / PT_TEMPORAL_TY));
  hipLaunchKernelGGL(k_temporal_accumulate, grid, dim3(PT_TEMPORAL_TX * PT_TEMPORAL_TY), 0, st, tp, d_raw, d_sq, d_feat, d_hist_prev, d_hist_out,
                     d_raw_out, d_err_out, d_motion_out, d_count);
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace

int32_t ptx_temporal_defaults(ptx_temporal_params* out) {
  if (!out) return fail(PTX_ERR_ARG, "NULL argument");
  out->max_history_passes = 64.0;
  out->normal_threshold = 0.9;
  out->depth_tolerance = 0.02;
  out->min_weight = 0x1p-10;
  return 0;
}

int32_t ptx_temporal_accumulate_device(int32_t device, int32_t width, int32_t height, const ptx_temporal_params* t, int32_t passes_done,
                                       int32_t feature_passes_done, const ptx_temporal_camera* cur, const ptx_temporal_camera* prev,
                                       const double* d_raw, const double* d_sq, const double* d_feat, const double* d_hist_prev,
                                       double* d_hist_out, double* d_raw_out, double* d_err_out, double* d_motion_out,
                                       int64_t* history_pixels_out, void* stream) {
  if (device < 0) return fail(PTX_ERR_STATE, "device %d: temporal accumulation runs on a HIP device only, no CPU fallback exists", device);
  if (!t || !cur || !d_raw || !d_sq || !d_feat || !d_hist_out || !d_raw_out || !d_err_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (width <= 0 || height <= 0) return fail(PTX_ERR_ARG, "bad dimensions (%d x %d)", width, height);
  if (d_hist_prev && !prev) return fail(PTX_ERR_ARG, "prev_camera may be NULL only with a NULL history");
  const size_t npix = (size_t)width * (size_t)height;
  /* no two buffers may overlap: a pixel's taps read records of the previous history that other pixels' threads would be writing */
  struct Span { const char* name; const double* p; size_t n; };
  const Span spans[8] = {{"d_raw", d_raw, npix * 3},           {"d_sq", d_sq, npix * 3},           {"d_feat", d_feat, npix * 8},
                         {"d_hist_prev", d_hist_prev, npix * 12}, {"d_hist_out", d_hist_out, npix * 12}, {"d_raw_out", d_raw_out, npix * 3},
                         {"d_err_out", d_err_out, npix * 3},   {"d_motion_out", d_motion_out, npix * 3}};
  for (int a = 0; a < 8; ++a)
    for (int b = a + 1; b < 8; ++b) {
      if (!spans[a].p || !spans[b].p) continue;
      const uintptr_t a0 = (uintptr_t)spans[a].p, a1 = a0 + spans[a].n * sizeof(double), b0 = (uintptr_t)spans[b].p, b1 = b0 + spans[b].n * sizeof(double);
      if (a0 < b1 && b0 < a1) return fail(PTX_ERR_ARG, "%s and %s must not alias", spans[a].name, spans[b].name);
    }
  if (((uintptr_t)d_feat | (uintptr_t)d_hist_prev | (uintptr_t)d_hist_out) & 15u) return fail(PTX_ERR_ARG, "d_feat, d_hist_prev and d_hist_out must be 16-byte aligned");
  if (passes_done < 2) return fail(PTX_ERR_ARG, "passes_done must be >= 2 (got %d): the error of fewer passes is infinite", passes_done);
  if (feature_passes_done < 1) return fail(PTX_ERR_ARG, "feature_passes_done must be >= 1 (got %d)", feature_passes_done);
  int rc = check_temporal_params(t);
  if (rc) return rc;
  rc = check_temporal_camera(cur, "current");
  if (rc) return rc;
  if (prev) {
    rc = check_temporal_camera(prev, "previous");
    if (rc) return rc;
  }
  rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  DevBuf<unsigned long long> count;
  HIP_TRY(count.ensure(1));
  hipStream_t st = (hipStream_t)stream;
  rc = temporal_queue(width, height, *t, passes_done, feature_passes_done, *cur, d_hist_prev ? prev : nullptr, d_raw, d_sq, d_feat, d_hist_prev,
                      d_hist_out, d_raw_out, d_err_out, d_motion_out, count.p, st);
  unsigned long long took = 0;
  hipError_t e = rc ? hipSuccess : hipMemcpyAsync(&took, count.p, sizeof took, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st); /* (also on an error: the count buffer goes with this call) */
  if (rc) return rc;
  HIP_TRY(e);
  HIP_TRY(e2);
  if (history_pixels_out) *history_pixels_out = (int64_t)took;
  return 0;
}

int32_t ptx_temporal_reset(ptx_scene* s) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the history cannot be dropped while a render runs on the scene");
  s->hist_valid = false;
  return 0;
}

int32_t ptx_render_temporal(ptx_scene* s, const ptx_render_params* p_in, const ptx_temporal_params* tp, const ptx_denoise_params* dp,
                            int32_t pass_first, int32_t pass_count, double* rgb_out, double* err_out, double* motion_out,
                            int64_t* history_pixels_out, ptx_stats* stats) {
  /* (before any device is touched: a host-only scene gets this answer too) */
  if (s && s->projection != PTX_PROJECTION_PERSPECTIVE)
    return fail(PTX_ERR_STATE, "temporal rendering needs a pinhole: its reprojection is a perspective camera's (ptx_scene_set_camera_projection(scene, PTX_PROJECTION_PERSPECTIVE) first)");
  if (s && s->shutter_on)
    return fail(PTX_ERR_STATE, "temporal rendering takes one pose per frame: its reprojection has no shutter (ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first)");
  int rc = check_render_args(s, p_in, (tp && rgb_out) ? nullptr : "NULL argument");
  if (rc) return rc;
  rc = check_one_gpu(p_in, "temporal rendering");
  if (rc) return rc;
  if (pass_count < 2) return fail(PTX_ERR_ARG, "pass_count must be >= 2 (got %d): the error of fewer passes is infinite", pass_count);
  rc = check_pass_range(p_in, pass_first, pass_count);
  if (rc) return rc;
  rc = check_temporal_params(tp);
  if (rc) return rc;
  if (dp) {
    rc = check_denoise_params(dp);
    if (rc) return rc;
  }
  if (s->lens_radius > 0.0)
    return fail(PTX_ERR_STATE, "temporal rendering needs a pinhole: a lens ray's first hit is not a pinhole projection (ptx_scene_set_lens(scene, 0, ...) first)");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "temporal rendering cannot start while a render runs on the scene");
  const ptx_temporal_camera cur = scene_temporal_camera(s);
  rc = check_temporal_camera(&cur, "current");
  if (rc) return rc;
  ptx_render_params p = *p_in;
  p.band_step = 0; /* whole image on this GPU */
  p.n_gpus = 0;
  p.flags = 0;
  HIP_TRY(hipSetDevice(s->device));
  RenderBusy busy(s);
  const double t0 = wall_ms();
  const size_t npix = (size_t)p.width * (size_t)p.height, n = npix * 3;
  /* a frame of another size starts without history; the handle's own history goes only once that frame stands */
  const bool have_hist = s->hist_valid && s->hist_w == p.width && s->hist_h == p.height;
  HIP_TRY(s->raw.ensure(n));
  HIP_TRY(s->sq.ensure(n));
  HIP_TRY(s->rgb.ensure(n));
  HIP_TRY(s->err.ensure(n));
  HIP_TRY(s->feat.ensure(npix * 8));
  HIP_TRY(s->temporal_raw.ensure(n));
  HIP_TRY(s->temporal_count.ensure(1));
  if (motion_out) HIP_TRY(s->temporal_motion.ensure(n));
  const int out = s->hist_valid ? 1 - s->hist_cur : s->hist_cur; /* (growing a buffer frees it: never the one that holds the history) */
  HIP_TRY(s->hist[out].ensure(npix * PTX_HISTORY_DOUBLES));
  if (dp) {
    HIP_TRY(s->den_raw.ensure(n));
    HIP_TRY(s->den_guide.ensure(npix * 8));
    HIP_TRY(s->den_cv[0].ensure(npix * 4));
    HIP_TRY(s->den_cv[1].ensure(npix * 4));
  }
  DrainOnExit drain;
  HIP_TRY(hipMemsetAsync(s->feat.p, 0, sizeof(double) * npix * 8, nullptr));
  rc = render_raw(s, &p, s->raw.p, nullptr, stats, nullptr, nullptr, nullptr, PassRange(pass_first, pass_count, true, s->sq.p));
  if (rc) return rc;
  rc = features_queue(s, &p, pass_first, pass_count, s->feat.p, nullptr);
  if (rc) return rc;
  const double* prev_hist = have_hist ? s->hist[s->hist_cur].p : nullptr;
  rc = temporal_queue(p.width, p.height, *tp, pass_count, pass_count, cur, prev_hist ? &s->hist_camera : nullptr, s->raw.p, s->sq.p, s->feat.p,
                      prev_hist, s->hist[out].p, s->temporal_raw.p, s->err.p, motion_out ? s->temporal_motion.p : nullptr, s->temporal_count.p, nullptr);
  if (rc) return rc;
  const double* filmed = s->temporal_raw.p;
  if (dp) {
    rc = denoise_queue(p.width, p.height, *dp, pass_count, nullptr, pass_count, s->temporal_raw.p, s->err.p, s->feat.p, s->den_guide.p,
                       s->den_cv[0].p, s->den_cv[1].p, s->den_raw.p, nullptr);
    if (rc) return rc;
    filmed = s->den_raw.p;
  }
  rc = film_resolve(p.width, p.height, pass_count, filmed, s->rgb.p, nullptr, PtBandMap{1, 1, 0}, 0, -1, s->film);
  if (rc) return rc;
  rc = framebuffer_to_host(s, s->rgb.p, rgb_out, n);
  if (!rc && err_out) rc = framebuffer_to_host(s, s->err.p, err_out, n);
  if (!rc && motion_out) rc = framebuffer_to_host(s, s->temporal_motion.p, motion_out, n);
  if (rc) return rc;
  unsigned long long took = 0;
  HIP_TRY(hipMemcpy(&took, s->temporal_count.p, sizeof took, hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(nullptr));
  drain.armed = false;
  /* the frame stands: the handle keeps its history and its camera */
  s->hist_cur = out;
  s->hist_valid = true;
  s->hist_w = p.width;
  s->hist_h = p.height;
  s->hist_camera = cur;
  if (history_pixels_out) *history_pixels_out = (int64_t)took;
  if (stats) {
    stats->samples = (int64_t)p.width * p.height * pass_count;
    stats->render_ms = wall_ms() - t0;
  }
  return 0;
}

namespace {
/* rays per batch of ptx_render_rays_device: PTX_RAYS_BATCH (a test hook: any batch size gives the same sums), else 16 M, and never
 * more than a path queue can number */
size_t rays_batch(const ptx_scene* s, int64_t n) {
  long long batch = 16ll << 20;
  if (const char* e = getenv("PTX_RAYS_BATCH")) batch = std::max(1ll, atoll(e));
  const size_t most = kPoolMaxEntries - shade_pool_slack(s) - 1;
  return std::min<size_t>(std::min<size_t>((size_t)batch, most), (size_t)n);
}

/* the caller's DEVICE arrays, checked on the device before anything else is queued (waits for st); the message names the lowest
 * refused ray and what is wrong with it (that one ray is read back) */
int check_rays_device(ptx_scene* s, int64_t n, const double* d_o, const double* d_d, const int32_t* d_off, hipStream_t st) {
  HIP_TRY(s->rays_lowest.ensure(1));
  HIP_TRY(hipMemsetAsync(s->rays_lowest.p, 0xff, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_rays_check, grid256(n), dim3(256), 0, st, (long long)n, d_o, d_d, d_off, s->rays_lowest.p);
  HIP_TRY(hipGetLastError());
  uint32_t lowest = 0xffffffffu;
  HIP_TRY(hipMemcpyAsync(&lowest, s->rays_lowest.p, sizeof lowest, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (lowest == 0xffffffffu) return 0;
  if ((int64_t)lowest >= n) return fail(PTX_ERR_HIP, "BUG: the ray check names ray %u of %lld", lowest, (long long)n);
  double o[3], d[3];
  int32_t off = 0;
  HIP_TRY(hipMemcpy(o, d_o + 3 * (size_t)lowest, sizeof o, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(d, d_d + 3 * (size_t)lowest, sizeof d, hipMemcpyDeviceToHost));
  if (d_off) HIP_TRY(hipMemcpy(&off, d_off + lowest, sizeof off, hipMemcpyDeviceToHost));
  const bool finite = std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]) && std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]);
  if (!finite) return fail(PTX_ERR_ARG, "ray %u has a component that is not finite (origin %g %g %g, direction %g %g %g)", lowest, o[0], o[1], o[2], d[0], d[1], d[2]);
  if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) return fail(PTX_ERR_ARG, "ray %u has the direction (0, 0, 0)", lowest);
  return fail(PTX_ERR_ARG, "ray %u has the sampler offset %d, outside [0, 2^31 - 2]", lowest, off);
}

/* what ptx_render_rays_device and ptx_render_rays check before a device is touched: the caller's arguments first (a host-only scene
 * gets the same PTX_ERR_ARG for them), then the scene's state */
int check_rays_args(const ptx_scene* s, const ptx_rays_params* rp, int64_t n, const void* origins, const void* directions, const void* sum) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (!rp) return fail(PTX_ERR_ARG, "NULL params");
  if (rp->max_bounces < 0 || rp->max_bounces > 126) return fail(PTX_ERR_ARG, "max_bounces must be in [0, 126] (got %d)", rp->max_bounces);
  if (rp->rays_per_bin < 1) return fail(PTX_ERR_ARG, "rays_per_bin must be >= 1 (got %d)", rp->rays_per_bin);
  if (rp->flags & ~PTX_RAYS_NORMALIZE) return fail(PTX_ERR_ARG, "unknown bits in flags (%d): only PTX_RAYS_NORMALIZE is defined", rp->flags);
  if (!origins || !directions || !sum) return fail(PTX_ERR_ARG, "NULL argument");
  if (n < 0 || n >= 0x7fffffffll) return fail(PTX_ERR_ARG, "bad ray count %lld: n must be in [0, 2^31 - 1)", (long long)n);
  if (n % rp->rays_per_bin != 0) return fail(PTX_ERR_ARG, "n = %lld is not a multiple of rays_per_bin = %d", (long long)n, rp->rays_per_bin);
  if (s->device < 0) return fail(PTX_ERR_STATE, "scene was created host-only (device -1): no CPU fallback exists");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "ptx_render_rays cannot start while a render runs on the scene (called from one of its callbacks?)");
  return 0;
}
}  // namespace

int32_t ptx_render_rays_device(ptx_scene* s, const ptx_rays_params* rp, int64_t n, const double* d_origins, const double* d_directions,
                               const int32_t* d_offsets, double* d_sum_inout, double* d_sq_inout, void* stream, ptx_stats* stats) {
  int rc = check_rays_args(s, rp, n, d_origins, d_directions, d_sum_inout);
  if (rc) return rc;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    fill_tree_stats(s, stats);
  }
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  const double t0 = wall_ms();
  hipStream_t st = (hipStream_t)stream;
  rc = check_rays_device(s, n, d_origins, d_directions, d_offsets, st);
  if (rc) return rc;
  RenderBusy busy(s);
  reschedule(s, 1);
  const size_t batch = rays_batch(s, n);
  Workspace w;
  rc = ensure_workspace(s, batch, rp->max_bounces, &w);
  if (rc) return rc;
  const bool count = rp->count_work != 0, normalize = (rp->flags & PTX_RAYS_NORMALIZE) != 0;
  const long long m = rp->rays_per_bin;
  if (count) HIP_TRY(hipMemsetAsync(s->counters.p, 0, sizeof(PtCounters), st));
  DrainOnExit drain; /* (an error half-way: nothing this call queued still reads the caller's arrays when it returns) */
  for (int64_t first = 0; first < n; first += (int64_t)batch) {
    const uint32_t nb = (uint32_t)std::min<int64_t>((int64_t)batch, n - first);
    HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * kCountsWords, st));
    /* a path that ends without a contribution leaves its entry as it is: zero (and max_bounces = 0 is zero for every ray) */
    HIP_TRY(hipMemsetAsync(w.contrib_all, 0, sizeof(double) * 4 * (size_t)nb, st));
    if (rp->max_bounces > 0) {
      PtQueue q0 = w.q[0];
      q0.count = w.counts;
      hipLaunchKernelGGL(normalize ? k_generate_rays<true> : k_generate_rays<false>, dim3((nb + 255u) / 256u), dim3(256), 0, st, s->dev, (long long)first, nb,
                         d_origins, d_directions, d_offsets, q0);
      run_bounces(s, st, w, (size_t)nb, rp->max_bounces, count, false, PrimaryLaunch());
    }
    const long long bins = (first + nb - 1) / m - first / m + 1;
    hipLaunchKernelGGL(d_sq_inout ? k_accum_rays<true> : k_accum_rays<false>, grid256(bins), dim3(256), 0, st, w.contrib, (long long)first,
                       (long long)nb, m, d_sum_inout, d_sq_inout);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  drain.armed = false;
  if (stats) {
    stats->samples = n;
    stats->render_ms = wall_ms() - t0;
    if (count) {
      rc = collect_counters(s, stats);
      if (rc) return rc;
    }
  }
  return 0;
}

int32_t ptx_render_rays(ptx_scene* s, const ptx_rays_params* rp, int64_t n, const double* origins, const double* directions, const int32_t* offsets,
                        double* sum_out, double* sq_out, ptx_stats* stats) {
  int rc = check_rays_args(s, rp, n, origins, directions, sum_out);
  if (rc) return rc;
  if (n == 0) return ptx_render_rays_device(s, rp, 0, origins, directions, offsets, sum_out, sq_out, nullptr, stats);
  HIP_TRY(hipSetDevice(s->device));
  const size_t n3 = (size_t)n * 3, bins3 = (size_t)(n / rp->rays_per_bin) * 3;
  DevBuf<double> d_o, d_d, d_sum, d_sq;
  DevBuf<int32_t> d_off;
  if ((rc = upload(d_o, origins, n3)) != 0 || (rc = upload(d_d, directions, n3)) != 0) return rc;
  if (offsets && (rc = upload(d_off, offsets, (size_t)n)) != 0) return rc;
  HIP_TRY(d_sum.ensure(bins3));
  HIP_TRY(hipMemset(d_sum.p, 0, sizeof(double) * bins3));
  if (sq_out) {
    HIP_TRY(d_sq.ensure(bins3));
    HIP_TRY(hipMemset(d_sq.p, 0, sizeof(double) * bins3));
  }
  rc = ptx_render_rays_device(s, rp, n, d_o.p, d_d.p, offsets ? d_off.p : nullptr, d_sum.p, sq_out ? d_sq.p : nullptr, nullptr, stats);
  if (rc) return rc;
  if ((rc = download(sum_out, d_sum, bins3)) != 0) return rc;
  return sq_out ? download(sq_out, d_sq, bins3) : 0;
}

int32_t ptx_kernel_table(char* names_out, int64_t capacity) {
  const std::vector<KernelEntry>& table = kernel_table();
  if (!names_out) return (int32_t)table.size();
  size_t need = 1;
  for (const KernelEntry& e : table) need += e.name.size() + 1;
  if (capacity < 0 || (size_t)capacity < need) return fail(PTX_ERR_ARG, "buffer too small: the %zu names take %zu bytes (capacity %lld)", table.size(), need, (long long)capacity);
  char* p = names_out;
  for (const KernelEntry& e : table) {
    std::memcpy(p, e.name.data(), e.name.size());
    p += e.name.size();
    *p++ = '\n';
  }
  *p = '\0';
  return (int32_t)table.size();
}

int32_t ptx_scene_launched_kernels(const ptx_scene* s, int32_t* indices_out, int32_t capacity) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (!indices_out) return fail(PTX_ERR_ARG, "NULL argument");
  const std::vector<KernelEntry>& table = kernel_table();
  std::vector<int32_t> found; /* (attr_done also holds what other launch functions prepared: only the table's kernels are reported) */
  for (size_t i = 0; i < table.size(); ++i)
    if (s->attr_done.count(table[i].kern)) found.push_back((int32_t)i);
  if (capacity < 0 || (size_t)capacity < found.size()) return fail(PTX_ERR_ARG, "buffer too small: %zu kernels were launched (capacity %d)", found.size(), capacity);
  std::copy(found.begin(), found.end(), indices_out);
  return (int32_t)found.size();
}

int32_t ptx_scene_clear_launched_kernels(ptx_scene* s) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (s->busy.load() != 0) return fail(PTX_ERR_STATE, "the launch record cannot be cleared while a render runs on the scene");
  s->attr_done.clear(); /* (a kernel's next launch prepares it again: the same limit, the same check) */
  return 0;
}

int32_t ptx_scene_tree(const ptx_scene* s, double* bbox_out, int32_t* info_out, int32_t node_capacity,
                       int32_t* prim_order_out, int32_t slot_capacity) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  const int n = (int)s->host->nodes.size();
  for (int i = 0; i < n && i < node_capacity; ++i) {
    const PtNode& nd = s->host->nodes[(size_t)i];
    if (bbox_out) {
      for (int k = 0; k < 3; ++k) {
        bbox_out[6 * i + k] = nd.mn[k];
        bbox_out[6 * i + 3 + k] = nd.mx[k];
      }
    }
    if (info_out) {
      const uint32_t axis = nd.b >> 30;
      const bool leaf = axis == PT_NODE_LEAF_AXIS;
      info_out[4 * i] = leaf ? 1 : 0;
      info_out[4 * i + 1] = leaf ? -1 : (int)axis;
      info_out[4 * i + 2] = (int32_t)nd.a;
      info_out[4 * i + 3] = (int32_t)(nd.b & 0x3fffffffu);
    }
  }
  if (prim_order_out)
    for (int i = 0; i < s->dev.n_slots && i < slot_capacity; ++i) prim_order_out[i] = s->host->slot_prim[(size_t)i];
  return n;
}

/* ---------------------------------------------------------------- progressive photon mapping */
int32_t ptx_ppm_render(ptx_scene* s, const ptx_ppm_params* p, const ptx_light* lights, int32_t n_lights, double* img_sum_out,
                       ptx_ppm_stats* stats, ptx_ppm_iteration_fn cb, void* user) {
  if (!s || !p || !lights || !img_sum_out) return fail(PTX_ERR_ARG, "NULL argument");
  /* (before any device is touched: a host-only scene gets this answer too) */
  if (s->projection != PTX_PROJECTION_PERSPECTIVE)
    return fail(PTX_ERR_STATE, "the photon mapper's eye pass looks through the scene's own pinhole: ptx_scene_set_camera_projection(scene, PTX_PROJECTION_PERSPECTIVE) first");
  if (s->pose_on) return fail(PTX_ERR_STATE, "the photon mapper's eye pass looks through the scene's own camera: switch the camera pose off with ptx_scene_set_camera_pose(scene, NULL, NULL, NULL) first");
  if (s->shutter_on) return fail(PTX_ERR_STATE, "the photon mapper's eye pass looks through the scene's own camera: switch the camera shutter off with ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first");
  if (s->device < 0) return fail(PTX_ERR_STATE, "scene was created host-only (device -1): no CPU fallback exists");
  if (p->width <= 0 || p->height <= 0 || p->iterations <= 0 || p->max_bounces <= 0 || p->max_bounces > 60 || p->photon_count <= 0 || n_lights <= 0)
    return fail(PTX_ERR_ARG, "bad photon-mapping parameters");
  if ((long long)p->iterations * ((long long)p->width * p->height > p->photon_count ? (long long)p->width * p->height : p->photon_count) >= 2147483647LL)
    return fail(PTX_ERR_ARG, "sampler offset does not fit 32 bits");
  if (s->host->nodes.empty()) return fail(PTX_ERR_STATE, "scene has no tree (Scene.bbox undefined)");
  if (s->lens_radius > 0.0) return fail(PTX_ERR_STATE, "the photon mapper's eye pass is a pinhole: switch the lens off with ptx_scene_set_lens(scene, 0, f) first");
  HIP_TRY(hipSetDevice(s->device));
  const double t_total0 = wall_ms();
  ptx_ppm_stats st;
  std::memset(&st, 0, sizeof st);
  const int W = p->width, H = p->height, mb = p->max_bounces;
  /* lights: Light.create_point / create_spot (:130-137), photons per light (:239-245) */
  std::vector<PtLightDev> hl((size_t)n_lights);
  std::vector<int> first((size_t)n_lights + 1, 0);
  double total_power = 0.0;
  std::vector<double> power((size_t)n_lights);
  for (int i = 0; i < n_lights; ++i) {
    const ptx_light& L = lights[i];
    if (L.kind != PTX_LIGHT_POINT && L.kind != PTX_LIGHT_SPOT) return fail(PTX_ERR_ARG, "light %d: unknown kind", i);
    /* the light table is checked here, on the host: none of these values may reach the photon split below or a kernel */
    if (!std::isfinite(L.power)) return fail(PTX_ERR_ARG, "light %d: power is not finite", i);
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(L.color[k]) || !std::isfinite(L.position[k])) return fail(PTX_ERR_ARG, "light %d: colour or position is not finite", i);
      if (!std::isfinite(L.power * L.color[k]) || L.power * L.color[k] < 0.0) return fail(PTX_ERR_ARG, "light %d: power x colour must be finite and >= 0", i);
    }
    if (L.kind == PTX_LIGHT_SPOT) {
      const double len2 = L.direction[0] * L.direction[0] + L.direction[1] * L.direction[1] + L.direction[2] * L.direction[2];
      if (!std::isfinite(len2) || !(len2 > 0.0)) return fail(PTX_ERR_ARG, "light %d: spot direction must be finite and of non-zero length", i);
    }
    PtLightDev& d = hl[(size_t)i];
    std::memset(&d, 0, sizeof d);
    d.kind = L.kind;
    for (int k = 0; k < 3; ++k) {
      d.pos[k] = L.position[k];
      d.color[k] = L.power * L.color[k]; /* Color.scale color power */
    }
    if (L.kind == PTX_LIGHT_SPOT) {
      const Quat q = pt_shader_rotation(v3_normalize(v3(L.direction[0], L.direction[1], L.direction[2])));
      d.rot[0] = q.r; d.rot[1] = q.v.x; d.rot[2] = q.v.y; d.rot[3] = q.v.z;
      const double angle = 0.5 * 45.0 * 3.14159265358979323846 / 180.0;
      d.disk_radius = std::atan(angle);
    }
    power[(size_t)i] = d.color[0] + d.color[1] + d.color[2]; /* Light.power */
    total_power = total_power + power[(size_t)i];
  }
  if (!std::isfinite(total_power) || !(total_power > 0.0)) return fail(PTX_ERR_ARG, "the lights' total power must be finite and positive");
  for (int i = 0; i < n_lights; ++i) {
    const double f = power[(size_t)i] / total_power;
    first[(size_t)i + 1] = first[(size_t)i] + (int)((double)p->photon_count * f); /* Int.of_float */
  }
  const int total = first[(size_t)n_lights];
  if (total <= 0) return fail(PTX_ERR_ARG, "BUG: no photons");
  /* samplers: p_sampler dimension 2 + 2 max_bounces, e_sampler 2 + max_bounces (:426-431) */
  const std::vector<double> p_alpha = lds_alpha(2 + 2 * mb), e_alpha = lds_alpha(2 + mb);
  /* init_radius2 (:292-297) from Scene.bbox = the tree's bbox */
  const PtNode& root = s->host->nodes[0];
  const double ext_x = root.mx[0] - root.mn[0], ext_y = root.mx[1] - root.mn[1], ext_z = root.mx[2] - root.mn[2];
  const double a = (ext_x + ext_y + ext_z) / 3.0;
  const double b = (double)(W + H) / (double)2;
  const double init_radius2 = (a / b) * (a / b);
  const double inv_photon_count = 1.0 / (double)p->photon_count;

  const size_t cap = (size_t)total * (size_t)mb;
  DevBuf<double> d_out, d_pm, d_palpha, d_ealpha, d_img;
  DevBuf<uint8_t> d_ndep;
  DevBuf<PtLightDev> d_lights;
  DevBuf<int> d_first;
  DevBuf<unsigned long long> d_cnt;
  DevBuf<PtNode> d_nodes;
  DevBuf<int> d_tile, d_src;
  const bool host_list = getenv("PTX_PPM_HOST_LIST") != nullptr && atoi(getenv("PTX_PPM_HOST_LIST")) != 0;
  auto release = [] {}; /* the buffers free themselves on every exit path */
#define PPM_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { release(); return fail(PTX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } } while (0)
  PPM_TRY(d_out.ensure(cap * 9));
  PPM_TRY(d_ndep.ensure((size_t)total));
  PPM_TRY(d_lights.ensure((size_t)n_lights));
  PPM_TRY(d_first.ensure((size_t)n_lights + 1));
  PPM_TRY(d_palpha.ensure(p_alpha.size()));
  PPM_TRY(d_ealpha.ensure(e_alpha.size()));
  PPM_TRY(d_img.ensure((size_t)W * H * 3));
  PPM_TRY(d_cnt.ensure(4));
  PPM_TRY(hipMemcpy(d_lights.p, hl.data(), sizeof(PtLightDev) * hl.size(), hipMemcpyHostToDevice));
  PPM_TRY(hipMemcpy(d_first.p, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice));
  PPM_TRY(hipMemcpy(d_palpha.p, p_alpha.data(), sizeof(double) * p_alpha.size(), hipMemcpyHostToDevice));
  PPM_TRY(hipMemcpy(d_ealpha.p, e_alpha.data(), sizeof(double) * e_alpha.size(), hipMemcpyHostToDevice));
  PPM_TRY(hipMemset(d_img.p, 0, sizeof(double) * (size_t)W * H * 3));
  PPM_TRY(hipMemset(d_cnt.p, 0, sizeof(unsigned long long) * 4));
  PtPhotonOut po;
  po.px = d_out.p; po.py = d_out.p + cap; po.pz = d_out.p + 2 * cap;
  po.nx = d_out.p + 3 * cap; po.ny = d_out.p + 4 * cap; po.nz = d_out.p + 5 * cap;
  po.fx = d_out.p + 6 * cap; po.fy = d_out.p + 7 * cap; po.fz = d_out.p + 8 * cap;
  po.n_deposits = d_ndep.p;
  std::vector<double> h_out; /* host copies: only for the host-side list / tree path */
  std::vector<uint8_t> h_ndep;
  std::vector<double> h_img;
  const bool array_mode = s->dev.mode == PT_MODE_ARRAY;

  for (int it = 0; it < p->iterations; ++it) {
    /* radius (i + 1), :381-392 */
    double product = 1.0;
    for (int k = 1; k <= it; ++k) {
      const double kf = (double)k;
      product = product * (kf + p->alpha) / kf;
    }
    const double radius = std::sqrt(product * init_radius2 / (double)(it + 1));
    st.last_radius = radius;
    /* ---- photon pass ---- */
    double t0 = wall_ms();
    {
      const int depth = std::max(1, s->tree_depth + 1);
      const size_t lds = (size_t)4 * depth * PT_WAVE * sizeof(uint32_t);
      const dim3 gd(grid256(total)), bd(256);
      /* (a scene with an image texture: the IMG instantiations, as in a render) */
      const auto kern = s->dev.n_images != 0 ? (array_mode ? k_ppm_photons<PT_MODE_ARRAY, true> : k_ppm_photons<PT_MODE_SIMD, true>)
                                             : (array_mode ? k_ppm_photons<PT_MODE_ARRAY> : k_ppm_photons<PT_MODE_SIMD>);
      hipLaunchKernelGGL(kern, gd, bd, lds, nullptr, s->dev, depth, d_lights.p, n_lights, d_first.p, it * p->photon_count, d_palpha.p, mb, po, d_cnt.p);
      PPM_TRY(hipGetLastError());
    }
    PPM_TRY(hipDeviceSynchronize());
    st.photon_ms += wall_ms() - t0;
    t0 = wall_ms();
    /* ---- photon list + Photon_map.Tree.create ~num_bins:8 (Array_leaf cutoff 8) ---- */
    size_t n_ph = 0, n_slots = 0;
    int tree_depth = 0, tree_nodes = 0;
    const PtNode* tree_nodes_dev = nullptr;
    bool on_device = false;
    if (!host_list) {
      /* everything stays on the device: scan of the deposit counts -> list + boxes -> GPU build -> slot order */
      const int n_tiles = (total + PPM_SCAN_TILE - 1) / PPM_SCAN_TILE;
      PPM_TRY(d_tile.ensure((size_t)n_tiles + 1));
      PPM_TRY(d_src.ensure(cap));
      BvhGpuWorkspace& bws = bvh_gpu_workspace();
      PPM_TRY(bws.d_box.ensure(cap * 6));
      hipLaunchKernelGGL(k_ppm_list_count, dim3((unsigned)n_tiles), dim3(256), 0, nullptr, d_ndep.p, total, d_tile.p);
      hipLaunchKernelGGL(k_ppm_list_offsets, dim3(1), dim3(1), 0, nullptr, d_tile.p, n_tiles, d_tile.p + n_tiles);
      hipLaunchKernelGGL(k_ppm_list_emit, dim3((unsigned)n_tiles), dim3(256), 0, nullptr, d_ndep.p, total, mb, d_tile.p, po.px, po.py, po.pz, radius, d_src.p, bws.d_box.p);
      PPM_TRY(hipGetLastError());
      int n_list = 0;
      PPM_TRY(hipMemcpy(&n_list, d_tile.p + n_tiles, sizeof(int), hipMemcpyDeviceToHost));
      if (n_list <= 0) { release(); return fail(PTX_ERR_STATE, "BUG: no photons"); }
      n_ph = (size_t)n_list;
      if (n_list >= 4096) {
        BvhDeviceTree dt;
        if (bvh_build_device(bws.d_box.p, n_list, nullptr, 8, 8, false, &dt)) {
          n_slots = (size_t)dt.n_slots;
          PPM_TRY(d_pm.ensure(n_slots * 9));
          hipLaunchKernelGGL(k_ppm_slots, grid256(n_slots), dim3(256), 0, nullptr, dt.slot_prim, d_src.p, (int)n_slots, d_out.p, cap, d_pm.p);
          PPM_TRY(hipGetLastError());
          tree_depth = dt.depth;
          tree_nodes = dt.n_nodes;
          tree_nodes_dev = dt.nodes;
          on_device = true;
          ++st.device_trees;
          ++st.gpu_built_trees;
        }
      }
    }
    if (!on_device) {
      /* small maps (and PTX_PPM_HOST_LIST=1): the list and the tree are made on the host */
      h_out.resize(cap * 9);
      h_ndep.resize((size_t)total);
      PPM_TRY(hipMemcpy(h_ndep.data(), d_ndep.p, h_ndep.size(), hipMemcpyDeviceToHost));
      PPM_TRY(hipMemcpy(h_out.data(), d_out.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost));
      std::vector<size_t> src;
      for (int i = total - 1; i >= 0; --i)
        for (int k = (int)h_ndep[(size_t)i] - 1; k >= 0; --k) src.push_back((size_t)i * (size_t)mb + (size_t)k);
      n_ph = src.size();
      if (n_ph == 0) { release(); return fail(PTX_ERR_STATE, "BUG: no photons"); }
      std::vector<Box> boxes(n_ph);
      for (size_t j = 0; j < n_ph; ++j) { /* Photon bbox: center - radius, center + radius (:150-156) */
        const size_t a0 = src[j];
        const V3 c = v3(h_out[a0], h_out[cap + a0], h_out[2 * cap + a0]);
        boxes[j].mn = v3(c.x - radius, c.y - radius, c.z - radius);
        boxes[j].mx = v3(c.x + radius, c.y + radius, c.z + radius);
      }
      BvhResult tree;
      bool built = false;
      if (n_ph >= 4096) built = bvh_build_gpu(boxes, 8, 8, false, &tree);
      if (built) ++st.gpu_built_trees;
      else tree = bvh_build(boxes, 8, 8, false);
      n_slots = tree.slot_prim.size();
      std::vector<double> pm_host(n_slots * 9);
      for (size_t sl = 0; sl < n_slots; ++sl) {
        const size_t a0 = src[(size_t)tree.slot_prim[sl]];
        for (int c = 0; c < 9; ++c) pm_host[(size_t)c * n_slots + sl] = h_out[(size_t)c * cap + a0];
      }
      PPM_TRY(d_pm.ensure(pm_host.size()));
      PPM_TRY(d_nodes.ensure(tree.nodes.size()));
      PPM_TRY(hipMemcpy(d_pm.p, pm_host.data(), sizeof(double) * pm_host.size(), hipMemcpyHostToDevice));
      PPM_TRY(hipMemcpy(d_nodes.p, tree.nodes.data(), sizeof(PtNode) * tree.nodes.size(), hipMemcpyHostToDevice));
      tree_depth = tree.depth;
      tree_nodes = (int)tree.nodes.size();
      tree_nodes_dev = d_nodes.p;
    }
    PPM_TRY(hipDeviceSynchronize());
    st.build_ms += wall_ms() - t0;
    st.photons_stored += (int64_t)n_ph;
    /* ---- eye pass ---- */
    t0 = wall_ms();
    {
      PtPhotonMapDev pm;
      pm.nodes = tree_nodes_dev; pm.n_nodes = tree_nodes; pm.pad = 0;
      pm.px = d_pm.p; pm.py = d_pm.p + n_slots; pm.pz = d_pm.p + 2 * n_slots;
      pm.nx = d_pm.p + 3 * n_slots; pm.ny = d_pm.p + 4 * n_slots; pm.nz = d_pm.p + 5 * n_slots;
      pm.fx = d_pm.p + 6 * n_slots; pm.fy = d_pm.p + 7 * n_slots; pm.fz = d_pm.p + 8 * n_slots;
      const int depth = std::max(std::max(1, s->tree_depth + 1), tree_depth + 1);
      const size_t lds = (size_t)4 * depth * PT_WAVE * sizeof(uint32_t);
      if (lds > 160 * 1024) { release(); return fail(PTX_ERR_STATE, "photon tree too deep for the LDS stack"); }
      const dim3 gd(grid256((int64_t)W * H)), bd(256);
      const auto kern = s->dev.n_images != 0 ? (array_mode ? k_ppm_gather<PT_MODE_ARRAY, true> : k_ppm_gather<PT_MODE_SIMD, true>)
                                             : (array_mode ? k_ppm_gather<PT_MODE_ARRAY> : k_ppm_gather<PT_MODE_SIMD>);
      if (lds > 64 * 1024) raise_dynamic_lds_limit((const void*)kern, (int)(160 * 1024 - 1024)); /* the kernels also hold static words (chunk counters, the floor triangles) */
      hipLaunchKernelGGL(kern, gd, bd, lds, nullptr, s->dev, depth, pm, radius, d_ealpha.p, it * W * H, W, H, mb, inv_photon_count, d_img.p, d_cnt.p + 1);
      PPM_TRY(hipGetLastError());
      PPM_TRY(hipDeviceSynchronize());
    }
    st.gather_ms += wall_ms() - t0;
    if (cb) {
      h_img.resize((size_t)W * H * 3);
      PPM_TRY(hipMemcpy(h_img.data(), d_img.p, sizeof(double) * h_img.size(), hipMemcpyDeviceToHost));
      cb(user, it, radius, (int64_t)n_ph, h_img.data());
    }
  }
  PPM_TRY(hipMemcpy(img_sum_out, d_img.p, sizeof(double) * (size_t)W * H * 3, hipMemcpyDeviceToHost));
  unsigned long long cnt[4];
  PPM_TRY(hipMemcpy(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost));
  st.photon_rays = (int64_t)cnt[0];
  st.eye_rays = (int64_t)cnt[1];
  st.neighbors = (int64_t)cnt[2];
  st.total_ms = wall_ms() - t_total0;
  if (stats) *stats = st;
  release();
#undef PPM_TRY
  return 0;
}

} /* extern "C" */
