/* probes.inc -- the point-probe entry points of include/ptx.h: n host-side items in, one kernel over them, n results back.
 * Diagnostics, not the rendering path -- but the GPU tests stand on them.  Included from kernels.hip directly after ptx_api.inc
 * (the same translation unit: fail, HIP_TRY, DevBuf, upload / download / grid256, the schedule and the workspace are that file's). */
#include <optional>

namespace {
/* the refusal every probe of a scene starts with */
int device_scene_ready(const ptx_scene* s) {
  if (!s) return fail(PTX_ERR_ARG, "NULL scene");
  if (s->device < 0) return fail(PTX_ERR_STATE, "scene was created host-only (device -1): no CPU fallback exists");
  return 0;
}

int light_half_ready(const ptx_scene* s) {
  if (const int rc = device_scene_ready(s)) return rc;
  if (s->dev.lighting != PTX_LIGHTING_SAMPLED || s->dev.n_lights + s->dev.n_sphere_lights < 1)
    return fail(PTX_ERR_STATE, "the light half needs PTX_LIGHTING_SAMPLED and a light triangle or a sphere light to sample");
  return 0;
}

int env_sampling_ready(const ptx_scene* s) {
  if (const int rc = device_scene_ready(s)) return rc;
  if (!s->env_sampling || !s->dev.env_sample) return fail(PTX_ERR_STATE, "environment sampling is off (ptx_scene_set_environment_sampling)");
  return 0;
}

/* ---- (x, y, pass) lists: ptx_trace_samples, ptx_camera_rays, ptx_debug_first_scatter.
 * The camera rays of explicit (x, y, pass) triples appended to q0 on the null stream, by the generator of this camera kind
 * (launch_generate_tiles and launch_generate_pixels are its siblings).  A C name: this function and the two walk selectors below stood
 * inside ptx_api.inc's extern "C" block, which put their names into the library's dynamic symbol table; the table stays as it was. */
extern "C" void launch_generate_list(ptx_scene* s, const ptx_render_params* p, PtCameraKind kind, int64_t n, const int32_t* dx, const int32_t* dy,
                          const int32_t* dp, const PtQueue& q0) {
  const PtCameraArg cam = scene_camera(s, p->max_bounces);
  with_camera_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(k_generate_list<decltype(k)::value>, grid256(n), dim3(256), 0, nullptr, s->dev, p->width, p->height,
                       p->samples_per_pixel, (long long)n, dx, dy, dp, cam, (const double*)s->alpha.p, q0);
  });
}

int check_sample_list(const ptx_render_params* p, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes) {
  for (int64_t i = 0; i < n; ++i)
    if (xs[i] < 0 || xs[i] >= p->width || ys[i] < 0 || ys[i] >= p->height || passes[i] < 0 || passes[i] >= p->samples_per_pixel)
      return fail(PTX_ERR_ARG, "sample %lld out of range", (long long)i);
  return 0;
}

/* what a staged list leaves its caller: the scene held busy, the workspace, the triples on the device and the queue of their rays */
struct SampleList {
  std::optional<RenderBusy> busy;
  Workspace w;
  DevBuf<int32_t> dx, dy, dp;
  PtQueue q0;
};
/* The front half the three share: the scene held busy and scheduled for one batch, a workspace for n paths, the triples uploaded, the
 * control words cleared, and -- unless `generate` is off: a depth-0 ptx_trace_samples traces nothing -- the camera rays of the scene's
 * own kind (camera_kind of the schedule just made) appended to q0 = the workspace's first queue, counted in counts[0]. */
int stage_sample_list(ptx_scene* s, const ptx_render_params* p, bool generate, int64_t n, const int32_t* xs, const int32_t* ys,
                      const int32_t* passes, SampleList* l) {
  HIP_TRY(hipSetDevice(s->device));
  l->busy.emplace(s);
  reschedule(s, 1);
  if (const int rc = ensure_workspace(s, (size_t)n, p->max_bounces, &l->w)) return rc;
  if (const int rc = upload(l->dx, xs, (size_t)n)) return rc;
  if (const int rc = upload(l->dy, ys, (size_t)n)) return rc;
  if (const int rc = upload(l->dp, passes, (size_t)n)) return rc;
  HIP_TRY(hipMemset(l->w.counts, 0, sizeof(uint32_t) * kCountsWords));
  l->q0 = l->w.q[0];
  l->q0.count = l->w.counts;
  if (generate) launch_generate_list(s, p, camera_kind(s->sched), n, l->dx.p, l->dy.p, l->dp.p, l->q0);
  return 0;
}

/* ---- the hit read-back of ptx_intersect_rays and ptx_walk_rays: hit slots -> primitive indices; a miss (slot < 0) reads t = 0, prim = -1 */
void slots_to_prims(const ptx_scene* s, int64_t n, const int32_t* slot, double* t_out, int32_t* prim_out) {
  for (int64_t i = 0; i < n; ++i) {
    prim_out[i] = slot[i] < 0 ? -1 : s->host->slot_prim[(size_t)slot[i]];
    if (slot[i] < 0) t_out[i] = 0.0;
  }
}

/* ---- the LDS walks: ptx_walk_rays, ptx_walk_next_leaf.
 * What each PTX_WALK_* is, stated once: the row is what the two kernel selectors instantiate from and what the gate refuses by.
 * `mode` is the leaf kind the walk is written for, or kSceneLeaf: the walk takes the scene's.  `node_loop`: the walk has a node loop
 * of its own, so k_next_leaf_eval can run it (the packet walks in lockstep; a tail walk differs only below the leaves' parents). */
constexpr int kSceneLeaf = -1;
struct WalkTraits {
  int walk, mode;
  bool packet, oct, zero, tail, node_loop;
};
constexpr WalkTraits kWalks[] = {
    /*                            mode           packet oct    zero   tail   node_loop */
    {PTX_WALK_SHARED_ASM,      PT_MODE_SIMD,  false, false, false, false, true},
    {PTX_WALK_OCT_ASM,         PT_MODE_SIMD,  false, true,  false, false, true},
    {PTX_WALK_SHARED_DIV,      PT_MODE_ARRAY, false, false, false, false, true},
    {PTX_WALK_PACKET,          kSceneLeaf,    true,  false, true,  false, false},
    {PTX_WALK_SHARED_ASM_ZERO, PT_MODE_SIMD,  false, false, true,  false, true},
    {PTX_WALK_OCT_ASM_ZERO,    PT_MODE_SIMD,  false, true,  true,  false, true},
    {PTX_WALK_SHARED_DIV_ZERO, PT_MODE_ARRAY, false, false, true,  false, true},
    {PTX_WALK_SHARED_ASM_TAIL, PT_MODE_SIMD,  false, false, false, true,  false},
    {PTX_WALK_OCT_ASM_TAIL,    PT_MODE_SIMD,  false, true,  false, true,  false},
    {PTX_WALK_SHARED_DIV_TAIL, PT_MODE_ARRAY, false, false, false, true,  false},
};
constexpr int kNumWalks = (int)(sizeof kWalks / sizeof kWalks[0]);
constexpr bool walk_rows_in_place(int i = 0) { return i == kNumWalks || (kWalks[i].walk == i && walk_rows_in_place(i + 1)); }
static_assert(kNumWalks == 10 && walk_rows_in_place(), "kWalks is indexed by PTX_WALK_*: row i describes walk i (include/ptx.h: dense, 0 to 9)");

/* of(std::integral_constant<int, walk>) with the run-time walk made a compile-time row number; nullptr for a walk the table lacks */
template <class Kernel, class Of, int... W>
Kernel kernel_of_walk(int walk, Of of, std::integer_sequence<int, W...>) {
  Kernel kern = nullptr;
  ((walk == W ? (void)(kern = of(std::integral_constant<int, W>())) : (void)0), ...);
  return kern;
}
/* The two selectors, each the row's instantiation (C names, like launch_generate_list: see there).
 * k_walk_eval: 11 = on the shared image {assembly loop, divergent loop} x {plain, origin zero, tail cut}, on the per-octant image the
 * assembly loop x the same three, and the packet walk per leaf kind.  Template arguments: <MODE, PACKET, LOCT, ZERO, TAIL>. */
using WalkKernel = decltype(&k_walk_eval<PT_MODE_SIMD, false, false, false, false>);
extern "C" WalkKernel walk_kernel(int walk, int scene_mode) {
  return kernel_of_walk<WalkKernel>(walk, [&](auto w) -> WalkKernel {
    constexpr WalkTraits r = kWalks[decltype(w)::value];
    if constexpr (r.mode != kSceneLeaf) return k_walk_eval<r.mode, r.packet, r.oct, r.zero, r.tail>;
    else return scene_mode == PT_MODE_SIMD ? k_walk_eval<PT_MODE_SIMD, r.packet, r.oct, r.zero, r.tail> : k_walk_eval<PT_MODE_ARRAY, r.packet, r.oct, r.zero, r.tail>;
  }, std::make_integer_sequence<int, kNumWalks>());
}
/* k_next_leaf_eval: 6 = the walks with a node loop of their own x {plain, origin zero}.  Template arguments: <MODE, LOCT, ZERO>. */
using NextLeafKernel = decltype(&k_next_leaf_eval<PT_MODE_SIMD, false, false>);
extern "C" NextLeafKernel next_leaf_kernel(int walk) {
  return kernel_of_walk<NextLeafKernel>(walk, [](auto w) -> NextLeafKernel {
    constexpr WalkTraits r = kWalks[decltype(w)::value];
    if constexpr (r.node_loop) return k_next_leaf_eval<r.mode, r.oct, r.zero>;
    else return nullptr;
  }, std::make_integer_sequence<int, kNumWalks>());
}

/* what the scene can take: the bounce kernels' own conditions (make_schedule), less the knobs that choose between possible walks.
 * After reschedule(s, 1). */
int check_walk_scene(const ptx_scene* s, int walk, const WalkTraits& row) {
  const Schedule& sc = s->sched;
  const bool simd = s->dev.mode == PT_MODE_SIMD;
  if (!sc.in_lds() || sc.from_hbm) return fail(PTX_ERR_STATE, "walk %d: the scene is walked from HBM / L2, these walks run on LDS-resident scenes", walk);
  if (row.mode == PT_MODE_SIMD && !simd) return fail(PTX_ERR_STATE, "walk %d is a Simd_leaf walk and the scene is Array_leaf", walk);
  if (row.mode == PT_MODE_ARRAY && simd) return fail(PTX_ERR_STATE, "walk %d is the Array_leaf walk and the scene is Simd_leaf", walk);
  if (row.oct && (s->dev.lds_oct == nullptr || !sc.carry_oct.fits)) return fail(PTX_ERR_STATE, "walk %d: the scene has no per-octant LDS image, or a launch does not fit with it", walk);
  if (!row.oct && !sc.carry.fits) return fail(PTX_ERR_STATE, "walk %d: a launch of the bounce kernel does not fit LDS with the scene's image", walk);
  if (sc.bounce_threads > PT_BOUNCE_THREADS) return fail(PTX_ERR_STATE, "walk %d: workgroups of %d threads", walk, sc.bounce_threads);
  return 0;
}

/* a _ZERO walk (and the packet) takes the origin as given: every component the bits of +0.0 */
int check_zero_origins(int walk, int64_t n, const double* origins) {
  if (!kWalks[walk].zero) return 0;
  const double pz = 0.0;
  for (int64_t k = 0; k < 3 * n; ++k)
    if (std::memcmp(&origins[k], &pz, sizeof pz) != 0)
      return fail(PTX_ERR_ARG, "walk %d takes the origin as (+0, +0, +0): component %lld of the origins is %a", walk, (long long)k, origins[k]);
  return 0;
}

/* k_bounce_carry's launch for n items: its workgroup, its dynamic LDS for the image the walk reads, one workgroup (one scene image)
 * per CU.  Prepares the kernel (its first launch on the scene raises the limit and checks the static LDS). */
struct WalkLaunch {
  dim3 grid, block;
  size_t lds;
  int stack_depth;
};
WalkLaunch prepare_walk_launch(ptx_scene* s, const void* kern, const char* name, const WalkTraits& row, int64_t n) {
  const Schedule& sc = s->sched;
  prepare_kernel(s, kern, name, !row.oct /* (record numbers, not 16-bit addresses) */, 160 * 1024 - 256, PT_LDS_CU_BYTES - PT_LDS_BOUNCE_LIMIT);
  const int threads = sc.bounce_threads;
  return WalkLaunch{dim3(strided_grid(s, (size_t)n, threads, 1)), dim3(threads), (size_t)(row.oct ? sc.carry_oct.total : sc.carry.total),
                    std::max(1, s->tree_depth + 1)};
}

}  // namespace

extern "C" {

int32_t ptx_light_sample(ptx_scene* s, int64_t n, const double* points, const double* uv, double* dir_out, int32_t* index_out) {
  if (const int rc = light_half_ready(s)) return rc;
  if (n < 0 || !points || !uv || !dir_out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_p, d_uv, d_out;
  DevBuf<int32_t> d_index;
  if (const int rc = upload(d_p, points, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_uv, uv, (size_t)n * 2)) return rc;
  HIP_TRY(d_out.ensure((size_t)n * 3));
  if (index_out) HIP_TRY(d_index.ensure((size_t)n));
  hipLaunchKernelGGL(k_light_sample, grid256(n), dim3(256), 0, nullptr, s->dev, (long long)n, d_p.p, d_uv.p, d_out.p, index_out ? d_index.p : nullptr);
  HIP_TRY(hipGetLastError());
  if (const int rc = download(dir_out, d_out, (size_t)n * 3)) return rc;
  return index_out ? download(index_out, d_index, (size_t)n) : 0;
}
int32_t ptx_light_pdf(ptx_scene* s, int64_t n, const double* points, const double* dirs, double* pd_out) {
  if (const int rc = light_half_ready(s)) return rc;
  if (n < 0 || !points || !dirs || !pd_out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_p, d_dirs, d_out;
  if (const int rc = upload(d_p, points, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_dirs, dirs, (size_t)n * 3)) return rc;
  HIP_TRY(d_out.ensure((size_t)n));
  hipLaunchKernelGGL(k_light_pdf, grid256(n), dim3(256), 0, nullptr, s->dev, (long long)n, d_p.p, d_dirs.p, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(pd_out, d_out, (size_t)n);
}

int32_t ptx_texture_eval(ptx_scene* s, int32_t index, int64_t n, const double* uv, double* rgb_out) {
  if (const int rc = device_scene_ready(s)) return rc;
  if (const int rc = check_texture_index(s, index)) return rc;
  if (n < 0 || !uv || !rgb_out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  /* the record a slot whose material points at this entry holds: the descriptor's texture, or the image in its place */
  PtShadeRec rec{};
  const PtTexture& t = s->host->texs[(size_t)index];
  rec.kind = PTX_MAT_LAMBERTIAN;
  rec.tex_kind = t.kind; rec.tex_w = t.width; rec.tex_h = t.height;
  std::memcpy(rec.even, t.even, sizeof rec.even);
  std::memcpy(rec.odd, t.odd, sizeof rec.odd);
  if (!s->images.empty() && s->images[(size_t)index]->host) {
    const ptx_scene::ImageSlot& e = *s->images[(size_t)index];
    const uint64_t texels = (uint64_t)(uintptr_t)e.dev.p, flags = (uint64_t)(uint32_t)e.host->flags;
    rec.tex_kind = PT_TEX_IMAGE; rec.tex_w = e.host->width; rec.tex_h = e.host->height;
    std::memset(rec.even, 0, sizeof rec.even);
    std::memcpy(&rec.even[0], &texels, sizeof texels);
    std::memcpy(&rec.even[1], &flags, sizeof flags);
  }
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_uv, d_out;
  if (const int rc = upload(d_uv, uv, (size_t)n * 2)) return rc;
  HIP_TRY(d_out.ensure((size_t)n * 3));
  hipLaunchKernelGGL(k_texture_eval, grid256(n), dim3(256), 0, nullptr, rec, (long long)n, d_uv.p, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(rgb_out, d_out, (size_t)n * 3);
}

int32_t ptx_environment_eval(ptx_scene* s, int64_t n, const double* dirs, double* rgb_out) {
  if (const int rc = device_scene_ready(s)) return rc;
  if (n < 0 || !dirs || !rgb_out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_dirs, d_out;
  if (const int rc = upload(d_dirs, dirs, (size_t)n * 3)) return rc;
  HIP_TRY(d_out.ensure((size_t)n * 3));
  hipLaunchKernelGGL(k_environment_eval, grid256(n), dim3(256), 0, nullptr, s->dev, (long long)n, d_dirs.p, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(rgb_out, d_out, (size_t)n * 3);
}
int32_t ptx_environment_sample(ptx_scene* s, int64_t n, const double* ab, double* dirs_out, int32_t* texel_out) {
  if (const int rc = env_sampling_ready(s)) return rc;
  if (n < 0 || !ab || !dirs_out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_ab, d_out;
  DevBuf<int32_t> d_texel;
  if (const int rc = upload(d_ab, ab, (size_t)n * 2)) return rc;
  HIP_TRY(d_out.ensure((size_t)n * 3));
  if (texel_out) HIP_TRY(d_texel.ensure((size_t)n * 2));
  hipLaunchKernelGGL(k_environment_sample, grid256(n), dim3(256), 0, nullptr, s->dev, (long long)n, d_ab.p, d_out.p, texel_out ? d_texel.p : nullptr);
  HIP_TRY(hipGetLastError());
  if (const int rc = download(dirs_out, d_out, (size_t)n * 3)) return rc;
  return texel_out ? download(texel_out, d_texel, (size_t)n * 2) : 0;
}
int32_t ptx_environment_pdf(ptx_scene* s, int64_t n, const double* dirs, double* pd_out) {
  if (const int rc = env_sampling_ready(s)) return rc;
  if (n < 0 || !dirs || !pd_out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_dirs, d_out;
  if (const int rc = upload(d_dirs, dirs, (size_t)n * 3)) return rc;
  HIP_TRY(d_out.ensure((size_t)n));
  hipLaunchKernelGGL(k_environment_pdf, grid256(n), dim3(256), 0, nullptr, s->dev, (long long)n, d_dirs.p, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(pd_out, d_out, (size_t)n);
}

int32_t ptx_trace_samples(ptx_scene* s, const ptx_render_params* p, int64_t n, const int32_t* xs, const int32_t* ys,
                          const int32_t* passes, double* rgb_out, ptx_stats* stats) {
  if (!s || !xs || !ys || !passes || !rgb_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (const int rc = check_render_args(s, p, nullptr)) return rc;
  if (n < 0 || n >= 0x7fffffffll) return fail(PTX_ERR_ARG, "bad sample count");
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    fill_tree_stats(s, stats);
  }
  if (n == 0) return 0;
  if (const int rc = check_sample_list(p, n, xs, ys, passes)) return rc;
  SampleList l;
  if (const int rc = stage_sample_list(s, p, p->max_bounces > 0, n, xs, ys, passes, &l)) return rc;
  Workspace& w = l.w;
  const bool count = p->count_work != 0;
  HIP_TRY(hipMemset(w.contrib_all, 0, sizeof(double) * w.contrib_n));
  if (count) HIP_TRY(hipMemset(s->counters.p, 0, sizeof(PtCounters)));
  if (p->max_bounces > 0) run_bounces(s, nullptr, w, (size_t)n, p->max_bounces, count, false, PrimaryLaunch());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<double> rgbx((size_t)n * 4);
  HIP_TRY(hipMemcpy(rgbx.data(), w.contrib.rgbx, sizeof(double) * rgbx.size(), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) rgb_out[3 * i + k] = rgbx[(size_t)i * 4 + k];
  if (stats) stats->samples = n;
  return stats && count ? collect_counters(s, stats) : 0;
}

int32_t ptx_camera_rays(ptx_scene* s, const ptx_render_params* p, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes,
                        double* origins_out, double* directions_out) {
  if (!s || !xs || !ys || !passes || !origins_out || !directions_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (const int rc = check_render_args(s, p, nullptr)) return rc;
  if (n < 0 || n >= 0x7fffffffll) return fail(PTX_ERR_ARG, "bad sample count");
  if (n == 0) return 0;
  if (const int rc = check_sample_list(p, n, xs, ys, passes)) return rc;
  SampleList l;
  if (const int rc = stage_sample_list(s, p, true, n, xs, ys, passes, &l)) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  /* the generator appends wave by wave: entry e is the ray of sample path[e].id */
  const size_t path_stride = s->dev.has_emit ? 2 : 1;
  std::vector<PtRayRec> rays((size_t)n);
  std::vector<PtPathRec> path((size_t)n * path_stride);
  HIP_TRY(hipMemcpy(rays.data(), l.q0.ray, sizeof(PtRayRec) * rays.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(path.data(), l.q0.path, sizeof(PtPathRec) * path.size(), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < (size_t)n; ++e) {
    const size_t i = path[e * path_stride].id;
    if (i >= (size_t)n) return fail(PTX_ERR_HIP, "BUG: camera ray %zu carries sample id %zu of %lld", e, i, (long long)n);
    const PtRayRec& r = rays[e];
    origins_out[3 * i] = r.ox; origins_out[3 * i + 1] = r.oy; origins_out[3 * i + 2] = r.oz;
    directions_out[3 * i] = r.dx; directions_out[3 * i + 1] = r.dy; directions_out[3 * i + 2] = r.dz;
  }
  return 0;
}

int32_t ptx_intersect_rays(ptx_scene* s, int64_t n, const double* origins, const double* directions, double* t_out,
                           int32_t* prim_out, ptx_stats* stats) {
  if (!s || !origins || !directions || !t_out || !prim_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (const int rc = device_scene_ready(s)) return rc;
  if (n < 0 || n >= 0x7fffffffll) return fail(PTX_ERR_ARG, "bad ray count");
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    fill_tree_stats(s, stats);
  }
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  Workspace w;
  reschedule(s, 1);
  /* this entry point hands the hit distances back: keep the records */
  if (const int rc = ensure_workspace(s, (size_t)n, 1, &w, 0, true)) return rc;
  DevBuf<double> d_o, d_d;
  if (const int rc = upload(d_o, origins, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_d, directions, (size_t)n * 3)) return rc;
  const uint32_t cnt = (uint32_t)n;
  HIP_TRY(hipMemset(w.counts, 0, sizeof(uint32_t) * kCountsWords));
  HIP_TRY(hipMemcpy(w.counts, &cnt, sizeof cnt, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(s->counters.p, 0, sizeof(PtCounters)));
  PtQueue q0 = w.q[0];
  q0.count = w.counts;
  hipLaunchKernelGGL(k_load_rays, grid256(n), dim3(256), 0, nullptr, (long long)n, d_o.p, d_d.p, q0);
  launch_trace(s, nullptr, q0, w.hits, (size_t)n, true, w.counts + kWorkBase, w.susp, kNoBounce);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int32_t> slot((size_t)n);
  if (w.hits.tuv) { /* scenes with triangles keep {t, u, v, -} records (PtHits) */
    std::vector<double> tuv((size_t)n * 4);
    HIP_TRY(hipMemcpy(tuv.data(), w.hits.tuv, sizeof(double) * tuv.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) t_out[i] = tuv[(size_t)i * 4];
  } else {
    HIP_TRY(hipMemcpy(t_out, w.hits.t, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipMemcpy(slot.data(), w.hits.slot, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  slots_to_prims(s, n, slot.data(), t_out, prim_out);
  return stats ? collect_counters(s, stats) : 0;
}

int32_t ptx_walk_rays(ptx_scene* s, int32_t walk, int64_t n, const double* origins, const double* directions, double* t_out,
                      int32_t* prim_out) {
  if (!s || !origins || !directions || !t_out || !prim_out) return fail(PTX_ERR_ARG, "NULL argument");
  if (walk < 0 || walk >= kNumWalks) return fail(PTX_ERR_ARG, "unknown walk %d", walk);
  if (const int rc = device_scene_ready(s)) return rc;
  if (n < 0 || n >= 0x7fffffffll) return fail(PTX_ERR_ARG, "bad ray count");
  HIP_TRY(hipSetDevice(s->device));
  reschedule(s, 1);
  const WalkTraits& row = kWalks[walk];
  if (const int rc = check_walk_scene(s, walk, row)) return rc;
  if (const int rc = check_zero_origins(walk, n, origins)) return rc;
  if (n == 0) return 0;
  DevBuf<double> d_o, d_d, d_t;
  DevBuf<int32_t> d_s;
  if (const int rc = upload(d_o, origins, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_d, directions, (size_t)n * 3)) return rc;
  HIP_TRY(d_t.ensure((size_t)n)); HIP_TRY(d_s.ensure((size_t)n));
  const WalkKernel kern = walk_kernel(walk, s->dev.mode);
  const WalkLaunch wl = prepare_walk_launch(s, (const void*)kern, "k_walk_eval", row, n);
  hipLaunchKernelGGL(kern, wl.grid, wl.block, wl.lds, nullptr, s->dev, (long long)n, d_o.p, d_d.p, d_t.p, d_s.p, wl.stack_depth);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int32_t> slot((size_t)n);
  if (const int rc = download(t_out, d_t, (size_t)n)) return rc;
  if (const int rc = download(slot.data(), d_s, (size_t)n)) return rc;
  slots_to_prims(s, n, slot.data(), t_out, prim_out);
  return 0;
}

int32_t ptx_walk_next_leaf(ptx_scene* s, int32_t walk, int64_t n, const double* origins, const double* directions, const int32_t* nodes,
                           const double* t_max, int32_t* leaf_out) {
  if (!s || !origins || !directions || !nodes || !t_max || !leaf_out) return fail(PTX_ERR_ARG, "NULL argument");
  const NextLeafKernel kern = next_leaf_kernel(walk);
  if (!kern) return fail(PTX_ERR_ARG, "unknown walk %d (the walks with a node loop of their own: no PACKET, no _TAIL)", walk);
  if (const int rc = device_scene_ready(s)) return rc;
  if (n < 0 || n >= 0x7fffffffll) return fail(PTX_ERR_ARG, "bad triple count");
  HIP_TRY(hipSetDevice(s->device));
  reschedule(s, 1);
  const WalkTraits& row = kWalks[walk];
  if (const int rc = check_walk_scene(s, walk, row)) return rc;
  if (const int rc = check_zero_origins(walk, n, origins)) return rc;
  const int64_t n_nodes = (int64_t)s->host->nodes.size();
  for (int64_t k = 0; k < n; ++k) {
    if (nodes[k] < 0 || (int64_t)nodes[k] >= n_nodes) return fail(PTX_ERR_ARG, "triple %lld: node %d is not one of the tree's %lld", (long long)k, nodes[k], (long long)n_nodes);
    if (!(t_max[k] >= 0.0)) return fail(PTX_ERR_ARG, "triple %lld: t_max %a is NaN or negative", (long long)k, t_max[k]);
  }
  if (n == 0) return 0;
  DevBuf<double> d_o, d_d, d_t;
  DevBuf<int32_t> d_k, d_l;
  if (const int rc = upload(d_o, origins, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_d, directions, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_t, t_max, (size_t)n)) return rc;
  if (const int rc = upload(d_k, nodes, (size_t)n)) return rc;
  HIP_TRY(d_l.ensure((size_t)n));
  const WalkLaunch wl = prepare_walk_launch(s, (const void*)kern, "k_next_leaf_eval", row, n);
  hipLaunchKernelGGL(kern, wl.grid, wl.block, wl.lds, nullptr, s->dev, (long long)n, d_o.p, d_d.p, d_k.p, d_t.p, d_l.p, wl.stack_depth);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return download(leaf_out, d_l, (size_t)n);
}

/* Debug / parity aid: the state of every path after ONE segment (generate + trace + shade of bounce 0):
 * alive_out[i] = 1 and ray_out[6i..] = (origin, direction), attn_out[3i..] when sample i scattered,
 * alive_out[i] = 0 when it terminated.  Not part of the rendering path. */
int32_t ptx_debug_first_scatter(ptx_scene* s, const ptx_render_params* p, int64_t n, const int32_t* xs, const int32_t* ys,
                                const int32_t* passes, double* ray_out, double* attn_out, int32_t* alive_out) {
  if (!s || !xs || !ys || !passes || !ray_out || !attn_out || !alive_out) return fail(PTX_ERR_ARG, "NULL argument");
  /* (before any device is touched: a host-only scene gets this answer too) */
  if (s->projection != PTX_PROJECTION_PERSPECTIVE)
    return fail(PTX_ERR_STATE, "ptx_debug_first_scatter traces the rays of the scene's own pinhole: ptx_scene_set_camera_projection(scene, PTX_PROJECTION_PERSPECTIVE) first");
  if (s->pose_on) return fail(PTX_ERR_STATE, "ptx_debug_first_scatter traces the rays of the scene's own camera: switch the camera pose off with ptx_scene_set_camera_pose(scene, NULL, NULL, NULL) first");
  if (s->shutter_on) return fail(PTX_ERR_STATE, "ptx_debug_first_scatter traces the rays of the scene's own camera: switch the camera shutter off with ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first");
  if (const int rc = check_render_args(s, p, nullptr)) return rc;
  if (n <= 0 || p->max_bounces < 2) return fail(PTX_ERR_ARG, "need n > 0 and max_bounces >= 2");
  if (s->lens_radius > 0.0) return fail(PTX_ERR_STATE, "ptx_debug_first_scatter traces the pinhole's rays: switch the lens off with ptx_scene_set_lens(scene, 0, f) first");
  /* no check_sample_list here, unlike the two callers above: this entry point has always taken its triples unchecked */
  SampleList l; /* (every camera kind but the pinhole was refused above) */
  if (const int rc = stage_sample_list(s, p, true, n, xs, ys, passes, &l)) return rc;
  Workspace& w = l.w;
  run_bounces(s, nullptr, w, (size_t)n, p->max_bounces, false, false, PrimaryLaunch(), 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  uint32_t cnt = 0;
  HIP_TRY(hipMemcpy(&cnt, w.counts + 1, sizeof cnt, hipMemcpyDeviceToHost));
  std::vector<PtRayRec> rays((size_t)cnt);
  const size_t pstride = s->dev.has_emit ? 2 : 1; /* emissive scenes: {path, emission} pairs (PtQueue) */
  std::vector<PtPathRec> paths((size_t)cnt * pstride);
  HIP_TRY(hipMemcpy(rays.data(), w.q[1].ray, sizeof(PtRayRec) * cnt, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(paths.data(), w.q[1].path, sizeof(PtPathRec) * cnt * pstride, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) alive_out[i] = 0;
  for (uint32_t j = 0; j < cnt; ++j) {
    const PtRayRec& r = rays[j];
    uint64_t dx_bits;
    memcpy(&dx_bits, &r.dx, sizeof dx_bits);
    if ((uint32_t)(dx_bits >> 32) == (uint32_t)PT_HOLE_HI) continue; /* an unused entry of a part-filled block (k_shade_pool) */
    const PtPathRec& pr = paths[(size_t)j * pstride];
    const uint32_t i = pr.id;
    alive_out[i] = 1;
    const double ray6[6] = {r.ox, r.oy, r.oz, r.dx, r.dy, r.dz};
    for (int k = 0; k < 6; ++k) ray_out[6 * (size_t)i + k] = ray6[k];
    attn_out[3 * (size_t)i] = pr.ar;
    attn_out[3 * (size_t)i + 1] = pr.ag;
    attn_out[3 * (size_t)i + 2] = pr.ab;
  }
  return 0;
}

int32_t ptx_lds_sample(int32_t device, int32_t dimension, int64_t n, const int32_t* offsets, const int32_t* dims, double* out) {
  if (dimension < 1 || n < 0 || !offsets || !dims || !out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  for (int64_t i = 0; i < n; ++i)
    if (dims[i] < 0 || dims[i] >= dimension) return fail(PTX_ERR_ARG, "dimension index out of range");
  HIP_TRY(hipSetDevice(device));
  const std::vector<double> alpha = lds_alpha(dimension);
  DevBuf<double> d_alpha, d_out;
  DevBuf<int32_t> d_off, d_dim;
  if (const int rc = upload(d_alpha, alpha.data(), (size_t)dimension)) return rc;
  if (const int rc = upload(d_off, offsets, (size_t)n)) return rc;
  if (const int rc = upload(d_dim, dims, (size_t)n)) return rc;
  HIP_TRY(d_out.ensure((size_t)n));
  hipLaunchKernelGGL(k_lds_sample, grid256(n), dim3(256), 0, nullptr, d_alpha.p, (long long)n, d_off.p, d_dim.p, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(out, d_out, (size_t)n);
}

#if PT_FILTER_DEBUG
/* diagnostic builds only (kernels.hip, k_filter_error; tools/filter_error_study.py) -- not declared in include/ptx.h, not in the product */
int32_t ptx_debug_filter_error(ptx_scene* s, int64_t n, const double* o3, const double* d3, const int32_t* nodes, const double* tmax, double* out6) {
  if (!s || n < 0 || !o3 || !d3 || !nodes || !tmax || !out6) return fail(PTX_ERR_ARG, "bad argument");
  if (s->device < 0 || !s->dev.nodes32o) return fail(PTX_ERR_ARG, "needs a scene on a device with the per-octant node image");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<double> d_o, d_d, d_t, d_out;
  DevBuf<int32_t> d_n;
  if (const int rc = upload(d_o, o3, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_d, d3, (size_t)n * 3)) return rc;
  if (const int rc = upload(d_t, tmax, (size_t)n)) return rc;
  if (const int rc = upload(d_n, nodes, (size_t)n)) return rc;
  HIP_TRY(d_out.ensure((size_t)n * 6));
  hipLaunchKernelGGL(k_filter_error, grid256(n), dim3(256), 0, nullptr, s->dev, (long long)n, d_o.p, d_d.p, d_n.p, d_t.p, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(out6, d_out, (size_t)n * 6);
}
#endif
int32_t ptx_math_eval(int32_t device, int32_t fn, int64_t n, const double* a, const double* b, double* out) {
  if (fn < 0 || fn > 14 || n < 0 || !a || !out) return fail(PTX_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> d_a, d_b, d_out;
  if (const int rc = upload(d_a, a, (size_t)n)) return rc;
  if (b)
    if (const int rc = upload(d_b, b, (size_t)n)) return rc;
  HIP_TRY(d_out.ensure((size_t)n));
  hipLaunchKernelGGL(k_math_eval, grid256(n), dim3(256), 0, nullptr, fn, (long long)n, d_a.p, b ? d_b.p : nullptr, d_out.p);
  HIP_TRY(hipGetLastError());
  return download(out, d_out, (size_t)n);
}

} /* extern "C" */
