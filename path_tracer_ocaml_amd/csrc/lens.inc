/* lens.inc -- the thin-lens camera's kernels (included from kernels.hip; the rule: include/ptx.h and pt_lens.h).
 * A lens ray does not start at the origin, which the fused camera launches take for granted, so a lens render WRITES its camera rays
 * into a path queue and bounces them from there like any queued rays: everything here only makes rays (and, for the feature
 * buffers, reads the hits of rays it made).  No kernel of the pinhole path is touched. */
#include "pt_lens.h"

/* The camera ray of sample (x, gy) with sampler offset `offset`: render_tile's film coordinates (integrator.ml:98-105) exactly as
 * pt_primary_dir and k_generate_list compute them, the lens pair from the sampler's last two dimensions at the same offset */
__device__ __forceinline__ void pt_lens_sample_ray(const PtSceneDev& sc, const PtLens& ln, const double* __restrict__ alpha, int x, int gy,
                                                   int width, int height, int offset, V3* o, V3* d) {
  const double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  const double dxs = pt_lds_get(alpha, offset, 0), dys = pt_lds_get(alpha, offset, 1);
  const double cx = ((double)x + dxs) * widthf;
  const double cy = 1.0 - (((double)gy + dys) * heightf);
  const double u = pt_lds_get(alpha, offset, ln.dim - 2), v = pt_lds_get(alpha, offset, ln.dim - 1);
  pt_lens_ray(sc.cam_llx, sc.cam_lly, sc.cam_vx, sc.cam_vy, cx, cy, ln.radius, ln.focus, u, v, o, d);
}
/* a fresh path: attenuation 1, no emission carried */
__device__ __forceinline__ void pt_lens_store(const PtSceneDev& sc, const PtQueue& q, uint32_t dst, V3 o, V3 d, uint32_t id, int offset) {
  if (sc.has_emit) pt_q_store<true>(q, dst, o, d, v3(1.0, 1.0, 1.0), v3(0.0, 0.0, 0.0), id, offset);
  else pt_q_store<false>(q, dst, o, d, v3(1.0, 1.0, 1.0), v3(0.0, 0.0, 0.0), id, offset);
}

/* The camera rays of a whole batch (g.n_pass passes of this rank's rows) in the order the fused camera launch enumerates its virtual
 * queue (pt_primary_decode): entry i = (pass_in_batch, 8x8 tile, lane), so 64 consecutive entries are one tile of one pass and a wave
 * of the bounce launch that follows walks a coherent bundle.  Every entry owns its slot (no append); the lanes of a ragged tile that
 * fall off the image are HOLES (PT_HOLE_HI, as k_shade_pool marks the unused entries of its blocks: every reader of a queue skips
 * them), so *q.count = n_pass * tiles * 64 entries, which is what the workspace of a full-frame batch is sized for.  The contribution
 * id is pt_primary_decode's: pass_in_batch * W * local_rows + y * W + x, what k_accum / k_accum_sq sum by.
 * PATH = false writes the rays alone (q.path is not touched): the feature buffers trace them and keep no path state. */
template <bool PATH>
__global__ __launch_bounds__(256) void k_generate_lens(PtSceneDev sc, PtGenParams g, PtLens ln, const double* __restrict__ alpha, PtQueue q) {
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
  pt_lens_sample_ray(sc, ln, alpha, ps.x, ps.gy, g.width, g.height, ps.offset, &o, &d);
  if (PATH) pt_lens_store(sc, q, i, o, d, ps.id, ps.offset);
  else pt_q_store_ray(q, i, o, d);
}

/* k_generate_pixels through the lens: the same entries, ids and count (list mode: adaptive rounds, ptx_render_pixels_device) */
__global__ __launch_bounds__(256) void k_generate_pixels_lens(PtSceneDev sc, int width, int height, int spp, int first_pass, int n_pass,
                                                              const int32_t* __restrict__ pix, long long n_list, PtLens ln,
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
  pt_lens_sample_ray(sc, ln, alpha, x, gy, width, height, offset, &o, &d);
  pt_lens_store(sc, q, (uint32_t)i, o, d, (uint32_t)i, offset);
}

/* k_generate_list through the lens: explicit (x, y, pass) triples (ptx_trace_samples) */
__global__ __launch_bounds__(256) void k_generate_list_lens(PtSceneDev sc, int width, int height, int spp, long long n,
                                                            const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                            const int32_t* __restrict__ passes, PtLens ln,
                                                            const double* __restrict__ alpha, PtQueue q) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  const uint32_t dst = pt_wave_append(q.count, valid);
  if (!valid) return;
  const int x = xs[i], gy = ys[i], pass = passes[i];
  const int offset = (gy * width) + x + (pass * spp);
  V3 o, d;
  pt_lens_sample_ray(sc, ln, alpha, x, gy, width, height, offset, &o, &d);
  pt_lens_store(sc, q, dst, o, d, (uint32_t)i, offset);
}

/* ------------------------------------------------------------------ first-hit features of the lens rays */
/* pt_feature_sample (denoise.inc) for a ray that has an origin: the same functions of the render's shade step on the hit the walk
 * of k_generate_lens<false>'s queue stored at entry i; depth is t along the lens ray */
template <bool IMG>
__device__ __forceinline__ PtFeature pt_feature_ray(const PtSceneDev& sc, V3 o, V3 d, const PtHits& hits, uint32_t i) {
  PtFeature f;
  const int slot = hits.slot[i];
  if (slot < 0) {
    f.albedo = pt_background<IMG>(sc, d);
    f.normal = v3(0.0, 0.0, 0.0);
    f.depth = 0.0;
    f.hit = 0.0;
    return f;
  }
  double t_hit = 0.0, bu = 0.0, bv = 0.0;
  PtSlotGeom geom;
  geom.cx = geom.cy = geom.cz = 0.0;
  geom.kind = PT_SLOT_SPHERE;
  if (sc.has_triangles) {
    geom.kind = (int)sc.slot_kind[slot];
    if (geom.kind == PT_SLOT_SPHERE) {
      const double* sp = sc.sph + (size_t)slot * 4;
      (void)pt_sphere_intersect_scalar(v3(sp[0], sp[1], sp[2]), sp[3], o, d, 0.0, PT_MAX_FINITE, &t_hit);
    } else {
      const double* tvx = sc.tri + (size_t)slot * 10;
      (void)pt_triangle_intersect(pt_load_v3(tvx), pt_load_v3(tvx + 3), pt_load_v3(tvx + 6), o, d, 0.0, PT_MAX_FINITE, &t_hit, &bu, &bv);
    }
  } else {
    t_hit = hits.t[i];
    const double2* sp = (const double2*)(sc.sph + (size_t)slot * 4);
    const double2 s0 = sp[0], s1 = sp[1];
    geom.cx = s0.x;
    geom.cy = s0.y;
    geom.cz = s1.x;
  }
  const PtMatRegs m = pt_mat_load<PT_CAT_NONE, false>(sc.slot_shade + slot);
  const bool is_tri = geom.kind != PT_SLOT_SPHERE;
  const PtSurface sf = pt_surface_hit<PT_CAT_NONE>(sc, o, d, slot, t_hit, is_tri ? bu : 0.0, is_tri ? bv : 0.0, m, geom);
  f.albedo = m.kind == 2 ? v3(1.0, 1.0, 1.0) : pt_texture_eval<IMG>(m, sf.tu, sf.tv);
  f.normal = sf.normal;
  f.depth = t_hit;
  f.hit = 1.0;
  return f;
}

/* k_features (denoise.inc) for a lens: the same thread-per-pixel sums in pass order over the queue k_generate_lens<false> wrote and
 * k_trace walked; the ray of an entry is read back from that queue (the pinhole's kernel computes it again: it has no queue) */
template <bool IMG>
__global__ __launch_bounds__(256) void k_features_lens(PtSceneDev sc, PtGenParams g, PtQueue q, PtHits hits, double* __restrict__ feat) {
  const uint32_t per_pass = (uint32_t)(g.tiles_x * g.tiles_y) * 64u;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= per_pass) return;
  const PtPrimarySample p0 = pt_primary_decode(g, j);
  if (!p0.valid) return;
  double2* rec = (double2*)(feat + ((long long)p0.gy * g.width + p0.x) * 8);
  double2 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
  for (int k = 0; k < g.n_pass; ++k) {
    const uint32_t i = (uint32_t)k * per_pass + j;
    V3 o, d;
    pt_q_load_ray(q, i, o, d);
    const PtFeature f = pt_feature_ray<IMG>(sc, o, d, hits, i);
    r0.x = r0.x + f.albedo.x;
    r0.y = r0.y + f.albedo.y;
    r1.x = r1.x + f.albedo.z;
    r1.y = r1.y + f.normal.x;
    r2.x = r2.x + f.normal.y;
    r2.y = r2.y + f.normal.z;
    r3.x = r3.x + f.depth;
    r3.y = r3.y + f.hit;
  }
  rec[0] = r0;
  rec[1] = r1;
  rec[2] = r2;
  rec[3] = r3;
}
