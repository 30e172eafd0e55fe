/* denoise.inc -- first-hit feature sums and the variance-guided a-trous filter (included from kernels.hip).
 * Image-space kernels beside the integrator: nothing here is called by a render of the k_bounce / k_trace / k_shade_pool paths.
 * The filter's rule is stated operation for operation in include/ptx.h (ptx_denoise_device); tests/denoise_reference.py restates it
 * in numpy and the GPU tests compare bit for bit, so every expression below keeps the header's grouping (the build has
 * -ffp-contract=off). */

/* ------------------------------------------------------------------ first-hit features */
/* The feature record of entry i of a k_trace launch whose ray was (o, d): the hit is the one the walk stored, and the surface comes
 * from the functions of the render's shade step (pt_shade_entry): the same operands through the same code, the same bits.  depth is t
 * along the ray. */
struct PtFeature {
  V3 albedo, normal;
  double depth, hit;
};
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
  if (sc.has_triangles) { /* (t, u, v) again from the ray and the primitive the walk settled on, as the shade step does */
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

/* ... of primary sample i of a PRIMARY launch (the virtual queue of pt_primary_decode): the pinhole's ray is computed again from the
 * sample's index by the launch's own functions */
template <bool IMG>
__device__ __forceinline__ PtFeature pt_feature_sample(const PtSceneDev& sc, const PtGenParams& g, const PtPrimarySample& ps,
                                                       const PtHits& hits, const double* __restrict__ alpha, uint32_t i) {
  const V3 o = v3(0.0, 0.0, 0.0), d = pt_primary_dir(sc, g, ps, alpha);
  return pt_feature_ray<IMG>(sc, o, d, hits, i);
}

/* a pixel's 64-byte record of sums, in and out as four 16-byte accesses */
struct PtFeatureSums {
  double2 r0, r1, r2, r3;
};
__device__ __forceinline__ PtFeatureSums pt_feature_sums_load(const double2* rec) { return PtFeatureSums{rec[0], rec[1], rec[2], rec[3]}; }
__device__ __forceinline__ void pt_feature_sums_add(PtFeatureSums& s, const PtFeature& f) {
  s.r0.x = s.r0.x + f.albedo.x;
  s.r0.y = s.r0.y + f.albedo.y;
  s.r1.x = s.r1.x + f.albedo.z;
  s.r1.y = s.r1.y + f.normal.x;
  s.r2.x = s.r2.x + f.normal.y;
  s.r2.y = s.r2.y + f.normal.z;
  s.r3.x = s.r3.x + f.depth;
  s.r3.y = s.r3.y + f.hit;
}
__device__ __forceinline__ void pt_feature_sums_store(double2* rec, const PtFeatureSums& s) {
  rec[0] = s.r0;
  rec[1] = s.r1;
  rec[2] = s.r2;
  rec[3] = s.r3;
}

/* feat[pixel] += the records of the batch's n_pass passes, in pass order.  One thread per entry j of ONE pass of the virtual primary
 * queue (8x8 tiles, ragged edges padded: neighbouring lanes read neighbouring hit records); it owns its pixel, so the sums need no
 * atomics and a pixel's additions run in pass order. */
template <bool IMG = false> /* IMG: scenes with an image texture or an environment (pt_shade_entry) */
__global__ __launch_bounds__(256) void k_features(PtSceneDev sc, PtGenParams g, PtHits hits, const double* __restrict__ alpha,
                                                  double* __restrict__ feat) {
  const uint32_t per_pass = (uint32_t)(g.tiles_x * g.tiles_y) * 64u;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= per_pass) return;
  const PtPrimarySample p0 = pt_primary_decode(g, j);
  if (!p0.valid) return; /* (n_pass >= 1: pass 0 of the batch decides for every pass) */
  double2* rec = (double2*)(feat + ((long long)p0.gy * g.width + p0.x) * 8);
  PtFeatureSums sums = pt_feature_sums_load(rec);
  for (int k = 0; k < g.n_pass; ++k) {
    const uint32_t i = (uint32_t)k * per_pass + j;
    const PtPrimarySample ps = pt_primary_decode(g, i);
    pt_feature_sums_add(sums, pt_feature_sample<IMG>(sc, g, ps, hits, alpha, i));
  }
  pt_feature_sums_store(rec, sums);
}

/* k_features for the cameras whose rays are generated (k_generate_tiles<CAM, false>): the same thread-per-pixel sums in pass order over
 * the queue the generator wrote and k_trace walked; the ray of an entry is read back from that queue */
template <bool IMG>
__global__ __launch_bounds__(256) void k_features_queue(PtSceneDev sc, PtGenParams g, PtQueue q, PtHits hits, double* __restrict__ feat) {
  const uint32_t per_pass = (uint32_t)(g.tiles_x * g.tiles_y) * 64u;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= per_pass) return;
  const PtPrimarySample p0 = pt_primary_decode(g, j);
  if (!p0.valid) return;
  double2* rec = (double2*)(feat + ((long long)p0.gy * g.width + p0.x) * 8);
  PtFeatureSums sums = pt_feature_sums_load(rec);
  for (int k = 0; k < g.n_pass; ++k) {
    const uint32_t i = (uint32_t)k * per_pass + j;
    V3 o, d;
    pt_q_load_ray(q, i, o, d);
    pt_feature_sums_add(sums, pt_feature_ray<IMG>(sc, o, d, hits, i));
  }
  pt_feature_sums_store(rec, sums);
}

/* the feature means of ptx_render_denoised's feat_out: sums / kf, the hits included */
__global__ __launch_bounds__(256) void k_feature_means(const double* __restrict__ feat, long long n, double kf, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = feat[i] / kf;
}

/* ------------------------------------------------------------------ a-trous filter */
struct PtDenoise {
  int32_t width, height;
  int32_t m;          /* normal_power_log2 */
  int32_t demodulate;
  double sl2, sz, sa2; /* sigma_l * sigma_l, sigma_z, sigma_a * sigma_a */
};
/* per pixel, so that no tap divides: the 64-byte guide {n.x, n.y, n.z, z, a.r, a.g, a.b, h} and the 32-byte {c.r, c.g, c.b, V} */
struct __attribute__((aligned(16))) PtGuide { double nx, ny, nz, z, ar, ag, ab, h; };

__device__ __forceinline__ double pt_demod(const PtDenoise& dn, double a) { return (dn.demodulate && a > 0x1p-7) ? a : 1.0; }

__global__ __launch_bounds__(256) void k_denoise_prepare(PtDenoise dn, int k, const int32_t* __restrict__ passes, double kf,
                                                         const double* __restrict__ raw, const double* __restrict__ err,
                                                         const double* __restrict__ feat, PtGuide* __restrict__ guide,
                                                         double4* __restrict__ cv) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long long)dn.width * dn.height) return;
  const double kd = (double)(passes ? passes[p] : k);
  const double2* f = (const double2*)(feat + p * 8);
  const double2 f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
  PtGuide gd;
  gd.ar = f0.x / kf;
  gd.ag = f0.y / kf;
  gd.ab = f1.x / kf;
  gd.nx = f1.y / kf;
  gd.ny = f2.x / kf;
  gd.nz = f2.y / kf;
  gd.z = f3.x / kf;
  gd.h = f3.y;
  const double dr = pt_demod(dn, gd.ar), dg = pt_demod(dn, gd.ag), db = pt_demod(dn, gd.ab);
  const double mr = raw[3 * p] / kd, mg = raw[3 * p + 1] / kd, mb = raw[3 * p + 2] / kd;
  const double er = err[3 * p], eg = err[3 * p + 1], eb = err[3 * p + 2];
  const double vr = er * er, vg = eg * eg, vb = eb * eb;
  const double V = (vr / (dr * dr) + vg / (dg * dg)) + vb / (db * db);
  guide[p] = gd;
  cv[p] = make_double4(mr / dr, mg / dg, mb / db, V);
}

constexpr int PT_ATROUS_TX = 32, PT_ATROUS_TY = 8; /* a workgroup's pixels: 32 x 8 (rows of 32 x 32 B = 1 KB of {c, V} per tap row) */
constexpr int PT_ATROUS_LDS_STEP = 2;              /* the LDS variant holds the tile and its halo of 2 * step pixels: steps 1 and 2 */
constexpr int PT_ATROUS_LDS_PIXELS = (PT_ATROUS_TX + 4 * PT_ATROUS_LDS_STEP) * (PT_ATROUS_TY + 4 * PT_ATROUS_LDS_STEP); /* 40 x 16 */

/* One level: step s, {c, V} from cv_in to cv_out (different buffers: launches on one stream order the levels).  One thread per
 * pixel.  LDS = false: every tap is a gather of the tap's 64-byte guide and 32-byte {c, V} through L1 / L2 (16-byte loads).
 * LDS = true (step <= PT_ATROUS_LDS_STEP; by default step 1 only, see denoise_queue): the workgroup first copies its tile and
 * the halo of 2 * step pixels into LDS (96 bytes per pixel, 60 KB at step 2) and the taps read that copy.  Both read the same
 * values in the same order: the same bits.  At step 4 the tile with its halo is 48 x 24 pixels (108 KB); from step 16 on the halo
 * is larger than any tile. */
template <bool LDS>
__global__ __launch_bounds__(PT_ATROUS_TX * PT_ATROUS_TY) void k_atrous(PtDenoise dn, int step, const PtGuide* __restrict__ guide,
                                                                        const double4* __restrict__ cv_in, double4* __restrict__ cv_out) {
  constexpr int NL = LDS ? PT_ATROUS_LDS_PIXELS : 1;
  __shared__ double4 l_cv[NL];
  __shared__ PtGuide l_g[NL];
  const int x = (int)blockIdx.x * PT_ATROUS_TX + (int)(threadIdx.x % PT_ATROUS_TX);
  const int y = (int)blockIdx.y * PT_ATROUS_TY + (int)(threadIdx.x / PT_ATROUS_TX);
  const long long W = dn.width;
  const int halo = 2 * step, rw = PT_ATROUS_TX + 2 * halo, rh = PT_ATROUS_TY + 2 * halo; /* the region in LDS */
  const int rx0 = (int)blockIdx.x * PT_ATROUS_TX - halo, ry0 = (int)blockIdx.y * PT_ATROUS_TY - halo;
  if (LDS) {
    for (int k = (int)threadIdx.x; k < rw * rh; k += PT_ATROUS_TX * PT_ATROUS_TY) {
      const int gx = rx0 + k % rw, gy = ry0 + k / rw;
      if (gx < 0 || gx >= dn.width || gy < 0 || gy >= dn.height) continue; /* never read: every tap is tested against the image */
      l_cv[k] = cv_in[(long long)gy * W + gx];
      l_g[k] = guide[(long long)gy * W + gx];
    }
    __syncthreads();
  }
  if (x >= dn.width || y >= dn.height) return;
  const long long p = (long long)y * W + x;
  auto load_cv = [&](int qx, int qy) -> double4 { return LDS ? l_cv[(qy - ry0) * rw + (qx - rx0)] : cv_in[(long long)qy * W + qx]; };
  auto load_g = [&](int qx, int qy) -> PtGuide { return LDS ? l_g[(qy - ry0) * rw + (qx - rx0)] : guide[(long long)qy * W + qx]; };
  const PtGuide gp = load_g(x, y);
  const double4 cp = load_cv(x, y);
  const double lp = (cp.x + cp.y) + cp.z;
  double vbar = 0.0;
  for (int j = -1; j <= 1; ++j) {
    const int qy = y + j;
    if (qy < 0 || qy >= dn.height) continue;
    const double bj = j == 0 ? 0.5 : 0.25;
    for (int i = -1; i <= 1; ++i) {
      const int qx = x + i;
      if (qx < 0 || qx >= dn.width) continue;
      const double bi = i == 0 ? 0.5 : 0.25;
      vbar = vbar + (bj * bi) * load_cv(qx, qy).w;
    }
  }
  const double den = dn.sl2 * vbar + 1e-12;
  double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0;
  for (int j = -2; j <= 2; ++j) {
    const int qy = y + step * j;
    if (qy < 0 || qy >= dn.height) continue;
    const double hj = j == 0 ? 0.375 : ((j == 1 || j == -1) ? 0.25 : 0.0625);
    for (int i = -2; i <= 2; ++i) {
      const int qx = x + step * i;
      if (qx < 0 || qx >= dn.width) continue;
      const double hi = i == 0 ? 0.375 : ((i == 1 || i == -1) ? 0.25 : 0.0625);
      const PtGuide gq = load_g(qx, qy);
      const double4 cq = load_cv(qx, qy);
      double wn = 1.0;
      if (!(gp.h == 0.0 && gq.h == 0.0)) {
        const double d = (gp.nx * gq.nx + gp.ny * gq.ny) + gp.nz * gq.nz;
        wn = d > 0.0 ? d : 0.0;
        for (int t = 0; t < dn.m; ++t) wn = wn * wn;
      }
      const double r = (gp.z - gq.z) / (dn.sz * (pt_fabs(gp.z) + pt_fabs(gq.z)) + 1e-300);
      const double wz = 1.0 / (1.0 + r * r);
      const double er = gp.ar - gq.ar, eg = gp.ag - gq.ag, eb = gp.ab - gq.ab;
      const double wa = 1.0 / (1.0 + ((er * er + eg * eg) + eb * eb) / dn.sa2);
      const double t = lp - ((cq.x + cq.y) + cq.z);
      const double wl = 1.0 / (1.0 + (t * t) / den);
      const double w = (hj * hi) * (((wn * wz) * wa) * wl);
      sw = sw + w;
      sr = sr + w * cq.x;
      sg = sg + w * cq.y;
      sb = sb + w * cq.z;
      sv = sv + (w * w) * cq.w;
    }
  }
  cv_out[p] = make_double4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

__global__ __launch_bounds__(256) void k_denoise_finish(PtDenoise dn, int k, const int32_t* __restrict__ passes,
                                                        const PtGuide* __restrict__ guide, const double4* __restrict__ cv,
                                                        double* __restrict__ out) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long long)dn.width * dn.height) return;
  const double kd = (double)(passes ? passes[p] : k);
  const PtGuide gd = guide[p];
  const double4 c = cv[p];
  out[3 * p] = (c.x * pt_demod(dn, gd.ar)) * kd;
  out[3 * p + 1] = (c.y * pt_demod(dn, gd.ag)) * kd;
  out[3 * p + 2] = (c.z * pt_demod(dn, gd.ab)) * kd;
}
