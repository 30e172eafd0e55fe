/* ppm.inc -- progressive photon mapping on the same traverse / intersect / scatter code (SURVEY.md section 8 F4).
 * Mirrors progressive-photon-map/src/progressive_photon_map.ml; included by kernels.hip.
 *
 *   k_ppm_photons : Photon_map.trace_photon (:196-233) -- one lane per photon path from the lights
 *   (host)        : the reference's photon list order, Photon_map.Tree.create ~num_bins:8 (cutoff 8)
 *   k_ppm_gather  : render_image / estimate_color (:299-381) -- one lane per pixel: eye path to the first diffuse
 *                   hit, then Tree.fold_neighbors with the cone filter, summed in the reference's order
 */

struct PtLightDev {
  int32_t kind, pad;
  double pos[3];
  double color[3]; /* already scaled by the power */
  double rot[4];   /* spot: Shader_space.rotation (r, x, y, z) of Shader_space.create (normalize direction) position */
  double disk_radius; /* spot: Float.atan (0.5 * 45 * pi / 180), computed by the host's libm like the reference (:88-89) */
};

struct PtPhotonOut { /* [photon index][deposit k], deposit order */
  double *px, *py, *pz; /* Photon.center = Shader_space.world_origin */
  double *nx, *ny, *nz; /* world_normal */
  double *fx, *fy, *fz; /* flux */
  uint8_t* n_deposits;  /* per photon index */
};

struct PtPhotonMapDev {
  const PtNode* nodes; /* pre-order, leaf a = first slot, b = count */
  int32_t n_nodes, pad;
  const double *px, *py, *pz, *nx, *ny, *nz, *fx, *fy, *fz; /* in leaf-slot order */
};

/* Light.random_ray (:112-118) */
__device__ __forceinline__ void pt_light_random_ray(const PtLightDev& l, double u, double v, V3* o, V3* d) {
  const double pi = 3.14159265358979323846;
  if (l.kind == 0) { /* Point_light.random_direction :69-78 */
    const double theta = 2.0 * pi * u;
    const double phi = pt_acos(1.0 - (2.0 * v));
    double s_phi, c_phi, s_th, c_th;
    pt_sincos(phi, &s_phi, &c_phi);
    pt_sincos(theta, &s_th, &c_th);
    *o = v3(l.pos[0], l.pos[1], l.pos[2]);
    *d = v3(s_phi * c_th, s_phi * s_th, c_phi);
    return;
  }
  /* Spot_light.random_ray :97-105 */
  const double r = l.disk_radius * pt_sqrt(u);
  const double theta = v * 2.0 * pi;
  double sn, cs;
  pt_sincos(theta, &sn, &cs);
  Quat rot;
  rot.r = l.rot[0];
  rot.v = v3(l.rot[1], l.rot[2], l.rot[3]);
  const V3 dir = pt_quat_transform(pt_quat_conj(rot), v3(r * cs, r * sn, 1.0)); /* Shader_space.world_ray */
  *o = v3_add(v3(l.pos[0], l.pos[1], l.pos[2]), v3_scale(dir, 1e-3));
  *d = dir;
}

template <int MODE, bool IMG = false> /* IMG: scenes with an image texture (pt_shade_entry) */
__global__ __launch_bounds__(256) void k_ppm_photons(PtSceneDev sc, int stack_depth, const PtLightDev* __restrict__ lights,
                                                     int n_lights, const int* __restrict__ light_first /* n_lights+1 */,
                                                     int base_offset, const double* __restrict__ alpha, int max_bounces,
                                                     PtPhotonOut out, unsigned long long* __restrict__ ray_counter) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  const int lane = pt_lane(), wave_in_block = (int)(threadIdx.x >> 6);
  uint32_t* stack = (uint32_t*)lds_raw + (size_t)wave_in_block * stack_depth * PT_WAVE + lane;
  PtSceneView sv;
  sv.nodes = sc.nodes; sv.skip32 = nullptr; sv.nodes32 = nullptr; sv.nodes32o = nullptr; sv.n_nodes = (uint32_t)sc.n_nodes; sv.swz_nodes = nullptr; sv.swz_root = 0u; sv.top = lds_raw; sv.has_top = false; sv.sph = sc.sph; sv.tri = sc.tri; sv.kind = sc.slot_kind; sv.floor_lds = nullptr; sv.n_floor_lds = 0;
  const int total = light_first[n_lights];
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  unsigned long long rays = 0;
  if (i < total) {
    int li = 0;
    while (li + 1 < n_lights && i >= light_first[li + 1]) ++li;
    const PtLightDev L = lights[li];
    const int offset = i + base_offset; /* offset_sampler p_sampler (iteration * photon_count), :394-396 */
    double u = pt_lds_get(alpha, offset, 0), v = pt_lds_get(alpha, offset, 1);
    V3 o, d;
    pt_light_random_ray(L, u, v, &o, &d);
    V3 flux = v3(L.color[0], L.color[1], L.color[2]);
    int dim = 2, deposits = 0;
    for (int mb = max_bounces; mb > 0; --mb) {
      u = pt_lds_get(alpha, offset, dim); /* take_2d BEFORE the intersection test */
      v = pt_lds_get(alpha, offset, dim + 1);
      dim += 2;
      unsigned long long c0 = 0, c1 = 0, c2 = 0;
      ++rays;
      const PtTraceResult r = pt_trace_ray<MODE, false, false, uint32_t>(sc, sv, stack, o, d, c0, c1, c2);
      if (r.slot < 0) break;
      const PtMatRegs mat = pt_mat_load<PT_CAT_NONE, false>(sc.slot_shade + r.slot);
      const PtSurface sf = pt_surface_hit(sc, o, d, r.slot, r.t, r.u, r.v, mat, pt_slot_geom(sc, r.slot));
      const PtScatter scat = pt_material_scatter<PT_CAT_NONE, IMG>(sc, sf, mat, u);
      if (scat.kind == 0) break;
      const Quat rot_inv = pt_quat_conj(sf.rot);
      if (scat.kind == 1) {
        const V3 dir = pt_quat_transform(rot_inv, scat.wo);
        o = v3_add(sf.point, v3_scale(dir, 1e-3));
        d = dir;
        flux = v3_mul(flux, scat.attenuation);
        continue;
      }
      const V3 color = scat.attenuation;
      flux = v3_mul(flux, color);
      { /* Photon.create :123-126 (wi and the rotation are not read by the radiance estimate: not stored) */
        const size_t at = (size_t)i * (size_t)max_bounces + (size_t)deposits;
        out.px[at] = sf.point.x; out.py[at] = sf.point.y; out.pz[at] = sf.point.z;
        out.nx[at] = sf.normal.x; out.ny[at] = sf.normal.y; out.nz[at] = sf.normal.z;
        out.fx[at] = flux.x; out.fy[at] = flux.y; out.fz[at] = flux.z;
        ++deposits;
      }
      const double color_max = pt_base_max(color.x, pt_base_max(color.y, color.z)); /* Color.max_coord */
      if (!(u <= color_max)) break;
      const double cm_inv = 1.0 / color_max;
      flux = v3_scale(flux, cm_inv);
      const double u2 = u * cm_inv;
      const double pi = 3.14159265358979323846;
      const double rr = pt_sqrt(u2);
      const double theta = v * 2.0 * pi;
      double sn, cs;
      pt_sincos(theta, &sn, &cs);
      const V3 wo = v3(rr * cs, rr * sn, pt_sqrt(1.0 - u2)); /* unit_square_to_hemisphere */
      const V3 dir = pt_quat_transform(rot_inv, wo);
      o = v3_add(sf.point, v3_scale(dir, 1e-3));
      d = dir;
    }
    out.n_deposits[i] = (uint8_t)deposits;
  }
  rays = pt_wave_sum(rays);
  if (lane == 0 && rays) atomicAdd(ray_counter, rays);
}

/* Bbox.mem (bbox.ml:58-64) */
__device__ __forceinline__ bool pt_box_mem(const PtNode* n, V3 p) {
  return n->mn[0] <= p.x && p.x <= n->mx[0] && n->mn[1] <= p.y && p.y <= n->mx[1] && n->mn[2] <= p.z && p.z <= n->mx[2];
}

template <int MODE, bool IMG = false>
__global__ __launch_bounds__(256) void k_ppm_gather(PtSceneDev sc, int stack_depth, PtPhotonMapDev pm, double radius,
                                                    const double* __restrict__ alpha, int eye_base, int width, int height,
                                                    int max_bounces, double inv_photon_count, double* __restrict__ img_sum,
                                                    unsigned long long* __restrict__ counters /* [0] eye rays [1] neighbours */) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds_raw[];
  const int lane = pt_lane(), wave_in_block = (int)(threadIdx.x >> 6);
  uint32_t* stack = (uint32_t*)lds_raw + (size_t)wave_in_block * stack_depth * PT_WAVE + lane;
  PtSceneView sv;
  sv.nodes = sc.nodes; sv.skip32 = nullptr; sv.nodes32 = nullptr; sv.nodes32o = nullptr; sv.n_nodes = (uint32_t)sc.n_nodes; sv.swz_nodes = nullptr; sv.swz_root = 0u; sv.top = lds_raw; sv.has_top = false; sv.sph = sc.sph; sv.tri = sc.tri; sv.kind = sc.slot_kind; sv.floor_lds = nullptr; sv.n_floor_lds = 0;
  const int pixel = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  unsigned long long rays = 0, n_acc = 0;
  if (pixel < width * height) {
    const double pi = 3.14159265358979323846;
    const int x = pixel % width, y = pixel / width;
    const int offset = pixel + eye_base; /* offset_sampler e_sampler (i * width * height) */
    const double inv_widthf = 1.0 / (double)width, inv_heightf = 1.0 / (double)height;
    const double dx = pt_lds_get(alpha, offset, 0), dy = pt_lds_get(alpha, offset, 1);
    const double cx = inv_widthf * (dx + (double)x), cy = inv_heightf * (dy + (double)y);
    V3 o = v3(0.0, 0.0, 0.0), d = pt_camera_dir(sc, cx, cy);
    V3 beta = v3(1.0, 1.0, 1.0), color = v3(0.0, 0.0, 0.0);
    int dimension = 2;
    for (int mb = max_bounces; mb > 0;) {
      unsigned long long c0 = 0, c1 = 0, c2 = 0;
      ++rays;
      const PtTraceResult r = pt_trace_ray<MODE, false, false, uint32_t>(sc, sv, stack, o, d, c0, c1, c2);
      if (r.slot < 0) break;
      --mb;
      const double u = pt_lds_get(alpha, offset, dimension);
      const PtMatRegs mat = pt_mat_load<PT_CAT_NONE, false>(sc.slot_shade + r.slot);
      const PtSurface sf = pt_surface_hit(sc, o, d, r.slot, r.t, r.u, r.v, mat, pt_slot_geom(sc, r.slot));
      const PtScatter scat = pt_material_scatter<PT_CAT_NONE, IMG>(sc, sf, mat, u);
      if (scat.kind == 0) break;
      if (scat.kind == 1) {
        beta = v3_mul(scat.attenuation, beta);
        const V3 dir = pt_quat_transform(pt_quat_conj(sf.rot), scat.wo);
        o = v3_add(sf.point, v3_scale(dir, 1e-3));
        d = dir;
        dimension += 1;
        continue;
      }
      beta = v3_mul(scat.attenuation, beta);
      /* Photon_map.fold_neighbors (:188-194) over Tree.fold_neighbors (shape_tree.ml:222-231), walked in REVERSE
       * (rhs before lhs, leaf elements last to first): the reference conses the accepted photons and then folds
       * that list, i.e. it sums them in reverse visit order. */
      const V3 hp = sf.point, hn = sf.normal;
      const double r2 = radius * radius; /* Float.square p.radius */
      V3 flux = v3(0.0, 0.0, 0.0);
      unsigned long long found = 0;
      if (pm.n_nodes > 0) {
        int sp = 0;
        uint32_t node = 0;
        for (;;) {
          const PtNode* np = pm.nodes + node;
          bool descend = false;
          if (pt_box_mem(np, hp)) {
            const uint32_t na = np->a, nb = np->b;
            if ((nb >> 30) == PT_NODE_LEAF_AXIS) {
              const int first = (int)na, cnt = (int)(nb & 0x3fffffffu);
              for (int k = cnt - 1; k >= 0; --k) {
                const int s = first + k;
                const V3 c = v3(pm.px[s], pm.py[s], pm.pz[s]);
                if (v3_quadrance(v3_sub(hp, c)) < r2) {
                  if (v3_dot(v3(pm.nx[s], pm.ny[s], pm.nz[s]), hn) > 1e-3) {
                    const double distance = pt_sqrt(v3_quadrance(v3_sub(c, hp)));
                    const double w = (1.0 - (distance / (1.0 * radius))) / 1.0; /* cone filter, k = 1; pdf = 1 */
                    flux = v3_add(flux, v3_scale(v3(pm.fx[s], pm.fy[s], pm.fz[s]), w));
                    ++found;
                  }
                }
              }
            } else {
              stack[sp * PT_WAVE] = na; /* lhs later */
              ++sp;
              node = nb & 0x3fffffffu;  /* rhs first */
              descend = true;
            }
          }
          if (!descend) {
            if (sp == 0) break;
            --sp;
            node = stack[sp * PT_WAVE];
          }
        }
      }
      n_acc += found;
      if (found) {
        const double normalizer = 1.0 - (2.0 / (3.0 * 1.0));
        const double area = pi * (radius * radius);
        color = v3_scale(v3_mul(beta, flux), 1.0 / (area * normalizer));
      }
      break;
    }
    const V3 c = v3_scale(color, inv_photon_count);
    double* px = img_sum + ((size_t)(height - 1 - y) * width + x) * 3; /* write_pixel flips y (:305-313) */
    px[0] = c.x + px[0];
    px[1] = c.y + px[1];
    px[2] = c.z + px[2];
  }
  rays = pt_wave_sum(rays);
  n_acc = pt_wave_sum(n_acc);
  if (lane == 0) {
    atomicAdd(&counters[0], rays);
    atomicAdd(&counters[1], n_acc);
  }
}

/* ---- the photon list on the device ----
 * The reference conses every path's deposits and prepends every path's list (progressive_photon_map.ml:230,248), so
 * list position j runs over paths i = total-1 .. 0 and, inside a path, deposits k = n-1 .. 0.  A plain three-pass
 * exclusive scan over the REVERSED per-path deposit counts gives every path its first list position; the emit pass
 * also writes the Photon bbox (center -/+ radius, :150-156) the tree builder consumes. */
#define PPM_SCAN_TILE 1024
__global__ __launch_bounds__(256) void k_ppm_list_count(const uint8_t* __restrict__ ndep, int total, int* __restrict__ tile_sum) {
  __shared__ int s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  int c = 0;
  for (int q = 0; q < 4; ++q) {
    const int r = (int)blockIdx.x * PPM_SCAN_TILE + (int)threadIdx.x * 4 + q;
    if (r < total) c += (int)ndep[total - 1 - r];
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum, c);
  __syncthreads();
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = s_sum;
}
__global__ void k_ppm_list_offsets(int* __restrict__ tile_sum, int n_tiles, int* __restrict__ n_photons) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int acc = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const int c = tile_sum[t];
    tile_sum[t] = acc;
    acc += c;
  }
  *n_photons = acc;
}
__global__ __launch_bounds__(256) void k_ppm_list_emit(const uint8_t* __restrict__ ndep, int total, int max_bounces,
                                                       const int* __restrict__ tile_off, const double* __restrict__ px,
                                                       const double* __restrict__ py, const double* __restrict__ pz,
                                                       double radius, int* __restrict__ src, double* __restrict__ boxes) {
  __shared__ int s_wave[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int cnt[4], mine = 0;
  for (int q = 0; q < 4; ++q) {
    const int r = (int)blockIdx.x * PPM_SCAN_TILE + tid * 4 + q;
    cnt[q] = r < total ? (int)ndep[total - 1 - r] : 0;
    mine += cnt[q];
  }
  int incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int j = tile_off[blockIdx.x] + incl - mine;
  for (int w = 0; w < wave; ++w) j += s_wave[w];
  for (int q = 0; q < 4; ++q) {
    const int r = (int)blockIdx.x * PPM_SCAN_TILE + tid * 4 + q;
    const int i = total - 1 - r;
    for (int k = cnt[q] - 1; k >= 0; --k, ++j) {
      const int a0 = i * max_bounces + k;
      src[j] = a0;
      const double cx = px[a0], cy = py[a0], cz = pz[a0];
      double* b = boxes + (size_t)j * 6;
      b[0] = cx - radius; b[1] = cy - radius; b[2] = cz - radius;
      b[3] = cx + radius; b[4] = cy + radius; b[5] = cz + radius;
    }
  }
}
/* photon records into leaf-slot order: slot sl holds list element slot_prim[sl] = deposit src[...] */
__global__ void k_ppm_slots(const int* __restrict__ slot_prim, const int* __restrict__ src, int n_slots,
                            const double* __restrict__ out9 /* 9 arrays, stride cap */, size_t cap,
                            double* __restrict__ pm9 /* 9 arrays, stride n_slots */) {
  const int sl = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (sl >= n_slots) return;
  const size_t a0 = (size_t)src[slot_prim[sl]];
  for (int c = 0; c < 9; ++c) pm9[(size_t)c * n_slots + sl] = out9[(size_t)c * cap + a0];
}
