/* scene_host.cpp -- see scene_host.h.  One function per array (or family of arrays) of PtHostArrays; scene_assemble at the end
 * calls them in the order their inputs become available.  Contraction is off for this file like for the kernels: tri_frame and
 * the light table must carry the bits the shade step itself would compute. */
#include "scene_host.h"

#include "pt_display.h"
#include "pt_lds_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace {

const uint32_t kNone = 0xffffffffu; /* skip32: nothing follows */

int reject(std::string* msg, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  *msg = buf;
  return PTX_ERR_ARG;
}

bool is_leaf(const PtNode& nd) { return (nd.b >> 30) == PT_NODE_LEAF_AXIS; }
bool any_triangles(const ptx_scene_desc* d) { return d->n_triangles > 0 || d->n_floor_triangles > 0; }
V3 vertex(const ptx_scene_desc* d, int i) { return v3(d->vertex_x[i], d->vertex_y[i], d->vertex_z[i]); }
bool emits(const ptx_material& m) { return m.emit[0] != 0.0 || m.emit[1] != 0.0 || m.emit[2] != 0.0; }
/* trees that will be walked from HBM / L2 on images of their own: too large for the LDS image whatever else the scene holds
 * (pt_lds_placement answers PT_PLACE_HBM_OCT on the node count alone) */
bool beyond_lds(const std::vector<PtNode>& nd) {
  PtLdsIn in{};
  in.n_nodes = (int)std::min<size_t>(nd.size(), 0x7fffffff);
  return pt_lds_placement(in) == PT_PLACE_HBM_OCT;
}

/* the emissive tree triangles in build-list order */
void emissive_list(const ptx_scene_desc* d, PtHostArrays* h) {
  h->n_emissive_tris = 0;
  h->emissive_tris.clear();
  for (int i = 0; i < d->n_triangles; ++i) {
    if (!emits(d->materials[d->tri_material[i]])) continue;
    if (h->n_emissive_tris++ > PTX_MAX_LIGHT_TRIANGLES) continue;
    for (int v = 0; v < 3; ++v) {
      const V3 pnt = vertex(d, d->tri_indices[3 * i + v]);
      h->emissive_tris.insert(h->emissive_tris.end(), {pnt.x, pnt.y, pnt.z});
    }
  }
}

/* the emissive tree spheres in build-list order */
void emissive_sphere_list(const ptx_scene_desc* d, PtHostArrays* h) {
  h->n_emissive_spheres = 0;
  h->emissive_spheres.clear();
  for (int i = 0; i < d->n_spheres; ++i) {
    if (!emits(d->materials[d->sphere_material[i]])) continue;
    if (h->n_emissive_spheres++ > PTX_MAX_LIGHT_SPHERES) continue;
    h->emissive_spheres.insert(h->emissive_spheres.end(), {d->sphere_x[i], d->sphere_y[i], d->sphere_z[i], d->sphere_r[i]});
  }
}

/* sph / tri / tri_uv / kind / slot_mat in the order of h->slot_prim: leaf order, then the floor */
void slot_arrays(const ptx_scene_desc* d, PtHostArrays* h) {
  const int n_tri = d->n_triangles, n_slots = h->dev.n_slots, total_slots = (int)h->slot_prim.size();
  h->sph.assign((size_t)total_slots * 4, 0.0);
  if (any_triangles(d)) {
    h->tri.assign((size_t)total_slots * 10, 0.0);
    h->tri_uv.assign((size_t)total_slots * 6, 0.0);
  }
  h->kind.assign((size_t)total_slots, PT_SLOT_PAD);
  h->slot_mat.assign((size_t)total_slots, 0);
  const double qnan = pt_nan();
  for (int sl = 0; sl < n_slots; ++sl) {
    const int e = h->slot_prim[(size_t)sl];
    if (e < 0) { /* Float.nan padding, main.ml:185 */
      for (int k = 0; k < 4; ++k) h->sph[(size_t)sl * 4 + k] = qnan;
      continue;
    }
    if (e < n_tri) {
      h->kind[(size_t)sl] = PT_SLOT_TRIANGLE;
      h->slot_mat[(size_t)sl] = d->tri_material[e];
      for (int v = 0; v < 3; ++v) {
        const int vi = d->tri_indices[3 * e + v];
        h->tri[(size_t)sl * 10 + 3 * v] = d->vertex_x[vi];
        h->tri[(size_t)sl * 10 + 3 * v + 1] = d->vertex_y[vi];
        h->tri[(size_t)sl * 10 + 3 * v + 2] = d->vertex_z[vi];
      }
      std::memcpy(&h->tri_uv[(size_t)sl * 6], &d->tri_uv[6 * e], sizeof(double) * 6);
    } else {
      const int si = e - n_tri;
      h->kind[(size_t)sl] = PT_SLOT_SPHERE;
      h->slot_mat[(size_t)sl] = d->sphere_material[si];
      h->sph[(size_t)sl * 4] = d->sphere_x[si];
      h->sph[(size_t)sl * 4 + 1] = d->sphere_y[si];
      h->sph[(size_t)sl * 4 + 2] = d->sphere_z[si];
      h->sph[(size_t)sl * 4 + 3] = d->sphere_r[si];
    }
  }
  for (int f = 0; f < d->n_floor_triangles; ++f) {
    const int sl = n_slots + f;
    h->kind[(size_t)sl] = PT_SLOT_TRIANGLE;
    h->slot_mat[(size_t)sl] = d->floor_material[f];
    std::memcpy(&h->tri[(size_t)sl * 10], &d->floor_vertices[9 * f], sizeof(double) * 9);
    std::memcpy(&h->tri_uv[(size_t)sl * 6], &d->floor_uv[6 * f], sizeof(double) * 6);
  }
}

/* PtSceneDev.tri_frame: small scenes only (the table of a large mesh would be one more gathered line per segment) */
void tri_frame_table(const SceneOptions& opt, PtHostArrays* h) {
  const int total_slots = (int)h->kind.size();
  if (h->tri.empty() || total_slots > kTriFrameMaxSlots || !opt.tri_frame) return;
  h->tri_frame.assign((size_t)total_slots * PT_TRI_FRAME_DOUBLES, 0.0);
  for (int sl = 0; sl < total_slots; ++sl) {
    if (h->kind[(size_t)sl] != PT_SLOT_TRIANGLE) continue;
    const double* t = &h->tri[(size_t)sl * 10];
    const V3 g = pt_tri_normal(v3(t[0], t[1], t[2]), v3(t[3], t[4], t[5]), v3(t[6], t[7], t[8]));
    const Quat qf = pt_shader_rotation(g), qb = pt_shader_rotation(v3_neg(g));
    double* o = &h->tri_frame[(size_t)sl * PT_TRI_FRAME_DOUBLES];
    o[0] = g.x; o[1] = g.y; o[2] = g.z;
    o[4] = qf.r; o[5] = qf.v.x; o[6] = qf.v.y; o[7] = qf.v.z;
    o[8] = qb.r; o[9] = qb.v.x; o[10] = qb.v.y; o[11] = qb.v.z;
  }
}

/* the shading category of every slot, the material and texture tables, and the per-slot shading records (material + its
 * texture, flattened) */
void shading_records(const ptx_scene_desc* d, PtHostArrays* h) {
  const int total_slots = (int)h->kind.size();
  h->cat.assign((size_t)total_slots, PT_CAT_NONE);
  for (int sl = 0; sl < total_slots; ++sl) {
    if (h->kind[(size_t)sl] == PT_SLOT_PAD) continue;
    const ptx_material& m = d->materials[h->slot_mat[(size_t)sl]];
    const bool checker = m.kind != PTX_MAT_DIELECTRIC && d->textures[m.texture].kind == PTX_TEX_CHECKER;
    h->cat[(size_t)sl] = m.kind == PTX_MAT_DIELECTRIC ? PT_CAT_DIELECTRIC : (m.kind == PTX_MAT_METAL ? PT_CAT_METAL : (checker ? PT_CAT_LAMBERT_CHECKER : PT_CAT_LAMBERT_SOLID));
  }
  h->mats.resize((size_t)d->n_materials);
  for (int i = 0; i < d->n_materials; ++i) {
    PtMaterial& m = h->mats[(size_t)i];
    std::memset(&m, 0, sizeof m);
    m.kind = d->materials[i].kind;
    m.texture = d->materials[i].kind == PTX_MAT_DIELECTRIC ? 0 : d->materials[i].texture;
    m.index = d->materials[i].index;
    std::memcpy(m.emit, d->materials[i].emit, sizeof m.emit);
  }
  h->texs.resize((size_t)std::max(d->n_textures, 1));
  std::memset(h->texs.data(), 0, sizeof(PtTexture) * h->texs.size());
  for (int i = 0; i < d->n_textures; ++i) {
    PtTexture& t = h->texs[(size_t)i];
    t.kind = d->textures[i].kind;
    t.width = d->textures[i].width;
    t.height = d->textures[i].height;
    std::memcpy(t.even, d->textures[i].even, sizeof t.even);
    std::memcpy(t.odd, d->textures[i].odd, sizeof t.odd);
  }
  h->shade.assign((size_t)total_slots, PtShadeRec{});
  for (int sl = 0; sl < total_slots; ++sl) {
    if (h->kind[(size_t)sl] == PT_SLOT_PAD) continue;
    const PtMaterial& m = h->mats[(size_t)h->slot_mat[(size_t)sl]];
    PtShadeRec& r = h->shade[(size_t)sl];
    r.kind = m.kind;
    r.index = m.index;
    std::memcpy(r.emit, m.emit, sizeof r.emit);
    if (m.kind != PTX_MAT_DIELECTRIC) {
      const PtTexture& t = h->texs[(size_t)m.texture];
      r.tex_kind = t.kind; r.tex_w = t.width; r.tex_h = t.height;
      std::memcpy(r.even, t.even, sizeof r.even);
      std::memcpy(r.odd, t.odd, sizeof r.odd);
    }
  }
}

/* the scalars of PtSceneDev that come straight from the descriptor (scene_set_tree has set n_nodes, n_slots, depth) */
void dev_scalars(const ptx_scene_desc* d, PtSceneDev* dv) {
  dv->mode = d->leaf_kind == PTX_LEAF_SIMD ? PT_MODE_SIMD : PT_MODE_ARRAY;
  dv->all_triangles = (d->n_triangles > 0 && d->n_spheres == 0) ? 1 : 0;
  dv->n_floor = d->n_floor_triangles;
  dv->has_triangles = any_triangles(d) ? 1 : 0;
  for (int i = 0; i < d->n_materials; ++i)
    if (emits(d->materials[i])) dv->has_emit = 1;
  for (int i = 0; i < d->n_textures; ++i)
    if (d->textures[i].kind == PTX_TEX_CHECKER) dv->has_checker = 1;
  dv->cam_llx = d->camera.lower_left_x; dv->cam_lly = d->camera.lower_left_y; dv->cam_vx = d->camera.view_x; dv->cam_vy = d->camera.view_y;
  dv->bg_kind = d->background.kind;
  std::memcpy(dv->bg_horizon, d->background.horizon, sizeof dv->bg_horizon);
  std::memcpy(dv->bg_zenith, d->background.zenith, sizeof dv->bg_zenith);
}

/* skip32: the tree threaded per direction octant (shape_tree.ml:201,209: bit `axis` of the octant set = lhs first) */
void thread_octants(PtHostArrays* h) {
  const std::vector<PtNode>& nd = h->nodes;
  h->skip32.assign(nd.size() * 8, kNone);
  std::vector<std::pair<uint32_t, uint32_t>> todo; /* (node, what follows its subtree) */
  for (uint32_t o = 0; o < 8; ++o) {
    todo.clear();
    todo.emplace_back(0u, kNone);
    while (!todo.empty()) {
      const auto [k, next] = todo.back();
      todo.pop_back();
      h->skip32[(size_t)k * 8 + o] = next;
      const uint32_t axis = nd[k].b >> 30;
      if (axis == PT_NODE_LEAF_AXIS) continue;
      const uint32_t lhs = nd[k].a, rhs = nd[k].b & 0x3fffffffu;
      const bool lhs_first = (o >> axis) & 1u;
      const uint32_t near_c = lhs_first ? lhs : rhs, far_c = lhs_first ? rhs : lhs;
      todo.emplace_back(near_c, far_c);
      todo.emplace_back(far_c, next);
    }
  }
}

/* nodes32: mn.xyz, mx.xyz rounded to binary32, a, b (leaf b: padded count | real count << 15 | tag) */
void binary32_image(PtHostArrays* h) {
  const std::vector<PtNode>& nd = h->nodes;
  h->nodes32.resize(nd.size() * 8);
  for (size_t k = 0; k < nd.size(); ++k) {
    uint32_t* w = &h->nodes32[k * 8];
    for (int a = 0; a < 3; ++a) {
      const float lo = (float)nd[k].mn[a], hi = (float)nd[k].mx[a];
      std::memcpy(&w[a], &lo, 4);
      std::memcpy(&w[3 + a], &hi, 4);
    }
    w[6] = nd[k].a;
    w[7] = is_leaf(nd[k]) ? ((nd[k].b & 0x7fffu) | ((nd[k].pad[0] & 0x7fffu) << 15) | (PT_NODE_LEAF_AXIS << 30)) : nd[k].b;
  }
}

/* nodes32o: the per-octant tagged image for trees that will be walked from HBM / L2, from nodes32 and skip32 */
void octant_image(const SceneOptions& opt, PtHostArrays* h) {
  const std::vector<PtNode>& nd = h->nodes;
  if (!opt.oct_image || !beyond_lds(nd) || nd.size() * 8 >= 0xffffffffull / 32u) return;
  for (size_t k = 0; k < nd.size(); ++k) {
    const bool ok = is_leaf(nd[k]) ? nd[k].a < (1u << PT_OCT_LEAF_FIRST_BITS) && nd[k].pad[0] <= PT_OCT_LEAF_REAL_MAX
                                   : nd[k].a == (uint32_t)k + 1u; /* pre-order: the lhs child follows its parent */
    if (!ok) return;
  }
  h->nodes32o.resize(nd.size() * 64);
  for (uint32_t o = 0; o < 8; ++o)
    for (size_t k = 0; k < nd.size(); ++k) {
      uint32_t* w = &h->nodes32o[((size_t)o * nd.size() + k) * 8];
      /* the tagged record (pt_scene.h, PT_OCT_*): near xyz, far xyz for this octant's direction signs (bit a set = component
       * a >= 0: near = mn), what a hit leads to, what a miss leads to */
      const uint32_t* b32 = &h->nodes32[k * 8]; /* mn.xyz, mx.xyz as binary32 */
      for (int a = 0; a < 3; ++a) {
        const bool pos = (o >> a) & 1u;
        w[a] = pos ? b32[a] : b32[3 + a];
        w[3 + a] = pos ? b32[3 + a] : b32[a];
      }
      const uint32_t axis = nd[k].b >> 30;
      /* links are record numbers in the whole image (this octant's base added), as the walk's `node` is */
      const uint32_t obase = o * (uint32_t)nd.size();
      w[6] = is_leaf(nd[k]) ? (PT_OCT_LEAF_TAG | (nd[k].pad[0] << PT_OCT_LEAF_FIRST_BITS) | nd[k].a)
                            : obase + (((o >> axis) & 1u) ? nd[k].a : (nd[k].b & 0x3fffffffu)); /* shape_tree.ml:209: lhs first where the component is >= 0 */
      const uint32_t sk = h->skip32[k * 8 + o];
      w[7] = sk == kNone ? PT_OCT_END : obase + sk;
    }
}

/* lds_oct: the per-octant LDS image of a small Simd_leaf tree (pt_scene.h, PT_LOCT_*), from nodes32 and skip32 like nodes32o: per
 * (octant, node) near xyz, far xyz, hit link | miss link << 16, the magnitude word of the shared LDS image; then the leaf table */
void lds_octant_image(const SceneOptions& opt, PtHostArrays* h) {
  const std::vector<PtNode>& nd = h->nodes;
  if (!opt.lds_oct || h->dev.mode != PT_MODE_SIMD || nd.empty() || nd.size() > (size_t)PT_LOCT_MAX_NODES) return;
  for (const PtNode& k : nd)
    if (is_leaf(k) && (k.a > 0xffffu || k.pad[0] > 0xffffu)) return;
  { /* a tree whose image alone, before any parked entry, is beyond what a launch may ask for can never be admitted (pt_lds_oct_layout) */
    PtLdsIn in{};
    in.mode = PT_MODE_SIMD;
    in.n_nodes = (int)nd.size();
    in.total_slots = h->dev.n_slots + h->dev.n_floor;
    if (pt_lds_oct_layout(in).end > PT_LDS_BOUNCE_LIMIT) return;
  }
  const uint32_t n = (uint32_t)nd.size();
  h->lds_oct.assign((size_t)n * 64 + PT_LOCT_LEAF_WORDS(n), 0u);
  for (uint32_t o = 0; o < 8; ++o)
    for (uint32_t k = 0; k < n; ++k) {
      uint32_t* w = &h->lds_oct[((size_t)o * n + k) * 8];
      const uint32_t* b32 = &h->nodes32[(size_t)k * 8]; /* mn.xyz, mx.xyz as binary32 */
      float mag = 0.0f;
      for (int a = 0; a < 3; ++a) {
        const bool pos = (o >> a) & 1u; /* bit a set = component a >= 0: near = mn */
        w[a] = pos ? b32[a] : b32[3 + a];
        w[3 + a] = pos ? b32[3 + a] : b32[a];
        float lo, hi;
        std::memcpy(&lo, &b32[a], 4);
        std::memcpy(&hi, &b32[3 + a], 4);
        mag = std::fmax(mag, std::fmax(std::fabs(lo), std::fabs(hi)));
      }
      const uint32_t axis = nd[k].b >> 30, obase = o * n;
      /* a hit: an inner node's near child (shape_tree.ml:209: lhs first where the component is >= 0), a leaf's own record under
       * "holds a leaf"; a miss -- and the end of a leaf -- the octant's skip link */
      const uint32_t hit = is_leaf(nd[k]) ? (PT_LOCT_LEAF_TAG | (obase + k)) : obase + (((o >> axis) & 1u) ? nd[k].a : (nd[k].b & 0x3fffffffu));
      const uint32_t sk = h->skip32[(size_t)k * 8 + o];
      w[6] = hit | ((sk == kNone ? PT_LOCT_END : obase + sk) << 16);
      /* as pt_scene_view stores it in the shared image: rounded up, the two lowest mantissa bits carry the axis */
      const float up = mag * 1.000001f;
      uint32_t mb;
      std::memcpy(&mb, &up, 4);
      w[7] = ((mb + 4u) & ~3u) | axis;
    }
  for (uint32_t k = 0; k < n; ++k)
    if (is_leaf(nd[k])) h->lds_oct[(size_t)n * 64 + k] = nd[k].a | (nd[k].pad[0] << 16);
}

/* top_nodes / skip32_top: the top of a tree that is too large for LDS as a whole, a breadth-first prefix */
void top_image(const SceneOptions& opt, PtHostArrays* h) {
  const std::vector<PtNode>& nd = h->nodes;
  const size_t want_top = (size_t)std::max(0, std::min(1023, opt.top_nodes));
  if (want_top == 0 || !beyond_lds(nd) || nd.size() >= (size_t)PT_TOP_FLAG) return;
  std::vector<uint32_t> bfs; /* top slot -> node */
  std::vector<int32_t> slot_of(nd.size(), -1);
  bfs.push_back(0u);
  for (size_t t = 0; t < bfs.size() && bfs.size() < want_top; ++t) {
    const uint32_t k = bfs[t];
    if (is_leaf(nd[k])) continue;
    /* both children or neither: a top node's skip targets are siblings of its ancestors, so siblings travel together */
    if (bfs.size() + 2 > want_top) break;
    bfs.push_back(nd[k].a);
    bfs.push_back(nd[k].b & 0x3fffffffu);
  }
  for (size_t t = 0; t < bfs.size(); ++t) slot_of[bfs[t]] = (int32_t)t;
  auto enc = [&](uint32_t node) { return slot_of[node] >= 0 ? (PT_TOP_FLAG | (uint32_t)slot_of[node] * PT_TOP_NODE_BYTES) : node; };
  h->top_nodes.assign(bfs.size() * 16, 0u);
  bool ok = true;
  for (size_t t = 0; t < bfs.size(); ++t) {
    const uint32_t k = bfs[t];
    uint32_t* w = &h->top_nodes[t * 16];
    std::memcpy(w, &h->nodes32[(size_t)k * 8], 6 * sizeof(uint32_t)); /* the same binary32 bounds */
    w[6] = is_leaf(nd[k]) ? nd[k].a : enc(nd[k].a);
    w[7] = is_leaf(nd[k]) ? h->nodes32[(size_t)k * 8 + 7] : ((nd[k].b & 0xc0000000u) | enc(nd[k].b & 0x3fffffffu));
    for (int o = 0; o < 8; ++o) { /* words 8 .. 11: eight 16-bit skip links, byte offsets into this image */
      const uint32_t nx = h->skip32[(size_t)k * 8 + o];
      uint16_t sk = 0xffffu;
      if (nx != kNone && slot_of[nx] < 0) ok = false; /* cannot happen: see above */
      else if (nx != kNone) sk = (uint16_t)((uint32_t)slot_of[nx] * PT_TOP_NODE_BYTES);
      std::memcpy((unsigned char*)(w + 8) + 2 * o, &sk, 2);
    }
    w[12] = k;
  }
  if (ok && bfs.size() >= 3) {
    h->skip32_top = h->skip32;
    for (uint32_t& v : h->skip32_top)
      if (v != kNone) v = enc(v);
  } else {
    h->top_nodes.clear();
  }
}

/* skip: the LDS image's 16-bit copy of skip32 */
void skip16_copy(PtHostArrays* h) {
  if (h->nodes.size() >= 65535) return;
  h->skip.resize(h->skip32.size());
  for (size_t i = 0; i < h->skip32.size(); ++i) h->skip[i] = (uint16_t)(h->skip32[i] == kNone ? 0xffffu : h->skip32[i]);
}

/* cyclic Jacobi on the symmetric 3x3 `cov`: it becomes (nearly) diagonal, the columns of v the eigenvectors */
void jacobi3(double cov[3][3], double v[3][3]) {
  for (int sweep = 0; sweep < 12; ++sweep)
    for (int p2 = 0; p2 < 3; ++p2)
      for (int q2 = p2 + 1; q2 < 3; ++q2) {
        if (std::fabs(cov[p2][q2]) < 1e-300) continue;
        const double th = 0.5 * std::atan2(2.0 * cov[p2][q2], cov[q2][q2] - cov[p2][p2]);
        const double cs = std::cos(th), sn = std::sin(th);
        for (int k = 0; k < 3; ++k) { /* rotate columns p2, q2 of cov and v */
          const double a1 = cov[k][p2], a2 = cov[k][q2];
          cov[k][p2] = cs * a1 - sn * a2; cov[k][q2] = sn * a1 + cs * a2;
          const double v1 = v[k][p2], v2 = v[k][q2];
          v[k][p2] = cs * v1 - sn * v2; v[k][q2] = sn * v1 + cs * v2;
        }
        for (int k = 0; k < 3; ++k) { /* and rows */
          const double a1 = cov[p2][k], a2 = cov[q2][k];
          cov[p2][k] = cs * a1 - sn * a2; cov[q2][k] = sn * a1 + cs * a2;
        }
      }
}

/* The bin key of the shade step (sort_axis / sort_by_* / root_*).  sort_axis: smallest-variance direction of the primitive
 * centres, the 5 % largest primitives left out (a ground sphere of radius 1000 is not part of the "slab" the small ones lie
 * in); oriented away from those large ones */
void bin_key(const std::vector<Box>& boxes, const SceneOptions& opt, PtHostArrays* h) {
  PtSceneDev& dv = h->dev;
  const std::vector<PtNode>& nodes = h->nodes;
  const int n = (int)boxes.size();
  std::vector<std::pair<double, int>> by_size((size_t)n);
  for (int i = 0; i < n; ++i) {
    const Box& b = boxes[(size_t)i];
    by_size[(size_t)i] = {(b.mx.x - b.mn.x) + (b.mx.y - b.mn.y) + (b.mx.z - b.mn.z), i};
  }
  std::sort(by_size.begin(), by_size.end());
  const int keep = std::max(1, n - n / 20);
  double mean[3] = {0, 0, 0}, big[3] = {0, 0, 0};
  auto centre = [&](int i, double c[3]) {
    const Box& b = boxes[(size_t)i];
    c[0] = 0.5 * (b.mn.x + b.mx.x); c[1] = 0.5 * (b.mn.y + b.mx.y); c[2] = 0.5 * (b.mn.z + b.mx.z);
  };
  for (int k = 0; k < keep; ++k) {
    double c[3];
    centre(by_size[(size_t)k].second, c);
    for (int a = 0; a < 3; ++a) mean[a] += c[a] / keep;
  }
  double cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int k = 0; k < keep; ++k) {
    double c[3];
    centre(by_size[(size_t)k].second, c);
    for (int a = 0; a < 3; ++a)
      for (int b2 = 0; b2 < 3; ++b2) cov[a][b2] += (c[a] - mean[a]) * (c[b2] - mean[b2]);
  }
  for (int k = keep; k < n; ++k) {
    double c[3];
    centre(by_size[(size_t)k].second, c);
    for (int a = 0; a < 3; ++a) big[a] += c[a] - mean[a];
  }
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  jacobi3(cov, v);
  int best = 0;
  for (int a = 1; a < 3; ++a)
    if (cov[a][a] < cov[best][best]) best = a;
  double ax[3] = {v[0][best], v[1][best], v[2][best]};
  const double len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  int worst = 0;
  for (int a = 1; a < 3; ++a)
    if (cov[a][a] > cov[worst][worst]) worst = a;
  dv.sort_by_elevation = (keep >= 16 && cov[best][best] < 0.02 * cov[worst][worst]) ? 1 : 0;
  /* a floor tested before the tree (ganesha's checker floor): most bounce rays start on it, outside the tree's box */
  dv.sort_by_root = (!dv.sort_by_elevation && dv.n_floor > 0 && !nodes.empty()) ? 1 : 0;
  if (opt.bin_key >= 0) {
    dv.sort_by_elevation = opt.bin_key == 1;
    dv.sort_by_root = (opt.bin_key == 2 && !nodes.empty()) ? 1 : 0;
  }
  double root_mag = 0.0;
  for (int a = 0; a < 3 && !nodes.empty(); ++a) {
    dv.root_mn[a] = (float)nodes[0].mn[a];
    dv.root_mx[a] = (float)nodes[0].mx[a];
    root_mag = std::fmax(root_mag, std::fmax(std::fabs(nodes[0].mn[a]), std::fabs(nodes[0].mx[a])));
  }
  /* rounded up; a NaN or a value beyond binary32 becomes +inf, which sends every ray of the scene to the binary64 test */
  dv.root_mag = (root_mag < 3.0e38) ? (float)(root_mag * 1.0000002) : INFINITY;
  dv.pad_f = 0.0f;
  const double toward_big = ax[0] * big[0] + ax[1] * big[1] + ax[2] * big[2];
  for (int a = 0; a < 3; ++a) dv.sort_axis[a] = (len > 0 && std::isfinite(len)) ? (toward_big > 0 ? -ax[a] : ax[a]) / len : (a == 1 ? 1.0 : 0.0);
}

}  // namespace

SceneOptions scene_options_from_env() {
  auto env_int = [](const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
  };
  SceneOptions o;
  o.tri_frame = env_int("PTX_TRI_FRAME", 1);
  o.oct_image = env_int("PTX_OCT_IMAGE", 1);
  o.lds_oct = env_int("PTX_LDS_OCT", 1);
  o.tile_lists = env_int("PTX_TILE_LISTS", 1);
  o.top_nodes = std::max(0, std::min(1023, env_int("PTX_TOP_NODES", 512)));
  if (std::getenv("PTX_BIN_KEY")) { /* any other value: by octant */
    const int k = env_int("PTX_BIN_KEY", 0);
    o.bin_key = (k == 1 || k == 2) ? k : 0;
  }
  return o;
}

int scene_check_desc(const ptx_scene_desc* d, std::string* msg) {
  const int n_tri = d->n_triangles, n_sph = d->n_spheres;
  if (n_tri < 0 || n_sph < 0 || d->n_floor_triangles < 0) return reject(msg, "negative primitive count");
  if (n_tri + n_sph == 0) return reject(msg, "Shape_tree.create: expected non-empty list of shapes");
  if (d->leaf_kind != PTX_LEAF_SIMD && d->leaf_kind != PTX_LEAF_ARRAY) return reject(msg, "unknown leaf_kind %d", d->leaf_kind);
  if (d->leaf_kind == PTX_LEAF_SIMD && (n_tri > 0 || d->n_floor_triangles > 0)) return reject(msg, "Simd_leaf holds spheres only");
  if (d->leaf_kind == PTX_LEAF_SIMD && d->length_cutoff > 16) return reject(msg, "Simd_leaf length_cutoff must be <= leaf_size () = 16");
  if (d->length_cutoff < 1) return reject(msg, "length_cutoff must be >= 1");
  if (scene_num_bins(d) < 4) return reject(msg, "num_bins must be >= 4 (shape_tree.ml:253)");
  if (d->n_materials <= 0 || !d->materials) return reject(msg, "no materials");
  if (n_sph > 0 && !(d->sphere_x && d->sphere_y && d->sphere_z && d->sphere_r && d->sphere_material)) return reject(msg, "sphere arrays missing");
  if (n_tri > 0 && !(d->vertex_x && d->vertex_y && d->vertex_z && d->tri_indices && d->tri_uv && d->tri_material)) return reject(msg, "triangle arrays missing");
  if (d->n_floor_triangles > 0 && !(d->floor_vertices && d->floor_uv && d->floor_material)) return reject(msg, "floor arrays missing");
  for (int i = 0; i < d->n_materials; ++i) {
    const ptx_material& m = d->materials[i];
    if (m.kind < 0 || m.kind > 2) return reject(msg, "material %d: unknown kind %d", i, m.kind);
    if (m.kind != PTX_MAT_DIELECTRIC && (m.texture < 0 || m.texture >= d->n_textures)) return reject(msg, "material %d: texture %d out of range", i, m.texture);
  }
  if (d->n_textures > 0 && !d->textures) return reject(msg, "texture array missing");
  for (int i = 0; i < d->n_textures; ++i)
    if (d->textures[i].kind != PTX_TEX_CHECKER && d->textures[i].kind != PTX_TEX_SOLID) return reject(msg, "texture %d: unknown kind", i);
  auto mat_ok = [&](int m) { return m >= 0 && m < d->n_materials; };
  for (int i = 0; i < n_tri; ++i) {
    const int ia = d->tri_indices[3 * i], ib = d->tri_indices[3 * i + 1], ic = d->tri_indices[3 * i + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= d->n_vertices || ib >= d->n_vertices || ic >= d->n_vertices) return reject(msg, "triangle %d: vertex index out of range", i);
    if (!mat_ok(d->tri_material[i])) return reject(msg, "triangle %d: material out of range", i);
  }
  for (int i = 0; i < n_sph; ++i)
    if (!mat_ok(d->sphere_material[i])) return reject(msg, "sphere %d: material out of range", i);
  for (int f = 0; f < d->n_floor_triangles; ++f)
    if (!mat_ok(d->floor_material[f])) return reject(msg, "floor triangle %d: material out of range", f);
  return 0;
}

std::vector<Box> scene_boxes(const ptx_scene_desc* d) {
  const int n_tri = d->n_triangles, n_sph = d->n_spheres;
  std::vector<Box> boxes((size_t)(n_tri + n_sph));
  for (int i = 0; i < n_tri; ++i) {
    /* Triangle.bbox (triangle.ml:67-72): lo (lo a b) c */
    Box ab, c;
    ab.mn = ab.mx = vertex(d, d->tri_indices[3 * i]);
    Box bb;
    bb.mn = bb.mx = vertex(d, d->tri_indices[3 * i + 1]);
    c.mn = c.mx = vertex(d, d->tri_indices[3 * i + 2]);
    boxes[(size_t)i] = box_union(box_union(ab, bb), c);
  }
  for (int i = 0; i < n_sph; ++i) {
    /* Sphere.bbox (sphere.ml:16-19): centre + (-r), centre + r */
    const V3 c = v3(d->sphere_x[i], d->sphere_y[i], d->sphere_z[i]);
    const double r = d->sphere_r[i];
    Box b;
    b.mn = v3(c.x + (-r), c.y + (-r), c.z + (-r));
    b.mx = v3(c.x + r, c.y + r, c.z + r);
    boxes[(size_t)(n_tri + i)] = b;
  }
  return boxes;
}

int scene_set_tree(const ptx_scene_desc* d, BvhResult&& tree, PtHostArrays* h, std::string* msg) {
  for (const PtNode& nd : tree.nodes)
    if (is_leaf(nd) && (nd.b & 0x3fffffffu) > 0x7fffu) return reject(msg, "a leaf holds more than 32767 slots (coincident centroids?)");
  if (d->leaf_kind == PTX_LEAF_SIMD) {
    for (const PtNode& nd : tree.nodes)
      if (is_leaf(nd) && (nd.b & 0x3fffffffu) > 16u) return reject(msg, "a Simd_leaf packet would exceed 16 lanes (coincident centroids?)");
  }
  h->nodes = std::move(tree.nodes);
  h->slot_prim = std::move(tree.slot_prim);
  std::memset(&h->dev, 0, sizeof h->dev);
  h->dev.n_nodes = (int)h->nodes.size();
  h->dev.n_slots = (int)h->slot_prim.size();
  h->dev.depth = tree.depth;
  h->n_textures = d->n_textures;
  for (int f = 0; f < d->n_floor_triangles; ++f) h->slot_prim.push_back(d->n_triangles + d->n_spheres + f);
  emissive_list(d, h);
  emissive_sphere_list(d, h);
  return 0;
}

void scene_assemble(const ptx_scene_desc* d, const std::vector<Box>& boxes, const SceneOptions& opt, PtHostArrays* h) {
  slot_arrays(d, h);
  tri_frame_table(opt, h);
  shading_records(d, h);
  dev_scalars(d, &h->dev);
  thread_octants(h);
  binary32_image(h);
  octant_image(opt, h);
  lds_octant_image(opt, h);
  top_image(opt, h);
  skip16_copy(h);
  bin_key(boxes, opt, h);
  h->tile_lists = opt.tile_lists != 0;
}

/* n = normalize(cross(b - a, c - a)) (pt_tri_normal: the host's pt_hypot chain, like tri_frame) and
 * A = 0.5 * sqrt(quadrance(cross(b - a, c - a))); cum = the running sum of the areas */
std::vector<double> light_table_build(const PtHostArrays& h) {
  const int n = h.n_emissive_tris;
  std::vector<double> table((size_t)n * PT_LIGHT_DOUBLES, 0.0);
  double cum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double* t = &h.emissive_tris[(size_t)k * 9];
    const V3 a = v3(t[0], t[1], t[2]), b = v3(t[3], t[4], t[5]), c = v3(t[6], t[7], t[8]);
    const V3 nrm = pt_tri_normal(a, b, c);
    const double area = 0.5 * std::sqrt(v3_quadrance(v3_cross(v3_sub(b, a), v3_sub(c, a))));
    cum = cum + area;
    double* o = &table[(size_t)k * PT_LIGHT_DOUBLES];
    std::memcpy(o, t, sizeof(double) * 9);
    o[9] = nrm.x; o[10] = nrm.y; o[11] = nrm.z;
    o[PT_LIGHT_AREA] = area;
    o[PT_LIGHT_CUM] = cum;
  }
  return table;
}

/* include/ptx.h, "cone-sampling emissive spheres": r2 = r * r, W = (2.0 * pi) * r2, cum runs on from the triangles' total */
std::vector<double> sphere_light_table_build(const PtHostArrays& h, double cum) {
  const double pi = 3.14159265358979323846;
  const int n = std::min(h.n_emissive_spheres, (int)(h.emissive_spheres.size() / 4));
  std::vector<double> table((size_t)n * PT_SLIGHT_DOUBLES, 0.0);
  for (int k = 0; k < n; ++k) {
    const double* sp = &h.emissive_spheres[(size_t)k * 4];
    double* o = &table[(size_t)k * PT_SLIGHT_DOUBLES];
    const double r2 = sp[3] * sp[3], w = (2.0 * pi) * r2;
    cum = cum + w;
    std::memcpy(o, sp, sizeof(double) * 4);
    o[PT_SLIGHT_R2] = r2;
    o[PT_SLIGHT_W] = w;
    o[PT_SLIGHT_CUM] = cum;
  }
  return table;
}

/* ---- image textures and the environment (scene_host.h) ---- */
int scene_check_image(const ptx_image* img, bool environment, std::string* msg) {
  const char* what = environment ? "environment" : "texture image";
  if (img->width < 1 || img->width > PTX_IMAGE_MAX_SIZE || img->height < 1 || img->height > PTX_IMAGE_MAX_SIZE)
    return reject(msg, "%s size %d x %d: width and height must be in [1, %d]", what, img->width, img->height, PTX_IMAGE_MAX_SIZE);
  const int known = PTX_IMAGE_BILINEAR | PTX_IMAGE_REPEAT_U | PTX_IMAGE_REPEAT_V;
  if (img->flags & ~known) return reject(msg, "%s: unknown bits in flags (0x%x)", what, (unsigned)img->flags);
  if (environment && (img->flags & ~PTX_IMAGE_BILINEAR))
    return reject(msg, "environment: a repeat flag is not accepted (an environment repeats in u and clamps in v); only PTX_IMAGE_BILINEAR is");
  if (img->reserved != 0) return reject(msg, "%s: reserved must be 0 (got %d)", what, img->reserved);
  if (!img->rgb) return reject(msg, "%s: rgb is NULL", what);
  const size_t n = (size_t)img->width * (size_t)img->height * 3;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(img->rgb[i]))
      return reject(msg, "%s: texel (%zu, %zu) channel %zu is not finite", what, (i / 3) % (size_t)img->width, (i / 3) / (size_t)img->width, i % 3);
  return 0;
}

std::vector<double> scene_image_records(const ptx_image* img) {
  const size_t n = (size_t)img->width * (size_t)img->height;
  std::vector<double> rec(n * 4, 0.0);
  for (size_t i = 0; i < n; ++i) std::memcpy(&rec[i * 4], &img->rgb[i * 3], sizeof(double) * 3);
  return rec;
}

void scene_image_overrides(const PtHostArrays& h, const std::vector<PtImageEntry>& entries, std::vector<uint8_t>* cat,
                           std::vector<PtShadeRec>* shade) {
  *cat = h.cat;
  *shade = h.shade;
  for (size_t sl = 0; sl < h.kind.size(); ++sl) {
    if (h.kind[sl] == PT_SLOT_PAD) continue;
    const PtMaterial& m = h.mats[(size_t)h.slot_mat[sl]];
    if (m.kind == PTX_MAT_DIELECTRIC || (size_t)m.texture >= entries.size()) continue;
    const PtImageEntry& e = entries[(size_t)m.texture];
    if (e.width == 0) continue;
    PtShadeRec& r = (*shade)[sl];
    r.tex_kind = PT_TEX_IMAGE;
    r.tex_w = e.width;
    r.tex_h = e.height;
    const uint64_t flags = (uint64_t)(uint32_t)e.flags;
    std::memset(r.even, 0, sizeof r.even);
    std::memset(r.odd, 0, sizeof r.odd);
    std::memcpy(&r.even[0], &e.texels, sizeof(uint64_t));
    std::memcpy(&r.even[1], &flags, sizeof(uint64_t));
    if (m.kind == PTX_MAT_LAMBERTIAN) (*cat)[sl] = PT_CAT_LAMBERT_CHECKER;
  }
}

/* ---- the density over the environment image (include/ptx.h states the rule; every expression keeps its grouping) ---- */
int scene_check_env_rotation(const double R[9], std::string* msg) {
  double worst = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = (R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2];
      const double e = std::fabs(g - (i == j ? 1.0 : 0.0));
      if (!(e <= worst)) worst = e; /* (a NaN stays) */
    }
  if (!(worst <= 1e-9))
    return reject(msg, "environment sampling needs a rotation: max |R R^T - I| = %g exceeds 1e-9", worst);
  return 0;
}

int scene_env_density(const double* rec, int32_t width, int32_t height, PtEnvDensity* out, std::string* msg) {
  const double pi = 3.14159265358979323846;
  const size_t W = (size_t)width, H = (size_t)height;
  out->width = width;
  out->height = height;
  out->last_row = 0;
  out->table.assign(PT_ENVD_SIZE(W, H), 0.0);
  double* m = out->table.data() + PT_ENVD_ROWS;
  double* lastx = out->table.data() + PT_ENVD_LASTX(H);
  double* cond = out->table.data() + PT_ENVD_COND(H);
  double* wt = out->table.data() + PT_ENVD_WEIGHT(W, H);
  double total = 0.0;
  for (size_t iy = 0; iy < H; ++iy) {
    const double s = pt_sin(pi * (((double)iy + 0.5) / (double)height));
    double run = 0.0;
    for (size_t ix = 0; ix < W; ++ix) {
      const double* t = rec + 4 * (iy * W + ix);
      double lum = (t[0] + t[1]) + t[2];
      if (!(lum > 0.0)) lum = 0.0;
      const double w = lum * s;
      run = run + w;
      cond[iy * W + ix] = run;
      wt[iy * W + ix] = w;
      if (w > 0.0) lastx[iy] = (double)ix;
    }
    if (run > 0.0) out->last_row = (int32_t)iy;
    total = total + run;
    m[iy] = total;
  }
  out->total = total;
  out->table[PT_ENVD_TOTAL] = total;
  out->table[PT_ENVD_LAST_ROW] = (double)out->last_row;
  if (!std::isfinite(total) || !(total > 0.0))
    return reject(msg, "environment sampling needs a total weight (sum of luminance x sin theta) that is finite and greater than 0 (got %g)", total);
  return 0;
}

/* ---- camera tile lists (scene_host.h) ---- */
bool scene_tile_lists_possible(const PtHostArrays& h) {
  return h.dev.mode == PT_MODE_SIMD && !h.dev.has_triangles && h.dev.n_floor == 0 && !h.nodes.empty() && h.dev.n_slots > 0 &&
         h.dev.n_slots <= 0x10000 && h.sph.size() >= (size_t)h.dev.n_slots * 4;
}

/* What tests/test_tile_lists.py breaks on purpose, in the build of tests/c/tile_lists_driver.cpp alone (host/Makefile defines
 * PT_TILE_TEST_MUTANTS for it): 1 = no inflation, 2 = lists in slot order.  The library's build has neither the word nor the tests. */
#ifdef PT_TILE_TEST_MUTANTS
int pt_tile_test_mutant = 0;
#define PT_TILE_MUTANT(bit) ((pt_tile_test_mutant & (bit)) != 0)
#else
#define PT_TILE_MUTANT(bit) false
#endif

namespace {
/* one side of the image's tile grid: per tile column (or row) the bounds [lo, hi] of the un-normalised direction component
 * ll + v c over the tile's pixels (pt_primary_dir), and the real slots whose inflated sphere is not wholly outside both planes */
struct TileAxis {
  std::vector<double> lo, hi;
  std::vector<std::vector<uint16_t>> pass; /* ascending slot numbers */
};
TileAxis tile_axis(const PtHostArrays& h, int n_tiles, int extent, double ll, double v, bool flip, int comp) {
  TileAxis ax;
  ax.lo.resize((size_t)n_tiles);
  ax.hi.resize((size_t)n_tiles);
  ax.pass.resize((size_t)n_tiles);
  const double scale = 1.0 / (double)extent;
  for (int t = 0; t < n_tiles; ++t) {
    const double p0 = (double)(8 * t) * scale, p1 = (double)std::min(8 * t + 8, extent) * scale;
    const double a = ll + (v * (flip ? 1.0 - p0 : p0)), b = ll + (v * (flip ? 1.0 - p1 : p1));
    const double lo = std::fmin(a, b), hi = std::fmax(a, b);
    ax.lo[(size_t)t] = (a != a || b != b) ? pt_nan() : lo;
    ax.hi[(size_t)t] = (a != a || b != b) ? pt_nan() : hi;
    const double nlo = std::sqrt(1.0 + (lo * lo)), nhi = std::sqrt(1.0 + (hi * hi));
    for (int sl = 0; sl < h.dev.n_slots; ++sl) {
      if (h.slot_prim[(size_t)sl] < 0) continue; /* NaN padding */
      const double* s = &h.sph[(size_t)sl * 4];
      const double r = std::fabs(s[3]);
      const double len = std::sqrt(((s[0] * s[0]) + (s[1] * s[1])) + (s[2] * s[2]));
      const double e = PT_TILE_MUTANT(1) ? r : r + (PT_TILE_INFLATE * (len + r));
      const double dl = s[comp] + (lo * s[2]), dh = s[comp] + (hi * s[2]);
      if (dl < -(e * nlo) || dh > e * nhi) continue;
      ax.pass[(size_t)t].push_back((uint16_t)sl);
    }
  }
  return ax;
}
}  // namespace

PtTileGrid scene_tile_lists(const PtHostArrays& h, int width, int height) {
  PtTileGrid g;
  if (!scene_tile_lists_possible(h) || width < 1 || height < 1) return g;
  g.width = width;
  g.height = height;
  g.tiles_x = (width + 7) / 8;
  g.tiles_y = (height + 7) / 8;
  const int n_slots = h.dev.n_slots;
  const std::vector<PtNode>& nd = h.nodes;
  /* rank[o][slot]: the position of the slot in the order in which octant o's near-first descent (shape_tree.ml:201,209) meets the leaves */
  std::vector<uint32_t> rank[4]; /* camera rays have d.z < 0: octants 0 .. 3 */
  for (uint32_t o = 0; o < 4; ++o) {
    rank[o].assign((size_t)n_slots, 0u);
    uint32_t next = 0;
    std::vector<uint32_t> todo{0u};
    while (!todo.empty()) {
      const uint32_t k = todo.back();
      todo.pop_back();
      if (is_leaf(nd[k])) {
        for (uint32_t j = 0; j < (nd[k].b & 0x3fffffffu) && nd[k].a + j < (uint32_t)n_slots; ++j) rank[o][nd[k].a + j] = next++;
        continue;
      }
      const uint32_t axis = nd[k].b >> 30, lhs = nd[k].a, rhs = nd[k].b & 0x3fffffffu;
      const bool lhs_first = (o >> axis) & 1u;
      todo.push_back(lhs_first ? rhs : lhs);
      todo.push_back(lhs_first ? lhs : rhs);
    }
  }
  /* a sphere the scan's guards are not sized for sends its tiles to the walk: non-finite, or |c| > PT_TILE_MAX_CR r */
  std::vector<uint8_t> odd((size_t)n_slots, 0);
  for (int sl = 0; sl < n_slots; ++sl) {
    if (h.slot_prim[(size_t)sl] < 0) continue;
    const double* s = &h.sph[(size_t)sl * 4];
    const double len = std::sqrt(((s[0] * s[0]) + (s[1] * s[1])) + (s[2] * s[2]));
    odd[(size_t)sl] = !(std::isfinite(len) && std::isfinite(s[3]) && len <= PT_TILE_MAX_CR * std::fabs(s[3]));
  }
  const TileAxis cols = tile_axis(h, g.tiles_x, width, h.dev.cam_llx, h.dev.cam_vx, false, 0);
  const TileAxis rows = tile_axis(h, g.tiles_y, height, h.dev.cam_lly, h.dev.cam_vy, true, 1);
  g.rec.assign((size_t)g.tiles_x * g.tiles_y, PtTileRec{});
  std::vector<uint8_t> in_row((size_t)n_slots);
  std::vector<uint16_t> list;
  for (int ty = 0; ty < g.tiles_y; ++ty) {
    std::fill(in_row.begin(), in_row.end(), (uint8_t)0);
    for (uint16_t sl : rows.pass[(size_t)ty]) in_row[sl] = 1;
    const double ylo = rows.lo[(size_t)ty], yhi = rows.hi[(size_t)ty];
    for (int tx = 0; tx < g.tiles_x; ++tx) {
      PtTileRec& r = g.rec[(size_t)ty * g.tiles_x + tx];
      const double xlo = cols.lo[(size_t)tx], xhi = cols.hi[(size_t)tx];
      /* one octant for the whole tile: no component's bounds are non-finite, straddle zero or touch it */
      bool walk = !(std::isfinite(xlo) && std::isfinite(xhi) && std::isfinite(ylo) && std::isfinite(yhi)) || (xlo <= 0.0 && xhi >= 0.0) ||
                  (ylo <= 0.0 && yhi >= 0.0);
      const uint32_t o = (xlo > 0.0 ? 1u : 0u) | (ylo > 0.0 ? 2u : 0u);
      list.clear();
      for (uint16_t sl : cols.pass[(size_t)tx])
        if (in_row[sl]) {
          list.push_back(sl);
          walk = walk || odd[sl];
        }
      if (walk || list.size() > (size_t)PT_TILE_MAX_SLOTS) {
        r.count = PT_TILE_WALK;
        g.n_walk++;
        continue;
      }
      if (!PT_TILE_MUTANT(2))
        std::sort(list.begin(), list.end(), [&](uint16_t a, uint16_t b) { return rank[o][a] < rank[o][b]; });
      r.count = (uint8_t)list.size();
      r.octant = (uint8_t)o;
      for (size_t k = 0; k < list.size(); ++k) r.slot[k] = list[k];
      g.longest = std::max(g.longest, (int)list.size());
    }
  }
  return g;
}

/* ---- display outputs (include/ptx.h): checks, the sRGB thresholds, the rule of pt_display.h over an image ---- */
int display_pixel_bytes(int32_t format) {
  switch (format) {
    case PTX_PIXEL_RGB8: return 3;
    case PTX_PIXEL_RGBA8: return 4;
    case PTX_PIXEL_RGB32F: return 12;
    case PTX_PIXEL_RGBA32F: return 16;
    default: return 0;
  }
}

int display_check(const ptx_display_params* d, std::string* msg) {
  if (display_pixel_bytes(d->format) == 0)
    return reject(msg, "display: unknown format %d (PTX_PIXEL_RGB8 0, RGBA8 1, RGB32F 2, RGBA32F 3)", d->format);
  if (d->transfer < PTX_TRANSFER_REFERENCE || d->transfer > PTX_TRANSFER_SRGB)
    return reject(msg, "display: unknown transfer %d (PTX_TRANSFER_REFERENCE 0, LINEAR 1, SRGB 2)", d->transfer);
  if (d->tone < PTX_TONE_NONE || d->tone > PTX_TONE_ACES)
    return reject(msg, "display: unknown tone %d (PTX_TONE_NONE 0, REINHARD 1, ACES 2)", d->tone);
  if (d->flags != 0) return reject(msg, "display: flags must be 0 (got %d)", d->flags);
  for (int i = 0; i < 4; ++i)
    if (d->reserved[i] != 0) return reject(msg, "display: reserved[%d] must be 0 (got %d)", i, d->reserved[i]);
  if (!std::isfinite(d->exposure) || d->exposure < 0.0) return reject(msg, "display: exposure must be finite and >= 0 (got %g)", d->exposure);
  if (d->transfer == PTX_TRANSFER_REFERENCE && (d->tone != PTX_TONE_NONE || d->exposure != 1.0))
    return reject(msg, "display: PTX_TRANSFER_REFERENCE needs tone PTX_TONE_NONE and exposure 1.0 (got tone %d, exposure %g): the reference's "
                       "conversion has neither; use PTX_TRANSFER_LINEAR or PTX_TRANSFER_SRGB", d->tone, d->exposure);
  if (d->transfer == PTX_TRANSFER_SRGB && (d->format == PTX_PIXEL_RGB32F || d->format == PTX_PIXEL_RGBA32F))
    return reject(msg, "display: the binary32 formats carry linear or reference values, not PTX_TRANSFER_SRGB (format %d)", d->format);
  return 0;
}

const double* display_thresholds() {
  struct Table {
    double t[PT_DISPLAY_THRESHOLDS];
    Table() {
      for (int k = 1; k <= PT_DISPLAY_THRESHOLDS; ++k) {
        const double e = ((double)k - 0.5) / 255.0;
        t[k - 1] = e <= 0.04045 ? e / 12.92 : std::pow((e + 0.055) / 1.055, 2.4);
      }
    }
  };
  static const Table table; /* initialised once, by whichever thread asks first */
  return table.t;
}

namespace {
template <class T, int C>
void display_apply_as(const ptx_display_params& d, int64_t n_pixels, const double* rgb, T* out, const double* th) {
  for (int64_t p = 0; p < n_pixels; ++p) {
    for (int c = 0; c < 3; ++c) {
      const double v = rgb[3 * p + c];
      if constexpr (sizeof(T) == 1) out[C * p + c] = pt_display_code(v, d.transfer, d.tone, d.exposure, th);
      else out[C * p + c] = pt_display_f32(v, d.transfer, d.tone, d.exposure);
    }
    if constexpr (C == 4) out[4 * p + 3] = sizeof(T) == 1 ? (T)255 : (T)1;
  }
}
}  // namespace

void display_apply_host(const ptx_display_params& d, int64_t n_pixels, const double* rgb, void* out) {
  const double* th = display_thresholds();
  switch (d.format) {
    case PTX_PIXEL_RGB8: display_apply_as<uint8_t, 3>(d, n_pixels, rgb, (uint8_t*)out, th); break;
    case PTX_PIXEL_RGBA8: display_apply_as<uint8_t, 4>(d, n_pixels, rgb, (uint8_t*)out, th); break;
    case PTX_PIXEL_RGB32F: display_apply_as<float, 3>(d, n_pixels, rgb, (float*)out, th); break;
    default: display_apply_as<float, 4>(d, n_pixels, rgb, (float*)out, th); break;
  }
}
