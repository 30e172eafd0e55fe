// Sanitizer driver for the HOST code of the product (CPU build only: -fsanitize=address,undefined): the PLY reader
// (host/ply.cpp mirrors a parser of untrusted binary input, ply_format/src/ply.ml:208-235,288-352), the scene builders
// (host/scenes.cpp), the PNG writer, the host BVH builder (csrc/bvh_build.cpp) and scene construction (csrc/scene_host.cpp: the
// descriptor check and everything between a tree and the arrays the kernels walk).  Built by `make asan` in
// path_tracer_ocaml_amd/host, run by tests/test_sanitizers.py and tests/test_scene_host.py.  Every mode exits 0 unless a
// sanitizer fires (they abort) or a check of its own fails.
//   ply <file>                  load, read every column / row the ganesha scene needs, build the ganesha scene from it, assemble it
//   scene <name>                build a scene, check it, Shape_tree.create on the host, assemble; print the tree size
//   arrays <name> [key=value]   the assembled scene as one JSON line: element count and FNV-1a digest of every vector of
//                               PtHostArrays, the scalars of its dev, the light table.  Keys: tri_frame, oct_image, top_nodes,
//                               bin_key (SceneOptions), dump=<dir> (the tree, threading and image vectors as raw files)
//   layout <name|ints> [key=value]  what csrc/pt_lds_layout.h says of a scene (or of explicit integers), as one JSON line: where it
//                               is walked from, and for k_trace, k_bounce and k_bounce_carry every region's offset in the dynamic LDS
//                               buffer and the total.  Keys: mode, n_nodes, total_slots, has_triangles, has_emit, lds_nodes64,
//                               tree_depth, n_top (a scene's own unless given), trace_waves, waves (workgroup sizes of k_trace / the
//                               k_bounce family), hbm (the k_bounce family walks from HBM / L2)
//   hostile                     broken descriptors: each must come back rejected, with its message
//   png <out.png>               write a small image
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../path_tracer_ocaml_amd/csrc/pt_lds_layout.h"
#include "../../path_tracer_ocaml_amd/csrc/scene_host.h"
#include "../../path_tracer_ocaml_amd/host/host.h"

static pth_scene* make_scene(const std::string& name) {
  if (name == "shirley") return pth_scene_shirley(96, 48, 0, 42);
  if (name == "shirley_array") return pth_scene_shirley(96, 48, 1, 42);
  if (name == "cornell") return pth_scene_cornell(64, 64, 12.0);
  if (name == "cornell_lamp") return pth_scene_cornell_lamp(64, 64, 0.0, 0.03, 0.999, 400.0); /* spheres + triangles, Array leaves */
  if (name == "ganesha_150k") return pth_scene_ganesha_like(64, 36, 150000, 7);                 /* the benchmark's mesh */
  return pth_scene_ganesha_like(64, 36, 3000, 7);
}

struct Assembled {
  PtHostArrays h;
  int n_prims = 0, depth = 0, leaves = 0;
};

/* what ptx_scene_create does with a descriptor, with the host builder */
static int assemble(const ptx_scene_desc* d, const SceneOptions& opt, Assembled* out, std::string* msg) {
  if (const int rc = scene_check_desc(d, msg)) return rc;
  const std::vector<Box> boxes = scene_boxes(d);
  BvhResult t = bvh_build(boxes, scene_num_bins(d), d->length_cutoff, d->leaf_kind == PTX_LEAF_SIMD);
  out->n_prims = (int)boxes.size();
  out->depth = t.depth;
  out->leaves = t.leaves;
  if (const int rc = scene_set_tree(d, std::move(t), &out->h, msg)) return rc;
  scene_assemble(d, boxes, opt, &out->h);
  return 0;
}

static int print_tree(const ptx_scene_desc* d) {
  Assembled a;
  std::string msg;
  if (assemble(d, SceneOptions{}, &a, &msg)) {
    std::printf("rejected: %s\n", msg.c_str());
    return 1;
  }
  std::printf("prims %d nodes %zu slots %d depth %d leaves %d\n", a.n_prims, a.h.nodes.size(), a.h.dev.n_slots, a.depth, a.leaves);
  return 0;
}

/* ---- arrays ---- */
static uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  return h;
}
template <class T>
static void put_vec(FILE* f, const char* name, const std::vector<T>& v, const char* sep = ",") {
  std::fprintf(f, "\"%s\":[%zu,\"%016llx\"]%s", name, v.size(), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)), sep);
}
static void put_int(FILE* f, const char* name, long long v, const char* sep = ",") { std::fprintf(f, "\"%s\":%lld%s", name, v, sep); }
/* floating-point scalars as their bits */
static void put_f64(FILE* f, const char* name, const double* v, int n, const char* sep = ",") {
  std::fprintf(f, "\"%s\":[", name);
  for (int i = 0; i < n; ++i) {
    uint64_t u;
    std::memcpy(&u, &v[i], 8);
    std::fprintf(f, "\"%016llx\"%s", (unsigned long long)u, i + 1 < n ? "," : "");
  }
  std::fprintf(f, "]%s", sep);
}
static void put_f32(FILE* f, const char* name, const float* v, int n, const char* sep = ",") {
  std::fprintf(f, "\"%s\":[", name);
  for (int i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &v[i], 4);
    std::fprintf(f, "\"%08x\"%s", u, i + 1 < n ? "," : "");
  }
  std::fprintf(f, "]%s", sep);
}
static void put_arrays(FILE* f, const PtHostArrays& h, int n_prims, int tree_depth, int tree_leaves, int n_emissive_tris,
                       const std::vector<double>& emissive_tris, const std::vector<double>& light_table) {
  std::fprintf(f, "{");
  put_int(f, "n_prims", n_prims); put_int(f, "tree_depth", tree_depth); put_int(f, "tree_leaves", tree_leaves);
  put_int(f, "n_emissive_tris", n_emissive_tris);
  std::fprintf(f, "\"vectors\":{");
  put_vec(f, "nodes", h.nodes); put_vec(f, "sph", h.sph); put_vec(f, "tri", h.tri); put_vec(f, "tri_uv", h.tri_uv);
  put_vec(f, "tri_frame", h.tri_frame); put_vec(f, "kind", h.kind); put_vec(f, "cat", h.cat); put_vec(f, "slot_mat", h.slot_mat);
  put_vec(f, "slot_prim", h.slot_prim); put_vec(f, "mats", h.mats); put_vec(f, "texs", h.texs); put_vec(f, "shade", h.shade);
  put_vec(f, "skip", h.skip); put_vec(f, "skip32", h.skip32); put_vec(f, "nodes32", h.nodes32); put_vec(f, "nodes32o", h.nodes32o);
  put_vec(f, "top_nodes", h.top_nodes); put_vec(f, "skip32_top", h.skip32_top); put_vec(f, "emissive_tris", emissive_tris, "},");
  const PtSceneDev& dv = h.dev;
  std::fprintf(f, "\"dev\":{");
  put_int(f, "n_nodes", dv.n_nodes); put_int(f, "depth", dv.depth); put_int(f, "mode", dv.mode); put_int(f, "n_slots", dv.n_slots);
  put_int(f, "n_floor", dv.n_floor); put_int(f, "has_triangles", dv.has_triangles); put_int(f, "has_emit", dv.has_emit);
  put_int(f, "has_checker", dv.has_checker); put_int(f, "lds_nodes64", dv.lds_nodes64); put_int(f, "n_top", dv.n_top);
  put_int(f, "all_triangles", dv.all_triangles); put_f64(f, "sort_axis", dv.sort_axis, 3);
  put_int(f, "sort_by_elevation", dv.sort_by_elevation); put_int(f, "sort_by_root", dv.sort_by_root);
  put_f32(f, "root_mn", dv.root_mn, 3); put_f32(f, "root_mx", dv.root_mx, 3); put_f32(f, "root_mag", &dv.root_mag, 1);
  put_f32(f, "pad_f", &dv.pad_f, 1);
  const double cam[4] = {dv.cam_llx, dv.cam_lly, dv.cam_vx, dv.cam_vy};
  put_f64(f, "cam", cam, 4); put_int(f, "bg_kind", dv.bg_kind); put_int(f, "pad0", dv.pad0);
  put_f64(f, "bg_horizon", dv.bg_horizon, 3); put_f64(f, "bg_zenith", dv.bg_zenith, 3);
  put_int(f, "n_lights", dv.n_lights); put_int(f, "lighting", dv.lighting); put_f64(f, "light_area", &dv.light_area, 1, "},");
  put_vec(f, "light_table", light_table, "}\n");
}

template <class T>
static bool dump_vec(const std::string& dir, const char* name, const std::vector<T>& v) {
  FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
  if (!f) return false;
  const size_t put = v.empty() ? 0 : std::fwrite(v.data(), sizeof(T), v.size(), f);
  return std::fclose(f) == 0 && put == v.size();
}

static int arrays_mode(int argc, char** argv) {
  SceneOptions opt;
  std::string dump;
  for (int i = 3; i < argc; ++i) {
    const std::string kv = argv[i];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return 2;
    const std::string key = kv.substr(0, eq), val = kv.substr(eq + 1);
    if (key == "tri_frame") opt.tri_frame = std::atoi(val.c_str());
    else if (key == "oct_image") opt.oct_image = std::atoi(val.c_str());
    else if (key == "top_nodes") opt.top_nodes = std::atoi(val.c_str());
    else if (key == "bin_key") opt.bin_key = std::atoi(val.c_str());
    else if (key == "dump") dump = val;
    else return 2;
  }
  pth_scene* s = make_scene(argv[2]);
  if (!s) return 1;
  Assembled a;
  std::string msg;
  const int rc = assemble(pth_scene_desc(s), opt, &a, &msg);
  pth_scene_free(s);
  if (rc) {
    std::printf("rejected: %s\n", msg.c_str());
    return 1;
  }
  const PtHostArrays& h = a.h;
  std::vector<double> lights;
  if (h.n_emissive_tris > 0 && h.n_emissive_tris <= PTX_MAX_LIGHT_TRIANGLES) lights = light_table_build(h);
  put_arrays(stdout, h, a.n_prims, a.depth, a.leaves, h.n_emissive_tris, h.emissive_tris, lights);
  if (!dump.empty()) {
    const bool ok = dump_vec(dump, "nodes", h.nodes) && dump_vec(dump, "skip", h.skip) && dump_vec(dump, "skip32", h.skip32) &&
                    dump_vec(dump, "nodes32", h.nodes32) && dump_vec(dump, "nodes32o", h.nodes32o) &&
                    dump_vec(dump, "top_nodes", h.top_nodes) && dump_vec(dump, "skip32_top", h.skip32_top);
    if (!ok) return 1;
  }
  return 0;
}

/* ---- layout ---- */
static void put_image(FILE* f, const PtLdsLayout& l) {
  put_int(f, "stacks", (long long)l.stacks); put_int(f, "nodes", (long long)l.image.nodes); put_int(f, "sph", (long long)l.image.sph);
  put_int(f, "tri", (long long)l.image.tri); put_int(f, "kind", (long long)l.image.kind); put_int(f, "cat", (long long)l.image.cat);
  put_int(f, "nodes64", (long long)l.image.nodes64); put_int(f, "image_end", (long long)l.image.end);
}
static int layout_mode(int argc, char** argv) {
  PtLdsIn in{};
  int tree_depth = 0, trace_waves = -1, waves = 16, hbm = 0;
  if (std::string(argv[2]) != "ints") {
    pth_scene* s = make_scene(argv[2]);
    if (!s) return 1;
    Assembled a;
    std::string msg;
    const int rc = assemble(pth_scene_desc(s), SceneOptions{}, &a, &msg);
    pth_scene_free(s);
    if (rc) return 1;
    const PtSceneDev& dv = a.h.dev;
    in.mode = dv.mode; in.n_nodes = dv.n_nodes; in.total_slots = dv.n_slots + dv.n_floor; in.has_triangles = dv.has_triangles;
    in.has_emit = dv.has_emit; in.n_top = (int)(a.h.top_nodes.size() / 16);
    tree_depth = a.depth;
  }
  for (int i = 3; i < argc; ++i) {
    const std::string kv = argv[i];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return 2;
    const std::string key = kv.substr(0, eq);
    const int val = std::atoi(kv.substr(eq + 1).c_str());
    if (key == "mode") in.mode = val;
    else if (key == "n_nodes") in.n_nodes = val;
    else if (key == "total_slots") in.total_slots = val;
    else if (key == "has_triangles") in.has_triangles = val;
    else if (key == "has_emit") in.has_emit = val;
    else if (key == "lds_nodes64") in.lds_nodes64 = val;
    else if (key == "tree_depth") tree_depth = val;
    else if (key == "n_top") in.n_top = val;
    else if (key == "trace_waves") trace_waves = val;
    else if (key == "waves") waves = val;
    else if (key == "hbm") hbm = val;
    else return 2;
  }
  if (trace_waves < 0) trace_waves = in.mode == PT_MODE_SIMD ? 16 : 8; /* the library's defaults: 1024 / 512 threads */
  in.stack_depth = tree_depth + 1 > 1 ? tree_depth + 1 : 1;
  in.kernel = PT_LDS_K_TRACE;
  in.waves = trace_waves;
  const int placement = pt_lds_placement(in);
  FILE* f = stdout;
  std::fprintf(f, "{\"in\":{");
  put_int(f, "mode", in.mode); put_int(f, "n_nodes", in.n_nodes); put_int(f, "total_slots", in.total_slots);
  put_int(f, "has_triangles", in.has_triangles); put_int(f, "has_emit", in.has_emit); put_int(f, "lds_nodes64", in.lds_nodes64);
  put_int(f, "tree_depth", tree_depth); put_int(f, "n_top", in.n_top); put_int(f, "trace_waves", trace_waves); put_int(f, "waves", waves);
  put_int(f, "hbm", hbm, "},");
  put_int(f, "placement", placement); put_int(f, "static_max", (long long)PT_LDS_STATIC_MAX);
  put_int(f, "lds_nodes64_kept", pt_lds_keep_nodes64(in, waves)); put_int(f, "bounce_limit", (long long)PT_LDS_BOUNCE_LIMIT); put_int(f, "shade_pool", (long long)pt_lds_shade_pool_bytes(waves));
  in.from_hbm = placement != PT_PLACE_LDS;
  const int n_top = in.n_top;
  if (!in.from_hbm) in.n_top = 0;
  PtLdsLayout l = pt_lds_layout(in);
  std::fprintf(f, "\"k_trace\":{");
  put_image(f, l); put_int(f, "top", (long long)l.top); put_int(f, "total", (long long)l.total, "},");
  in.n_top = n_top;
  in.waves = waves;
  in.from_hbm = hbm;
  in.kernel = PT_LDS_K_BOUNCE;
  l = pt_lds_layout(in);
  std::fprintf(f, "\"k_bounce\":{");
  put_image(f, l); put_int(f, "pool_off", (long long)l.pool_off); put_int(f, "pool_i", (long long)l.work.pool_i);
  put_int(f, "pool_s", (long long)l.work.pool_s); put_int(f, "park0", (long long)l.work.park0); put_int(f, "park_uv", (long long)l.work.park_uv);
  put_int(f, "park_w", (long long)l.work.park_w); put_int(f, "total", (long long)l.total); put_int(f, "fits", l.fits, "},");
  in.kernel = PT_LDS_K_BOUNCE_CARRY;
  in.from_hbm = 0; /* (k_bounce_carry is for LDS-resident scenes only) */
  l = pt_lds_layout(in);
  std::fprintf(f, "\"k_bounce_carry\":{");
  put_image(f, l); put_int(f, "pool_off", (long long)l.pool_off); put_int(f, "park0", (long long)l.work.park0);
  put_int(f, "park_emit", (long long)l.work.park_emit); put_int(f, "park_uv", (long long)l.work.park_uv);
  put_int(f, "total", (long long)l.total); put_int(f, "fits", l.fits, "}}\n");
  return 0;
}

/* ---- hostile ---- */
static int g_accepted = 0;
static void expect_rejected(const char* what, const ptx_scene_desc& d) {
  Assembled a;
  std::string msg;
  if (assemble(&d, SceneOptions{}, &a, &msg) == 0) {
    std::printf("ACCEPTED %s\n", what);
    ++g_accepted;
  } else {
    std::printf("rejected %s: %s\n", what, msg.c_str());
  }
}

static int hostile_mode() {
  pth_scene* cornell = make_scene("cornell"); /* triangles + spheres, Array leaves */
  pth_scene* ganesha = make_scene("ganesha"); /* a mesh on floor triangles */
  pth_scene* shirley = make_scene("shirley"); /* Simd leaves */
  if (!cornell || !ganesha || !shirley) return 1;
  const ptx_scene_desc c = *pth_scene_desc(cornell), g = *pth_scene_desc(ganesha), sh = *pth_scene_desc(shirley);
  for (const ptx_scene_desc* ok : {&c, &g, &sh}) { /* the cases below start from descriptors that pass */
    Assembled a;
    std::string msg;
    if (assemble(ok, SceneOptions{}, &a, &msg)) return 1;
  }
  ptx_scene_desc d;
#define CASE(base, name, mutation) \
  d = base;                        \
  mutation;                        \
  expect_rejected(name, d)
  CASE(c, "n_triangles -1", d.n_triangles = -1);
  CASE(c, "n_spheres -1", d.n_spheres = -1);
  CASE(c, "n_floor_triangles -1", d.n_floor_triangles = -1);
  CASE(c, "no primitives", (d.n_triangles = 0, d.n_spheres = 0));
  CASE(c, "materials NULL", d.materials = nullptr);
  CASE(c, "n_materials 0", d.n_materials = 0);
  CASE(c, "textures NULL", d.textures = nullptr);
  CASE(c, "sphere_x NULL", d.sphere_x = nullptr);
  CASE(c, "sphere_y NULL", d.sphere_y = nullptr);
  CASE(c, "sphere_z NULL", d.sphere_z = nullptr);
  CASE(c, "sphere_r NULL", d.sphere_r = nullptr);
  CASE(c, "sphere_material NULL", d.sphere_material = nullptr);
  CASE(c, "vertex_x NULL", d.vertex_x = nullptr);
  CASE(c, "vertex_y NULL", d.vertex_y = nullptr);
  CASE(c, "vertex_z NULL", d.vertex_z = nullptr);
  CASE(c, "tri_indices NULL", d.tri_indices = nullptr);
  CASE(c, "tri_uv NULL", d.tri_uv = nullptr);
  CASE(c, "tri_material NULL", d.tri_material = nullptr);
  CASE(g, "floor_vertices NULL", d.floor_vertices = nullptr);
  CASE(g, "floor_uv NULL", d.floor_uv = nullptr);
  CASE(g, "floor_material NULL", d.floor_material = nullptr);
  /* indices: a copy of the array with one entry changed */
  std::vector<int32_t> idx;
  auto with = [&idx](const int32_t* src, int n, int at, int32_t v) {
    idx.assign(src, src + n);
    idx[(size_t)at] = v;
    return idx.data();
  };
  CASE(c, "vertex index n_vertices", d.tri_indices = with(c.tri_indices, 3 * c.n_triangles, 3 * c.n_triangles - 1, c.n_vertices));
  CASE(c, "vertex index -1", d.tri_indices = with(c.tri_indices, 3 * c.n_triangles, 4, -1));
  CASE(c, "triangle material n_materials", d.tri_material = with(c.tri_material, c.n_triangles, c.n_triangles - 1, c.n_materials));
  CASE(c, "triangle material -1", d.tri_material = with(c.tri_material, c.n_triangles, 0, -1));
  CASE(c, "sphere material n_materials", d.sphere_material = with(c.sphere_material, c.n_spheres, c.n_spheres - 1, c.n_materials));
  CASE(c, "sphere material -1", d.sphere_material = with(c.sphere_material, c.n_spheres, 0, -1));
  CASE(g, "floor material n_materials", d.floor_material = with(g.floor_material, g.n_floor_triangles, g.n_floor_triangles - 1, g.n_materials));
  CASE(g, "floor material -1", d.floor_material = with(g.floor_material, g.n_floor_triangles, 0, -1));
  std::vector<ptx_material> mats;
  auto with_mat = [&mats, &c]() {
    mats.assign(c.materials, c.materials + c.n_materials);
    return &mats[0]; /* cornell's material 0: Metal with a texture */
  };
  CASE(c, "texture index n_textures", (with_mat()->texture = c.n_textures, d.materials = mats.data()));
  CASE(c, "texture index -1", (with_mat()->texture = -1, d.materials = mats.data()));
  CASE(c, "material kind 3", (with_mat()->kind = 3, d.materials = mats.data()));
  CASE(c, "material kind -1", (with_mat()->kind = -1, d.materials = mats.data()));
  std::vector<ptx_texture> texs(c.textures, c.textures + c.n_textures);
  texs.back().kind = 7;
  CASE(c, "texture kind 7", d.textures = texs.data());
  CASE(c, "leaf_kind 5", d.leaf_kind = 5);
  CASE(c, "Simd leaves over triangles", d.leaf_kind = PTX_LEAF_SIMD);
  CASE(sh, "Simd length_cutoff 0", d.length_cutoff = 0);
  CASE(sh, "Simd length_cutoff 17", d.length_cutoff = 17);
  CASE(c, "num_bins 3", d.num_bins = 3);
#undef CASE
  pth_scene_free(cornell);
  pth_scene_free(ganesha);
  pth_scene_free(shirley);
  return g_accepted == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "hostile") return hostile_mode();
  if (argc < 3) return 2;
  if (mode == "ply") {
    pth_ply* p = pth_ply_load(argv[2]);
    if (!p) {
      std::printf("rejected: %s\n", pth_last_error());
    } else {
      double acc = 0.0;
      const int64_t nv = pth_ply_count(p, "vertex");
      for (const char* name : {"x", "y", "z", "nx", "confidence"}) {
        const double* f = pth_ply_floats(p, "vertex", name);
        const int64_t* q = pth_ply_ints(p, "vertex", name);
        for (int64_t i = 0; i < nv && (f || q); ++i) acc += f ? f[i] : (double)q[i];
      }
      const int32_t* lens = nullptr;
      const int64_t* rows = pth_ply_rows(p, "vertex_indices", &lens);
      const int64_t nr = pth_ply_count(p, "vertex_indices");
      int64_t off = 0;
      for (int64_t r = 0; rows && r < nr; ++r)
        for (int32_t k = 0; k < lens[r]; ++k) acc += (double)rows[off++];
      std::printf("loaded: vertex %lld rows %lld checksum %.17g\n", (long long)nv, (long long)nr, acc);
      pth_ply_free(p);
    }
    pth_scene* s = pth_scene_ganesha_ply(argv[2], 64, 36); /* Mesh.create + floor + camera */
    if (!s) {
      std::printf("no scene: %s\n", pth_last_error());
    } else {
      print_tree(pth_scene_desc(s));
      pth_scene_free(s);
    }
    return 0;
  }
  if (mode == "scene") {
    const std::string name = argv[2];
    pth_scene* s = make_scene(name);
    if (!s) return 1;
    const int rc = print_tree(pth_scene_desc(s));
    ptx_light lights[2];
    if (name == "cornell") pth_lights_cornell(64, 64, lights);
    if (name == "ganesha") pth_lights_ganesha(s, lights);
    pth_scene_free(s);
    return rc;
  }
  if (mode == "arrays") return arrays_mode(argc, argv);
  if (mode == "layout") return layout_mode(argc, argv);
  if (mode == "png") {
    const int w = 37, h = 11;
    std::vector<double> img((size_t)w * h * 3);
    for (size_t i = 0; i < img.size(); ++i) img[i] = (double)(i % 97) / 64.0 - 0.1; /* values below 0 and above 1 too */
    img[5] = NAN;
    std::vector<double> g(img.size());
    pth_ppm_gamma(img.data(), (int64_t)img.size(), 3, g.data());
    return pth_write_png(argv[2], w, h, img.data()) == 0 ? 0 : 1;
  }
  return 2;
}
