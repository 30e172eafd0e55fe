// Driver for the per-octant LDS node image (csrc/scene_host.cpp: PtHostArrays::lds_oct; csrc/pt_lds_layout.h: pt_lds_oct_layout), CPU
// build only, under -fsanitize=address,undefined like tests/c/asan_host_driver.cpp.  Built by `make asan` in
// path_tracer_ocaml_amd/host, run by tests/test_lds_oct_image.py.
//   image <shirley | soup<N>> <dir> [lds_oct=0]   assemble the scene (soup<N>: N spheres of a fixed pseudo-random soup, Simd leaves) and
//                               write nodes.bin, nodes32.bin and lds_oct.bin into <dir>; prints "nodes <n> slots <n> depth <d> words <n>"
//   layout key=value ...        pt_lds_oct_layout of explicit integers as one JSON line.  Keys: mode, n_nodes, total_slots, has_emit,
//                               lds_nodes64, waves
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../path_tracer_ocaml_amd/csrc/pt_lds_layout.h"
#include "../../path_tracer_ocaml_amd/csrc/scene_host.h"
#include "../../path_tracer_ocaml_amd/host/host.h"

template <class T>
static bool dump_vec(const std::string& dir, const char* name, const std::vector<T>& v) {
  FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
  if (!f) return false;
  const size_t put = v.empty() ? 0 : std::fwrite(v.data(), sizeof(T), v.size(), f);
  return std::fclose(f) == 0 && put == v.size();
}

static int assemble(const ptx_scene_desc* d, const SceneOptions& opt, PtHostArrays* h, int* depth) {
  std::string msg;
  if (scene_check_desc(d, &msg)) return 1;
  const std::vector<Box> boxes = scene_boxes(d);
  BvhResult t = bvh_build(boxes, scene_num_bins(d), d->length_cutoff, d->leaf_kind == PTX_LEAF_SIMD);
  *depth = t.depth;
  if (scene_set_tree(d, std::move(t), h, &msg)) return 1;
  scene_assemble(d, boxes, opt, h);
  return 0;
}

static int image_mode(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string name = argv[2], dir = argv[3];
  SceneOptions opt;
  for (int i = 4; i < argc; ++i)
    if (std::string(argv[i]) == "lds_oct=0") opt.lds_oct = 0;
    else return 2;
  PtHostArrays h;
  int depth = 0, rc;
  if (name == "shirley") {
    pth_scene* s = pth_scene_shirley(1920, 1080, 0, 42); /* the benchmark's scene: the tree does not depend on the image size */
    if (!s) return 1;
    rc = assemble(pth_scene_desc(s), opt, &h, &depth);
    pth_scene_free(s);
  } else if (name.rfind("soup", 0) == 0) {
    const int n = std::atoi(name.c_str() + 4);
    if (n < 1 || n > 100000) return 2;
    std::vector<double> x((size_t)n), y((size_t)n), z((size_t)n), r((size_t)n);
    std::vector<int32_t> m((size_t)n, 0);
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto uni = [&st]() { /* splitmix64 -> [0, 1) */
      st += 0x9e3779b97f4a7c15ull;
      uint64_t v = st;
      v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
      v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
      v ^= v >> 31;
      return (double)(v >> 11) / 9007199254740992.0;
    };
    for (int i = 0; i < n; ++i) {
      x[(size_t)i] = 6.0 * uni() - 3.0;
      y[(size_t)i] = 4.0 * uni() - 2.0;
      z[(size_t)i] = -3.0 - 6.0 * uni();
      r[(size_t)i] = 0.02 + 0.4 * uni() * uni();
    }
    ptx_material mat{};
    ptx_texture tex{};
    ptx_scene_desc d{};
    d.n_spheres = n;
    d.sphere_x = x.data(); d.sphere_y = y.data(); d.sphere_z = z.data(); d.sphere_r = r.data(); d.sphere_material = m.data();
    d.n_materials = 1; d.materials = &mat; d.n_textures = 1; d.textures = &tex;
    d.leaf_kind = PTX_LEAF_SIMD;
    d.length_cutoff = 16;
    rc = assemble(&d, opt, &h, &depth);
  } else return 2;
  if (rc) return 1;
  if (!dump_vec(dir, "nodes", h.nodes) || !dump_vec(dir, "nodes32", h.nodes32) || !dump_vec(dir, "lds_oct", h.lds_oct)) return 1;
  std::printf("nodes %zu slots %d depth %d words %zu\n", h.nodes.size(), h.dev.n_slots + h.dev.n_floor, depth, h.lds_oct.size());
  return 0;
}

static int layout_mode(int argc, char** argv) {
  PtLdsIn in{};
  in.mode = PT_MODE_SIMD;
  in.waves = 16;
  in.kernel = PT_LDS_K_BOUNCE_CARRY;
  for (int i = 2; i < argc; ++i) {
    const std::string kv = argv[i];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return 2;
    const std::string key = kv.substr(0, eq);
    const int val = std::atoi(kv.substr(eq + 1).c_str());
    if (key == "mode") in.mode = val;
    else if (key == "n_nodes") in.n_nodes = val;
    else if (key == "total_slots") in.total_slots = val;
    else if (key == "has_emit") in.has_emit = val;
    else if (key == "lds_nodes64") in.lds_nodes64 = val;
    else if (key == "waves") in.waves = val;
    else return 2;
  }
  const PtLdsOctLayout l = pt_lds_oct_layout(in);
  std::printf("{\"oct\":%zu,\"leaf\":%zu,\"sph\":%zu,\"cat\":%zu,\"nodes64\":%zu,\"end\":%zu,\"pool_off\":%zu,\"park0\":%zu,\"park_emit\":%zu,"
              "\"park_end\":%zu,\"total\":%zu,\"fits\":%d,\"limit\":%zu}\n",
              l.oct, l.leaf, l.sph, l.cat, l.nodes64, l.end, l.pool_off, l.work.park0, l.work.park_emit, l.work.park_end, l.total, l.fits,
              (size_t)PT_LDS_BOUNCE_LIMIT);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "image") return image_mode(argc, argv);
  if (mode == "layout") return layout_mode(argc, argv);
  return 2;
}
