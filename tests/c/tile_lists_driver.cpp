// Driver for the camera tile lists (csrc/scene_host.cpp: scene_tile_lists) and the scan of them (csrc/pt_tile_scan.h: the function the
// kernel runs, compiled here for the host), CPU build only, under -fsanitize=address,undefined like tests/c/lds_oct_driver.cpp.  Built
// by `make asan` in path_tracer_ocaml_amd/host, run by tests/test_tile_lists.py.
//   grid <scene> <width> <height> <dir> [mutant=<bits>]
//       assemble the scene, build the grid and write nodes.bin, sph.bin, slot_prim.bin and grid.bin into <dir>; prints
//       "nodes <n> slots <n> tiles_x <n> tiles_y <n> walk <n> longest <n> build_us <n>" and "camera <llx> <lly> <vx> <vy>" (hex floats)
//   scan <scene> <width> <height> <dir> [mutant=<bits>] [guards=0]
//       reads <dir>/samples.bin, pairs of binary64 pixel coordinates (x + dx, y + dy) inside the image, makes each sample's camera ray as
//       pt_primary_dir does, scans the list of the sample's tile, and writes dirs.bin (3 binary64 per ray) and hits.bin (per ray binary64 t,
//       int32 slot, int32 status: 0 scanned, 1 a guard fired, 2 the tile walks or the ray's octant is not the record's)
//   <scene>: shirley, or file:<path> = binary64 quadruples (x, y, z, r), Simd leaves, the camera (-1, -0.5, 2, 1)
//   mutant: 1 = no inflation, 2 = lists in slot order (csrc/scene_host.cpp, compiled in only with -DPT_TILE_TEST_MUTANTS, as `make asan`
//   builds this driver); guards=0: the scan without its guards
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../path_tracer_ocaml_amd/csrc/pt_tile_scan.h"
#include "../../path_tracer_ocaml_amd/csrc/scene_host.h"
#include "../../path_tracer_ocaml_amd/host/host.h"

#ifdef PT_TILE_TEST_MUTANTS
extern int pt_tile_test_mutant;
#endif

template <class T>
static bool dump(const std::string& dir, const char* name, const T* p, size_t n) {
  FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
  if (!f) return false;
  const size_t put = n ? std::fwrite(p, sizeof(T), n, f) : 0;
  return std::fclose(f) == 0 && put == n;
}

static bool slurp(const std::string& path, std::vector<double>* v) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes < 0 || bytes % 8) {
    std::fclose(f);
    return false;
  }
  v->resize((size_t)bytes / 8);
  const size_t got = v->empty() ? 0 : std::fread(v->data(), 8, v->size(), f);
  std::fclose(f);
  return got == v->size();
}

static int assemble(const ptx_scene_desc* d, PtHostArrays* h) {
  std::string msg;
  if (scene_check_desc(d, &msg)) return 1;
  const std::vector<Box> boxes = scene_boxes(d);
  BvhResult t = bvh_build(boxes, scene_num_bins(d), d->length_cutoff, d->leaf_kind == PTX_LEAF_SIMD);
  if (scene_set_tree(d, std::move(t), h, &msg)) return 1;
  scene_assemble(d, boxes, SceneOptions(), h);
  return 0;
}

static int load_scene(const std::string& name, int width, int height, PtHostArrays* h) {
  if (name == "shirley") {
    pth_scene* s = pth_scene_shirley(width, height, 0, 42);
    if (!s) return 1;
    const int rc = assemble(pth_scene_desc(s), h);
    pth_scene_free(s);
    return rc;
  }
  if (name.rfind("file:", 0) != 0) return 2;
  std::vector<double> q;
  if (!slurp(name.substr(5), &q) || q.empty() || q.size() % 4) return 2;
  const size_t n = q.size() / 4;
  std::vector<double> x(n), y(n), z(n), r(n);
  std::vector<int32_t> m(n, 0);
  for (size_t i = 0; i < n; ++i) {
    x[i] = q[4 * i];
    y[i] = q[4 * i + 1];
    z[i] = q[4 * i + 2];
    r[i] = q[4 * i + 3];
  }
  ptx_material mat{};
  ptx_texture tex{};
  ptx_scene_desc d{};
  d.n_spheres = (int32_t)n;
  d.sphere_x = x.data(); d.sphere_y = y.data(); d.sphere_z = z.data(); d.sphere_r = r.data(); d.sphere_material = m.data();
  d.n_materials = 1; d.materials = &mat; d.n_textures = 1; d.textures = &tex;
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -0.5; d.camera.view_x = 2.0; d.camera.view_y = 1.0;
  d.leaf_kind = PTX_LEAF_SIMD;
  d.length_cutoff = 16;
  return assemble(&d, h);
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const std::string mode = argv[1], dir = argv[5];
  const int width = std::atoi(argv[3]), height = std::atoi(argv[4]);
  int mutant = 0;
  bool guards = true;
  for (int i = 6; i < argc; ++i) {
    const std::string a = argv[i];
    if (a.rfind("mutant=", 0) == 0) mutant = std::atoi(a.c_str() + 7);
    else if (a == "guards=0") guards = false;
    else return 2;
  }
  if (width < 1 || height < 1 || (mode != "grid" && mode != "scan")) return 2;
#ifdef PT_TILE_TEST_MUTANTS
  pt_tile_test_mutant = mutant;
#else
  if (mutant) return 2;
#endif
  PtHostArrays h;
  if (const int rc = load_scene(argv[2], width, height, &h)) return rc;
  if (!scene_tile_lists_possible(h)) return 1;
  const auto t0 = std::chrono::steady_clock::now();
  const PtTileGrid g = scene_tile_lists(h, width, height);
  const long long us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  if (g.rec.size() != (size_t)g.tiles_x * g.tiles_y || g.rec.empty()) return 1;
  if (mode == "grid") {
    if (!dump(dir, "nodes", h.nodes.data(), h.nodes.size()) || !dump(dir, "sph", h.sph.data(), (size_t)h.dev.n_slots * 4) ||
        !dump(dir, "slot_prim", h.slot_prim.data(), (size_t)h.dev.n_slots) || !dump(dir, "grid", g.rec.data(), g.rec.size()))
      return 1;
    std::printf("nodes %zu slots %d tiles_x %d tiles_y %d walk %d longest %d build_us %lld\n", h.nodes.size(), h.dev.n_slots, g.tiles_x, g.tiles_y,
                g.n_walk, g.longest, us);
    std::printf("camera %a %a %a %a\n", h.dev.cam_llx, h.dev.cam_lly, h.dev.cam_vx, h.dev.cam_vy);
    return 0;
  }
  std::vector<double> samples;
  if (!slurp(dir + "/samples.bin", &samples) || samples.size() % 2) return 2;
  const size_t n = samples.size() / 2;
  struct Hit {
    double t;
    int32_t slot, status;
  };
  std::vector<double> dirs(3 * n);
  std::vector<Hit> hits(n);
  const double widthf = 1.0 / (double)width, heightf = 1.0 / (double)height;
  long long n_guard = 0, n_walk = 0;
  for (size_t i = 0; i < n; ++i) {
    const double px = samples[2 * i], py = samples[2 * i + 1];
    if (!(px >= 0.0 && px < (double)width && py >= 0.0 && py < (double)height)) return 2;
    /* pt_primary_dir: cx = (x + dxs) widthf, cy = 1 - (gy + dys) heightf; Camera.ray */
    const double cx = px * widthf, cy = 1.0 - (py * heightf);
    const V3 d = v3_normalize(v3(h.dev.cam_llx + (h.dev.cam_vx * cx), h.dev.cam_lly + (h.dev.cam_vy * cy), -1.0));
    dirs[3 * i] = d.x;
    dirs[3 * i + 1] = d.y;
    dirs[3 * i + 2] = d.z;
    const PtTileRec& rec = g.rec[(size_t)((int)py >> 3) * g.tiles_x + ((int)px >> 3)];
    const uint32_t oct = (d.x >= 0.0 ? 1u : 0u) | (d.y >= 0.0 ? 2u : 0u) | (d.z >= 0.0 ? 4u : 0u);
    Hit& o = hits[i];
    o.t = 0.0;
    o.slot = -1;
    if (rec.count == PT_TILE_WALK || oct != rec.octant) {
      o.status = 2;
      n_walk++;
      continue;
    }
    const auto slot_of = [&rec](int k) { return (uint32_t)rec.slot[k]; };
    const auto any = [](bool b) { return b; };
    const PtTileHit th = guards ? pt_tile_scan<true>(h.sph.data(), slot_of, any, rec.count, true, d, 1.7976931348623157e308)
                                : pt_tile_scan<false>(h.sph.data(), slot_of, any, rec.count, true, d, 1.7976931348623157e308);
    o.t = th.slot >= 0 ? th.t : 0.0;
    o.slot = th.slot;
    o.status = th.guard ? 1 : 0;
    n_guard += th.guard;
  }
  if (!dump(dir, "dirs", dirs.data(), dirs.size()) || !dump(dir, "hits", hits.data(), hits.size())) return 1;
  std::printf("rays %zu guards %lld walk %lld\n", n, n_guard, n_walk);
  return 0;
}
