// Driver for the sphere light list and table (csrc/scene_host.cpp: the emissive-sphere list of scene_set_tree, sphere_light_table_build
// beside light_table_build), CPU build only, under -fsanitize=address,undefined like tests/c/env_density_driver.cpp.  Built by `make asan`
// in path_tracer_ocaml_amd/host, run by tests/test_spherelight_sanitizers.py.
//   table <n_spheres> <spheres.bin> <with_triangle 0|1> <out.bin>
//       <spheres.bin>: n_spheres records of 5 binary64 {x, y, z, r, emit}: material i emits (emit, emit, emit).  with_triangle: one
//       emissive triangle precedes the spheres in the build list.  Builds the tree with the host builder, takes it (scene_set_tree makes
//       both emissive lists), builds the triangles' table and the sphere table that continues its running sum, and writes the sphere
//       records (pt_scene.h, PT_SLIGHT_*: c, r, r2, W, cum, 0) to <out.bin>;
//       prints "rc <code> triangles <n> spheres <n> kept <n> base <hex float> records <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../path_tracer_ocaml_amd/csrc/scene_host.h"

int main(int argc, char** argv) {
  if (argc != 6 || std::strcmp(argv[1], "table")) {
    std::fprintf(stderr, "usage: sphere_light_driver table N spheres.bin WITH_TRIANGLE out.bin\n");
    return 2;
  }
  const int n = std::atoi(argv[2]), with_triangle = std::atoi(argv[4]);
  if (n < 1 || n > 100000) return 2;
  std::vector<double> rec((size_t)n * 5);
  FILE* f = std::fopen(argv[3], "rb");
  if (!f || std::fread(rec.data(), sizeof(double), rec.size(), f) != rec.size()) return 3;
  std::fclose(f);
  std::vector<double> sx((size_t)n), sy((size_t)n), sz((size_t)n), sr((size_t)n);
  std::vector<int32_t> sm((size_t)n);
  std::vector<ptx_material> mats((size_t)n + 1);
  std::memset(mats.data(), 0, sizeof(ptx_material) * mats.size());
  ptx_texture tex;
  std::memset(&tex, 0, sizeof tex);
  tex.kind = PTX_TEX_SOLID;
  for (int i = 0; i < n; ++i) {
    sx[(size_t)i] = rec[(size_t)i * 5];
    sy[(size_t)i] = rec[(size_t)i * 5 + 1];
    sz[(size_t)i] = rec[(size_t)i * 5 + 2];
    sr[(size_t)i] = rec[(size_t)i * 5 + 3];
    sm[(size_t)i] = i;
    mats[(size_t)i].kind = PTX_MAT_LAMBERTIAN;
    for (int c = 0; c < 3; ++c) mats[(size_t)i].emit[c] = rec[(size_t)i * 5 + 4];
  }
  mats[(size_t)n].kind = PTX_MAT_LAMBERTIAN;
  for (int c = 0; c < 3; ++c) mats[(size_t)n].emit[c] = 7.0;
  const double vx[3] = {-1.0, 2.0, 0.5}, vy[3] = {4.0, 4.0, 4.5}, vz[3] = {-3.0, -3.5, -6.0}, uv[6] = {0, 0, 1, 0, 0, 1};
  const int32_t idx[3] = {0, 1, 2}, tm[1] = {n};
  ptx_scene_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_spheres = n;
  d.sphere_x = sx.data(); d.sphere_y = sy.data(); d.sphere_z = sz.data(); d.sphere_r = sr.data();
  d.sphere_material = sm.data();
  if (with_triangle) {
    d.n_vertices = 3;
    d.vertex_x = vx; d.vertex_y = vy; d.vertex_z = vz;
    d.n_triangles = 1;
    d.tri_indices = idx; d.tri_uv = uv; d.tri_material = tm;
  }
  d.n_materials = n + 1;
  d.materials = mats.data();
  d.n_textures = 1;
  d.textures = &tex;
  d.camera.lower_left_x = -1.0; d.camera.lower_left_y = -0.5; d.camera.view_x = 2.0; d.camera.view_y = 1.0;
  d.leaf_kind = PTX_LEAF_ARRAY;
  d.length_cutoff = 4;
  d.num_bins = 32;
  std::string msg;
  int rc = scene_check_desc(&d, &msg);
  if (rc) {
    std::printf("rc %d\nmsg %s\n", rc, msg.c_str());
    return 0;
  }
  PtHostArrays h;
  const std::vector<Box> boxes = scene_boxes(&d);
  BvhResult t = bvh_build(boxes, scene_num_bins(&d), d.length_cutoff, false);
  if ((rc = scene_set_tree(&d, std::move(t), &h, &msg)) != 0) {
    std::printf("rc %d\nmsg %s\n", rc, msg.c_str());
    return 0;
  }
  double base = 0.0;
  if (h.n_emissive_tris >= 1 && h.n_emissive_tris <= PTX_MAX_LIGHT_TRIANGLES) {
    const std::vector<double> tri = light_table_build(h);
    base = tri[tri.size() - PT_LIGHT_DOUBLES + PT_LIGHT_CUM];
  }
  // what the setter does: it takes the list only when it holds 1 .. PTX_MAX_LIGHT_SPHERES spheres
  std::vector<double> table;
  if (h.n_emissive_spheres >= 1 && h.n_emissive_spheres <= PTX_MAX_LIGHT_SPHERES) table = sphere_light_table_build(h, base);
  std::printf("rc 0 triangles %d spheres %d kept %zu base %a records %zu\n", h.n_emissive_tris, h.n_emissive_spheres,
              h.emissive_spheres.size() / 4, base, table.size() / PT_SLIGHT_DOUBLES);
  f = std::fopen(argv[5], "wb");
  if (!f || (table.size() && std::fwrite(table.data(), sizeof(double), table.size(), f) != table.size()) || std::fclose(f) != 0) return 4;
  return 0;
}
