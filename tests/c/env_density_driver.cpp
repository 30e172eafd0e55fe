// Driver for the density over the environment image (csrc/scene_host.cpp: scene_env_density, scene_check_env_rotation), CPU build only,
// under -fsanitize=address,undefined like tests/c/tile_lists_driver.cpp.  Built by `make asan` in path_tracer_ocaml_amd/host, run by
// tests/test_envlight_sanitizers.py.
//   density <width> <height> <rgb.bin> <out.bin>
//       <rgb.bin>: width * height * 3 binary64 texels, row 0 first.  Makes the texel records the library keeps (scene_image_records),
//       builds the density of them and writes its table (pt_scene.h, PT_ENVD_*: T, last row, m[H], last column [H], c[H x W], w[H x W]) to
//       <out.bin>;
//       prints "rc <code> total <hex float> last_row <n> doubles <n>" and, when the density is refused, "msg <text>"
//   rotation <9 numbers>
//       prints "rc <code>" and, when the matrix is refused, "msg <text>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../path_tracer_ocaml_amd/csrc/scene_host.h"

int main(int argc, char** argv) {
  if (argc == 11 && !std::strcmp(argv[1], "rotation")) {
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = std::strtod(argv[2 + k], nullptr);
    std::string msg;
    const int rc = scene_check_env_rotation(R, &msg);
    std::printf("rc %d\n", rc);
    if (rc) std::printf("msg %s\n", msg.c_str());
    return 0;
  }
  if (argc != 6 || std::strcmp(argv[1], "density")) {
    std::fprintf(stderr, "usage: env_density_driver density W H rgb.bin out.bin | rotation r0 .. r8\n");
    return 2;
  }
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  if (W < 1 || H < 1 || W > PTX_IMAGE_MAX_SIZE || H > PTX_IMAGE_MAX_SIZE) return 2;
  std::vector<double> rgb((size_t)W * (size_t)H * 3);
  FILE* f = std::fopen(argv[4], "rb");
  if (!f || std::fread(rgb.data(), sizeof(double), rgb.size(), f) != rgb.size()) return 3;
  std::fclose(f);
  ptx_image img{};
  img.width = W;
  img.height = H;
  img.rgb = rgb.data();
  std::string msg;
  if (scene_check_image(&img, true, &msg) != 0) {
    std::printf("rc %d\nmsg %s\n", PTX_ERR_ARG, msg.c_str());
    return 0;
  }
  const std::vector<double> rec = scene_image_records(&img);
  PtEnvDensity d;
  const int rc = scene_env_density(rec.data(), W, H, &d, &msg);
  std::printf("rc %d total %a last_row %d doubles %zu\n", rc, d.total, d.last_row, d.table.size());
  if (rc) std::printf("msg %s\n", msg.c_str());
  f = std::fopen(argv[5], "wb");
  if (!f || std::fwrite(d.table.data(), sizeof(double), d.table.size(), f) != d.table.size() || std::fclose(f) != 0) return 4;
  return 0;
}
