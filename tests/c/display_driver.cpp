// Driver for the host half of the display rule (csrc/scene_host.cpp: display_check, display_thresholds, display_apply_host over
// csrc/pt_display.h), CPU build only, under -fsanitize=address,undefined like tests/c/env_density_driver.cpp.  Built by `make asan` in
// path_tracer_ocaml_amd/host, run by tests/test_display_sanitizers.py.
//   thresholds <out.bin>
//       writes the 255 sRGB thresholds; prints "rc 0 doubles 255"
//   apply <format> <transfer> <tone> <exposure> <n_pixels> <rgb.bin> <out.bin>
//       <rgb.bin>: n_pixels * 3 binary64 values.  The settings are checked as every entry point checks them; the rule then runs from a
//       heap buffer of exactly n_pixels * 3 doubles into one of exactly n_pixels * pixel_bytes bytes (an access beyond either is the
//       sanitizer's to report), which is written to <out.bin>;
//       prints "rc <code> bytes <n>" and, when the settings are refused, "msg <text>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../path_tracer_ocaml_amd/csrc/scene_host.h"

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "thresholds")) {
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(display_thresholds(), sizeof(double), 255, f) != 255 || std::fclose(f) != 0) return 4;
    std::printf("rc 0 doubles 255\n");
    return 0;
  }
  if (argc != 9 || std::strcmp(argv[1], "apply")) {
    std::fprintf(stderr, "usage: display_driver thresholds out.bin | apply format transfer tone exposure n_pixels rgb.bin out.bin\n");
    return 2;
  }
  ptx_display_params d{};
  d.format = std::atoi(argv[2]);
  d.transfer = std::atoi(argv[3]);
  d.tone = std::atoi(argv[4]);
  d.exposure = std::strtod(argv[5], nullptr);
  const long long n = std::atoll(argv[6]);
  if (n < 0 || n > (1ll << 24)) return 2;
  std::string msg;
  const int rc = display_check(&d, &msg);
  if (rc) {
    std::printf("rc %d bytes 0\nmsg %s\n", rc, msg.c_str());
    return 0;
  }
  const size_t n_in = (size_t)n * 3, n_out = (size_t)n * (size_t)display_pixel_bytes(d.format);
  std::unique_ptr<double[]> rgb(new double[n_in]);
  std::unique_ptr<unsigned char[]> out(new unsigned char[n_out]);
  FILE* f = std::fopen(argv[7], "rb");
  if (!f || std::fread(rgb.get(), sizeof(double), n_in, f) != n_in) return 3;
  std::fclose(f);
  display_apply_host(d, n, rgb.get(), out.get());
  f = std::fopen(argv[8], "wb");
  if (!f || std::fwrite(out.get(), 1, n_out, f) != n_out || std::fclose(f) != 0) return 4;
  std::printf("rc 0 bytes %zu\n", n_out);
  return 0;
}
