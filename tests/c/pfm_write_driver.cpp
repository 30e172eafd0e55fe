// pfm_write_driver.cpp -- the hosts' PFM writer (path_tracer_ocaml_amd/host/pfm.cpp, pth_pfm_write) as a stand-alone program for
// the sanitizer build (host/Makefile `asan`; tests/test_pfm_write.py): `pfm_write_driver DIR` writes images of several sizes into
// DIR, loads each back through pth_pfm_load and compares it with the binary32 rounding of what was written, row for row; then the
// refusals.  Prints one line per step and exits 0 when every step did what it should: a sanitizer report is the other failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../path_tracer_ocaml_amd/host/host.h"

static int failures = 0;
static void expect(bool ok, const std::string& what) {
  std::printf("%s %s\n", ok ? "ok" : "FAILED", what.c_str());
  if (!ok) ++failures;
}

// values that exercise the rounding: binary64 values between two binary32 ones, ties, subnormals of binary32, negatives, zeros
static double value(uint64_t& state) {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  const double u = (double)(state >> 11) * (1.0 / 9007199254740992.0);
  switch ((state >> 7) % 8) {
    case 0: return u;
    case 1: return -u * 1e3;
    case 2: return u * 1e-42; // subnormal in binary32
    case 3: return 1.0 + std::ldexp(1.0, -24); // a tie between two binary32 values
    case 4: return u * 1e30;
    case 5: return (state & 1) ? 0.0 : -0.0;
    case 6: return std::ldexp(u, -160); // rounds to zero in binary32
    default: return u * u * 65504.0;
  }
}

static void round_trip(const std::string& dir, int w, int h, uint64_t seed) {
  std::vector<double> rgb((size_t)w * h * 3);
  for (double& v : rgb) v = value(seed);
  const std::string path = dir + "/w" + std::to_string(w) + "x" + std::to_string(h) + ".pfm";
  const std::string tag = std::to_string(w) + " x " + std::to_string(h);
  expect(pth_pfm_write(path.c_str(), w, h, rgb.data()) == 0, "write " + tag);
  pth_image* img = pth_pfm_load(path.c_str());
  expect(img != nullptr, "load " + tag);
  if (!img) return;
  bool same = pth_image_width(img) == w && pth_image_height(img) == h && pth_image_channels(img) == 3;
  const double* back = pth_image_rgb(img);
  for (size_t i = 0; same && i < rgb.size(); ++i) {
    const double want = (double)(float)rgb[i];
    same = back[i] == want && std::signbit(back[i]) == std::signbit(want);
  }
  expect(same, "round trip " + tag + " is the binary32 rounding, rows in the same order");
  pth_image_free(img);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  round_trip(dir, 1, 1, 1);
  round_trip(dir, 16, 8, 2);
  round_trip(dir, 7, 13, 3);
  round_trip(dir, 257, 3, 4);
  const double one[3] = {1.0, 2.0, 3.0};
  const std::string path = dir + "/refused.pfm";
  expect(pth_pfm_write(nullptr, 1, 1, one) == -1, "NULL path");
  expect(pth_pfm_write(path.c_str(), 1, 1, nullptr) == -1, "NULL image");
  expect(pth_pfm_write(path.c_str(), 0, 1, one) == -1 && pth_pfm_write(path.c_str(), 1, -4, one) == -1, "sizes below 1");
  expect(pth_pfm_write(path.c_str(), PTX_IMAGE_MAX_SIZE + 1, 1, one) == -1, "a size above the limit");
  const double bad[3] = {1.0, std::numeric_limits<double>::quiet_NaN(), 3.0};
  expect(pth_pfm_write(path.c_str(), 1, 1, bad) == -1 && std::string(pth_image_error()).find("not finite") != std::string::npos, "a NaN");
  const double big[3] = {1.0, 2.0, 1e39}; // finite in binary64, infinite in binary32
  expect(pth_pfm_write(path.c_str(), 1, 1, big) == -1 && std::string(pth_image_error()).find("pixel (0, 0)") != std::string::npos, "a value beyond binary32");
  expect(pth_pfm_write((dir + "/no/such/dir/x.pfm").c_str(), 1, 1, one) == -1, "a path that cannot be written");
  std::FILE* f = std::fopen(path.c_str(), "rb");
  expect(f == nullptr, "a refused image leaves no file");
  if (f) std::fclose(f);
  return failures ? 1 : 0;
}
