// pfm_driver.cpp -- the hosts' PFM reader (path_tracer_ocaml_amd/host/pfm.cpp) as a stand-alone program for the sanitizer build
// (host/Makefile `asan`; tests/test_pfm.py): `pfm_driver FILE...` loads every file and prints one line per file --
//   ok WIDTH HEIGHT CHANNELS then the width * height * 3 values as hexadecimal floats, or
//   error MESSAGE
// and always exits 0: a refused file is an answer, a sanitizer report is the failure.
#include <cstdio>

#include "../../path_tracer_ocaml_amd/host/host.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    pth_image* img = pth_pfm_load(argv[i]);
    if (!img) {
      std::printf("error %s\n", pth_image_error());
      continue;
    }
    const int w = pth_image_width(img), h = pth_image_height(img);
    std::printf("ok %d %d %d", w, h, pth_image_channels(img));
    const double* rgb = pth_image_rgb(img);
    for (long k = 0; k < (long)w * h * 3; ++k) std::printf(" %a", rgb[k]);
    std::printf("\n");
    pth_image_free(img);
  }
  // the in-memory entry point on an empty and on a one-byte buffer
  const unsigned char one[1] = {'P'};
  if (pth_pfm_parse(nullptr, 0) || pth_pfm_parse(one, 0) || pth_pfm_parse(one, 1)) return 1;
  return 0;
}
