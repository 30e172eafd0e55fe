// pfm.cpp -- a reader for Portable Float Map images, the one image format the hosts decode (--envmap, --ground-texture), and the
// writer that mirrors it (--hdr-out).
//
//   "PF" (three channels) or "Pf" (one, read as grey: r = g = b), white space, WIDTH, white space, HEIGHT, white space, SCALE, exactly
//   one white-space byte, then WIDTH * HEIGHT * channels binary32 values, rows BOTTOM TO TOP.  SCALE < 0: little-endian, > 0:
//   big-endian; its magnitude, a unit the writer chose, is not applied.
//
// The file's row order is the image rule's: row 0 is v = 0 (include/ptx.h), so the rows are kept as they come.  The values go to
// binary64 unchanged (linear, no colour-space conversion).  A parser of untrusted input: every length is checked against the bytes
// that are there before anything is read or allocated (tests/c/pfm_driver.cpp runs it under the sanitizers).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host.h"

struct pth_image {
  int32_t width = 0, height = 0, channels = 0;
  std::vector<double> rgb;
};

namespace {
thread_local std::string g_pfm_err;

pth_image* fail(const std::string& msg) {
  g_pfm_err = "PFM: " + msg;
  return nullptr;
}
bool is_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

// the next white-space separated token of the header, at most 32 bytes; false when the bytes run out first
bool token(const unsigned char* p, size_t n, size_t* at, std::string* out) {
  while (*at < n && is_space(p[*at])) ++*at;
  out->clear();
  while (*at < n && !is_space(p[*at])) {
    if (out->size() >= 32) return false;
    out->push_back((char)p[(*at)++]);
  }
  return !out->empty() && *at < n; // a token the file ends in has no separator behind it
}
bool parse_int(const std::string& s, long* out) {
  char* end = nullptr;
  const long v = std::strtol(s.c_str(), &end, 10);
  if (end == s.c_str() || *end) return false;
  *out = v;
  return true;
}
}  // namespace

extern "C" {

const char* pth_image_error(void) { return g_pfm_err.c_str(); }

pth_image* pth_pfm_parse(const unsigned char* bytes, size_t n) {
  if (!bytes && n) return fail("no data");
  try {
    size_t at = 0;
    std::string magic, ws, hs, ss;
    if (n < 2 || bytes[0] != 'P' || (bytes[1] != 'F' && bytes[1] != 'f')) return fail("expected the file to start with \"PF\" or \"Pf\"");
    if (!token(bytes, n, &at, &magic) || magic.size() != 2) return fail("malformed header (the magic number)");
    const int channels = magic[1] == 'F' ? 3 : 1;
    if (!token(bytes, n, &at, &ws) || !token(bytes, n, &at, &hs)) return fail("malformed header (width and height)");
    long w = 0, h = 0;
    if (!parse_int(ws, &w) || !parse_int(hs, &h)) return fail("width and height must be integers (got \"" + ws + "\", \"" + hs + "\")");
    if (w < 1 || w > PTX_IMAGE_MAX_SIZE || h < 1 || h > PTX_IMAGE_MAX_SIZE)
      return fail("size " + std::to_string(w) + " x " + std::to_string(h) + ": width and height must be in [1, " + std::to_string(PTX_IMAGE_MAX_SIZE) + "]");
    if (!token(bytes, n, &at, &ss)) return fail("malformed header (the scale)");
    char* end = nullptr;
    const double scale = std::strtod(ss.c_str(), &end);
    if (end == ss.c_str() || *end || !std::isfinite(scale) || scale == 0.0) return fail("the scale must be a finite non-zero number (got \"" + ss + "\")");
    ++at; // the one white-space byte behind the scale (token() has seen that it is there)
    const size_t count = (size_t)w * (size_t)h * (size_t)channels; // <= 3 * 2^28
    if ((n - at) / 4 < count)
      return fail("the file ends early: " + std::to_string(count * 4) + " bytes of pixels expected, " + std::to_string(n - at) + " present");
    const bool little = scale < 0.0;
    pth_image* img = new pth_image();
    img->width = (int32_t)w;
    img->height = (int32_t)h;
    img->channels = channels;
    img->rgb.resize((size_t)w * (size_t)h * 3);
    const unsigned char* px = bytes + at;
    for (size_t i = 0; i < count; ++i) {
      const unsigned char* b = px + 4 * i;
      const uint32_t u = little ? ((uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24)
                                : ((uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24);
      float f;
      std::memcpy(&f, &u, 4);
      if (!std::isfinite(f)) {
        const size_t pixel = i / (size_t)channels;
        delete img;
        return fail("pixel (" + std::to_string(pixel % (size_t)w) + ", " + std::to_string(pixel / (size_t)w) + ") is not finite");
      }
      if (channels == 3) img->rgb[i] = (double)f;
      else img->rgb[3 * i] = img->rgb[3 * i + 1] = img->rgb[3 * i + 2] = (double)f;
    }
    return img;
  } catch (const std::exception& e) { // bad_alloc: report, never terminate the host
    return fail(std::string("load failed: ") + e.what());
  }
}

pth_image* pth_pfm_load(const char* path) {
  std::FILE* f = path ? std::fopen(path, "rb") : nullptr;
  if (!f) return fail(std::string("cannot open ") + (path ? path : "(null)"));
  std::vector<unsigned char> bytes;
  try {
    unsigned char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) {
      bytes.insert(bytes.end(), buf, buf + got);
      if (bytes.size() > ((size_t)PTX_IMAGE_MAX_SIZE * PTX_IMAGE_MAX_SIZE * 12 + 4096)) break; // more than the largest image: not read
    }
  } catch (const std::exception& e) {
    std::fclose(f);
    return fail(std::string("load failed: ") + e.what());
  }
  std::fclose(f);
  return pth_pfm_parse(bytes.data(), bytes.size());
}

// The mirror of pth_pfm_load: "PF", WIDTH HEIGHT, the scale -1.0 (little-endian), one newline each, then width * height * 3 binary32
// values -- each the binary64 value rounded to nearest -- rows in the order they are given (the reader keeps them as they come, so
// a file written and read back is the binary32 rounding of what was written, row for row).  A value that is not finite, or that
// rounds to a binary32 that is not, is refused: the reader would refuse the file.  0 on success, -1 + pth_image_error().
int32_t pth_pfm_write(const char* path, int32_t width, int32_t height, const double* rgb) {
  if (!path || !rgb) return fail("pth_pfm_write: NULL argument"), -1;
  if (width < 1 || width > PTX_IMAGE_MAX_SIZE || height < 1 || height > PTX_IMAGE_MAX_SIZE)
    return fail("size " + std::to_string(width) + " x " + std::to_string(height) + ": width and height must be in [1, " + std::to_string(PTX_IMAGE_MAX_SIZE) + "]"), -1;
  try {
    const size_t count = (size_t)width * (size_t)height * 3;
    const std::string header = "PF\n" + std::to_string(width) + " " + std::to_string(height) + "\n-1.0\n";
    std::vector<unsigned char> bytes(header.size() + count * 4);
    std::memcpy(bytes.data(), header.data(), header.size());
    unsigned char* px = bytes.data() + header.size();
    for (size_t i = 0; i < count; ++i) {
      const float f = (float)rgb[i];
      if (!std::isfinite(f)) {
        const size_t pixel = i / 3;
        return fail("pixel (" + std::to_string(pixel % (size_t)width) + ", " + std::to_string(pixel / (size_t)width) + ") is not finite in binary32"), -1;
      }
      uint32_t u;
      std::memcpy(&u, &f, 4);
      px[4 * i] = (unsigned char)(u & 0xffu);
      px[4 * i + 1] = (unsigned char)((u >> 8) & 0xffu);
      px[4 * i + 2] = (unsigned char)((u >> 16) & 0xffu);
      px[4 * i + 3] = (unsigned char)((u >> 24) & 0xffu);
    }
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return fail(std::string("cannot write ") + path), -1;
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (std::fclose(f) != 0 || !ok) return fail(std::string("writing ") + path + " failed"), -1;
    return 0;
  } catch (const std::exception& e) {
    return fail(std::string("write failed: ") + e.what()), -1;
  }
}

void pth_image_free(pth_image* img) { delete img; }
int32_t pth_image_width(const pth_image* img) { return img ? img->width : 0; }
int32_t pth_image_height(const pth_image* img) { return img ? img->height : 0; }
int32_t pth_image_channels(const pth_image* img) { return img ? img->channels : 0; }
const double* pth_image_rgb(const pth_image* img) { return img ? img->rgb.data() : nullptr; }

void pth_rotation_y(double degrees, double R[9]) {
  const double t = degrees * (3.14159265358979323846 / 180.0), c = std::cos(t), s = std::sin(t);
  const double m[9] = {c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c};
  std::memcpy(R, m, sizeof m);
}

int32_t pth_ground_texture(const ptx_scene_desc* d) {
  if (!d) return -1;
  if (d->n_floor_triangles > 0) {
    const ptx_material& m = d->materials[d->floor_material[0]];
    return m.kind == PTX_MAT_DIELECTRIC ? -1 : m.texture;
  }
  for (int32_t i = 0; i < d->n_textures; ++i)
    if (d->textures[i].kind == PTX_TEX_CHECKER) return i;
  return -1;
}

}  // extern "C"
