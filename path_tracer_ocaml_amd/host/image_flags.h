// image_flags.h -- what the three executables share of --envmap / --envmap-rotate / --ground-texture / --texture-nearest: the PFM
// files through libpt_host.so's reader (pfm.cpp) into ptx_scene_set_environment / ptx_scene_set_texture_image.  Header only: the
// executables link libptx_hip.so, libpt_host.so does not.
#ifndef PTH_IMAGE_FLAGS_H
#define PTH_IMAGE_FLAGS_H

#include <cstdlib>
#include <string>

#include "host.h"

struct ImageFlags {
  std::string envmap;          // --envmap=FILE.pfm: a latitude-longitude environment, bilinear
  double envmap_rotate = 0.0;  // --envmap-rotate=DEG: about the camera-space y axis
  std::string ground_texture;  // --ground-texture=FILE.pfm: on the ground / floor material's texture, repeated on both axes
  bool texture_nearest = false; // --texture-nearest: the one texel instead of the bilinear four
};

// one argument of the command line; true when it was one of the four (*bad set when its value is malformed)
inline bool image_flag(const std::string& a, ImageFlags* f, std::string* bad) {
  auto value = [&](const char* name, std::string* out) {
    const std::string p = std::string("--") + name + "=";
    if (a.rfind(p, 0) != 0) return false;
    *out = a.substr(p.size());
    return true;
  };
  std::string v;
  if (value("envmap", &f->envmap)) {
    if (f->envmap.empty()) *bad = "invalid value for --envmap, expected a PFM file";
    return true;
  }
  if (value("ground-texture", &f->ground_texture)) {
    if (f->ground_texture.empty()) *bad = "invalid value for --ground-texture, expected a PFM file";
    return true;
  }
  if (value("envmap-rotate", &v)) {
    char* end = nullptr;
    f->envmap_rotate = std::strtod(v.c_str(), &end);
    if (end == v.c_str() || *end || !(f->envmap_rotate - f->envmap_rotate == 0.0)) *bad = "invalid value for --envmap-rotate, expected degrees";
    return true;
  }
  if (a == "--texture-nearest") {
    f->texture_nearest = true;
    return true;
  }
  return false;
}

// what the flags ask of each other, and of the executable: empty, or the message.  photon_mapper: cornell_box / ganesha, whose paths
// end where they leave the scene (progressive_photon_map.ml:326), so that --envmap is accepted and never seen; has_ground: the
// executable has a ground or floor material to put --ground-texture on (shirley_spheres, ganesha; not cornell_box)
inline std::string image_flags_check(const ImageFlags& f, bool has_ground) {
  if (f.texture_nearest && f.ground_texture.empty()) return "--texture-nearest requires --ground-texture";
  if (f.envmap_rotate != 0.0 && f.envmap.empty()) return "--envmap-rotate requires --envmap";
  if (!f.ground_texture.empty() && !has_ground) return "--ground-texture: this scene has no ground or floor material (shirley_spheres and ganesha have)";
  return "";
}
#define PTH_IMAGE_FLAGS_USAGE "[--envmap=FILE.pfm] [--envmap-rotate=DEG] [--ground-texture=FILE.pfm] [--texture-nearest]"

// 0, or -1 with *err set
inline int apply_image_flags(ptx_scene* scene, const ptx_scene_desc* d, const ImageFlags& f, std::string* err) {
  if (!f.envmap.empty()) {
    pth_image* img = pth_pfm_load(f.envmap.c_str());
    if (!img) { *err = f.envmap + ": " + pth_image_error(); return -1; }
    double R[9];
    pth_rotation_y(f.envmap_rotate, R);
    const ptx_image pi = {pth_image_width(img), pth_image_height(img), PTX_IMAGE_BILINEAR, 0, pth_image_rgb(img)};
    const int32_t rc = ptx_scene_set_environment(scene, &pi, R);
    pth_image_free(img);
    if (rc != 0) { *err = std::string("ptx_scene_set_environment: ") + ptx_last_error(); return -1; }
  }
  if (!f.ground_texture.empty()) {
    const int32_t index = pth_ground_texture(d);
    if (index < 0) { *err = "--ground-texture: the scene has no ground or floor texture to put an image on"; return -1; }
    pth_image* img = pth_pfm_load(f.ground_texture.c_str());
    if (!img) { *err = f.ground_texture + ": " + pth_image_error(); return -1; }
    const ptx_image pi = {pth_image_width(img), pth_image_height(img),
                          (f.texture_nearest ? 0 : PTX_IMAGE_BILINEAR) | PTX_IMAGE_REPEAT_U | PTX_IMAGE_REPEAT_V, 0, pth_image_rgb(img)};
    const int32_t rc = ptx_scene_set_texture_image(scene, index, &pi);
    pth_image_free(img);
    if (rc != 0) { *err = std::string("ptx_scene_set_texture_image: ") + ptx_last_error(); return -1; }
  }
  return 0;
}

#endif
