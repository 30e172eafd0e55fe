// render_command.cpp -- the reference's command line, kept flag for flag, in front of libptx_hip.so.
//
// Mirrors Render_command.Args.term (render_command/src/render_command.ml:16-47):
//   -d, --dimension=WIDTH,HEIGHT   (required)      --samples-per-pixel=INT (default 1)
//   -o, --output=PATH (default output.png)         --no-progress
//   --max-ray-bounces=INT (default 8)
// plus shirley_spheres' own --no-simd (shirley_spheres/bin/main.ml:12-23), and the prints of
// shirley_spheres/bin/main.ml:254-267 / render_command.ml:108.  Additions: --scene, --device, --gpus (SURVEY section 5
// "config / flags": the image spread over N GPUs of the node inside this process, ptx_render_params.n_gpus), and
// --progressive=K / --target-error=E: -o rewritten after every K passes (ptx_render_progressive), as the photon-map binaries
// rewrite it after every iteration, stopping early once the frame's relative standard error is at most E; and --adaptive=T
// (with --progressive=K passes per round and --min-passes=M): per-pixel pass counts, ptx_render_adaptive.
// --lighting=reference|path-order|sampled: the scene's lighting mode (ptx_scene_set_lighting); --lamp=HALF_SIDE,Y,EMIT (with
// --scene=cornell): a square lamp of that half side and emission at height Y (pth_scene_cornell_lamp).
// --denoise[=LEVELS]: the image of every update filtered by the variance-guided a-trous denoiser (ptx_render_denoised; with
// --progressive=K an update every K passes, without it one update after the last pass); --aov=PREFIX (with --denoise) also writes the
// first-hit feature means as PREFIX-albedo.png, PREFIX-normal.png (n / 2 + 1 / 2) and PREFIX-depth.png (z / max z).
// --envmap=FILE.pfm [--envmap-rotate=DEG]: a latitude-longitude environment in place of the background (ptx_scene_set_environment; the
// rotation is about the camera-space y axis); --ground-texture=FILE.pfm [--texture-nearest]: an image, repeated on both axes, on
// the ground (shirley) or floor (ganesha) material (ptx_scene_set_texture_image); image_flags.h.
// --lens-radius=R [--focus-distance=F]: a thin lens (ptx_scene_set_lens); without F it focuses on the camera's look-at target.
// --camera-eye=X,Y,Z --camera-target=X,Y,Z [--camera-fov=DEG]: renders from another camera (world coordinates, the scene's own up
// vector) over the scene built with its default one (ptx_scene_set_camera_pose: no vertex is transformed again, no tree rebuilt).
// --turntable=N: N frames on a circle about the vertical axis through the target, through ONE scene handle; frame k goes to the -o name
// with -kkk in front of its extension.  --turntable-arc=DEG (default 360): the N frames cover that arc, so a short sequence takes
// small steps.
// --temporal[=CAP] (with --turntable=T): every frame accumulates onto the history of the frames before, reprojected through the two
// cameras (ptx_render_temporal; CAP = max_history_passes, default 64).  --samples-per-pixel=S is then ONE FRAME's passes: the
// sequence's N is S * min(T, 16) and frame f renders slice f mod min(T, 16) of it, so consecutive frames draw different points of
// the low-discrepancy sequence.  With --denoise[=LEVELS] the accumulated frame is filtered.  Each frame prints
// "frame f -> FILE, history = P pixels".
// --envmap-sample (with --envmap and --lighting=sampled): the environment is importance-sampled (ptx_scene_set_environment_sampling),
// and sampled lighting then needs no emissive triangle.
// --sphere-lamp=X,Y,Z,R,EMIT (with --scene=shirley): a white Lambertian lamp sphere at that world point (pth_scene_shirley_lamp);
// --light-spheres (with --lighting=sampled): the emissive spheres are cone-sampled (ptx_scene_set_sphere_light_sampling), and sampled
// lighting then needs no emissive triangle.
// --panorama: a 360-degree lat-long panorama in the environment map's (u, v) convention (ptx_scene_set_camera_projection), for every
// --scene=; taken from the scene's own eye, or from --camera-eye / --turntable's; refused with --lens-radius and --temporal.
// --hdr-out=FILE.pfm (any render): also writes the square of every value of the final image -- the filmed linear radiance -- as a PFM
// (pth_pfm_write), which --envmap reads back: a panorama written here lights another scene.  With --turntable, frame k goes to the name
// with -kkk in front of its extension.
// --shutter=F (with --turntable=N; 0 < F <= 1): motion blur (ptx_scene_set_camera_shutter) -- frame f is exposed while the camera moves
// from its pose to fraction F of the way to frame f + 1's (pth_camera_shutter_between; 0.5 is a 180-degree shutter).
// --shutter-eye=X,Y,Z [--shutter-target=X,Y,Z] (with --camera-eye, no turntable): one frame exposed while the camera moves from
// --camera-eye / --camera-target to that eye (and target; default: --camera-target).  The library refuses --temporal under a shutter:
// its message, exit code 124.
// --exposure=E, --tone=none|reinhard|aces, --transfer=reference|linear|srgb (any render): the display of the image (include/ptx.h,
// "display outputs"); -o is written from its RGB8 bytes (pth_write_png8).  The plain render, --progressive and --denoise get those bytes
// from the device (ptx_render_display, ptx_render_progressive_display); --adaptive, --turntable, --temporal, --aov and --hdr-out keep the
// f64 image and convert it with ptx_display_apply, the same rule.  With no such flag the display is the reference's own conversion and
// every file is what it always was.  --hdr-out is the RGB32F / linear / no-tone display at exposure 1 whatever the flags say.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host.h"
#include "image_flags.h"

namespace {

struct Args {
  int width = 0, height = 0;
  int samples_per_pixel = 1;
  std::string output = "output.png";
  bool no_progress = false;
  int max_bounces = 8;
  bool no_simd = false;
  std::string scene = "shirley";
  int device = 0;
  int gpus = 1;
  int ganesha_triangles = 150000;
  double ceiling_emit = 12.0;
  std::string ganesha_ply; // -ganesha-ply <file> (ganesha/bin/main.ml:19-24); empty = synthetic stand-in mesh
  int progressive = 0;       // passes per update; 0 = one ptx_render
  double target_error = 0.0; // stop at the first update whose rel_err is <= this (0 = never)
  double adaptive = -1.0;    // per-pixel target T of ptx_render_adaptive (< 0: not adaptive)
  int min_passes = 0;        // --min-passes (0: not given; 8 with --adaptive)
  int lighting = PTX_LIGHTING_REFERENCE; // --lighting
  bool have_lamp = false;                // --lamp=HALF_SIDE,Y,EMIT
  double lamp_half_side = 0.0, lamp_y = 0.0, lamp_emit = 0.0;
  int denoise = -1;                      // --denoise[=LEVELS]: a-trous levels (< 0: no denoiser)
  std::string aov;                       // --aov=PREFIX
  bool have_filter = false;              // --filter=ORDER,RADIUS and / or --filter-renormalise
  ptx_film_params film{5, 1, 0, 0};      // ptx_film_defaults
  ImageFlags images;                     // --envmap, --envmap-rotate, --ground-texture, --texture-nearest
  bool envmap_sample = false;            // --envmap-sample
  bool light_spheres = false;            // --light-spheres
  bool have_sphere_lamp = false;         // --sphere-lamp=X,Y,Z,R,EMIT
  double sphere_lamp[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double lens_radius = 0.0;              // --lens-radius=R (0: the pinhole)
  double focus_distance = 0.0;           // --focus-distance=F (0: not given -- the distance from the eye to the look-at target)
  bool have_eye = false, have_target = false; // --camera-eye, --camera-target (given together)
  double camera_eye[3] = {0, 0, 0}, camera_target[3] = {0, 0, 0};
  double camera_fov = 0.0;               // --camera-fov=DEG (0: the scene camera's)
  int turntable = 0;                     // --turntable=N (0: one frame)
  double turntable_arc = 360.0;          // --turntable-arc=DEG
  bool have_arc = false;
  double temporal = -1.0;                // --temporal[=CAP]: max_history_passes (< 0: no temporal accumulation)
  double shutter = 0.0;                  // --shutter=F (0: none)
  bool have_shutter_eye = false, have_shutter_target = false; // --shutter-eye, --shutter-target
  double shutter_eye[3] = {0, 0, 0}, shutter_target[3] = {0, 0, 0};
  bool panorama = false;                 // --panorama
  std::string hdr_out;                   // --hdr-out=FILE.pfm
  ptx_display_params display{PTX_PIXEL_RGB8, PTX_TRANSFER_REFERENCE, PTX_TONE_NONE, 0, 1.0, {0, 0, 0, 0}}; // --transfer, --tone, --exposure
};

[[noreturn]] void usage(const char* prog, const char* msg) {
  if (msg) std::fprintf(stderr, "%s: %s\n", prog, msg);
  std::fprintf(stderr,
               "Usage: %s -d WIDTH,HEIGHT [--samples-per-pixel=INT] [-o PATH] [--no-progress]\n"
               "          [--max-ray-bounces=INT] [--no-simd] [--scene=shirley|cornell|ganesha] [--device=INT] [--gpus=INT]\n"
               "          [--ganesha-ply=PATH] [--triangles=INT] [--ceiling-emit=FLOAT]\n"
               "          [--progressive=K] [--target-error=FLOAT] [--adaptive=FLOAT] [--min-passes=M]\n"
               "          [--lighting=reference|path-order|sampled] [--lamp=HALF_SIDE,Y,EMIT]\n"
               "          [--denoise[=LEVELS]] [--aov=PREFIX] [--filter=ORDER,RADIUS] [--filter-renormalise]\n"
               "          " PTH_IMAGE_FLAGS_USAGE " [--envmap-sample]\n"
               "          [--lens-radius=FLOAT] [--focus-distance=FLOAT]\n"
               "          [--light-spheres] [--sphere-lamp=X,Y,Z,R,EMIT]\n"
               "          [--camera-eye=X,Y,Z --camera-target=X,Y,Z] [--camera-fov=DEG] [--turntable=N]\n"
               "          [--turntable-arc=DEG] [--temporal[=CAP]] [--panorama] [--hdr-out=FILE.pfm]\n"
               "          [--shutter=FRACTION] [--shutter-eye=X,Y,Z [--shutter-target=X,Y,Z]]\n"
               "          [--exposure=FLOAT] [--tone=none|reinhard|aces] [--transfer=reference|linear|srgb]\n",
               prog);
  std::exit(msg ? 124 : 0); // Cmdliner exits 124 on a CLI error
}

bool take_value(int argc, char** argv, int& i, const char* long_name, const char* short_name, std::string* out) {
  const std::string a = argv[i];
  const std::string ln = std::string("--") + long_name;
  if (a.rfind(ln + "=", 0) == 0) {
    *out = a.substr(ln.size() + 1);
    return true;
  }
  if (a == ln || (short_name && a == std::string("-") + short_name)) {
    if (i + 1 >= argc) usage(argv[0], ("option " + a + " needs an argument").c_str());
    *out = argv[++i];
    return true;
  }
  if (short_name && a.rfind(std::string("-") + short_name, 0) == 0 && a.size() > 2 && a[1] != '-') {
    *out = a.substr(2);
    return true;
  }
  return false;
}

Args parse(int argc, char** argv) {
  Args a;
  bool have_dim = false;
  for (int i = 1; i < argc; ++i) {
    std::string v, bad;
    if (!std::strcmp(argv[i], "--envmap-sample")) a.envmap_sample = true;
    else if (!std::strcmp(argv[i], "--light-spheres")) a.light_spheres = true;
    else if (!std::strcmp(argv[i], "--panorama")) a.panorama = true;
    else if (take_value(argc, argv, i, "hdr-out", nullptr, &v)) {
      if (v.empty()) usage(argv[0], "invalid value for --hdr-out, expected a file name");
      a.hdr_out = v;
    }
    else if (take_value(argc, argv, i, "exposure", nullptr, &v)) {
      char* end = nullptr;
      a.display.exposure = std::strtod(v.c_str(), &end);
      if (end == v.c_str() || *end || !(a.display.exposure >= 0.0) || !std::isfinite(a.display.exposure))
        usage(argv[0], "invalid value for --exposure, must be finite and >= 0");
    } else if (take_value(argc, argv, i, "tone", nullptr, &v)) {
      if (v == "none") a.display.tone = PTX_TONE_NONE;
      else if (v == "reinhard") a.display.tone = PTX_TONE_REINHARD;
      else if (v == "aces") a.display.tone = PTX_TONE_ACES;
      else usage(argv[0], "invalid value for --tone, expected none, reinhard or aces");
    } else if (take_value(argc, argv, i, "transfer", nullptr, &v)) {
      if (v == "reference") a.display.transfer = PTX_TRANSFER_REFERENCE;
      else if (v == "linear") a.display.transfer = PTX_TRANSFER_LINEAR;
      else if (v == "srgb") a.display.transfer = PTX_TRANSFER_SRGB;
      else usage(argv[0], "invalid value for --transfer, expected reference, linear or srgb");
    }
    else if (take_value(argc, argv, i, "sphere-lamp", nullptr, &v)) {
      char tail = 0;
      double* l = a.sphere_lamp;
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf,%lf,%lf%c", &l[0], &l[1], &l[2], &l[3], &l[4], &tail) != 5)
        usage(argv[0], "invalid value for --sphere-lamp, expected X,Y,Z,R,EMIT");
      for (int k = 0; k < 5; ++k)
        if (!std::isfinite(l[k])) usage(argv[0], "invalid value for --sphere-lamp, every number must be finite");
      if (!(l[3] > 0.0) || !(l[4] > 0.0)) usage(argv[0], "invalid value for --sphere-lamp, R and EMIT must be > 0");
      a.have_sphere_lamp = true;
    }
    else if (image_flag(argv[i], &a.images, &bad)) {
      if (!bad.empty()) usage(argv[0], bad.c_str());
    } else if (take_value(argc, argv, i, "dimension", "d", &v)) {
      if (std::sscanf(v.c_str(), "%d,%d", &a.width, &a.height) != 2) usage(argv[0], "invalid value for --dimension, expected WIDTH,HEIGHT");
      have_dim = true;
    } else if (take_value(argc, argv, i, "samples-per-pixel", nullptr, &v)) a.samples_per_pixel = std::atoi(v.c_str());
    else if (take_value(argc, argv, i, "output", "o", &v)) a.output = v;
    else if (take_value(argc, argv, i, "max-ray-bounces", nullptr, &v)) a.max_bounces = std::atoi(v.c_str());
    else if (take_value(argc, argv, i, "scene", nullptr, &v)) a.scene = v;
    else if (take_value(argc, argv, i, "device", nullptr, &v)) a.device = std::atoi(v.c_str());
    else if (take_value(argc, argv, i, "gpus", nullptr, &v)) a.gpus = std::atoi(v.c_str());
    else if (take_value(argc, argv, i, "triangles", nullptr, &v)) a.ganesha_triangles = std::atoi(v.c_str());
    else if (take_value(argc, argv, i, "ceiling-emit", nullptr, &v)) a.ceiling_emit = std::atof(v.c_str());
    else if (take_value(argc, argv, i, "ganesha-ply", nullptr, &v)) a.ganesha_ply = v;
    else if (take_value(argc, argv, i, "progressive", nullptr, &v)) {
      a.progressive = std::atoi(v.c_str());
      if (a.progressive < 1) usage(argv[0], "invalid value for --progressive, must be >= 1");
    } else if (take_value(argc, argv, i, "target-error", nullptr, &v)) {
      a.target_error = std::atof(v.c_str());
      if (!(a.target_error > 0.0)) usage(argv[0], "invalid value for --target-error, must be > 0");
    } else if (take_value(argc, argv, i, "adaptive", nullptr, &v)) {
      a.adaptive = std::atof(v.c_str());
      if (!(a.adaptive >= 0.0)) usage(argv[0], "invalid value for --adaptive, must be >= 0");
    } else if (take_value(argc, argv, i, "min-passes", nullptr, &v)) {
      a.min_passes = std::atoi(v.c_str());
      if (a.min_passes < 2) usage(argv[0], "invalid value for --min-passes, must be >= 2");
    } else if (take_value(argc, argv, i, "lighting", nullptr, &v)) {
      if (v == "reference") a.lighting = PTX_LIGHTING_REFERENCE;
      else if (v == "path-order") a.lighting = PTX_LIGHTING_PATH_ORDER;
      else if (v == "sampled") a.lighting = PTX_LIGHTING_SAMPLED;
      else usage(argv[0], "invalid value for --lighting, expected reference, path-order or sampled");
    } else if (take_value(argc, argv, i, "lamp", nullptr, &v)) {
      char tail = 0;
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &a.lamp_half_side, &a.lamp_y, &a.lamp_emit, &tail) != 3)
        usage(argv[0], "invalid value for --lamp, expected HALF_SIDE,Y,EMIT");
      if (!(a.lamp_half_side > 0.0) || !(a.lamp_emit > 0.0) || !(a.lamp_y == a.lamp_y)) usage(argv[0], "invalid value for --lamp, HALF_SIDE and EMIT must be > 0");
      a.have_lamp = true;
    }
    else if (!std::strcmp(argv[i], "--denoise")) a.denoise = 5; // ptx_denoise_defaults' levels
    else if (!std::strncmp(argv[i], "--denoise=", 10)) {
      char* end = nullptr;
      const long l = std::strtol(argv[i] + 10, &end, 10);
      if (end == argv[i] + 10 || *end || l < 0 || l > 8) usage(argv[0], "invalid value for --denoise, LEVELS must be in 0..8");
      a.denoise = (int)l;
    } else if (take_value(argc, argv, i, "aov", nullptr, &v)) {
      if (v.empty()) usage(argv[0], "invalid value for --aov, expected a file name prefix");
      a.aov = v;
    }
    else if (take_value(argc, argv, i, "filter", nullptr, &v)) {
      char tail = 0;
      int order = 0, radius = 0;
      if (std::sscanf(v.c_str(), "%d,%d%c", &order, &radius, &tail) != 2) usage(argv[0], "invalid value for --filter, expected ORDER,RADIUS");
      a.film.order = order;
      a.film.pixel_radius = radius;
      a.have_filter = true;
    } else if (!std::strcmp(argv[i], "--filter-renormalise")) {
      a.film.flags |= PTX_FILM_RENORMALISE;
      a.have_filter = true;
    }
    else if (take_value(argc, argv, i, "lens-radius", nullptr, &v)) {
      char* end = nullptr;
      a.lens_radius = std::strtod(v.c_str(), &end);
      if (end == v.c_str() || *end || !(a.lens_radius >= 0.0) || !std::isfinite(a.lens_radius)) usage(argv[0], "invalid value for --lens-radius, must be >= 0");
    } else if (take_value(argc, argv, i, "focus-distance", nullptr, &v)) {
      char* end = nullptr;
      a.focus_distance = std::strtod(v.c_str(), &end);
      if (end == v.c_str() || *end || !(a.focus_distance > 0.0) || !std::isfinite(a.focus_distance)) usage(argv[0], "invalid value for --focus-distance, must be > 0");
    }
    else if (take_value(argc, argv, i, "camera-eye", nullptr, &v)) {
      char tail = 0;
      double* c = a.camera_eye;
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &c[0], &c[1], &c[2], &tail) != 3 || !std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
        usage(argv[0], "invalid value for --camera-eye, expected X,Y,Z");
      a.have_eye = true;
    } else if (take_value(argc, argv, i, "camera-target", nullptr, &v)) {
      char tail = 0;
      double* c = a.camera_target;
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &c[0], &c[1], &c[2], &tail) != 3 || !std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
        usage(argv[0], "invalid value for --camera-target, expected X,Y,Z");
      a.have_target = true;
    } else if (take_value(argc, argv, i, "camera-fov", nullptr, &v)) {
      char* end = nullptr;
      a.camera_fov = std::strtod(v.c_str(), &end);
      if (end == v.c_str() || *end || !(a.camera_fov > 0.0) || !(a.camera_fov < 180.0)) usage(argv[0], "invalid value for --camera-fov, must be in (0, 180)");
    } else if (take_value(argc, argv, i, "turntable", nullptr, &v)) {
      char* end = nullptr;
      const long n = std::strtol(v.c_str(), &end, 10);
      if (end == v.c_str() || *end || n < 1 || n > 999) usage(argv[0], "invalid value for --turntable, must be in 1..999");
      a.turntable = (int)n;
    } else if (take_value(argc, argv, i, "turntable-arc", nullptr, &v)) {
      char* end = nullptr;
      a.turntable_arc = std::strtod(v.c_str(), &end);
      if (end == v.c_str() || *end || !(a.turntable_arc > 0.0) || !(a.turntable_arc <= 360.0)) usage(argv[0], "invalid value for --turntable-arc, must be in (0, 360]");
      a.have_arc = true;
    } else if (take_value(argc, argv, i, "shutter", nullptr, &v)) {
      char* end = nullptr;
      a.shutter = std::strtod(v.c_str(), &end);
      if (end == v.c_str() || *end || !(a.shutter > 0.0) || !(a.shutter <= 1.0)) usage(argv[0], "invalid value for --shutter, must be in (0, 1]");
    } else if (take_value(argc, argv, i, "shutter-eye", nullptr, &v)) {
      char tail = 0;
      double* c = a.shutter_eye;
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &c[0], &c[1], &c[2], &tail) != 3 || !std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
        usage(argv[0], "invalid value for --shutter-eye, expected X,Y,Z");
      a.have_shutter_eye = true;
    } else if (take_value(argc, argv, i, "shutter-target", nullptr, &v)) {
      char tail = 0;
      double* c = a.shutter_target;
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &c[0], &c[1], &c[2], &tail) != 3 || !std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
        usage(argv[0], "invalid value for --shutter-target, expected X,Y,Z");
      a.have_shutter_target = true;
    } else if (!std::strcmp(argv[i], "--temporal")) {
      a.temporal = 64.0; // ptx_temporal_defaults' max_history_passes
    } else if (!std::strncmp(argv[i], "--temporal=", 11)) {
      char* end = nullptr;
      a.temporal = std::strtod(argv[i] + 11, &end);
      if (end == argv[i] + 11 || *end || !(a.temporal >= 0.0) || !std::isfinite(a.temporal)) usage(argv[0], "invalid value for --temporal, CAP must be >= 0");
    }
    else if (!std::strcmp(argv[i], "-ganesha-ply") && i + 1 < argc) a.ganesha_ply = argv[++i]; // Stdlib.Arg spelling
    else if (!std::strcmp(argv[i], "--no-progress")) a.no_progress = true;
    else if (!std::strcmp(argv[i], "--no-simd")) a.no_simd = true;
    else if (!std::strcmp(argv[i], "--help") || !std::strcmp(argv[i], "-h")) usage(argv[0], nullptr);
    else usage(argv[0], (std::string("unknown option ") + argv[i]).c_str());
  }
  if (!have_dim) usage(argv[0], "required option --dimension is missing");
  // checked here, before anything is allocated from them (Cmdliner would also refuse a malformed WIDTH,HEIGHT)
  if (a.width <= 0 || a.height <= 0) usage(argv[0], "invalid value for --dimension, WIDTH and HEIGHT must be positive");
  if ((long long)a.width * a.height > (1ll << 31)) usage(argv[0], "invalid value for --dimension, image too large");
  if (a.samples_per_pixel < 1) usage(argv[0], "invalid value for --samples-per-pixel, must be >= 1");
  if (a.max_bounces < 0) usage(argv[0], "invalid value for --max-ray-bounces, must be >= 0");
  if (a.gpus < 1) usage(argv[0], "invalid value for --gpus, must be >= 1");
  const bool adaptive = a.adaptive >= 0.0;
  if (adaptive && a.target_error > 0.0) usage(argv[0], "--adaptive cannot be combined with --target-error");
  if (adaptive && a.gpus > 1) usage(argv[0], "--adaptive renders on one GPU (--gpus=1)");
  if (a.min_passes && !adaptive) usage(argv[0], "--min-passes requires --adaptive");
  if (a.target_error > 0.0 && !a.progressive) usage(argv[0], "--target-error requires --progressive");
  if (a.progressive && a.gpus > 1) usage(argv[0], "--progressive renders on one GPU (--gpus=1)");
  if (a.have_lamp && a.scene != "cornell") usage(argv[0], "--lamp requires --scene=cornell");
  if (!a.aov.empty() && a.denoise < 0) usage(argv[0], "--aov requires --denoise");
  if (a.denoise >= 0 && adaptive) usage(argv[0], "--denoise cannot be combined with --adaptive");
  if (a.denoise >= 0 && a.gpus > 1) usage(argv[0], "--denoise renders on one GPU (--gpus=1)");
  if (a.denoise >= 0 && a.samples_per_pixel < 2) usage(argv[0], "--denoise requires --samples-per-pixel >= 2");
  if (a.denoise >= 0 && a.progressive == 1) usage(argv[0], "--denoise requires --progressive >= 2");
  {
    const std::string bad = image_flags_check(a.images, a.scene != "cornell");
    if (!bad.empty()) usage(argv[0], bad.c_str());
  }
  if (a.focus_distance > 0.0 && !(a.lens_radius > 0.0)) usage(argv[0], "--focus-distance requires --lens-radius > 0");
  if (a.have_eye != a.have_target) usage(argv[0], "--camera-eye and --camera-target are given together");
  if (a.have_eye && a.camera_eye[0] == a.camera_target[0] && a.camera_eye[1] == a.camera_target[1] && a.camera_eye[2] == a.camera_target[2])
    usage(argv[0], "--camera-eye and --camera-target must differ");
  if (a.camera_fov > 0.0 && !a.have_eye && a.turntable == 0) usage(argv[0], "--camera-fov requires --camera-eye and --camera-target, or --turntable");
  if (a.have_arc && a.turntable == 0) usage(argv[0], "--turntable-arc requires --turntable");
  if (a.shutter > 0.0 && a.turntable == 0) usage(argv[0], "--shutter requires --turntable (a single frame takes --shutter-eye)");
  if (a.have_shutter_eye && (!a.have_eye || a.turntable > 0)) usage(argv[0], "--shutter-eye requires --camera-eye and --camera-target, without --turntable");
  if (a.have_shutter_target && !a.have_shutter_eye) usage(argv[0], "--shutter-target requires --shutter-eye");
  if (a.have_shutter_eye) {
    const double* t = a.have_shutter_target ? a.shutter_target : a.camera_target;
    if (a.shutter_eye[0] == t[0] && a.shutter_eye[1] == t[1] && a.shutter_eye[2] == t[2]) usage(argv[0], "--shutter-eye and its target must differ");
  }
  if (a.temporal >= 0.0) {
    if (a.turntable == 0) usage(argv[0], "--temporal requires --turntable");
    if (a.samples_per_pixel < 2) usage(argv[0], "--temporal requires --samples-per-pixel >= 2 (one frame's passes)");
    if (adaptive || a.progressive) usage(argv[0], "--temporal cannot be combined with --adaptive or --progressive");
    if (a.gpus > 1) usage(argv[0], "--temporal renders on one GPU (--gpus=1)");
    if (a.lens_radius > 0.0) usage(argv[0], "--temporal needs a pinhole: it cannot be combined with --lens-radius");
    if (!a.aov.empty()) usage(argv[0], "--aov cannot be combined with --temporal");
  }
  if (a.panorama && a.lens_radius > 0.0) usage(argv[0], "--panorama has no lens: it cannot be combined with --lens-radius");
  if (a.panorama && a.temporal >= 0.0) usage(argv[0], "--temporal needs a pinhole: it cannot be combined with --panorama");
  if (a.envmap_sample && a.images.envmap.empty()) usage(argv[0], "--envmap-sample requires --envmap");
  if (a.envmap_sample && a.lighting != PTX_LIGHTING_SAMPLED) usage(argv[0], "--envmap-sample requires --lighting=sampled");
  if (a.have_sphere_lamp && a.scene != "shirley") usage(argv[0], "--sphere-lamp requires --scene=shirley");
  if (a.light_spheres && a.lighting != PTX_LIGHTING_SAMPLED) usage(argv[0], "--light-spheres requires --lighting=sampled");
  if (a.have_filter) { // the library's own check and message (host only: no device is touched)
    double w[2 * PTX_FILM_MAX_RADIUS + 1];
    if (ptx_film_weights(&a.film, w, nullptr) != 0) usage(argv[0], ptx_last_error());
  }
  return a;
}

double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

struct Progress {
  long long total = 0, done = 0;
  double t0 = 0, last = 0;
};
void on_progress(void* user, int64_t pixels) { // the ASCII bar of render_command.ml:86-103
  Progress* p = (Progress*)user;
  p->done += pixels;
  const double t = now_ms();
  if (t - p->last < 200.0 && p->done < p->total) return; // min_interval 0.2 s
  p->last = t;
  const int width = 40, fill = (int)(width * (double)p->done / (double)p->total);
  std::fprintf(stderr, "\r%6.1fs [", (t - p->t0) * 1e-3);
  for (int i = 0; i < width; ++i) std::fputc(i < fill ? '#' : '-', stderr);
  std::fprintf(stderr, "] %3.0f%%    ", 100.0 * (double)p->done / (double)p->total);
  if (p->done >= p->total) std::fputc('\n', stderr);
}

// the PNG of an f64 image under the display: its RGB8 bytes by the library's rule on the host (ptx_display_apply)
int write_display_png(const char* path, int width, int height, const double* rgb, const ptx_display_params& display) {
  std::vector<uint8_t> codes((size_t)width * height * 3);
  if (ptx_display_apply(&display, (int64_t)width * height, rgb, codes.data()) != 0) return -1;
  return pth_write_png8(path, width, height, codes.data());
}

struct Updates { // --progressive: the PNG rewritten after every update, one line per update on stdout
  const char* output;
  int width, height;
  const ptx_display_params* display;
  bool write_failed = false;
};
int32_t on_update(void* user, int32_t passes_done, double rel_err, const double* rgb, const double*) {
  Updates* u = (Updates*)user;
  std::printf("#passes = %d, error = %.6g\n", passes_done, rel_err);
  std::fflush(stdout);
  if (write_display_png(u->output, u->width, u->height, rgb, *u->display) != 0) {
    u->write_failed = true;
    return 1;
  }
  return 0;
}
// the same for updates that arrive as RGB8 display pixels (ptx_render_progressive_display)
int32_t on_update_display(void* user, int32_t passes_done, double rel_err, const void* pixels, const double*) {
  Updates* u = (Updates*)user;
  std::printf("#passes = %d, error = %.6g\n", passes_done, rel_err);
  std::fflush(stdout);
  if (pth_write_png8(u->output, u->width, u->height, (const uint8_t*)pixels) != 0) {
    u->write_failed = true;
    return 1;
  }
  return 0;
}

// --adaptive: the PNG rewritten after every round, one line per round on stdout
int32_t on_round(void* user, int32_t round, int32_t passes_done, int64_t active_next, int64_t samples, double rel_err,
                 const double* rgb, const double*, const int32_t*) {
  Updates* u = (Updates*)user;
  std::printf("#round = %d, passes = %d, active = %lld, samples = %lld, error = %.6g\n", round, passes_done, (long long)active_next,
              (long long)samples, rel_err);
  std::fflush(stdout);
  if (write_display_png(u->output, u->width, u->height, rgb, *u->display) != 0) {
    u->write_failed = true;
    return 1;
  }
  return 0;
}

// --aov: the feature means (8 doubles per pixel: albedo, normal, depth, hits) as three PNGs
int write_aovs(const std::string& prefix, int width, int height, const std::vector<double>& feat) {
  const size_t npix = (size_t)width * height;
  std::vector<double> img(npix * 3);
  for (size_t p = 0; p < npix; ++p)
    for (int c = 0; c < 3; ++c) img[3 * p + c] = feat[8 * p + c];
  if (pth_write_png((prefix + "-albedo.png").c_str(), width, height, img.data()) != 0) return -1;
  for (size_t p = 0; p < npix; ++p)
    for (int c = 0; c < 3; ++c) img[3 * p + c] = feat[8 * p + 3 + c] * 0.5 + 0.5;
  if (pth_write_png((prefix + "-normal.png").c_str(), width, height, img.data()) != 0) return -1;
  double zmax = 0.0;
  for (size_t p = 0; p < npix; ++p) zmax = feat[8 * p + 6] > zmax ? feat[8 * p + 6] : zmax;
  for (size_t p = 0; p < npix; ++p)
    for (int c = 0; c < 3; ++c) img[3 * p + c] = zmax > 0.0 ? feat[8 * p + 6] / zmax : 0.0;
  return pth_write_png((prefix + "-depth.png").c_str(), width, height, img.data()) != 0 ? -1 : 0;
}

// The camera of frame `frame`: --camera-eye / --camera-target / --camera-fov where given, else the scene's own; a turntable turns the
// eye about the axis through the target along the scene camera's up vector (Rodrigues).  closing: the pose a single frame's shutter
// closes at (--shutter-eye / --shutter-target) instead.
struct CameraPose {
  double origin[3], rotation[9];
  ptx_camera view;
};
int camera_of_frame(pth_scene* hs, const Args& a, int frame, bool closing, CameraPose* out) {
  double eye[3], target[3], up[3], fov = 0.0, look_at[16];
  if (pth_scene_camera(hs, eye, target, up, &fov, look_at) != 0) {
    std::fprintf(stderr, "the scene records no camera to pose against\n");
    return -1;
  }
  if (a.have_eye) {
    std::memcpy(eye, a.camera_eye, sizeof eye);
    std::memcpy(target, a.camera_target, sizeof target);
  }
  if (closing) {
    std::memcpy(eye, a.shutter_eye, sizeof eye);
    if (a.have_shutter_target) std::memcpy(target, a.shutter_target, sizeof target);
  }
  if (a.camera_fov > 0.0) fov = a.camera_fov;
  if (a.turntable > 0) {
    const double len = std::sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
    const double k[3] = {up[0] / len, up[1] / len, up[2] / len};
    // (the full circle keeps its own expression: the default arc gives the angles it always gave)
    const double arc = a.turntable_arc == 360.0 ? 2.0 * 3.14159265358979323846 : a.turntable_arc * (3.14159265358979323846 / 180.0);
    const double th = arc * (double)frame / (double)a.turntable, c = std::cos(th), s = std::sin(th);
    const double v[3] = {eye[0] - target[0], eye[1] - target[1], eye[2] - target[2]};
    const double kxv[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
    const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
    for (int i = 0; i < 3; ++i) eye[i] = target[i] + (v[i] * c + kxv[i] * s + k[i] * kv * (1.0 - c));
  }
  pth_camera_pose_look_at(look_at, eye, target, up, (double)a.width / (double)a.height, fov, out->origin, out->rotation, &out->view);
  return 0;
}

// poses the scene for frame `frame` (ptx_scene_set_camera_pose) and, with --shutter or --shutter-eye, opens its shutter
// (ptx_scene_set_camera_shutter): towards frame + 1's pose by the fraction --shutter, or all the way to --shutter-eye's
int pose_camera(ptx_scene* scene, pth_scene* hs, const Args& a, int frame) {
  CameraPose cp;
  if (camera_of_frame(hs, a, frame, false, &cp) != 0) return -1;
  if (ptx_scene_set_camera_pose(scene, cp.origin, cp.rotation, &cp.view) != 0) {
    std::fprintf(stderr, "ptx_scene_set_camera_pose: %s\n", ptx_last_error());
    return -1;
  }
  if (!(a.shutter > 0.0) && !a.have_shutter_eye) return 0;
  CameraPose next;
  if (camera_of_frame(hs, a, frame + 1, a.have_shutter_eye, &next) != 0) return -1;
  double translation[3], axis[3], angle = 0.0;
  pth_camera_shutter_between(cp.origin, cp.rotation, next.origin, next.rotation, translation, axis, &angle);
  if (a.shutter > 0.0) {
    for (int i = 0; i < 3; ++i) translation[i] = translation[i] * a.shutter;
    angle = angle * a.shutter;
  }
  if (ptx_scene_set_camera_shutter(scene, translation, axis, angle) != 0) {
    std::fprintf(stderr, "ptx_scene_set_camera_shutter: %s\n", ptx_last_error());
    return -1;
  }
  return 0;
}

// out.png -> out-007.png
std::string frame_name(const std::string& output, int frame) {
  char tag[16];
  std::snprintf(tag, sizeof tag, "-%03d", frame);
  const size_t dot = output.rfind('.'), slash = output.rfind('/');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return output + tag;
  return output.substr(0, dot) + tag + output.substr(dot);
}

}  // namespace

int main(int argc, char** argv) {
  const Args a = parse(argc, argv);
  if (ptx_display_check(&a.display) != 0) usage(argv[0], ptx_last_error()); // e.g. --tone without --transfer=linear|srgb
  pth_scene* hs = nullptr;
  if (a.scene == "shirley")
    hs = a.have_sphere_lamp ? pth_scene_shirley_lamp(a.width, a.height, a.no_simd ? 1 : 0, 42, a.sphere_lamp[0], a.sphere_lamp[1], a.sphere_lamp[2],
                                                     a.sphere_lamp[3], a.sphere_lamp[4])
                            : pth_scene_shirley(a.width, a.height, a.no_simd ? 1 : 0, 42); // Random.init 42
  else if (a.scene == "cornell")
    hs = a.have_lamp ? pth_scene_cornell_lamp(a.width, a.height, a.ceiling_emit, a.lamp_half_side, a.lamp_y, a.lamp_emit)
                     : pth_scene_cornell(a.width, a.height, a.ceiling_emit);
  else if (a.scene == "ganesha")
    hs = a.ganesha_ply.empty() ? pth_scene_ganesha_like(a.width, a.height, a.ganesha_triangles, 7) : pth_scene_ganesha_ply(a.ganesha_ply.c_str(), a.width, a.height);
  else usage(argv[0], "unknown --scene");
  if (!hs) {
    std::fprintf(stderr, "%s: cannot build scene %s: %s\n", argv[0], a.scene.c_str(), pth_last_error());
    return 1;
  }
  const ptx_scene_desc* d = pth_scene_desc(hs);
  std::printf("dim = %d x %d;\n", a.width, a.height);
  if (d->n_spheres) std::printf("#spheres = %d\n", d->n_spheres);
  if (d->n_triangles) std::printf("#triangles = %d\n", d->n_triangles);
  ptx_scene* scene = ptx_scene_create(d, a.device);
  if (!scene) {
    std::fprintf(stderr, "ptx_scene_create: %s\n", ptx_last_error());
    return 1;
  }
  if (a.light_spheres && ptx_scene_set_sphere_light_sampling(scene, 1) != 0) {
    std::fprintf(stderr, "ptx_scene_set_sphere_light_sampling: %s\n", ptx_last_error());
    return 1;
  }
  // (with --envmap-sample the mode is set behind the environment and its sampling, which it may need)
  if (!a.envmap_sample && a.lighting != PTX_LIGHTING_REFERENCE && ptx_scene_set_lighting(scene, a.lighting) != 0) {
    std::fprintf(stderr, "ptx_scene_set_lighting: %s\n", ptx_last_error());
    return 1;
  }
  // the thin lens: without --focus-distance it focuses on the camera's look-at target
  if (a.lens_radius > 0.0 && ptx_scene_set_lens(scene, a.lens_radius, a.focus_distance > 0.0 ? a.focus_distance : pth_scene_focus_distance(hs)) != 0) {
    std::fprintf(stderr, "ptx_scene_set_lens: %s\n", ptx_last_error());
    return 1;
  }
  if (a.panorama && ptx_scene_set_camera_projection(scene, PTX_PROJECTION_LATLONG) != 0) {
    std::fprintf(stderr, "ptx_scene_set_camera_projection: %s\n", ptx_last_error());
    return 1;
  }
  if (a.have_filter && ptx_scene_set_film(scene, &a.film) != 0) {
    std::fprintf(stderr, "ptx_scene_set_film: %s\n", ptx_last_error());
    return 1;
  }
  {
    std::string err;
    if (apply_image_flags(scene, d, a.images, &err) != 0) {
      std::fprintf(stderr, "%s: %s\n", argv[0], err.c_str());
      return 1;
    }
  }
  if (a.envmap_sample) {
    if (ptx_scene_set_environment_sampling(scene, 1) != 0) {
      std::fprintf(stderr, "ptx_scene_set_environment_sampling: %s\n", ptx_last_error());
      return 1;
    }
    if (ptx_scene_set_lighting(scene, a.lighting) != 0) {
      std::fprintf(stderr, "ptx_scene_set_lighting: %s\n", ptx_last_error());
      return 1;
    }
  }
  ptx_stats st;
  ptx_scene_stats(scene, &st);
  std::printf("tree depth = %d\n", st.tree_depth);
  std::printf("build time = %.3f ms\n", st.build_ms);
  { // leaf lengths = ((size n) (count m)) ..., like Leaf_lengths (main.ml:233-248,265-267)
    std::vector<int32_t> info((size_t)st.tree_nodes * 4);
    ptx_scene_tree(scene, nullptr, info.data(), st.tree_nodes, nullptr, 0);
    std::map<int, int> hist;
    for (int i = 0; i < st.tree_nodes; ++i)
      if (info[(size_t)4 * i]) hist[info[(size_t)4 * i + 3]]++;
    std::printf("leaf lengths =\n(");
    bool first = true;
    for (auto& kv : hist) {
      std::printf("%s((size %d) (count %d))", first ? "" : " ", kv.first, kv.second);
      first = false;
    }
    std::printf(")\n");
    std::fflush(stdout);
  }
  const bool posed = a.have_eye || a.turntable > 0;
  for (int frame = 0; frame < (a.turntable > 0 ? a.turntable : 1); ++frame) {
  const std::string output = a.turntable > 0 ? frame_name(a.output, frame) : a.output;
  if (posed && pose_camera(scene, hs, a, frame) != 0) return 1;
  ptx_render_params p;
  std::memset(&p, 0, sizeof p);
  p.width = a.width; p.height = a.height; p.samples_per_pixel = a.samples_per_pixel; p.max_bounces = a.max_bounces;
  p.n_gpus = a.gpus;
  /* the display route: the RGB8 bytes come from the device.  The drivers below that keep their f64 image (and --aov's feature image,
   * --hdr-out's binary32 one, which need it) convert it on the host by the same rule. */
  const bool on_device = a.temporal < 0.0 && a.adaptive < 0.0 && a.turntable == 0 && a.aov.empty() && a.hdr_out.empty();
  std::vector<double> rgb(on_device ? 0 : (size_t)a.width * a.height * 3);
  std::vector<uint8_t> rgb8(on_device ? (size_t)a.width * a.height * 3 : 0);
  Progress prog;
  prog.total = (long long)a.width * a.height;
  prog.t0 = prog.last = now_ms();
  const double t0 = now_ms();
  /* the image lives until the PNG is written, like the reference's Bimage (render_command.ml:64-70): pin it, so the frame comes
   * back with one DMA (optional: a failure only means the staged copy) */
  if (on_device) (void)ptx_image_pin_bytes(scene, rgb8.data(), (int64_t)rgb8.size());
  else (void)ptx_image_pin(scene, rgb.data(), (int64_t)rgb.size());
  Updates upd{output.c_str(), a.width, a.height, &a.display};
  int rc;
  const bool adaptive = a.adaptive >= 0.0;
  long long history_pixels = 0;
  if (a.temporal >= 0.0) {
    // one frame's passes are a slice of the sequence's N = S * min(T, 16): frame f renders slice f mod min(T, 16)
    const int slices = a.turntable < 16 ? a.turntable : 16, slice = frame % slices;
    p.samples_per_pixel = a.samples_per_pixel * slices;
    ptx_temporal_params tp;
    ptx_temporal_defaults(&tp);
    tp.max_history_passes = a.temporal;
    ptx_denoise_params dn;
    ptx_denoise_defaults(&dn);
    if (a.denoise >= 0) dn.levels = a.denoise;
    int64_t took = 0;
    rc = ptx_render_temporal(scene, &p, &tp, a.denoise >= 0 ? &dn : nullptr, slice * a.samples_per_pixel, a.samples_per_pixel, rgb.data(), nullptr,
                             nullptr, &took, &st);
    history_pixels = (long long)took;
  } else if (adaptive) {
    ptx_adaptive_params ap;
    std::memset(&ap, 0, sizeof ap);
    ap.min_passes = a.min_passes ? a.min_passes : 8;
    ap.passes_per_round = a.progressive ? a.progressive : 8;
    ap.target_rel_err = a.adaptive;
    ap.radiance_floor = 1e-3;
    rc = ptx_render_adaptive(scene, &p, &ap, rgb.data(), nullptr, nullptr, &st, on_round, &upd);
  } else if (a.denoise >= 0) {
    ptx_progressive_params pp;
    std::memset(&pp, 0, sizeof pp);
    pp.passes_per_update = a.progressive ? a.progressive : a.samples_per_pixel; // without --progressive: one update, after the last pass
    pp.want_error = 1;
    pp.target_rel_err = a.target_error;
    ptx_denoise_params dn;
    ptx_denoise_defaults(&dn);
    dn.levels = a.denoise;
    std::vector<double> feat(a.aov.empty() ? 0 : (size_t)a.width * a.height * PTX_FEATURE_DOUBLES);
    int32_t passes_done = 0;
    if (on_device) rc = ptx_render_progressive_display(scene, &p, &pp, &dn, &a.display, rgb8.data(), nullptr, &passes_done, &st, on_update_display, &upd);
    else rc = ptx_render_denoised(scene, &p, &pp, &dn, rgb.data(), nullptr, feat.empty() ? nullptr : feat.data(), &passes_done, &st, on_update,
                             &upd);
    if (rc == 0 && !feat.empty() && write_aovs(a.aov, a.width, a.height, feat) != 0) {
      std::fprintf(stderr, "cannot write %s-*.png\n", a.aov.c_str());
      return 1;
    }
  } else if (a.progressive) {
    ptx_progressive_params pp;
    std::memset(&pp, 0, sizeof pp);
    pp.passes_per_update = a.progressive;
    pp.want_error = 1;
    pp.target_rel_err = a.target_error;
    int32_t passes_done = 0;
    if (on_device) rc = ptx_render_progressive_display(scene, &p, &pp, nullptr, &a.display, rgb8.data(), nullptr, &passes_done, &st, on_update_display, &upd);
    else rc = ptx_render_progressive(scene, &p, &pp, rgb.data(), nullptr, &passes_done, &st, on_update, &upd);
  } else {
    if (on_device) rc = ptx_render_display(scene, &p, &a.display, rgb8.data(), &st, a.no_progress ? nullptr : on_progress, &prog);
    else rc = ptx_render(scene, &p, rgb.data(), &st, a.no_progress ? nullptr : on_progress, &prog);
  }
  (void)ptx_image_unpin(scene);
  const double elapsed = now_ms() - t0;
  if (rc != 0) {
    std::fprintf(stderr, "%s: %s\n", a.temporal >= 0.0 ? "ptx_render_temporal" : adaptive ? "ptx_render_adaptive" : a.denoise >= 0 ? "ptx_render_denoised" : a.progressive ? "ptx_render_progressive" : "ptx_render",
                 ptx_last_error());
    return (rc == -3 /* PTX_ERR_STATE */ && a.temporal >= 0.0 && a.shutter > 0.0) ? 124 : 1; // (a shutter under --temporal: the library's refusal)
  }
  if (upd.write_failed || (on_device ? pth_write_png8(output.c_str(), a.width, a.height, rgb8.data())
                                     : write_display_png(output.c_str(), a.width, a.height, rgb.data(), a.display)) != 0) {
    std::fprintf(stderr, "cannot write %s\n", output.c_str());
    return 1;
  }
  if (!a.hdr_out.empty()) { // the image is sqrt(filmed radiance): its RGB32F / linear display at exposure 1 -- the square, in binary32
    const ptx_display_params hdr_display{PTX_PIXEL_RGB32F, PTX_TRANSFER_LINEAR, PTX_TONE_NONE, 0, 1.0, {0, 0, 0, 0}};
    std::vector<float> linear32(rgb.size());
    if (ptx_display_apply(&hdr_display, (int64_t)a.width * a.height, rgb.data(), linear32.data()) != 0) {
      std::fprintf(stderr, "ptx_display_apply: %s\n", ptx_last_error());
      return 1;
    }
    const std::vector<double> linear(linear32.begin(), linear32.end()); // (exact: the writer's rounding to binary32 gives them back)
    const std::string hdr = a.turntable > 0 ? frame_name(a.hdr_out, frame) : a.hdr_out;
    if (pth_pfm_write(hdr.c_str(), a.width, a.height, linear.data()) != 0) {
      std::fprintf(stderr, "cannot write %s: %s\n", hdr.c_str(), pth_image_error());
      return 1;
    }
  }
  if (a.temporal >= 0.0) std::printf("frame %d -> %s, history = %lld pixels\n", frame, output.c_str(), history_pixels);
  else if (a.turntable > 0) std::printf("frame %d -> %s\n", frame, output.c_str());
  std::printf("rendered in: %.3f ms\n", elapsed);
  std::printf("throughput: %.3f Msamples/s\n", (double)st.samples / elapsed * 1e-3);
  } // (frames)
  ptx_scene_destroy(scene);
  pth_scene_free(hs);
  return 0;
}
