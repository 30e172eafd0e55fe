/* host.h -- C interface of libpt_host.so: the host-side mirror of the reference's scene executables and
 * Render_command (the parts of the reference that sit ABOVE the integrator boundary). */
#ifndef PT_HOST_H
#define PT_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/ptx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pth_scene pth_scene; /* owns the arrays a ptx_scene_desc points into */

const ptx_scene_desc* pth_scene_desc(pth_scene* s);
void pth_scene_free(pth_scene* s);
/* the distance from the eye to the look-at target of the scene's camera: the default focus distance of a thin lens (ptx_scene_set_lens) */
double pth_scene_focus_distance(const pth_scene* s);
/* the camera the scene was built for -- its geometry is in that camera's space: eye, target, up, the vertical field of view in degrees
 * and the Mat4.look_at rows (what pth_camera_pose_look_at takes as scene_look_at).  Any out pointer may be NULL; -1 for a scene that
 * records none. */
int32_t pth_scene_camera(const pth_scene* s, double eye_out[3], double target_out[3], double up_out[3], double* fov_deg_out, double look_at_out[16]);

/* Camera.create (path_tracer/src/camera.ml:58-83): view = the four fields Camera.ray reads;
 * look_at (optional) = Mat4.look_at rows, row-major 4x4 */
void pth_camera_create(const double eye[3], const double target[3], const double up[3], double aspect, double fov_deg,
                       ptx_camera* view_out, double look_at_out[16]);
/* A camera pose for ptx_scene_set_camera_pose: the camera (eye, target, up, aspect, fov_deg) seen from a scene that was built for
 * another camera, whose Mat4.look_at rows (pth_camera_create's look_at_out) are scene_look_at.  origin = Mat4.transform scene_look_at
 * eye; rotation = R_scene * R_new^T on the 3 x 3 row blocks, every sum left-associated; view = pth_camera_create's for the new
 * camera.  Any out pointer may be NULL.  The scene's own eye and target give the identity and the origin 0 within rounding only
 * (1e-15 and 1e-12 of the scene's units): "posed back home" is not "off". */
void pth_camera_pose_look_at(const double scene_look_at[16], const double eye[3], const double target[3], const double up[3], double aspect,
                             double fov_deg, double origin_out[3], double rotation_out[9], ptx_camera* view_out);

/* A camera shutter for ptx_scene_set_camera_shutter: the motion that takes pose 0 (origin0, rotation0 -- what
 * ptx_scene_set_camera_pose takes) to pose 1 while the shutter is open.  translation = origin1 - origin0; (axis, angle) = the turn
 * R1 * R0^T about a unit axis of the scene's space, angle in [0, pi]; no turn within rounding gives angle 0 and a zero axis.  Any out
 * pointer may be NULL. */
void pth_camera_shutter_between(const double origin0[3], const double rotation0[9], const double origin1[3], const double rotation1[9],
                                double translation_out[3], double axis_out[3], double* angle_out);

/* shirley_spheres/bin/main.ml (Random.init seed; the reference uses 42) */
pth_scene* pth_scene_shirley(int32_t width, int32_t height, int32_t no_simd, int64_t seed);
/* the same scene with a white Lambertian lamp sphere of radius r that emits (emit, emit, emit) at the WORLD point (x, y, z), moved to
 * camera space like every other sphere; it is appended after the random spheres, so everything before it is pth_scene_shirley's */
pth_scene* pth_scene_shirley_lamp(int32_t width, int32_t height, int32_t no_simd, int64_t seed, double x, double y, double z, double r,
                                  double emit);
/* cornell-box/bin/main.ml geometry + documented ceiling emitter */
pth_scene* pth_scene_cornell(int32_t width, int32_t height, double ceiling_emit);
/* pth_scene_cornell plus a lamp, two triangles appended after all others: a horizontal square of half side lamp_half_side centred at
 * (0.5, lamp_y, 0.5), vertices a = (-, y, -), b = (+, y, -), c = (+, y, +), d = (-, y, +), triangles (a, b, c) and (a, c, d), through
 * the camera like the rest; Lambertian, solid black, emit = lamp_emit (the reference lights this box from light_center =
 * (0.5, 0.82, 0.5)).  What ptx_scene_set_lighting(PTX_LIGHTING_SAMPLED) is for. */
pth_scene* pth_scene_cornell_lamp(int32_t width, int32_t height, double ceiling_emit, double lamp_half_side, double lamp_y,
                                  double lamp_emit);
/* ganesha/bin/main.ml camera / floor / material over a synthetic mesh of ~n_target triangles */
pth_scene* pth_scene_ganesha_like(int32_t width, int32_t height, int32_t n_target, uint64_t seed);

/* lights of the photon-mapped scenes (camera space): cornell-box/bin/main.ml:225-228, ganesha/bin/main.ml:267-282 */
int32_t pth_lights_cornell(int32_t width, int32_t height, ptx_light* out);      /* writes 1 */
int32_t pth_lights_ganesha(pth_scene* ganesha_scene, ptx_light* out /* 2 */); /* writes 2 */
/* save_image's gamma (progressive_photon_map.ml:398-410): avg = (sum / n) ** (1 / 2.2), in place into out */
void pth_ppm_gamma(const double* img_sum, int64_t count, int32_t n, double* out);

/* ---- PLY (ply_format/src/ply.ml) ---- */
typedef struct pth_ply pth_ply;
const char* pth_last_error(void);
/* Ply.of_bigstring over the file's bytes: NULL + pth_last_error() on failure */
pth_ply* pth_ply_load(const char* path);
void pth_ply_free(pth_ply* p);
/* number of rows of an element (fixed-width) or of a list PROPERTY (keyed by property name, ply.ml:234); -1 if absent */
int64_t pth_ply_count(const pth_ply* p, const char* key);
const double* pth_ply_floats(const pth_ply* p, const char* element, const char* property);  /* Column.Floats */
const int64_t* pth_ply_ints(const pth_ply* p, const char* element, const char* property);   /* Column.Ints */
const int64_t* pth_ply_rows(pth_ply* p, const char* list_property, const int32_t** lengths_out); /* Column.Rows, flattened */
/* ganesha/bin/main.ml with -ganesha-ply PATH: Mesh.create + floor + camera; sky background (extension) */
pth_scene* pth_scene_ganesha_ply(const char* path, int32_t width, int32_t height);
/* the synthetic stand-in mesh written as a PLY file with the real model's layout */
int32_t pth_write_ganesha_like_ply(const char* path, int32_t n_target, uint64_t seed);

/* ---- PFM images (pfm.cpp): the hosts' one image decoder, for --envmap and --ground-texture ----
 * "PF" / "Pf" (grey: r = g = b), either byte order by the sign of the scale, rows bottom to top = the image rule's v = 0 first
 * (include/ptx.h).  NULL + pth_image_error() on a file that cannot be opened or is malformed. */
typedef struct pth_image pth_image;
const char* pth_image_error(void);
pth_image* pth_pfm_load(const char* path);
pth_image* pth_pfm_parse(const unsigned char* bytes, size_t n);
/* the mirror of pth_pfm_load: a little-endian "PF" file of width * height * 3 values rounded to binary32, rows in the order given
 * (row 0 = v = 0), so a file written and loaded back is the binary32 rounding of `rgb`, row for row.  0, or -1 + pth_image_error()
 * (NULL argument, a size outside [1, PTX_IMAGE_MAX_SIZE], a value that is not finite in binary32, a file that cannot be written) */
int32_t pth_pfm_write(const char* path, int32_t width, int32_t height, const double* rgb);
void pth_image_free(pth_image* img);
int32_t pth_image_width(const pth_image* img);
int32_t pth_image_height(const pth_image* img);
int32_t pth_image_channels(const pth_image* img); /* of the file: 3 or 1 */
const double* pth_image_rgb(const pth_image* img); /* width * height * 3 */
/* the row-major matrix of a rotation by `degrees` about the camera-space y axis (ptx_scene_set_environment's R) */
void pth_rotation_y(double degrees, double R[9]);
/* the texture-table entry --ground-texture replaces: the floor triangles' material's texture, else the first checker (Shirley's
 * ground); -1 when the scene has neither */
int32_t pth_ground_texture(const ptx_scene_desc* d);

/* Bimage_unix.Stb.write of the f64 image (render_command.ml:66-70): 8-bit RGB PNG, v -> int(v*255) clamped.
 * returns 0 on success */
int32_t pth_write_png(const char* path, int32_t width, int32_t height, const double* rgb);
/* the same file from 8-bit codes, width * height * 3 of them (PTX_PIXEL_RGB8: what ptx_render_display hands back); pth_write_png is
 * its own conversion in front of this */
int32_t pth_write_png8(const char* path, int32_t width, int32_t height, const uint8_t* rgb8);

#ifdef __cplusplus
}
#endif
#endif
