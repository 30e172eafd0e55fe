/* scene_host.h -- from a caller's ptx_scene_desc to the arrays the kernels walk (PtHostArrays), in plain C++: no HIP call, so the
 * sanitizer build (host/Makefile `asan`, tests/c/asan_host_driver.cpp) compiles and runs exactly what the library ships.
 * ptx_api.inc drives it: scene_check_desc, scene_boxes, a tree (bvh_build or the GPU builder), scene_set_tree, and for a scene
 * with a device scene_assemble, then the upload. */
#ifndef SCENE_HOST_H
#define SCENE_HOST_H

#include <string>
#include <vector>

#include "../../include/ptx.h"
#include "bvh_build.h"

/* the codes the C ABI returns (include/ptx.h); everything this unit rejects is an argument error */
#define PTX_ERR_ARG (-1)
#define PTX_ERR_HIP (-2)
#define PTX_ERR_STATE (-3)

/* Everything ptx_scene_create uploads, kept on the host (<= 20 MB even for 150 k triangles) so that a REPLICA of the
 * scene on another device is one more upload, not another BVH build (ptx_scene_replicate, ptx_render n_gpus > 1).
 * A host-only scene (device -1) holds nodes, slot_prim, the emissive list and dev.n_nodes / n_slots / depth only. */
struct PtHostArrays {
  std::vector<PtNode> nodes;
  std::vector<double> sph, tri, tri_uv, tri_frame;
  std::vector<uint8_t> kind, cat;
  std::vector<int32_t> slot_mat, slot_prim;
  std::vector<PtMaterial> mats;
  std::vector<PtTexture> texs;
  std::vector<PtShadeRec> shade;
  std::vector<uint16_t> skip; /* node_skip: n_nodes x 8, empty for trees of >= 65535 nodes */
  std::vector<uint32_t> skip32; /* node_skip32: n_nodes x 8 */
  std::vector<uint32_t> nodes32; /* 8 words per node: the binary32 filter image for the walk from HBM / L2 */
  std::vector<uint32_t> nodes32o; /* PtSceneDev.nodes32o: 8 octants x 8 words per node; empty = not built */
  std::vector<uint32_t> lds_oct; /* PtSceneDev.lds_oct: 8 octants x 8 words per node, then the leaf table; empty = not built */
  std::vector<uint32_t> top_nodes, skip32_top; /* PtSceneDev.top_nodes (16 words per top node) / node_skip32_top; empty = none */
  /* the emissive tree triangles of the build list, in its order: 9 doubles each, kept up to one past PTX_MAX_LIGHT_TRIANGLES;
   * n_emissive_tris counts them all (ptx_scene_set_lighting makes the light table of them) */
  std::vector<double> emissive_tris;
  int n_emissive_tris = 0;
  /* the emissive tree spheres of the build list, in its order: {x, y, z, r} each, kept up to one past PTX_MAX_LIGHT_SPHERES;
   * n_emissive_spheres counts them all (ptx_scene_set_sphere_light_sampling makes the sphere light table of them) */
  std::vector<double> emissive_spheres;
  int n_emissive_spheres = 0;
  int n_textures = 0; /* the descriptor's texture table (ptx_scene_set_texture_image checks its index against it, host-only scenes too) */
  int tile_lists = 0; /* SceneOptions::tile_lists, kept for the schedule: camera launches may scan per-tile sphere lists (scene_tile_lists) */
  PtSceneDev dev{}; /* the scalar fields; device pointers are filled per upload */
};

/* the tuning switches of scene construction (documented in DESIGN.md), read once per ptx_scene_create */
struct SceneOptions {
  int tri_frame = 1;   /* PTX_TRI_FRAME: 0 = no tri_frame table */
  int oct_image = 1;   /* PTX_OCT_IMAGE: 0 = keep the shared image + skip table */
  int lds_oct = 1;     /* PTX_LDS_OCT: 0 = no per-octant LDS image: every launch keeps the shared one */
  int tile_lists = 1;  /* PTX_TILE_LISTS: 0 = camera rays always walk the tree (no per-tile sphere lists) */
  int top_nodes = 512; /* PTX_TOP_NODES: size of the breadth-first top image, clamped to 0 .. 1023 */
  int bin_key = -1;    /* PTX_BIN_KEY: -1 = by scene, 0 octant, 1 elevation, 2 reaches-the-root-box */
};
SceneOptions scene_options_from_env();

/* ?num_bins of Shape_tree.create: 32 unless the descriptor says otherwise */
inline int scene_num_bins(const ptx_scene_desc* d) { return d->num_bins > 0 ? d->num_bins : 32; }

/* Every check of an untrusted descriptor: counts, NULL arrays, material and texture kinds, then per element its vertex and
 * material indices.  0, or PTX_ERR_ARG with *msg set; nothing below is called with a descriptor this rejected. */
int scene_check_desc(const ptx_scene_desc* d, std::string* msg);

/* Leaf.elt_bbox of every element, build list = [triangles] @ [spheres] */
std::vector<Box> scene_boxes(const ptx_scene_desc* d);

/* Takes the tree: rejects leaves the kernels cannot hold (0, or PTX_ERR_ARG with *msg set), then fills h->nodes, h->slot_prim (leaf
 * order, then the floor triangles), the emissive list and dev.n_nodes / n_slots / depth.  Host-only scenes stop here. */
int scene_set_tree(const ptx_scene_desc* d, BvhResult&& tree, PtHostArrays* h, std::string* msg);

/* Everything else a device needs, from h->nodes and h->slot_prim: slot arrays, tri_frame, shading records, the threading and the
 * node images, the bin key, the remaining scalars of h->dev.  boxes = scene_boxes(d). */
void scene_assemble(const ptx_scene_desc* d, const std::vector<Box>& boxes, const SceneOptions& opt, PtHostArrays* h);

/* The light table of PTX_LIGHTING_SAMPLED: per emissive tree triangle PT_LIGHT_DOUBLES doubles {a, b, c, n, A, cum} */
std::vector<double> light_table_build(const PtHostArrays& h);
/* The sphere lights of ptx_scene_set_sphere_light_sampling: per emissive tree sphere PT_SLIGHT_DOUBLES doubles {c, r, r2, W, cum, 0};
 * cum = the running sum the first record continues (the triangles' total area, 0.0 without light triangles) */
std::vector<double> sphere_light_table_build(const PtHostArrays& h, double cum);

/* ---- image textures and the environment (include/ptx.h) ----
 * Every check of a caller's ptx_image: size, flags (an environment accepts PTX_IMAGE_BILINEAR only), reserved, every texel finite.
 * 0, or PTX_ERR_ARG with *msg naming what was wrong. */
int scene_check_image(const ptx_image* img, bool environment, std::string* msg);
/* the texels as the device holds them: one 32-byte record {r, g, b, 0} per texel, bit for bit */
std::vector<double> scene_image_records(const ptx_image* img);
/* One entry of the texture table that carries an image: its size and flags and where one device holds its texels (width 0 = the entry
 * keeps the descriptor's texture). */
struct PtImageEntry {
  int32_t width = 0, height = 0, flags = 0;
  uint64_t texels = 0; /* device address of the records */
};
/* h.cat and h.shade with the images of `entries` (one per texture-table entry) in place: a slot whose material points at such an entry
 * gets tex_kind PT_TEX_IMAGE, the size, and the address and flags in the bits of even[0] / even[1] (pt_scene.h); a Lambertian one moves
 * to the textured-Lambertian category, whose shade step computes tex coords. */
void scene_image_overrides(const PtHostArrays& h, const std::vector<PtImageEntry>& entries, std::vector<uint8_t>* cat,
                           std::vector<PtShadeRec>* shade);

/* ---- the density over the environment image (include/ptx.h, ptx_scene_set_environment_sampling) ----
 * One table of doubles, as the device holds it behind the environment's texels (pt_scene.h, PT_ENVD_*): T, last_row, m[H], per row the
 * last column with w > 0 (0 for a row without one) [H], c_iy[ix] [H x W], w(ix, iy) [H x W]; last_row = the last row with r_iy > 0,
 * total = T. */
struct PtEnvDensity {
  int32_t width = 0, height = 0, last_row = 0;
  double total = 0.0;
  std::vector<double> table;
};
/* max |R R^T - I| <= 1e-9, or PTX_ERR_ARG with *msg naming the rule */
int scene_check_env_rotation(const double R[9], std::string* msg);
/* The density of the texel records `rec` (4 doubles per texel, scene_image_records).  0, or PTX_ERR_ARG with *msg set when the total
 * weight is not finite or not greater than 0 (*out is then unspecified). */
int scene_env_density(const double* rec, int32_t width, int32_t height, PtEnvDensity* out, std::string* msg);

/* ---- camera tile lists: which spheres a camera ray through an 8 x 8 pixel tile can meet ----
 * One 32-byte record per tile of the GLOBAL tile grid of a width x height image, row-major, tiles_x = ceil(width / 8):
 *   byte 0      the number of slots listed, 0 .. PT_TILE_MAX_SLOTS, or PT_TILE_WALK (pt_scene.h): the tile's rays walk the tree
 *   byte 1      the direction octant (PtTraverser::dirs) every ray of the tile has
 *   bytes 2..31 up to 15 leaf-order slot numbers (uint16), in the order in which a near-first descent of that octant meets their
 *               leaves, slot order inside a leaf -- the relative order in which the walk tests them
 * A slot is listed unless its sphere, its radius inflated by PT_TILE_INFLATE (|c| + r), lies wholly outside one of the four side
 * planes of the pyramid the tile's camera rays span from the origin (rows and columns are tested on their own: separable). */
#define PT_TILE_MAX_SLOTS 15
#define PT_TILE_INFLATE 0x1p-40
#define PT_TILE_MAX_CR 0x1p18 /* a listed sphere with |c| > PT_TILE_MAX_CR r makes its tiles walk: the scan's guard on the discriminant assumes |c| / r <= 2^19 */
struct PtTileRec {
  uint8_t count, octant;
  uint16_t slot[PT_TILE_MAX_SLOTS];
};
static_assert(sizeof(PtTileRec) == 32, "one 32-byte record per tile");
struct PtTileGrid {
  int width = 0, height = 0, tiles_x = 0, tiles_y = 0;
  int n_walk = 0, longest = 0; /* tiles marked PT_TILE_WALK; the longest list */
  std::vector<PtTileRec> rec;  /* tiles_x * tiles_y */
};
/* the scene can have tile lists at all: Simd_leaf spheres only, no floor, slot numbers within 16 bits */
bool scene_tile_lists_possible(const PtHostArrays& h);
PtTileGrid scene_tile_lists(const PtHostArrays& h, int width, int height);

/* ---- display outputs (include/ptx.h): the host half of the rule of pt_display.h ----
 * Every check of a caller's ptx_display_params.  0, or PTX_ERR_ARG with *msg naming the rule that refused. */
int display_check(const ptx_display_params* d, std::string* msg);
/* bytes of a pixel of `format`, 0 for an unknown one */
int display_pixel_bytes(int32_t format);
/* the 255 sRGB thresholds, [k - 1] = T[k]: computed with libm the first time they are asked for and kept for the process */
const double* display_thresholds();
/* the rule over n_pixels pixels (3 doubles each) into n_pixels * display_pixel_bytes(d.format) bytes; d has passed display_check */
void display_apply_host(const ptx_display_params& d, int64_t n_pixels, const double* rgb, void* out);

#endif /* SCENE_HOST_H */
