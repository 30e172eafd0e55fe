/* pt_scene.h -- the flattened scene as it lives in HBM, shared by the host builder
 * (bvh_build.cpp for the tree, scene_host.cpp for everything made of it) and the HIP kernels (kernels.hip).
 *
 * Layout decisions:
 *  - BVH node = one 64-byte record (bbox 6 x f64 + two u32 links), 64-byte aligned: a lane
 *    that visits a node touches exactly one cache line / four 16-byte LDS reads.
 *  - leaf primitive slots are stored in LEAF ORDER, contiguous per leaf ("packets"):
 *      sphere slot   = 4 x f64 {x, y, z, r}        (32 B; NaN padding slots for Simd_leaf)
 *      triangle slot = 10 x f64 {a, b, c, pad}     (80 B, 16-byte aligned)
 *    so a leaf is one contiguous burst, never an index gather.
 *  - a slot's shading data (material id, kind, primitive id, triangle UVs) sits in
 *    separate arrays touched only by the shade stage for the ONE slot that was hit.
 */
#ifndef PT_SCENE_H
#define PT_SCENE_H

#include <stdint.h>

#define PT_NODE_LEAF_AXIS 3u /* axis code stored in the two top bits of `b` for leaves */
#define PT_TOP_FLAG 0x20000000u /* a node reference into the LDS-resident top image (PtSceneDev.top_nodes): flag | byte offset */
#define PT_TOP_NODE_BYTES 64
#define PT_MAX_FINITE 1.7976931348623157e308

/* Layout constants of the images the host builds (scene_host.cpp) and the kernels walk (kernels.hip describes the walks). */
/* bytes per node of the LDS-resident filter image; the host's "fits LDS" threshold: a tree of n_nodes * PT_SWZ_NODE_BYTES >= 65535
 * bytes is walked from HBM / L2 and gets the per-octant and the top image */
#define PT_SWZ_NODE_BYTES 92 /* 80 used + 12: 23 words, an ODD stride, so that node k starts in LDS bank 21 k mod 64 -- all 64 banks.
                                With 80 bytes (20 words) the nodes start in 16 of the 64 banks only, with 64 bytes in 4 */
/* the per-octant record (PtSceneDev.nodes32o): word 6 of a leaf = PT_OCT_LEAF_TAG | real slots << PT_OCT_LEAF_FIRST_BITS | first slot,
 * word 7 = the octant's skip link or PT_OCT_END */
#define PT_OCT_LEAF_FIRST_BITS 22
#define PT_OCT_LEAF_REAL_MAX 255u
#define PT_OCT_END 0x80000000u
#define PT_OCT_LEAF_TAG 0x40000000u
/* the per-octant LDS image (PtSceneDev.lds_oct; the walk: kernels.hip, PtLdsOctTag): 8 x n_nodes records of 32 bytes -- near xyz,
 * far xyz for the octant's direction signs, word 6 = hit link | miss link << 16, word 7 = the node's magnitude as the shared LDS image
 * stores it -- then the leaf table, one word per node (a leaf: first slot | real slots << 16), padded to 16 bytes.  A link is a record
 * number in the whole image (14 bits: the octant's base added) under two control bits: 00 a node to visit, 01 (a leaf's hit link:
 * its own record) "this lane holds a leaf", 10 the walk is over.  After its leaf phase a lane goes on at the leaf record's miss link. */
#define PT_LOCT_RECORD_BYTES 32
#define PT_LOCT_LEAF_TAG 0x4000u
#define PT_LOCT_END 0x8000u
#define PT_LOCT_MAX_NODES 2047 /* 8 x n_nodes record numbers below 2^14 */
#define PT_LOCT_LEAF_WORDS(n_nodes) (((uint32_t)(n_nodes) + 3u) & ~3u)
#define PT_TRI_FRAME_DOUBLES 12 /* PtSceneDev.tri_frame: doubles per slot */
constexpr int kTriFrameMaxSlots = 1024; /* PtSceneDev.tri_frame: <= 96 KB, resident in L1 / L2 */

/* One BVH node, 64 bytes.  Tree.t = Bbox.t * (Leaf | Branch {axis; lhs; rhs}), shape_tree.ml:153-161 */
struct __attribute__((aligned(64))) PtNode {
  double mn[3];
  double mx[3];
  uint32_t a; /* branch: index of lhs        | leaf: first slot            */
  uint32_t b; /* branch: index of rhs + axis<<30 | leaf: slot count + 3<<30 */
  uint32_t pad[2]; /* leaf: pad[0] = number of real (non-padding) slots */
};

#define PT_SLOT_SPHERE 0
#define PT_SLOT_TRIANGLE 1
#define PT_SLOT_PAD 2 /* NaN padding slot of a Simd_leaf packet */

/* shading categories: what a segment will execute in the shade stage */
#define PT_CAT_MISS 0
#define PT_CAT_LAMBERT_SOLID 1
#define PT_CAT_LAMBERT_CHECKER 2
#define PT_CAT_METAL 3
#define PT_CAT_DIELECTRIC 4
#define PT_CAT_NONE 5 /* beyond the end of the queue */
#define PT_N_CAT 6

/* scene "mode" = which Leaf implementation the tree was built with */
#define PT_MODE_SIMD 0  /* Simd_leaf packets: every slot a sphere, Rust x86 arithmetic */
#define PT_MODE_ARRAY 1 /* Array_leaf: spheres (scalar Sphere.intersect) and/or triangles */

struct PtMaterial { /* 48 B */
  int32_t kind;
  int32_t texture;
  double index;
  double emit[3];
  double pad;
};
struct PtTexture { /* 64 B */
  int32_t kind;
  int32_t width, height;
  int32_t pad;
  double even[3];
  double odd[3];
  double pad2;
};

/* What shading one hit on a slot needs besides the slot's geometry, in ONE 96-byte record per slot: material kind /
 * index / emission and the texture it points at.  The shade stage used to reach this through three dependent gathers
 * (slot -> slot_material -> materials -> textures: each ~1-2 us under load, with the kernel 70 % of its time parked on
 * s_waitcnt); now the hop after the hit slot is the last one. */
struct __attribute__((aligned(16))) PtShadeRec {
  int32_t kind;     /* PTX_MAT_* */
  int32_t tex_kind; /* PTX_TEX_* (Lambertian / Metal), or PT_TEX_IMAGE */
  int32_t tex_w, tex_h;
  double index;
  double even[3];
  double odd[3];
  double emit[3];
};
/* An entry of the texture table that carries an image (ptx_scene_set_texture_image): tex_w x tex_h texels, and in place of the two
 * colours, which an image does not use, the bits of even[0] = the device address of the texels (32-byte records {r, g, b, -}) and
 * of even[1] = the PTX_IMAGE_* flags -- the hop after the hit slot stays the last one before the texels.  Only the instantiations
 * flagged IMG look for it, and only scenes with an image or an environment launch those. */
#define PT_TEX_IMAGE 2
#define PT_BG_ENV 2 /* PtSceneDev.bg_kind: the environment image (ptx_scene_set_environment) */
#define PT_IMAGE_BILINEAR 1 /* = PTX_IMAGE_* */
#define PT_IMAGE_REPEAT_U 2
#define PT_IMAGE_REPEAT_V 4

/* everything a kernel needs, passed by value (pointers are device pointers) */
struct PtSceneDev {
  const PtNode* nodes;
  int32_t n_nodes;
  int32_t depth;       /* tree depth = max traversal stack entries */
  int32_t mode;        /* PT_MODE_* */
  int32_t n_slots;
  const double* sph;   /* n_slots x 4 (valid where slot_kind != TRIANGLE) */
  const double* tri;   /* n_slots x 10 (valid where slot_kind == TRIANGLE); NULL if no triangles */
  const double* tri_uv;/* n_slots x 6 */
  /* Small scenes with triangles: what Triangle.Hit.to_hit + Shader_space.create derive from the triangle ALONE, per slot, 12 doubles:
   * {g_normal xyz, -, rotation of +g_normal (r, x, y, z), rotation of -g_normal}.  Computed once on the host with the functions
   * the shade step itself uses (pt_tri_normal / pt_shader_rotation of pt_vec.h; scene_host.cpp), so a load replaces ~130 vector
   * instructions per triangle hit with the same bits.  NULL: the shade step computes them (large meshes: the table would be one more gathered line per segment). */
  const double* tri_frame;
  const uint8_t* slot_kind;
  const uint8_t* slot_cat;  /* shading category of the slot's material, PT_CAT_* (wave-coherent shading) */
  const int32_t* slot_material;
  const int32_t* slot_prim; /* build-list primitive index, -1 for padding */
  /* floor triangles tested before the tree (ganesha Floor): appended after the tree slots
   * in tri / tri_uv / slot_* at indices n_slots .. n_slots + n_floor - 1 */
  int32_t n_floor;
  int32_t has_triangles;
  int32_t has_emit;
  int32_t has_checker;
  /* LDS-resident scenes: 1 = the LDS image also carries every node's six binary64 bounds (48 bytes per node) for the tests the
   * binary32 filter leaves undecided -- 2 % (Shirley) to 5.5 % (cornell) of a walk's wave steps, each of which otherwise waits for a
   * global load.  Set per upload (scene_upload in ptx_api.inc: it depends on the device's LDS, unlike the
   * scalars scene_host.cpp fills) when the scene still fits LDS with them. */
  int32_t lds_nodes64;
  const PtMaterial* materials;
  const PtTexture* textures;
  const PtShadeRec* slot_shade; /* per slot (padding slots zero) */
  /* n_nodes x 8 (u16 node indices, 0xffff = none): per direction octant, the node visited after a node's subtree
   * (the threading of the LDS node image, kernels.hip); NULL when the tree has 65535 nodes or more */
  const uint16_t* node_skip;
  /* the same threading with 32-bit node indices (0xffffffff = none): scenes walked from HBM / L2 */
  const uint32_t* node_skip32;
  /* n_nodes x 32 bytes: mn.xyz, mx.xyz rounded to binary32, a, b (leaf b: padded count | real count << 15 | tag): the filter
   * image of the walk from HBM / L2 -- half the bytes per visit of the 64-byte binary64 node, which only undecided tests read */
  const void* nodes32;
  /* 8 x n_nodes x 32 bytes, or NULL: the same image once per direction octant with that octant's skip link inside the record
   * (mn.xyz, mx.xyz, link, skip) -- a visit is two loads instead of three (kernels.hip, PtThreadOctTag).  Built when the tree
   * is in pre-order with lhs = node + 1 (always) and every leaf fits the packed link (first slot < 2^22, <= 255 real slots). */
  const void* nodes32o;
  /* Scenes walked from HBM / L2: the TOP of the tree (the first n_top nodes in breadth-first order) as 64-byte records that
   * every trace workgroup copies into LDS -- 6 binary32 bounds, links a / b as in nodes32, eight 16-bit skip links (byte
   * offsets into this image; the node that follows a top node's subtree is an ancestor's sibling, hence a top node too), the
   * node's own index.  A link to a top node is PT_TOP_FLAG | byte offset, here and in node_skip32_top (= node_skip32 with
   * top targets encoded that way).  Half of a large mesh's node visits are within its first ~1000 nodes: those steps stop
   * waiting for L2.  NULL / 0 when the scene has no such image. */
  const uint32_t* top_nodes;
  const uint32_t* node_skip32_top;
  int32_t n_top;
  int32_t all_triangles; /* 1: every tree slot is a triangle (a mesh): the leaf loop needs no per-slot kind */
  /* unit vector (camera space) along which the primitives' centres vary least = the normal of the scene's ground plane when it
   * has one.  A HEURISTIC sort key only (shade bins survivors by the elevation of the new direction above that plane, a
   * predictor of how long the next walk is); it never enters a pixel value. */
  double sort_axis[3];
  int32_t sort_by_elevation; /* 1: the centres do lie in a slab (smallest variance < 2 % of the largest): bin by elevation; 0: by direction octant */
  /* 1: bin by whether the new ray reaches the tree's bounding box at all (+ two direction signs).  Scenes whose rays mostly start
   * OUTSIDE the tree (a mesh standing on a floor that is tested before the tree): a ray that misses the box costs one node test, one
   * that enters it walks a hundred nodes, and a wave that holds both waits for the longest.  Heuristic, binary32, never enters a pixel. */
  int32_t sort_by_root;
  float root_mn[3], root_mx[3];
  /* max |coordinate| of the tree's root box, rounded UP to binary32 (+inf when it exceeds the format): every node lies inside
   * the root box, so this bounds every node's magnitude.  The binary32 node filter applies to a ray only if
   * (root_mag + max|o|) * max|1/d| < 2^100 -- then no binary32 intermediate of the filter can overflow (kernels.hip, begin()). */
  float root_mag;
  union { /* (one word, two names, like env_sample below) */
    float pad_f;
    /* ptx_scene_set_sphere_light_sampling is on, in lighting mode 2: this many sphere light records lie behind the n_lights triangle
     * records of `lights` (PT_SLIGHT_* below), and light_area is the joined table's last running sum.  Read only by the instantiations
     * flagged LIT, behind a wave-uniform branch */
    int32_t n_sphere_lights;
  };
  double cam_llx, cam_lly, cam_vx, cam_vy;
  int32_t bg_kind;
  union { /* (one word, two names: scenes without environment sampling, and everything that only copies the struct, see padding) */
    int32_t pad0;
    int32_t env_sample; /* ptx_scene_set_environment_sampling is on: the density table lies behind the environment's texels (PT_ENVD_* below) */
  };
  double bg_horizon[3];
  double bg_zenith[3];
  /* The lighting mode in effect (PTX_LIGHTING_*; ptx_scene_set_lighting) and, in mode 2, the light table: n_lights records of
   * PT_LIGHT_DOUBLES doubles {a, b, c, unit normal, area, running sum of the areas}, the scene's emissive tree triangles in build-list
   * order.  Read only by the instantiations flagged LIT (pt_shade_entry), which mode 0 never launches. */
  const double* lights;
  int32_t n_lights;
  int32_t lighting;
  double light_area; /* the sum of the areas = the last record's running sum */
  /* Simd_leaf trees of at most PT_LOCT_MAX_NODES nodes: the per-octant LDS image (PT_LOCT_* above), 8 x n_nodes x 8 words of records
   * and PT_LOCT_LEAF_WORDS(n_nodes) words of leaf table, or NULL.  The non-counting k_bounce_carry launches of a scene whose buffer
   * fits with it (pt_lds_layout.h, pt_lds_oct_layout; Schedule::lds_oct) copy it into LDS in place of the shared node image. */
  const uint32_t* lds_oct;
  /* the camera tile lists of the image being rendered (scene_host.h, PtTileRec: 32 bytes per 8 x 8 tile of the global grid), or NULL.
   * Set per launch (launch_bounce_carry); read only by k_bounce_carry's TILE instantiations, which are launched only with it. */
  const uint32_t* tile_lists;
  /* ptx_scene_set_texture_image / _set_environment: how many entries of the texture table carry an image; the environment's texels
   * (32-byte records, NULL = none: bg_kind then is the descriptor's), its size, its PTX_IMAGE_BILINEAR flag and the row-major matrix
   * from camera space to environment space.  Read only by the instantiations flagged IMG. */
  const double* env;
  int32_t env_w, env_h;
  int32_t env_flags;
  int32_t n_images;
  double env_rot[9];
};
/* ptx_scene_set_environment_sampling keeps PtSceneDev as it is (its size is every kernel's argument layout): env_sample takes the place of
 * a padding word, and while it is set the density table lies in the environment's own buffer, right behind the W x H texel records
 * (env + 4 W H doubles).  env_sample is read only by the LIT && IMG instantiations, in lighting mode 2 (a wave-uniform branch,
 * pt_shade_entry); a scene with it on and no emitter still has has_emit = 1: it is scheduled as a lit scene, with the queue's emission
 * record, which then stays zero.
 * The density table (scene_host.h, PtEnvDensity), offsets in doubles for a W x H image: the total weight T and the last row with a
 * positive weight (as a double); the running sums of the rows m[H]; per row the last column with w > 0 [H] (as doubles); the running
 * sums inside the rows c[H x W]; the weights w[H x W] */
#define PT_ENVD_TOTAL 0
#define PT_ENVD_LAST_ROW 1
#define PT_ENVD_ROWS 2
#define PT_ENVD_LASTX(H) (2 + (size_t)(H))
#define PT_ENVD_COND(H) (2 + 2 * (size_t)(H))
#define PT_ENVD_WEIGHT(W, H) (2 + 2 * (size_t)(H) + (size_t)(W) * (size_t)(H))
#define PT_ENVD_SIZE(W, H) (2 + 2 * (size_t)(H) + 2 * (size_t)(W) * (size_t)(H))
#define PT_TILE_WALK 0xffu /* a record's count byte: the tile's rays walk the tree */

#define PT_LIGHTING_SAMPLED 2 /* = PTX_LIGHTING_SAMPLED */
#define PT_LIGHT_DOUBLES 14
#define PT_LIGHT_AREA 12
#define PT_LIGHT_CUM 13
/* ptx_scene_set_sphere_light_sampling keeps PtSceneDev as it is, as environment sampling does (its size is every kernel's argument
 * layout: a pointer and a count appended at its end changed the register and scratch figures of kernels that never look at a light,
 * profiles/pr_sphere_lights_kernel_resources_*.txt): the count takes a padding word, and the records lie in the light table's own
 * buffer, right behind the triangles' (lights + n_lights * PT_LIGHT_DOUBLES), 8 doubles each: {c, r, r * r, W = (2 pi) r^2, running sum
 * continuing the triangles', 0} */
#define PT_SLIGHT_DOUBLES 8 /* one 64-byte record per sphere light */
#define PT_SLIGHT_R 3
#define PT_SLIGHT_R2 4
#define PT_SLIGHT_W 5
#define PT_SLIGHT_CUM 6

#endif /* PT_SCENE_H */
