/* ptx.h -- C ABI of the MI355X path-tracing integrator (libptx_hip.so).
 *
 * Drop-in boundary for ONE hot path of dalev/path-tracer-ocaml: the per-pixel
 * sampling integrator (Integrator.create / Integrator.render,
 * path_tracer/src/integrator.mli:4-16, driven by Render_command.Make.run,
 * render_command/src/render_command.ml:64-109).
 *
 * The reference's only FFI is per-leaf (one ray x one <=16-sphere packet):
 *   external spheres_intersect_native : coords -> float -> float -> Ray.t -> float_ref -> int
 *   external leaf_size : unit -> int          (shirley_spheres/bin/main.ml:162-172,
 *                                              sphere-intersect-rs/src/lib.rs:15-18,53-76)
 * A GPU cannot be called once per BVH leaf per ray, and the reference's
 * intersect / background / do_scatter are opaque OCaml closures
 * (render_command.mli:18-22), so the accelerated boundary sits one level up:
 * the host hands over a DECLARATIVE scene (what main.ml builds before it calls
 * Render_cmd.run) and gets the post-gamma f64 framebuffer back -- exactly what
 * Integrator.render leaves in its Bimage (integrator.ml:130-156).
 *
 * Conventions: plain pointers and sizes; the caller owns every input and output
 * buffer; the library copies what it keeps.  All geometry is ALREADY in camera
 * space (the reference pre-transforms it: shirley_spheres/bin/main.ml:258-260,
 * ganesha/bin/main.ml:74-79).  No exceptions cross the boundary: every call
 * returns 0 / a handle on success and a negative code / NULL on failure, with
 * ptx_last_error() giving the message.  One render per handle at a time.
 */
#ifndef PTX_H
#define PTX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTX_ABI_VERSION 6

/* ---- materials: Material.t, path_tracer/src/material.ml:3-14 ---- */
#define PTX_MAT_LAMBERTIAN 0 /* Lambertian of Texture.t */
#define PTX_MAT_METAL 1      /* Metal of Texture.t (no fuzz) */
#define PTX_MAT_DIELECTRIC 2 /* Dielectric {index; index_inv = 1/index} */

typedef struct ptx_material {
  int32_t kind;
  int32_t texture; /* index into textures (Lambertian / Metal) */
  double index;    /* Dielectric only */
  /* Hit.emit slot (hit.ml:5).  The reference's Material.emit is constant black
   * (material.ml:59); non-zero values are the documented emitter extension used
   * by the cornell-box configuration only. */
  double emit[3];
} ptx_material;

/* ---- textures: Texture.solid / Texture.checker, path_tracer/src/texture.ml:16-31 ---- */
#define PTX_TEX_SOLID 0
#define PTX_TEX_CHECKER 1

typedef struct ptx_texture {
  int32_t kind;
  int32_t width, height; /* checker ~width ~height (the code uses width-1, height-1) */
  int32_t reserved;
  double even[3]; /* solid colour, or the checker's "even" solid */
  double odd[3];
} ptx_texture;

/* ---- camera: the four fields Camera.ray reads, path_tracer/src/camera.ml:50-53,93-102 ---- */
typedef struct ptx_camera {
  double lower_left_x, lower_left_y, view_x, view_y;
} ptx_camera;

/* ---- background: Scene.background closure made declarative ---- */
#define PTX_BG_BLACK 0
#define PTX_BG_SKY 1 /* lerp t horizon zenith, t = .5*(normalize(dir).y + 1); main.ml:104-110 */

typedef struct ptx_background {
  int32_t kind;
  int32_t reserved;
  double horizon[3]; /* Color.white in the reference */
  double zenith[3];  /* escape_color (.5,.7,1) */
} ptx_background;

/* ---- leaf flavours: Shape_tree.Leaf implementations ---- */
#define PTX_LEAF_SIMD 0  /* Simd_leaf: <=16-sphere SoA packets, Rust x86 arithmetic (lib.rs:102-178) */
#define PTX_LEAF_ARRAY 1 /* Array_leaf: linear scan, Sphere.intersect / Triangle.intersect */

typedef struct ptx_scene_desc {
  /* spheres (Sphere.t: centre, radius, material), SoA like Simd_leaf.coords */
  int32_t n_spheres;
  const double* sphere_x;
  const double* sphere_y;
  const double* sphere_z;
  const double* sphere_r;
  const int32_t* sphere_material;

  /* triangle mesh (ganesha Mesh.t: SoA vertices + index triples; cornell Face.t) */
  int32_t n_vertices;
  const double* vertex_x;
  const double* vertex_y;
  const double* vertex_z;
  int32_t n_triangles;
  const int32_t* tri_indices;  /* 3 per triangle: a, b, c */
  const double* tri_uv;        /* 6 per triangle: (ua,va),(ub,vb),(uc,vc) */
  const int32_t* tri_material; /* 1 per triangle */

  /* triangles tested BEFORE the tree, clipping t_max (ganesha Floor, main.ml:205-298) */
  int32_t n_floor_triangles;
  const double* floor_vertices; /* 9 per triangle */
  const double* floor_uv;       /* 6 per triangle */
  const int32_t* floor_material;

  int32_t n_materials;
  const ptx_material* materials;
  int32_t n_textures;
  const ptx_texture* textures;

  ptx_camera camera;
  ptx_background background;

  /* Shape_tree.create ?num_bins (default 32), Leaf.length_cutoff, leaf flavour.
   * The tree is built over [triangles in order] @ [spheres in order]
   * (cornell-box/bin/main.ml:213-218). */
  int32_t leaf_kind;
  int32_t length_cutoff; /* 16 for SIMD (lib.rs:13), 4 / 2 / 8 for the array leaves */
  int32_t num_bins;      /* 0 -> 32 */
  int32_t reserved;      /* BVH builder: 0 auto (GPU for >= 4096 primitives, else host), 1 host, 2 GPU -- same tree.
                          * The GPU builder takes at most 64 bins and no primitive boxes of which one bound (min x .. max z)
                          * is +0.0 in one box and -0.0 in another: there the reference's result depends on the order of
                          * the primitives.  0 builds such scenes on the host; 2 fails with PTX_ERR_ARG, as it does on a
                          * host-only scene. */
} ptx_scene_desc;

/* ---- render parameters: Render_command.Args.t (render_command.ml:7-14) ---- */
typedef struct ptx_render_params {
  int32_t width, height;
  int32_t samples_per_pixel;
  int32_t max_bounces;
  /* Image rows are dealt to ranks in horizontal bands: rank `band_first` of
   * `band_step` renders bands band_first, band_first+band_step, ... of
   * `band_rows` rows each.  band_step <= 1 renders the whole image. */
  int32_t band_rows;
  int32_t band_first;
  int32_t band_step;
  /* 1: also count BVH nodes tested / primitive slots tested (slower; parity vs
   * the instrumented oracle and the algorithmic-bytes figure). */
  int32_t count_work;
  /* 1: bracket every kernel launch with HIP events (per-kernel ms in ptx_stats). */
  int32_t time_kernels;
  /* samples per wavefront batch in passes; 0 = library default */
  int32_t passes_per_batch;
  /* ptx_render only: GPUs of this node to spread the image over, inside this one process (SURVEY section 8 B3 / E;
   * the reference's Domainslib pool over tiles, integrator.ml:136-151, becomes one host thread per device over
   * interleaved row bands).  0 or 1 = the scene's own device only.  Devices used: the scene's, then the following
   * ordinals (mod ptx_device_count()); replicas of the scene are made on first use and kept with the handle. */
  int32_t n_gpus;
  /* PTX_RENDER_ASYNC (ptx_render_raw_device only): return as soon as the frame is QUEUED on `stream` -- the caller's next use
   * of the buffer must be ordered after it on that stream (as a following ptx_* call or a collective on it is), or wait for
   * the stream.  `stats` then carries no timings or counters; count_work / time_kernels renders always wait.  For hosts
   * that pipeline frames (one rank of a multi-GPU job: the next frame is queued while this one's bands travel). */
  int32_t flags;
} ptx_render_params;
#define PTX_RENDER_ASYNC 1

#define PTX_KERNEL_GENERATE 0
#define PTX_KERNEL_TRACE 1
#define PTX_KERNEL_SHADE 2
#define PTX_KERNEL_ACCUM 3
#define PTX_KERNEL_FILM 4
#define PTX_KERNEL_BOUNCE 5 /* trace + shade of one bounce in ONE launch (scenes whose tree fits LDS); then TRACE / SHADE count only what ran separately */
#define PTX_N_KERNELS 6

typedef struct ptx_stats {
  int64_t samples;       /* W * rows * spp actually rendered */
  int64_t segments;      /* rays traced (Scene.intersect calls, integrator.ml:35) */
  int64_t nodes_tested;  /* Bbox.is_hit evaluations (shape_tree.ml:203), if count_work */
  int64_t prims_tested;  /* leaf slots tested incl. NaN padding, if count_work */
  int64_t floor_tested;  /* floor triangle tests, if count_work */
  double render_ms;      /* host wall time of the call (after the final sync) */
  double kernel_ms[PTX_N_KERNELS]; /* summed HIP-event time per kernel kind, if time_kernels */
  int64_t kernel_launches[PTX_N_KERNELS];
  int32_t tree_nodes, tree_depth, tree_leaves, leaf_slots;
  double build_ms; /* BVH build + upload at ptx_scene_create */
  int32_t traversal_in_lds; /* 1: tree + leaf packets fit the per-workgroup LDS copy; 0: traversed from HBM / L2 */
  int32_t bvh_built_on_gpu; /* 1: csrc/bvh_build_gpu.inc built the tree, 0: the host builder (same tree) */
  /* if count_work: Bbox.is_hit evaluations the binary32 filter in front of the binary64 slab test could NOT decide (they
   * then ran the reference's binary64 arithmetic, bbox.ml:40-56), and the wave steps that entered that branch.  Both
   * are 0 for walks that never use the filter; the parity tests assert the branch is exercised. */
  int64_t filter_undecided;
  int64_t filter_fallback_steps;
  /* ptx_render with n_gpus > 1 / ptx_render_multi: how each replica's raw sums reached the root device --
   * peer_copies = device-to-device with peer access enabled (xGMI), staged_copies = hipMemcpyPeer without peer
   * access (the runtime stages through host memory).  Replicas that share the root's device count in neither. */
  int32_t peer_copies;
  int32_t staged_copies;
  /* if count_work: launches of the one-kernel-per-bounce path that found their input small enough (PTX_SOLO_ENTRIES) to run all
   * remaining bounces of their batch by themselves; the batch's later launches return at once (ABI 6) */
  int32_t solo_launches;
  /* if count_work: launches of the one-kernel-per-bounce path in the shade-first order (k_bounce_carry; PTX_BOUNCE_ORDER=0 and the
   * modes that keep the walk-first order give 0).  Took the place of a reserved word: the layout of ABI 6 is unchanged */
  int32_t carry_launches;
  /* if count_work: camera launches (k_bounce / k_bounce_carry, LDS-resident scenes) whose rays walked the tree one per lane
   * (pt_trace_ray) instead of as a wave packet (pt_trace_packet): PTX_PRIMARY_WALK.  APPENDED: every offset of ABI 6 is unchanged but
   * sizeof(ptx_stats) grows by 8 bytes (the word and its padding), and the library writes the whole struct: a caller must be
   * compiled against this header (the Python, OCaml and host callers of this repository are).  ptx_version() stays 6 */
  int32_t primary_lane_walks;
  /* renders (1 per ptx_render-family call or slice, summed over the slices of a progressive render) whose non-counting k_bounce_carry launches held
   * the per-octant LDS node image and walked it (PTX_LDS_OCT; Simd_leaf scenes whose launch buffer fits with it).  0 for counting
   * renders: they keep the shared image.  APPENDED into the padding behind primary_lane_walks: no offset and not the size of the
   * struct changes.  ptx_version() stays 6 */
  int32_t lds_oct_launches;
} ptx_stats;

/* ---- progressive photon mapping (progressive-photon-map/src/progressive_photon_map.ml) ---- */
#define PTX_LIGHT_POINT 0 /* Light.create_point ~position ~power ~color  (:64-84) */
#define PTX_LIGHT_SPOT 1  /* Light.create_spot ~position ~direction ~color ~power (:86-110) */

typedef struct ptx_light {
  int32_t kind;
  int32_t reserved;
  double position[3];  /* camera space, like every other coordinate */
  double direction[3]; /* spot only (not normalised by the caller) */
  double color[3];     /* BEFORE the power scaling */
  double power;
} ptx_light;

/* Progressive_photon_map.Args.t (:7-16) */
typedef struct ptx_ppm_params {
  int32_t width, height;
  int32_t iterations;   /* default 10 */
  int32_t max_bounces;  /* default 4 */
  int32_t photon_count; /* default 75000 */
  int32_t reserved;
  double alpha;         /* default 2/3 */
} ptx_ppm_params;

typedef struct ptx_ppm_stats {
  int64_t photons_stored;  /* Photon_map.length summed over iterations */
  int64_t photon_rays;     /* segments traced from the lights */
  int64_t eye_rays;        /* segments traced from the camera */
  int64_t neighbors;       /* photons accepted by the radiance estimates */
  double photon_ms, build_ms, gather_ms, total_ms;
  double last_radius;
  int64_t device_trees;    /* iterations whose photon list and tree were made on the device and never left it */
  int64_t gpu_built_trees; /* iterations whose tree the GPU builder made (those, and host-side lists of >= 4096 photons) */
} ptx_ppm_stats;

typedef struct ptx_scene ptx_scene; /* opaque */

typedef void (*ptx_progress_fn)(void* user, int64_t pixels_done);

/* ---- entry points ---- */
int32_t ptx_version(void);
/* replaces `leaf_size : unit -> int` (lib.rs:15-18) */
int32_t ptx_leaf_size(void);
const char* ptx_last_error(void);

/* number of HIP devices visible; negative on error */
int32_t ptx_device_count(void);

/* Builds the BVH on the host exactly as Shape_tree.create does (shape_tree.ml:252-263),
 * flattens it and uploads everything to HIP device `device`.
 * device == -1 builds a HOST-ONLY scene (nothing uploaded): only ptx_scene_tree / ptx_scene_stats /
 * ptx_scene_destroy accept it; every compute entry point returns an error (there is no CPU fallback). */
ptx_scene* ptx_scene_create(const ptx_scene_desc* desc, int32_t device);
void ptx_scene_destroy(ptx_scene* scene);
/* copies the build statistics (tree_* and build_ms fields) */
int32_t ptx_scene_stats(const ptx_scene* scene, ptx_stats* out);
/* Camera tile lists (PTX_TILE_LISTS): of the last render call (or slice) on this handle, out = {camera launches that
 * scanned their tiles' sphere lists instead of walking the tree, tiles of the image's grid, tiles of it that keep the walk, the
 * longest list, chunks of camera rays a guard of the scan sent back to the walk}.  All zero when that render scanned no lists: a
 * counting render, a scene without lists, PTX_TILE_LISTS=0.  The last figure is not per render: it runs on from the handle's first
 * render that scanned lists (a counting render sets it back to zero), so that no render has to touch it while another is queued.
 * A handle keeps the lists of at most 8 image sizes (32 bytes per 8 x 8 tile, on the host and on every device it renders on) for
 * its life; renders of a further size walk the tree.  Waits for the device.  ptx_stats and ptx_version() are unchanged. */
int32_t ptx_tile_list_stats(const ptx_scene* scene, int64_t out[5]);

/* The lighting mode of a scene: how a path sums emission and what a Diffuse scatter samples.  Sticky state of the handle (default
 * PTX_LIGHTING_REFERENCE), read by every entry point that shades -- ptx_render, _multi, _raw_device, _passes_device, _pixels_device,
 * _progressive, _adaptive, ptx_trace_samples, ptx_debug_first_scatter -- and not by ptx_ppm_render; ptx_scene_replicate copies it, and
 * the replicas a scene owns (ptx_render with n_gpus > 1) follow it.
 *   REFERENCE   the reference's text: Pdf.diffuse, emit0' = a * emit0 + emit (integrator.ml:46,65).  With real emitters that formula
 *               is order-reversed: it scales the emission of EARLIER hits by the attenuation of LATER ones.
 *   PATH_ORDER  Pdf.diffuse, emit0' = fma(attn0, emit, emit0): every hit's emission weighted by what came BEFORE it.  On a scene
 *               without emitters this is REFERENCE (there is no emission to order).
 *   SAMPLED     PATH_ORDER with diffuse_plus_light = 1/2 cosine + 1/2 the emissive triangles, sampled uniformly by area from the hit's
 *               own two sampler dimensions (the sampler's dimension stays 2 + 2 * max_bounces).  The light list is built the first time
 *               this mode is set: the tree triangles whose material has a non-zero emit, in build-list order.  Floor triangles are
 *               not sampled, and emissive spheres only with ptx_scene_set_sphere_light_sampling (they still emit when hit; the cosine
 *               half keeps the estimator unbiased).
 *               PTX_ERR_ARG when the scene has no emissive tree triangle or more than PTX_MAX_LIGHT_TRIANGLES of them.
 *               (With ptx_scene_set_environment_sampling on, a scene without emissive tree triangles is accepted and the environment is
 *               sampled too: see there.  With ptx_scene_set_sphere_light_sampling on, likewise, and the emissive spheres are sampled
 *               beside the triangles: see there.)
 * A host-only scene accepts the call (the light list can be inspected without a GPU).  PTX_ERR_STATE while a render runs on the
 * scene (from a progress or update callback); PTX_ERR_ARG for an unknown mode. */
#define PTX_LIGHTING_REFERENCE 0
#define PTX_LIGHTING_PATH_ORDER 1
#define PTX_LIGHTING_SAMPLED 2
#define PTX_MAX_LIGHT_TRIANGLES 64
int32_t ptx_scene_set_lighting(ptx_scene* scene, int32_t mode);
/* The mode last set and, once PTX_LIGHTING_SAMPLED has been set, the light list's length and total area (0 and 0.0 before).  Any
 * out pointer may be NULL. */
int32_t ptx_scene_lighting(const ptx_scene* scene, int32_t* mode_out, int32_t* n_light_triangles_out, double* light_area_out);

/* Replaces Integrator.render (integrator.ml:130-156) for the whole image on one GPU:
 * rgb_out is HOST memory, width*height*3 doubles, index (y*W + x)*3 + c, y = 0 at the
 * top, post-gamma -- the contents of the reference's Bimage after render. */
int32_t ptx_render(ptx_scene* scene, const ptx_render_params* params, double* rgb_out,
                   ptx_stats* stats, ptx_progress_fn progress, void* user);

/* The same render over several GPUs of one node inside ONE process, for hosts that are a single process (the OCaml
 * executable, the C++ CLI): scenes[k] is a replica of the scene on the k-th device (ptx_scene_replicate; scenes[0]
 * may be the original), image rows are dealt in interleaved bands of params->band_rows rows (0 -> 8), one host
 * thread per scene renders its bands (integrator.ml:138-146), the raw sums travel to scenes[0]'s device as one
 * peer-to-peer copy per replica (xGMI), and the film pass runs there.  n_scenes = 1 is ptx_render bit for bit; any
 * n_scenes gives bit-identical raw sums (the sampler offset depends only on the global pixel, integrator.ml:98).
 * progress is invoked on the CALLING thread only.  Scenes may share a device (tests on a one-GPU box). */
int32_t ptx_render_multi(ptx_scene* const* scenes, int32_t n_scenes, const ptx_render_params* params,
                         double* rgb_out, ptx_stats* stats, ptx_progress_fn progress, void* user);

/* A replica of `scene` on HIP device `device`: the flattened tree / slots / materials the original kept on the host
 * are uploaded again (no second BVH build).  Independent handle: destroy it with ptx_scene_destroy. */
ptx_scene* ptx_scene_replicate(const ptx_scene* scene, int32_t device);

/* Frees the calling thread's cached GPU-BVH-builder buffers (they otherwise live as long as the thread). */
void ptx_release_workspaces(void);

/* Optional: page-lock the caller's framebuffer for as long as it will be rendered into.  ptx_render / ptx_render_multi into
 * exactly this image (rgb_out inside [image, image + n_doubles)) then fill it with ONE DMA instead of copying through a staging
 * buffer (1080p: ~1.1 ms instead of ~2.8).  The reference's image lives as long as the run (the Bimage of
 * render_command/src/render_command.ml:64-70), which is the caller this is for.  CONTRACT: the image must stay mapped until
 * ptx_image_unpin or ptx_scene_destroy -- a DMA into a registration whose pages were unmapped aborts the process -- which is
 * why the library never pins an image behind the caller's back.  One pinned image per handle (pinning another releases the
 * first).  Returns 0, or an error code (the caller may ignore it: renders then take the staged copy). */
int32_t ptx_image_pin(ptx_scene* scene, double* image, int64_t n_doubles);
int32_t ptx_image_unpin(ptx_scene* scene);

/* Device-resident form, for one rank of a multi-GPU job and for benchmarking with no
 * PCIe traffic in the timed region.  d_raw_out is DEVICE memory holding this rank's
 * rows compactly: ptx_local_rows(params) * width * 3 doubles of raw per-pixel radiance
 * sums (no filter, no gamma).  `stream` is a hipStream_t (NULL = default stream).
 * The call returns after the work is enqueued AND complete (it syncs the stream). */
int32_t ptx_local_rows(const ptx_render_params* params);
/* global image row of local row k (or -1) */
int32_t ptx_global_row(const ptx_render_params* params, int32_t local_row);
int32_t ptx_render_raw_device(ptx_scene* scene, const ptx_render_params* params,
                              double* d_raw_out, void* stream, ptx_stats* stats);

/* Film: 3x3 binomial reconstruction (Filter_kernel.Binomial order 5 radius 1,
 * filter_kernel.ml:49-85) with the reference's unnormalised image border
 * (integrator.ml:114-128), then sqrt(v / spp) (integrator.ml:152-154).
 * d_raw_full: DEVICE, height*width*3 raw sums in image row order; d_rgb_out: DEVICE. */
int32_t ptx_film_resolve_device(int32_t device, int32_t width, int32_t height,
                                int32_t samples_per_pixel, const double* d_raw_full,
                                double* d_rgb_out, void* stream);

/* The film pass reading the GATHERED multi-rank layout in place: d_gathered is DEVICE memory
 * [n_ranks][pad_rows][width][3], slice r = rank r's compact rows exactly as ptx_render_raw_device wrote them with
 * band_first = r, band_step = n_ranks, band_rows (pad_rows >= every rank's ptx_local_rows).  No un-permute copy. */
int32_t ptx_film_resolve_banded_device(int32_t device, int32_t width, int32_t height, int32_t samples_per_pixel,
                                       const double* d_gathered, int32_t n_ranks, int32_t band_rows, int32_t pad_rows,
                                       double* d_rgb_out, void* stream);
/* The same pass QUEUED on `stream` without waiting for it (the twin of PTX_RENDER_ASYNC: a rank that pipelines frames). */
int32_t ptx_film_resolve_banded_queue(int32_t device, int32_t width, int32_t height, int32_t samples_per_pixel,
                                      const double* d_gathered, int32_t n_ranks, int32_t band_rows, int32_t pad_rows,
                                      double* d_rgb_out, void* stream);

/* ---- progressive rendering ----
 * The sampler offset of a sample depends only on (x, y, pass, N) (integrator.ml:98), and the raw sums add the passes in order,
 * so a frame rendered as consecutive pass slices into the same sums is bit for bit the frame rendered at once. */

/* Passes [pass_first, pass_first + pass_count) of the frame `params` describes -- params->samples_per_pixel is the frame's
 * TOTAL N, which fixes the sampler offsets -- ADDED to this rank's raw sums at d_raw_inout (never zeroed: the caller zeroes
 * them before the first slice).  d_sq_inout (DEVICE, nullable, same layout) receives the sums of the squared per-sample
 * contributions in the same pass order (s = s + c * c), for ptx_pixel_error_device.  Bands, `stream` and PTX_RENDER_ASYNC as
 * in ptx_render_raw_device; ptx_render_raw_device is the range [0, N) with zeroing.  PTX_ERR_ARG for a range outside
 * [0, N) or pass_count < 1. */
int32_t ptx_render_passes_device(ptx_scene* scene, const ptx_render_params* params, int32_t pass_first, int32_t pass_count,
                                 double* d_raw_inout, double* d_sq_inout, void* stream, ptx_stats* stats);

/* Per-pixel, per-channel standard error of the pixel's sample mean after k = passes_done passes, from the DEVICE sums S1
 * (d_raw) and S2 (d_sq) of `rows` x `width` pixels: se = sqrt(max(0, S2 - S1 * S1 / k) / (k (k - 1))) for k >= 2, +inf for
 * k < 2 -- linear radiance, before the film and the gamma.  d_err_out (DEVICE, nullable) receives se, 3 per pixel;
 * *rel_err_out (HOST, nullable) the frame summary sqrt(sum se^2) / sqrt(sum (S1 / k)^2), 0 when both sums are 0, +inf for
 * k < 2, reduced in a fixed order (the same sums give the same bits on every run).  se is the estimate for INDEPENDENT samples;
 * the sampler is a low-discrepancy sequence, so it usually OVERESTIMATES the error of the rendered mean.  Waits for `stream`. */
int32_t ptx_pixel_error_device(int32_t device, int32_t width, int32_t rows, int32_t passes_done, const double* d_raw,
                               const double* d_sq, double* d_err_out, double* rel_err_out, void* stream);

typedef struct ptx_progressive_params {
  int32_t passes_per_update; /* K >= 1: an update after every K passes, and after the last */
  int32_t want_error;        /* 1: keep the square sums and compute rel_err (and err_out) at every update */
  double target_rel_err;     /* > 0 (needs want_error): stop at the first update with rel_err <= this; 0 = never */
} ptx_progressive_params;

/* Called on the CALLING thread after every update with the passes done so far (k), the frame's rel_err (NaN without
 * want_error), the image filmed from k passes (rgb_out) and its per-pixel error (err_out, or NULL).  Non-zero stops the render. */
typedef int32_t (*ptx_update_fn)(void* user, int32_t passes_done, double rel_err, const double* rgb, const double* err);

/* ptx_render as a sequence of updates, on ONE GPU (params->n_gpus > 1: PTX_ERR_ARG).  After every passes_per_update passes and
 * after the last, the running sums are filmed with spp = k (ptx_film_resolve_device), the image is copied into rgb_out (HOST,
 * W*H*3; a pinned image takes one DMA), err into err_out (HOST, nullable, needs want_error), and on_update (nullable) is
 * called.  It stops when the callback returns non-zero, when rel_err <= target_rel_err > 0, or after N passes.  On return
 * rgb_out holds the image handed to the last callback, *passes_done_out (nullable) its k, stats->samples = W*H*k, and nothing
 * the call queued is still running (also on every error).  Run to N passes, rgb_out is ptx_render's image bit for bit.  The
 * film and the copy of update j overlap the bounces of the next slice, so an early stop discards at most one slice of work. */
int32_t ptx_render_progressive(ptx_scene* scene, const ptx_render_params* params, const ptx_progressive_params* progressive,
                               double* rgb_out, double* err_out, int32_t* passes_done_out, ptx_stats* stats,
                               ptx_update_fn on_update, void* user);

/* ---- adaptive sampling ----
 * A pixel that stops after n passes holds the pass-order prefix of its own N-pass sums (the sampler offset depends only on
 * (x, y, pass, N)), so every pixel's sums are bit for bit ptx_render_passes_device's over [0, n).  All of these run on ONE GPU over
 * the whole image (n_gpus > 1 or band_step > 1: PTX_ERR_ARG). */

/* Passes [pass_first, pass_first + pass_count) of the N-pass frame for the DEVICE list d_pixels of n_pixels DISTINCT indices
 * y * W + x, ADDED to the whole-image sums d_raw_inout (and the squares to d_sq_inout, DEVICE, nullable), in pass order as
 * ptx_render_passes_device adds them; unlisted pixels are untouched.  PTX_ERR_ARG for a bad pass range, n_pixels outside
 * [0, W*H], or an index outside [0, W*H) -- checked on the device before anything is queued, the sums left untouched (the check
 * waits for `stream`).  stats->samples = n_pixels * pass_count.  `stream` and PTX_RENDER_ASYNC as in ptx_render_raw_device. */
int32_t ptx_render_pixels_device(ptx_scene* scene, const ptx_render_params* params, int32_t pass_first, int32_t pass_count,
                                 const int32_t* d_pixels, int64_t n_pixels, double* d_raw_inout, double* d_sq_inout, void* stream,
                                 ptx_stats* stats);

/* ptx_film_resolve_device with a per-pixel pass count d_passes (DEVICE, W*H, every count >= 1).  Where all in-image taps of the
 * 3x3 film have the same count n, the pixel is ptx_film_resolve_device's with spp = n, bit for bit; elsewhere it is
 * sqrt(sum w * (S(q) * (1 / n(q)))), the film of each tap's own mean.  Waits for `stream`. */
int32_t ptx_film_resolve_counts_device(int32_t device, int32_t width, int32_t height, const double* d_raw, const int32_t* d_passes,
                                       double* d_rgb_out, void* stream);

/* ptx_pixel_error_device with the pixel's own pass count k = d_passes[p] (DEVICE, rows * W): se per pixel and channel into
 * d_err_out (nullable), *rel_err_out = sqrt(sum se^2) / sqrt(sum (S1 / k)^2) in the same fixed order (0 when both sums are 0;
 * +inf when some pixel has k < 2).  A uniform map gives ptx_pixel_error_device's bits.  Waits for `stream`. */
int32_t ptx_pixel_error_counts_device(int32_t device, int32_t width, int32_t rows, const int32_t* d_passes, const double* d_raw,
                                      const double* d_sq, double* d_err_out, double* rel_err_out, void* stream);

typedef struct ptx_adaptive_params {
  int32_t min_passes;       /* M >= 2: round 1 gives every pixel passes [0, min(M, N)) */
  int32_t passes_per_round; /* K >= 1: every later round gives the pixels still active K more passes (the last one fewer) */
  double target_rel_err;    /* T >= 0: a pixel stops once e <= T * d (below); 0 = no pixel stops before N */
  double radiance_floor;    /* F >= 0: d is at least this, so dark pixels stop on an absolute error */
} ptx_adaptive_params;

/* Called on the CALLING thread after every round: its number (1, 2, ...), the passes the round ended at (b), how many pixels the
 * next round renders (0: none, the render ends), the samples so far (the sum of the count map), the frame's rel_err, the image,
 * its per-pixel error (or NULL) and the count map (or NULL).  Non-zero stops the render. */
typedef int32_t (*ptx_round_fn)(void* user, int32_t round, int32_t passes_done, int64_t active_next, int64_t samples,
                                double rel_err, const double* rgb, const double* err, const int32_t* passes);

/* ptx_render with per-pixel pass counts.  Round 1 gives every pixel passes [0, min(M, N)).  After a round that ended at b < N,
 * the next round gives the pixels of that round that have NOT converged passes [b, min(b + K, N)); the render ends at N, when no
 * pixel is left, or when on_round (nullable) returns non-zero.  The rule, for a pixel with k passes and sums S1_c, S2_c:
 *   se_c = sqrt(max(0, S2_c - S1_c * S1_c / k) / (k (k - 1))),  m_c = S1_c / k,  e = sqrt((se_r^2 + se_g^2) + se_b^2),
 *   d = max(sqrt((m_r^2 + m_g^2) + m_b^2), F),  converged <=> T > 0 and e <= T * d.
 * After every round the sums are filmed with the count map (ptx_film_resolve_counts_device) into rgb_out (HOST, W*H*3), the
 * per-pixel error goes to err_out (HOST, nullable; ptx_pixel_error_counts_device), the map to passes_out (HOST, W*H, nullable),
 * and on_round is called.  On return they hold what the last callback saw, stats->samples is the sum of the map, and nothing the
 * call queued is still running (also on every error).  A round over the whole image is a plain slice; the next list is selected
 * on the device in a fixed order (8x8-tile order, no atomics), so a frame gives the same map on every run.  With T = 0 every
 * pixel gets N passes and rgb_out is ptx_render's image bit for bit.  PTX_ERR_ARG for M < 2, K < 1, T or F negative or NaN. */
int32_t ptx_render_adaptive(ptx_scene* scene, const ptx_render_params* params, const ptx_adaptive_params* adaptive,
                            double* rgb_out, double* err_out, int32_t* passes_out, ptx_stats* stats, ptx_round_fn on_round,
                            void* user);

/* ---- first-hit feature buffers and the variance-guided a-trous denoiser ----
 * Image-space passes beside the integrator: no render entry point above changes, and the ABI version stays 6 (only entry points and
 * structs were added).  Everything here runs on ONE GPU over the whole image. */

/* The feature record of one sample = what the FIRST hit of its camera ray shows (the first hit, not the first non-specular one: a
 * mirror or a glass ball shows its own surface).  8 doubles per pixel, index (y * W + x) * 8:
 *   [0..2] albedo  at a hit: Texture.eval of the hit material's texture at the hit's texture coordinates for Lambertian and Metal
 *                  (the texture colour, not the Schlick-tinted attenuation), (1, 1, 1) for Dielectric; at a miss: Scene.background
 *                  of the ray
 *   [3..5] normal  the facing shading normal (Sphere.hit / Triangle.Hit.to_hit, negated when hit_front is false; floor triangles
 *                  included); 0 at a miss
 *   [6]    depth   t_hit; 0 at a miss
 *   [7]    hits    1 at a hit, 0 at a miss */
#define PTX_FEATURE_DOUBLES 8 /* albedo r g b, normal x y z, depth, hits */

/* The records of the camera rays of every sample (x, y, pass), pass in [pass_first, pass_first + pass_count), of the frame `params`
 * describes -- the ray the render traces: sampler offset y * W + x + pass * N, dimensions 0 and 1, Camera.ray -- ADDED to
 * d_feat_inout (DEVICE, W * H * 8 doubles, never zeroed: the caller zeroes it before the first slice) per pixel in pass order, so
 * slices of a range give the range's sums bit for bit, and no float atomics are used: the same inputs give the same bits on every
 * run.  Every value comes from the functions the render's own first segment uses (same bits).  max_bounces fixes the sampler's
 * dimension as in a render.  PTX_ERR_ARG for band_step > 1 or n_gpus > 1 and for a range outside [0, N) or pass_count < 1.
 * stats->samples = W * H * pass_count.  `stream` and PTX_RENDER_ASYNC as in ptx_render_passes_device; queued calls on one handle
 * share its feature workspace and must be ordered on ONE stream.  d_feat_inout must be 16-byte aligned (the records move as
 * 16-byte accesses; any hipMalloc'ed buffer is). */
int32_t ptx_render_features_device(ptx_scene* scene, const ptx_render_params* params, int32_t pass_first, int32_t pass_count,
                                   double* d_feat_inout, void* stream, ptx_stats* stats);

#define PTX_DENOISE_DEMODULATE 1
typedef struct ptx_denoise_params {      /* 40 bytes */
  int32_t levels;             /* L, 0..8: a-trous iterations, step 2^l */
  int32_t normal_power_log2;  /* m, 0..8: w_n = max(0, n_p . n_q)^(2^m) by m squarings */
  int32_t feature_passes;     /* ptx_render_denoised only: features from passes [0, min(F, k)); 0 = all */
  int32_t flags;              /* PTX_DENOISE_DEMODULATE */
  double sigma_luminance, sigma_depth, sigma_albedo;   /* each > 0 and finite */
} ptx_denoise_params;
/* levels 5, normal_power_log2 5, feature_passes 8, flags PTX_DENOISE_DEMODULATE, sigmas 4.0, 0.05, 0.2 */
int32_t ptx_denoise_defaults(ptx_denoise_params* out);

/* The edge-avoiding a-trous wavelet filter, guided by the feature sums and the per-pixel standard error.  DEVICE inputs: the raw
 * sums S1 (d_raw, W*H*3), se per channel exactly as ptx_pixel_error_device / ptx_pixel_error_counts_device write it (d_err, W*H*3),
 * the feature sums of kf = feature_passes_done >= 1 passes (d_feat, W*H*8); k = passes_done, or the pixel's own d_passes[p]
 * (DEVICE, nullable, every count >= 2: what ptx_render_adaptive leaves).  k < 2 is PTX_ERR_ARG (se would be infinite, and an
 * infinite variance times a zero weight is NaN); a count map is not checked.  Output d_raw_out (DEVICE, W*H*3, not d_raw): the
 * denoised SUMS, mean * k(p), so ptx_film_resolve_device / ptx_film_resolve_counts_device apply unchanged.  levels = 0 copies
 * d_raw bit for bit.  Waits for `stream`.  PTX_ERR_ARG for levels or normal_power_log2 outside 0..8, unknown flags, a sigma that is
 * not > 0 and finite.  d_feat must be 16-byte aligned (as ptx_render_features_device's buffer is).
 *
 * The rule, operation for operation (binary64, no contraction; every sum over taps starts at 0 and runs in row-major tap order,
 * j outer, i inner; a tap outside the image is skipped):
 *   prepare   kd = (double)k, kfd = (double)kf;  m_c = S1_c / kd;  var_c = se_c * se_c;
 *             a_c = A_c / kfd, n = N / kfd, z = Z / kfd (A, N, Z: the albedo, normal and depth sums), h = the hits sum;
 *             D_c = (DEMODULATE and a_c > 2^-7) ? a_c : 1;  c_c = m_c / D_c;
 *             V = (var_r / (D_r * D_r) + var_g / (D_g * D_g)) + var_b / (D_b * D_b)
 *   level l = 0 .. L-1, step s = 2^l, for every pixel p from the level's input (c, V):
 *             lambda(q) = (c_r(q) + c_g(q)) + c_b(q)
 *             Vbar = sum over q = p + (i, j), i, j in -1..1, of (b_j * b_i) * V(q), b = (1/4, 1/2, 1/4) (not renormalised)
 *             den = (sigma_l * sigma_l) * Vbar + 1e-12
 *             for q = p + s * (i, j), i, j in -2..2, with h5 = (1/16, 1/4, 3/8, 1/4, 1/16):
 *               w_n = 1 when h(p) = 0 and h(q) = 0; else d = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z,
 *                     w_n = d > 0 ? d : 0, then w_n = w_n * w_n, m times
 *               r = (z_p - z_q) / (sigma_z * (|z_p| + |z_q|) + 1e-300);  w_z = 1 / (1 + r * r)
 *               e = a_p - a_q;  w_a = 1 / (1 + ((e_r * e_r + e_g * e_g) + e_b * e_b) / (sigma_a * sigma_a))
 *               t = lambda(p) - lambda(q);  w_l = 1 / (1 + (t * t) / den)
 *               w = (h5_j * h5_i) * (((w_n * w_z) * w_a) * w_l)
 *               sw = sw + w;  sc_c = sc_c + w * c_c(q);  sv = sv + (w * w) * V(q)
 *             c'_c = sc_c / sw;  V' = sv / (sw * sw)       (the centre tap has w = (3/8)^2, so sw > 0)
 *   finish    out_c = (c_c * D_c) * kd */
int32_t ptx_denoise_device(int32_t device, int32_t width, int32_t height, const ptx_denoise_params* denoise,
                           int32_t passes_done, const int32_t* d_passes /* nullable, W*H, each >= 2 */,
                           int32_t feature_passes_done /* kf >= 1 */,
                           const double* d_raw, const double* d_err, const double* d_feat,
                           double* d_raw_out, void* stream);

/* ptx_render_progressive whose updates show the DENOISED image.  The square sums are always kept (progressive->want_error is
 * implied; target_rel_err works as there, on the un-denoised sums); passes_per_update >= 2 is required.  Beside every slice
 * [first, first + count) the feature slice [first, min(first + count, F)) is rendered while first < F (F = denoise->feature_passes,
 * 0 = N).  An update after k passes is: ptx_pixel_error_device, ptx_denoise_device with kf = min(F, k) into a buffer the scene
 * owns, ptx_film_resolve_device of the denoised sums with spp = k.  rgb_out: the denoised image; err_out (HOST, nullable): the
 * un-denoised se; feat_out (HOST, nullable, W*H*8): the feature MEANS, sums / kf.  The callback sees the denoised image and the
 * un-denoised se.  Early stop, the drain on every exit, PTX_ERR_STATE for ptx_scene_set_lighting from a callback, and the refusal
 * of a host-only scene are ptx_render_progressive's.  With levels = 0, run to N passes, rgb_out is ptx_render's image bit for bit. */
int32_t ptx_render_denoised(ptx_scene* scene, const ptx_render_params* params, const ptx_progressive_params* progressive,
                            const ptx_denoise_params* denoise, double* rgb_out, double* err_out /* nullable */,
                            double* feat_out /* nullable, HOST, W*H*8 means */, int32_t* passes_done_out, ptx_stats* stats,
                            ptx_update_fn on_update, void* user);

/* ---- the film at any order and radius ----
 * Filter_kernel.Binomial.create ~order ~pixel_radius (filter_kernel.ml:49-85) in full, in front of Film_tile at any radius
 * (film_tile.ml:15-45).  The default (5, 1, flags 0) is the film every entry point above applies, and runs through the same kernels.
 *
 * Accepted: 1 <= order <= PTX_FILM_MAX_ORDER, 0 <= pixel_radius <= PTX_FILM_MAX_RADIUS, order >= 2 * pixel_radius + 1,
 * flags within PTX_FILM_RENORMALISE, reserved = 0; everything else is PTX_ERR_ARG.  Why order < 2 * pixel_radius + 1 is refused:
 * there a tap covers less than one cell of the binomial row, the reference's `k = 0` branch (one minus the fractional part of the
 * tap's start) wins over its `k = len - 1` branch for such one-cell taps, and the kernel comes out lopsided -- (1, 1) gives
 * [1/2, 1/3, 1/6], (3, 2) gives [0.208, 0.167, 0.333, 0.167, 0.125].  From order >= 2 * pixel_radius + 1 on the reference's rule is
 * the plain overlap rule (tap i covers [i * order / f, (i + 1) * order / f) of the row, f = 2 * pixel_radius + 1): the 1-D weights
 * are positive and palindromic bit for bit, and the 2-D weights sum to 1 within 2.3e-16.
 *
 * The weights: the reference's sums in exact rationals, float_of_num (to nearest), total = the left fold of + from 0.0 over the
 * 2r + 1 values, w[i] = w[i] / total; the 2-D weight is W[j][i] = w[j] * w[i], one multiplication.
 *
 * The rule, operation for operation (binary64, no contraction), r = pixel_radius, w = the 1-D weights, S = the raw sums:
 *   for pixel (x, y):  acc_c = 0; ws = 0; clipped = false
 *     for dy = -r..r (outer), dx = -r..r (inner), W = w[dy + r] * w[dx + r]:
 *       (sx, sy) = (x - dx, y - dy); outside the image: clipped = true, skip
 *       acc_c = fma(W, S_c(sx, sy), acc_c);  ws = ws + W
 *     if PTX_FILM_RENORMALISE and clipped: acc_c = acc_c / ws
 *     out_c = sqrt(acc_c * (1.0 / spp))
 * Without PTX_FILM_RENORMALISE the border keeps the reference's darkening (integrator.ml:114-128 drops the taps that fall outside
 * the image: a 3x3 corner keeps about 59 %).  At (5, 1, 0) this is ptx_film_resolve_device bit for bit.
 * Banded: S is read in place from the gathered layout, as ptx_film_resolve_banded_device does; band_rows may be smaller than r.
 * Counts: `same` holds exactly when every in-image tap of the (2r + 1)^2 window has the centre's count n.  If same: the rule above
 * with spp = n.  Otherwise acc_c = fma(W, S_c(q) * (1.0 / n(q)), acc_c), then the renormalisation, then out_c = sqrt(acc_c). */
#define PTX_FILM_MAX_ORDER 16
#define PTX_FILM_MAX_RADIUS 7
#define PTX_FILM_RENORMALISE 1
typedef struct ptx_film_params { /* 16 bytes */
  int32_t order;        /* Binomial.create ~order */
  int32_t pixel_radius; /* ... ~pixel_radius: a (2r + 1)^2 window */
  int32_t flags;        /* PTX_FILM_RENORMALISE */
  int32_t reserved;     /* 0 */
} ptx_film_params;
/* order 5, pixel_radius 1, flags 0 */
int32_t ptx_film_defaults(ptx_film_params* out);
/* Host only, needs no device: the normalised 1-D weights (w1d_out, 2r + 1 doubles) and, nullable, their outer product (w2d_out,
 * (2r + 1)^2 doubles, row-major).  PTX_ERR_ARG for NULL film or w1d_out and for refused parameters. */
int32_t ptx_film_weights(const ptx_film_params* film, double* w1d_out, double* w2d_out);
/* The film of a scene: sticky state of the handle, like the lighting mode (NULL = the defaults).  Every entry point that films
 * through the scene reads it -- ptx_render (a pinned image included), ptx_render_multi and n_gpus > 1 (the film of scenes[0] governs:
 * the film runs there), ptx_render_progressive, ptx_render_adaptive, ptx_render_denoised; the scene-less ptx_film_resolve_device /
 * _banded_device / _banded_queue / _counts_device stay (5, 1, 0).  A host-only scene accepts it; PTX_ERR_STATE while a render runs on
 * the scene (from a progress / update / round callback); ptx_scene_replicate copies it. */
int32_t ptx_scene_set_film(ptx_scene* scene, const ptx_film_params* film);
int32_t ptx_scene_film(const ptx_scene* scene, ptx_film_params* out);
/* ptx_film_resolve_device / _banded_device / _counts_device with a film (NULL = the defaults).  Each waits for `stream`. */
int32_t ptx_film_resolve_ex_device(int32_t device, int32_t width, int32_t height, int32_t samples_per_pixel,
                                   const ptx_film_params* film, const double* d_raw_full, double* d_rgb_out, void* stream);
int32_t ptx_film_resolve_banded_ex_device(int32_t device, int32_t width, int32_t height, int32_t samples_per_pixel,
                                          const ptx_film_params* film, const double* d_gathered, int32_t n_ranks, int32_t band_rows,
                                          int32_t pad_rows, double* d_rgb_out, void* stream);
int32_t ptx_film_resolve_counts_ex_device(int32_t device, int32_t width, int32_t height, const ptx_film_params* film,
                                          const double* d_raw, const int32_t* d_passes, double* d_rgb_out, void* stream);

/* ---- image textures and a lat-long environment map ----
 * Texture.t stops at one colour and a two-colour checker (texture.ml:16-31), Scene.background at a closure; these two sticky
 * setters put a picture on a texture entry and light the scene with a sky image.  Only entry points and one struct are added: no
 * existing struct changes, the ABI version stays 6, and a scene without an image launches the kernels it launched before.
 *
 * An image is width x height texels of three binary64 values, linear (no colour-space conversion): texel (ix, iy) is
 * rgb[3 * (iy * width + ix) ..], row 0 is v = 0.  1 <= width, height <= PTX_IMAGE_MAX_SIZE, every value finite.  The library
 * copies the texels (on the device: one 32-byte record {r, g, b, -} per texel, bit for bit).
 *
 * The rule, operation for operation (binary64, no fma, no contraction), for texture coordinates (u, v), W = width, H = height:
 *   wrap of an integer index i on an axis of n texels:  repeat ((i % n) + n) % n;  clamp min(max(i, 0), n - 1)
 *     (PTX_IMAGE_REPEAT_U / _V choose repeat for that axis, otherwise it clamps)
 *   p = u * (double)W, q = v * (double)H;  a product that is NaN or not below 2^62 in magnitude is replaced by 0.0
 *   nearest:   ix = wrap((long long)p), iy = wrap((long long)q): truncation toward zero, the checker's Float.to_int;
 *              the colour is texel (ix, iy)
 *   bilinear:  x = p - 0.5;  x0 = floor(x);  fx = x - x0;  ix0 = wrap((long long)x0), ix1 = wrap((long long)x0 + 1)
 *              y = q - 0.5;  y0 = floor(y);  fy = y - y0;  iy0, iy1 likewise;  then per channel, c(i, j) = texel (i, j):
 *              top = c(ix0, iy0) * (1 - fx) + c(ix1, iy0) * fx
 *              bot = c(ix0, iy1) * (1 - fx) + c(ix1, iy1) * fx
 *              result = top * (1 - fy) + bot * fy
 * The environment, for a ray direction d and the caller's row-major 3x3 matrix R (camera space -> environment space; geometry
 * arrives in camera space):
 *   e = normalize(d) as the sky gradient does;  m_k = (R[3k] * e.x + R[3k+1] * e.y) + R[3k+2] * e.z, k = 0, 1, 2
 *   u = (pi + atan2(-m.z, m.x)) * (1 / (2 pi));  v = acos(-min(max(m.y, -1), 1)) * (1 / pi)
 * -- Sphere.tex_coord (sphere.ml:25-33) with the functions of pt_math.h: the environment is the texture of an infinitely large
 * sphere seen from inside -- then the image rule with repeat in u and clamp in v.  A miss returns that colour where it returned
 * Scene.background before.
 *
 * Both setters are sticky state of the handle, read by everything that shades through the scene: the ptx_render family
 * (progressive, adaptive, denoised, n_gpus > 1), ptx_trace_samples, ptx_debug_first_scatter, ptx_render_features_device (the albedo
 * is the texel; a miss's albedo the environment colour), ptx_ppm_render's shading, all three lighting modes.  The replicas a scene
 * owns follow it, and ptx_scene_replicate copies both.  A host-only scene accepts a valid call, as ptx_scene_set_lighting does.
 * Every argument is checked before any device call.  PTX_ERR_STATE while a render runs on the scene; a setter waits for the
 * device (frames queued with PTX_RENDER_ASYNC have finished when it returns).
 * A scene with an image or an environment takes the walk-first kernels' image instantiations: no shade-first
 * order, no per-octant LDS image, no camera tile lists.
 * Out of scope: mip maps and anisotropic filtering, 8-bit or binary32 texels, image decoders other than the hosts' PFM reader,
 * image-driven emission, roughness or normals.  (Importance-sampling the environment: ptx_scene_set_environment_sampling below.) */
#define PTX_IMAGE_BILINEAR 1
#define PTX_IMAGE_REPEAT_U 2
#define PTX_IMAGE_REPEAT_V 4
#define PTX_IMAGE_MAX_SIZE 16384
typedef struct ptx_image { /* 24 bytes */
  int32_t width, height;
  int32_t flags;    /* PTX_IMAGE_*; unknown bits are PTX_ERR_ARG */
  int32_t reserved; /* 0 */
  const double* rgb; /* width * height * 3; NULL in what the getters return */
} ptx_image;
/* From now on every material that points at entry texture_index of the scene's texture table evaluates the image (an entry declared
 * solid included); NULL restores the descriptor's texture.  A texture_index the scene's texture table does not have is PTX_ERR_ARG
 * ("texture index ... out of range ..."), from the setter and from the getter alike, and changes nothing. */
int32_t ptx_scene_set_texture_image(ptx_scene* scene, int32_t texture_index, const ptx_image* image);
/* NULL image restores the descriptor's background; NULL R is the identity; of the flags only PTX_IMAGE_BILINEAR is accepted. */
int32_t ptx_scene_set_environment(ptx_scene* scene, const ptx_image* image, const double R[9]);
/* Dimensions and flags of what is set, rgb NULL; width 0 = none.  R_out (nullable) receives the matrix (the identity when none). */
int32_t ptx_scene_texture_image(const ptx_scene* scene, int32_t texture_index, ptx_image* out);
int32_t ptx_scene_environment(const ptx_scene* scene, ptx_image* out, double R_out[9]);
/* Diagnostics, in the family of ptx_math_eval: the device's own evaluation functions on explicit inputs.  uv: n x 2, dirs: n x 3,
 * rgb_out: n x 3, HOST.  ptx_texture_eval on an entry without an image evaluates its solid or checker texture;
 * ptx_environment_eval without an environment evaluates the descriptor's background. */
int32_t ptx_texture_eval(ptx_scene* scene, int32_t texture_index, int64_t n, const double* uv, double* rgb_out);
int32_t ptx_environment_eval(ptx_scene* scene, int64_t n, const double* dirs, double* rgb_out);

/* ---- importance-sampling the environment in PTX_LIGHTING_SAMPLED ----
 * Integrator.create ~diffuse_plus_light (integrator.ml:48-66) with a light density over the environment image: a sky whose sun covers
 * a few texels is found by sampling it, not by scattering alone.  Only entry points are added; the ABI version stays 6.
 *
 * ptx_scene_set_environment_sampling(scene, on): sticky state of the handle, default off; the replicas a scene owns follow it and
 * ptx_scene_replicate copies it; a host-only scene accepts it.  Turning it on builds the density below and needs
 *   an environment (ptx_scene_set_environment with an image),
 *   a matrix R with max |R R^T - I| <= 1e-9 (row-major products, (R[3i] R[3j] + R[3i+1] R[3j+1]) + R[3i+2] R[3j+2]): the density
 *     assumes a rotation,
 *   a total weight T that is finite and greater than 0;
 * anything else is PTX_ERR_ARG with a message that names the rule, and nothing changes.  PTX_ERR_STATE while a render runs on the scene.
 * While it is on: ptx_scene_set_lighting(PTX_LIGHTING_SAMPLED) also accepts a scene without emissive tree triangles (the light half is
 * then the environment alone); ptx_scene_set_environment with a new image or R rebuilds the density, and refuses (the old state kept)
 * an image or R that fails the conditions above; clearing the environment (NULL) is PTX_ERR_STATE, "turn environment sampling off
 * first"; turning sampling off while the mode is PTX_LIGHTING_SAMPLED and nothing else is left to sample -- the light list is empty and
 * sphere light sampling (below) is off -- is PTX_ERR_STATE likewise ("set another lighting mode first"); with sphere light sampling on
 * it is accepted, and the light half is then the sphere lights alone.  In modes 0 and 1 the flag has no effect on a pixel.
 *
 * The rule, operation for operation (binary64, no fma, no contraction; sin, cos, atan2, acos are pt_math.h's), W x H the image:
 *   The density (built on the host), texel (ix, iy) = (r, g, b):
 *     lum = (r + g) + b, taken as 0.0 unless lum > 0;   s_iy = sin(pi * (((double)iy + 0.5) / (double)H));   w(ix, iy) = lum * s_iy
 *     c_iy[ix] = c_iy[ix - 1] + w(ix, iy) from 0.0, left to right;  r_iy = c_iy[W - 1]
 *     m[iy] = m[iy - 1] + r_iy from 0.0, top to bottom;              T = m[H - 1]
 *   Sample, from (a, b) in [0, 1)^2:
 *     x = a * T;  iy = the first row with x < m[iy], or the last row with r_iy > 0 if there is none
 *     fy = min((x - (iy > 0 ? m[iy - 1] : 0.0)) / r_iy, 1.0)
 *     y = b * r_iy;  ix = the first column with y < c_iy[ix], or the last column of the row with w > 0 if there is none
 *     fx = min((y - (ix > 0 ? c_iy[ix - 1] : 0.0)) / w(ix, iy), 1.0)
 *     u = ((double)ix + fx) / (double)W;  v = ((double)iy + fy) / (double)H
 *     al = u * (2.0 * pi) - pi;  th = v * pi;  (sa, ca) = sincos(al);  (st, ct) = sincos(th)
 *     m = (st * ca, -ct, -(st * sa));  d_k = (R[k] * m.x + R[3 + k] * m.y) + R[6 + k] * m.z, k = 0, 1, 2 (R^T m);  direction = normalize(d)
 *     (both searches are binary searches whose result is the linear "first with" above: m and c_iy never decrease)
 *   Density of a direction w (per solid angle):
 *     e = normalize(w);  m = R e, u, v as in the environment rule above
 *     ix = min((long long)(u * (double)W), W - 1), iy = min((long long)(v * (double)H), H - 1), either taken as 0 when the product is NaN
 *     st = sin(v * pi);  pd = st > 0 ? ((w(ix, iy) / T) * ((double)W * (double)H)) / ((2.0 * (pi * pi)) * st) : 0.0
 *     -- piecewise constant per texel whatever PTX_IMAGE_BILINEAR says: the cosine half keeps the estimator unbiased.
 *   The mixture, at a Diffuse scatter in PTX_LIGHTING_SAMPLED with sampling on, (su, sv) the hit's two sampler dimensions:
 *     with light triangles:  su < 0.25         the triangle rule with its 2u := 4.0 * su
 *                            0.25 <= su < 0.5  the environment on (4.0 * su - 1.0, sv)
 *                            otherwise         the cosine half on (2.0 * su - 1.0, sv)
 *                            divisor = (0.5 * diffuse_pd + 0.25 * light_pd) + 0.25 * env_pd
 *     environment only:      su < 0.5 the environment on (2.0 * su, sv), otherwise the cosine half;
 *                            divisor = 0.5 * diffuse_pd + 0.5 * env_pd
 *     The environment direction is rotated into shader space and back exactly as the triangle direction is; env_pd is evaluated for
 *     the world direction the scattered ray will have.  Everything else of PTX_LIGHTING_SAMPLED, where a path ends included, is unchanged.
 * What it does not help: an environment behind glass or seen in a mirror (specular scatters do not sample), and the
 * bilinear interpolant's departure from the per-texel density (variance only).  No shadow rays, no multiple importance sampling. */
int32_t ptx_scene_set_environment_sampling(ptx_scene* scene, int32_t on);
/* The flag and, while it is on, the total weight T (0.0 while off).  Either out pointer may be NULL. */
int32_t ptx_scene_environment_sampling(const ptx_scene* scene, int32_t* on_out, double* total_out);
/* Host-only inspection of the density (needs sampling on; works on a host-only scene): marginal_out (nullable) H doubles m[iy],
 * conditional_out (nullable) H x W doubles c_iy[ix], row-major.  PTX_ERR_STATE while sampling is off. */
int32_t ptx_environment_distribution(const ptx_scene* scene, double* marginal_out, double* conditional_out);
/* Diagnostics, in the family of ptx_environment_eval: the shade step's own two device functions on explicit HOST inputs (sampling must
 * be on).  ab: n x 2 -> dirs_out: n x 3 and texel_out (nullable): n x 2 {ix, iy} as drawn;  dirs: n x 3 -> pd_out: n. */
int32_t ptx_environment_sample(ptx_scene* scene, int64_t n, const double* ab, double* dirs_out, int32_t* texel_out);
int32_t ptx_environment_pdf(ptx_scene* scene, int64_t n, const double* dirs, double* pd_out);

/* ---- cone-sampling emissive spheres in PTX_LIGHTING_SAMPLED ----
 * The light half of Integrator.create ~diffuse_plus_light with the scene's emissive tree spheres beside its emissive triangles, under one
 * table: a small lamp sphere is found by sampling the cone it spans, not by scattering alone.  Only entry points are added: no struct
 * changes and the ABI version stays 6.
 *
 * ptx_scene_set_sphere_light_sampling(scene, on): sticky state of the handle, default off; the replicas a scene owns follow it and
 * ptx_scene_replicate copies it; a host-only scene accepts it.  Turning it on needs at least one emissive tree sphere (a sphere whose
 * material has a non-zero emit) and at most PTX_MAX_LIGHT_SPHERES of them: anything else is PTX_ERR_ARG with a message that names the
 * count, and nothing changes.  PTX_ERR_STATE while a render runs on the scene.  While it is on,
 * ptx_scene_set_lighting(PTX_LIGHTING_SAMPLED) also accepts a scene without emissive tree triangles; turning it off while the mode is
 * PTX_LIGHTING_SAMPLED and nothing else is left to sample is PTX_ERR_STATE ("set another lighting mode first").  While it is off nothing
 * differs from a handle that never heard of it: emissive spheres emit when hit and none is sampled.  In modes 0 and 1 the flag has no
 * effect on a pixel.
 *
 * The rule, operation for operation (binary64, no contraction; dot a b = fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)) as everywhere in the
 * shade step; sqrt is IEEE; sin, cos and the hypot inside normalize are pt_math.h's; pi = 3.14159265358979323846):
 *   The list (built on the host): the tree spheres whose material emits, in build-list order; sphere light k holds its centre c_k, r_k,
 *     r2_k = r_k * r_k and W_k = (2.0 * pi) * r2_k -- the area a point outside can see at most, what a two-sided triangle's A is.
 *     cum continues the triangles' running sum: cum_k = cum_(k-1) + W_k, starting from the triangles' A_total (0.0 without any).  The
 *     triangles' records keep their bits.  W_total = the last running sum of the joined table (triangles first, spheres behind them);
 *     it stands wherever the triangle rule says A_total.  Emission does not weight the pick.
 *   Sample, in the light half, at the point p, from the rule's (2u, v):
 *     x = 2u * W_total;  k = the first entry of the joined table with x < cum_k, or the last entry if there is none;
 *     before = cum_(k-1), 0.0 for k = 0;  u2 = min((x - before) / W_k, 1.0) (A_k for a triangle, which then goes on as the triangle rule says)
 *     k a sphere:  f = c_k - p;  d2 = dot f f;  phi = (v * 2.0) * pi;  (sn, cs) = sincos(phi)
 *       d2 <= r2_k (p inside or on the light: the whole sphere of directions, world space, no frame):
 *         z = 1.0 - 2.0 * u2;  m = 1.0 - z * z, taken as 0.0 unless m > 0;  s = sqrt(m);  w = (s * cs, s * sn, z)
 *       otherwise:
 *         s2 = r2_k / d2;  q = s2 / (1.0 + sqrt(1.0 - s2))   (1 - cos(theta_max) without the cancellation)
 *         t = u2 * q;  ct = 1.0 - t;  st = sqrt(t * (2.0 - t))
 *         w = rotate_inv (Shader_space.create (normalize f)) (st * cs, st * sn, ct)   -- the shade step's own frame rule
 *           (shader_space.ml:11-23 with Quaternion.normalize and Quaternion.transform, as at every hit)
 *     The world direction w is rotated into the hit's shader space and back exactly as the triangle direction is.
 *   Density of the world direction w at p, added to the triangles' sum (whose terms read t^2 / (W_total * |n . w|)), sphere lights in
 *   list order:
 *     f, d2 as above;  share = W_k / W_total
 *     d2 <= r2_k:  pd = pd + share / (4.0 * pi)
 *     otherwise:   bp = dot f w;  g = f - bp * w (per component);  if bp > 0 and r2_k - dot g g >= 0:  pd = pd + share / ((2.0 * pi) * q)
 *     -- the cone test is the discriminant on the perpendicular offset, not d2 - bp^2: a far, small lamp is decided without cancellation.
 *   The mixture is PTX_LIGHTING_SAMPLED's own with "the triangles" read as "the joined table": 1/2 cosine + 1/2 lights; with
 *   environment sampling on 1/2 + 1/4 + 1/4, and 1/2 + 1/2 environment when the joined table is empty.  Emission stays in path order.
 * What it does not help: lamps behind glass or seen in a mirror (specular scatters do not sample), floor triangles, scenes with more
 * than 64 lights of a kind (no light hierarchy), and a lamp hidden from the point (no shadow rays: the draw is spent on the occluder). */
#define PTX_MAX_LIGHT_SPHERES 64
int32_t ptx_scene_set_sphere_light_sampling(ptx_scene* scene, int32_t on);
/* The flag, and while it is on the number of sphere lights and W_total, the joined table's last running sum (0 and 0.0 while off).
 * ptx_scene_lighting keeps reporting the triangles' own count and area.  Any out pointer may be NULL. */
int32_t ptx_scene_sphere_lights(const ptx_scene* scene, int32_t* on_out, int32_t* n_out, double* weight_out);
/* Host-only inspection of the joined table (works on a host-only scene): triangles_out (nullable) 14 doubles per light triangle
 * {a, b, c, unit normal, A, cum} -- filled once PTX_LIGHTING_SAMPLED has been set, ptx_scene_lighting gives the count -- and
 * spheres_out (nullable) 8 doubles per sphere light {c, r, r2, W, cum, 0.0}, filled while sphere light sampling is on. */
int32_t ptx_light_table(const ptx_scene* scene, double* triangles_out, double* spheres_out);
/* Diagnostics, in the family of ptx_environment_sample / _pdf: the shade step's own two light-half functions, triangles and spheres
 * together, on explicit HOST inputs; the lighting mode must be PTX_LIGHTING_SAMPLED with a non-empty joined table.  points: n x 3;
 * uv: n x 2 = the hit's two sampler dimensions as the light half takes them (x = (2.0 * u) * W_total);  dir_out: n x 3 world-space unit
 * directions;  index_out (nullable): n, the joined table's entry drawn.  dirs: n x 3 world directions -> pd_out: n. */
int32_t ptx_light_sample(ptx_scene* scene, int64_t n, const double* points, const double* uv, double* dir_out, int32_t* index_out);
int32_t ptx_light_pdf(ptx_scene* scene, int64_t n, const double* points, const double* dirs, double* pd_out);

/* ---- thin-lens camera: aperture and focus distance ----
 * Camera.ray (camera.ml:93-102) is a pinhole: every ray starts at P3.origin.  ptx_scene_set_lens gives the camera a lens, and with it
 * depth of field.  Only entry points are added: no struct changes and the ABI version stays 6.
 *
 * ptx_scene_set_lens(scene, radius, focus_distance): sticky state of the handle.  radius == 0 switches the lens OFF, which is the
 * state of every scene that never called the setter; an off scene renders through the pinhole's own path, kernels and alpha table,
 * bit for bit (radius 0 does not mean "a lens of radius 0": normalize(F * q) rounds differently from normalize(q)).  Accepted:
 * radius >= 0, focus_distance > 0, both finite; anything else is PTX_ERR_ARG with a message that names the rule ("lens: ...").
 * PTX_ERR_STATE while a render runs on the scene.  A host-only scene accepts it; the replicas a scene owns follow it and
 * ptx_scene_replicate copies it.  ptx_scene_lens returns what was set (radius 0 and the focus last given, 1.0 at first); either
 * out pointer may be NULL.
 *
 * Camera space is the existing one: the camera at the origin looking down -z.  The lens is the disc of radius A = radius around the
 * origin in the plane z = 0; the plane of focus is z = -F, F = focus_distance.
 *
 * The rule, operation for operation (binary64, no fma, no contraction; sqrt is IEEE, sin and cos are pt_math.h's), for a sample
 * with film coordinates (cx, cy) -- computed exactly as for the pinhole -- and the camera's (llx, lly, vx, vy):
 *   q  = (llx + (vx * cx), lly + (vy * cy), -1.0)            the pinhole's direction before it is normalised
 *   P  = (F * q.x, F * q.y, F * q.z)                         where the pinhole ray meets the plane of focus (P.z = -F exactly)
 *   r  = sqrt(u);  th = (v * 2.0) * pi;  lx = r * cos(th);  ly = r * sin(th)
 *                                                            the first two components of Shader_space.unit_square_to_hemisphere u v
 *   L  = (A * lx, A * ly, +0.0)                              the ray's origin
 *   e  = (P.x - L.x, P.y - L.y, P.z - L.z)
 *   d  = V3.normalize e = (s * e.x, s * e.y, s * e.z), s = 1 / hypot(e.x, hypot(e.y, e.z))      the ray's direction
 *   1/d = (1 / d.x, 1 / d.y, 1 / d.z) as Ray.create makes it
 * Every sample's ray passes through P (within rounding), so what lies in the plane of focus is sharp.
 *
 * Sampler dimensions.  A lens render's sampler has d = 4 + 2 * max_bounces dimensions (Low_discrepancy_sequence.create d).  The pixel
 * jitter stays in dimensions 0 and 1 and bounce k in 2 + 2k and 3 + 2k; (u, v) of the lens are the LAST two, d - 2 and d - 1, at the
 * sample's own offset.  The sequence's alpha_i = 1 / phi_d^(i + 1) depends on d through phi_d, so EVERY dimension of a lens render
 * differs from the same dimension of a pinhole render of the same depth: the jitter and the scatters too, not the lens pair alone.
 * max_bounces stays capped at 126: d = 256 then, which the 256-entry tables of the sampler's restatements still hold.
 *
 * Entry points.  The lens is read by ptx_render, ptx_render_multi (every scene passed must carry the same lens: PTX_ERR_ARG
 * otherwise), ptx_render_raw_device (bands and PTX_RENDER_ASYNC included), _passes_device, _pixels_device, _progressive, _adaptive,
 * _denoised, ptx_render_features_device (the first hit of the LENS ray; depth is t along that ray) and ptx_trace_samples.
 * ptx_ppm_render and ptx_debug_first_scatter return PTX_ERR_STATE on a scene whose lens is on ("... ptx_scene_set_lens(scene, 0, f)
 * first"); ptx_intersect_rays and ptx_walk_rays take explicit rays and are unaffected.
 * A lens render writes its camera rays into a path queue (one launch per batch, counted under PTX_KERNEL_GENERATE) and bounces them
 * from there in the walk-first order: no fused camera launch, no shade-first order, no per-octant LDS image,
 * no camera tile lists, no solo run.  The queue keeps the fused launch's order -- 64 consecutive entries are one 8 x 8 pixel tile
 * of one pass; the lanes of a ragged tile that fall off the image are holes, marked as the queues mark theirs.
 * Out of scope: polygonal or anamorphic apertures, focus by picking a pixel, a lens in the photon mapper.  (Motion blur of a moving
 * camera: the camera shutter below; with it the lens pair is the two dimensions BEFORE the last.) */
int32_t ptx_scene_set_lens(ptx_scene* scene, double radius, double focus_distance);
int32_t ptx_scene_lens(const ptx_scene* scene, double* radius_out, double* focus_distance_out);

/* ---- camera pose: a movable camera, no rebuild ----
 * The camera is the four fields Camera.ray reads, frozen into the descriptor, and the geometry is handed over in that camera's space.
 * ptx_scene_set_camera_pose places the camera anywhere in that space -- the scene's space: the camera space of the descriptor -- and
 * may give it another frustum, so a viewport or a turntable moves the camera of ONE handle instead of transforming every vertex,
 * rebuilding the tree and uploading the scene again.  Only entry points are added: no struct or call changes, the ABI version stays 6.
 *
 * ptx_scene_set_camera_pose(scene, origin, rotation, view): sticky state of the handle, like the lens, the film and the lighting
 * mode.  origin: where the camera stands; rotation: 3 x 3, row-major, from the posed camera's space (looking down -z, y up) to scene
 * space; view: the posed camera's own (lower_left_x, lower_left_y, view_x, view_y), NULL = the scene's.
 *   - all three NULL switches the pose OFF, the state of every scene that never called the setter: an off scene launches exactly
 *     what it launched before this entry point existed, bit for bit;
 *   - origin and rotation are given together or not at all; with `view` alone the pose is origin 0 and the identity rotation;
 *   - any non-NULL call switches the pose ON, the identity at origin 0 included: an on scene always takes the route below.
 * PTX_ERR_ARG with a message that starts "camera pose: " and names the rule: origin and rotation together; the origin finite; the
 * rotation finite, max |R R^T - I| <= 1e-9 (the environment rotation's bar) and det R > 0; the view finite (ptx_scene_create reads
 * the descriptor's camera as it is and applies no check of its own to it).  A refused call changes nothing.  PTX_ERR_STATE while a
 * render runs on the scene.  A host-only scene accepts it; the replicas a scene owns follow it and ptx_scene_replicate copies it.
 * ptx_scene_camera_pose returns 1 while the pose is on and 0 while it is off (a negative code for a NULL scene) and writes the
 * origin, the rotation and the view in effect -- the pose's, else the scene's own; off: origin 0, the identity; any out pointer may
 * be NULL.
 *
 * The rule, operation for operation (binary64, no fma, no contraction), for a sample with film coordinates (cx, cy) -- computed
 * exactly as for the pinhole -- the view (llx, lly, vx, vy), the pose's if it has one, else the scene's, origin o and rotation
 * R = (r00 r01 r02 / r10 r11 r12 / r20 r21 r22):
 *   q  = (llx + (vx * cx), lly + (vy * cy), -1.0)
 *   no lens:  e = q;  l = none
 *   lens:     P = (F * q.x, F * q.y, F * q.z);  L as in the lens rule above;  e = (P.x - L.x, P.y - L.y, P.z - L.z);  l = L
 *   Rv(a) = ((r00 * a.x + r01 * a.y) + r02 * a.z, (r10 * a.x + r11 * a.y) + r12 * a.z, (r20 * a.x + r21 * a.y) + r22 * a.z)
 *   direction = V3.normalize (Rv(e))                         normalised AFTER it is rotated
 *   origin    = no lens: o exactly;  lens: (o.x + Rv(l).x, o.y + Rv(l).y, o.z + Rv(l).z)
 *   the ray is Ray.create origin direction
 * Because the vector is rotated before it is normalised, the identity pose at origin 0 gives EXACTLY the pinhole's ray: 1 * x +
 * 0 * y + 0 * z is x, and 0 + x is x; with a lens on, the same pose gives exactly the lens's ray.  The one caveat is the sign of a
 * zero: a component that is -0 there can be +0 here (0 * y is -0 for a negative y, and x + -0 keeps x but -0 + +0 is +0).  No
 * walk or shade result depends on it.  The film coordinates and the sampler are the pinhole's, or the lens's where a lens is on:
 * THE POSE ADDS NO SAMPLER DIMENSION, so every alpha table is the one the same render without a pose reads.  The background, the
 * environment map, normals and texture coordinates stay in scene space: the world does not tilt with the camera.
 * "Off" and "posed back home" are different states: a pose computed for the scene's own eye and target
 * (pth_camera_pose_look_at) is the identity within rounding only, and even the exact identity takes the route below.
 *
 * Entry points.  The pose is read by ptx_render, ptx_render_multi (every scene passed must carry the same pose: PTX_ERR_ARG
 * otherwise), ptx_render_raw_device (bands and PTX_RENDER_ASYNC included), _passes_device, _pixels_device, _progressive, _adaptive,
 * _denoised, ptx_render_features_device (the first hit of the posed ray; depth is t along that ray) and ptx_trace_samples.
 * ptx_ppm_render and ptx_debug_first_scatter return PTX_ERR_STATE while a pose is on ("... ptx_scene_set_camera_pose(scene, NULL,
 * NULL, NULL) first"), before any device is touched; ptx_intersect_rays and ptx_walk_rays take explicit rays and are unaffected.
 * A posed render takes the lens's route: its camera rays are written into a path queue (k_generate_tiles, one launch per batch,
 * counted under PTX_KERNEL_GENERATE; the same 8 x 8-tile order, ids and holes) and bounced from there in the walk-first order.  It
 * gives up the fused camera launch, the shade-first order, the per-octant LDS image, the camera tile lists (none is built) and the
 * solo run.  Recorded on the MI355X (tools/camera_pose_cost.py, profiles/pr_camera_pose_cost.json, medians of 5): the 1080p spp 64
 * depth 8 Shirley frame takes 16.4 ms as it is, 23.3 ms under the identity pose and 22.1 ms under an oblique one; eight turntable
 * frames over a 148 k-triangle mesh take 29 ms each against 656 ms (host BVH builder) or 848 ms (GPU builder) for destroy / create /
 * render.
 *
 * ptx_camera_rays (diagnostic): the camera rays the scene's renders launch for explicit (x, y, pass) triples under `params`
 * (width, height, samples_per_pixel and max_bounces, which with a lens sets the sampler's dimension) -- the pose's, a lens's or the
 * pinhole's, whatever the handle's state selects.  Host in, host out: origins_out and directions_out take 3 n doubles each.
 *
 * A camera that moves while a frame is exposed: the camera shutter below (its time dimension keeps the sampler inside its 256-entry
 * tables by capping a lens + shutter render at 125 bounces).
 * Out of scope: a pose in the photon mapper; moving the geometry instead of the camera; the fused camera launch for poses that happen to have
 * origin 0. */
int32_t ptx_scene_set_camera_pose(ptx_scene* scene, const double origin[3], const double rotation[9] /* row-major */,
                                  const ptx_camera* view /* NULL = the scene's own llx, lly, vx, vy */);
int32_t ptx_scene_camera_pose(const ptx_scene* scene, double origin_out[3], double rotation_out[9], ptx_camera* view_out); /* 1 = on, 0 = off */
int32_t ptx_camera_rays(ptx_scene* scene, const ptx_render_params* params, int64_t n, const int32_t* xs, const int32_t* ys, const int32_t* passes,
                        double* origins_out /* 3n */, double* directions_out /* 3n */);

/* ---- camera projection: a lat-long panorama ----
 * The library can be lit by a lat-long image (ptx_scene_set_environment); with PTX_PROJECTION_LATLONG it can produce one.  The
 * panorama uses the environment's own (u, v) convention, so a probe rendered at a point can light another scene.  Only entry points
 * and two defines are added: no struct or call changes, the ABI version stays 6.
 *
 * ptx_scene_set_camera_projection(scene, projection): sticky state of the handle, like the pose.  PTX_PROJECTION_PERSPECTIVE is
 * the state of every scene that never called the setter, and renders as before, bit for bit.  PTX_ERR_ARG for another value;
 * PTX_ERR_STATE while a render runs on the scene, and for LATLONG while a lens is on ("... ptx_scene_set_lens(scene, 0, 1) first";
 * ptx_scene_set_lens with a radius > 0 is refused likewise while LATLONG is on).  A refused call changes nothing.  A host-only scene
 * accepts it; the replicas a scene owns follow it and ptx_scene_replicate copies it.  ptx_scene_camera_projection returns the kind,
 * or a negative code for a NULL scene.
 *
 * The rule, operation for operation (binary64, no fma, no contraction; sincos is pt_math.h's), for a sample with film coordinates
 * (cx, cy) -- computed exactly as for the pinhole -- with pi = Float.pi:
 *   u = cx;  v = 1.0 - cy;  al = u * (2.0 * pi) - pi;  th = v * pi
 *   (sa, ca) = sincos(al);  (st, ct) = sincos(th)
 *   e = (st * ca, -ct, -(st * sa))
 *   direction = V3.normalize (Rv(e));  origin = o        the pose rule's Rv and o; origin 0 and the identity while the pose is off
 *   the ray is Ray.create origin direction
 * e is the environment-sampling rule's m from (u, v), so the rule is the inverse of the environment lookup: the lookup of the
 * direction of film point (cx, cy), under an environment rotation that is the pose's transpose, lands on (u, v) = (cx, 1 - cy).  Image
 * row 0 is v = 0, which the environment map puts at -y (straight down in the pose's space; the last row looks straight up), the
 * centre column looks down +x of the pose's space and the left and right edges meet at -x: the environment map's convention, row
 * for row -- viewed as a picture with row 0 on top, a panorama shows the ground above the sky, exactly as an environment image does.  So a panorama rendered at a point and loaded as an environment with the
 * identity R shows a second scene what the first one looked like from that point.  The view fields (the scene's and the pose's) are
 * not read.  THE PROJECTION ADDS NO SAMPLER DIMENSION.
 *
 * Route.  A LATLONG scene takes the posed route whether a pose is on or not: its camera rays are written into a path queue
 * (k_generate_tiles, counted under PTX_KERNEL_GENERATE; the same 8 x 8-tile order, ids and holes) and bounced walk-first, through
 * every driver the pose serves: ptx_render, ptx_render_multi (every scene passed must carry the same projection: PTX_ERR_ARG
 * otherwise), ptx_render_raw_device, _passes_device, _pixels_device, _progressive, _adaptive, _denoised,
 * ptx_render_features_device, ptx_trace_samples and ptx_camera_rays.  ptx_render_temporal (its reprojection is a pinhole's),
 * ptx_ppm_render and ptx_debug_first_scatter return PTX_ERR_STATE while LATLONG is on ("... ptx_scene_set_camera_projection(scene,
 * PTX_PROJECTION_PERSPECTIVE) first"), before anything is launched.
 *
 * Out of scope: fisheye and orthographic projections; a lens or temporal accumulation under LATLONG. */
#define PTX_PROJECTION_PERSPECTIVE 0
#define PTX_PROJECTION_LATLONG 1
int32_t ptx_scene_set_camera_projection(ptx_scene* scene, int32_t projection);
int32_t ptx_scene_camera_projection(const ptx_scene* scene); /* the kind, or a negative code */

/* ---- camera shutter: motion blur between two poses ----
 * Every frame of a posed sequence is exposed for an instant, so a moving camera strobes.  ptx_scene_set_camera_shutter lets the camera
 * move while the frame is exposed: each sample draws a time t in [0, 1) and sees the scene from the camera of that time.  Only entry
 * points are added: no struct or call changes, the ABI version stays 6.
 *
 * ptx_scene_set_camera_shutter(scene, translation, axis, angle): sticky state of the handle, like the pose.  While the shutter is open
 * the camera moves from the pose's origin o to o + translation and turns from the pose's rotation R to Rot(axis, angle) * R, at
 * constant velocity and constant angular velocity.  translation and axis are in scene space, axis is a unit vector, angle in radians.
 *   - NULL, NULL, 0.0 switches the shutter OFF, the state of every scene that never called the setter: an off scene launches exactly
 *     what it launched before this entry point existed, bit for bit, with the same alpha tables;
 *   - any other accepted call switches it ON, a zero translation with angle 0 included (the axis may then be zero): an on scene always
 *     takes the route below;
 *   - while the shutter is on and the pose is off, the pose is origin 0 and the identity (as under PTX_PROJECTION_LATLONG).
 * PTX_ERR_ARG with a message that starts "camera shutter: " and names the rule: translation and axis are given together or not at all
 * (and not NULL with an angle != 0); every value finite; |angle| <= pi; and, while angle != 0, | |axis| - 1 | <= 1e-9 (the rotation's
 * bar).  PTX_ERR_STATE while a render runs on the scene.  A refused call changes nothing.  A host-only scene accepts it; the replicas a
 * scene owns follow it and ptx_scene_replicate copies it.  ptx_scene_camera_shutter returns 1 while the shutter is on and 0 while it
 * is off (a negative code for a NULL scene) and writes what was set (off: zeros); any out pointer may be NULL.
 *
 * The rule, operation for operation (binary64, no fma, no contraction; sincos is pt_math.h's), for a sample with film coordinates
 * (cx, cy), its time t, translation T, axis k and angle A:
 *   a = t * A;  (sn, cs) = sincos(a);  oc = 1.0 - cs
 *   S(w):  kw = (k.x * w.x + k.y * w.y) + k.z * w.z
 *          c  = ((k.y * w.z) - (k.z * w.y), (k.z * w.x) - (k.x * w.z), (k.x * w.y) - (k.y * w.x))
 *          S(w).i = ((w.i * cs) + (c.i * sn)) + (k.i * (kw * oc))                                  i = x, y, z
 *   ot = (o.x + (t * T.x), o.y + (t * T.y), o.z + (t * T.z))
 *   pose, no lens:  direction = V3.normalize (S(Rv(q)));      origin = ot
 *   pose, lens:     direction = V3.normalize (S(Rv(P - L)));  origin = (ot.x + S(Rv(L)).x, ot.y + S(Rv(L)).y, ot.z + S(Rv(L)).z)
 *   lat-long:       direction = V3.normalize (S(Rv(e)));      origin = ot
 *   the ray is Ray.create origin direction
 * q, P, L, e and Rv are exactly the pose, lens and projection rules' own (kw and c are written out: V3.dot and V3.cross are fused).
 * The vector is turned AFTER Rv and BEFORE it is normalised.  With T = 0 and A = 0, sn = 0, cs = 1 and oc = 0, so S(w) = w and
 * ot = o: the rule gives the posed ray of the same (cx, cy, u, v), up to the sign of a zero (w * 1 + c * 0 + k * 0 turns a -0 into
 * +0).  S is Rodrigues' rotation by t A about k, so the ray at time t is, within rounding, the posed ray of the pose
 * (o + t T, Rot(k, t A) * R), and with a lens every sample's ray passes through that camera's focus point.
 *
 * Sampler dimensions.  A shutter render's sampler has ONE MORE dimension: d = 2 + 2 * max_bounces (+ 2 with a lens) + 1.  t is the
 * LAST dimension, d - 1, at the sample's own offset; the lens pair moves to d - 3 and d - 2; the jitter and the bounces stay where
 * they are.  alpha_i depends on d, so EVERY alpha of a shutter render differs from the same render without a shutter, as with the
 * lens.  d stays <= 256: lens + shutter at max_bounces = 126 is PTX_ERR_ARG ("camera shutter: ... at most 125 bounces with a lens");
 * without a lens 126 stays legal (d = 255).
 *
 * Entry points.  The shutter is read by ptx_render, ptx_render_multi (every scene passed must carry the same shutter: PTX_ERR_ARG
 * otherwise), ptx_render_raw_device (bands and PTX_RENDER_ASYNC included), _passes_device, _pixels_device, _progressive, _adaptive,
 * _denoised and the display forms, ptx_render_features_device (the first hit of the shutter ray), ptx_trace_samples and
 * ptx_camera_rays.  A shutter scene takes the posed route whether a pose is on or not (k_generate_*, three camera kinds of their own).
 * ptx_render_temporal (its reprojection takes one pose per frame), ptx_ppm_render and ptx_debug_first_scatter return PTX_ERR_STATE
 * while the shutter is on ("... ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first"), before anything is queued.
 * ptx_render_rays*, ptx_intersect_rays and ptx_walk_* take explicit rays and are unaffected.
 *
 * Out of scope: moving geometry or lights; a shutter curve other than uniform; a rolling shutter; motion vectors for
 * ptx_render_temporal under a shutter; a shutter in the photon mapper. */
int32_t ptx_scene_set_camera_shutter(ptx_scene* scene, const double translation[3], const double axis[3], double angle);
int32_t ptx_scene_camera_shutter(const ptx_scene* scene, double translation_out[3], double axis_out[3], double* angle_out); /* 1 = on, 0 = off */

/* ---- temporal accumulation: the frame history reprojected across camera poses ----
 * The temporal half of the variance-guided filter: the per-pixel moments of the frames before are carried into the new frame by
 * reprojecting every pixel's first hit through the two cameras, and dropped where the surface changed.  Only entry points and two
 * structs are added: no existing struct or kernel changes, the ABI version stays 6, and a scene that never calls these launches
 * exactly what it launched before.  Everything here runs on ONE GPU over the whole image.
 *
 * The history record of a pixel: PTX_HISTORY_DOUBLES doubles at index (y * W + x) * 12 of a 16-byte aligned buffer (the records
 * move as 16-byte accesses; any hipMalloc'ed buffer is aligned):
 *   [0..2]  M1  the running mean radiance
 *   [3..5]  M2  the running mean of the squared samples
 *   [6]     N   the effective passes behind them, as a double; 0 = no history, so a zeroed buffer is the empty history
 *   [7]     hf  h / kfd: the share of the feature passes that hit
 *   [8..10] n   the mean normal
 *   [11]    zc  the mean hit distance from the camera of the frame that wrote the record (0 where nothing was hit)
 *
 * A camera (ptx_temporal_camera, 128 bytes) is an origin, a row-major rotation and the four view fields, as
 * ptx_scene_set_camera_pose takes them; it is checked like a pose (finite, max |R R^T - I| <= 1e-9, det R > 0) and view_x and
 * view_y must be non-zero (the rule divides by them).  The settings (ptx_temporal_params, 32 bytes) are accepted when all four are
 * finite, max_history_passes >= 0, normal_threshold in [-1, 1], depth_tolerance >= 0 and 0 <= min_weight < 1.
 * ptx_temporal_defaults gives 64, 0.9, 0.02 and 2^-10; they may be retuned only with the CPU quality table of
 * tests/test_temporal_reference.py recorded beside them (README.md).
 *
 * The rule, operation for operation (binary64, no fma, no contraction), for pixel (x, y) of a W x H frame with k = passes_done >= 2
 * passes, kf = feature_passes_done >= 1 feature passes, the raw sums S1 and square sums S2 of THIS frame's passes (as
 * ptx_render_passes_device leaves them), the feature sums A, Nrm, Z, h (ptx_render_features_device), the current camera
 * (o, R, llx, lly, vx, vy), the camera of the frame that wrote the previous history (primed: o', R' = (r00' r01' r02' / r10' ... ),
 * llx', lly', vx', vy') and cap = max_history_passes:
 *   current     kd = (double)k;  kfd = (double)kf
 *               mu_c = S1_c / kd;  nu_c = S2_c / kd
 *               hf = h / kfd;  n = Nrm / kfd;  z = h > 0 ? Z / h : 0.0
 *               cx = ((double)x + 0.5) * (1.0 / W);  cy = 1.0 - ((double)y + 0.5) * (1.0 / H)
 *               d = the camera-pose rule's direction for (cx, cy), no lens, under the CURRENT camera
 *   reproject   (a NULL previous history: every pixel takes "no history")
 *               h > 0:   P = (o.x + z * d.x, o.y + z * d.y, o.z + z * d.z);  v = (P.x - o'.x, P.y - o'.y, P.z - o'.z)
 *               h == 0:  v = d                                               (a miss is a point at infinity)
 *               c = ((r00' * v.x + r10' * v.y) + r20' * v.z, (r01' * v.x + r11' * v.y) + r21' * v.z,
 *                    (r02' * v.x + r12' * v.y) + r22' * v.z)                 (R'^T v)
 *               if !(c.z < 0): no history
 *               iz = -c.z;  qx = c.x / iz;  qy = c.y / iz
 *               fx = ((qx - llx') / vx') * (double)W - 0.5;  fy = (1.0 - (qy - lly') / vy') * (double)H - 0.5
 *               if !(fx > -1 && fx < W && fy > -1 && fy < H): no history     (NaN fails)
 *               x0 = floor(fx), y0 = floor(fy);  tx = fx - x0;  ty = fy - y0
 *               dist = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z)
 *               sw = a1_c = a2_c = aN = 0;  taps j = 0, 1 (outer), i = 0, 1 (inner), q = (x0 + i, y0 + j):
 *                 skip q outside the image;  rec = the previous history at q;  skip unless rec.N > 0
 *                 h == 0:  skip unless rec.hf == 0
 *                 h > 0:   skip unless rec.hf > 0 and (n.x * rec.n.x + n.y * rec.n.y) + n.z * rec.n.z >= normal_threshold
 *                                                 and fabs(dist - rec.zc) <= depth_tolerance * dist
 *                 w = (i ? tx : 1.0 - tx) * (j ? ty : 1.0 - ty)
 *                 sw = sw + w;  a1_c = a1_c + w * rec.M1_c;  a2_c = a2_c + w * rec.M2_c;  aN = aN + w * rec.N
 *               history iff sw > min_weight
 *   blend       history:     H1_c = a1_c / sw;  H2_c = a2_c / sw;  NH = aN / sw;  if NH > cap: NH = cap
 *                            al = kd / (NH + kd);  M1_c = H1_c * (1.0 - al) + mu_c * al;  M2_c = H2_c * (1.0 - al) + nu_c * al
 *                            N = NH + kd
 *               no history:  M1 = mu;  M2 = nu;  N = kd
 *   outputs     the new record {M1, M2, N, hf, n, z}
 *               raw_out_c = M1_c * kd: SUMS as of k passes, so ptx_denoise_device with passes_done = k and the film with spp = k
 *                 apply unchanged
 *               var_c = M2_c - M1_c * M1_c, set to 0 unless var_c > 0;  err_out_c = sqrt(var_c / (N - 1.0))
 *               motion_out (nullable, W * H * 3): (fx - x, fy - y, sw) with history, (0, 0, 0) without
 * With cap = 0 the blend has al = 1 and returns mu bit for bit while the pixel still counts as having history.  A miss matches
 * misses only (a sky pixel's history follows the rotation, not the translation).
 *
 * ptx_temporal_accumulate_device: all buffers are DEVICE memory -- d_raw, d_sq, d_raw_out, d_err_out W*H*3, d_feat W*H*8,
 * d_hist_prev (nullable) and d_hist_out W*H*12, d_motion_out (nullable) W*H*3 -- and must not alias one another (d_hist_out ==
 * d_hist_prev included: a pixel's taps read records other pixels write).  *history_pixels_out (HOST, nullable): the pixels that
 * took history.  prev_camera may be NULL only with a NULL history (it is then not read).  One thread owns a pixel, no float
 * atomics: the same inputs give the same bits on every run.  Waits for `stream`.  PTX_ERR_ARG for NULL or aliased buffers,
 * passes_done < 2, feature_passes_done < 1, refused settings or cameras; PTX_ERR_STATE for device < 0 (no CPU fallback). */
#define PTX_HISTORY_DOUBLES 12
typedef struct ptx_temporal_camera { /* 128 bytes */
  double origin[3];
  double rotation[9]; /* row-major */
  ptx_camera view;
} ptx_temporal_camera;
typedef struct ptx_temporal_params { /* 32 bytes */
  double max_history_passes; /* cap >= 0: a history counts for at most this many passes against the frame's k */
  double normal_threshold;   /* in [-1, 1]: a tap is kept when n . n_tap >= this */
  double depth_tolerance;    /* >= 0: ... and |dist - zc_tap| <= this * dist */
  double min_weight;         /* in [0, 1): history needs more than this much bilinear weight left */
} ptx_temporal_params;
/* 64, 0.9, 0.02, 2^-10 */
int32_t ptx_temporal_defaults(ptx_temporal_params* out);
int32_t ptx_temporal_accumulate_device(int32_t device, int32_t width, int32_t height, const ptx_temporal_params* temporal,
                                       int32_t passes_done /* k >= 2 */, int32_t feature_passes_done /* kf >= 1 */,
                                       const ptx_temporal_camera* cur_camera, const ptx_temporal_camera* prev_camera,
                                       const double* d_raw, const double* d_sq, const double* d_feat,
                                       const double* d_hist_prev /* nullable */, double* d_hist_out, double* d_raw_out,
                                       double* d_err_out, double* d_motion_out /* nullable */,
                                       int64_t* history_pixels_out /* HOST, nullable */, void* stream);

/* One frame of a sequence on a scene handle.  params->samples_per_pixel is the SEQUENCE's N, which fixes the sampler; the frame
 * renders passes [pass_first, pass_first + pass_count) of it.  ADVANCE pass_first FROM FRAME TO FRAME (and wrap around N): under a
 * still camera the same slice draws the same samples again, the history and the frame are then the same numbers, and accumulating
 * them gains nothing -- different slices are different points of the low-discrepancy sequence, and their mean converges.
 * The call is this chain and equals it bit for bit:
 *   1. zero the raw sums, the square sums and the feature sums
 *   2. ptx_render_passes_device over the range, with square sums
 *   3. ptx_render_features_device over the same range
 *   4. ptx_temporal_accumulate_device with k = kf = pass_count; the current camera is the scene's pose (ptx_scene_camera_pose), or
 *      origin 0, the identity and the scene's own view while the pose is off; the previous camera and history are what the handle
 *      kept from the frame before (none: a NULL history)
 *   5. with `denoise` (nullable: no spatial filter): ptx_denoise_device(passes_done = pass_count, kf = pass_count) on the
 *      accumulated sums and error (denoise->feature_passes is not read)
 *   6. the scene's film (ptx_scene_set_film) with spp = pass_count
 *   7. the copy to rgb_out (HOST, W*H*3); err_out (HOST, nullable, W*H*3): the accumulated err; motion_out (HOST, nullable, W*H*3);
 *      *history_pixels_out (nullable)
 * The handle then keeps the new history and the camera (it owns two history buffers and swaps them).  The history is dropped by
 * ptx_temporal_reset and by a frame of another width or height, AND NEVER OTHERWISE: a caller who changes the lighting mode, a
 * texture image, the environment or anything else the radiance depends on calls ptx_temporal_reset themself.  Moving geometry or
 * lights, and what is seen through a reflection or refraction at the first hit, are not reprojected (the first hit's motion is).
 * PTX_ERR_STATE on a scene whose lens is on (a lens ray's first hit is not a pinhole projection), on a host-only scene and from a
 * callback of a running render; PTX_ERR_ARG for n_gpus > 1, band_step > 1, pass_count < 2, a range outside [0, N) and refused
 * settings.  A failed call leaves the history as it was, a failed frame of another size included: that frame reads no history, and
 * the handle's is replaced only once the frame stands.  stats->samples = W * H * pass_count. */
int32_t ptx_render_temporal(ptx_scene* scene, const ptx_render_params* params, const ptx_temporal_params* temporal,
                            const ptx_denoise_params* denoise /* nullable */, int32_t pass_first, int32_t pass_count, double* rgb_out,
                            double* err_out /* nullable */, double* motion_out /* nullable */, int64_t* history_pixels_out /* nullable */,
                            ptx_stats* stats);
/* drops the history the handle keeps (its buffers stay); a host-only scene accepts it; PTX_ERR_STATE while a render runs */
int32_t ptx_temporal_reset(ptx_scene* scene);

/* ---- radiance along rays the caller owns ----
 * Every other radiance entry point starts at a pixel of the scene's camera.  ptx_render_rays_device runs the same paths from rays
 * the caller hands over -- light probes, irradiance at surface points, a sensor that is no pinhole, a batch a device program built --
 * by the route a lens or a posed render takes: the rays are written into a path queue and bounced from there in the walk-first
 * order.  Only entry points, one struct and one define are added: no existing struct, kernel or call changes, the ABI version
 * stays 6, and a scene that never calls these launches exactly what it launched before.
 *
 * The path.  Ray i is Ray.create o_i d_i with (o_i, d_i) the i-th triples of `origins` and `directions`; with PTX_RAYS_NORMALIZE,
 * Ray.create o_i (V3.normalize d_i).  Its radiance is path_tracer's (integrator.ml:16-69) from that ray at depth max_bounces, under
 * the handle's shading state: the lighting mode, image textures, the environment, environment sampling and sphere-light sampling.
 * The lens, the pose and the scene's camera are not read.  The caller hands UNIT directions, as every camera of the library does.
 * Without the flag a direction is used as it is given and no length is checked: a non-unit one is walked correctly (hit distances
 * are then in units of its length, and the closest hit is the same), but the shade step's formulas that take the incoming direction
 * for a unit vector (the mirror and refraction directions, Schlick's cosine) get it as it is, as the reference would for a ray
 * created that way -- the value is well defined and reproducible, and it is not the radiance along the normalised ray.
 *
 * The sampler.  The path of ray i reads the low-discrepancy sequence at offset offsets[i] (offsets == NULL: offset i = i), with the
 * dimension the scene's own renders of that depth use: 2 + 2 max_bounces, and two more while the scene has a lens.  Bounce k reads
 * dimensions 2 + 2 k and 3 + 2 k, exactly as for a camera ray.  Dimensions 0 and 1 (and the lens pair, the last two) are not read
 * here: they belong to the caller, who may have drawn the ray from them -- ptx_lds_sample gives them.  So the rays ptx_camera_rays
 * returns for samples (x, y, pass), with the offsets y W + x + pass N those samples have, give what ptx_trace_samples gives for
 * them, bit for bit.  Offsets lie in [0, 2^31 - 2] (Low_discrepancy_sequence.get forms 1 + offset in 32 bits).
 *
 * The sums.  With m = rays_per_bin, bin b is rays [b m, (b + 1) m) and n must be a multiple of m.  For every ray of the bin, in ray
 * order, with c its radiance: sum[b]_c = sum[b]_c + c and, if d_sq_inout is given, sq[b]_c = sq[b]_c + (c * c) -- a left fold onto
 * what the buffers held (binary64, the product rounded before the add).  NOTHING IS ZEROED by the device call; m = 1 onto zeros is
 * the per-ray radiance.  No floating-point atomics: the same inputs give the same bits on every run and for every batch size.
 *
 * Batching.  n may exceed any workspace: the call runs the rays in batches (16 M rays; PTX_RAYS_BATCH, a test hook, sets another
 * size), each one generate launch (k_generate_rays: entry = id = the ray's index in the batch), the bounces, and one fold
 * (k_accum_rays: a thread per bin).  A bin may straddle batches: the later batch's fold continues from the buffer.
 *
 * Checks.  Before a device is touched, in this order: PTX_ERR_ARG for NULL scene, params, origins, directions or sums, max_bounces
 * outside [0, 126], rays_per_bin < 1, unknown bits in flags, n < 0, n >= 2^31 - 1, n no multiple of rays_per_bin; PTX_ERR_STATE for a
 * host-only scene and for a call made while a render runs on the scene (from one of its callbacks).  n == 0 returns 0.  Then, on the
 * device and before anything is queued (k_rays_check), every ray: a component of the origin or the direction that is not finite, a
 * direction whose three components are all zero, or an offset outside [0, 2^31 - 2] is PTX_ERR_ARG, the message starts
 * "ray <lowest refused index> " and the sums are left untouched.
 *
 * Stream and stats.  All pointers of ptx_render_rays_device are DEVICE pointers on the scene's device; the work is queued on
 * `stream` (NULL: the null stream) and the call waits for it.  stats (nullable): samples = n; with count_work, segments and the
 * work counters as ptx_trace_samples reports them.  ptx_render_rays is the same with HOST pointers: it zeroes the sums (n / m bins
 * of 3 doubles; sq_out nullable), runs the device call and copies them back. */
#define PTX_RAYS_NORMALIZE 1
typedef struct ptx_rays_params { /* 16 bytes */
  int32_t max_bounces;  /* as ptx_render_params */
  int32_t rays_per_bin; /* m >= 1; n must be a multiple of m */
  int32_t flags;        /* PTX_RAYS_NORMALIZE; unknown bits are PTX_ERR_ARG */
  int32_t count_work;   /* as ptx_render_params */
} ptx_rays_params;
int32_t ptx_render_rays_device(ptx_scene* scene, const ptx_rays_params* params, int64_t n, const double* d_origins /* n x 3 */,
                               const double* d_directions /* n x 3 */, const int32_t* d_offsets /* n, nullable: offset i = i */,
                               double* d_sum_inout /* (n / m) x 3 */, double* d_sq_inout /* nullable */, void* stream, ptx_stats* stats);
int32_t ptx_render_rays(ptx_scene* scene, const ptx_rays_params* params, int64_t n, const double* origins, const double* directions,
                        const int32_t* offsets, double* sum_out, double* sq_out, ptx_stats* stats);

/* ---- display outputs: 8-bit and binary32 framebuffers, exposure, tone curves ----
 * Every image above is binary64, sqrt-encoded and unclamped: 24 bytes a pixel, of which a PNG, a display or an encoder wants 3, 4,
 * 12 or 16.  The display is a function of THE IMAGE ptx_render RETURNS: per channel it takes the binary64 value v of the filmed,
 * sqrt-encoded image, so "the display of the f64 image" (ptx_display_apply on the host, ptx_display_image_device on a device) and
 * "the display entry point" (ptx_render_display, ptx_render_progressive_display) are the same bits for every setting.  Only entry
 * points, one struct and one callback type are added: no existing struct, kernel or call changes, the ABI version stays 6.
 *
 * The rule, operation for operation (binary64, no fma, no contraction), for one channel value v:
 *   Stage A, the value t
 *     REFERENCE:         t = v                               (needs tone == NONE and exposure == 1.0)
 *     LINEAR and SRGB:   L = (v * v) * exposure;  L = (L > 0x1p40) ? 0x1p40 : L      (a NaN stays a NaN; the cap keeps inf / inf
 *                                                                                     out of the curves)
 *       NONE:            t = L
 *       REINHARD:        t = L / (1.0 + L)
 *       ACES:            t = (L * ((2.51 * L) + 0.03)) / ((L * ((2.43 * L) + 0.59)) + 0.14)      (the Narkowicz fit)
 *   Stage B, the stored channel
 *     8 bits, REFERENCE or LINEAR:   y = t * 255.0;  if (!(y > 0.0)) y = 0.0;  if (y > 255.0) y = 255.0;  code = (uint8_t)(int)y
 *                                    -- the PNG writer's conversion, a truncation; NaN gives 0
 *     8 bits, SRGB:                  code = the number of k in 1 .. 255 with T[k] <= t; NaN gives 0.  T[k] is the binary64 threshold
 *                                    between codes k - 1 and k under round-to-nearest of the sRGB encoding:
 *                                      e = (k - 0.5) / 255.0;  T[k] = e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4)
 *                                    computed ONCE on the host with libm's pow, held by the library, copied to each device and handed
 *                                    out by ptx_display_thresholds: host, device and any restatement search the same 255 doubles
 *     binary32, REFERENCE or LINEAR: (float)t, round to nearest even, subnormal results included; no clamp, infinities and NaN pass
 *     binary32 with SRGB:            refused: the binary32 formats carry linear or reference values
 *   Alpha is 255 or 1.0f.  Every channel of a pixel goes through the same path.
 *
 * Refusals (ptx_display_check is what every entry point below applies, before anything is queued): PTX_ERR_ARG with a message that
 * starts "display: " and names the rule for an unknown format, transfer or tone; non-zero flags or reserved words; an exposure that
 * is not finite or is negative; REFERENCE with a tone other than NONE or an exposure other than 1.0; a binary32 format with SRGB.
 *
 * Out of scope: dithering, 16-bit PNG and half floats, a display transform inside the photon mappers, chromatic adaptation or
 * colour spaces other than the scene's own RGB, a film kernel fused with the display. */
#define PTX_PIXEL_RGB8 0    /* 3 bytes a pixel */
#define PTX_PIXEL_RGBA8 1   /* 4 */
#define PTX_PIXEL_RGB32F 2  /* 12 */
#define PTX_PIXEL_RGBA32F 3 /* 16 */
#define PTX_TRANSFER_REFERENCE 0
#define PTX_TRANSFER_LINEAR 1
#define PTX_TRANSFER_SRGB 2
#define PTX_TONE_NONE 0
#define PTX_TONE_REINHARD 1
#define PTX_TONE_ACES 2
typedef struct ptx_display_params { /* 40 bytes */
  int32_t format;    /* PTX_PIXEL_* */
  int32_t transfer;  /* PTX_TRANSFER_* */
  int32_t tone;      /* PTX_TONE_* */
  int32_t flags;     /* 0 */
  double exposure;   /* multiplies linear radiance; finite, >= 0 */
  int32_t reserved[4]; /* 0 */
} ptx_display_params;
/* RGB8, REFERENCE, NONE, exposure 1.0: the bytes the PNG writer makes of ptx_render's image */
int32_t ptx_display_defaults(ptx_display_params* out);
/* 0, or PTX_ERR_ARG with the rule in ptx_last_error().  Needs no device. */
int32_t ptx_display_check(const ptx_display_params* display);
/* bytes of one pixel of `format`, or PTX_ERR_ARG */
int32_t ptx_display_pixel_bytes(int32_t format);
/* out[k - 1] = T[k], k = 1 .. 255.  Needs no device. */
int32_t ptx_display_thresholds(double out[255]);
/* The rule on the host: n_pixels pixels of 3 doubles at rgb to n_pixels * ptx_display_pixel_bytes(format) bytes at out.  Needs no
 * device.  n_pixels == 0 returns 0. */
int32_t ptx_display_apply(const ptx_display_params* display, int64_t n_pixels, const double* rgb, void* out);
/* The rule on a device, for any filmed f64 image there: the film's output, ptx_denoise_device's after the film, a frame of
 * ptx_render_temporal.  d_rgb and d_out are DEVICE memory, both 16-byte aligned (any hipMalloc'ed buffer is) and not overlapping.
 * Queued on `stream`; waits for it, like ptx_film_resolve_device.  PTX_ERR_STATE for device < 0 (the host has ptx_display_apply). */
int32_t ptx_display_image_device(int32_t device, const ptx_display_params* display, int64_t n_pixels, const double* d_rgb,
                                 void* d_out, void* stream);
/* The same over pixels [pixel_first, pixel_first + n_pixels) of the two images, whose bases d_rgb and d_out stay the images' first
 * pixels (aligned as above): the form ptx_render_display's row slabs take, a range that starts at row0 * width pixels.  Bytes of
 * d_out outside the range are not written, whatever the range's alignment to the kernel's four-pixel quads -- two adjacent ranges
 * never write the same byte.  ptx_display_image_device is the range [0, n_pixels). */
int32_t ptx_display_range_device(int32_t device, const ptx_display_params* display, int64_t pixel_first, int64_t n_pixels,
                                 const double* d_rgb, void* d_out, void* stream);
/* The byte-typed twin of ptx_image_pin, for a display image: same contract, and still ONE pinned image per handle of either kind
 * (pinning another releases the first); ptx_image_unpin releases either. */
int32_t ptx_image_pin_bytes(ptx_scene* scene, void* image, int64_t n_bytes);
/* ptx_render with `out` (HOST, width * height * ptx_display_pixel_bytes(format) bytes) in the named format: the film runs into the
 * handle's f64 image as in ptx_render, the display kernel runs over it, and the display bytes are what is copied.  Into a pinned
 * image (ptx_image_pin_bytes) the frame's tail is ptx_render's row-slab pipeline: per slab the film, the display kernel over the
 * slab's rows, the copy of the slab's display bytes.  n_gpus > 1 renders as ptx_render_multi does and displays the image filmed on
 * the first device.  out == display_apply(ptx_render's image), bit for bit.  A refused call leaves `out` untouched. */
int32_t ptx_render_display(ptx_scene* scene, const ptx_render_params* params, const ptx_display_params* display, void* out,
                           ptx_stats* stats, ptx_progress_fn progress, void* user);
/* ptx_update_fn with the update's image as display pixels */
typedef int32_t (*ptx_update_display_fn)(void* user, int32_t passes_done, double rel_err, const void* pixels, const double* err);
/* ptx_render_progressive -- with `denoise` (nullable) ptx_render_denoised -- whose updates are display images: after every update's
 * film the display kernel runs over the image, and the display bytes are what is copied into `out` and handed to the callback.  The
 * error image (err_out, nullable, with denoise the un-denoised se) stays f64.  Everything else -- the checks, the slices, the early
 * stop, the drain on every exit -- is the f64 entry point's.  Run to N passes with REFERENCE / RGB8, `out` is the display of
 * ptx_render's image bit for bit. */
int32_t ptx_render_progressive_display(ptx_scene* scene, const ptx_render_params* params, const ptx_progressive_params* progressive,
                                       const ptx_denoise_params* denoise /* nullable */, const ptx_display_params* display, void* out,
                                       double* err_out /* nullable */, int32_t* passes_done_out, ptx_stats* stats,
                                       ptx_update_display_fn on_update, void* user);

/* Per-sample radiance for explicit (x, y, pass) triples -- the value Integrator's
 * trace_path returns (integrator.ml:106).  Host in / host out, n*3 doubles.
 * Used by the parity tests (bit-exact against the oracle). */
int32_t ptx_trace_samples(ptx_scene* scene, const ptx_render_params* params, int64_t n,
                          const int32_t* xs, const int32_t* ys, const int32_t* passes,
                          double* rgb_out, ptx_stats* stats);

/* Closest-hit queries on the device for explicit rays (Scene.intersect,
 * shirley_spheres/bin/main.ml:273-277): n rays (origin, direction: 3 doubles each),
 * outputs t_hit (DBL_MAX-as-miss is NOT used: prim_out = -1 on a miss) and the index of
 * the primitive in the build list ([triangles] @ [spheres]; floor triangles are
 * n_triangles + n_spheres + i). */
int32_t ptx_intersect_rays(ptx_scene* scene, int64_t n, const double* origins,
                           const double* directions, double* t_out, int32_t* prim_out,
                           ptx_stats* stats);

/* Diagnostic, in the family of ptx_math_eval: the walks the bounce kernels run on LDS-resident scenes -- which ptx_intersect_rays,
 * whose kernel has its own node loop, does not -- on explicit rays.  Arguments and results as ptx_intersect_rays (prim_out = -1 and
 * t_out = 0 on a miss).  `walk` names one walk; a walk the scene cannot take is PTX_ERR_STATE, and so is a host-only scene:
 *   SHARED_ASM   the assembly node loop on the shared LDS image          Simd_leaf, LDS-resident
 *   OCT_ASM      the assembly node loop on the per-octant LDS image      Simd_leaf, the per-octant image exists and a launch fits with it
 *   SHARED_DIV   the divergent node loop on the shared LDS image         Array_leaf, LDS-resident
 *   PACKET       the camera rays' wave-packet walk                       LDS-resident, either leaf kind
 *   ..._ZERO     the camera launch's form of the first three: the origin is taken as (+0, +0, +0) without being read
 *   ..._TAIL     the first three with the tail cut: a chunk of 64 rays stops once fewer than 16 are walking, and the walks it cut
 *                short are resumed from (node, closest hit) as the bounce kernels resume their parked walks
 * PACKET and the _ZERO walks need every origin component to have the bits of +0.0: anything else (-0.0 included) is PTX_ERR_ARG.
 * Nothing is launched when an error is returned; n == 0 returns 0. */
#define PTX_WALK_SHARED_ASM 0
#define PTX_WALK_OCT_ASM 1
#define PTX_WALK_SHARED_DIV 2
#define PTX_WALK_PACKET 3
#define PTX_WALK_SHARED_ASM_ZERO 4
#define PTX_WALK_OCT_ASM_ZERO 5
#define PTX_WALK_SHARED_DIV_ZERO 6
#define PTX_WALK_SHARED_ASM_TAIL 7
#define PTX_WALK_OCT_ASM_TAIL 8
#define PTX_WALK_SHARED_DIV_TAIL 9
int32_t ptx_walk_rays(ptx_scene* scene, int32_t walk, int64_t n, const double* origins, const double* directions,
                      double* t_out, int32_t* prim_out);

/* Diagnostic, beside ptx_walk_rays: the BOX DECISIONS of the walks that have a node loop of their own (SHARED_ASM, OCT_ASM,
 * SHARED_DIV and their _ZERO forms; PACKET and the _TAIL walks are PTX_ERR_ARG), one leaf at a time.  Per triple i: the ray
 * (origins, directions: 3 doubles each), nodes[i] = a node in the numbering of ptx_scene_tree and t_max[i] = the closest hit so far.
 * leaf_out[i] = the first slot of the next leaf whose box test the walk passes, starting with the visit of nodes[i] (the order of a
 * walk resumed there: near child first on a hit, on past the subtree on a miss), or -1 when the walk runs off the tree first.  No
 * leaf is entered, so t_max stays what the caller gave and the result depends on box decisions alone: the binary32 filter's, the
 * nested-interval rule's and the binary64 test's, made by the production node loops.
 * Errors as ptx_walk_rays'; also PTX_ERR_ARG for a node outside 0 .. n_nodes - 1 and for a t_max that is NaN or negative.  Nothing is
 * launched when an error is returned; n == 0 returns 0. */
int32_t ptx_walk_next_leaf(ptx_scene* scene, int32_t walk, int64_t n, const double* origins, const double* directions,
                           const int32_t* nodes, const double* t_max, int32_t* leaf_out);

/* Diagnostic, for the test suite's coverage record: the instantiations of the four hot kernel families (k_trace, k_shade_pool,
 * k_bounce_carry, k_bounce) the library is built with, and which of them a handle has launched.
 * ptx_kernel_table: every family's selector walked over the whole cube of its arguments in a fixed order; an instantiation is entered
 * the first time it is returned, under a name made of the arguments that returned it ("k_bounce/array/count/lit/queued/hbm/plain/img").
 * Returns the number of instantiations; names_out (NULL: the count alone) receives the names in table order, each followed by '\n',
 * then a NUL -- PTX_ERR_ARG when `capacity` bytes do not hold them.  Needs no device.
 * ptx_scene_launched_kernels: the table indices, ascending, of the instantiations launched on this handle since it was created or
 * since ptx_scene_clear_launched_kernels -- the pointers handed to the launches themselves, not a schedule read again.  Returns their
 * number; PTX_ERR_ARG for a NULL scene, a NULL buffer and a `capacity` (in entries) that does not hold them (nothing is written).
 * A host-only scene has launched nothing.  Clearing while a render runs on the scene is PTX_ERR_STATE. */
int32_t ptx_kernel_table(char* names_out, int64_t capacity);
int32_t ptx_scene_launched_kernels(const ptx_scene* scene, int32_t* indices_out, int32_t capacity);
int32_t ptx_scene_clear_launched_kernels(ptx_scene* scene);

/* Replaces Progressive_photon_map.Make(Scene).go (:420-451) up to, but not including, the per-iteration
 * gamma + PNG write: img_sum_out (HOST, width*height*3, row 0 = top as Bimage stores it) receives the
 * reference's img_sum after `iterations` iterations, i.e. the sum over iterations of estimate / photon_count.
 * Scene.bbox is the bounding box of the scene's tree; the eye pass and the photon pass use the scene's camera.
 * iteration_cb (optional) is called on the calling thread after every iteration with the running img_sum.
 * The light table is checked before anything is allocated or launched: PTX_ERR_ARG for a light whose power, colour or position
 * is not finite, whose power x colour has a negative component, for a spot direction of zero length, and for lights whose total
 * power is not positive, and ("BUG: no photons") when every light's share of photon_count truncates to no path at all.
 * PTX_ERR_STATE ("BUG: no photons") when paths were traced and an iteration stored no photon. */
typedef void (*ptx_ppm_iteration_fn)(void* user, int32_t iteration, double radius, int64_t photon_map_length,
                                     const double* img_sum);
int32_t ptx_ppm_render(ptx_scene* scene, const ptx_ppm_params* params, const ptx_light* lights, int32_t n_lights,
                       double* img_sum_out, ptx_ppm_stats* stats, ptx_ppm_iteration_fn iteration_cb, void* user);

/* Flattened tree, for inspection / parity of the builder: returns the node count and,
 * if the pointers are non-NULL, copies per node: bbox (6 doubles: min xyz, max xyz),
 * and 4 ints: {is_leaf, axis (0,1,2; -1 for leaves), lhs | first slot, rhs | slot count}.
 * prim_order (optional) receives, per leaf slot, the build-list primitive index or -1
 * for a NaN padding slot. */
int32_t ptx_scene_tree(const ptx_scene* scene, double* bbox_out, int32_t* info_out,
                       int32_t node_capacity, int32_t* prim_order_out, int32_t slot_capacity);

/* Sampler: Low_discrepancy_sequence.create / get evaluated on the device
 * (low_discrepancy_sequence.ml:27-36): out[i] = get ~offset:offsets[i] ~dimension:dims[i]
 * for a sampler of `dimension` dimensions. */
int32_t ptx_lds_sample(int32_t device, int32_t dimension, int64_t n, const int32_t* offsets,
                       const int32_t* dims, double* out);

/* pt_math.h functions evaluated on the device, for the host==device bit-identity test.
 * fn: 0 hypot(a,b) 1 sin(a) 2 cos(a) 3 acos(a) 4 atan2(a,b) 5 pow5(a) 6 sqrt(a) 7 a/b
 *     8 fma(a,b,b) */
int32_t ptx_math_eval(int32_t device, int32_t fn, int64_t n, const double* a, const double* b,
                      double* out);

/* Diagnostic (parity tooling, tools/diag_scatter.py): the state of the listed paths after ONE segment (camera ray,
 * trace, shade of bounce 0) -- alive_out[i] = 1 with ray_out[6i..] = (origin, direction) and attn_out[3i..] when
 * sample i scattered, 0 when it terminated.  This is how the hipcc miscompile of the dielectric branch was isolated
 * (DESIGN.md section 2).  Not part of the rendering path; needs max_bounces >= 2. */
int32_t ptx_debug_first_scatter(ptx_scene* scene, const ptx_render_params* params, int64_t n, const int32_t* xs,
                                const int32_t* ys, const int32_t* passes, double* ray_out, double* attn_out,
                                int32_t* alive_out);

#ifdef __cplusplus
}
#endif
#endif /* PTX_H */
