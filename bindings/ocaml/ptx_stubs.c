/* ptx_stubs.c -- OCaml C stubs for libptx_hip.so (include/ptx.h), bound by ptx.ml's `external`s.
 *
 * Same kind of binding as the reference's only FFI, `external spheres_intersect_native ... [@@noalloc]` and
 * `external leaf_size` (shirley_spheres/bin/main.ml:162-172, implemented in sphere-intersect-rs/src/lib.rs:15-18,53-76
 * and linked by shirley_spheres/bin/dune:8-33): plain `external` C symbols, OCaml values unpacked by hand, pointers
 * BORROWED for the duration of the call -- but one call per render instead of one per BVH leaf per ray.
 *
 * Needs the OCaml runtime headers (<caml/...>), so it is not compiled into anything in this repository's image; the
 * marshalling it performs lives in ptx_ml_marshal.h and is exercised without OCaml by tests/test_ocaml_binding.py, which
 * also type-checks THIS file (gcc -fsyntax-only) against minimal declarations of the runtime's API (tests/c/mock_caml).
 *
 * Value conventions:
 *   floatarray          Double_array_tag block: (double*) v is the flat data, Wosize_val(v) / Double_wosize the length
 *                       (the reference reads `coords` the same way: header >> 10 words, lib.rs:26-36)
 *   Bigarray.Array1     Caml_ba_data_val(v), Caml_ba_array_val(v)->dim[0]
 *   int                 Long_val / Val_long
 *   scene handle        custom block holding the ptx_scene* and an in-use count, finalised with ptx_scene_destroy.  The count
 *                       is raised for the duration of a render (which runs with the runtime lock released): Ptx.scene_destroy
 *                       from another thread or domain meanwhile raises Failure instead of freeing what the render reads
 *   errors              caml_failwith (ptx_last_error ()): no error code ever reaches OCaml unraised
 *   callbacks           update_progress / on_iteration run on the CALLING thread (the library's contract).  The runtime
 *                       lock is RELEASED for the duration of the render (other domains and threads keep running; the
 *                       reference's own integrator leaves them running too) and re-taken around each callback.  A
 *                       callback that raises does not unwind through the library's C++ frames: the exception is caught
 *                       (caml_callback_exn), kept, no further callbacks are made, and it is re-raised after the library
 *                       call has returned.
 */
#define CAML_NAME_SPACE
#include <caml/alloc.h>
#include <caml/bigarray.h>
#include <caml/callback.h>
#include <caml/custom.h>
#include <caml/fail.h>
#include <caml/memory.h>
#include <caml/mlvalues.h>
#include <caml/threads.h>

#include <stdlib.h>

#include "ptx_ml_marshal.h"

typedef struct ptx_ml_handle {
  ptx_scene* scene;
  /* renders running on the scene right now (atomic: OCaml 5 domains run in parallel); + PTX_ML_EXCLUSIVE while image_pin /
   * image_unpin change what a render reads (the registered image): they need the scene to themselves */
  int in_use;
  /* the pinned image, kept alive from here: a generational global root in a malloc'ed cell (a custom block's own data may move
   * with the block, a root's address may not), NULL while nothing is pinned.  While it exists the Bigarray cannot be collected,
   * so neither a pin that outlives the caller's last reference nor the finaliser (whose order against the image's is not
   * defined) can leave the library holding a registration of freed memory. */
  value* pin_root;
} ptx_ml_handle;
#define PTX_ML_EXCLUSIVE (1 << 20)
#define Handle_val(v) ((ptx_ml_handle*)Data_custom_val(v))
#define Scene_val(v) (Handle_val(v)->scene)

static void ptx_ml_drop_pin_root(ptx_ml_handle* h) {
  if (h->pin_root) {
    caml_remove_generational_global_root(h->pin_root);
    free(h->pin_root);
    h->pin_root = NULL;
  }
}
/* the finaliser: runs only when nothing reaches the handle any more, so no render can be using it.  ptx_scene_destroy ends the
 * pin (the image is still alive: the root below is dropped after it) */
static void ptx_ml_scene_finalize(value v) {
  if (Scene_val(v)) {
    ptx_scene_destroy(Scene_val(v));
    Scene_val(v) = NULL;
  }
  ptx_ml_drop_pin_root(Handle_val(v));
}
/* a render takes the scene for the time the runtime lock is released; NULL = already destroyed, or being re-pinned (*busy) */
static ptx_scene* ptx_ml_scene_acquire(value handle, int* busy) {
  ptx_ml_handle* h = Handle_val(handle);
  *busy = 0;
  const int n = __atomic_add_fetch(&h->in_use, 1, __ATOMIC_ACQ_REL);
  ptx_scene* s = __atomic_load_n(&h->scene, __ATOMIC_ACQUIRE);
  if (n >= PTX_ML_EXCLUSIVE) { /* image_pin / image_unpin is at work on another thread or domain */
    *busy = 1;
    s = NULL;
  }
  if (!s) __atomic_sub_fetch(&h->in_use, 1, __ATOMIC_ACQ_REL);
  return s;
}
static void ptx_ml_scene_release(value handle) { __atomic_sub_fetch(&Handle_val(handle)->in_use, 1, __ATOMIC_ACQ_REL); }
/* image_pin / image_unpin: the scene with NO render running, and none starting until ptx_ml_scene_release_exclusive.
 * 1 = taken; 0 = a render (or another pin) is running: nothing changed */
static int ptx_ml_scene_acquire_exclusive(value handle) {
  ptx_ml_handle* h = Handle_val(handle);
  if (__atomic_add_fetch(&h->in_use, PTX_ML_EXCLUSIVE, __ATOMIC_ACQ_REL) != PTX_ML_EXCLUSIVE) {
    __atomic_sub_fetch(&h->in_use, PTX_ML_EXCLUSIVE, __ATOMIC_ACQ_REL);
    return 0;
  }
  return 1;
}
static void ptx_ml_scene_release_exclusive(value handle) { __atomic_sub_fetch(&Handle_val(handle)->in_use, PTX_ML_EXCLUSIVE, __ATOMIC_ACQ_REL); }

static struct custom_operations ptx_ml_scene_ops = {
    "dalev.path_tracer.ptx_scene", ptx_ml_scene_finalize, custom_compare_default, custom_hash_default,
    custom_serialize_default,       custom_deserialize_default, custom_compare_ext_default, custom_fixed_length_default};

static const double* floatarray_data(value v) { return (const double*)v; }
static int32_t floatarray_length(value v) { return (int32_t)(Wosize_val(v) / Double_wosize); }
static int32_t int32_ba_length(value v) { return (int32_t)Caml_ba_array_val(v)->dim[0]; }
static const int32_t* int32_ba_data(value v) { return (const int32_t*)Caml_ba_data_val(v); }

/* external leaf_size : unit -> int = "ptx_ml_leaf_size"   (replaces `leaf_size`, lib.rs:15-18) */
CAMLprim value ptx_ml_leaf_size(value unit) {
  (void)unit;
  return Val_long(ptx_leaf_size());
}

/* external device_count : unit -> int = "ptx_ml_device_count" */
CAMLprim value ptx_ml_device_count(value unit) {
  (void)unit;
  return Val_long(ptx_device_count());
}

/* external scene_create_flat : flat -> int -> scene = "ptx_ml_scene_create_stub"
 * flat = { xs; ys; zs; rs; sphere_material; materials; textures; camera; background; leaf_kind; length_cutoff;
 *          vertex_x; vertex_y; vertex_z; tri_indices; tri_uv; tri_material; floor_vertices; floor_uv; floor_material }
 * (field order of Ptx.flat in ptx.ml) */
CAMLprim value ptx_ml_scene_create_stub(value flat, value device) {
  CAMLparam2(flat, device);
  CAMLlocal1(handle);
  ptx_ml_flat f;
  memset(&f, 0, sizeof f);
  f.xs = floatarray_data(Field(flat, 0));
  f.ys = floatarray_data(Field(flat, 1));
  f.zs = floatarray_data(Field(flat, 2));
  f.rs = floatarray_data(Field(flat, 3));
  f.n_spheres = floatarray_length(Field(flat, 0));
  if (floatarray_length(Field(flat, 1)) != f.n_spheres || floatarray_length(Field(flat, 2)) != f.n_spheres ||
      floatarray_length(Field(flat, 3)) != f.n_spheres || int32_ba_length(Field(flat, 4)) != f.n_spheres)
    caml_invalid_argument("Ptx.scene_create: sphere arrays differ in length");
  f.sphere_material = int32_ba_data(Field(flat, 4));
  f.materials = floatarray_data(Field(flat, 5));
  f.n_materials = floatarray_length(Field(flat, 5)) / 6;
  f.textures = floatarray_data(Field(flat, 6));
  f.n_textures = floatarray_length(Field(flat, 6)) / 9;
  if (floatarray_length(Field(flat, 7)) != 4 || floatarray_length(Field(flat, 8)) != 7)
    caml_invalid_argument("Ptx.scene_create: camera needs 4 floats, background 7");
  f.camera = floatarray_data(Field(flat, 7));
  f.background = floatarray_data(Field(flat, 8));
  f.leaf_kind = (int32_t)Long_val(Field(flat, 9));
  f.length_cutoff = (int32_t)Long_val(Field(flat, 10));
  /* the triangle mesh (ganesha Mesh.t / cornell-box Face.t) */
  f.n_vertices = floatarray_length(Field(flat, 11));
  if (floatarray_length(Field(flat, 12)) != f.n_vertices || floatarray_length(Field(flat, 13)) != f.n_vertices)
    caml_invalid_argument("Ptx.scene_create: vertex arrays differ in length");
  f.vertex_x = floatarray_data(Field(flat, 11));
  f.vertex_y = floatarray_data(Field(flat, 12));
  f.vertex_z = floatarray_data(Field(flat, 13));
  f.n_triangles = int32_ba_length(Field(flat, 14)) / 3;
  if (int32_ba_length(Field(flat, 14)) != 3 * f.n_triangles || floatarray_length(Field(flat, 15)) != 6 * f.n_triangles ||
      int32_ba_length(Field(flat, 16)) != f.n_triangles)
    caml_invalid_argument("Ptx.scene_create: a mesh needs 3 indices, 6 texture coordinates and 1 material per triangle");
  f.tri_indices = int32_ba_data(Field(flat, 14));
  f.tri_uv = floatarray_data(Field(flat, 15));
  f.tri_material = int32_ba_data(Field(flat, 16));
  /* triangles tested before the tree (ganesha Floor) */
  f.n_floor_triangles = int32_ba_length(Field(flat, 19));
  if (floatarray_length(Field(flat, 17)) != 9 * f.n_floor_triangles || floatarray_length(Field(flat, 18)) != 6 * f.n_floor_triangles)
    caml_invalid_argument("Ptx.scene_create: a floor triangle needs 9 coordinates and 6 texture coordinates");
  f.floor_vertices = floatarray_data(Field(flat, 17));
  f.floor_uv = floatarray_data(Field(flat, 18));
  f.floor_material = int32_ba_data(Field(flat, 19));
  /* no OCaml allocation between reading the pointers above and the end of ptx_ml_scene_create: nothing can move
   * (the runtime lock stays held here: the floatarrays live in the OCaml heap) */
  ptx_scene* s = ptx_ml_scene_create(&f, (int32_t)Long_val(device));
  if (!s) caml_failwith(ptx_ml_scene_create_error());
  handle = caml_alloc_custom(&ptx_ml_scene_ops, sizeof(ptx_ml_handle), 0, 1);
  Handle_val(handle)->scene = s;
  Handle_val(handle)->in_use = 0;
  Handle_val(handle)->pin_root = NULL;
  CAMLreturn(handle);
}

/* external scene_destroy : scene -> unit = "ptx_ml_scene_destroy_stub"   (optional: the finaliser does the same) */
CAMLprim value ptx_ml_scene_destroy_stub(value handle) {
  ptx_ml_handle* h = Handle_val(handle);
  /* take the scene out of the handle first, then look at the count: a render that starts after this sees NULL, one that
   * started before it is counted */
  ptx_scene* s = __atomic_exchange_n(&h->scene, NULL, __ATOMIC_ACQ_REL);
  if (!s) return Val_unit;
  if (__atomic_load_n(&h->in_use, __ATOMIC_ACQUIRE) > 0) {
    __atomic_store_n(&h->scene, s, __ATOMIC_RELEASE); /* put it back: the finaliser or a later call frees it */
    caml_failwith("Ptx.scene_destroy: a render is running on this scene");
  }
  ptx_scene_destroy(s); /* (ends a pin) */
  ptx_ml_drop_pin_root(h);
  return Val_unit;
}

/* external scene_tree_stats : scene -> int * int * int * int = "ptx_ml_scene_tree_stats_stub"   (depth, nodes, leaves, slots) */
CAMLprim value ptx_ml_scene_tree_stats_stub(value handle) {
  CAMLparam1(handle);
  CAMLlocal1(tuple);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.scene_tree_stats: scene already destroyed");
  ptx_stats st;
  if (ptx_scene_stats(s, &st) != 0) caml_failwith(ptx_last_error());
  tuple = caml_alloc_tuple(4);
  Store_field(tuple, 0, Val_long(st.tree_depth));
  Store_field(tuple, 1, Val_long(st.tree_nodes));
  Store_field(tuple, 2, Val_long(st.tree_leaves));
  Store_field(tuple, 3, Val_long(st.leaf_slots));
  CAMLreturn(tuple);
}

/* external image_pin : scene -> image -> unit = "ptx_ml_image_pin_stub" / external image_unpin : scene -> unit (ptx_image_pin).
 * Both change the registration a running render reads (its last step is the DMA into the image): they take the scene
 * exclusively and raise Failure while a render runs on another thread or domain; a render that starts meanwhile raises Failure
 * too.  The pinned Bigarray is kept alive from the handle (ptx_ml_handle.pin_root). */
CAMLprim value ptx_ml_image_pin_stub(value handle, value image) {
  CAMLparam2(handle, image);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.image_pin: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.image_pin: a render is running on this scene");
  ptx_ml_handle* h = Handle_val(handle); /* (nothing below allocates on the OCaml heap: the block does not move) */
  ptx_scene* s = __atomic_load_n(&h->scene, __ATOMIC_ACQUIRE);
  int32_t rc = -1;
  if (s) rc = ptx_image_pin(s, (double*)Caml_ba_data_val(image), (int64_t)Caml_ba_array_val(image)->dim[0]);
  if (s && rc == 0) {
    if (!h->pin_root) {
      h->pin_root = (value*)malloc(sizeof(value));
      if (h->pin_root) {
        *h->pin_root = image;
        caml_register_generational_global_root(h->pin_root);
      } else { /* no cell for the root: do not keep a pin nothing keeps alive */
        (void)ptx_image_unpin(s);
        rc = -1;
      }
    } else {
      caml_modify_generational_global_root(h->pin_root, image);
    }
  } else if (s) {
    ptx_ml_drop_pin_root(h); /* ptx_image_pin ends the previous pin before it tries the new one */
  }
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.image_pin: scene already destroyed");
  if (rc != 0) caml_failwith(h->pin_root || rc != -1 ? ptx_last_error() : "Ptx.image_pin: out of memory");
  CAMLreturn(Val_unit);
}
CAMLprim value ptx_ml_image_unpin_stub(value handle) {
  CAMLparam1(handle);
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.image_unpin: a render is running on this scene");
  ptx_ml_handle* h = Handle_val(handle);
  ptx_scene* s = __atomic_load_n(&h->scene, __ATOMIC_ACQUIRE);
  if (s) (void)ptx_image_unpin(s);
  ptx_ml_drop_pin_root(h);
  ptx_ml_scene_release_exclusive(handle);
  CAMLreturn(Val_unit);
}

/* external set_lighting_int : scene -> int -> unit = "ptx_ml_set_lighting_stub" (ptx_scene_set_lighting; Ptx.set_lighting maps the
 * variant).  The mode changes what a running render launches next: like image_pin it takes the scene exclusively and raises Failure
 * while a render runs on another thread or domain. */
CAMLprim value ptx_ml_set_lighting_stub(value handle, value mode) {
  CAMLparam2(handle, mode);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_lighting: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_lighting: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_scene_set_lighting(s, (int32_t)Long_val(mode));
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_lighting: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external set_film_int : scene -> int -> int -> int -> unit = "ptx_ml_set_film_stub" (ptx_scene_set_film: order, pixel_radius,
 * flags; Ptx.set_film maps ~renormalise).  The film is what a running render applies at its end: like set_lighting it takes the scene
 * exclusively and raises Failure while a render runs on another thread or domain, and Failure with the library's message for a
 * refused (order, pixel_radius). */
CAMLprim value ptx_ml_set_film_stub(value handle, value order, value pixel_radius, value flags) {
  CAMLparam4(handle, order, pixel_radius, flags);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_film: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_film: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_set_film(s, (int32_t)Long_val(order), (int32_t)Long_val(pixel_radius), (int32_t)Long_val(flags));
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_film: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external set_texture_image_raw : scene -> int -> int * int * int -> texels -> unit = "ptx_ml_set_texture_image_stub"
 * (ptx_scene_set_texture_image: the entry, (width, height, flags), width * height * 3 doubles; (0, 0, _) restores the descriptor's
 * texture).  What a running render shades with: like set_lighting it takes the scene exclusively and raises Failure while a render
 * runs on another thread or domain, and Failure with the library's message for a refused image. */
CAMLprim value ptx_ml_set_texture_image_stub(value handle, value index, value dims, value texels) {
  CAMLparam4(handle, index, dims, texels);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_texture_image: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_texture_image: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s)
    rc = ptx_ml_set_texture_image(s, (int32_t)Long_val(index), (int32_t)Long_val(Field(dims, 0)), (int32_t)Long_val(Field(dims, 1)),
                                  (int32_t)Long_val(Field(dims, 2)), (const double*)Caml_ba_data_val(texels),
                                  (int64_t)Caml_ba_array_val(texels)->dim[0]);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_texture_image: scene already destroyed");
  if (rc == -4) caml_invalid_argument("Ptx.set_texture_image: the texels hold fewer than width * height * 3 doubles");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external set_environment_raw : scene -> int * int * int -> texels -> texels -> unit = "ptx_ml_set_environment_stub"
 * (ptx_scene_set_environment: (width, height, flags), the texels, the 9 doubles of the rotation or an empty Bigarray for the
 * identity; (0, 0, _) restores the descriptor's background) */
CAMLprim value ptx_ml_set_environment_stub(value handle, value dims, value texels, value rotation) {
  CAMLparam4(handle, dims, texels, rotation);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_environment: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_environment: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s)
    rc = ptx_ml_set_environment(s, (int32_t)Long_val(Field(dims, 0)), (int32_t)Long_val(Field(dims, 1)), (int32_t)Long_val(Field(dims, 2)),
                                (const double*)Caml_ba_data_val(texels), (int64_t)Caml_ba_array_val(texels)->dim[0],
                                (const double*)Caml_ba_data_val(rotation), (int64_t)Caml_ba_array_val(rotation)->dim[0]);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_environment: scene already destroyed");
  if (rc == -4) caml_invalid_argument("Ptx.set_environment: the texels hold fewer than width * height * 3 doubles");
  if (rc == -5) caml_invalid_argument("Ptx.set_environment: the rotation must hold 9 doubles (row-major 3 x 3)");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external set_environment_sampling_int : scene -> int -> unit = "ptx_ml_set_environment_sampling_stub"
 * (ptx_scene_set_environment_sampling).  What a running render samples: like set_lighting it takes the scene exclusively and raises
 * Failure while a render runs on another thread or domain, and Failure with the library's message for a refused call. */
CAMLprim value ptx_ml_set_environment_sampling_stub(value handle, value on) {
  CAMLparam2(handle, on);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_environment_sampling: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_environment_sampling: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_scene_set_environment_sampling(s, Long_val(on) != 0 ? 1 : 0);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_environment_sampling: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external environment_sampling_raw : scene -> int * float = "ptx_ml_environment_sampling_stub" (ptx_scene_environment_sampling) */
CAMLprim value ptx_ml_environment_sampling_stub(value handle) {
  CAMLparam1(handle);
  CAMLlocal2(tuple, total_v);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.environment_sampling: scene already destroyed");
  int32_t on = 0;
  double total = 0.0;
  if (ptx_scene_environment_sampling(s, &on, &total) != 0) caml_failwith(ptx_last_error());
  total_v = caml_copy_double(total);
  tuple = caml_alloc_tuple(2);
  Store_field(tuple, 0, Val_long(on));
  Store_field(tuple, 1, total_v);
  CAMLreturn(tuple);
}

/* external set_sphere_light_sampling_int : scene -> int -> unit = "ptx_ml_set_sphere_light_sampling_stub"
 * (ptx_scene_set_sphere_light_sampling).  What a running render samples: like set_lighting it takes the scene exclusively and raises
 * Failure while a render runs on another thread or domain, and Failure with the library's message for a refused call. */
CAMLprim value ptx_ml_set_sphere_light_sampling_stub(value handle, value on) {
  CAMLparam2(handle, on);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_sphere_light_sampling: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_sphere_light_sampling: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_scene_set_sphere_light_sampling(s, Long_val(on) != 0 ? 1 : 0);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_sphere_light_sampling: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external sphere_lights_raw : scene -> int * int * float = "ptx_ml_sphere_lights_stub" (ptx_scene_sphere_lights) */
CAMLprim value ptx_ml_sphere_lights_stub(value handle) {
  CAMLparam1(handle);
  CAMLlocal2(tuple, total_v);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.sphere_lights: scene already destroyed");
  int32_t on = 0, n = 0;
  double total = 0.0;
  if (ptx_scene_sphere_lights(s, &on, &n, &total) != 0) caml_failwith(ptx_last_error());
  total_v = caml_copy_double(total);
  tuple = caml_alloc_tuple(3);
  Store_field(tuple, 0, Val_long(on));
  Store_field(tuple, 1, Val_long(n));
  Store_field(tuple, 2, total_v);
  CAMLreturn(tuple);
}

/* external set_lens_raw : scene -> texels -> unit = "ptx_ml_set_lens_stub" (ptx_scene_set_lens: a Bigarray of the two doubles radius,
 * focus_distance, as the other stubs take their doubles; radius 0 switches the lens off).  What a running render's camera rays are made of: like set_lighting it takes the scene exclusively and raises
 * Failure while a render runs on another thread or domain, and Failure with the library's message for a refused pair. */
CAMLprim value ptx_ml_set_lens_stub(value handle, value pair) {
  CAMLparam2(handle, pair);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_lens: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_lens: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_set_lens(s, (const double*)Caml_ba_data_val(pair), (int64_t)Caml_ba_array_val(pair)->dim[0]);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_lens: scene already destroyed");
  if (rc == -4) caml_invalid_argument("Ptx.set_lens: the pair must hold 2 doubles (radius, focus_distance)");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external lens : scene -> float * float = "ptx_ml_lens_stub" (ptx_scene_lens: radius, focus_distance) */
CAMLprim value ptx_ml_lens_stub(value handle) {
  CAMLparam1(handle);
  CAMLlocal3(tuple, radius_v, focus_v);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.lens: scene already destroyed");
  double radius = 0.0, focus = 0.0;
  if (ptx_ml_lens(s, &radius, &focus) != 0) caml_failwith(ptx_last_error());
  radius_v = caml_copy_double(radius);
  focus_v = caml_copy_double(focus);
  tuple = caml_alloc_tuple(2);
  Store_field(tuple, 0, radius_v);
  Store_field(tuple, 1, focus_v);
  CAMLreturn(tuple);
}

/* external set_camera_pose_raw : scene -> doubles -> doubles -> unit = "ptx_ml_set_camera_pose_stub" (ptx_scene_set_camera_pose: a
 * Bigarray of the 12 doubles origin, rotation -- or an empty one -- and one of the 4 doubles of the view -- or an empty one).  What a
 * running render's camera rays are made of: like set_lens it takes the scene exclusively and raises Failure while a render runs on
 * another thread or domain, and Failure with the library's message for a refused pose. */
CAMLprim value ptx_ml_set_camera_pose_stub(value handle, value pose, value view) {
  CAMLparam3(handle, pose, view);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_camera_pose: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_camera_pose: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s)
    rc = ptx_ml_set_camera_pose(s, (const double*)Caml_ba_data_val(pose), (int64_t)Caml_ba_array_val(pose)->dim[0],
                                (const double*)Caml_ba_data_val(view), (int64_t)Caml_ba_array_val(view)->dim[0]);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_camera_pose: scene already destroyed");
  if (rc == -4) caml_invalid_argument("Ptx.set_camera_pose: the pose must hold 12 doubles or none, the view 4 or none, and one of them be given");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external clear_camera_pose : scene -> unit = "ptx_ml_clear_camera_pose_stub" (ptx_scene_set_camera_pose(scene, NULL, NULL, NULL)) */
CAMLprim value ptx_ml_clear_camera_pose_stub(value handle) {
  CAMLparam1(handle);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.clear_camera_pose: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.clear_camera_pose: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_clear_camera_pose(s);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.clear_camera_pose: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external camera_pose_raw : scene -> doubles -> int = "ptx_ml_camera_pose_stub" (ptx_scene_camera_pose into a Bigarray of 16 doubles:
 * origin, rotation, the view in effect; 1 = on, 0 = off) */
CAMLprim value ptx_ml_camera_pose_stub(value handle, value out) {
  CAMLparam2(handle, out);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.camera_pose: scene already destroyed");
  const int32_t rc = ptx_ml_camera_pose(s, (double*)Caml_ba_data_val(out), (int64_t)Caml_ba_array_val(out)->dim[0]);
  if (rc == -4) caml_invalid_argument("Ptx.camera_pose: the output must hold 16 doubles");
  if (rc < 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_int(rc));
}

/* external set_camera_shutter_raw : scene -> doubles -> unit = "ptx_ml_set_camera_shutter_stub" (ptx_scene_set_camera_shutter: a Bigarray
 * of the 7 doubles translation, axis, angle).  What a running render's camera rays are made of: like set_camera_pose it takes the scene
 * exclusively and raises Failure while a render runs on another thread or domain, and Failure with the library's message for a refused
 * shutter. */
CAMLprim value ptx_ml_set_camera_shutter_stub(value handle, value motion) {
  CAMLparam2(handle, motion);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_camera_shutter: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_camera_shutter: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_set_camera_shutter(s, (const double*)Caml_ba_data_val(motion), (int64_t)Caml_ba_array_val(motion)->dim[0]);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_camera_shutter: scene already destroyed");
  if (rc == -4) caml_invalid_argument("Ptx.set_camera_shutter: the motion must hold 7 doubles");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external clear_camera_shutter : scene -> unit = "ptx_ml_clear_camera_shutter_stub" (ptx_scene_set_camera_shutter(scene, NULL, NULL, 0)) */
CAMLprim value ptx_ml_clear_camera_shutter_stub(value handle) {
  CAMLparam1(handle);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.clear_camera_shutter: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.clear_camera_shutter: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_clear_camera_shutter(s);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.clear_camera_shutter: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external camera_shutter_raw : scene -> doubles -> int = "ptx_ml_camera_shutter_stub" (ptx_scene_camera_shutter into a Bigarray of 7
 * doubles: translation, axis, angle; 1 = on, 0 = off) */
CAMLprim value ptx_ml_camera_shutter_stub(value handle, value out) {
  CAMLparam2(handle, out);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.camera_shutter: scene already destroyed");
  const int32_t rc = ptx_ml_camera_shutter(s, (double*)Caml_ba_data_val(out), (int64_t)Caml_ba_array_val(out)->dim[0]);
  if (rc == -4) caml_invalid_argument("Ptx.camera_shutter: the output must hold 7 doubles");
  if (rc < 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_int(rc));
}

/* external set_camera_projection_int : scene -> int -> unit = "ptx_ml_set_camera_projection_stub" (ptx_scene_set_camera_projection).  What
 * a running render's camera rays are made of: like set_lens it takes the scene exclusively and raises Failure while a render runs on
 * another thread or domain, and Failure with the library's message for a refused projection (an unknown kind, LATLONG under a lens). */
CAMLprim value ptx_ml_set_camera_projection_stub(value handle, value projection) {
  CAMLparam2(handle, projection);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.set_camera_projection: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.set_camera_projection: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_set_camera_projection(s, (int32_t)Int_val(projection));
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.set_camera_projection: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* external camera_projection_int : scene -> int = "ptx_ml_camera_projection_stub" (ptx_scene_camera_projection: 0 or 1) */
CAMLprim value ptx_ml_camera_projection_stub(value handle) {
  CAMLparam1(handle);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.camera_projection: scene already destroyed");
  const int32_t rc = ptx_ml_camera_projection(s);
  if (rc < 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_int(rc));
}

/* external render_rays_flat : scene -> floatarray -> doubles -> doubles -> int32s -> doubles -> doubles -> unit
 * = "ptx_ml_render_rays_stub_bytecode" "ptx_ml_render_rays_stub" (scene, the 3 floats of ptx_ml_render_rays, origins (3 n), directions
 * (3 n), offsets (n or empty), sums (3 n / m), squares (as many or empty)).  No callback runs, so nothing can raise while the lock is
 * released. */
CAMLprim value ptx_ml_render_rays_stub(value handle, value params, value origins, value directions, value offsets, value sums, value sq) {
  CAMLparam5(handle, params, origins, directions, offsets);
  CAMLxparam2(sums, sq);
  if (floatarray_length(params) != 3) caml_invalid_argument("Ptx.render_rays: params needs 3 floats");
  double p3[3];
  memcpy(p3, floatarray_data(params), sizeof p3);
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_rays: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_rays: scene already destroyed");
  /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  const double* o = (const double*)Caml_ba_data_val(origins);
  const double* d = (const double*)Caml_ba_data_val(directions);
  const int32_t* off = (const int32_t*)Caml_ba_data_val(offsets);
  double* sum_out = (double*)Caml_ba_data_val(sums);
  double* sq_out = (double*)Caml_ba_data_val(sq);
  const int64_t n_o = (int64_t)Caml_ba_array_val(origins)->dim[0], n_d = (int64_t)Caml_ba_array_val(directions)->dim[0];
  const int64_t n_off = (int64_t)Caml_ba_array_val(offsets)->dim[0], n_sum = (int64_t)Caml_ba_array_val(sums)->dim[0];
  const int64_t n_sq = (int64_t)Caml_ba_array_val(sq)->dim[0];
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_rays(s, p3, o, n_o, d, n_d, off, n_off, sum_out, n_sum, sq_out, n_sq);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (rc == -4)
    caml_invalid_argument("Ptx.render_rays: origins and directions hold 3 floats a ray, offsets one a ray or none, sums and squares 3 a bin");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* bytecode entry of the 7-argument external */
CAMLprim value ptx_ml_render_rays_stub_bytecode(value* argv, int argn) {
  (void)argn;
  return ptx_ml_render_rays_stub(argv[0], argv[1], argv[2], argv[3], argv[4], argv[5], argv[6]);
}

/* external film_int : scene -> int * int * int = "ptx_ml_film_stub" (ptx_scene_film: order, pixel_radius, flags) */
CAMLprim value ptx_ml_film_stub(value handle) {
  CAMLparam1(handle);
  CAMLlocal1(tuple);
  ptx_scene* s = Scene_val(handle);
  if (!s) caml_invalid_argument("Ptx.film: scene already destroyed");
  ptx_film_params f;
  if (ptx_scene_film(s, &f) != 0) caml_failwith(ptx_last_error());
  tuple = caml_alloc_tuple(3);
  Store_field(tuple, 0, Val_long(f.order));
  Store_field(tuple, 1, Val_long(f.pixel_radius));
  Store_field(tuple, 2, Val_long(f.flags));
  CAMLreturn(tuple);
}

/* external film_weights_into : int -> int -> weights -> unit = "ptx_ml_film_weights_stub" (ptx_film_weights, host only): the 2r + 1
 * normalised 1-D weights of Binomial.create ~order ~pixel_radius into a Bigarray of at least 2r + 1 doubles */
CAMLprim value ptx_ml_film_weights_stub(value order, value pixel_radius, value out) {
  CAMLparam3(order, pixel_radius, out);
  const int32_t rc = ptx_ml_film_weights((int32_t)Long_val(order), (int32_t)Long_val(pixel_radius), (double*)Caml_ba_data_val(out),
                                         (int64_t)Caml_ba_array_val(out)->dim[0]);
  if (rc == -4) caml_invalid_argument("Ptx.film_weights: the output holds fewer than 2 * pixel_radius + 1 doubles");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* What a callback trampoline needs: the closure (a GC root registered by the stub that owns this struct) and the first
 * exception a callback raised.  While `raised` is set no further callbacks are made. */
typedef struct ptx_ml_cb {
  value* closure;
  value* exn; /* GC root; Val_unit until a callback raises */
  int raised;
} ptx_ml_cb;

static void ptx_ml_progress(void* user, int64_t pixels_done) {
  ptx_ml_cb* cb = (ptx_ml_cb*)user;
  if (cb->raised) return;
  caml_acquire_runtime_system(); /* the render runs with the lock released */
  value r = caml_callback_exn(*cb->closure, Val_long(pixels_done));
  if (Is_exception_result(r)) {
    *cb->exn = Extract_exception(r);
    cb->raised = 1;
  }
  caml_release_runtime_system();
}

/* external render_flat : scene -> int -> int -> int -> int -> int -> image -> (int -> unit) -> unit
 *   = "ptx_ml_render_stub_bytecode" "ptx_ml_render_stub"
 * (scene, width, height, samples_per_pixel, max_bounces, gpus, Bimage data as a float64 Bigarray of W*H*3, update_progress)
 * replaces Integrator.create ... |> Integrator.render ~update_progress (render_command.ml:71-104) */
CAMLprim value ptx_ml_render_stub(value handle, value width, value height, value spp, value max_bounces, value gpus, value image,
                                  value update_progress) {
  CAMLparam5(handle, width, height, spp, max_bounces);
  CAMLxparam3(gpus, image, update_progress);
  CAMLlocal1(exn);
  const intnat w = Long_val(width), h = Long_val(height);
  if (Caml_ba_array_val(image)->dim[0] != w * h * 3) caml_invalid_argument("Ptx.render: image must hold width * height * 3 floats");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render: scene already destroyed");
  double* out = (double*)Caml_ba_data_val(image); /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  const int32_t i_spp = (int32_t)Long_val(spp), i_mb = (int32_t)Long_val(max_bounces), i_gpus = (int32_t)Long_val(gpus);
  exn = Val_unit;
  ptx_ml_cb cb = {&update_progress, &exn, 0};
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render(s, (int32_t)w, (int32_t)h, i_spp, i_mb, i_gpus, out, ptx_ml_progress, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.raised) caml_raise(exn); /* update_progress raised: the render completed, its exception surfaces here */
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

CAMLprim value ptx_ml_render_stub_bytecode(value* argv, int argn) {
  (void)argn;
  return ptx_ml_render_stub(argv[0], argv[1], argv[2], argv[3], argv[4], argv[5], argv[6], argv[7]);
}

/* runs with the runtime lock held */
static void ptx_ml_call_on_iteration(ptx_ml_cb* cb, int32_t iteration, double radius, int64_t photon_map_length) {
  CAMLparam0();
  CAMLlocal2(boxed_radius, r);
  boxed_radius = caml_copy_double(radius);
  r = caml_callback3_exn(*cb->closure, Val_long(iteration), boxed_radius, Val_long(photon_map_length));
  if (Is_exception_result(r)) {
    *cb->exn = Extract_exception(r);
    cb->raised = 1;
  }
  CAMLreturn0;
}

/* the iteration callback of the library hands over ITS host copy of the running sum; the OCaml side reads its own Bigarray
 * (save_image reads img_sum.data, progressive_photon_map.ml:406-418), so the sum is copied there first */
typedef struct ptx_ml_ppm_cb {
  ptx_ml_cb cb;
  double* img_sum;
  size_t n;
} ptx_ml_ppm_cb;

static void ptx_ml_on_iteration_copy(void* user, int32_t iteration, double radius, int64_t photon_map_length, const double* img_sum) {
  ptx_ml_ppm_cb* p = (ptx_ml_ppm_cb*)user;
  if (p->cb.raised) return;
  memcpy(p->img_sum, img_sum, sizeof(double) * p->n);
  caml_acquire_runtime_system(); /* the render runs with the lock released */
  ptx_ml_call_on_iteration(&p->cb, iteration, radius, photon_map_length);
  caml_release_runtime_system();
}

/* external ppm_render_flat : scene -> floatarray -> floatarray -> img_sum -> (int -> float -> int -> unit) -> unit
 *   = "ptx_ml_ppm_render_stub"
 * replaces the loop of Progressive_photon_map.Make(Scene).go (progressive_photon_map.ml:433-450) */
CAMLprim value ptx_ml_ppm_render_stub(value handle, value params, value lights, value img_sum, value on_iteration) {
  CAMLparam5(handle, params, lights, img_sum, on_iteration);
  CAMLlocal1(exn);
  if (floatarray_length(params) != 6) caml_invalid_argument("Ptx.ppm_render: params needs 6 floats");
  const int32_t n_lights = floatarray_length(lights) / 11;
  if (floatarray_length(lights) != 11 * n_lights || n_lights < 1 || n_lights > 64)
    caml_invalid_argument("Ptx.ppm_render: 1 to 64 lights of 11 floats each");
  /* params / lights live in the OCaml heap and the lock is about to be released: copy them out */
  double p6[6], l11[64 * 11];
  memcpy(p6, floatarray_data(params), sizeof p6);
  memcpy(l11, floatarray_data(lights), sizeof(double) * 11 * (size_t)n_lights);
  const intnat w = (intnat)p6[0], h = (intnat)p6[1];
  if (w <= 0 || h <= 0 || Caml_ba_array_val(img_sum)->dim[0] != w * h * 3)
    caml_invalid_argument("Ptx.ppm_render: img_sum must hold width * height * 3 floats");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.ppm_render: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.ppm_render: scene already destroyed");
  exn = Val_unit;
  ptx_ml_ppm_cb cb = {{&on_iteration, &exn, 0}, (double*)Caml_ba_data_val(img_sum), (size_t)(w * h * 3)};
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_ppm_render(s, p6, l11, n_lights, cb.img_sum, ptx_ml_on_iteration_copy, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.cb.raised) caml_raise(exn);
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* the update callback: the library has already filled the caller's Bigarrays (image, err) when it calls */
typedef struct ptx_ml_update_cb {
  ptx_ml_cb cb;
  int32_t samples_per_pixel; /* N: the update of N passes is the last */
  int stop;                  /* what the closure returned */
} ptx_ml_update_cb;

/* runs with the runtime lock held */
static void ptx_ml_call_on_update(ptx_ml_update_cb* u, int32_t passes_done, double rel_err) {
  CAMLparam0();
  CAMLlocal2(boxed_rel_err, r);
  boxed_rel_err = caml_copy_double(rel_err);
  r = caml_callback3_exn(*u->cb.closure, Val_long(passes_done), boxed_rel_err, Val_int(passes_done >= u->samples_per_pixel));
  if (Is_exception_result(r)) {
    *u->cb.exn = Extract_exception(r);
    u->cb.raised = 1;
  } else {
    u->stop = Int_val(r) != 0;
  }
  CAMLreturn0;
}

static int32_t ptx_ml_on_update(void* user, int32_t passes_done, double rel_err, const double* rgb, const double* err) {
  ptx_ml_update_cb* u = (ptx_ml_update_cb*)user;
  (void)rgb;
  (void)err;
  if (u->cb.raised) return 1;
  caml_acquire_runtime_system(); /* the render runs with the lock released */
  ptx_ml_call_on_update(u, passes_done, rel_err);
  caml_release_runtime_system();
  return (u->cb.raised || u->stop) ? 1 : 0; /* a raise stops the render: no callbacks after it */
}

/* external render_progressive_flat : scene -> floatarray -> image -> err -> (int -> float -> bool -> bool) -> int
 *   = "ptx_ml_render_progressive_stub"
 * (scene, [width; height; samples_per_pixel; max_bounces; passes_per_update; target_rel_err], image (W*H*3), err (W*H*3 or
 * empty), on_update passes_done rel_err last -> stop) -> passes done.  The exception of a callback that raised is raised here,
 * after the library has returned (and has drained everything it queued). */
CAMLprim value ptx_ml_render_progressive_stub(value handle, value params, value image, value err, value on_update) {
  CAMLparam5(handle, params, image, err, on_update);
  CAMLlocal1(exn);
  if (floatarray_length(params) != 6) caml_invalid_argument("Ptx.render_progressive: params needs 6 floats");
  double p6[6];
  memcpy(p6, floatarray_data(params), sizeof p6);
  const intnat w = (intnat)p6[0], h = (intnat)p6[1];
  if (w <= 0 || h <= 0 || Caml_ba_array_val(image)->dim[0] != w * h * 3)
    caml_invalid_argument("Ptx.render_progressive: image must hold width * height * 3 floats");
  const intnat n_err = Caml_ba_array_val(err)->dim[0];
  if (n_err != 0 && n_err != w * h * 3) caml_invalid_argument("Ptx.render_progressive: err must be empty or hold width * height * 3 floats");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_progressive: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_progressive: scene already destroyed");
  double* out = (double*)Caml_ba_data_val(image); /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  double* err_out = n_err ? (double*)Caml_ba_data_val(err) : NULL;
  exn = Val_unit;
  ptx_ml_update_cb cb = {{&on_update, &exn, 0}, (int32_t)p6[2], 0};
  int32_t passes_done = 0;
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_progressive(s, p6, out, err_out, &passes_done, ptx_ml_on_update, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.cb.raised) caml_raise(exn);
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_long(passes_done));
}

/* the round callback: the library has already filled the caller's Bigarrays (image, err, passes) when it calls */
typedef struct ptx_ml_round_cb {
  ptx_ml_cb cb;
  int stop; /* what the closure returned */
} ptx_ml_round_cb;

/* runs with the runtime lock held: on_round round passes_done (active_next, samples, rel_err) */
static void ptx_ml_call_on_round(ptx_ml_round_cb* u, int32_t round, int32_t passes_done, int64_t active_next, int64_t samples,
                                 double rel_err) {
  CAMLparam0();
  CAMLlocal3(boxed_rel_err, info, r);
  boxed_rel_err = caml_copy_double(rel_err);
  info = caml_alloc_tuple(3);
  Store_field(info, 0, Val_long(active_next));
  Store_field(info, 1, Val_long(samples));
  Store_field(info, 2, boxed_rel_err);
  r = caml_callback3_exn(*u->cb.closure, Val_long(round), Val_long(passes_done), info);
  if (Is_exception_result(r)) {
    *u->cb.exn = Extract_exception(r);
    u->cb.raised = 1;
  } else {
    u->stop = Int_val(r) != 0;
  }
  CAMLreturn0;
}

static int32_t ptx_ml_on_round(void* user, int32_t round, int32_t passes_done, int64_t active_next, int64_t samples, double rel_err,
                               const double* rgb, const double* err, const int32_t* passes) {
  ptx_ml_round_cb* u = (ptx_ml_round_cb*)user;
  (void)rgb;
  (void)err;
  (void)passes;
  if (u->cb.raised) return 1;
  caml_acquire_runtime_system(); /* the render runs with the lock released */
  ptx_ml_call_on_round(u, round, passes_done, active_next, samples, rel_err);
  caml_release_runtime_system();
  return (u->cb.raised || u->stop) ? 1 : 0; /* a raise stops the render: no callbacks after it */
}

/* external render_adaptive_flat : scene -> floatarray -> image -> err -> passes -> (int -> int -> int * int * float -> bool) -> int
 *   = "ptx_ml_render_adaptive_stub"
 * (scene, [width; height; samples_per_pixel; max_bounces; min_passes; passes_per_round; target_rel_err; radiance_floor], image
 * (W*H*3), err (W*H*3 or empty), passes (int32, W*H or empty), on_round round passes_done (active_next, samples, rel_err) -> stop)
 * -> samples (the sum of the count map).  The exception of a callback that raised is raised here, after the library has returned
 * (and has drained everything it queued). */
CAMLprim value ptx_ml_render_adaptive_stub(value handle, value params, value image, value err, value passes, value on_round) {
  CAMLparam5(handle, params, image, err, passes);
  CAMLxparam1(on_round);
  CAMLlocal1(exn);
  if (floatarray_length(params) != 8) caml_invalid_argument("Ptx.render_adaptive: params needs 8 floats");
  double p8[8];
  memcpy(p8, floatarray_data(params), sizeof p8);
  const intnat w = (intnat)p8[0], h = (intnat)p8[1];
  if (w <= 0 || h <= 0 || Caml_ba_array_val(image)->dim[0] != w * h * 3)
    caml_invalid_argument("Ptx.render_adaptive: image must hold width * height * 3 floats");
  const intnat n_err = Caml_ba_array_val(err)->dim[0];
  if (n_err != 0 && n_err != w * h * 3) caml_invalid_argument("Ptx.render_adaptive: err must be empty or hold width * height * 3 floats");
  const intnat n_passes = Caml_ba_array_val(passes)->dim[0];
  if (n_passes != 0 && n_passes != w * h) caml_invalid_argument("Ptx.render_adaptive: passes must be empty or hold width * height int32s");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_adaptive: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_adaptive: scene already destroyed");
  double* out = (double*)Caml_ba_data_val(image); /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  double* err_out = n_err ? (double*)Caml_ba_data_val(err) : NULL;
  int32_t* passes_out = n_passes ? (int32_t*)Caml_ba_data_val(passes) : NULL;
  exn = Val_unit;
  ptx_ml_round_cb cb = {{&on_round, &exn, 0}, 0};
  int64_t samples = 0;
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_adaptive(s, p8, out, err_out, passes_out, &samples, ptx_ml_on_round, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.cb.raised) caml_raise(exn);
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_long(samples));
}

/* bytecode entry of the 6-argument external */
CAMLprim value ptx_ml_render_adaptive_stub_bytecode(value* argv, int argn) {
  (void)argn;
  return ptx_ml_render_adaptive_stub(argv[0], argv[1], argv[2], argv[3], argv[4], argv[5]);
}

/* external render_denoised_flat : scene -> floatarray -> image -> err -> feat -> (int -> float -> bool -> bool) -> int
 *   = "ptx_ml_render_denoised_stub"
 * (scene, the 13 floats of ptx_ml_render_denoised, image (W*H*3), err (W*H*3 or empty), feat (W*H*8 or empty), on_update passes_done
 * rel_err last -> stop) -> passes done.  The exception of a callback that raised is raised here, after the library has returned
 * (and has drained everything it queued). */
CAMLprim value ptx_ml_render_denoised_stub(value handle, value params, value image, value err, value feat, value on_update) {
  CAMLparam5(handle, params, image, err, feat);
  CAMLxparam1(on_update);
  CAMLlocal1(exn);
  if (floatarray_length(params) != 13) caml_invalid_argument("Ptx.render_denoised: params needs 13 floats");
  double p13[13];
  memcpy(p13, floatarray_data(params), sizeof p13);
  const intnat w = (intnat)p13[0], h = (intnat)p13[1];
  if (w <= 0 || h <= 0 || Caml_ba_array_val(image)->dim[0] != w * h * 3)
    caml_invalid_argument("Ptx.render_denoised: image must hold width * height * 3 floats");
  const intnat n_err = Caml_ba_array_val(err)->dim[0];
  if (n_err != 0 && n_err != w * h * 3) caml_invalid_argument("Ptx.render_denoised: err must be empty or hold width * height * 3 floats");
  const intnat n_feat = Caml_ba_array_val(feat)->dim[0];
  if (n_feat != 0 && n_feat != w * h * PTX_FEATURE_DOUBLES)
    caml_invalid_argument("Ptx.render_denoised: feat must be empty or hold width * height * 8 floats");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_denoised: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_denoised: scene already destroyed");
  double* out = (double*)Caml_ba_data_val(image); /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  double* err_out = n_err ? (double*)Caml_ba_data_val(err) : NULL;
  double* feat_out = n_feat ? (double*)Caml_ba_data_val(feat) : NULL;
  exn = Val_unit;
  ptx_ml_update_cb cb = {{&on_update, &exn, 0}, (int32_t)p13[2], 0};
  int32_t passes_done = 0;
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_denoised(s, p13, out, err_out, feat_out, &passes_done, ptx_ml_on_update, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.cb.raised) caml_raise(exn);
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_long(passes_done));
}

/* bytecode entry of the 6-argument external */
CAMLprim value ptx_ml_render_denoised_stub_bytecode(value* argv, int argn) {
  (void)argn;
  return ptx_ml_render_denoised_stub(argv[0], argv[1], argv[2], argv[3], argv[4], argv[5]);
}

/* external render_temporal_flat : scene -> floatarray -> image -> err -> motion -> int = "ptx_ml_render_temporal_stub"
 * (scene, the 18 floats of ptx_ml_render_temporal, image (W*H*3), err (W*H*3 or empty), motion (W*H*3 or empty)) -> the pixels that
 * took history.  One frame of a sequence: no callback runs, so nothing can raise while the lock is released. */
CAMLprim value ptx_ml_render_temporal_stub(value handle, value params, value image, value err, value motion) {
  CAMLparam5(handle, params, image, err, motion);
  if (floatarray_length(params) != 18) caml_invalid_argument("Ptx.render_temporal: params needs 18 floats");
  double p18[18];
  memcpy(p18, floatarray_data(params), sizeof p18);
  const intnat w = (intnat)p18[0], h = (intnat)p18[1];
  if (w <= 0 || h <= 0 || Caml_ba_array_val(image)->dim[0] != w * h * 3)
    caml_invalid_argument("Ptx.render_temporal: image must hold width * height * 3 floats");
  const intnat n_err = Caml_ba_array_val(err)->dim[0];
  if (n_err != 0 && n_err != w * h * 3) caml_invalid_argument("Ptx.render_temporal: err must be empty or hold width * height * 3 floats");
  const intnat n_motion = Caml_ba_array_val(motion)->dim[0];
  if (n_motion != 0 && n_motion != w * h * 3) caml_invalid_argument("Ptx.render_temporal: motion must be empty or hold width * height * 3 floats");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_temporal: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_temporal: scene already destroyed");
  double* out = (double*)Caml_ba_data_val(image); /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  double* err_out = n_err ? (double*)Caml_ba_data_val(err) : NULL;
  double* motion_out = n_motion ? (double*)Caml_ba_data_val(motion) : NULL;
  int64_t history_pixels = 0;
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_temporal(s, p18, out, err_out, motion_out, &history_pixels);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_long((intnat)history_pixels));
}

/* external temporal_reset : scene -> unit = "ptx_ml_temporal_reset_stub" (ptx_temporal_reset).  Like set_camera_pose it takes the scene
 * exclusively: Failure while a render runs on another thread or domain. */
CAMLprim value ptx_ml_temporal_reset_stub(value handle) {
  CAMLparam1(handle);
  if (!Scene_val(handle)) caml_invalid_argument("Ptx.temporal_reset: scene already destroyed");
  if (!ptx_ml_scene_acquire_exclusive(handle)) caml_failwith("Ptx.temporal_reset: a render is running on this scene");
  ptx_scene* s = __atomic_load_n(&Handle_val(handle)->scene, __ATOMIC_ACQUIRE);
  int32_t rc = 0;
  if (s) rc = ptx_ml_temporal_reset(s);
  ptx_ml_scene_release_exclusive(handle);
  if (!s) caml_invalid_argument("Ptx.temporal_reset: scene already destroyed");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* ---- display outputs (include/ptx.h, "display outputs") ---- */

/* external display_defaults_flat : unit -> int * int * int * float = "ptx_ml_display_defaults_stub" (ptx_display_defaults, host only):
 * format, transfer, tone as the PTX_* values, exposure */
CAMLprim value ptx_ml_display_defaults_stub(value unit) {
  CAMLparam1(unit);
  CAMLlocal2(tuple, boxed);
  double d4[4];
  if (ptx_ml_display_defaults(d4) != 0) caml_failwith(ptx_last_error());
  boxed = caml_copy_double(d4[3]);
  tuple = caml_alloc_tuple(4);
  Store_field(tuple, 0, Val_long((intnat)d4[0]));
  Store_field(tuple, 1, Val_long((intnat)d4[1]));
  Store_field(tuple, 2, Val_long((intnat)d4[2]));
  Store_field(tuple, 3, boxed);
  CAMLreturn(tuple);
}

/* external render_display_u8 / render_display_f32 : scene -> floatarray -> pixels -> (int -> unit) -> unit = "ptx_ml_render_display_stub"
 * (scene, [width; height; samples_per_pixel; max_bounces; gpus; format; transfer; tone; exposure], the display image as an
 * int8_unsigned or float32 Bigarray of W*H*channels -- the OCaml side picks the external whose element type fits the format --
 * update_progress) */
CAMLprim value ptx_ml_render_display_stub(value handle, value params, value pixels, value update_progress) {
  CAMLparam4(handle, params, pixels, update_progress);
  CAMLlocal1(exn);
  if (floatarray_length(params) != 9) caml_invalid_argument("Ptx.render_display: params needs 9 floats");
  double p9[9];
  memcpy(p9, floatarray_data(params), sizeof p9);
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_display: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_display: scene already destroyed");
  void* out = Caml_ba_data_val(pixels); /* Bigarray data lives outside the OCaml heap: stable while the lock is released */
  const int64_t n = (int64_t)Caml_ba_array_val(pixels)->dim[0];
  exn = Val_unit;
  ptx_ml_cb cb = {&update_progress, &exn, 0};
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_display(s, p9, out, n, ptx_ml_progress, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.raised) caml_raise(exn);
  if (rc == -4) caml_invalid_argument("Ptx.render_display: pixels must hold width * height * channels elements");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_unit);
}

/* ptx_ml_on_update for updates that arrive as display pixels: the library has already filled the caller's Bigarrays when it calls */
static int32_t ptx_ml_on_update_display(void* user, int32_t passes_done, double rel_err, const void* pixels, const double* err) {
  ptx_ml_update_cb* u = (ptx_ml_update_cb*)user;
  (void)pixels;
  (void)err;
  if (u->cb.raised) return 1;
  caml_acquire_runtime_system(); /* the render runs with the lock released */
  ptx_ml_call_on_update(u, passes_done, rel_err);
  caml_release_runtime_system();
  return (u->cb.raised || u->stop) ? 1 : 0; /* a raise stops the render: no callbacks after it */
}

/* external render_progressive_display_u8 / _f32 : scene -> floatarray -> pixels -> err -> (int -> float -> bool -> bool) -> int
 *   = "ptx_ml_render_progressive_display_stub"
 * (scene, the 18 floats of ptx_ml_render_progressive_display, the display image, err (W*H*3 float64 or empty),
 * on_update passes_done rel_err last -> stop) -> passes done */
CAMLprim value ptx_ml_render_progressive_display_stub(value handle, value params, value pixels, value err, value on_update) {
  CAMLparam5(handle, params, pixels, err, on_update);
  CAMLlocal1(exn);
  if (floatarray_length(params) != 18) caml_invalid_argument("Ptx.render_progressive_display: params needs 18 floats");
  double p18[18];
  memcpy(p18, floatarray_data(params), sizeof p18);
  const intnat w = (intnat)p18[0], h = (intnat)p18[1];
  const intnat n_err = Caml_ba_array_val(err)->dim[0];
  if (n_err != 0 && (w <= 0 || h <= 0 || n_err != w * h * 3))
    caml_invalid_argument("Ptx.render_progressive_display: err must be empty or hold width * height * 3 floats");
  int busy = 0;
  ptx_scene* s = ptx_ml_scene_acquire(handle, &busy);
  if (!s && busy) caml_failwith("Ptx.render_progressive_display: the scene's image is being pinned or unpinned on another thread");
  if (!s) caml_invalid_argument("Ptx.render_progressive_display: scene already destroyed");
  void* out = Caml_ba_data_val(pixels);
  const int64_t n = (int64_t)Caml_ba_array_val(pixels)->dim[0];
  double* err_out = n_err ? (double*)Caml_ba_data_val(err) : NULL;
  exn = Val_unit;
  ptx_ml_update_cb cb = {{&on_update, &exn, 0}, (int32_t)p18[2], 0};
  int32_t passes_done = 0;
  caml_release_runtime_system();
  const int32_t rc = ptx_ml_render_progressive_display(s, p18, out, n, err_out, &passes_done, ptx_ml_on_update_display, &cb);
  caml_acquire_runtime_system();
  ptx_ml_scene_release(handle);
  if (cb.cb.raised) caml_raise(exn);
  if (rc == -4) caml_invalid_argument("Ptx.render_progressive_display: pixels must hold width * height * channels elements");
  if (rc != 0) caml_failwith(ptx_last_error());
  CAMLreturn(Val_long(passes_done));
}
