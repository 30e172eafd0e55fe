(* ptx.ml -- OCaml side of the binding to libptx_hip.so (include/ptx.h): the MI355X integrators behind
   Integrator.create / Integrator.render (shirley_spheres) and Progressive_photon_map.Make(Scene).go (cornell-box, ganesha).

   The reference hands its integrators closures (camera, intersect, background: render_command.mli:18-22;
   progressive_photon_map.mli:35-41); a GPU cannot call closures, so this module takes the same scene DECLARATIVELY:
   the spheres / triangle mesh / pre-tested floor triangles main.ml has just built (already in camera space), what their
   materials and textures are, the four numbers Camera.ray reads, the background gradient, and -- for the photon mapper --
   the lights.  [render] then fills the Bimage exactly as Integrator.render would; [ppm_render] accumulates img_sum
   exactly as Progressive_photon_map's [go] does and calls back after every iteration so the caller can save the image. *)
open! Base

module Texture = struct
  type rgb = float * float * float

  type t =
    | Solid of rgb (* Texture.solid *)
    | Checker of
        { width : int
        ; height : int
        ; even : rgb
        ; odd : rgb
        } (* Texture.checker ~width ~height (solid even) (solid odd) *)
end

module Material = struct
  type t =
    | Lambertian of Texture.t
    | Metal of Texture.t
    | Dielectric of float (* index; Material.glass = Dielectric 1.5 *)
    | Emitting of t * Texture.rgb
        (* the Hit.emit slot (hit.ml:5): the reference's Material.emit is constant black (material.ml:59); non-black values
           are the documented extension that lights cornell-box under the path integrator *)
end

type sphere =
  { x : float
  ; y : float
  ; z : float (* centre in CAMERA space: Sphere.transform s ~f:(Camera.transform camera) *)
  ; radius : float
  ; material : Material.t
  }

type uv = float * float (* Texture.Coord.t *)

(* Triangle.Make(Face).t over shared vertices (ganesha's Mesh.t + Face.t, ganesha/bin/main.ml:37-119) or with private
   vertices (cornell-box's Face.t, cornell-box/bin/main.ml:5-28: three fresh vertices per face) *)
type mesh =
  { vx : floatarray
  ; vy : floatarray
  ; vz : floatarray (* vertices in CAMERA space *)
  ; faces : (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t (* 3 vertex indices per triangle: a, b, c *)
  ; face_uv : uv * uv * uv (* Face.tex_coords of face i = face_uvs.(i) if given, else this *)
  ; face_uvs : (uv * uv * uv) array (* empty = every face uses [face_uv] *)
  ; face_material : Material.t (* Face.material of face i = face_materials.(i) if given, else this *)
  ; face_materials : Material.t array (* empty = every face uses [face_material] *)
  }

let empty_mesh =
  { vx = Stdlib.Float.Array.create 0
  ; vy = Stdlib.Float.Array.create 0
  ; vz = Stdlib.Float.Array.create 0
  ; faces = Bigarray.Array1.create Bigarray.int32 Bigarray.c_layout 0
  ; face_uv = (0., 0.), (0., 0.), (0., 0.)
  ; face_uvs = [||]
  ; face_material = Material.Dielectric 1.5
  ; face_materials = [||]
  }
;;

type p3 = float * float * float

(* a triangle tested BEFORE the tree, its hit clipping t_max for the tree (ganesha's Floor, ganesha/bin/main.ml:205-298) *)
type floor_triangle =
  { vertices : p3 * p3 * p3
  ; uvs : uv * uv * uv
  ; surface : Material.t
  }

type camera =
  { lower_left_x : float
  ; lower_left_y : float
  ; view_x : float
  ; view_y : float
  }

type background =
  | Black
  | Sky of
      { horizon : Texture.rgb
      ; zenith : Texture.rgb
      } (* lerp t horizon zenith, t = .5 * (normalize(dir).y + 1): shirley_spheres/bin/main.ml:104-110 *)

type leaf =
  | Simd_leaf (* <= leaf_size () spheres per packet, the Rust x86 arithmetic *)
  | Array_leaf of int (* Shape_tree.Array_leaf, length_cutoff: 4 (--no-simd), 2 (cornell-box), 8 (ganesha) *)

(* Progressive_photon_map.Light.create_point / create_spot (progressive_photon_map.ml:59-137), positions in camera space *)
type light =
  | Point of
      { position : p3
      ; color : Texture.rgb
      ; power : float
      }
  | Spot of
      { position : p3
      ; direction : p3 (* not normalised by the caller, like create_spot's ~direction *)
      ; color : Texture.rgb
      ; power : float
      }

(* what crosses the FFI: flat unboxed arrays, like Simd_leaf.coords (main.ml:137-142).  The stub indexes this record
   with Field (flat, i): keep the field order in step with ptx_stubs.c *)
type flat =
  { xs : floatarray
  ; ys : floatarray
  ; zs : floatarray
  ; rs : floatarray
  ; sphere_material : (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t
  ; materials : floatarray (* 6 per material: kind, texture, index, emit r g b *)
  ; textures : floatarray (* 9 per texture: kind, width, height, even r g b, odd r g b *)
  ; camera : floatarray (* lower_left_x, lower_left_y, view_x, view_y *)
  ; background : floatarray (* kind, horizon r g b, zenith r g b *)
  ; leaf_kind : int
  ; length_cutoff : int
  ; vertex_x : floatarray
  ; vertex_y : floatarray
  ; vertex_z : floatarray
  ; tri_indices : (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t (* 3 per triangle *)
  ; tri_uv : floatarray (* 6 per triangle: ua va ub vb uc vc *)
  ; tri_material : (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t
  ; floor_vertices : floatarray (* 9 per floor triangle *)
  ; floor_uv : floatarray (* 6 per floor triangle *)
  ; floor_material : (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t
  }

type scene (* custom block around the ptx_scene* handle; finalised by the GC *)

external leaf_size : unit -> int = "ptx_ml_leaf_size"
external device_count : unit -> int = "ptx_ml_device_count"
external scene_create_flat : flat -> int -> scene = "ptx_ml_scene_create_stub"
external scene_destroy : scene -> unit = "ptx_ml_scene_destroy_stub"

(* tree depth, nodes, leaves, leaf slots: what main.ml prints after Shape_tree.create (ganesha/bin/main.ml:191-195) *)
external scene_tree_stats : scene -> int * int * int * int = "ptx_ml_scene_tree_stats_stub"

(* Optional: page-lock the image the renders go into (ptx_image_pin): the frame then comes back with one DMA.  A Bigarray's data
   is outside the OCaml heap and does not move; the pin must end (image_unpin, scene_destroy) before the image is collected --
   with_pinned_image below keeps the image reachable for exactly that long. *)
external image_pin : scene -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t -> unit = "ptx_ml_image_pin_stub"
external image_unpin : scene -> unit = "ptx_ml_image_unpin_stub"

(* What Integrator.create's ~diffuse_plus_light slot becomes (ptx_scene_set_lighting): Reference = Pdf.diffuse and the reference's
   emission formula emit0' = a * emit0 + emit (order-reversed once something emits); Path_order = Pdf.diffuse with every hit's emission
   weighted by what came before it; Sampled = Path_order with diffuse_plus_light = 1/2 cosine + 1/2 the scene's emissive triangles.
   Sticky: every later render of the scene reads it.  Failure when Sampled finds no emissive triangle (or more than 64), or while a
   render runs on the scene. *)
type lighting = Reference | Path_order | Sampled

external set_lighting_int : scene -> int -> unit = "ptx_ml_set_lighting_stub"

let set_lighting scene lighting =
  set_lighting_int scene (match lighting with Reference -> 0 | Path_order -> 1 | Sampled -> 2)

(* The reconstruction filter the reference hard-wires in Integrator.render (Filter_kernel.Binomial.create ~order:5 ~pixel_radius:1),
   at any accepted order and radius (ptx_scene_set_film): 1 <= order <= 16, 0 <= pixel_radius <= 7, order >= 2 * pixel_radius + 1 --
   below that the reference's kernel comes out lopsided, and the library refuses it.  ~renormalise divides a border pixel by the weight
   that stayed inside the image (the reference lets the border darken).  Sticky: every later render of the scene reads it.  Failure
   for a refused pair, or while a render runs on the scene. *)
external set_film_int : scene -> int -> int -> int -> unit = "ptx_ml_set_film_stub"
external film_int : scene -> int * int * int = "ptx_ml_film_stub"

external film_weights_into
  :  int
  -> int
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> unit
  = "ptx_ml_film_weights_stub"

let set_film ?(renormalise = false) scene ~order ~pixel_radius =
  set_film_int scene order pixel_radius (if renormalise then 1 else 0)

(* order, pixel_radius, renormalise *)
let film scene =
  let order, pixel_radius, flags = film_int scene in
  order, pixel_radius, flags land 1 <> 0

(* Binomial.create's normalised 1-D weights, 2 * pixel_radius + 1 of them; the 2-D weight is w.(j) *. w.(i) *)
let film_weights ~order ~pixel_radius =
  let n = (2 * max 0 (min pixel_radius 7)) + 1 in
  let out = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout n in
  film_weights_into order pixel_radius out;
  Array.init n (fun i -> Bigarray.Array1.get out i)

(* Image textures and a latitude-longitude environment (ptx_scene_set_texture_image / ptx_scene_set_environment; the rule is in
   include/ptx.h).  [texels] holds width * height * 3 linear binary64 values, texel (ix, iy) at 3 * (iy * width + ix), row 0 = v 0; the
   library copies them.  set_texture_image: from then on every material that points at entry [index] of the scene's texture table (the
   order in which [flatten] interned the textures) evaluates the image; ~bilinear interpolates the four nearest texels, ~repeat_u /
   ~repeat_v wrap around instead of clamping.  set_environment: a ray that leaves the scene returns the image's colour in its
   direction; [rotation] is the row-major 3 x 3 matrix from camera space to the environment's space (default: identity).  Sticky:
   every later render of the scene reads them.  Failure for a refused image, or while a render runs on the scene. *)
type texels = (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t

external set_texture_image_raw : scene -> int -> int * int * int -> texels -> unit = "ptx_ml_set_texture_image_stub"
external set_environment_raw : scene -> int * int * int -> texels -> texels -> unit = "ptx_ml_set_environment_stub"

let no_texels () = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 0

let set_texture_image ?(bilinear = false) ?(repeat_u = false) ?(repeat_v = false) scene ~index ~width ~height texels =
  let flags = (if bilinear then 1 else 0) lor (if repeat_u then 2 else 0) lor if repeat_v then 4 else 0 in
  if width < 1 || height < 1 then invalid_arg "Ptx.set_texture_image: width and height must be >= 1";
  set_texture_image_raw scene index (width, height, flags) texels

let clear_texture_image scene ~index = set_texture_image_raw scene index (0, 0, 0) (no_texels ())

let set_environment ?(bilinear = true) ?rotation scene ~width ~height texels =
  if width < 1 || height < 1 then invalid_arg "Ptx.set_environment: width and height must be >= 1";
  let rot =
    match rotation with
    | None -> no_texels ()
    | Some m ->
      if Array.length m <> 9 then invalid_arg "Ptx.set_environment: rotation must hold 9 floats (row-major 3 x 3)";
      Bigarray.Array1.of_array Bigarray.float64 Bigarray.c_layout m
  in
  set_environment_raw scene (width, height, if bilinear then 1 else 0) texels rot

let clear_environment scene = set_environment_raw scene (0, 0, 0) (no_texels ()) (no_texels ())

(* Importance-sampling the environment (ptx_scene_set_environment_sampling; the rule is in include/ptx.h): with [Sampled] lighting a
   Diffuse scatter also draws directions from the environment image, in proportion to luminance x sin theta per texel, and [Sampled]
   then accepts a scene without emissive triangles.  Needs an environment whose rotation is orthonormal and whose total weight is
   positive.  Sticky.  Failure when a condition fails, when turning it off would leave [Sampled] nothing to sample, or while a render
   runs on the scene.  environment_sampling: (on, the density's total weight). *)
external set_environment_sampling_int : scene -> int -> unit = "ptx_ml_set_environment_sampling_stub"
external environment_sampling_raw : scene -> int * float = "ptx_ml_environment_sampling_stub"

let set_environment_sampling scene on = set_environment_sampling_int scene (if on then 1 else 0)

let environment_sampling scene =
  let on, total = environment_sampling_raw scene in
  on <> 0, total

(* Cone-sampling emissive spheres (ptx_scene_set_sphere_light_sampling; the rule is in include/ptx.h): with [Sampled] lighting the
   light half also draws directions towards the scene's emissive spheres, uniformly over the cone each spans from the hit, and
   [Sampled] then accepts a scene without emissive triangles.  Needs 1 .. 64 emissive spheres.  Sticky.  Failure when the count is
   outside that, when turning it off would leave [Sampled] nothing to sample, or while a render runs on the scene.
   sphere_lights: (on, the number of sphere lights, the joined light table's total weight). *)
external set_sphere_light_sampling_int : scene -> int -> unit = "ptx_ml_set_sphere_light_sampling_stub"
external sphere_lights_raw : scene -> int * int * float = "ptx_ml_sphere_lights_stub"

let set_sphere_light_sampling scene on = set_sphere_light_sampling_int scene (if on then 1 else 0)

let sphere_lights scene =
  let on, n, total = sphere_lights_raw scene in
  on <> 0, n, total

(* The thin-lens camera (ptx_scene_set_lens; the rule is in include/ptx.h): a lens of [radius] around the camera's origin, focused on
   the plane [focus_distance] in front of it, so that what lies off that plane blurs.  [radius] 0. switches the lens off, which is a
   scene's first state: the pinhole Camera.ray, bit for bit.  Sticky: every later render of the scene reads it.  Failure for a negative
   or non-finite radius, a focus distance that is not positive and finite, or while a render runs on the scene.
   lens: (radius, focus_distance). *)
external set_lens_raw
  :  scene
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> unit
  = "ptx_ml_set_lens_stub"

external lens : scene -> float * float = "ptx_ml_lens_stub"

let set_lens scene ~radius ~focus_distance =
  set_lens_raw scene (Bigarray.Array1.of_array Bigarray.float64 Bigarray.c_layout [| radius; focus_distance |])

(* The camera pose (ptx_scene_set_camera_pose; the rule is in include/ptx.h): the camera stands at [origin] of the scene's space,
   turned by [rotation] (9 floats, row-major, posed camera space -> scene space) and, with [view] = (lower_left_x, lower_left_y,
   view_x, view_y), looks through a frustum of its own: a viewport or a turntable moves the camera of one handle instead of building
   the scene again.  Sticky: every later render of the scene reads it.  [pose] and [view] are each optional, but one must be given;
   [view] alone keeps origin 0 and the identity.  Any pose, the identity included, switches the posed route on;
   [clear_camera_pose] switches it off, which is a scene's first state: its own camera and its own launches, bit for bit.  Failure
   for a non-finite origin, a matrix that is not a rotation (max |R R^T - I| > 1e-9 or det R <= 0), a non-finite view, or while a
   render runs on the scene.  [camera_pose]: None while off, else (origin, rotation, view in effect). *)
external set_camera_pose_raw
  :  scene
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> unit
  = "ptx_ml_set_camera_pose_stub"

external clear_camera_pose : scene -> unit = "ptx_ml_clear_camera_pose_stub"

external camera_pose_raw
  :  scene
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> int
  = "ptx_ml_camera_pose_stub"

let set_camera_pose ?pose ?view scene =
  let doubles a = Bigarray.Array1.of_array Bigarray.float64 Bigarray.c_layout a in
  let pose =
    match pose with
    | None -> [||]
    | Some (origin, rotation) ->
      if Array.length origin <> 3 || Array.length rotation <> 9
      then invalid_arg "Ptx.set_camera_pose: origin holds 3 floats and rotation 9";
      Array.append origin rotation
  in
  let view =
    match view with
    | None -> [||]
    | Some (llx, lly, vx, vy) -> [| llx; lly; vx; vy |]
  in
  set_camera_pose_raw scene (doubles pose) (doubles view)

let camera_pose scene =
  let out = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 16 in
  if camera_pose_raw scene out = 0
  then None
  else (
    let get i = Bigarray.Array1.get out i in
    Some (Array.init 3 get, Array.init 9 (fun i -> get (3 + i)), (get 12, get 13, get 14, get 15)))

(* The camera shutter (ptx_scene_set_camera_shutter; the rule is in include/ptx.h): while a frame is exposed the camera moves from the
   pose's origin by [translation] (3 floats, scene space) and turns by [angle] radians about the unit vector [axis] (3 floats, scene
   space), at constant velocity, so every later render of the scene is blurred by that motion.  Sticky.  Any shutter, a zero motion
   included, switches the shutter's route on; [clear_camera_shutter] switches it off, which is a scene's first state: its own launches,
   bit for bit.  Failure for a non-finite value, |angle| > pi, an axis that is not a unit vector while angle <> 0, or while a render runs
   on the scene.  [camera_shutter]: None while off, else (translation, axis, angle). *)
external set_camera_shutter_raw
  :  scene
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> unit
  = "ptx_ml_set_camera_shutter_stub"

external clear_camera_shutter : scene -> unit = "ptx_ml_clear_camera_shutter_stub"

external camera_shutter_raw
  :  scene
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> int
  = "ptx_ml_camera_shutter_stub"

let set_camera_shutter scene ~translation ~axis ~angle =
  if Array.length translation <> 3 || Array.length axis <> 3
  then invalid_arg "Ptx.set_camera_shutter: translation and axis hold 3 floats each";
  set_camera_shutter_raw
    scene
    (Bigarray.Array1.of_array Bigarray.float64 Bigarray.c_layout (Array.concat [ translation; axis; [| angle |] ]))

let camera_shutter scene =
  let out = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 7 in
  if camera_shutter_raw scene out = 0
  then None
  else (
    let get i = Bigarray.Array1.get out i in
    Some (Array.init 3 get, Array.init 3 (fun i -> get (3 + i)), get 6))

(* The camera projection (ptx_scene_set_camera_projection; the rule is in include/ptx.h): [Perspective] is the pinhole, a scene's first
   state; [Latlong] is a 360-degree panorama in the environment map's (u, v) convention, taken from the pose's origin (the scene's own
   while the pose is off): written as a PFM it lights another scene.  Sticky.  Failure for [Latlong] while a lens is on, or while a
   render runs on the scene. *)
type projection =
  | Perspective
  | Latlong

external set_camera_projection_int : scene -> int -> unit = "ptx_ml_set_camera_projection_stub"
external camera_projection_int : scene -> int = "ptx_ml_camera_projection_stub"

let set_camera_projection scene projection =
  set_camera_projection_int
    scene
    (match projection with
     | Perspective -> 0
     | Latlong -> 1)

let camera_projection scene = if camera_projection_int scene = 1 then Latlong else Perspective

(* Radiance along rays the caller owns (ptx_render_rays; the rule is in include/ptx.h): [origins] and [directions] hold 3 floats a ray
   (unit directions, or any length with [normalize]), [offsets] the sampler offset of every ray (default: its index).  Returns
   (sums, squares): 3 floats per bin of [rays_per_bin] consecutive rays, folded in ray order from zero; [squares] is empty without
   [want_sq].  One ray per bin is the per-ray radiance.  Failure for a ray that is not finite, a zero direction or an offset outside
   [0, 2^31 - 2] (the message names the lowest bad index), and for a host-only scene. *)
external render_rays_flat
  :  scene
  -> floatarray (* max_bounces, rays_per_bin, normalize *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* origins, 3 n *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* directions, 3 n *)
  -> (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t (* offsets, n, or empty *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* sums, 3 n / m *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* squares, 3 n / m, or empty *)
  -> unit
  = "ptx_ml_render_rays_stub_bytecode" "ptx_ml_render_rays_stub"

let render_rays ?offsets ?(max_bounces = 8) ?(rays_per_bin = 1) ?(normalize = false) ?(want_sq = false) scene ~origins ~directions =
  let n3 = Bigarray.Array1.dim origins in
  if rays_per_bin < 1 || n3 mod (3 * rays_per_bin) <> 0
  then invalid_arg "Ptx.render_rays: origins hold 3 floats a ray and the rays a whole number of bins";
  let bins3 = n3 / rays_per_bin in
  let zeros k =
    let a = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout k in
    Bigarray.Array1.fill a 0.;
    a
  in
  let offsets = Option.value offsets ~default:(Bigarray.Array1.create Bigarray.int32 Bigarray.c_layout 0) in
  let sums = zeros bins3 in
  let sq = zeros (if want_sq then bins3 else 0) in
  let params = Stdlib.Float.Array.of_list [ Float.of_int max_bounces; Float.of_int rays_per_bin; (if normalize then 1. else 0.) ] in
  render_rays_flat scene params origins directions offsets sums sq;
  sums, sq

external render_flat
  :  scene
  -> int (* width *)
  -> int (* height *)
  -> int (* samples_per_pixel *)
  -> int (* max_bounces *)
  -> int (* gpus *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (int -> unit)
  -> unit
  = "ptx_ml_render_stub_bytecode" "ptx_ml_render_stub"

external ppm_render_flat
  :  scene
  -> floatarray (* width, height, iterations, max_bounces, photon_count, alpha *)
  -> floatarray (* 11 per light: kind, position xyz, direction xyz, color rgb, power *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* img_sum, W*H*3 *)
  -> (int -> float -> int -> unit) (* iteration, radius, photon map length; img_sum holds the running sum *)
  -> unit
  = "ptx_ml_ppm_render_stub"

external render_progressive_flat
  :  scene
  -> floatarray (* width, height, samples_per_pixel, max_bounces, passes_per_update, target_rel_err *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* image, W*H*3 *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* per-pixel error, W*H*3, or empty *)
  -> (int -> float -> bool -> bool) (* passes done, rel_err, last update; true stops the render *)
  -> int
  = "ptx_ml_render_progressive_stub"

external render_adaptive_flat
  :  scene
  -> floatarray
     (* width, height, samples_per_pixel, max_bounces, min_passes, passes_per_round, target_rel_err, radiance_floor *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* image, W*H*3 *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* per-pixel error, W*H*3, or empty *)
  -> (int32, Bigarray.int32_elt, Bigarray.c_layout) Bigarray.Array1.t (* per-pixel pass count, W*H, or empty *)
  -> (int -> int -> int * int * float -> bool)
     (* round, passes done, (pixels of the next round, samples so far, rel_err); true stops the render *)
  -> int
  = "ptx_ml_render_adaptive_stub_bytecode" "ptx_ml_render_adaptive_stub"

external render_denoised_flat
  :  scene
  -> floatarray
     (* width, height, samples_per_pixel, max_bounces, passes_per_update, target_rel_err, levels, normal_power_log2,
        feature_passes, flags, sigma_luminance, sigma_depth, sigma_albedo *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* image, W*H*3 *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* per-pixel error, W*H*3, or empty *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* first-hit feature means, W*H*8, or empty *)
  -> (int -> float -> bool -> bool) (* passes done, rel_err, last update; true stops the render *)
  -> int
  = "ptx_ml_render_denoised_stub_bytecode" "ptx_ml_render_denoised_stub"

external render_temporal_flat
  :  scene
  -> floatarray
     (* width, height, samples_per_pixel, max_bounces, pass_first, pass_count, max_history_passes, normal_threshold,
        depth_tolerance, min_weight, denoise, levels, normal_power_log2, feature_passes, flags, sigma_luminance, sigma_depth,
        sigma_albedo *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* image, W*H*3 *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* accumulated per-pixel error, W*H*3, or empty *)
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* motion (dx, dy, weight), W*H*3, or empty *)
  -> int
  = "ptx_ml_render_temporal_stub"

(* Drops the frame history the scene keeps (ptx_temporal_reset): call it after a change of lighting, textures or environment, which
   the library does not do for you.  Failure while a render runs on the scene. *)
external temporal_reset : scene -> unit = "ptx_ml_temporal_reset_stub"

module FA = Stdlib.Float.Array

(* the tables are interned structurally: a 150 k-triangle mesh with one material gets one row, not 150 k *)
type tables =
  { tex_rows : float Queue.t
  ; mat_rows : float Queue.t
  ; tex_ids : (Texture.t, int) Hashtbl.Poly.t
  ; mat_ids : (Material.t, int) Hashtbl.Poly.t
  }

let add_texture tb (t : Texture.t) =
  Hashtbl.find_or_add tb.tex_ids t ~default:(fun () ->
    let row =
      match t with
      | Solid (r, g, b) -> [ 0.; 0.; 0.; r; g; b; 0.; 0.; 0. ]
      | Checker { width; height; even = er, eg, eb; odd = or_, og, ob } ->
        [ 1.; Float.of_int width; Float.of_int height; er; eg; eb; or_; og; ob ]
    in
    let idx = Queue.length tb.tex_rows / 9 in
    List.iter row ~f:(Queue.enqueue tb.tex_rows);
    idx)
;;

let add_material tb (m : Material.t) =
  Hashtbl.find_or_add tb.mat_ids m ~default:(fun () ->
    let rec row (m : Material.t) (er, eg, eb) =
      match m with
      | Lambertian t -> [ 0.; Float.of_int (add_texture tb t); 0.; er; eg; eb ]
      | Metal t -> [ 1.; Float.of_int (add_texture tb t); 0.; er; eg; eb ]
      | Dielectric index -> [ 2.; 0.; index; er; eg; eb ]
      | Emitting (inner, emit) -> row inner emit
    in
    let r = row m (0., 0., 0.) in
    let idx = Queue.length tb.mat_rows / 6 in
    List.iter r ~f:(Queue.enqueue tb.mat_rows);
    idx)
;;

let int32_array n ~f =
  let a = Bigarray.Array1.create Bigarray.int32 Bigarray.c_layout n in
  for i = 0 to n - 1 do
    a.{i} <- Int32.of_int_exn (f i)
  done;
  a
;;

let uv6 ((ua, va), (ub, vb), (uc, vc)) = [ ua; va; ub; vb; uc; vc ]

let flatten ~leaf ~(mesh : mesh) ~(floor : floor_triangle list) camera background (spheres : sphere array) =
  let tb =
    { tex_rows = Queue.create ()
    ; mat_rows = Queue.create ()
    ; tex_ids = Hashtbl.Poly.create ()
    ; mat_ids = Hashtbl.Poly.create ()
    }
  in
  let n = Array.length spheres in
  let xs = FA.init n (fun i -> spheres.(i).x)
  and ys = FA.init n (fun i -> spheres.(i).y)
  and zs = FA.init n (fun i -> spheres.(i).z)
  and rs = FA.init n (fun i -> spheres.(i).radius) in
  let sphere_material = int32_array n ~f:(fun i -> add_material tb spheres.(i).material) in
  let n_tri = Bigarray.Array1.dim mesh.faces / 3 in
  if Bigarray.Array1.dim mesh.faces <> 3 * n_tri then invalid_arg "Ptx: mesh.faces holds 3 indices per triangle";
  if (not (Array.is_empty mesh.face_uvs)) && Array.length mesh.face_uvs <> n_tri
  then invalid_arg "Ptx: mesh.face_uvs must be empty or hold one entry per triangle";
  if (not (Array.is_empty mesh.face_materials)) && Array.length mesh.face_materials <> n_tri
  then invalid_arg "Ptx: mesh.face_materials must be empty or hold one entry per triangle";
  let tri_uv =
    let shared = Array.of_list (uv6 mesh.face_uv) in
    if Array.is_empty mesh.face_uvs
    then FA.init (6 * n_tri) (fun k -> shared.(k % 6))
    else (
      let rows = Array.map mesh.face_uvs ~f:(fun t -> Array.of_list (uv6 t)) in
      FA.init (6 * n_tri) (fun k -> rows.(k / 6).(k % 6)))
  in
  let tri_material =
    if Array.is_empty mesh.face_materials
    then (
      let m = if n_tri > 0 then add_material tb mesh.face_material else 0 in
      int32_array n_tri ~f:(fun _ -> m))
    else int32_array n_tri ~f:(fun i -> add_material tb mesh.face_materials.(i))
  in
  let floor = Array.of_list floor in
  let n_floor = Array.length floor in
  let floor_vertices =
    let rows =
      Array.map floor ~f:(fun f ->
        let (ax, ay, az), (bx, by, bz), (cx, cy, cz) = f.vertices in
        [| ax; ay; az; bx; by; bz; cx; cy; cz |])
    in
    FA.init (9 * n_floor) (fun k -> rows.(k / 9).(k % 9))
  in
  let floor_uv =
    let rows = Array.map floor ~f:(fun f -> Array.of_list (uv6 f.uvs)) in
    FA.init (6 * n_floor) (fun k -> rows.(k / 6).(k % 6))
  in
  let floor_material = int32_array n_floor ~f:(fun i -> add_material tb floor.(i).surface) in
  let of_queue q = FA.of_list (Queue.to_list q) in
  let background =
    match background with
    | Black -> FA.of_list [ 0.; 0.; 0.; 0.; 0.; 0.; 0. ]
    | Sky { horizon = hr, hg, hb; zenith = zr, zg, zb } -> FA.of_list [ 1.; hr; hg; hb; zr; zg; zb ]
  in
  let leaf_kind, length_cutoff =
    match leaf with
    | Simd_leaf -> 0, leaf_size ()
    | Array_leaf cutoff -> 1, cutoff
  in
  { xs
  ; ys
  ; zs
  ; rs
  ; sphere_material
  ; materials = of_queue tb.mat_rows
  ; textures = of_queue tb.tex_rows
  ; camera = FA.of_list [ camera.lower_left_x; camera.lower_left_y; camera.view_x; camera.view_y ]
  ; background
  ; leaf_kind
  ; length_cutoff
  ; vertex_x = mesh.vx
  ; vertex_y = mesh.vy
  ; vertex_z = mesh.vz
  ; tri_indices = mesh.faces
  ; tri_uv
  ; tri_material
  ; floor_vertices
  ; floor_uv
  ; floor_material
  }
;;

(* Shape_tree.create + uploading the scene: what main.ml does before Render_cmd.run / Ppm.go.  The tree is built over
   [triangles of the mesh, in order] @ [spheres, in order] -- cornell-box's shape list (cornell-box/bin/main.ml:213-218) *)
let scene_create ?(device = 0) ?(leaf = Simd_leaf) ?(mesh = empty_mesh) ?(floor = []) ~camera ~background spheres =
  scene_create_flat (flatten ~leaf ~mesh ~floor camera background spheres) device
;;

(* Bbox of the mesh = union of its triangles' boxes: what Shape_tree.create computes for the root (shape_tree.ml:257-260)
   and what ganesha's Floor and lights are placed from BEFORE the tree exists here (ganesha/bin/main.ml:203-228,267-275) *)
let mesh_bbox (mesh : mesh) =
  let n = Bigarray.Array1.dim mesh.faces in
  if n = 0 then invalid_arg "Ptx.mesh_bbox: empty mesh";
  let lo = [| Float.infinity; Float.infinity; Float.infinity |]
  and hi = [| Float.neg_infinity; Float.neg_infinity; Float.neg_infinity |] in
  for k = 0 to n - 1 do
    let i = Int32.to_int_exn mesh.faces.{k} in
    let p = [| FA.get mesh.vx i; FA.get mesh.vy i; FA.get mesh.vz i |] in
    for a = 0 to 2 do
      lo.(a) <- Float.min lo.(a) p.(a);
      hi.(a) <- Float.max hi.(a) p.(a)
    done
  done;
  (lo.(0), lo.(1), lo.(2)), (hi.(0), hi.(1), hi.(2))
;;

(* Integrator.create ... |> Integrator.render ~update_progress, on [gpus] GPUs of this node *)
let render ?(gpus = 1) scene ~width ~height ~samples_per_pixel ~max_bounces ~image ~update_progress =
  render_flat scene width height samples_per_pixel max_bounces gpus image update_progress
;;

(* [render] as a sequence of updates: after every [passes_per_update] passes and after the last, [image] holds the frame filmed
   from the passes done so far, [err] (if given) its per-pixel standard error, and [on_update] runs on the calling thread;
   it returns true to stop, and the render also stops at the first update whose [rel_err] is at most [target_rel_err] > 0.
   The result is the number of passes in [image]; run to [samples_per_pixel] passes, [image] is what [render] gives.  An
   exception raised by [on_update] stops the render and is raised again once the library has returned. *)
let render_progressive
  ?(target_rel_err = 0.)
  ?err
  scene
  ~width
  ~height
  ~samples_per_pixel
  ~max_bounces
  ~passes_per_update
  ~image
  ~on_update
  =
  let err = Option.value err ~default:(Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 0) in
  let params =
    FA.of_list
      [ Float.of_int width
      ; Float.of_int height
      ; Float.of_int samples_per_pixel
      ; Float.of_int max_bounces
      ; Float.of_int passes_per_update
      ; target_rel_err
      ]
  in
  render_progressive_flat scene params image err (fun passes_done rel_err last ->
    on_update ~passes_done ~rel_err ~last)
;;

(* [render_progressive] whose updates show the image filtered by the variance-guided a-trous denoiser (ptx_render_denoised):
   [levels] iterations (0 = no filter), the normal weight raised to 2^[normal_power_log2], the first-hit features taken from the
   first [feature_passes] passes (0 = all), [demodulate] dividing the radiance by the first-hit albedo before filtering.  The
   defaults are ptx_denoise_defaults'.  [passes_per_update] is at least 2.  [err] (if given) receives the UN-denoised per-pixel
   standard error and [features] (if given, W*H*8: albedo, normal, depth, hits) the feature means. *)
let render_denoised
  ?(target_rel_err = 0.)
  ?(levels = 5)
  ?(normal_power_log2 = 5)
  ?(feature_passes = 8)
  ?(demodulate = true)
  ?(sigma_luminance = 4.)
  ?(sigma_depth = 0.05)
  ?(sigma_albedo = 0.2)
  ?err
  ?features
  scene
  ~width
  ~height
  ~samples_per_pixel
  ~max_bounces
  ~passes_per_update
  ~image
  ~on_update
  =
  let empty () = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 0 in
  let err = Option.value err ~default:(empty ()) in
  let features = Option.value features ~default:(empty ()) in
  let params =
    FA.of_list
      [ Float.of_int width
      ; Float.of_int height
      ; Float.of_int samples_per_pixel
      ; Float.of_int max_bounces
      ; Float.of_int passes_per_update
      ; target_rel_err
      ; Float.of_int levels
      ; Float.of_int normal_power_log2
      ; Float.of_int feature_passes
      ; (if demodulate then 1. else 0.)
      ; sigma_luminance
      ; sigma_depth
      ; sigma_albedo
      ]
  in
  render_denoised_flat scene params image err features (fun passes_done rel_err last ->
    on_update ~passes_done ~rel_err ~last)
;;

(* One frame of a sequence with temporal accumulation (ptx_render_temporal; the rule is in include/ptx.h): passes [pass_first,
   pass_first + pass_count) of the SEQUENCE's [samples_per_pixel], accumulated onto the history the scene keeps from the frames
   before by reprojecting every pixel's first hit through the last frame's camera and this one's ([set_camera_pose]); history is
   dropped where the surface changed.  Advance [pass_first] from frame to frame (and wrap around [samples_per_pixel]): the same
   slice under a still camera adds the same samples again and gains nothing.  [pass_count] is at least 2.  [denoise] runs the
   variance-guided a-trous filter on the accumulated frame, with [render_denoised]'s settings.  [err] (if given) receives the
   accumulated per-pixel standard error and [motion] (if given, W*H*3) each pixel's (dx, dy, weight) into the frame before.
   The result is the number of pixels that took history: 0 for the first frame of a sequence.  History is dropped by
   [temporal_reset] and by a frame of another size, never otherwise.  Failure on a scene whose lens is on. *)
let render_temporal
  ?(max_history_passes = 64.)
  ?(normal_threshold = 0.9)
  ?(depth_tolerance = 0.02)
  ?(min_weight = 0x1p-10)
  ?(denoise = false)
  ?(levels = 5)
  ?(normal_power_log2 = 5)
  ?(demodulate = true)
  ?(sigma_luminance = 4.)
  ?(sigma_depth = 0.05)
  ?(sigma_albedo = 0.2)
  ?err
  ?motion
  scene
  ~width
  ~height
  ~samples_per_pixel
  ~max_bounces
  ~pass_first
  ~pass_count
  ~image
  =
  let empty () = Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 0 in
  let err = Option.value err ~default:(empty ()) in
  let motion = Option.value motion ~default:(empty ()) in
  let params =
    FA.of_list
      [ Float.of_int width
      ; Float.of_int height
      ; Float.of_int samples_per_pixel
      ; Float.of_int max_bounces
      ; Float.of_int pass_first
      ; Float.of_int pass_count
      ; max_history_passes
      ; normal_threshold
      ; depth_tolerance
      ; min_weight
      ; (if denoise then 1. else 0.)
      ; Float.of_int levels
      ; Float.of_int normal_power_log2
      ; 0.
      ; (if demodulate then 1. else 0.)
      ; sigma_luminance
      ; sigma_depth
      ; sigma_albedo
      ]
  in
  render_temporal_flat scene params image err motion
;;

(* [render] with per-pixel pass counts: round 1 gives every pixel [min_passes] passes, every later round gives the pixels whose
   standard error is still above [target_rel_err] times their mean radiance (at least [radiance_floor])
   [passes_per_round] more, up to [samples_per_pixel].  After every round [image] holds the frame filmed from each pixel's
   own passes, [err] (if given) its per-pixel standard error, [passes] (if given) the count map, and [on_round] runs on the
   calling thread; it returns true to stop.  The result is the number of samples in [image].  With [target_rel_err] = 0
   every pixel gets [samples_per_pixel] passes and [image] is what [render] gives.  An exception raised by [on_round] stops
   the render and is raised again once the library has returned. *)
let render_adaptive
  ?(min_passes = 8)
  ?(passes_per_round = 8)
  ?(radiance_floor = 1e-3)
  ?err
  ?passes
  scene
  ~width
  ~height
  ~samples_per_pixel
  ~max_bounces
  ~target_rel_err
  ~image
  ~on_round
  =
  let err = Option.value err ~default:(Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 0) in
  let passes = Option.value passes ~default:(Bigarray.Array1.create Bigarray.int32 Bigarray.c_layout 0) in
  let params =
    FA.of_list
      [ Float.of_int width
      ; Float.of_int height
      ; Float.of_int samples_per_pixel
      ; Float.of_int max_bounces
      ; Float.of_int min_passes
      ; Float.of_int passes_per_round
      ; target_rel_err
      ; radiance_floor
      ]
  in
  render_adaptive_flat scene params image err passes (fun round passes_done (active_next, samples, rel_err) ->
    on_round ~round ~passes_done ~active_next ~samples ~rel_err)
;;

(* [f ()] with [image] pinned; a host that renders many frames into one Bimage (an animation loop around Render_command's run)
   wraps the loop in this.  A pin that cannot be had is not an error: the renders then take the staged copy. *)
let with_pinned_image scene image f =
  (try image_pin scene image with Failure _ -> ());
  Fun.protect f ~finally:(fun () ->
    image_unpin scene;
    ignore (Sys.opaque_identity image))
;;

(* Progressive_photon_map.Make(Scene).go without its prints and its PNG: [img_sum] (W*H*3, the data of a Bimage f64 rgb)
   receives the running sum; [on_iteration] runs on the calling thread after every iteration *)
let ppm_render scene ~width ~height ~iterations ~max_bounces ~photon_count ~alpha ~(lights : light list) ~img_sum ~on_iteration =
  let params =
    FA.of_list
      [ Float.of_int width
      ; Float.of_int height
      ; Float.of_int iterations
      ; Float.of_int max_bounces
      ; Float.of_int photon_count
      ; alpha
      ]
  in
  let rows =
    List.concat_map lights ~f:(function
      | Point { position = px, py, pz; color = r, g, b; power } -> [ 0.; px; py; pz; 0.; 0.; 0.; r; g; b; power ]
      | Spot { position = px, py, pz; direction = dx, dy, dz; color = r, g, b; power } ->
        [ 1.; px; py; pz; dx; dy; dz; r; g; b; power ])
  in
  ppm_render_flat scene params (FA.of_list rows) img_sum (fun iteration radius photon_map_length ->
    on_iteration ~iteration ~radius ~photon_map_length)
;;

(* Display outputs (ptx_render_display / ptx_render_progressive_display; the rule is in include/ptx.h): the image as 8-bit or
   binary32 pixels in the format, transfer, tone curve and exposure the caller names, converted on the device and copied as what it
   is.  [Reference] is the conversion Render_command.run's PNG gets (it needs [No_tone] and exposure 1); [Linear] and [Srgb] take the
   square of the image times [exposure] through the tone curve; the binary32 formats refuse [Srgb].  The library's refusals surface
   as Failure with the rule in the message. *)
type pixel_format =
  | Rgb8
  | Rgba8
  | Rgb32f
  | Rgba32f

type transfer =
  | Reference
  | Linear
  | Srgb

type tone =
  | No_tone
  | Reinhard
  | Aces

type display =
  { format : pixel_format
  ; transfer : transfer
  ; tone : tone
  ; exposure : float
  }

(* the display image: width * height * 3 or 4 elements, row 0 on top *)
type pixels =
  | Bytes of (int, Bigarray.int8_unsigned_elt, Bigarray.c_layout) Bigarray.Array1.t
  | Floats of (float, Bigarray.float32_elt, Bigarray.c_layout) Bigarray.Array1.t

external display_defaults_flat : unit -> int * int * int * float = "ptx_ml_display_defaults_stub"

(* one C stub behind two element types: the wrappers below pick the external that fits the format *)
external render_display_u8
  :  scene
  -> floatarray (* width, height, samples_per_pixel, max_bounces, gpus, format, transfer, tone, exposure *)
  -> (int, Bigarray.int8_unsigned_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (int -> unit)
  -> unit
  = "ptx_ml_render_display_stub"

external render_display_f32
  :  scene
  -> floatarray
  -> (float, Bigarray.float32_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (int -> unit)
  -> unit
  = "ptx_ml_render_display_stub"

external render_progressive_display_u8
  :  scene
  -> floatarray (* the 18 floats of ptx_ml_render_progressive_display *)
  -> (int, Bigarray.int8_unsigned_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t (* per-pixel error, W*H*3, or empty *)
  -> (int -> float -> bool -> bool)
  -> int
  = "ptx_ml_render_progressive_display_stub"

external render_progressive_display_f32
  :  scene
  -> floatarray
  -> (float, Bigarray.float32_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (float, Bigarray.float64_elt, Bigarray.c_layout) Bigarray.Array1.t
  -> (int -> float -> bool -> bool)
  -> int
  = "ptx_ml_render_progressive_display_stub"

let pixel_format_code = function
  | Rgb8 -> 0
  | Rgba8 -> 1
  | Rgb32f -> 2
  | Rgba32f -> 3
;;

let transfer_code = function
  | Reference -> 0
  | Linear -> 1
  | Srgb -> 2
;;

let tone_code = function
  | No_tone -> 0
  | Reinhard -> 1
  | Aces -> 2
;;

let pixel_channels = function
  | Rgb8 | Rgb32f -> 3
  | Rgba8 | Rgba32f -> 4
;;

(* ptx_display_defaults: Rgb8, Reference, No_tone, exposure 1 *)
let display_defaults () =
  let format, transfer, tone, exposure = display_defaults_flat () in
  { format = (match format with 1 -> Rgba8 | 2 -> Rgb32f | 3 -> Rgba32f | _ -> Rgb8)
  ; transfer = (match transfer with 1 -> Linear | 2 -> Srgb | _ -> Reference)
  ; tone = (match tone with 1 -> Reinhard | 2 -> Aces | _ -> No_tone)
  ; exposure
  }
;;

let display_floats d =
  [ Float.of_int (pixel_format_code d.format)
  ; Float.of_int (transfer_code d.transfer)
  ; Float.of_int (tone_code d.tone)
  ; d.exposure
  ]
;;

(* a fresh display image for a width x height frame in [format] *)
let create_pixels format ~width ~height =
  let n = width * height * pixel_channels format in
  match format with
  | Rgb8 | Rgba8 -> Bytes (Bigarray.Array1.create Bigarray.int8_unsigned Bigarray.c_layout n)
  | Rgb32f | Rgba32f -> Floats (Bigarray.Array1.create Bigarray.float32 Bigarray.c_layout n)
;;

(* [render] whose image comes back as display pixels: bit for bit the display of the image [render] gives *)
let render_display ?(gpus = 1) ?display scene ~width ~height ~samples_per_pixel ~max_bounces ~update_progress =
  let display = match display with Some d -> d | None -> display_defaults () in
  let params =
    FA.of_list
      ([ Float.of_int width
       ; Float.of_int height
       ; Float.of_int samples_per_pixel
       ; Float.of_int max_bounces
       ; Float.of_int gpus
       ]
       @ display_floats display)
  in
  let pixels = create_pixels display.format ~width ~height in
  (match pixels with
   | Bytes b -> render_display_u8 scene params b update_progress
   | Floats f -> render_display_f32 scene params f update_progress);
  pixels
;;

(* [render_progressive] -- with [denoise], [render_denoised] with its settings -- whose updates are display pixels: [pixels]
   (from [create_pixels], the display's format) holds the update's display image when [on_update] runs, [err] (if given) its f64
   per-pixel standard error.  The result is the number of passes in [pixels]. *)
let render_progressive_display
  ?(target_rel_err = 0.)
  ?(denoise = false)
  ?(levels = 5)
  ?(normal_power_log2 = 5)
  ?(feature_passes = 8)
  ?(demodulate = true)
  ?(sigma_luminance = 4.)
  ?(sigma_depth = 0.05)
  ?(sigma_albedo = 0.2)
  ?display
  ?err
  scene
  ~width
  ~height
  ~samples_per_pixel
  ~max_bounces
  ~passes_per_update
  ~pixels
  ~on_update
  =
  let display = match display with Some d -> d | None -> display_defaults () in
  let err = Option.value err ~default:(Bigarray.Array1.create Bigarray.float64 Bigarray.c_layout 0) in
  let params =
    FA.of_list
      ([ Float.of_int width
       ; Float.of_int height
       ; Float.of_int samples_per_pixel
       ; Float.of_int max_bounces
       ; Float.of_int passes_per_update
       ; target_rel_err
       ]
       @ display_floats display
       @ [ (if denoise then 1. else 0.)
         ; Float.of_int levels
         ; Float.of_int normal_power_log2
         ; Float.of_int feature_passes
         ; (if demodulate then 1. else 0.)
         ; sigma_luminance
         ; sigma_depth
         ; sigma_albedo
         ])
  in
  let callback passes_done rel_err last = on_update ~passes_done ~rel_err ~last in
  match pixels, display.format with
  | Bytes b, (Rgb8 | Rgba8) -> render_progressive_display_u8 scene params b err callback
  | Floats f, (Rgb32f | Rgba32f) -> render_progressive_display_f32 scene params f err callback
  | Bytes _, _ | Floats _, _ -> invalid_arg "Ptx.render_progressive_display: pixels do not have the display's element type"
;;
