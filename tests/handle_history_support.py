"""A ptx_scene handle taken through many states: the model of its sticky state, the walks, and the references of every state.

Every feature of the handle was tested on a fresh one; a host changes one handle for minutes.  This module holds what the two
history modules share and needs no GPU to import:

  State, Params       the handle's sticky state as one immutable record, and the render parameters a step can change
  set_*, apply        one function per setter: the next State, or a Refusal -- the rules are include/ptx.h's text, not the library's
                      code (tests/test_handle_history_plan.py runs every walk against the library's getters on host-only handles)
  WALKS               the table: a scene of test_gpu_kernel_coverage.SCENES, its PTX_* knobs, a list of steps
  resolve, reference  the arguments a State stands for, and the restatements' samples, sums, segments and counters of a
                      (scene, State, depth, size), computed once and left unchanged

A state field holds a NAME (IMAGES, ENVS, LENSES, POSES, FILMS below say what it stands for), so states compare and hash.  The
images are a sorted tuple of (entry, name) for the entries that carry one: Shirley's texture table has 508 entries.
"""
from collections import namedtuple

import numpy as np

import test_gpu_kernel_coverage as KC

W, H, SPP, DEPTH = KC.W, KC.H, KC.SPP, KC.DEPTH
ERR_ARG, ERR_STATE = -1, -3  # PTX_ERR_ARG, PTX_ERR_STATE: what ptx_last_error()'s call returned, in PtxError's text as "(-1)"
BILINEAR, REPEAT_U, REPEAT_V = 1, 2, 4

State = namedtuple("State", "light images env env_sampling sphere_sampling lens pose projection film")
Params = namedtuple("Params", "depth count size")  # max_bounces, count_work, k: the frame is k * 13 x k * 11
Refusal = namedtuple("Refusal", "code rule message")  # message: the words include/ptx.h documents for it, or None where it gives none
Step = namedtuple("Step", "kind name arg refused")  # kind: set / params / driver; refused: the rule that refuses it, or None
Walk = namedtuple("Walk", "name scene knobs steps")

# ---- what the names stand for
IMAGES = {"A": (16, 8, 40, BILINEAR | REPEAT_U | REPEAT_V), "B": (5, 3, 42, REPEAT_U), "C": (7, 9, 44, REPEAT_V)}  # width, height, seed, flags
ENVS = ("E1", "E2")        # E1: envlight_support.environment(); E2: 12 x 6, nearest, another rotation.  "Z": 4 x 2 of zeros (no weight)
LENSES = {"off": (0.0, 1.0), "L1": (0.05, 4.0), "L2": (0.08, 3.7)}  # (radius, focus): 3.7 is no power of two, so F * q rounds
POSES = ("off", "identity", "oblique", "view")
PROJECTIONS = ("perspective", "latlong")
FILMS = {"default": (5, 1, False), "f51": (5, 1, False), "f73": (7, 3, True), "f50": (5, 0, False)}  # (order, radius, renormalise)
START = State(0, (), None, False, False, "off", "off", "perspective", FILMS["default"])
START_PARAMS = Params(DEPTH, False, 1)
# the values whose every ordered pair some step must take (the plan test); images: per entry
VALUES = {"light": (0, 1, 2), "images": (None, "A", "B", "C"), "env": (None, "E1", "E2"), "env_sampling": (False, True),
          "sphere_sampling": (False, True), "lens": tuple(LENSES), "pose": POSES, "projection": PROJECTIONS,
          "film": ((5, 1, False), (7, 3, True), (5, 0, False))}
IMAGE_PAIRS = {(None, "A"), ("A", "C"), ("C", None), (None, "C"), ("C", "A"), ("A", None), (None, "B"), ("B", None)}  # entry 0: A, C; entry 1: B
BOTH_PLACEMENTS = ("light", "images", "env", "lens", "pose")  # ... once on an LDS-resident scene and once on one walked from HBM / L2

# ---- the refusals include/ptx.h documents, by rule: (code, the words it gives for the message)
RULES = {
    "lens under latlong": (ERR_STATE, None),  # "ptx_scene_set_lens with a radius > 0 is refused likewise while LATLONG is on"
    "latlong under a lens": (ERR_STATE, "ptx_scene_set_lens(scene, 0, 1) first"),
    "sampled with nothing to sample": (ERR_ARG, None),
    "environment sampling without an environment": (ERR_ARG, "environment"),  # "a message that names the rule"
    "environment sampling without weight": (ERR_ARG, "weight"),
    "clearing a sampled environment": (ERR_STATE, "turn environment sampling off first"),
    "environment sampling off with nothing else to sample": (ERR_STATE, "set another lighting mode first"),
    "sphere sampling off with nothing else to sample": (ERR_STATE, "set another lighting mode first"),
    "sphere sampling without an emissive sphere": (ERR_ARG, "0"),  # "a message that names the count"
    "image on an entry the scene does not have": (ERR_ARG, "out of range"),
    "setter while a render runs": (ERR_STATE, None),
    "photon mapper under a lens": (ERR_STATE, "ptx_scene_set_lens(scene, 0, f) first"),
    "photon mapper under a pose": (ERR_STATE, "ptx_scene_set_camera_pose(scene, NULL, NULL, NULL) first"),
}


def refusal(rule):
    return Refusal(RULES[rule][0], rule, RULES[rule][1])


def facts(scene):
    """what the rules read of a scene: its texture entries, whether tree triangles emit, whether tree spheres do"""
    f = KC.SCENES[scene]
    return {"n_textures": KC.scene(scene)[0].contents.n_textures, "tris": f["emit"] and f["mode"] == "array",
            "spheres": f["emit"] and f["mode"] == "simd", "lds": f["lds"]}


# ------------------------------------------------------------------------------------------------ the setters, from include/ptx.h
def set_light(st, f, mode):
    if mode == 2 and not (f["tris"] or st.env_sampling or st.sphere_sampling):
        return refusal("sampled with nothing to sample")
    return st._replace(light=mode)


def set_image(st, f, arg):
    entry, name = arg
    if not 0 <= entry < f["n_textures"]:
        return refusal("image on an entry the scene does not have")
    images = dict(st.images)
    images.pop(entry, None)
    if name is not None:
        images[entry] = name
    return st._replace(images=tuple(sorted(images.items())))


def set_env(st, f, name):
    if name is None and st.env_sampling:
        return refusal("clearing a sampled environment")
    if name == "Z" and st.env_sampling:
        return refusal("environment sampling without weight")  # (the new image fails the conditions: refused, the old state kept)
    return st._replace(env=name)


def set_env_sampling(st, f, on):
    if on:
        if st.env is None:
            return refusal("environment sampling without an environment")
        if st.env == "Z":
            return refusal("environment sampling without weight")
    elif st.env_sampling and st.light == 2 and not f["tris"] and not st.sphere_sampling:
        return refusal("environment sampling off with nothing else to sample")
    return st._replace(env_sampling=bool(on))


def set_sphere_sampling(st, f, on):
    if on and not f["spheres"]:
        return refusal("sphere sampling without an emissive sphere")
    if not on and st.sphere_sampling and st.light == 2 and not f["tris"] and not st.env_sampling:
        return refusal("sphere sampling off with nothing else to sample")
    return st._replace(sphere_sampling=bool(on))


def set_lens(st, f, name):
    if LENSES[name][0] > 0.0 and st.projection == "latlong":
        return refusal("lens under latlong")
    return st._replace(lens=name)


def set_pose(st, f, name):
    assert name in POSES
    return st._replace(pose=name)


def set_projection(st, f, name):
    if name == "latlong" and LENSES[st.lens][0] > 0.0:
        return refusal("latlong under a lens")
    return st._replace(projection=name)


def set_film(st, f, name):
    return st._replace(film=FILMS[name])


SETTERS = {"light": set_light, "image": set_image, "env": set_env, "env_sampling": set_env_sampling, "sphere_sampling": set_sphere_sampling,
           "lens": set_lens, "pose": set_pose, "projection": set_projection, "film": set_film}
DRIVERS = ("progressive", "adaptive", "pixels", "features", "temporal", "render_rays", "intersect_rays", "walk_rays", "ppm", "multi")


def driver_refusal(st, name):
    """the refusal a driver call meets in a state, or None"""
    if name == "ppm":
        if LENSES[st.lens][0] > 0.0:
            return refusal("photon mapper under a lens")
        if st.pose != "off":
            return refusal("photon mapper under a pose")
        assert st.projection == "perspective"
    if name == "temporal":
        assert LENSES[st.lens][0] == 0.0 and st.projection == "perspective", "the walks run it where it is accepted"
    return None


def apply(st, params, f, step):
    """(state, params, refusal or None) after a step"""
    if step.kind == "set":
        got = SETTERS[step.name](st, f, step.arg)
        return (st, params, got) if isinstance(got, Refusal) else (got, params, None)
    if step.kind == "params":
        return st, params._replace(**step.arg), None
    assert step.kind == "driver" and step.name in DRIVERS, step
    return st, params, driver_refusal(st, step.name)


def restated_by_the_sphere_lights(st):
    """sphere-light sampling changes a pixel in mode 2 only; the composed restatement does not take it, spherelight_support's does --
    without images, a lens, a pose or the panorama, so the walks keep those off while it matters"""
    return st.sphere_sampling and st.light == 2


# ------------------------------------------------------------------------------------------------ the walks
def S(name, arg):
    return Step("set", name, arg, None)


def R(name, arg, rule):
    return Step("set", name, arg, rule)


def Pm(**kw):
    return Step("params", None, kw, None)


def D(name, rule=None):
    return Step("driver", name, None, rule)


def circuit(values):
    """the successive values of a closed walk from values[0] that takes every ordered pair of distinct values once (Hierholzer on the
    complete digraph)"""
    out = {a: [b for b in values if b != a] for a in values}
    stack, path = [values[0]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop(0))
        else:
            path.append(stack.pop())
    path.reverse()
    assert len(path) == len(values) * (len(values) - 1) + 1 and path[0] == path[-1] == values[0]
    return path[1:]


def _images_every_pair():
    """the issue's sequence on two entries -- on 0, on 1, 0 replaced by another size and filter, 0 cleared (n_images stays 1), 1 cleared
    (slot_cat back to the plain records) -- then the pairs of entry 0 it leaves out"""
    return [S("image", (0, "A")), S("image", (1, "B")), S("image", (0, "C")), S("image", (0, None)), S("image", (1, None)),
            S("image", (0, "C")), S("image", (0, "A")), S("image", (0, None))]


def _env_every_pair(lit):
    """set, sampled (in mode 2 where `lit`), replaced by one of another size and rotation while sampled, refused to clear, cleared;
    then the pairs left"""
    steps = [S("env", "E1"), S("env_sampling", True)]
    if lit:
        steps += [S("light", 2)]
    steps += [S("env", "E2"), R("env", None, "clearing a sampled environment")]
    if lit:
        steps += [S("light", 0)]
    return steps + [S("env_sampling", False), S("env", None), S("env", "E2"), S("env", "E1"), S("env", None)]


def _depths():
    return [Pm(depth=0), Pm(depth=8), Pm(depth=1), Pm(depth=4)]


def _walks():
    out = []

    def add(name, scene, steps, **knobs):
        k = dict(KC.KNOBS)
        for key, v in knobs.items():
            assert "PTX_" + key in KC.KNOBS, key
            k["PTX_" + key] = v
        assert not KC.SCENES[scene]["lds"] or "BOUNCE_ORDER" in knobs, name
        out.append(Walk(name, scene, tuple(sorted(k.items())), tuple(steps)))

    lens, pose = circuit(tuple(LENSES)), circuit(POSES)
    # ---- cornell: LDS, Array_leaf, emissive triangles, eight texture entries
    add("cornell/walk-first/camera", "cornell", BOUNCE_ORDER=0, steps=(
        [S("lens", lens[0]), D("ppm", "photon mapper under a lens"), R("projection", "latlong", "latlong under a lens")]
        + [S("lens", v) for v in lens[1:]]
        + [S("pose", pose[0]), D("ppm", "photon mapper under a pose")] + [S("pose", v) for v in pose[1:]]
        + [D("ppm"), S("projection", "latlong"), R("lens", "L1", "lens under latlong"), S("pose", "oblique"), S("pose", "off"),
           S("projection", "perspective"), D("render_rays"), D("intersect_rays"), D("walk_rays")]))
    add("cornell/shade-first/depths", "cornell", BOUNCE_ORDER=1, steps=(
        _depths() + [Pm(count=True), Pm(count=False), S("lens", "L1")] + _depths() + [Pm(count=True), Pm(depth=8), Pm(count=False), Pm(depth=4),
                                                                                    S("lens", "off"), Pm(depth=8), Pm(depth=1), Pm(depth=4)]))
    add("cornell/shade-first/shading", "cornell", BOUNCE_ORDER=1, steps=(
        [S("light", v) for v in circuit((0, 2, 1))] + [D("progressive")] + _images_every_pair()[:3] + [D("pixels"), D("features")]
        + _images_every_pair()[3:] + [R("image", (99, "A"), "image on an entry the scene does not have"),
                                      R("sphere_sampling", True, "sphere sampling without an emissive sphere")]
        + [S("film", "f51"), S("film", "f73"), D("adaptive"), S("film", "f50"), S("film", "default"), S("film", "f50"), S("film", "f73"),
           D("progressive"), S("film", "default")]
        + _env_every_pair(lit=True) + [D("temporal")]))
    # ---- shirley: LDS, Simd_leaf, no emitter: tile lists, the per-octant image, 508 texture entries
    add("shirley/shade-first/sizes", "shirley", BOUNCE_ORDER=1, steps=(
        [Pm(size=1), Pm(count=True), Pm(count=False)] + [Pm(size=k) for k in range(2, 11)] + [Pm(size=1), Pm(size=9), Pm(size=5), Pm(size=1)]))
    add("shirley/shade-first/emit", "shirley", BOUNCE_ORDER=1, steps=(
        # has_emit 0 -> 1 -> 0 on a handle whose queues, lds_nodes64 and per-octant layout were sized for 0
        [S("env", "E1"), S("env_sampling", True), S("light", 2), Pm(count=True), Pm(count=False),
         R("env_sampling", False, "environment sampling off with nothing else to sample"), S("light", 0), S("env_sampling", False), S("env", None),
         R("light", 2, "sampled with nothing to sample"), R("env_sampling", True, "environment sampling without an environment"),
         S("env", "Z"), R("env_sampling", True, "environment sampling without weight"), S("env", None),
         # the shade-first, per-octant and tile-list kernels go and come back
         S("lens", "L1"), S("lens", "off"), S("pose", "identity"), S("pose", "off"), S("image", (0, "A")), S("image", (0, None)),
         S("light", 1), S("light", 0), D("progressive"), D("render_rays"), D("walk_rays")]))
    add("shirley/walk-first/mixed", "shirley", BOUNCE_ORDER=0, steps=(
        [D("multi"), S("lens", "L2"), S("film", "f73"), S("env", "E2"), D("multi"), S("lens", "off"), S("film", "default"), S("env", None), D("multi"),
         S("projection", "latlong"), S("pose", "view"), S("projection", "perspective"), S("pose", "off"), Pm(depth=1), Pm(depth=4),
         D("temporal"), D("adaptive")]))
    # ---- walked from HBM / L2
    add("mesh_lamp/shading", "mesh_lamp", steps=(
        [S("light", v) for v in circuit((0, 2, 1))] + _images_every_pair() + [D("pixels")] + _env_every_pair(lit=True) + [D("progressive")]))
    add("mesh_lamp/camera", "mesh_lamp", steps=(
        [S("lens", v) for v in lens] + [D("features")] + [S("pose", v) for v in pose]
        + [S("projection", "latlong"), S("projection", "perspective")] + _depths() + [Pm(count=True), Pm(depth=8), Pm(count=False), Pm(depth=4),
                                                                                     D("render_rays"), D("intersect_rays")]))
    add("soup_lamp/lights", "soup_lamp", steps=(
        [S("sphere_sampling", True), S("light", 2), R("sphere_sampling", False, "sphere sampling off with nothing else to sample"),
         S("light", 1), S("sphere_sampling", False), R("light", 2, "sampled with nothing to sample"), S("sphere_sampling", True),
         S("light", 2), S("light", 0), S("sphere_sampling", False),
         # both halves on, then each alone: either may be switched off in mode 2 while the other is left to sample
         S("env", "E1"), S("env_sampling", True), S("light", 2), S("sphere_sampling", True), S("env_sampling", False), S("env_sampling", True),
         S("sphere_sampling", False), S("light", 0),
         S("env_sampling", False), S("env", None), S("lens", "L1"), S("image", (1, "B")), S("lens", "off"), S("pose", "oblique"),
         S("image", (1, None)), S("pose", "off"), D("adaptive")]))
    assert len({w.name for w in out}) == len(out)
    return out


WALKS = _walks()


def trace(walk):
    """[(step, state, params, refusal)] of a walk from START, by the model"""
    f = facts(walk.scene)
    st, params, out = START, START_PARAMS, []
    for step in walk.steps:
        st, params, ref = apply(st, params, f, step)
        out.append((step, st, params, ref))
    return out


# ------------------------------------------------------------------------------------------------ what a state stands for
_ENV = {}


def environment(name):
    """(image, flags, R) of ENVS' names and of "Z" """
    if name is None:
        return None
    if name not in _ENV:
        import envlight_support as ES
        import texture_support as TS
        _ENV[name] = {"E1": ES.environment, "E2": lambda: (TS.random_environment(12, 6, 3), 0, TS.rotation([1.0, 0.2, -0.4], 115.0)),
                      "Z": lambda: (np.zeros((2, 4, 3)), BILINEAR, None)}[name]()
    return _ENV[name]


def image(name):
    import texture_support as TS
    w, h, seed, flags = IMAGES[name]
    return TS.random_image(w, h, seed), flags


def pose_of(scene, name):
    import camera_pose_support as CP
    if name == "off":
        return None
    if name == "identity":
        return CP.Pose(CP.ZERO, CP.IDENTITY)
    if name == "oblique":
        return CP.Pose(np.array([0.05, -0.03, 0.08]), CP.OBLIQUE_R)
    llx, lly, vx, vy = CP.cam4_of(KC.scene(scene)[0])
    return CP.Pose(view=(0.7 * llx, 1.25 * lly, 0.9 * vx, 1.125 * vy))


def resolve(scene, st):
    """(images, environment, lens, pose) as the setters and the restatements take them"""
    images = {entry: image(name) for entry, name in st.images} or None
    lens = LENSES[st.lens] if LENSES[st.lens][0] > 0.0 else None
    return images, environment(st.env), lens, pose_of(scene, st.pose)


def getters_want(scene, st):
    """what the handle's getters return in a state"""
    import camera_pose_support as CP
    env = environment(st.env)
    pose = pose_of(scene, st.pose)
    return {"light": st.light,
            "images": {e: IMAGES[n][:2] + (IMAGES[n][3],) for e, n in st.images},
            "env": None if env is None else ((env[0].shape[1], env[0].shape[0], env[1]), np.eye(3) if env[2] is None else np.asarray(env[2])),
            "env_sampling": st.env_sampling, "sphere_sampling": st.sphere_sampling, "lens": LENSES[st.lens],
            "pose": None if pose is None else (pose.origin, pose.rotation, pose.view or CP.cam4_of(KC.scene(scene)[0])),
            "projection": st.projection, "film": st.film}


def getters_differ(g, scene, st):
    """the getters of a handle (host-only or not) that do not return what the model says: [] when all agree"""
    want, bad = getters_want(scene, st), []
    n = KC.scene(scene)[0].contents.n_textures
    if g.lighting()[0] != want["light"]:
        bad.append(("light", g.lighting()[0]))
    for e in sorted({0, 1, 2, n - 1} | set(want["images"])):
        if g.texture_image(e) != want["images"].get(e):
            bad.append(("image", e, g.texture_image(e)))
    env = g.environment()
    if (env is None) != (want["env"] is None) or (env is not None and (env[0] != want["env"][0] or not np.array_equal(env[1], want["env"][1]))):
        bad.append(("env", env))
    if g.environment_sampling()[0] != want["env_sampling"]:
        bad.append(("env_sampling", g.environment_sampling()))
    if g.sphere_lights()[0] != want["sphere_sampling"]:
        bad.append(("sphere_sampling", g.sphere_lights()))
    if g.lens() != want["lens"]:
        bad.append(("lens", g.lens()))
    pose = g.camera_pose
    if (pose is None) != (want["pose"] is None) or (pose is not None and not (
            np.array_equal(pose[0], want["pose"][0]) and np.array_equal(pose[1], want["pose"][1]) and tuple(pose[2]) == tuple(want["pose"][2]))):
        bad.append(("pose", pose))
    if g.camera_projection != want["projection"]:
        bad.append(("projection", g.camera_projection))
    if g.film() != want["film"]:
        bad.append(("film", g.film()))
    return bad


def call_setter(g, scene, step):
    """the library call of a setter step"""
    name, arg = step.name, step.arg
    if name == "light":
        g.set_lighting(arg)
    elif name == "image":
        if arg[1] is None:
            g.set_texture_image(arg[0], None)
        else:
            img, flags = image(arg[1])
            g.set_texture_image(arg[0], img, bilinear=bool(flags & BILINEAR), repeat=(bool(flags & REPEAT_U), bool(flags & REPEAT_V)))
    elif name == "env":
        env = environment(arg)
        if env is None:
            g.set_environment(None)
        else:
            g.set_environment(env[0], env[2], bilinear=bool(env[1] & BILINEAR))
    elif name == "env_sampling":
        g.set_environment_sampling(arg)
    elif name == "sphere_sampling":
        g.set_sphere_light_sampling(arg)
    elif name == "lens":
        g.set_lens(*LENSES[arg])
    elif name == "pose":
        pose = pose_of(scene, arg)
        if pose is None:
            g.set_camera_pose()
        else:
            pose.set_on(g)
    elif name == "projection":
        g.set_camera_projection(arg)
    else:
        assert name == "film", name
        if arg == "default":
            g.set_film()
        else:
            g.set_film(*FILMS[arg])


def refused_as_documented(err, ref):
    """a PtxError's text against a Refusal: the code, and the header's words where it gives some"""
    text = str(err)
    return ("(%d)" % ref.code) in text and (ref.message is None or ref.message in text)


def case_of(walk, st, params):
    """the state as test_gpu_kernel_coverage.expected reads it"""
    return KC.Case(walk.name, walk.scene, walk.knobs, st.light, bool(st.images), st.env is not None, st.env_sampling,
                   LENSES[st.lens][0] > 0.0, st.pose != "off" or st.projection == "latlong", (params.count,))


# ------------------------------------------------------------------------------------------------ the references
_REF, _RESTATEMENT = {}, {}


def _restatement(scene, kind):
    if (scene, kind) not in _RESTATEMENT:
        import camera_pose_support as CP
        import lens_support as LS
        import rays_support as RS
        import spherelight_support as SL
        ptr, keep = KC.scene(scene)
        _RESTATEMENT[scene, kind] = {"composed": CP.Restatement, "lens": LS.Restatement, "rays": RS.Restatement, "spheres": SL.Restatement}[kind](ptr, keep)
    return _RESTATEMENT[scene, kind]


def size_of(k):
    return k * W, k * H


def latlong_rays(scene, st, w, h, depth):
    """(rays n x 6, offsets) of every sample of the frame under the panorama: include/ptx.h's rule in numpy (projection_reference)"""
    import camera_pose_support as CP
    import projection_reference as PR
    xs, ys, ps = CP.all_samples(w, h, SPP)
    pose = pose_of(scene, st.pose)
    cxcy, _ = PR.film_coordinates(w, h, SPP, 2 + 2 * depth, xs, ys, ps)
    o, d = PR.latlong_rays(CP.ZERO if pose is None else pose.origin, CP.IDENTITY if pose is None else pose.rotation, cxcy)
    return np.concatenate([o, d], axis=1), CP.i32(ys.astype(np.int64) * w + xs + ps.astype(np.int64) * SPP)


def reference(scene, st, depth, k=1):
    """the restatement's samples of the whole frame, their pass-order sums, the segments (None where the restatement reports none), the
    oracle's counters where the paths are the oracle's, and at the base size the first-hit feature sums (None under the panorama)"""
    key = (scene, st._replace(film=None), depth, k)
    if key in _REF:
        return _REF[key]
    import camera_pose_support as CP
    from oracle import oracle as O
    ptr, keep = KC.scene(scene)
    images, env, lens, pose = resolve(scene, st)
    w, h = size_of(k)
    xs, ys, ps = CP.all_samples(w, h, SPP)
    seg, counters, feats = None, None, None
    if restated_by_the_sphere_lights(st):
        assert images is None and lens is None and pose is None and st.projection == "perspective", st
        want = _restatement(scene, "spheres").trace_samples(2, True, w, h, SPP, depth, xs, ys, ps, env, st.env_sampling)
    elif st.projection == "latlong":
        assert lens is None
        rays, offsets = latlong_rays(scene, st, w, h, depth)
        want, seg = _restatement(scene, "rays").trace_rays(rays, offsets, depth, None, images, env, st.light, st.env_sampling)
    else:
        want, seg = _restatement(scene, "composed").trace_samples(pose, w, h, SPP, depth, xs, ys, ps, images, env, st.light, st.env_sampling, lens)
    if st.light in (0, 1) and lens is None and pose is None and st.projection == "perspective":
        o = O.Scene(ptr, keep)
        _, counters = o.trace_samples(w, h, SPP, depth, xs, ys, ps)
        o.close()
        assert seg is None or counters["segments"] == seg, (scene, st)
    if k == 1 and st.projection == "perspective":
        if pose is not None:
            hits = _restatement(scene, "composed").first_hits(pose, w, h, SPP, depth, xs, ys, ps, images, env, lens=lens)
        else:
            hits = _restatement(scene, "lens").first_hits(lens or LENSES["off"], w, h, SPP, depth, xs, ys, ps, images, env)
        hits = hits.reshape(h * w, SPP, 8)
        feats = np.zeros((h * w, 8))
        for p in range(SPP):
            feats = feats + hits[:, p]
        feats.setflags(write=False)
    assert np.isfinite(want).all(), (scene, st)
    want.setflags(write=False)
    sums = CP.pass_order_sums(want, w, h, SPP)
    sums.setflags(write=False)
    _REF[key] = {"want": want, "sums": sums, "segments": seg, "counters": counters, "features": feats}
    return _REF[key]


def filmed(sums, film, spp=SPP):
    """tests/film_reference.py on the reference sums under a film (order, radius, renormalise)"""
    import film_reference as FR
    return FR.film(np.asarray(sums), film[0], film[1], FR.RENORMALISE if film[2] else 0, spp)
