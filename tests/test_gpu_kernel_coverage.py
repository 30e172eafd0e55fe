"""Every instantiation of the four hot kernel families -- k_trace, k_shade_pool, k_bounce_carry, k_bounce: ptx_kernel_table -- launched
on the GPU and pinned, bit for bit, to the composed restatement (camera_pose_support.Restatement: tests/c/camera_pose_oracle.c over the
lens, environment-light and texture oracles and oracle/pt_oracle.c).

The module is one table, CASES.  A case is a scene, the state its setters give the handle (lighting mode, images, environment and its
sampling, lens, pose), the PTX_* knobs (read when the handle is created: set with monkeypatch before P.Scene) and the count flags it
runs with.  What a case is expected to launch is `expected(case)`: make_schedule(), run_bounces() and the four launch functions of
csrc/ptx_api.inc restated over the case's fields and the scene's facts (SCENES) -- a second statement of the scheduler, so the equality
of the launched set with it pins the scheduler's choice too.  UNREACHABLE lists the instantiations no combination of setters and knobs
selects, each with the line that excludes it.  That the cases' expected sets and UNREACHABLE together are exactly the kernel table is
checked without a device in test_kernel_coverage_abi.py: "every instantiation is launched" is a property of this table, whatever the
test order or a -k selection.

A case, per count flag: ptx_render_raw_device (the camera launches; a lens or a pose turns them into queued ones) and
ptx_trace_samples over every sample of the frame (queued launches); every sample's radiance and the raw sums equal the reference's
(uint64 views, nothing excluded); counting runs report the reference's segments, and the oracle's node, primitive and floor tests where
neither the lighting mode nor a lens or a pose changes the paths (modes 0 and 1: an image changes colours and never a path).

Frame 13 x 11 at 3 samples (two tile columns and two tile rows, both ragged), depth 4 (a camera bounce, queued bounces, a last bounce,
bounce numbers on both sides of PTX_BOUNCE_PACKET = 2)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 13, 11, 3, 4
COUNTERS = ("nodes_tested", "prims_tested", "floor_tested")

# what make_schedule reads of a scene: the leaf kind, where k_trace walks it from, whether anything in it emits, whether it can have
# camera tile lists (Simd_leaf spheres, no floor: scene_tile_lists_possible); oct: a k_bounce_carry launch fits with the per-octant LDS
# image (pt_lds_oct_layout: an emitter's larger parked record leaves no room for Shirley's); gap: beyond LDS by the address bound alone
# (pt_lds_placement's PT_PLACE_HBM_SHARED): no per-octant image and no top image, hence k_trace + k_shade_pool whatever the knobs say
SCENES = {
    "shirley": dict(mode="simd", lds=True, emit=False, tiles=True, oct=True),
    "shirley_lamp": dict(mode="simd", lds=True, emit=True, tiles=True),       # + one emissive sphere, black background
    "small_lamp": dict(mode="simd", lds=True, emit=True, tiles=True, oct=True),  # 100 spheres and an emissive one
    "soup_gap": dict(mode="simd", lds=False, emit=False, tiles=False, gap=True),  # the smallest sphere soup that is not LDS-resident
    "shirley_array": dict(mode="array", lds=True, emit=False, tiles=False),
    "cornell": dict(mode="array", lds=True, emit=True, tiles=False),          # the ceiling's two light triangles
    "mesh": dict(mode="array", lds=False, emit=False, tiles=False),           # 6000 triangles: walked from HBM / L2
    "mesh_lamp": dict(mode="array", lds=False, emit=True, tiles=False),       # + a two-triangle lamp
    "soup": dict(mode="simd", lds=False, emit=False, tiles=False),            # the smallest sphere soup with a per-octant image in HBM
    "soup_lamp": dict(mode="simd", lds=False, emit=True, tiles=False),        # ... with an emissive sphere in front of it
}
# the knobs a case can set, with the library's defaults; every case sets all of them, so nothing of the caller's environment leaks in
KNOBS = {"PTX_FUSED": 2, "PTX_FUSED_GLOBAL": 1, "PTX_BOUNCE_ORDER": 2, "PTX_PRIMARY_WALK": 2, "PTX_SOLO_ENTRIES": 0, "PTX_BOUNCE_PACKET": 0,
         "PTX_OCT_IMAGE": 1, "PTX_LDS_OCT": 1, "PTX_TILE_LISTS": 1, "PTX_TRACE_TOP": 0}
SOLO = 1 << 30

Case = namedtuple("Case", "name scene knobs light tex env sampling lens pose counts")

# (name, reason): no combination of the public setters and the PTX_* knobs selects these
UNREACHABLE = [
    ("k_trace/%s/%s/camera/lds/nopacket" % (mode, count),
     "launch_trace (csrc/ptx_api.inc): `packet = lds_scene ? (pl.on ? true : ...)` -- a camera launch on an LDS-resident scene always "
     "walks as a wave packet, whatever PTX_BOUNCE_PACKET says")
    for mode in ("simd", "array") for count in ("nocount", "count")
]


def _cases():
    out = []

    def add(name, scene, light=0, tex=False, env=False, sampling=False, lens=False, pose=False, counts=(False, True), **knobs):
        k = dict(KNOBS)
        for key, v in knobs.items():
            assert "PTX_" + key in KNOBS, key
            k["PTX_" + key] = v
        if SCENES[scene]["lds"]:  # the default order is by scene (Schedule::carry_ok): an LDS case says which it means
            assert "BOUNCE_ORDER" in knobs, name
        assert not sampling or env, name
        out.append(Case(name, scene, tuple(sorted(k.items())), light, tex, env, sampling, lens, pose, tuple(counts)))

    # ---- the two-kernel route: k_trace + k_shade_pool (PTX_FUSED = 0; from HBM / L2: PTX_FUSED_GLOBAL = 0, no per-octant image, the top in LDS)
    add("two/shirley", "shirley", FUSED=0, BOUNCE_PACKET=2, BOUNCE_ORDER=0)
    add("two/shirley_lamp/emit", "shirley_lamp", FUSED=0, BOUNCE_ORDER=0)
    add("two/shirley_lamp/lit", "shirley_lamp", light=1, FUSED=0, BOUNCE_ORDER=0)
    add("two/shirley_array/img", "shirley_array", tex=True, FUSED=0, BOUNCE_PACKET=2, BOUNCE_ORDER=0)
    add("two/cornell/emit/img", "cornell", tex=True, FUSED=0, BOUNCE_ORDER=0)
    add("two/cornell/lit/env", "cornell", light=2, env=True, sampling=True, FUSED=0, BOUNCE_ORDER=0)
    add("two/mesh", "mesh", FUSED_GLOBAL=0)
    add("two/mesh/shared-image", "mesh", OCT_IMAGE=0)
    add("two/soup", "soup", FUSED_GLOBAL=0)
    add("two/soup_lamp/top", "soup_lamp", TRACE_TOP=1)
    add("two/soup_gap", "soup_gap")  # every knob at its default
    add("camera-two/shirley", "shirley", FUSED=1, BOUNCE_ORDER=0)  # the camera rays' bounce by two kernels, the queued ones fused
    # ---- the shade-first route: k_bounce_carry (PTX_BOUNCE_ORDER = 1), its per-octant and tile-list kernels
    for scene in ("shirley", "shirley_lamp"):
        add("carry/%s" % scene, scene, BOUNCE_ORDER=1)
        add("carry/%s/packet" % scene, scene, BOUNCE_ORDER=1, PRIMARY_WALK=0)
    for scene in ("shirley", "small_lamp"):
        add("carry/%s/no-tiles" % scene, scene, counts=(False,), BOUNCE_ORDER=1, TILE_LISTS=0)
    add("carry/shirley/no-oct", "shirley", counts=(False,), BOUNCE_ORDER=1, LDS_OCT=0)
    add("carry/small_lamp", "small_lamp", counts=(False,), BOUNCE_ORDER=1)
    for scene in ("shirley_array", "cornell"):
        add("carry/%s" % scene, scene, BOUNCE_ORDER=1)
        add("carry/%s/lanewalk" % scene, scene, BOUNCE_ORDER=1, PRIMARY_WALK=1)
    # ---- k_bounce on LDS scenes, walk-first: both camera walks, the solo loop
    for scene, light in (("shirley", 0), ("shirley_lamp", 0), ("shirley_array", 0), ("cornell", 0)):
        add("bounce/%s/lanewalk" % scene, scene, light=light, BOUNCE_ORDER=0, PRIMARY_WALK=1)
        add("bounce/%s/packet-solo" % scene, scene, light=light, BOUNCE_ORDER=0, PRIMARY_WALK=0, SOLO_ENTRIES=SOLO)
    for scene, light in (("shirley_lamp", 1), ("cornell", 2)):
        add("bounce/%s/lit/lanewalk" % scene, scene, light=light, BOUNCE_ORDER=0, PRIMARY_WALK=1)
        add("bounce/%s/lit/packet" % scene, scene, light=light, BOUNCE_ORDER=0, PRIMARY_WALK=0, SOLO_ENTRIES=SOLO)  # (lit: never solo)
    # ---- k_bounce from HBM / L2
    for scene in ("mesh", "soup", "mesh_lamp", "soup_lamp"):
        add("bounce/%s" % scene, scene)
        add("bounce/%s/solo" % scene, scene, SOLO_ENTRIES=SOLO)
    add("bounce/mesh_lamp/lit", "mesh_lamp", light=2)
    add("bounce/soup_lamp/lit", "soup_lamp", light=1, SOLO_ENTRIES=SOLO)
    # ---- the IMG kernels: an image on a texture entry, or an environment
    for scene, light, how in (("shirley", 0, "tex"), ("shirley_lamp", 0, "tex"), ("shirley_lamp", 1, "tex"), ("shirley_array", 0, "env"),
                              ("cornell", 0, "tex"), ("cornell", 2, "tex")):
        kw = dict(light=light, tex=how == "tex", env=how == "env", BOUNCE_ORDER=1)  # (order 1 asked for: an IMG scene never takes it)
        add("img/%s/%d/lanewalk" % (scene, light), scene, PRIMARY_WALK=1, **kw)
        add("img/%s/%d/packet" % (scene, light), scene, PRIMARY_WALK=0, SOLO_ENTRIES=SOLO, **kw)  # (IMG: never solo)
    for scene, light, how in (("mesh", 0, "env"), ("mesh_lamp", 0, "tex"), ("mesh_lamp", 2, "tex"), ("soup", 0, "tex"), ("soup_lamp", 0, "env"),
                              ("soup_lamp", 1, "tex")):
        add("img/%s/%d" % (scene, light), scene, light=light, tex=how == "tex", env=how == "env")
    # ---- LIT x IMG behind a lens or a pose: the queued route with ray origins that are not zero
    add("img/shirley_lamp/1/lens", "shirley_lamp", light=1, tex=True, lens=True, BOUNCE_ORDER=0)
    add("img/cornell/2/env/pose", "cornell", light=2, env=True, sampling=True, pose=True, BOUNCE_ORDER=0)
    add("img/mesh_lamp/2/lens+pose", "mesh_lamp", light=2, tex=True, lens=True, pose=True)
    add("img/soup_lamp/1/env/pose", "soup_lamp", light=1, env=True, pose=True)
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------ the scheduler, restated
def expected(case, depth=DEPTH):
    """the names (ptx_kernel_table's) of the instantiations the case launches at `depth` bounces: make_schedule, run_bounces and the
    launch functions"""
    f, k = SCENES[case.scene], {key[4:]: v for key, v in case.knobs}
    simd, lds = f["mode"] == "simd", f["lds"]
    has_emit = f["emit"] or (case.light == 2 and case.sampling)  # apply_lighting: a sampled environment is an emitter
    lit = case.light != 0 and has_emit
    img = case.tex or case.env
    shading = "lit" if lit else ("emit" if has_emit else "none")
    oct_image = (not lds) and k["OCT_IMAGE"] != 0 and not f.get("gap")
    top = (not lds) and k["TRACE_TOP"] != 0 and not f.get("gap")
    from_hbm = oct_image and k["FUSED_GLOBAL"] != 0 and not top
    fused = k["FUSED"] != 0 and (lds or from_hbm)
    queued_camera = case.lens or case.pose
    carry_ok = (k["BOUNCE_ORDER"] == 1 and not lit and not img and not queued_camera and k["FUSED"] >= 2 and k["SOLO_ENTRIES"] <= 0 and lds)
    lane_walk = k["PRIMARY_WALK"] == 1 or (k["PRIMARY_WALK"] >= 2 and simd)
    lds_oct = k["LDS_OCT"] != 0 and simd and carry_ok and lane_walk and f.get("oct", False)
    tile_lists = lds_oct and k["TILE_LISTS"] != 0 and f["tiles"]
    solo = k["SOLO_ENTRIES"] > 0 and not lit and not img and not case.pose
    names = set()
    for count in case.counts:
        cnt = "count" if count else "nocount"
        for camera in ((False,) if queued_camera else (True, False)):  # render_raw_device, then trace_samples
            carry = camera and carry_ok and fused and depth >= 2  # run_bounces: the shade-first order needs a bounce to carry into
            for b in range(depth):
                primary = camera and b == 0
                prim = "camera" if primary else "queued"
                if carry:
                    walk = "lanewalk" if (primary and lane_walk) else "plain"
                    if lds_oct and not count:
                        names.add("k_bounce_carry/simd/nocount/%s/%s/%s/%s" % ("emit" if has_emit else "none", prim, walk,
                                                                              "oct-tiles" if (primary and tile_lists) else "oct"))
                    else:
                        names.add("k_bounce_carry/%s/%s/%s/%s/%s" % (f["mode"], cnt, "emit" if has_emit else "none", prim, walk))
                elif fused and (not primary or k["FUSED"] >= 2):
                    where = "hbm" if from_hbm else "lds"
                    variant = ("lanewalk" if (lane_walk and not from_hbm) else "plain") if primary else ("solo" if solo else "plain")
                    names.add("k_bounce/%s/%s/%s/%s/%s/%s/%s" % (f["mode"], cnt, shading, prim, where, variant, "img" if img else "noimg"))
                else:
                    bounce = 0 if primary else max(b, 1)
                    packet = (primary or 1 <= bounce <= k["BOUNCE_PACKET"]) if lds else (oct_image and not top)
                    names.add("k_trace/%s/%s/%s/%s/%s" % (f["mode"], cnt, prim, "lds" if lds else "hbm", "packet" if packet else "nopacket"))
                    names.add("k_shade_pool/%s/%s/%s" % (shading, prim, "img" if img else "noimg"))
    return names


# ------------------------------------------------------------------------------------------------ scenes, state, references
_SCENE, _REF = {}, {}


def _smallest_soup_beyond_lds(make, gap=False):
    """the smallest soup of the family (steps of 20 spheres) that is not LDS-resident (gap: by pt_lds_placement's address bound, the
    tree itself still below 64 KB) or whose tree alone is beyond LDS, so that it gets the per-octant image in HBM: host-only handles,
    as test_the_per_octant_walk_at_its_capacity_bound finds its bound"""
    import path_tracer_ocaml_amd as P
    from test_gpu_lds_oct import keeps_nodes64
    for n in range(600, 4000, 20):
        d, keep = make(n)
        host = P.Scene(d, -1, keepalive=keep)
        st = host.stats()
        host.close()
        beyond = st["tree_nodes"] * 92 >= 65535  # PT_SWZ_NODE_BYTES
        if gap and keeps_nodes64(st["tree_nodes"], st["leaf_slots"], st["tree_depth"]) is None:
            assert not beyond, n
            return d, keep
        if not gap and beyond:
            return d, keep
    raise AssertionError("the soups never left LDS")


def scene(name):
    """(ptx_scene_desc pointer, keepalive) of a scene of SCENES"""
    if name in _SCENE:
        return _SCENE[name]
    from oracle import oracle as O
    import lighting_support as LI
    import spherelight_support as SL
    from test_gpu_lds_oct import soup_desc
    if name in ("shirley", "shirley_array"):
        d = O.desc_shirley(W, H, no_simd=(name == "shirley_array"))
        got = (d.ptr, d)
    elif name == "shirley_lamp":
        got = SL.descs("shirley", W, H)[:2]
    elif name == "cornell":
        d = O.desc_cornell(W, H)
        got = (d.ptr, d)
    elif name == "mesh":
        d = O.desc_ganesha_like(W, H, n_target=6000)
        got = (d.ptr, d)
    elif name == "mesh_lamp":
        d, keep = LI.mesh_with_lamp(O, W, H)
        got = (C.pointer(d), (d, keep))
    elif name in ("soup", "soup_gap"):
        d, keep = _smallest_soup_beyond_lds(soup_desc, gap=(name == "soup_gap"))
        got = (C.pointer(d), (d, keep))
    elif name == "small_lamp":
        d, keep = SL.with_spheres(soup_desc(100), [(0.2, -0.1, -2.5, 0.25, 40.0, 1.0)], leaf_kind=0)
        got = (C.pointer(d), (d, keep))
    else:
        assert name == "soup_lamp"
        d, keep = _smallest_soup_beyond_lds(lambda n: SL.with_spheres(soup_desc(n), [(0.2, -0.1, -2.5, 0.25, 40.0, 1.0)], leaf_kind=0))
        got = (C.pointer(d), (d, keep))
    assert got[0].contents.leaf_kind == (0 if SCENES[name]["mode"] == "simd" else 1), name
    _SCENE[name] = got
    return got


def state(case):
    """(images, environment, lens, pose) as the setters and the restatement take them"""
    import camera_pose_support as CP
    import envlight_support as ES
    import texture_support as TS
    ptr, _ = scene(case.scene)
    images = None
    if case.tex:
        images = {0: (TS.random_image(16, 8, 40), TS.BILINEAR | TS.REPEAT_U | TS.REPEAT_V)}
        if ptr.contents.n_textures > 1:
            images[1] = (TS.random_image(5, 3, 42), TS.REPEAT_U)
    env = ES.environment() if case.env else None
    lens = (0.05, 4.0) if case.lens else None
    pose = CP.Pose(np.array([0.05, -0.03, 0.08]), CP.OBLIQUE_R) if case.pose else None
    return images, env, lens, pose


def reference(case):
    """the restatement's samples, their pass-order sums and segments, and the oracle's counters where the paths are the oracle's;
    computed once per (scene, state) and left unchanged"""
    key = (case.scene, case.light, case.tex, case.env, case.sampling, case.lens, case.pose)
    if key in _REF:
        return _REF[key]
    import camera_pose_support as CP
    from oracle import oracle as O
    ptr, keep = scene(case.scene)
    images, env, lens, pose = state(case)
    xs, ys, ps = CP.all_samples(W, H, SPP)
    r = CP.Restatement(ptr, keep)
    want, seg = r.trace_samples(pose, W, H, SPP, DEPTH, xs, ys, ps, images, env, case.light, case.sampling, lens)
    r.close()
    counters = None
    if case.light in (0, 1) and not case.lens and not case.pose:
        o = O.Scene(ptr, keep)
        rgb, counters = o.trace_samples(W, H, SPP, DEPTH, xs, ys, ps)
        o.close()
        if case.light == 0 and not case.tex and not case.env:  # no feature set: the restatement is the oracle
            assert np.array_equal(CP.bits(want), CP.bits(rgb)), case.scene
            assert counters["segments"] == seg, case.scene
    assert np.isfinite(want).all() and (want > 0).any(), case.name
    want.setflags(write=False)
    _REF[key] = {"want": want, "sums": CP.pass_order_sums(want, W, H, SPP), "segments": seg, "counters": counters}
    return _REF[key]


def gpu_scene(P, case):
    import envlight_support as ES
    import texture_support as TS
    ptr, keep = scene(case.scene)
    images, env, lens, pose = state(case)
    g = P.Scene(ptr, 0, keepalive=keep)
    if images:
        TS.set_images(g, images)
    if env is not None:
        g.set_environment(env[0], env[2], bilinear=bool(env[1] & ES.BILINEAR))
    if case.sampling:
        g.set_environment_sampling(True)
    g.set_lighting(case.light)
    if lens is not None:
        g.set_lens(*lens)
    if pose is not None:
        pose.set_on(g)
    return g


def run_case(P, torch, case, setenv):
    """the figures of one case: per count flag the samples and sums that differ from the reference and the counters, then what was
    launched.  Nothing is asserted here."""
    import camera_pose_support as CP
    for key, v in case.knobs:
        setenv(key, str(v))
    ref = reference(case)
    xs, ys, ps = CP.all_samples(W, H, SPP)
    differ = lambda a, b: int((CP.bits(a) != CP.bits(b)).any(axis=-1).sum())  # noqa: E731
    out = {"runs": []}
    g = gpu_scene(P, case)
    try:
        out["in_lds"] = g.stats()["traversal_in_lds"]
        g.clear_launched_kernels()
        out["after_clear"] = g.launched_kernels()
        for count in case.counts:
            raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
            st_r = g.render_raw_device(P.render_params(W, H, SPP, DEPTH, count_work=count), raw.data_ptr())
            got, st_t = g.trace_samples(W, H, SPP, DEPTH, xs, ys, ps, count_work=count)
            out["runs"].append({"count": count, "sums_differ": differ(raw.cpu().numpy(), ref["sums"]), "samples_differ": differ(got, ref["want"]),
                                "render": {c: int(st_r[c]) for c in ("segments",) + COUNTERS},
                                "trace": {c: int(st_t[c]) for c in ("segments",) + COUNTERS}})
        out["launched"] = g.launched_kernels()
    finally:
        g.close()
    return out


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_a_case_launches_its_kernels_and_renders_the_restatement(P, torch, case, monkeypatch):
    out = run_case(P, torch, case, monkeypatch.setenv)
    ref = reference(case)
    print(case.name, out)
    assert out["in_lds"] == int(SCENES[case.scene]["lds"])
    assert out["after_clear"] == []
    for run in out["runs"]:
        what = (case.name, run["count"])
        assert run["samples_differ"] == 0, what  # every sample of the frame, none excluded
        assert run["sums_differ"] == 0, what
        if run["count"]:
            assert run["render"]["segments"] == ref["segments"] and run["trace"]["segments"] == ref["segments"], what
            if ref["counters"] is not None:
                for c in COUNTERS:
                    assert run["render"][c] == ref["counters"][c] and run["trace"][c] == ref["counters"][c], (what, c)
    launched, want = set(out["launched"]), expected(case)
    assert len(launched) == len(out["launched"])
    assert launched == want, (sorted(launched - want), sorted(want - launched))  # nothing missing, nothing extra
    assert not launched & {name for name, _ in UNREACHABLE}


def test_the_launch_record_refuses_a_buffer_that_is_too_small(P, torch, monkeypatch):
    """after a render the record is not empty: a capacity of zero is refused and nothing is written; clearing empties it"""
    case = CASES[0]
    for key, v in case.knobs:
        monkeypatch.setenv(key, str(v))
    g = gpu_scene(P, case)
    try:
        raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        g.render_raw_device(P.render_params(W, H, SPP, DEPTH), raw.data_ptr())
        n = len(g.launched_kernels())
        assert n >= 2
        idx = np.full(n, -7, dtype=np.int32)
        assert P.lib().ptx_scene_launched_kernels(g._h, idx.ctypes.data_as(P.abi.c_int32_p), n - 1) == -1
        assert "too small" in P.last_error() and (idx == -7).all()
        assert P.lib().ptx_scene_launched_kernels(g._h, idx.ctypes.data_as(P.abi.c_int32_p), n) == n
        assert (np.diff(idx) > 0).all()
        g.clear_launched_kernels()
        assert g.launched_kernels() == []
    finally:
        g.close()
