"""The table of handle walks (tests/handle_history_support.py) checked without a GPU: the conditions that make the walks a test of
history -- every ordered pair of values of every state field is taken, on both placements where it matters, every walk comes back to
where it began and revisits states -- and the model of the setters checked against the library itself: every walk's setter steps run on
a host-only handle (P.Scene(desc, -1)), whose getters must equal the model after every step, refused ones included.  The GPU module
(tests/test_gpu_handle_history.py) then takes the same walks on a device."""
import pytest

import handle_history_support as HS
import test_gpu_kernel_coverage as KC

WALK_IDS = [w.name for w in HS.WALKS]


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


def _transitions(walk):
    """(field, old, new) of every accepted setter step; images: per entry"""
    out, before = [], HS.START
    for step, st, _, ref in HS.trace(walk):
        if step.kind == "set" and ref is None:
            if step.name == "image":
                out.append(("images", dict(before.images).get(step.arg[0]), step.arg[1]))
            else:
                field = step.name
                out.append((field, getattr(before, field), getattr(st, field)))
        before = st
    return out


def test_every_ordered_pair_of_every_field_is_taken():
    taken = {t for w in HS.WALKS for t in _transitions(w)}
    for field, values in HS.VALUES.items():
        pairs = HS.IMAGE_PAIRS if field == "images" else {(a, b) for a in values for b in values if a != b}
        missing = sorted((p for p in pairs if (field,) + p not in taken), key=repr)
        assert not missing, (field, missing)


@pytest.mark.parametrize("field", HS.BOTH_PLACEMENTS)
def test_the_fields_the_placement_matters_for_take_every_pair_on_both(field):
    values = HS.VALUES[field]
    pairs = HS.IMAGE_PAIRS if field == "images" else {(a, b) for a in values for b in values if a != b}
    for lds in (True, False):
        taken = {t[1:] for w in HS.WALKS if KC.SCENES[w.scene]["lds"] == lds for t in _transitions(w) if t[0] == field}
        assert not pairs - taken, (field, "LDS" if lds else "HBM / L2", sorted(pairs - taken, key=repr))


def test_the_scenes_and_orders_the_issue_names_are_walked():
    scenes = {w.scene for w in HS.WALKS}
    assert {"shirley", "cornell", "mesh_lamp", "soup_lamp"} <= scenes
    for scene in ("shirley", "cornell"):
        orders = {dict(w.knobs)["PTX_BOUNCE_ORDER"] for w in HS.WALKS if w.scene == scene}
        assert {0, 1} <= orders, scene
    for w in HS.WALKS:
        assert set(dict(w.knobs)) == set(KC.KNOBS), w.name  # every knob set explicitly


@pytest.mark.parametrize("walk", HS.WALKS, ids=WALK_IDS)
def test_a_walk_returns_revisits_and_stays_short(walk):
    steps = HS.trace(walk)
    assert len(steps) <= 60
    assert steps[-1][1] == HS.START and steps[-1][2] == HS.START_PARAMS
    seen, revisits = {(HS.START, HS.START_PARAMS)}, 0
    for step, st, params, ref in steps:
        revisits += (st, params) in seen
        seen.add((st, params))
        # a step is refused exactly where the table says so, by the rule it names
        assert (ref.rule if ref else None) == step.refused, (walk.name, step)
        if HS.restated_by_the_sphere_lights(st):
            assert not st.images and st.lens == "off" and st.pose == "off" and st.projection == "perspective", (walk.name, step)
        assert 0 <= params.depth <= 8 and 1 <= params.size <= 10
    assert 3 * revisits >= len(steps), (revisits, len(steps))


def test_the_transitions_the_issue_lists_are_in_the_table():
    def has(walk_filter, wanted):
        """some walk passing the filter holds the steps `wanted` in order (not necessarily adjacent)"""
        for w in HS.WALKS:
            if not walk_filter(w):
                continue
            it = iter(w.steps)
            if all(any(s == x for s in it) for x in wanted):
                return True
        return False
    every = lambda w: True  # noqa: E731
    S, Pm = HS.S, HS.Pm
    assert has(every, [S("lens", "L1"), S("lens", "off"), S("lens", "L2")])
    assert has(every, [S("pose", "identity"), S("pose", "oblique"), S("pose", "view"), S("pose", "off")])
    assert has(every, [S("projection", "latlong"), S("projection", "perspective")])
    assert has(every, [S("light", 2), S("light", 1), S("light", 0)])
    assert has(lambda w: w.scene == "soup_lamp", [S("sphere_sampling", True), S("light", 2), S("sphere_sampling", False)])
    assert has(lambda w: w.scene == "shirley", [S("env", "E1"), S("env_sampling", True), S("light", 2), S("light", 0)])
    assert has(lambda w: w.scene == "cornell", [S("image", (0, "A")), S("image", (1, "B")), S("image", (0, "C")), S("image", (0, None)),
                                                S("image", (1, None))])
    for lens_on in (False, True):  # the alpha tables of 2 + 2d and of 4 + 2d dimensions
        found = False
        for w in HS.WALKS:
            depths = [p.depth for step, st, p, _ in HS.trace(w) if step.kind == "params" and (st.lens != "off") == lens_on and "depth" in step.arg]
            found |= any(depths[i:i + 4] == [0, 8, 1, 4] for i in range(len(depths)))
        assert found, lens_on
    sizes = [w for w in HS.WALKS if w.scene == "shirley" and dict(w.knobs)["PTX_BOUNCE_ORDER"] == 1
             and has(lambda v: v is w, [Pm(size=k) for k in range(1, 11)] + [Pm(size=1), Pm(size=9)])]
    assert sizes
    assert has(every, [S("film", "f51"), S("film", "f73"), S("film", "f50"), S("film", "default")])
    drivers = {s.name for w in HS.WALKS for s in w.steps if s.kind == "driver"}
    assert drivers == set(HS.DRIVERS)
    refused = [(w.name, i) for w in HS.WALKS for i, s in enumerate(w.steps) if s.kind == "set" and s.refused]
    assert len(refused) >= 6


def test_every_documented_refusal_occurs_in_some_walk():
    """... "setter while a render runs" in the progressive driver's callback, which every progressive step makes"""
    hit = {s.refused for w in HS.WALKS for s in w.steps if s.refused}
    if any(s.kind == "driver" and s.name == "progressive" for w in HS.WALKS for s in w.steps):
        hit.add("setter while a render runs")
    assert hit == set(HS.RULES), sorted(set(HS.RULES) ^ hit)


@pytest.mark.parametrize("walk", HS.WALKS, ids=WALK_IDS)
def test_the_model_is_the_librarys_on_a_host_only_handle(P, walk):
    """the setters work without a device; after every step the getters equal the model, and a refusal -- by the code and the words the
    header documents -- keeps the state"""
    ptr, keep = KC.scene(walk.scene)
    g = P.Scene(ptr, -1, keepalive=keep)
    try:
        assert HS.getters_differ(g, walk.scene, HS.START) == []
        for step, st, _, ref in HS.trace(walk):
            if step.kind != "set":
                continue
            if ref is None:
                HS.call_setter(g, walk.scene, step)
            else:
                with pytest.raises(P.PtxError) as err:
                    HS.call_setter(g, walk.scene, step)
                assert HS.refused_as_documented(err.value, ref), (step, str(err.value))
            assert HS.getters_differ(g, walk.scene, st) == [], (walk.name, step)
    finally:
        g.close()


@pytest.mark.parametrize("case", KC.CASES, ids=[c.name for c in KC.CASES])
def test_the_model_takes_a_coverage_case_to_the_state_it_describes(case):
    """gpu_scene(P, case)'s setters, in its order, on the model: none is refused, and what the state stands for is state(case)"""
    import numpy as np
    f = HS.facts(case.scene)
    steps = []
    if case.tex:
        steps.append(HS.S("image", (0, "A")))
        if f["n_textures"] > 1:
            steps.append(HS.S("image", (1, "B")))
    if case.env:
        steps.append(HS.S("env", "E1"))
    if case.sampling:
        steps.append(HS.S("env_sampling", True))
    steps.append(HS.S("light", case.light))
    if case.lens:
        steps.append(HS.S("lens", "L1"))
    if case.pose:
        steps.append(HS.S("pose", "oblique"))
    st, params = HS.START, HS.START_PARAMS
    for step in steps:
        st, params, ref = HS.apply(st, params, f, step)
        assert ref is None, (case.name, step, ref)
    got, want = HS.resolve(case.scene, st), KC.state(case)
    assert (got[0] is None) == (want[0] is None)
    for entry in want[0] or {}:
        assert np.array_equal(got[0][entry][0], want[0][entry][0]) and got[0][entry][1] == want[0][entry][1]
    assert (got[1] is None) == (want[1] is None)
    if want[1] is not None:
        assert np.array_equal(got[1][0], want[1][0]) and got[1][1] == want[1][1] and np.array_equal(got[1][2], want[1][2])
    assert got[2] == want[2]
    assert (got[3] is None) == (want[3] is None)
    if want[3] is not None:
        assert np.array_equal(got[3].origin, want[3].origin) and np.array_equal(got[3].rotation, want[3].rotation) and got[3].view == want[3].view
    c = HS.case_of(HS.Walk(case.name, case.scene, case.knobs, ()), st, params)
    assert (c.light, c.tex, c.env, c.sampling, c.lens, c.pose) == (case.light, case.tex, case.env, case.sampling, case.lens, case.pose)
    assert KC.expected(c._replace(counts=case.counts)) == KC.expected(case)
