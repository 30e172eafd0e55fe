"""The dynamic-LDS layout of k_trace, k_bounce and k_bounce_carry and the "where is this scene walked from" decision
(path_tracer_ocaml_amd/csrc/pt_lds_layout.h) without a GPU: host_asan_driver's `layout` mode prints what the header says of a scene
or of explicit integers, under AddressSanitizer + UndefinedBehaviorSanitizer.

* tests/golden/lds_layout.json pins every figure to what the commit BEFORE the header computed, where host and kernels each ran
  sums of their own.  It was recorded from that commit's own text: trace_stack_bytes, trace_scene_lds_bytes, bounce_lds_bytes,
  kBounceLdsLimit, the `lds` expressions of launch_trace_inst and launch_shade_pool and scene_upload's lds_nodes64 decision out of
  ptx_api.inc, beyond_lds out of scene_host.cpp, and the offset arithmetic of pt_scene_view, k_bounce and k_bounce_carry out of
  kernels.hip (around a buffer at address 0), copied verbatim into a stand-alone program around stubs for trace_block_lds,
  bounce_threads and bounce_from_hbm, built with g++ under the same sanitizers.  The stock scenes' integers are the ones the
  driver assembles (the arrays are that commit's: tests/golden/scene_arrays.json); every synthetic case sits on one side of a
  threshold that was FOUND by bisecting that commit's predicate, the other side is the next integer.
* The k_bounce family is reached by LDS-resident scenes only, whose image is bounded by what k_trace admits, so what can push a
  launch over kBounceLdsLimit is the stacks of a deep tree: at 1, 2 and 8 waves no depth the 16-bit address bound admits does
  (the cases named "unreachable" are the deepest tree with the fullest image), at 16 waves the cases are the last depth that
  fits and the next.
* The properties further down need no fixture."""
import json
import os

import pytest

from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "lds_layout.json")))
SCENES = ["shirley", "shirley_array", "cornell", "cornell_lamp", "ganesha", "ganesha_150k"]
LDS, HBM_OCT, HBM_SHARED = 0, 1, 2
CU_BYTES = 160 * 1024
_cache = {}


def layout(built, case):
    """the driver's answer for a fixture case, computed once: a stock scene by name (its integers must come out as recorded), the
    rest by integers"""
    if case["name"] not in _cache:
        a = case["args"]
        if case["name"] in SCENES:
            cmd = ["layout", case["name"]] + [f"{k}={a[k]}" for k in ("trace_waves", "waves", "hbm", "lds_nodes64")]
        else:
            cmd = ["layout", "ints"] + [f"{k}={v}" for k, v in a.items()]
        _cache[case["name"]] = json.loads(run_clean([os.path.join(built, "host_asan_driver")] + cmd, timeout=900))
    return _cache[case["name"]]


def resident(case):
    return case["parent"]["trace_scene_lds_bytes"] > 0


def bounce_kernels(case):
    """the kernels of the k_bounce family a scene like this can reach: both on an LDS-resident scene, k_bounce on a walk from HBM / L2"""
    return ("k_bounce", "k_bounce_carry") if resident(case) else (("k_bounce",) if case["args"]["hbm"] else ())


def case_id(case):
    return case["name"]


def test_the_fixture_is_not_trivial():
    names = [c["name"] for c in FIXTURE]
    assert names[:14] == ["shirley", "shirley-lds_nodes64", "shirley-64threads", "shirley_array", "shirley_array-lds_nodes64",
                          "shirley_array-64threads", "cornell", "cornell-lds_nodes64", "cornell-64threads", "cornell_lamp",
                          "cornell_lamp-lds_nodes64", "cornell_lamp-64threads", "ganesha", "ganesha_150k"]
    by = {c["name"]: c for c in FIXTURE}
    assert by["ganesha_150k"]["args"]["n_nodes"] > 90000 and not resident(by["ganesha"]) and resident(by["cornell_lamp"])
    # one case on each side of every threshold
    assert by["beyond_lds-712"]["parent"]["beyond_lds"] == 0 and by["beyond_lds-713"]["parent"]["beyond_lds"] == 1
    assert not resident(by["beyond_lds-712"])  # the gap: small for scene_host, sent to HBM / L2 by the address bound
    for d in (1, 16, 63):
        lo, hi = [c for c in FIXTURE if c["name"].startswith(f"address-depth{d}-")]
        assert hi["args"]["n_nodes"] == lo["args"]["n_nodes"] + 1 and resident(lo) and not resident(hi) and not hi["parent"]["beyond_lds"]
    for tag in ("limit-mode0-tri0", "limit-mode1-tri0", "limit-mode1-tri1"):
        lo, hi = [c for c in FIXTURE if c["name"].startswith(tag)]
        assert hi["args"]["total_slots"] == lo["args"]["total_slots"] + 1 and resident(lo) and not resident(hi)
    assert [by[f"slots-{s}"]["args"]["total_slots"] for s in (65535, 65536)] == [65535, 65536]
    for tag in ("nodes64-kept-", "nodes64-dropped-", "nodes64-kept-bounce-", "nodes64-dropped-bounce-"):
        (c,) = [c for c in FIXTURE if c["name"].startswith(tag) and c["name"][len(tag)].isdigit()]
        assert resident(c) and c["parent"]["lds_nodes64_kept"] == (1 if "kept" in tag else 0)
    for kern in ("k_bounce", "k_bounce_carry"):
        for mode in (0, 1):
            for emit in (0, 1):
                for w in (1, 2, 8):
                    (c,) = [c for c in FIXTURE if c["name"].startswith(f"bounce_limit-{kern}-mode{mode}-emit{emit}-waves{w}-")]
                    assert "unreachable" in c["name"] and resident(c) and c["parent"][kern]["fits"] == 1 and c["args"]["waves"] == w
                lo, hi = [c for c in FIXTURE if c["name"].startswith(f"bounce_limit-{kern}-mode{mode}-emit{emit}-waves16-")]
                assert hi["args"]["tree_depth"] == lo["args"]["tree_depth"] + 1 and resident(lo) and resident(hi)
                assert lo["parent"][kern]["fits"] == 1 and hi["parent"][kern]["fits"] == 0
    assert [by[f"hbm-mode{m}-top{t}"]["args"]["n_top"] for m in (0, 1) for t in (0, 1, 1023)] == [0, 1, 1023] * 2
    assert all(by[f"hbm-mode{m}-top{t}"]["args"]["waves"] == 16 for m in (0, 1) for t in (0, 1, 1023))


@pytest.mark.parametrize("case", FIXTURE, ids=case_id)
def test_layout_equals_the_parent_commits(built, case):
    got, want = layout(built, case), case["parent"]
    assert got["in"] == want["in"] == case["args"]
    # the one placement function = beyond_lds AND trace_scene_lds_bytes > 0, as the parent's two translation units answered
    assert got["placement"] == (LDS if resident(case) else (HBM_OCT if want["beyond_lds"] else HBM_SHARED))
    assert got["lds_nodes64_kept"] == want["lds_nodes64_kept"]
    assert got["shade_pool"] == want["shade_pool"]
    t = dict(want["k_trace"])
    assert got["k_trace"]["nodes"] == t.pop("stack_bytes")  # the stacks open the buffer and end where the image starts
    if resident(case):
        assert got["k_trace"]["image_end"] - got["k_trace"]["nodes"] == want["trace_scene_lds_bytes"]
    for key, v in t.items():
        assert got["k_trace"][key] == v, ("k_trace", key)
    for kern in bounce_kernels(case):
        for key, v in want[kern].items():
            assert got[kern][key] == v, (kern, key)


REGIONS = {  # in the documented order, with the widest access of each
    "k_trace": [("stacks", 16), ("nodes", 64), ("sph", 16), ("tri", 16), ("kind", 16), ("cat", 16), ("nodes64", 16)],
    "k_bounce": [("stacks", 16), ("nodes", 64), ("sph", 16), ("tri", 16), ("kind", 16), ("cat", 16), ("nodes64", 16), ("pool_i", 4),
                 ("pool_s", 2), ("park0", 16), ("park_uv", 16), ("park_w", 16)],
    "k_bounce_carry": [("stacks", 16), ("nodes", 64), ("sph", 16), ("tri", 16), ("kind", 16), ("cat", 16), ("nodes64", 16), ("park0", 16),
                       ("park_emit", 16), ("park_uv", 16)],
}


def region_sizes(a, kern, waves, hbm):
    """what each region must hold, from the scene's integers alone"""
    n, s, arr = a["n_nodes"], a["total_slots"], a["mode"] == 1
    cap = 64 + waves * (32 if hbm else 16)
    size = {"stacks": 0 if hbm else waves * max(1, a["tree_depth"] + 1) * 16, "nodes": 0 if hbm else n * 92, "sph": 0 if hbm else s * 32,
            "tri": s * 80 if (arr and a["has_triangles"] and not hbm) else 0, "kind": s if (arr and not hbm) else 0, "cat": 0 if hbm else s,
            "nodes64": n * 48 if (a["lds_nodes64"] and not hbm) else 0}
    if kern == "k_bounce":
        size.update(pool_i=waves * 5 * 128 * 4, pool_s=waves * 5 * 128 * (4 if hbm else 2), park0=cap * 16, park_uv=cap * 16 if arr else 0,
                    park_w=cap * 16 if hbm else 0)
    if kern == "k_bounce_carry":
        size.update(park0=6 * cap * 16, park_emit=2 * cap * 16 if a["has_emit"] else 0, park_uv=cap * 16 if arr else 0)
    return size


@pytest.mark.parametrize("case", FIXTURE, ids=case_id)
def test_regions_are_ordered_disjoint_aligned_and_end_at_the_total(built, case):
    got, a = layout(built, case), case["args"]
    kernels = (("k_trace",) if resident(case) else ()) + bounce_kernels(case)
    for kern in kernels:
        g = got[kern]
        waves = a["trace_waves"] if kern == "k_trace" else a["waves"]
        hbm = kern == "k_bounce" and not resident(case)
        size = region_sizes(a, kern, waves, hbm)
        end = 0
        for name, align in REGIONS[kern]:
            assert g[name] >= end, (kern, name, "overlaps the region before it")
            assert g[name] % align == 0, (kern, name)
            end = g[name] + size[name]
        assert end == g["total"], (kern, "the last region ends at the total")
        if kern != "k_trace":
            assert g["pool_off"] % 64 == 0 and g["fits"] == (g["total"] <= got["bounce_limit"])
            if g["fits"]:  # a launch that is made leaves the kernel's static words their room
                assert g["total"] + got["static_max"] <= CU_BYTES
    if not resident(case):  # k_trace on a walk from HBM / L2 holds the tree's top and nothing else
        assert got["k_trace"]["top"] == 0 and got["k_trace"]["total"] == a["n_top"] * 64


@pytest.mark.parametrize("case", [c for c in FIXTURE if c["parent"]["trace_scene_lds_bytes"] > 0], ids=case_id)
def test_an_lds_resident_scene_fits_a_cu_and_16_bit_addresses(built, case):
    got, a = layout(built, case), case["args"]
    assert got["placement"] == LDS and got["k_trace"]["total"] + got["static_max"] <= CU_BYTES
    assert a["total_slots"] < 65536
    # the start of the last node at the largest workgroup (16 waves), behind the most static LDS a kernel may hold
    stacks16 = 16 * max(1, a["tree_depth"] + 1) * 16
    assert stacks16 % 64 == 0 and got["static_max"] % 64 == 0
    assert got["static_max"] + stacks16 + (a["n_nodes"] - 1) * 92 <= 0xFFFC
    for kern in ("k_trace", "k_bounce", "k_bounce_carry"):  # no workgroup starts its image later than the largest does
        assert got[kern]["nodes"] <= stacks16
