"""The host builder's outputs, bit for bit, against tests/golden/hierarchy_hashes.json (no GPU): a sha256 per array of
mrt_debug_build_hierarchy, mrt_debug_build_boxes, mrt_debug_build_boxes_top_down (open and not), mrt_debug_build_sweep and
mrt_debug_pool_clusters, recorded by scripts/record_hierarchy_hashes.py from the commit the fixture names.  The invariants of
the builder are tests/test_hierarchy_host.py's; this test says that a change which means to leave the builder's arithmetic alone
did.  A change that means to move a bound re-records the fixture (the script's docstring) and says so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from record_hierarchy_hashes import FIXTURE, host_hashes  # noqa: E402
from test_hierarchy_host import scenes  # noqa: E402


def host_cases(mrt):
    """(key, (scene, max_levels, top_target, with mrt_debug_build_sweep)): every scene of test_hierarchy_host.scenes under the
    automatic depth rule and two forced ones, and the layouts of test_gpu_update_spheres as its tests build them, the 4,200-sphere
    one also forced to four levels"""
    from test_gpu_update_spheres import HASH_LAYOUTS, LAYOUTS, scene
    for name, sc in scenes(mrt):
        for levels, target in ((4, 0), (4, 1), (2, 8)):
            yield f"{name}|{levels},{target}", (sc, levels, target, (levels, target) == (4, 0))
    for name, (_, forced) in LAYOUTS.items():
        levels, target = forced or (4, 0)
        yield f"{name}|{levels},{target}", (scene(mrt, name), levels, target, True)
    base, (levels, target) = HASH_LAYOUTS["deep-4200"]
    yield f"deep-4200|{levels},{target}", (scene(mrt, base), levels, target, False)


def test_the_host_builders_arrays_hash_to_the_recorded_ones(mrt):
    want = json.load(open(FIXTURE))["host"]["hashes"]
    seen = set()
    for key, case in host_cases(mrt):
        got = host_hashes(mrt, *case)
        assert key in want, f"{key}: not in the fixture"
        assert got.keys() == want[key].keys(), key
        differ = sorted(k for k in got if got[k] != want[key][k])
        assert not differ, f"{key}: {differ} differ from the recorded build"
        seen.add(key)
    assert seen == set(want)


def test_the_deep_layout_has_four_levels(mrt):
    """what the device test of the 64-lane refit kernel relies on: 4,200 spheres forced to (4, 8) give 1,050 clusters under
    levels of 263, 66 and 17 (the top) real records"""
    import numpy as np
    from test_gpu_update_spheres import HASH_LAYOUTS, scene
    from test_hierarchy_host import build
    base, (levels, target) = HASH_LAYOUTS["deep-4200"]
    h = build(mrt, scene(mrt, base), levels, target)
    assert h["levels"] == 4 and len(h["top"]) == 32
    bases = h["level_base"] + [len(h["nodes"])]
    real = [int(np.isfinite(h["nodes"][bases[k]:bases[k + 1], 3]).sum()) for k in (1, 2, 3)] + [int(np.isfinite(h["top"][:, 3]).sum())]
    assert real == [1050, 263, 66, 17]
