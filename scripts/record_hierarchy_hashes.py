#!/usr/bin/env python3
"""Records tests/golden/hierarchy_hashes.json: a sha256 per array of what the host builder makes of a scene (the mrt_debug_build_*
entry points) and of what the device holds after mrt_update_spheres / mrt_regroup_spheres (mrt_debug_read_hierarchy), with the
commit they were recorded from.  tests/test_hierarchy_hashes_host.py and tests/test_gpu_update_spheres.py recompute the hashes
and compare, so a change that is meant to leave the hierarchy's bits alone can show that it did.  The cases are the tests' own
(host_cases there, HASH_CASES here); this file only hashes.

A pull request that MEANS to change the builder or the refit re-records, from its own build, and says so:
    python scripts/record_hierarchy_hashes.py --host                       (no GPU)
    python scripts/record_hierarchy_hashes.py --device [--commit ID]       (GPU; --commit where there is no git checkout)
Each run keeps the other part of the file as it is.  --out writes somewhere else than the fixture."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hierarchy_hashes.json")


def digest(v):
    """sha256 of an array's dtype, shape and bytes; scalars, tuples and lists as int64 / float64 arrays"""
    a = np.ascontiguousarray(v)
    if a.dtype == bool or (a.dtype.kind in "iu" and not isinstance(v, np.ndarray)):
        a = a.astype(np.int64)
    elif a.dtype.kind == "f" and not isinstance(v, np.ndarray):
        a = a.astype(np.float64)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def host_hashes(mrt, sc, max_levels, top_target, sweep=False):
    """every output of the host builder's diagnostic entry points for one scene and depth rule (`sweep`: mrt_debug_build_sweep as
    well, which builds with the automatic depth rule whatever max_levels / top_target say)"""
    from myraytracer_amd import _lib
    L = _lib.load()
    sc = np.ascontiguousarray(sc, mrt.SPHERE_DTYPE)
    n, out = len(sc), {}
    info = (C.c_uint32 * 10)()
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, n, max_levels, top_target, None, 0, None, 0, None, 0, None, 0, None, info) == 0
    top, nodes = np.zeros((info[1], 4), np.float32), np.zeros((info[2], 4), np.float32)
    midx, mf = np.zeros(info[3], np.uint32), np.zeros(info[1] // 32 * 512, np.uint16)
    org = (C.c_float * 3)()
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, n, max_levels, top_target, top.ctypes.data, len(top), nodes.ctypes.data, len(nodes),
                                       midx.ctypes.data, len(midx), mf.ctypes.data, len(mf), org, info) == 0
    out.update({"hierarchy.info": digest(list(info)), "hierarchy.top": digest(top), "hierarchy.nodes": digest(nodes),
                "hierarchy.member_index": digest(midx), "hierarchy.mfma": digest(mf), "hierarchy.origin": digest(np.array(list(org), np.float32))})
    binfo = (C.c_uint32 * 8)()
    assert L.mrt_debug_build_boxes(sc.ctypes.data, n, max_levels, top_target, None, 0, binfo) == 0
    boxes = np.zeros((binfo[1], 8), np.float32)
    assert L.mrt_debug_build_boxes(sc.ctypes.data, n, max_levels, top_target, boxes.ctypes.data, len(boxes), binfo) == 0
    out.update({"boxes.info": digest(list(binfo)), "boxes": digest(boxes)})
    for key, wide in (("boxes_top_down", 0), ("boxes_top_down_open", 1)):
        tinfo = (C.c_uint32 * 5)()
        assert L.mrt_debug_build_boxes_top_down(sc.ctypes.data, n, max_levels, top_target, wide, None, 0, tinfo) == 0
        dev = np.zeros((tinfo[1], 8), np.float32)
        assert L.mrt_debug_build_boxes_top_down(sc.ctypes.data, n, max_levels, top_target, wide, dev.ctypes.data, len(dev), tinfo) == 0
        out.update({key + ".info": digest(list(tinfo)), key: digest(dev)})
    n_pool = C.c_uint32()
    assert L.mrt_debug_pool_clusters(sc.ctypes.data, n, max_levels, top_target, C.byref(n_pool)) == 0
    out["pool_clusters"] = digest(int(n_pool.value))
    if sweep:
        for key, force in (("sweep", None), ("sweep_forced_2_1_4", (C.c_float * 3)(2.0, 1.0, 4.0))):
            assert L.mrt_debug_build_hierarchy(sc.ctypes.data, n, 4, 0, None, 0, None, 0, None, 0, None, 0, None, info) == 0
            axis, sorg, reach = (C.c_float * 3)(), (C.c_float * 3)(), C.c_double()
            rec, smf = np.zeros((info[1], 4), np.float32), np.zeros(info[1] // 32 * 512, np.uint16)
            assert L.mrt_debug_build_sweep(sc.ctypes.data, n, force, axis, rec.ctypes.data, len(rec), smf.ctypes.data, len(smf), sorg,
                                           C.byref(reach)) == 0
            out.update({key + ".axis": digest(np.array(list(axis), np.float32)), key + ".records": digest(rec), key + ".operand": digest(smf),
                        key + ".origin": digest(np.array(list(sorg), np.float32)), key + ".reach": digest(np.float64(reach.value))})
    return out


def device_hashes(h):
    """every array and scalar of State.debug_read_hierarchy()"""
    return {k: digest(v) for k, v in sorted(h.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    if not (a.host or a.device):
        ap.error("nothing to record: --host and / or --device")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import myraytracer_amd as mrt
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    doc = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}
    if a.host:
        from test_hierarchy_hashes_host import host_cases
        doc["host"] = {"commit": commit, "hashes": {key: host_hashes(mrt, *case) for key, case in host_cases(mrt)}}
    if a.device:
        from test_gpu_update_spheres import HASH_CASES, refitted_hierarchy
        doc["device"] = {"commit": commit, "hashes": {f"{name}|{which}": device_hashes(refitted_hierarchy(mrt, name, which)) for name, which in HASH_CASES}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: " + ", ".join(f"{len(doc[p]['hashes'])} {p} cases from {doc[p]['commit'][:12]}" for p in ("host", "device") if p in doc))


if __name__ == "__main__":
    main()
