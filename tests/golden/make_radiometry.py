#!/usr/bin/env python3
"""The Monte-Carlo fixtures tests/golden/radiometry_<scene>.npz: per pixel the mean RGB, the mean luminance and the per-sample
variance of the luminance (float64), by the float64 numpy path tracer of tests/radiometry_ref.py (numpy's PCG64; neither the
oracle nor the product takes part), with its own sample count `n`, so that the fixture's error enters every comparison.

The image is cut into row bands, every band has a PCG64 stream of its own spawned from (seed, scene, row), so the result does
not depend on the number of worker processes.

Run from the repository root:
    python tests/golden/make_radiometry.py [--n 32768] [--only glass,fuzzy,...] [--jobs 8]
    python tests/golden/make_radiometry.py --selfcheck [--n 1024]     # the reference through its own test, five other seeds
"""
import argparse
import os
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(GOLDEN))

import radiometry_ref as R

SEED = 20240607
BAND = 2                                    # rows per work item
# closed-form scenes: only the pixels that are not smooth (silhouettes, the edge of total reflection) need the integrator, and
# they need MORE samples: a pixel the sphere covers by 2e-4 has a variance made of rare events, and a truth that has seen none
# of them underestimates it (an 8,192-sample truth read |z| = 10.6 for the oracle at such a pixel)
EDGES_ONLY = tuple(n for n in R.CLOSED_FORM if n not in R.FIXTURES and n != "sky")
EDGE_N = 65536


def _band(args):
    name, n, seed, y0, edges = args
    mask = np.zeros((R.HEIGHT, R.WIDTH), bool)
    mask[y0:y0 + BAND] = True
    if edges:                               # the closed form holds everywhere else: the other pixels stay NaN
        mask &= ~R.truth(name)["smooth"]
    mc = R.monte_carlo(name, n, np.random.SeedSequence([seed, zlib.crc32(name.encode()), y0]), pixels=mask)
    return y0, {k: mc[k][y0:y0 + BAND] for k in ("rgb", "mu", "var")}


def render(name, n, seed, pool, edges=False):
    out = dict(rgb=np.zeros((R.HEIGHT, R.WIDTH, 3)), mu=np.zeros((R.HEIGHT, R.WIDTH)), var=np.zeros((R.HEIGHT, R.WIDTH)), n=n)
    for y0, part in pool.map(_band, [(name, n, seed, y0, edges) for y0 in range(0, R.HEIGHT, BAND)]):
        for k, v in part.items():
            out[k][y0:y0 + BAND] = v
    return out


def path(name):
    return os.path.join(GOLDEN, f"radiometry_{name}.npz")


def load(name):
    with np.load(path(name)) as f:
        return {k: (int(f[k]) if k == "n" else f[k]) for k in f.files}


def selfcheck(n, pool):
    """Integrator (c) with five other seeds at the host test's sample count through the assertions the oracle is put
    through: against the closed forms on the smooth pixels and against the committed fixtures."""
    lines = []
    for seed in (1, 2, 3, 4, 5):
        for name in R.CLOSED_FORM + tuple(f for f in R.FIXTURES if f not in R.CLOSED_FORM):
            got = render(name, n, seed, pool)
            tr = R.truth(name, load(name) if name != "sky" else None)
            groups = ([("smooth", tr["smooth"])] if name in R.CLOSED_FORM else []) + [("all", None)]
            for label, pixels in groups:
                lines.append(R.check(R.statistics(got["rgb"], tr, 1.0 / n, pixels), label=f"reference seed {seed} {name} [{label}] n={n}"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--only", default=",".join(R.FIXTURES + EDGES_ONLY))
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--selfcheck", action="store_true")
    ap.add_argument("--out", default=None, help="--selfcheck: append the lines to this file")
    a = ap.parse_args()
    with ProcessPoolExecutor(a.jobs) as pool:
        if a.selfcheck:
            lines = selfcheck(a.n or 1024, pool)
            if a.out:
                with open(a.out, "a") as f:
                    f.write("\n".join(lines) + "\n")
            return
        for name in a.only.split(","):
            t0 = time.time()
            mc = render(name, EDGE_N if name in EDGES_ONLY else (a.n or 32768), SEED, pool, edges=name in EDGES_ONLY)
            np.savez_compressed(path(name), rgb=mc["rgb"], mu=mc["mu"], var=mc["var"], n=np.int64(mc["n"]))
            print(f"{name}: n={mc['n']} mean L={np.nanmean(mc['mu']):.5f} {time.time() - t0:.1f} s -> {os.path.getsize(path(name))} bytes")


if __name__ == "__main__":
    main()
