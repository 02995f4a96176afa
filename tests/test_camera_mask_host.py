"""The bound behind the camera-ray cluster masks (myraytracer_amd/csrc/cam_mask.hip), held on the CPU: its float64 restatement
(tests/camera_mask_ref.py) against camera rays drawn with the kernel's own float32 camera arithmetic -- every jitter corner, lens
points on the rim, both camera modes -- and the oracle's `required` set (discriminant >= 0, sphere not entirely behind the
origin): every required sphere of a ray lies in a cluster that is set in the entry of the ray's texel.

A mutation check (rho or h shrunk by 10 %: some case must fail) shows that the sampled rays reach the bound, and the tightness
check that the masks do work: on cover-glass 64x36 an entry has no more bits set than the sweep itself finds candidates for a
camera ray (experiments/cam_mask_model.py)."""
import os
import sys

import numpy as np
import pytest

import camera_mask_ref as R
from camera_mask_cases import CASES, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks(c, **kw):
    return R.camera_masks_ref(c["members"], c["n_top"], c["direct_first"], c["raw"], c["W"], c["H"], **kw)


def _missing(c, masks):
    ri, si = R.missing_pairs(masks, c["ray_tex"], c["required"], c["cluster_of"])
    return len(ri)


@pytest.mark.parametrize("name", CASES)
def test_every_required_sphere_lies_in_a_set_cluster(mrt, oracle, name):
    c = case(mrt, oracle, name)
    assert c["n_top"] <= R.MAX_RECORDS
    assert c["required"][:, c["cluster_of"] >= 0].sum() > 0, "the sampled rays meet no clustered sphere"
    masks = _masks(c)
    assert masks.shape == ((R.local_texels(c["W"], c["H"]) + 7) // 8, 4)
    n = _missing(c, masks)
    assert n == 0, f"{name}: {n} (ray, sphere) pairs the oracle requires lie in a cluster the ray's entry does not set"


def test_entries_straddle_rows_at_21x13(mrt, oracle):
    """21 is no multiple of 8: entry 2 holds texels 16 .. 23, the end of row 0 and the start of row 1, and is their union"""
    c = case(mrt, oracle, "21x13")
    masks = R.mask_bits(_masks(c))
    W = c["W"]
    both = [e for e in range(len(masks)) if (8 * e) // W != (8 * e + 7) // W]
    assert 2 in both and len(both) > 5
    ri, si = np.nonzero(c["required"])
    cl = c["cluster_of"][si]
    tex = c["ray_tex"][ri]
    for e in both[:6]:
        for row in {(8 * e) // W, (8 * e + 7) // W}:
            need = np.unique(cl[(tex >> 3 == e) & (tex // W == row) & (cl >= 0)])
            assert masks[e, need].all()


def test_shrinking_rho_or_h_by_a_tenth_loses_a_required_sphere(mrt, oracle):
    lost = {}
    for what in ("rho_scale", "h_scale"):
        lost[what] = {name: _missing(case(mrt, oracle, name), _masks(case(mrt, oracle, name), **{what: 0.9})) for name in CASES}
    print(lost)
    assert any(v > 0 for v in lost["rho_scale"].values()), "no sampled ray reaches the lens' rim"
    assert any(v > 0 for v in lost["h_scale"].values()), "no sampled ray reaches a patch's corner"


def test_an_entry_sets_no_more_clusters_than_the_sweep_finds_for_a_camera_ray(mrt, oracle):
    sys.path.insert(0, os.path.join(ROOT, "experiments"))
    from cam_mask_model import camera_ray_model
    c = case(mrt, oracle, "cover-glass")
    _, _, cand, _ = camera_ray_model(c["sc"], c["cam"], c["W"], c["H"], 10 ** 9)
    sweep_mean = cand.sum(1).mean()
    bits = R.mask_bits(_masks(c))
    px, py = R.texel_pixels(8 * len(bits), c["W"])
    on_image = (py < c["H"]).reshape(-1, 8).any(1)
    mean_bits = bits[on_image].sum(1).mean()
    print(f"cover-glass 64x36: {mean_bits:.2f} bits per entry, the sweep's {sweep_mean:.2f} candidates per camera ray")
    assert mean_bits <= sweep_mean
