"""The camera-ray sphere lists on the CPU (tests/camera_list_ref.py, the float64 restatement of cam_mask.hip's second table):
every (ray, sphere) the oracle requires of a sampled camera ray -- discriminant >= 0, the sphere not entirely behind the origin --
has the sphere's member slot on the list of the ray's entry; the masks' cluster bit is the OR of its members' list bits; the
packed entry holds at most 8 slots and marks an entry with more as overflowed."""
import numpy as np
import pytest

import camera_list_ref as L
import camera_mask_ref as R
from camera_list_cases import OVERFLOW_ENTRY, OVERFLOW_SHAPE, case


@pytest.mark.parametrize("name", ["cover-pinhole", "cover-glass"])
def test_every_required_sphere_is_on_the_list_of_its_rays_entry(mrt, oracle, name):
    c = case(mrt, oracle, name, 64, 40, rays=True)
    assert c["required"][:, c["slot_of"] >= 0].sum() > 0, "the sampled rays meet no clustered sphere"
    on = c["lists"]
    assert on.shape == ((R.local_texels(64, 40) + 7) // 8, c["n_slots"])
    ri, si = L.missing_pairs(on, np.zeros(len(on), bool), c["ray_tex"], c["required"], c["slot_of"])
    assert len(ri) == 0, f"{name}: {len(ri)} (ray, sphere) pairs the oracle requires are not on the list of the ray's entry"
    # ... and through the packed form, whose overflowed entries stand for "every sphere"
    got, over = L.unpack(L.pack(on), c["n_slots"])
    ri, si = L.missing_pairs(got, over, c["ray_tex"], c["required"], c["slot_of"])
    assert len(ri) == 0
    assert np.array_equal(got[~over], on[~over]) and np.array_equal(over, on.sum(1) > L.CAP)
    print(f"{name}: {on.sum(1).mean():.2f} slots per entry, the longest {on.sum(1).max()}, {int(over.sum())} overflowed")


@pytest.mark.parametrize("name", ["cover-pinhole", "cover-glass", "default"])
def test_a_cluster_bit_is_the_or_of_its_members(mrt, oracle, name):
    c = case(mrt, oracle, name, 64, 40)
    bits = R.mask_bits(R.camera_masks_ref(c["members"], c["n_top"], c["direct_first"], c["raw"], 64, 40))
    got, over = L.unpack(L.pack(c["lists"]), c["n_slots"])
    pad = np.zeros((len(got), 4 * R.MAX_RECORDS), bool)
    pad[:, :c["n_slots"]] = got
    assert (~over).sum() > 0
    assert np.array_equal(pad.reshape(len(got), R.MAX_RECORDS, 4).any(2)[~over], bits[~over])


def test_the_cap_is_eight_slots_and_one_more_overflows():
    on = np.zeros((4, 700), bool)
    on[0, [3, 1023 % 700, 5]] = True
    on[1, np.arange(8) * 87 + 1] = True                                    # 8: the last entry that fits
    on[2, np.arange(9) * 70 + 2] = True                                    # 9: overflowed
    words = L.pack(on)
    assert list(words[:, 0]) == [3, 8, L.OVERFLOW, 0] and not words[2, 1:].any() and not words[3].any()
    # id k at bits 10 k .. 10 k + 9 of the 96 bits: the seventh id straddles words 2 and 3
    ids = [int(s) for s in np.nonzero(on[1])[0]]
    assert int(words[1, 1]) & 1023 == ids[0] and (int(words[1, 2]) >> 28 | (int(words[1, 3]) & 63) << 4) == ids[6]
    got, over = L.unpack(words, 700)
    assert list(over) == [False, False, True, False]
    assert np.array_equal(got[[0, 1, 3]], on[[0, 1, 3]]) and not got[2].any()


def test_the_overflow_scene_overflows_exactly_the_entry_of_its_pixel(mrt, oracle):
    W, H = OVERFLOW_SHAPE
    c = case(mrt, oracle, "overflow", W, H, rays=True)
    on = c["lists"]
    assert list(np.nonzero(on.sum(1) > L.CAP)[0]) == [OVERFLOW_ENTRY]
    assert on[OVERFLOW_ENTRY, c["slot_of"][1:13]].all()                    # the column's twelve (+ what else its 8 texels see)
    got, over = L.unpack(L.pack(on), c["n_slots"])
    assert list(np.nonzero(over)[0]) == [OVERFLOW_ENTRY]
    ri, _ = L.missing_pairs(got, over, c["ray_tex"], c["required"], c["slot_of"])
    assert len(ri) == 0
