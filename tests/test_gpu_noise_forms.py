"""The one reduction kernel of the noise report (noise.hip) in its four forms -- a uniform K or K per tile, a max-rel or a
summed-S tile map -- on the same crafted data (tests/noise_cases.py: NaN and +-inf in S and in a colour, L = 0, S = 0, an S whose
product with K overflows), at the sizes where its indexing can go wrong: a partial tile column, a partial band whose rows at or
beyond the height are skipped, exactly one block of 256 columns, a second block of one column.  Every expected value comes from
the references the other tests use (noise_ref, adaptive_ref, budget_ref); mrt_create accepts all five sizes as they are."""
import numpy as np
import pytest

import noise_cases
from myraytracer_amd.api import noise_report_dict

pytestmark = pytest.mark.gpu

THR, FLOOR = 0.05, 0.02


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("form", list(noise_cases.FORMS))
@pytest.mark.parametrize("size", noise_cases.FORM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_form_on_the_same_crafted_data(mrt, size, form):
    w, h = size
    S, rgba = noise_cases.form_case(size)
    want = noise_cases.form_expected(size, form, THR, FLOOR)
    frames, _ = noise_cases.FORMS[form]
    with mrt.State(mrt.Args(w, h, 1, 4, noise_cases.FORM_MAX_W), seed=5) as st:
        st.set_world(mrt.scene_default())
        st.set_noise_tracking(True)
        if frames:
            st.render(frames)
        st.debug_load_accumulation(rgba, S, noise_cases.form_tile_frames(size, form))
        st.noise_query(THR, FLOOR)
        a, max_rel = noise_cases.raw_report(mrt, st), st.read_noise_tiles()
        st.noise_query(THR, FLOOR, tile_map="sum_s")
        b, sum_s = noise_cases.raw_report(mrt, st), st.read_noise_tiles()
    noise_cases.check_same_but_kind(mrt, a, b)
    rep = noise_report_dict(a)
    print(form, size, {k: rep[k] for k in ("pixels", "non_finite", "above", "noise_factor", "sum_var", "sum_lum", "max_se")})
    assert rep["pixels"] + rep["non_finite"] == w * h
    assert rep["frames_done"] == frames and rep["noise_factor"] == want["report"]["noise_factor"]
    noise_cases.check_report(rep, want["report"])
    assert max_rel.shape == sum_s.shape == want["max_rel"].shape == want["sum_s"].shape
    assert np.array_equal(_bits(max_rel), _bits(want["max_rel"])), (max_rel, want["max_rel"])
    assert np.array_equal(_bits(sum_s), _bits(want["sum_s"])), (sum_s, want["sum_s"])
