"""CPU: the numpy statement of the feature-mix launches (tests/_featmix_ref.py) against what the REFERENCE returned
(tests/golden/featmix.json + .npz, tools/make_golden_featmix.py) for every golden group: the float64 truth lies within the recorded
``reference_max_abs`` of the reference's batch (that IS its definition; a drift of either shows here), the float32 model of the launch is
within the bar -- per element ``max(2 x reference_max_abs, 2 x spacing(float32(|truth|)))`` -- and copy-form rows are bit-equal.  The
binary16 fixtures widened to float32 give the same model bit for bit."""
import numpy as np
import pytest

import _featmix_ref as R

GROUPS = ["right", "left", "both", "cutmix", "snr_first", "pad_value", "off_by_one", "truncated", "k2"]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def test_the_groups_are_what_the_issue_lists(golden):
    assert sorted(golden) == sorted(GROUPS)
    cm = golden["cutmix"]["table"]
    assert max(len(c.tracks) for c in cm) >= 5 and any(t.snr is not None and t.first > 0 for c in cm for t in c.tracks)
    assert golden["snr_first"]["table"][0].ref_track == 1 and golden["snr_first"]["table"][0].tracks[0].snr == 7.5
    assert golden["pad_value"]["table"][0].pad_value == -5.0 and golden["pad_value"]["table"][0].form == 0
    assert any(t.rows == t.frames - 1 for c in golden["off_by_one"]["table"] for t in c.tracks)
    assert all(c.form == 0 for c in golden["right"]["table"]) and any(c.form == 1 for c in golden["left"]["table"])
    assert all(r is None or 0 < r < 1e-5 for g in golden.values() for r in g["reference_max_abs"])


@pytest.mark.parametrize("name", GROUPS)
def test_truth_and_model_against_the_reference(golden, name):
    g = golden[name]
    truth = R.batch(g["arena"], g["table"], g["F"], g["row_frames"])
    for b, r in enumerate(g["reference_max_abs"]):
        if r is not None:  # the truth is where the fixture says it is
            assert float(np.abs(g["ref"][b].astype(np.float64) - truth[b]).max()) == pytest.approx(r, rel=1e-6)
    assert (g["lens"] <= g["row_frames"]).all() and g["ref"].shape == (len(g["table"]), g["row_frames"], g["F"])
    model = R.batch(g["arena"], g["table"], g["F"], g["row_frames"], model=True)
    R.check_against_golden(g, model, name)
    wide, table = R.widened(g["arena"], g["table"], g["F"])
    assert np.array_equal(R.batch(wide, table, g["F"], g["row_frames"], model=True).view(np.uint32), model.view(np.uint32))


def test_the_tail_of_both_holds_log_2e_10(golden):
    g = golden["both"]
    short = int(np.argmin(g["lens"]))
    assert np.allclose(g["ref"][short][-3:], np.log(2e-10), rtol=0, atol=1e-5)
    assert np.allclose(R.batch(g["arena"], g["table"], g["F"], g["row_frames"])[short][-3:], np.log(2e-10), rtol=0, atol=1e-6)  # (the padding value is float32(log(1e-10)))
