"""launch_timestamp_rules (csrc/kernels.hip) and the TokenHead's timestamp mode (csrc/decode_head.h) through the probe library, against
tests/whisper_timestamps_ref.py: real leading dimension, pad columns at +1e30. The kernel only masks, so the expected logits are exact: -inf where the
rules mask, the input bit for bit elsewhere. The one inexact step, the timestamps' log-sum-exp against the best text logit, is planted on either side
of the flip by the margin the reference asserts (64 budgets of the f32 sum), so every row of every case is compared.

Cases per (n_valid, eot, ts_begin) geometry: the five kinds of history, the largest timestamp at the last id, history lengths on both sides of the
256-id boundary of the scan and at the table's end, one shared counter and per-row counters, max_initial at -1 / 0 / 50 / past the timestamps, a row that
is -inf outside eot, and arbitrary ids after an eot. Three to five rows per call."""
import numpy as np
import pytest

import whisper_timestamps_ref as ref
from conftest import sub

pytestmark = pytest.mark.gpu


def _ids(g):
    return "x".join(map(str, g))


@pytest.fixture(scope="module", params=ref.GEOMETRIES, ids=_ids)
def cases(request):
    return request.param, ref.kernel_cases(request.param)


def test_the_kernel_masks_exactly_what_the_rule_masks(cases):
    geom, cs = cases
    n_valid = geom[0]
    probe = sub("_probe")
    for name, c in cs.items():
        want, margins, budgets = ref.apply(c["logits"], c["hists"], c["params"])
        assert np.all(margins >= ref.MARGIN_FACTOR * budgets), name
        out = probe.token_head("timestamp_rules", c["logits"], save_ids=c["save_ids"], n_saved=c["n_saved"], timestamps=c["params"])
        got = out["logits"]
        assert not np.isnan(got).any(), name
        assert (got[:, n_valid:] == probe.PAD_LOGIT).all(), name                            # the pad columns are not touched
        same = got[:, :n_valid].view(np.uint32) == want.view(np.uint32)
        assert same.all(), (name, np.argwhere(~same)[:8].tolist(), margins.tolist())
        assert np.array_equal(out["save_ids"], c["save_ids"]), name                          # the history is only read
        if np.ndim(c["n_saved"]) == 0:
            assert out["n_saved"] == c["n_saved"], name


def test_the_launcher_refuses_ids_out_of_order():
    probe, AsrError = sub("_probe"), sub("_lib").AsrError
    x = ref.grid_logits([5], 3, 129)
    tab = np.zeros((3, 8), np.int32)
    for bad in [(100, 99, 99, -1), (100, 100, 90, -1), (129, 99, 90, -1), (100, 99, -1, -1), (100, 99, 90, -2)]:
        with pytest.raises(AsrError, match="timestamp_rules"):
            probe.token_head("timestamp_rules", x, save_ids=tab, n_saved=0, timestamps=bad)


@pytest.mark.parametrize("name", list(ref.head_steps_cases()))
def test_head_steps_in_timestamp_mode(name):
    """A TokenHead in timestamp mode over 9 steps on 3 rows of width 257, alone, after the penalty and before the sampler: picks and the history table."""
    c = ref.HEAD_STEPS
    kw = ref.head_steps_cases()[name]
    x, _, _ = ref.head_steps_inputs()
    picks, save, n, decided, margins, budgets = ref.head_steps(x, c["steps"], c["ld_save"], **kw)
    assert np.all(margins >= ref.MARGIN_FACTOR * budgets) and decided.all()
    out = sub("_probe").head_steps(x, c["steps"], c["ld_save"], **kw)
    assert out["n_saved"] == n == c["steps"]
    assert np.array_equal(out["picks"], picks), (out["picks"].T, picks.T)
    assert np.array_equal(out["save_ids"], save)


def test_head_steps_without_the_mode_are_what_they_were():
    """Mode off: the head neither masks nor appends (a plain arg-max head keeps no history)."""
    c = ref.HEAD_STEPS
    x, bias, _ = ref.head_steps_inputs()
    out = sub("_probe").head_steps(x, c["steps"], c["ld_save"], c["range_"], 1.0, 0, bias=bias)
    want = ref.thr.head_steps(x, c["steps"], c["ld_save"], c["range_"], 1.0, 0, bias=bias)
    assert out["n_saved"] == 0 and np.array_equal(out["picks"], want[0])
