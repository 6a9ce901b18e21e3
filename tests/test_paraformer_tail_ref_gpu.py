"""The offline Paraformer tail (CIF predictor + non-autoregressive decoder, `SvSession::enqueue_paraformer_tail`) against the float64 reference of its stages
(tests/paraformer_tail_ref.py), per utterance and per stage.

One ParaformerSession per (case, path) -- the dispatch switches are read at session creation -- on paraformer_tiny with the planted weights, eager with taps and
the profile on. Each session runs the three batches (maximum encoder length <= 128, 129 .. 256, > 256: the three attention instances), and each batch three
times over: the batch, a long batch of other data, the batch again. Per utterance, every stage on the session's OWN tapped rows of the stage before:

    alphas    predictor_exact on its `enc_out` rows                                  stat(alphas - exact)   <= 3 x E_round
    acoustic  cif_exact on its `alphas` and `enc_out` rows: the fire COUNT equal for every utterance, the n fired rows      <= 3 x E_round
    dec{i}    layer_exact(i) on its max(n, 1) rows of `acoustic` / `dec{i-1}`, its `enc_out` rows as memory                 <= 3 x E_round
    logits    head_exact on its last `dec{i}` rows                                                                          <= 3 x E_round

with E_round = stat(exact - rounded) from the two references alone (R.BF16_ROUNDINGS), both statistics (worst row's RMS, max abs; equality where E_round is
zero). The reference takes its fire decisions from the session's own f32 alphas by the rule itself, so no utterance is left out near an integer boundary and no
share of mismatches is tolerated. The f32 session has no rounding model: it is held to TOL_F32 = 1e-3 of tests/test_paraformer_gpu.py in max abs. Also asserted:
the pad rows of `acoustic` (from an utterance's count to its 16-row boundary, the dummy row of a zero-token clip) are exactly zero in the first and in the third
run, the third run's rows equal the first's bit for bit, the returned ids are the arg-max of the tapped logits rows, the batch is of the attention instance it
was built for (from the maximum encoder length; the profile shows the launches of the tail), the `run_timed` path gives the untimed path's `acoustic`, `dec{i}`
and `logits` bit for bit and the reference's fire rows (what tests/test_paraformer_timed_gpu.py and tests/test_cif_scan_timed_gpu.py assert is not repeated).

The margin of 3 is the project's (sanm_block_ref.MARGIN): it covers what the rounded twins do not model (f32 summation order, the hardware exp, flips of single
roundings). Measured stat / E_round on an MI355X, worst utterance of each (case, batch) (RMS ratio, then max-abs ratio). The three bf16 paths give the same
figures to the digits shown -- `bf16_timed` is the untimed path bit for bit, and the per-layer cross-K/V launches compute the batched ones' products:

    case   batch    alphas      acoustic    dec0        dec1        dec2        logits
    sparse le128    1.00 1.00   1.04 1.00   1.02 1.04   1.02 1.03   1.00 1.00   1.00 1.00
    sparse le256    1.00 1.00   0.97 0.87   1.00 1.00   1.02 1.00   1.00 1.00   1.00 1.00
    sparse gt256    1.00 1.00   1.00 1.00   1.00 1.00   1.02 1.00   1.00 1.00   1.00 1.00
    dense  le128    1.00 1.00   1.16 1.32   1.00 1.02   1.01 1.03   1.00 1.00   1.00 1.00
    dense  le256    1.00 1.00   1.04 1.00   1.00 1.00   1.06 1.03   1.00 1.00   1.00 1.00
    dense  gt256    1.00 1.00   1.02 1.47   1.00 1.00   1.01 1.04   1.00 1.00   1.00 1.00
    f32, max abs against the exact reference (bar 1e-3), worst batch: sparse alphas 8.1e-09 acoustic 1.0e-06 dec0 6.3e-06 dec1 4.6e-06 dec2 2.6e-06 logits 2.3e-06;
                                                                      dense  alphas 1.9e-07 acoustic 8.4e-05 dec0 9.3e-06 dec1 1.6e-05 dec2 3.7e-06 logits 3.5e-06

No stage needed a rounding point beyond those the code documents, with one remark: the `acoustic` figures hold against a twin whose RUNNING sum of alpha x hidden
is f32, as cif_scan_kernel's `hsum` is documented. Against the oracle's own line, torch.cumsum on f32 -- which on the CPU keeps the running sum in double and
rounds each output once -- the kernel sat at 9.7 (RMS) / 17 (max abs) x E_round in the sparse case and at 2.7 / 3.0 in the dense one (paraformer_tail_ref.py
says so next to the twin). No product bug was found.

NOT covered: rows of the taps at or past the device-side token-row count are not compared (they hold nothing defined); the grid splits of attn_f32_kernel that
only more than ~128 query blocks select are not reached; the wide-tile GEMM dispatch of batch 64 is not reached (tests/test_ops_gpu.py holds that).

The planted mistakes this comparison catches, and by how much, are in tests/test_paraformer_tail_ref_cpu.py (there the rounded twin stands in for a kernel).
"""
import numpy as np
import pytest

import paraformer_tail_ref as R
from conftest import sub
from test_paraformer_gpu import TOL_F32

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
# every switch the tail reads, at its default; a path overrides some. The integer-valued ones have no neutral value and are unset.
DEFAULTS = {"ASR_PF_KV_BATCH": "1", "ASR_GEMM_T144": "1", "ASR_GEMM_T144W": "1", "ASR_GEMM_T288W": "1", "ASR_GEMM_AMAX_PP": "1", "ASR_GEMM_BIG": "1",
            "ASR_GEMM_PP": "1", "ASR_GEMM_SPLITK": "1", "ASR_GEMM_DEEP": "1", "ASR_SKINNY_M144": "0"}
UNSET = ("ASR_ATTN_QT", "ASR_ATTN_NW", "ASR_SKINNY_SPLITK", "ASR_GEMM_TALL_MIN", "ASR_SKINNY_MAX_M", "ASR_SKINNY_NT", "ASR_NO_GRAPH")
# name -> (precision, environment, through run_timed)
PATHS = {
    "bf16": (BF16, {}, False),
    "bf16_kv_per_layer": (BF16, {"ASR_PF_KV_BATCH": "0"}, False),
    "bf16_timed": (BF16, {}, True),
    "f32": (F32, {}, False),
}
CASES, BATCHES = ("sparse", "dense"), tuple(R.BATCH_T)
# the attention instance of a batch: (query tiles per wave, waves, keys per chunk) from the maximum encoder length, as attention_geometry and
# launch_attention_bf16_hd128 choose them
GEOMETRY = {"le128": (1, 8, 256), "le256": (2, 8, 256), "gt256": (2, 8, 128)}
TAPS = ("enc_out", "alphas", "acoustic", "logits")

_records = {}


def _geometry(max_T):
    tiles = (max_T + 15) // 16
    qt = 1 if tiles <= 8 else 2
    return qt, min(8, (tiles + qt - 1) // qt), 256 if max_T <= 256 else 128


def _run(sess, cfg, clips, timed):
    """One eager run with taps and the profile on -> (per utterance record, the whole `acoustic` tap, the token row offsets, the profile)."""
    sess.profile_reset()
    if timed:
        out = sess.run_timed(list(clips))
        toks, fires = [o["ids"] for o in out], [o["fire_frame"] for o in out]
    else:
        toks, fires = sess.run(list(clips)), None
    prof = sess.profile_read()
    n_layers = cfg.n_dec + cfg.n_dec3
    taps = {name: sess.tap(name) for name in TAPS + tuple(f"dec{i}" for i in range(n_layers))}
    rows = sess.utterance_rows([a.size for a in clips])
    trow = sess.token_rows([t.size for t in toks])
    record = []
    for b, ((r0, T), t0) in enumerate(zip(rows, trow)):
        n = int(toks[b].size)
        m = max(n, 1)
        u = dict(enc_out=taps["enc_out"][r0:r0 + T].copy(), alphas=taps["alphas"][r0:r0 + T, 0].copy(), n=n, acoustic=taps["acoustic"][t0:t0 + m].copy(),
                 dec=[taps[f"dec{i}"][t0:t0 + m].copy() for i in range(n_layers)], logits=taps["logits"][t0:t0 + m].copy(), tokens=toks[b],
                 pad=taps["acoustic"][t0 + n:t0 + R.round_up(m, 16)].copy())
        if fires is not None:
            u["fire"] = fires[b]
        record.append(u)
    return record, prof


def _session_records(monkeypatch, case, path):
    """{batch: (first run's record, third run's record, profile of the first run)} of one session; cached, so that the timed path finds the untimed one's rows."""
    if (case, path) in _records:
        return _records[(case, path)]
    for k in UNSET:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**DEFAULTS, **PATHS[path][1]}.items():
        monkeypatch.setenv(k, v)
    cfg, ck = R.case(case)
    sess = sub("engine").ParaformerSession.from_checkpoint(cfg, ck, precision=PATHS[path][0])
    sess.taps(True)
    sess.profile(True)
    out = {}
    for b in BATCHES:
        first, prof = _run(sess, cfg, R.batch(b), PATHS[path][2])
        _run(sess, cfg, R.long_batch(), PATHS[path][2])
        again, _ = _run(sess, cfg, R.batch(b), PATHS[path][2])
        out[b] = (first, again, prof)
    _records[(case, path)] = out
    return out


def _check_batch(cfg, b, first, again, prof):
    lens = R.batch_lengths(b)
    assert tuple(u["enc_out"].shape[0] for u in first) == lens
    assert _geometry(max(lens)) == GEOMETRY[b], (b, max(lens))                                      # the batch is a test of the instance it was built for
    n = lambda name: prof.get(name, {}).get("launches", 0)
    assert n("cif") >= 1 and n("gemm_out") >= 1 and n("gemm_dec") >= 1 and n("fsmn") >= cfg.n_dec and n("attention") >= cfg.n_dec, prof
    for i, (u, v) in enumerate(zip(first, again)):
        for rec in (u, v):
            assert rec["pad"].shape[0] == R.round_up(max(rec["n"], 1), 16) - rec["n"] and not rec["pad"].any(), (b, i)      # the zero fill, not luck
            assert np.array_equal(rec["tokens"], rec["logits"][:rec["n"]].argmax(axis=1)), (b, i)
            assert all(np.isfinite(rec[f]).all() for f in ("alphas", "acoustic", "logits")), (b, i)
        assert u["n"] == v["n"] and np.array_equal(u["tokens"], v["tokens"]), (b, i)
        for f in ("enc_out", "alphas", "acoustic", "logits"):
            assert np.array_equal(u[f], v[f]), (b, i, f)
        assert all(np.array_equal(x, y) for x, y in zip(u["dec"], v["dec"])), (b, i)


def _against_the_reference(monkeypatch, case, path):
    """{batch: per utterance {stage: dict(stat, e_round, ratio)}} of one (case, path); the discrete checks are asserted on the way."""
    cfg, ck = R.case(case)
    rnd = R.F32_ROUNDINGS if PATHS[path][0] == F32 else R.BF16_ROUNDINGS
    out = {}
    for b, (first, again, prof) in _session_records(monkeypatch, case, path).items():
        _check_batch(cfg, b, first, again, prof)
        res = R.stage_runs(cfg, ck, first, rnd)
        for i, (u, r) in enumerate(zip(first, res)):
            assert u["n"] == r["n"], (case, path, b, i, u["n"], r["n"])                              # the fire count, for EVERY utterance
            if "fire" in u:
                assert np.array_equal(u["fire"], r["fire"]), (case, path, b, i)
            got = dict(alphas=u["alphas"][None], acoustic=u["acoustic"][:u["n"]], logits=u["logits"], **{f"dec{k}": x for k, x in enumerate(u["dec"])})
            for s in R.stages(cfg):
                e = r[s]
                e["stat"] = R.stat(got[s].astype(np.float64) - e["exact"]) if e["exact"].shape[0] else (0.0, 0.0)
                e["ratio"] = (R.ratio(e["stat"][0], e["e_round"][0]), R.ratio(e["stat"][1], e["e_round"][1]))
        out[b] = res
    return out


def _worst(cfg, res, field, k):
    return {s: max(r[s][field][k] for r in res) for s in R.stages(cfg)}


@pytest.mark.parametrize("path", [p for p in PATHS if PATHS[p][0] == BF16])
@pytest.mark.parametrize("case", CASES)
def test_tail_stages_against_the_float64_reference(monkeypatch, case, path):
    cfg, _ = R.case(case)
    runs = _against_the_reference(monkeypatch, case, path)
    over = []
    for b, res in runs.items():
        rms, mx = _worst(cfg, res, "ratio", 0), _worst(cfg, res, "ratio", 1)
        print(f"\n    {case:6s} {path:18s} {b:6s} " + "  ".join(f"{s} {rms[s]:.2f} {mx[s]:.2f}" for s in R.stages(cfg)))
        over += [(b, i, s, r[s]["stat"], r[s]["e_round"]) for i, r in enumerate(res) for s in R.stages(cfg) if max(r[s]["ratio"]) > R.MARGIN]
    assert not over, (case, path, len(over), over[:6])
    if path == "bf16_kv_per_layer":                              # the profile shows the path: two more cross-K/V projections per further full layer
        plain = _session_records(monkeypatch, case, "bf16")
        for b, (_, _, prof) in _session_records(monkeypatch, case, path).items():
            assert prof["gemm_dec"]["launches"] > plain[b][2]["gemm_dec"]["launches"], (b, prof["gemm_dec"], plain[b][2]["gemm_dec"])
    if PATHS[path][2]:                                           # through run_timed: the untimed path's rows, bit for bit
        plain = _session_records(monkeypatch, case, "bf16")
        for b, (first, _, _) in _session_records(monkeypatch, case, path).items():
            for i, (u, v) in enumerate(zip(first, plain[b][0])):
                assert u["n"] == v["n"] and np.array_equal(u["tokens"], v["tokens"]), (b, i)
                assert np.array_equal(u["acoustic"], v["acoustic"]) and np.array_equal(u["logits"], v["logits"]), (b, i)
                assert all(np.array_equal(x, y) for x, y in zip(u["dec"], v["dec"])), (b, i)


@pytest.mark.parametrize("case", CASES)
def test_f32_tail_stages_against_the_float64_reference(monkeypatch, case):
    cfg, _ = R.case(case)
    runs = _against_the_reference(monkeypatch, case, "f32")
    over = []
    for b, res in runs.items():
        mx = _worst(cfg, res, "stat", 1)
        print(f"\n    {case:6s} f32 {b:6s} max abs: " + "  ".join(f"{s} {mx[s]:.2e}" for s in R.stages(cfg)))
        over += [(b, i, s, r[s]["stat"]) for i, r in enumerate(res) for s in R.stages(cfg) if not r[s]["stat"][1] < TOL_F32]
    assert not over, (case, len(over), over[:6])
