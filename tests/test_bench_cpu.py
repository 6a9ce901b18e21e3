"""CPU: the evidence bench.py folds into its JSON line parses -- the committed rocprofv3 summaries under profiles/ (HBM traffic and SQ
counter passes, kernel-trace stats) -- and the committed bench lines keep the contract's keys."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_counter_summaries_feed_the_roofline():
    t = bench.hbm_traffic("gemm_bf16_t144")
    assert t and t["bytes_per_launch"] > 1e6 and t["source"].startswith("profiles/")
    m = bench.mfma_util("gemm_bf16_t144")
    assert m and 0.0 < m["mfma_busy_frac"] < 1.0
    shares = m["wave_cycles"]
    assert 0.9 < shares["wait_any_share"] + shares["wait_inst_any_share"] + shares["active_inst_share"] < 1.1   # disjoint buckets of the wave cycles
    r = bench.rocprof_avg_us(("gemm_bf16_t144<", "gemm_bf16_t288w<1,"))
    assert r and 5.0 < r["avg_launch_us"] < 200.0 and r["launches"] > 100


def test_committed_bench_lines_keep_the_contract():
    need = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config", "roofline"}
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[0-9]_bench_*n1.json")))
    assert len(files) >= 18 and os.path.join(ROOT, "profiles", "r02_bench_n1.json") in files
    for f in files:
        d = json.load(open(f))
        assert need <= set(d), (f, need - set(d))
        assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["data"] == "synthetic" and "workload" in d["config"], f
        assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(d["roofline"]), f
    for rnd in ("r01", "r02"):
        head = json.load(open(os.path.join(ROOT, "profiles", rnd + "_bench_n1.json")))
        assert head["cpu_baseline"]["kind"] == "port" and head["cpu_baseline"]["cores"] >= 1 and head["cpu_baseline"]["sample"]
        assert head["roofline"]["bound"] == "mfma" and abs(head["roofline"]["frac"] - head["roofline"]["achieved"] / head["roofline"]["peak"]) < 1e-3
    for f in files:      # no line prices a kernel above the machine
        frac = json.load(open(f))["roofline"]["frac"]
        assert frac is None or 0.0 < frac < 1.0, f


def test_block_kernel_numerator_is_a_known_answer():
    """roofline.achieved of the headline line = algorithmic work of the 69 blocks the block-kernel launches walk (block 0 runs as three other
    launches outside the "sanm_block" scope) / their measured time: 901.9 MFLOP x 64 windows x 69 blocks = 3 982.8 GFLOP per 64 x 8 s step."""
    import importlib
    cfgmod = importlib.import_module("automatic-speech-recognition-asr-onnx_amd.config")
    cfg = cfgmod.SenseVoiceConfig()
    lengths = [128000] * 64
    walked = bench.sensevoice_algorithmic_flops(cfg, lengths, blocks=(cfg.n_enc0, cfg.n_blocks))
    assert cfg.n_blocks - cfg.n_enc0 == 69
    assert abs(sum(walked.values()) / 1e9 - 3982.8) < 0.5
    assert walked["gemm_ctc"] == 0.0 and walked["fbank"] == 0.0
    whole = bench.sensevoice_algorithmic_flops(cfg, lengths)
    assert abs(sum(whole.values()) / 1e12 - 4.29) < 0.01                  # 67.03 GFLOP per window
    per_class = ("gemm_qkv", "gemm_out", "gemm_ffn1", "gemm_ffn2", "attention", "fsmn")
    block0 = bench.sensevoice_algorithmic_flops(cfg, lengths, blocks=(0, cfg.n_enc0))
    for k in per_class:
        assert abs(walked[k] + block0[k] - whole[k]) < 1e-3 * whole[k]


def test_full_report_prices_the_profiled_block_kernel():
    """bench.py --full: the keys sensevoice_full_report adds to the line, from a profile of two block-kernel launches of 2.864 ms per step
    (the r06 headline's sanm_block scope) over the 3 982.8 GFLOP those launches walk. The line of a plain run (sensevoice_line alone)
    carries the headline and none of the keys --full adds."""
    import argparse
    import importlib
    cfg = importlib.import_module("automatic-speech-recognition-asr-onnx_amd.config").SenseVoiceConfig()
    lengths = [128000] * 64
    flops = bench.sensevoice_algorithmic_flops(cfg, lengths)
    prof = {"sanm_block": {"total_ms": 3 * 5.7295, "launches": 6}, "gemm_ctc": {"total_ms": 3 * 0.1989, "launches": 3}}
    legs = {"elapsed_resident": 20 * 6.4e-3, "steady": None, "prof": prof, "t_inflight": 6.2e-3}
    args = argparse.Namespace(steps=20, profile_steps=3)
    rep = bench.sensevoice_full_report(args, cfg, 64, 128000, 1, lengths, 512.0, 6.481, flops, sum(flops.values()), legs)
    assert set(rep) == {"audio_resident", "steady", "roofline", "kernels", "inflight"} and rep["steady"] is None
    assert rep["kernels"]["sanm_block"] == {"ms_per_step": 5.7295, "launches_per_step": 2, "tflops": 695.1}
    assert rep["roofline"]["achieved"] == 695.1 and rep["roofline"]["launches_per_step"] == 2 and rep["roofline"]["blocks_per_step"] == 69
    assert rep["audio_resident"]["ms_per_step"] == 6.4 and rep["inflight"]["ms_per_batch"] == 6.2
    args = argparse.Namespace(steps=20, warmup=5, seconds=8.0)
    line = bench.sensevoice_line(args, 64, 1, 512.0, 20 * 6.481e-3, 6.481, 512.0 / 6.481e-3, sum(flops.values()), 0.05)
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"} <= set(line)
    assert line["value"] == round(512.0 / 6.481e-3, 1) and line["ms_per_step"] == 6.481 and line["unit"] == "audio-s/s" and line["dtype"] == "bf16"
    assert not set(line) & (set(rep) | {"cpu_baseline", "parity_spotcheck", "secondary"})


def test_dump_outputs_writes_float64_npy_files_within_the_bound(tmp_path):
    tok = np.arange(64 * 137, dtype=np.int32).reshape(64, 137)
    num = np.full(64, 137, np.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"token_ids": tok, "num_ids": num})
    for name, want in (("token_ids", tok), ("num_ids", num)):
        got = np.load(tmp_path / "d" / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    with pytest.raises(ValueError, match="exceed"):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, np.float32)})
    assert not os.path.exists(tmp_path / "big")


@pytest.mark.parametrize("argv,msg", [(["--steps", "0"], "--steps must be at least 1"),
                                      (["--workload", "whisper", "--dump-outputs", "d"], "--dump-outputs is implemented for the sensevoice workload only")])
def test_bench_rejects_arguments_it_cannot_honour(argv, msg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and msg in r.stderr
