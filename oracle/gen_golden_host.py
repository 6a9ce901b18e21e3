"""Host-side goldens from the REAL reference functions (build container only); see oracle/gen_golden.py.

    python -m oracle.gen_golden_host       # writes tests/golden/ort_io_reference.npz, whisper_repeats_reference.npz

Two pieces of the reference's host code have restatements in the product package: ORT_IO.py (array_for /
scalar_for, restated by ort_io.py) and Whisper's remove_repeated_parts (restated by whisper.py). The case grids
below are the single definition of their inputs: this script runs the reference on them and commits the
outputs as data, and tests/test_shim_cpu.py / tests/test_whisper_host.py replay the same grids against the
restatements. Nothing of the reference's source is copied.
"""
from __future__ import annotations

import ast
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


class Meta:
    """Stand-in for onnxruntime's NodeArg: the three attributes ORT_IO reads."""
    def __init__(self, name, shape, type_):
        self.name, self.shape, self.type = name, shape, type_


ORT_IO_METAS = [Meta("a", [1, 1, "L"], "tensor(float)"), Meta("b", ["batch", 20, 64, "hist"], "tensor(float16)"),
                Meta("c", [1], "tensor(int64)"), Meta("d", [], "tensor(int32)")]


def ort_io_cases():
    """(meta, axes, value) of every array_for call, in order; value draws come from one seeded generator."""
    rng = np.random.default_rng(0)
    for m in ORT_IO_METAS:
        for axes in (None, {0: 2}, {0: 1, 1: 1, 2: 4, 3: 0}):
            for val in (rng.standard_normal(4), np.zeros((2, 20, 64, 3)), 5):
                yield m, axes, val


SCALAR_VALUE = 3


def repeat_cases():
    """(ids, threshold, ids_len) of every remove_repeated_parts call: short runs over a 4-symbol alphabet so repeats are common."""
    rng = np.random.default_rng(0)
    for _ in range(200):
        ids = rng.integers(0, 4, size=int(rng.integers(0, 14))).tolist()
        yield ids, 3, len(ids)


def gen_ort_io(ref_root):
    spec = importlib.util.spec_from_file_location("ref_ort_io", os.path.join(ref_root, "ORT_IO.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for i, (m, axes, val) in enumerate(ort_io_cases()):
        try:
            out[f"array_{i}"] = ref.array_for(m, val, axes=axes)
        except Exception as e:          # noqa: BLE001 -- the exception type IS the expected output
            assert type(e).__module__ == "builtins", type(e)
            out[f"array_{i}_raises"] = np.str_(type(e).__name__)
    for j, m in enumerate(ORT_IO_METAS):
        out[f"scalar_{j}"] = ref.scalar_for(m, SCALAR_VALUE)
    np.savez_compressed(os.path.join(GOLDEN, "ort_io_reference.npz"), **out)
    print("ort_io_reference:", len(out), "entries")


def gen_whisper_repeats(ref_root):
    src = open(os.path.join(ref_root, "Whisper", "Inference_Whisper_ONNX.py"), encoding="utf-8").read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "remove_repeated_parts"][0]
    ns = {}
    exec(compile(ast.Module([fn], []), "ref", "exec"), ns)
    outs = [list(ns["remove_repeated_parts"](ids, thr, n)) for ids, thr, n in repeat_cases()]
    np.savez_compressed(os.path.join(GOLDEN, "whisper_repeats_reference.npz"),
                        lengths=np.array([len(o) for o in outs], np.int32),
                        ids=np.array([t for o in outs for t in o], np.int32))
    print("whisper_repeats_reference:", len(outs), "cases")


if __name__ == "__main__":
    from oracle.reference_harness import REFERENCE_ROOT, reference_available
    assert reference_available(), f"the reference is not at {REFERENCE_ROOT}"
    os.makedirs(GOLDEN, exist_ok=True)
    gen_ort_io(REFERENCE_ROOT)
    gen_whisper_repeats(REFERENCE_ROOT)
