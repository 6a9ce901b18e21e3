"""The layout arithmetic behind every plan blob (csrc/plan_layout.h), checked by a stand-alone C++ program under AddressSanitizer + UBSan: for the section
lists of the four call sites, every section is aligned, in bounds and behind its predecessor, the total is sections + padding, and the offsets are those of
the hand-written layouts the sites had before (tests/cpp/plan_layout_check.cpp spells them out). The same program takes csrc/result_layout.h, the result
blob of the SenseVoice / Paraformer session, through every form: sections 4-byte aligned, pairwise disjoint, in bounds, at the offsets the session computed
by hand before, the total equal to what the pinned buffer is reserved for. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "automatic-speech-recognition-asr-onnx_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "plan_layout_check.cpp")


def _compiler():
    """(compiler, flags that link the sanitizer runtimes statically): clang links them so by default, g++ has to be told"""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if os.path.isfile(clang):
        return clang, []
    gxx = shutil.which("g++")
    return (gxx, ["-static-libasan", "-static-libubsan"]) if gxx else (None, [])


def test_plan_layout_matches_the_hand_layouts(tmp_path):
    cxx, extra = _compiler()
    if cxx is None:
        pytest.fail("no C++ compiler (ROCm clang++ or g++) to build the layout check with")
    exe = str(tmp_path / "plan_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *extra,
                            "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan layout ok" in run.stdout
