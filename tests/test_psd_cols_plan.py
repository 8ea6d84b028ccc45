"""The grid plan of the PSD columns loop (pysdr_amd/csrc/host_plan.h plan_psd_cols) and the frame walk the kernel steps with
(psd_cols_geom.h), in a stand-alone C++ program (tests/psd_cols_plan/plan_main.cpp) built with AddressSanitizer + UBSan and
run here.  CPU only; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_workgroup_walks_its_frames_once_and_touches_no_other(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "psd_cols_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "tests", "host_san", "fake_hip"), "-I" + os.path.join(ROOT, "pysdr_amd", "csrc"),
           os.path.join(ROOT, "tests", "psd_cols_plan", "plan_main.cpp"), "-o", exe]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and ("cannot find -lasan" in p.stderr or "cannot find -lubsan" in p.stderr):
        pytest.skip("sanitizer runtime not usable here: " + p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    if p.returncode != 0 and "unexpected memory mapping" in p.stderr:
        pytest.skip("sanitizer runtime not usable here: " + p.stderr[-200:])
    assert p.returncode == 0 and "PSD_COLS_PLAN_OK" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])
