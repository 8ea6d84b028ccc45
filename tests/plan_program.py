"""Build and run one of the stand-alone C++ plan programs (tests/*_plan/plan_main.cpp): under AddressSanitizer + UBSan where
their runtime is usable; where it is not (no libasan to link, or a host whose memory layout the runtime refuses) the same
program is built and run without them, and the output says which: the programs' own checks do not depend on the
sanitizers.  CPU only; nothing that is loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ("tests/host_san/fake_hip", "pysdr_amd/csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def run(source, ok_marker, tmp_path, extra_flags=(), includes=INCLUDES, args=()):
    """``source`` and ``includes`` are paths from the repository root, ``args`` the program's arguments.  -> the program's
    stdout, which holds ``ok_marker``"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    base = (["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
            + list(extra_flags) + ["-I" + os.path.join(ROOT, i) for i in includes] + [os.path.join(ROOT, source)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    stem = os.path.basename(os.path.dirname(source))
    for name, flags in (("sanitized", SANITIZE), ("plain", [])):
        exe = str(tmp_path / (stem + "_" + name))
        p = subprocess.run(base + flags + ["-o", exe], cwd=ROOT, capture_output=True, text=True, timeout=600)
        if p.returncode != 0 and flags and ("cannot find -lasan" in p.stderr or "cannot find -lubsan" in p.stderr):
            print("sanitizer runtime not linkable here, running the plain build:", p.stderr[-200:])
            continue
        assert p.returncode == 0, p.stderr[-3000:]
        p = subprocess.run([exe, *args], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
        if p.returncode != 0 and flags and "unexpected memory mapping" in p.stderr:
            print("sanitizer runtime not usable here, running the plain build:", p.stderr[-200:])
            continue
        assert p.returncode == 0 and ok_marker in p.stdout, (name, p.stdout[-1500:], p.stderr[-3000:])
        print(f"{source}: {name} build:", p.stdout.strip())
        return p.stdout
    raise AssertionError(f"{source}: neither the sanitized nor the plain build ran")
