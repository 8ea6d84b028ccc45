"""Generate tests/golden/ft_py_trace.json: the C calls the Python layer of the FT8 and FT4 skimmers makes, and what its methods
return, in the scenarios of tests/test_ft_py_trace.py with tests/fake_pysdr_lib.py in place of the library.  The file was
recorded with the Python layer as it stood while ``ft8.py`` held both modes' bank and skimmer and ``ft4.py`` inherited them;
record it again only when a call is meant to change.  Refuses to write a trace that misses a handle call, a decoded and an
undecoded record, a reported record or a record of the second pass.  Needs the built library (for the plan functions), no device.

    python tests/golden/make_ft_py_trace_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pysdr_amd import _lib                      # noqa: E402
from tests import test_ft_py_trace as t          # noqa: E402


def missing(out):
    """what the trace lacks, as a list of sentences"""
    lines = [ln for tr in out.values() for ln in tr]
    lack = [f"no call of pysdr_{k}_{what}" for k in t.MODES for what in t.HANDLE_CALLS
            if not any(ln.startswith(f"pysdr_{k}_{what} ") for ln in lines)]
    first = [r for r in t.RECORDS if r.get("pass", 1) == 1 and "ok" in r]
    if not any(r["ok"] for r in first):
        lack.append("no record of pass 1 with ok")
    if all(r["ok"] for r in first):
        lack.append("no record of pass 1 without ok")
    if not any(r.get("snr") is not None for r in t.RECORDS):
        lack.append("no record with the report's keys filled")
    if not any(r.get("pass") == 2 for r in t.RECORDS):
        lack.append("no record of pass 2")
    return lack


def main():
    real, real_lib, real_require = _lib.lib(), _lib.lib, _lib.require_gpu

    def install(fake):
        _lib.lib = lambda: fake
        _lib.require_gpu = lambda: None

    try:
        out = t.record(real, install)
    finally:
        _lib.lib, _lib.require_gpu = real_lib, real_require
    lack = missing(out)
    if lack:
        sys.exit("not written: " + "; ".join(lack))
    with open(t.GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(t.GOLDEN, {k: len(v) for k, v in out.items()}, os.path.getsize(t.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
