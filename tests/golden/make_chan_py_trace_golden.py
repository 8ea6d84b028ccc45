"""Generate tests/golden/chan_py_trace.json: the C calls the Python layer of the channelizer family makes, and what its
methods return, in the scenarios of tests/test_chan_py_trace.py with tests/fake_pysdr_lib.py in place of the library.  The
file was recorded with the Python layer as it stood before Channelizer / FineChannelizer, the CW / PSK decoder banks and the
two skimmers were put on shared cores; record it again only when a call is meant to change.  Needs the built library (for
the plan functions), no device.

    python tests/golden/make_chan_py_trace_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pysdr_amd import _lib                      # noqa: E402
from tests import test_chan_py_trace as t        # noqa: E402


def main():
    real, real_lib, real_require = _lib.lib(), _lib.lib, _lib.require_gpu

    def install(fake):
        _lib.lib = lambda: fake
        _lib.require_gpu = lambda: None

    try:
        out = t.record(real, install)
    finally:
        _lib.lib, _lib.require_gpu = real_lib, real_require
    with open(t.GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(t.GOLDEN, {k: len(v) for k, v in out.items()}, os.path.getsize(t.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
