"""SURVEY.md 5 "sanitizers on the CPU build": the HOST half of libpysdr_hip.so -- pysdr_amd/csrc/api.hip
(context / receiver bookkeeping, tile geometry handed to the mix + decimate kernel, PLL plans, the setter
snapshot, the ingest ring's slot state machine, the spectrum object), api_objects.hip (waterfall, RTTY decoder
bank, channelizer, channel bank in its five modes: ring wraparound, row pitches, strided copies, lazy staging), api_cw.hip
and api_psk.hip (the two skimmers that borrow a channelizer, with chan_client.h, the core they share with the bank: event
caps and pitches, the history room in front of a row, half-built objects) and api_fine.hip (the fine channelizer behind the
same handle: the row buffer of its first stage, the roll) compiled as plain C++ over a fake
HIP runtime whose "device" memory is the host heap, with a launch layer that touches exactly what each
kernel may touch and re-walks every mixdec tile with the kernel's own geometry code
(pysdr_amd/csrc/mixdec_geom.h) -- built and run under AddressSanitizer + UBSan, and the RX-thread-vs-Qt-
thread scenario under ThreadSanitizer.  CPU only; no GPU sanitizer exists on this pool.

Seeded-bug check done when the harness was written: halving the d_am allocation is reported by ASan in
launch_apply (IQ mode writes 2 floats per output), removing the lock of apply_pending by TSan.  Repeated when the
channelizer's clients came under the harness: halving the CW skimmer's d_events is reported by ASan in launch_cw_decode,
dropping kPskHpad from the PSK31 skimmer's row pointer in launch_psk_decode."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "tests", "host_san", "run.sh")


def _run(which, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    env = dict(os.environ, HOST_SAN_OUT=str(tmp_path))
    p = subprocess.run(["bash", RUN, which], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0 and ("cannot find -lasan" in p.stderr or "cannot find -ltsan" in p.stderr or "unexpected memory mapping" in p.stderr):
        pytest.skip("sanitizer runtime not usable here: " + p.stderr[-200:])
    assert p.returncode == 0 and "HOST_SAN_ALL_OK" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])
    return p.stdout


def test_host_half_and_mixdec_plans_under_address_and_ub_sanitizers(tmp_path):
    """The launch layer checks every mix + decimate launch against the library's own plan header
    (pysdr_amd/csrc/mixdec_plan.h); the driver also sweeps the planner over every shape, tile override and thread count."""
    out = _run("asan", tmp_path)
    assert "HOST_SAN_OK" in out and "HOST_SAN_RACE_OK" in out
    assert "planner sweep: 1920 plans" in out
    assert "pll plan sweep:" in out
    assert "stream objects: 432 calls" in out
    assert "channelizer clients: 195 skimmer calls, 98 fine calls, 324 sideband bank calls" in out
    assert "HOST_SAN_ALLOCFAIL_OK" in out


def test_setters_against_process_under_thread_sanitizer_over_the_shared_plan(tmp_path):
    assert "HOST_SAN_RACE_OK" in _run("tsan", tmp_path)
