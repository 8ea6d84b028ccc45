"""bench.py's plain line and --dump-outputs on the device: a run without --full prints the contract's keys and does none of
the extra work (no oracle check, no CPU baseline, no verbose file), and what it dumps is what the same arguments dump under
--full, where the last step is also verified against the float32 oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_what_the_verified_full_run_dumps(tmp_path):
    common = ["--gpus", "1", "--chunks", "16", "--steps", "3", "--warmup", "1"]
    plain = _bench(*common, "--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["unit"] == "MS/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and plain["metric"].startswith("complex IQ MS/s")
    assert "verified_ranks" not in plain and plain["cpu_baseline"] is None and plain["full"] is None
    full = _bench(*common, "--full", "--no-cpu-baseline", "--no-host-fed", "--dump-outputs", str(tmp_path / "full"), "--full-line")
    assert full["verified_ranks"] == 1 and full["verify_worst_rel"] <= 1e-5
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert set(a) == set(b) and {"psd", "psd_frames", "chunks"} | {f"rx{r}_{k}" for r in range(4) for k in ("audio", "iq", "counts", "peak")} == set(a)
    assert sum(os.path.getsize(tmp_path / "plain" / f) for f in os.listdir(tmp_path / "plain")) <= 64 * 10 ** 6
    assert np.array_equal(a["chunks"], np.arange(16)) and a["psd"].shape[1] == 65536
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].shape == b[k].shape, k
        scale = max(float(np.max(np.abs(b[k]))), 1e-30)
        assert float(np.max(np.abs(a[k].astype(np.float64) - b[k]))) <= 1e-6 * scale, k
    for r in range(4):
        assert a[f"rx{r}_counts"].sum() == len(a[f"rx{r}_audio"]) == len(a[f"rx{r}_iq"])
