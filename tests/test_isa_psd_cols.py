"""Build-time check on the ISA of the PSD columns loop (psdfft.hip psd_cols_pk_kernel; CPU: hipcc cross-compiles for gfx950):
the loop keeps the window, the four-step twiddles and the next frame's samples in registers on top of what a unit needs.
The 37 KB of LDS of a workgroup allow four workgroups of four waves on a CU, one wave of each per SIMD, and a SIMD's 512
registers per lane hold four waves only up to 128 each -- so the kernel must stay at or below 128 vector registers, and must
not touch private memory (a spilled register is a memory round trip on the chain the loop exists to shorten)."""
import os
import re

import pytest

from tests.test_isa_checks import HIPCC, _isa


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_psd_cols_loop_has_no_scratch_and_keeps_four_waves_per_simd():
    from pysdr_amd import build as pb
    lines = _isa("psdfft.hip", ["-fPIC", *pb.EXTRA_FLAGS.get("psdfft.hip", [])])
    meta, name = {}, None
    for ln in lines:
        m = re.search(r"\.name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"\.(private_segment_fixed_size|vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", ln)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    mine = [k for k in meta if re.search(r"\d+psd_cols_pk_kernelE", k)]
    assert len(mine) == 1, sorted(meta)
    k = meta[mine[0]]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    inside, scratch = False, []
    for ln in lines:
        code = ln.split(";")[0].strip()
        if code == mine[0] + ":":
            inside = True
        elif inside and code.startswith(".Lfunc_end"):
            break
        elif inside and code.startswith("scratch_"):
            scratch.append(code)
    assert inside and not scratch, scratch[:4]
    # 512 registers per lane and SIMD (vector + accumulation registers of one unified file), four waves
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, k
