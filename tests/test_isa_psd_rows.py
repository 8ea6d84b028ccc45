"""Build-time check on the ISA of the PSD rows loop (psdfft.hip psd_rows_pk_kernel; CPU: hipcc cross-compiles for gfx950): the
loop keeps the next frame's 16 HI and 16 LO words in registers on top of what a unit needs.  The 72 KB of LDS of a workgroup
allow two workgroups of eight waves on a CU, four waves per SIMD, and a SIMD's 512 registers per lane hold four waves only
up to 128 each -- so the kernel must stay at or below 128 vector registers, and must not touch private memory.  The block
scales travel the scalar path: 16 scalar loads per prefetch (prologue and loop), and no vector load of the loop is the
compiler's own -- every one comes from the prefetch's asm statements, whose completion the kernel counts by hand."""
import os
import re

import pytest

from tests.test_isa_checks import HIPCC, _isa


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_psd_rows_loop_has_no_scratch_keeps_four_waves_per_simd_and_loads_its_scales_as_scalars():
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
    mine = [k for k in meta if re.search(r"\d+psd_rows_pk_kernelE", k)]
    assert len(mine) == 1, sorted(meta)
    k = meta[mine[0]]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    inside, body = False, []
    for ln in lines:
        code = ln.split(";")[0].strip()
        if code == mine[0] + ":":
            inside = True
        elif inside and code.startswith(".Lfunc_end"):
            break
        elif inside and code:
            body.append(code)
    assert body and not [c for c in body if c.startswith("scratch_")]
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, k
    # prologue + loop: 2 x (16 HI dwords + 16 LO halfwords + 16 scales), nothing else read from global memory by vector loads
    count = lambda op: sum(1 for c in body if c.split()[0] == op)
    assert count("global_load_dword") == 32 and count("global_load_ushort") == 32, (count("global_load_dword"), count("global_load_ushort"))
    assert sum(1 for c in body if re.match(r"(global|flat|buffer)_load", c)) == 64
    assert sum(1 for c in body if re.match(r"s_load_dword\s+s\d+, s\[\d+:\d+\], 0x[0-9a-f]0$", c)) == 32
    assert count("s_barrier") == 3, count("s_barrier")          # the table's, and two per frame
