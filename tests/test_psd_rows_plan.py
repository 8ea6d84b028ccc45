"""The grid plan of the PSD rows loop (pysdr_amd/csrc/host_plan.h plan_psd_rows), the frame walk the kernel steps with
(psd_rows_geom.h) and the rows part of PYSDR_PSD_PATH, in a stand-alone C++ program (tests/psd_rows_plan/plan_main.cpp) built
and run by tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.  CPU only; nothing is loaded into
Python."""
import pytest

from tests import plan_program

SOURCE, OK = "tests/psd_rows_plan/plan_main.cpp", "PSD_ROWS_PLAN_OK"


def test_every_workgroup_walks_its_frames_once_and_touches_no_other(tmp_path):
    plan_program.run(SOURCE, OK, tmp_path, extra_flags=["-O2"])


def test_a_seeded_off_by_one_in_has_next_is_caught(tmp_path, capsys):
    """`<=` for `<` in has_next: the workgroup that holds the last frame prefetches frame nframes -- the same program must fail"""
    with pytest.raises(AssertionError) as failure:
        plan_program.run(SOURCE, OK, tmp_path, extra_flags=["-DPSD_ROWS_SEED_DEFECT"])
    assert "prefetch of frame" in str(failure.value) and OK not in capsys.readouterr().out
