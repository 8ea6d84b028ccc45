"""The grid plan of the PSD columns loop (pysdr_amd/csrc/host_plan.h plan_psd_cols) and the frame walk the kernel steps with
(psd_cols_geom.h), in a stand-alone C++ program (tests/psd_cols_plan/plan_main.cpp) built and run by tests/plan_program.py,
under AddressSanitizer + UBSan where they are usable.  CPU only; nothing is loaded into Python."""
from tests import plan_program


def test_every_workgroup_walks_its_frames_once_and_touches_no_other(tmp_path):
    plan_program.run("tests/psd_cols_plan/plan_main.cpp", "PSD_COLS_PLAN_OK", tmp_path)
