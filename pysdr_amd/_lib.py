"""ctypes binding of libpysdr_hip.so (include/pysdr_hip.h).

There is NO CPU fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# the diagnostic build (work-skipping ablation switches compiled in) is a different file and is
# only ever loaded on explicit request
# ... and so is an A/B variant (python -m pysdr_amd.build --variant NAME): only under the tuning master switch
_variant = os.environ.get("PYSDR_LIB_VARIANT", "") if os.environ.get("PYSDR_TUNING", "0") not in ("", "0") else ""
LIB_PATH = os.path.join(HERE, "libpysdr_hip_diag.so" if os.environ.get("PYSDR_USE_DIAG_LIB") == "1"
                        else (f"libpysdr_hip_{_variant}.so" if _variant else "libpysdr_hip.so"))

MAX_RX = 8


class PysdrError(RuntimeError):
    pass


class Cfg(C.Structure):
    _fields_ = [("srate", C.c_double), ("up", C.c_int32), ("down", C.c_int32),
                ("in_chunk", C.c_int32), ("max_chunks", C.c_int32),
                ("ntaps_dec", C.c_int32), ("ntaps_af", C.c_int32),
                ("device", C.c_int32), ("reserved", C.c_int32)]


class AgcState(C.Structure):
    _fields_ = [("agc", C.c_float), ("gain", C.c_float), ("maxbuf", C.c_float),
                ("ref", C.c_float), ("err", C.c_float)]


class Out(C.Structure):
    _fields_ = [("am", C.POINTER(C.c_float)), ("iq", C.POINTER(C.c_float)),
                ("cap", C.c_int32), ("n_out", C.c_int32),
                ("am_is_complex", C.c_int32), ("peak_in", C.c_float)]


class CwCfg(C.Structure):
    _fields_ = [("a_s", C.c_float), ("a_p", C.c_float), ("a_n", C.c_float),
                ("snr_min", C.c_float), ("hi", C.c_float), ("lo", C.c_float), ("fl", C.c_float),
                ("d0", C.c_int32), ("dmin", C.c_int32), ("dmax", C.c_int32), ("n0", C.c_int32)]


class PskCfg(C.Structure):
    _fields_ = [("a_t", C.c_float), ("a_q", C.c_float), ("hi", C.c_float), ("lo", C.c_float), ("hy", C.c_float),
                ("pmax", C.c_float), ("n0", C.c_int32)]


class Ft8Cfg(C.Structure):
    _fields_ = [("smin", C.c_float), ("hmin", C.c_int32), ("pmax", C.c_float)]


class Ft4Cfg(C.Structure):
    _fields_ = [("smin", C.c_float), ("hmin", C.c_int32), ("pmax", C.c_float)]


class LdpcCfg(C.Structure):
    _fields_ = [("iters", C.c_int32), ("alpha", C.c_float)]


class OsdCfg(C.Structure):
    _fields_ = [("order", C.c_int32)]


class ApCfg(C.Structure):
    _fields_ = [("mag", C.c_float), ("nerr_max", C.c_int32)]


class PassCfg(C.Structure):
    _fields_ = [("reach_t", C.c_int32), ("trials", C.c_int32), ("pulse", C.POINTER(C.c_uint32)), ("lut", C.POINTER(C.c_float))]


class FskCfg(C.Structure):
    _fields_ = [("a_q", C.c_float), ("a_b", C.c_float), ("hi", C.c_float), ("lo", C.c_float), ("bal", C.c_float),
                ("pmax", C.c_float), ("n0", C.c_int32)]


class PktCfg(C.Structure):
    _fields_ = [("gain", C.c_float * 8), ("pmax", C.c_float), ("w_mark", C.c_uint32), ("w_space", C.c_uint32),
                ("w_baud", C.c_uint32), ("pll_shift", C.c_int32)]


class SstvMode(C.Structure):
    _fields_ = [("code", C.c_int32), ("scans", C.c_int32), ("width", C.c_int32), ("lines", C.c_int32), ("sync_q", C.c_uint32),
                ("porch_q", C.c_uint32), ("scan_q", C.c_uint32), ("sep_q", C.c_uint32)]


class SstvCfg(C.Structure):
    _fields_ = [("det", C.c_int32), ("nmodes", C.c_int32), ("w_sub", C.c_uint32), ("w_tick", C.c_uint32), ("k_hz", C.c_float),
                ("k_rho", C.c_float), ("pmax", C.c_float), ("W", C.c_int32), ("R0", C.c_int32), ("lag", C.c_int32), ("modes", SstvMode * 16)]


class RdsCfg(C.Structure):
    _fields_ = [("w19", C.c_uint32)]


class AcarsCfg(C.Structure):
    _fields_ = [("pmax", C.c_float), ("w_car", C.c_uint32), ("w_baud", C.c_uint32), ("pll_shift", C.c_int32)]


_vp, _i, _sz, _d, _f, _u32 =C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_float, C.c_uint32
_pd, _pf, _pi = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
_ll, _pll, _p32, _pu8 = C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
_cands = [_p32, _pll, _i]                                               # FT8 / FT4: candidates (F, t0, n) ...
_decoded = [C.POINTER(LdpcCfg), _p32, _pu8, _pf]                        # ... the decoder's cfg, status, bits and post ...
_osd = [C.POINTER(OsdCfg), _p32]                                        # ... and the second stage's cfg and detail
# a-priori decoding: the table (hyps, H), the pairs (pairs, P), both cfgs, ap, bits and detail
_ap = [_pu8, _i, _p32, _i, C.POINTER(LdpcCfg), C.POINTER(ApCfg), _p32, _pu8, _p32]

# name -> (restype, argtypes); every symbol include/pysdr_hip.h declares
PROTOTYPES = {
    "pysdr_strerror": (C.c_char_p, [_i]),
    "pysdr_last_error": (C.c_char_p, []),
    "pysdr_device_count": (_i, [_pi]),
    "pysdr_version": (_i, []),
    "pysdr_create": (_i, [C.POINTER(Cfg), C.POINTER(_vp)]),
    "pysdr_destroy": (None, [_vp]),
    "pysdr_rx_add": (_i, [_vp, _i, _d, _pd, _pd, _d, _pi]),
    "pysdr_set_lo": (_i, [_vp, _i, _d, _pd]),
    "pysdr_set_dec_taps": (_i, [_vp, _i, _pd, _i]),
    "pysdr_set_mode": (_i, [_vp, _i, _i, _pd, _i, _d]),
    "pysdr_wfm_params": (_i, [_d, _d, _pi, _pi, _pi]),
    "pysdr_set_wfm_taps": (_i, [_vp, _i, _pd, _i, _pd, _i]),
    "pysdr_reset": (_i, [_vp, _i, C.c_uint]),
    "pysdr_agc_get": (_i, [_vp, _i, C.POINTER(AgcState)]),
    "pysdr_pll_stats": (_i, [_vp, _i, _pi, _pi]),
    "pysdr_set_pll_segments": (_i, [_vp, _i]),
    "pysdr_build_flags_hash": (_i, []),
    "pysdr_set_overlap": (_i, [_vp, _i]),
    "pysdr_get_overlap": (_i, [_vp]),
    "pysdr_last_call_overlapped": (_i, [_vp]),
    "pysdr_pll_join_margin": (_i, [_vp, _i, _pi, _pf]),
    "pysdr_pll_linear_starts": (_i, [_vp, _i, _pi]),
    "pysdr_set_agc": (_i, [_vp, _i, _i, _f]),
    "pysdr_set_squelch": (_i, [_vp, _i, _f]),
    "pysdr_squelch_get": (_i, [_vp, _i, _pf, _pi]),
    "pysdr_set_squelch_ratio": (_i, [_vp, _i, _f, _pf, _pf, _i]),
    "pysdr_squelch_ratio_get": (_i, [_vp, _i, _pf, _pf, _pi]),
    "pysdr_process": (_i, [_vp, _pf, _sz, C.POINTER(Out)]),
    "pysdr_process_batch": (_i, [_vp, _vp, _i, _sz, _i]),
    "pysdr_fetch": (_i, [_vp, _i, _pf, _pf, _i, _pi, _pi, _pi, _pf]),
    "pysdr_sync": (_i, [_vp]),
    "pysdr_set_profile": (_i, [_vp, _i]),
    "pysdr_get_elapsed_ms": (_i, [_vp, _i, _i, _pf]),
    "pysdr_set_tile": (_i, [_vp, _i, _i]),
    "pysdr_get_tuning": (_i, [_vp, _p32]),
    "pysdr_front_end_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p32]),
    "pysdr_front_end_shapes": (_i, [_i, _i, _p32, _pi]),
    "pysdr_resamp_plan": (_i, [_i, _i, _i, _i, _p32]),
    "pysdr_get_resamp_tuning": (_i, [_vp, _p32]),
    "pysdr_quad_mixer": (_i, [_i, _pf, _pf, _sz, _u32, _u32, C.POINTER(_u32)]),
    "pysdr_freq_word": (_u32, [_d, _d, _pd]),
    "pysdr_fir_real": (_i, [_i, _pf, _pf, _i, _pf, _sz]),
    "pysdr_spectrum_create": (_i, [_i, _i, _i, _i, _pf, C.POINTER(_vp)]),
    "pysdr_spectrum_destroy": (None, [_vp]),
    "pysdr_spectrum_frame": (_i, [_vp, _pf, _i, _i, _pf, _pi]),
    "pysdr_spectrum_batch": (_i, [_vp, _vp, _i, _sz, _vp]),
    "pysdr_spectrum_sync": (_i, [_vp]),
    "pysdr_spectrum_get_tuning": (_i, [_vp, _p32]),
    "pysdr_spectrum_elapsed_ms": (_i, [_vp, _pf]),
    "pysdr_spectrum_order": (_i, [_vp, _vp, _i]),
    "pysdr_ingest_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "pysdr_ingest_create_batched": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "pysdr_ingest_chunks": (_i, [_vp, _i, _i, _pi, _pi, _pf]),
    "pysdr_ingest_destroy": (None, [_vp]),
    "pysdr_ingest_buffer": (_i, [_vp, _i, C.POINTER(_pf), C.POINTER(C.c_size_t)]),
    "pysdr_ingest_submit": (_i, [_vp, _i, C.c_size_t]),
    "pysdr_ingest_collect": (_i, [_vp, _i, C.POINTER(Out)]),
    "pysdr_waterfall_create": (_i, [_i, _i, _i, C.POINTER(_vp)]),
    "pysdr_waterfall_destroy": (None, [_vp]),
    "pysdr_waterfall_push": (_i, [_vp, _vp, _i, _i]),
    "pysdr_waterfall_roll": (_i, [_vp, _i]),
    "pysdr_waterfall_image": (_i, [_vp, _f, _pf, _pf, _pf]),
    "pysdr_waterfall_image_rows": (_i, [_vp, _f, _i, _pf, _pf, _pf]),
    "pysdr_waterfall_peaks": (_i, [_vp, _pf, _i, C.c_double, _i, _p32, _i, _p32]),
    "pysdr_rtty_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "pysdr_rtty_destroy": (None, [_vp]),
    "pysdr_rtty_reset": (_i, [_vp]),
    "pysdr_rtty_decode": (_i, [_vp, _vp, _i, _i, _i, _pi, _pll, _pd, _pi, _pi, _pi, _pf]),
    "pysdr_chan_plan": (_i, [_i, _i, _i, _i, _i, _p32]),
    "pysdr_chan_create": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "pysdr_chan_destroy": (None, [_vp]),
    "pysdr_chan_set_taps": (_i, [_vp, _pd, _i]),
    "pysdr_chan_reset": (_i, [_vp]),
    "pysdr_chan_sync": (_i, [_vp]),
    "pysdr_chan_process": (_i, [_vp, _vp, _i, _i, _vp, _ll, _i, _pi]),
    "pysdr_chan_fine_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _p32]),
    "pysdr_chan_fine_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "pysdr_chan_fine_set_taps": (_i, [_vp, _pd, _i, _pd, _i]),
    "pysdr_bank_plan": (_i, [_i, _i, _i, _p32]),
    "pysdr_bank_create": (_i, [_vp, _d, _i, _i, C.POINTER(_vp)]),
    "pysdr_bank_destroy": (None, [_vp]),
    "pysdr_bank_set_mode": (_i, [_vp, _i, _pd, _i]),
    "pysdr_bank_set_mode_cplx": (_i, [_vp, _i, _pd, _pd, _i, _d]),
    "pysdr_bank_set_agc": (_i, [_vp, _i, _f]),
    "pysdr_bank_set_squelch": (_i, [_vp, _f]),
    "pysdr_bank_reset": (_i, [_vp]),
    "pysdr_bank_process": (_i, [_vp, _vp, _i, _i, _vp, _ll, _i, _pi]),
    "pysdr_bank_state": (_i, [_vp, _pf, _pf, _pf, _pf, _pu8]),
    "pysdr_bank_fetch": (_i, [_vp, _pi, _i, _pf, _pf, _ll]),
    "pysdr_bank_sync": (_i, [_vp]),
    "pysdr_cw_plan": (_i, [_i, _i, C.POINTER(CwCfg), _p32]),
    "pysdr_cw_create": (_i, [_vp, C.POINTER(CwCfg), _i, C.POINTER(_vp)]),
    "pysdr_cw_destroy": (None, [_vp]),
    "pysdr_cw_reset": (_i, [_vp]),
    "pysdr_cw_sync": (_i, [_vp]),
    "pysdr_cw_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll]),
    "pysdr_cw_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_cw_state": (_i, [_vp, _pf, _pf, _pf, _p32]),
    "pysdr_psk_plan": (_i, [_i, _i, _i, C.POINTER(PskCfg), _p32]),
    "pysdr_psk_create": (_i, [_vp, _i, C.POINTER(PskCfg), _pf, _pf, _i, C.POINTER(_vp)]),
    "pysdr_psk_destroy": (None, [_vp]),
    "pysdr_psk_reset": (_i, [_vp]),
    "pysdr_psk_sync": (_i, [_vp]),
    "pysdr_psk_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll, _pf, _p32]),
    "pysdr_psk_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_psk_state": (_i, [_vp, _pf, _pf, _p32]),
    "pysdr_fsk_plan": (_i, [_i, _i, _i, C.POINTER(FskCfg), _p32]),
    "pysdr_fsk_create": (_i, [_vp, _i, C.POINTER(FskCfg), _pf, _pf, _i, C.POINTER(_vp)]),
    "pysdr_fsk_destroy": (None, [_vp]),
    "pysdr_fsk_reset": (_i, [_vp]),
    "pysdr_fsk_sync": (_i, [_vp]),
    "pysdr_fsk_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll, _pf, _p32]),
    "pysdr_fsk_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_fsk_state": (_i, [_vp, _pf, _p32]),
    "pysdr_pkt_plan": (_i, [_i, _i, _i, C.POINTER(PktCfg), _p32]),
    "pysdr_pkt_create": (_i, [_vp, _i, C.POINTER(PktCfg), _pf, _pf, _i, C.POINTER(_vp)]),
    "pysdr_pkt_destroy": (None, [_vp]),
    "pysdr_pkt_reset": (_i, [_vp]),
    "pysdr_pkt_sync": (_i, [_vp]),
    "pysdr_pkt_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll]),
    "pysdr_pkt_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_pkt_state": (_i, [_vp, _p32, C.POINTER(_u32)]),
    "pysdr_sstv_plan": (_i, [_i, _i, _i, C.POINTER(SstvCfg), _p32]),
    "pysdr_sstv_create": (_i, [_vp, _i, C.POINTER(SstvCfg), _pf, _pf, _i, C.POINTER(_vp)]),
    "pysdr_sstv_destroy": (None, [_vp]),
    "pysdr_sstv_reset": (_i, [_vp]),
    "pysdr_sstv_sync": (_i, [_vp]),
    "pysdr_sstv_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll]),
    "pysdr_sstv_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_sstv_state": (_i, [_vp, _p32, _pf, _pf, C.POINTER(_u32)]),
    "pysdr_rds_plan": (_i, [_i, _i, _i, C.POINTER(RdsCfg), _p32]),
    "pysdr_rds_create": (_i, [_vp, _i, C.POINTER(RdsCfg), _pf, _pf, _i, C.POINTER(_vp)]),
    "pysdr_rds_destroy": (None, [_vp]),
    "pysdr_rds_reset": (_i, [_vp]),
    "pysdr_rds_sync": (_i, [_vp]),
    "pysdr_rds_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll]),
    "pysdr_rds_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_rds_state": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32), _pf]),
    "pysdr_acars_plan": (_i, [_i, _i, _i, C.POINTER(AcarsCfg), _p32]),
    "pysdr_acars_create": (_i, [_vp, _i, C.POINTER(AcarsCfg), _pf, _pf, _i, C.POINTER(_vp)]),
    "pysdr_acars_destroy": (None, [_vp]),
    "pysdr_acars_reset": (_i, [_vp]),
    "pysdr_acars_sync": (_i, [_vp]),
    "pysdr_acars_process": (_i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll]),
    "pysdr_acars_fetch": (_i, [_vp, _pi, _i, _p32, _ll]),
    "pysdr_acars_state": (_i, [_vp, _p32, C.POINTER(_u32)]),
    "pysdr_ldpc_plan": (_i, [C.POINTER(LdpcCfg), _p32]),
    "pysdr_osd_plan": (_i, [C.POINTER(OsdCfg), _p32]),
    "pysdr_ap_plan": (_i, [C.POINTER(ApCfg), _p32]),
    "pysdr_report_plan": (_i, [_i, _p32]),
    "pysdr_pass_plan": (_i, [_i, _i, _i, _i, _i, _p32]),
    # the FT8 and the FT4 skimmer (ft.py): one set of entry points per mode, told apart by the name and the cfg struct
    **{f"pysdr_{k}_{what}": (res, args) for k, cfg in (("ft8", Ft8Cfg), ("ft4", Ft4Cfg)) for what, res, args in (
        ("plan", _i, [_i, _i, _i, C.POINTER(cfg), _p32]),
        ("create", _i, [_vp, _i, C.POINTER(cfg), _pf, _i, C.POINTER(_vp)]),
        ("destroy", None, [_vp]),
        ("reset", _i, [_vp]),
        ("sync", _i, [_vp]),
        ("process", _i, [_vp, _vp, _i, _i, _pi, _p32, _p32, _ll, _pll]),
        ("fetch", _i, [_vp, _pi, _i, _p32, _ll]),
        ("state", _i, [_vp, _pf, _p32, _pf, _pll]),
        ("llr", _i, [_vp] + _cands + [_pf]),
        ("decode", _i, [_vp] + _cands + _decoded),
        ("decode_osd", _i, [_vp] + _cands + _decoded + _osd),
        ("decode_llr", _i, [_vp, _pf, _i] + _decoded),
        ("decode_llr_osd", _i, [_vp, _pf, _i] + _decoded + _osd),
        ("decode_ap", _i, [_vp] + _cands + _ap),
        ("decode_llr_ap", _i, [_vp, _pf, _i] + _ap),
        ("report", _i, [_vp, _p32, _pll, _pu8, _i, _pf, _p32]),
        ("floor", _i, [_vp, _ll, _i, _pf]),
        ("keep", _i, [_vp, C.POINTER(PassCfg)]),
        ("subtract", _i, [_vp, _p32, _pll, _pu8, _p32, _i, _p32]),
        ("rescan", _i, [_vp, _i, _i, _ll, _ll, C.POINTER(cfg), _p32, _p32]),
        ("pass_decode", _i, [_vp] + _cands + _decoded + _osd),
        ("pass_llr", _i, [_vp] + _cands + [_pf]),
        ("pass_state", _i, [_vp, _pf, _pf, _pll]))},
    "pysdr_dev_alloc": (_i, [_i, _sz, C.POINTER(_vp)]),
    "pysdr_dev_free": (_i, [_i, _vp]),
    "pysdr_dev_upload": (_i, [_i, _vp, _vp, _sz]),
    "pysdr_dev_download": (_i, [_i, _vp, _vp, _sz]),
    "pysdr_dev_copy": (_i, [_i, _vp, _vp, _sz]),
    "pysdr_comm_unique_id": (_i, [C.c_char_p]),
    "pysdr_comm_init": (_i, [_vp, C.c_char_p, _i, _i]),
    "pysdr_comm_bcast": (_i, [_vp, _vp, _sz, _i]),
    "pysdr_comm_destroy": (_i, [_vp]),
}

_lib = None


def lib():
    """Load the HIP library (once).  Raises PysdrError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PysdrError(
                f"{LIB_PATH} not found: build it with `python -m pysdr_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:
            L = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)
        except OSError as e:
            raise PysdrError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        L = lib()
        msg = L.pysdr_strerror(rc).decode()
        detail = L.pysdr_last_error().decode()
        raise PysdrError(f"{what}: {msg} ({rc}) {detail}")


def plan_call(name, nwords, *args):
    """One ``pysdr_*_plan`` call (no device needed): ``args`` and an int32 array of ``nwords`` for the answer -> the words
    as a list.  Raises PysdrError outside the plan's rules."""
    out = (C.c_int32 * nwords)()
    check(getattr(lib(), name)(*args, out), name)
    return list(out)


class Handle:
    """One owned object of the C ABI: the library ``_L``, the handle ``_h`` (None before create and after close) and
    ``DESTROY``, the name of its ``pysdr_*_destroy``.  ``close()`` may be called any number of times; a class that owns
    more than the handle frees it in ``_release()``."""
    DESTROY = None
    _L = _h = None

    def _create(self, name, *args):
        """the object's create call: ``args`` and, last, where the handle goes"""
        self._L = lib()
        hd = C.c_void_p()
        check(getattr(self._L, name)(*args, C.byref(hd)), name)
        self._h = hd

    def _check_open(self):
        if self._h is None:
            raise PysdrError(f"{type(self).__name__} is closed")

    def close(self):
        if self._h:
            getattr(self._L, self.DESTROY)(self._h)
            self._h = None
        self._release()

    def _release(self):
        """what goes after the handle; runs on every close()"""

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be torn down: leave the device
        # memory to process exit rather than call into a dead runtime
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def device_count():
    n = C.c_int(0)
    rc = lib().pysdr_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def require_gpu():
    if device_count() < 1:
        raise PysdrError("no HIP device visible: pysdr_amd has no CPU path "
                         "(the NumPy oracle under oracle/ is test infrastructure only)")


def as_pd(a):
    return a.ctypes.data_as(_pd)


def as_pf(a):
    return a.ctypes.data_as(_pf)


def as_pi(a):
    return a.ctypes.data_as(_pi)
