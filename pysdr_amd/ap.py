"""A-priori decoding for the FT8 and FT4 decoder banks (kernels ``ap.hip``, pure half ``ap_plan.h``,
host half ``ap_host.h``): the LDPC decoder told some of the message's bits in advance, once per hypothesis, every
(candidate, hypothesis) pair a workgroup of its own.  Here: the settings, the hypotheses over ``ft8msg``, the two calls on a
bank, the policy that turns the calls heard on a frequency into hypotheses for the next slots (``History``, no device), and
``FT8_AP_Skimmer``, an ``FT8_Skimmer`` that sends the frames min-sum could not decode through both.  Off unless asked for.

A hypothesis is ``(mask, value)``, each uint8 [12]: message bit i is bit 7 - (i & 7) of byte i >> 3, only bits 0 .. 76 may be
set in the mask, and the value has no bit outside it.  The kinds:

    1  ``hyp_cq()``            CQ ? ?        29 + 3 bits
    2  ``hyp_from(call)``      ? call ?      32 bits
    3  ``hyp_pair(a, b)``      a b ?         61 bits
    4  ``hyp_cq_from(call)``   CQ call ?     61 bits
    5  ``hyp_text(text)``      the message   77 bits
"""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np

from . import _lib
from . import ft8msg as _msg
from . import ldpc as _ldpc
from ._lib import ApCfg
from .ft import FT_Skimmer, _cands
from .ft8 import FT8_Skimmer

HYP_MAX, PAIR_MAX, CAND_MAX = 4096, 65536, 4096     # of one call of the C ABI
MSG = 77
NERR_MAX = 174                                   # the default: off (DESIGN.md 3 item 28 says why)
KIND_CQ, KIND_FROM, KIND_PAIR, KIND_CQ_FROM, KIND_TEXT = 1, 2, 3, 4, 5
_p32, _pu8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
# the standard message's fields: the first call and its suffix bit, the second likewise, and the type
_FIRST, _SECOND, _I3 = slice(0, 29), slice(29, 58), slice(74, 77)


def params(mag=1.0, nerr_max=NERR_MAX):
    """The settings as the ``_lib.ApCfg`` the C ABI takes: a hypothesised bit enters the decoder as ``mag`` times the
    word's greatest |soft bit|; a pair is accepted with at most ``nerr_max`` hard errors outside its mask."""
    return ApCfg(mag=float(np.float32(mag)), nerr_max=int(nerr_max))


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in ApCfg._fields_}


def plan(cfg):
    """What one AP call launches (no device needed): dict of threads per pair, LDS bytes, pairs and hypotheses per call.
    Raises PysdrError for a cfg outside the rules (mag finite and in [0.25, 16], nerr_max in [0, 174])."""
    v = _lib.plan_call("pysdr_ap_plan", 4, C.byref(cfg) if cfg is not None else None)
    return {"threads": v[0], "lds_bytes": v[1], "max_pairs": v[2], "max_hyps": v[3]}


# ---- hypotheses ---------------------------------------------------------------------------------------------------------------
def _word(bits):
    b = np.zeros(96, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b)


def hyp_bits(mask77, value77):
    """77 mask bits and 77 value bits -> (mask, value) as the C ABI takes them; the value is kept under the mask only"""
    m = np.asarray(mask77, np.uint8).reshape(MSG) & 1
    if not m.any():
        raise ValueError("a hypothesis names at least one bit")
    return _word(m), _word(m & np.asarray(value77, np.uint8).reshape(MSG))


def _standard(first, second):
    """the bits of ``first second`` with a sign-off behind them, which only the fields outside the hypothesis hold"""
    if len(str(first).split()) != 1 or len(str(second).split()) != 1:
        raise ValueError(f"not two standard calls: {first!r} {second!r}")
    bits = _msg.pack77(f"{first} {second} 73")
    if _msg.types(bits)[0] not in (1, 2):
        raise ValueError(f"not two standard calls: {first!r} {second!r}")
    return bits


def _fields(bits, *fields):
    mask = np.zeros(MSG, np.uint8)
    for f in fields:
        mask[f] = 1
    return hyp_bits(mask, bits)


def hyp_cq():
    """``CQ ? ?``: the first call's field and the type, 29 + 3 bits"""
    return _fields(_standard("CQ", "K1ABC"), _FIRST, _I3)


def hyp_from(call):
    """``? call ?``: the second call's field and the type, 32 bits"""
    return _fields(_standard("CQ", call), _SECOND, _I3)


def hyp_pair(a, b):
    """``a b ?``: both calls' fields and the type, 61 bits"""
    return _fields(_standard(a, b), _FIRST, _SECOND, _I3)


def hyp_cq_from(call):
    """``CQ call ?``, 61 bits"""
    return hyp_pair("CQ", call)


def hyp_text(text):
    """every one of the 77 bits of ``ft8msg.pack77(text)``"""
    return hyp_bits(np.ones(MSG, np.uint8), _msg.pack77(text))


def table(hyps):
    """[(mask, value)] -> uint8 [H][24]"""
    out = np.zeros((len(hyps), 24), np.uint8)
    for h, (m, v) in enumerate(hyps):
        out[h, :12], out[h, 12:] = np.asarray(m, np.uint8).reshape(12), np.asarray(v, np.uint8).reshape(12)
    return out


# ---- the two calls on a bank --------------------------------------------------------------------------------------------------
def _chunks(n, pairs):
    """candidates [lo, hi) and their pairs [p_lo, p_hi) in calls of at most 4096 candidates and 65536 pairs"""
    at = np.searchsorted(pairs[:, 0], np.arange(n + 1), "left") if len(pairs) else np.zeros(n + 1, np.int64)
    out, lo = [], 0
    while lo < n:
        hi = min(n, lo + CAND_MAX)
        while hi > lo + 1 and at[hi] - at[lo] > PAIR_MAX:
            hi -= 1
        out.append((lo, hi, int(at[lo]), int(at[hi])))
        lo = hi
    return out


def _run(dec, what, n, head, pairs, hyps, cfg, ldpc, detail):
    cfg = params() if cfg is None else cfg
    ldpc = _ldpc.params() if ldpc is None else ldpc
    tab = table(hyps)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if len(pairs) > 1 and not ((np.diff(pairs[:, 0]) > 0) | ((np.diff(pairs[:, 0]) == 0) & (np.diff(pairs[:, 1]) > 0))).all():
        raise ValueError("pairs: strictly increasing in (candidate, hypothesis)")
    if len(pairs) and (pairs[:, 0].min() < 0 or pairs[:, 0].max() >= n):
        raise ValueError(f"pairs: a candidate outside [0, {n})")
    ap, bits = np.zeros((n, 4), np.int32), np.zeros((n, 12), np.uint8)
    de = np.zeros((len(pairs), 4), np.int32) if detail else None
    for lo, hi, p_lo, p_hi in _chunks(n, pairs):
        pp = pairs[p_lo:p_hi] - np.array([lo, 0], np.int32)
        dec._call(what, *head(slice(lo, hi)), hi - lo, tab.ctypes.data_as(_pu8), len(tab), pp.ctypes.data_as(_p32), len(pp), C.byref(ldpc),
                  C.byref(cfg), ap[lo:hi].ctypes.data_as(_p32), bits[lo:hi].ctypes.data_as(_pu8),
                  None if de is None or p_hi == p_lo else de[p_lo:p_hi].ctypes.data_as(_p32))
        ap[lo:hi, 0] += np.where(ap[lo:hi, 0] >= 0, p_lo, 0).astype(np.int32)
    pair = ap[:, 0].copy()
    out = dict(pair=pair, hyp=np.where(pair >= 0, pairs[np.maximum(pair, 0), 1] if len(pairs) else -1, -1).astype(np.int32),
               iterations=ap[:, 1].copy(), nerr=ap[:, 2].copy(), count=ap[:, 3].copy(), bits=_ldpc.unpack_bits(bits))
    if de is not None:
        out["detail"] = de
    return out


def decode(dec, F, t0, pairs, hyps, cfg=None, ldpc=None, detail=False):
    """The candidates (F[i], t0[i]) of ``dec.decode`` (an ``FT8_Decoders`` or ``FT4_Decoders`` bank), under its rules,
    from the first spectrum ring, each decoded once per pair (candidate, hypothesis) of ``pairs`` int32 [P][2] -- strictly
    increasing -- under the hypothesis ``hyps[hypothesis]`` = (mask, value).  ``cfg``: ``params()``; ``ldpc``: ``ldpc.params()``.
    -> dict of pair int32 [n] (the candidate's pair of status 2 with the least nerr, ties to the lower index; -1: none),
    hyp (that pair's hypothesis or -1), iterations, nerr (hard errors outside the mask), count (its pairs of status 2),
    bits uint8 [n][91] (zero behind a -1) and, with ``detail``, detail int32 [P][4] = (status, iterations, nerr, nap) of
    every pair.  In calls of at most 4096 candidates and 65536 pairs."""
    F, t0, at = _cands(F, t0)
    return _run(dec, "decode_ap", len(F), at, pairs, hyps, cfg, ldpc, detail)


def decode_llr(dec, llr, pairs, hyps, cfg=None, ldpc=None, detail=False):
    """``decode`` on soft bits from the host, float32 [n][174], positive for bit 1, any scale; a value that is not finite
    is refused."""
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, dec.MODE.BITS)
    return _run(dec, "decode_llr_ap", len(llr), lambda s: (_lib.as_pf(llr[s]),), pairs, hyps, cfg, ldpc, detail)


# ---- what was heard, and what to expect ---------------------------------------------------------------------------------------
def calls_of(text):
    """the text of a standard message -> (first call or None where a CQ, DE or QRZ stands in its place, second call, whether
    it is a plain CQ), or None for anything else"""
    if not text:
        return None
    tokens = str(text).upper().split()
    try:
        if _msg.types(_msg.pack77(text))[0] not in (1, 2) or len(tokens) < 2:
            return None
    except ValueError:
        return None
    c1, used = _msg._pack_first(tokens)
    if c1 is None:
        return tokens[0], tokens[1], False
    return None, tokens[used], c1 == 2


class History:
    """Pure policy, no device: which hypotheses a frame that failed at fine row ``F`` and step ``t0`` is worth, from the
    frames decoded near that row in the slots before.  ``note(rec)`` remembers (t0, F, first call, second call) of an
    ``ok`` record whose text is a standard two-call or CQ message.  ``hypotheses(F, t0)`` -> [(kind, (mask, value))], at
    most 8: ``CQ ? ?`` always; then, the newest remembered frame first, for every frame within ``reach_f`` fine rows whose
    t0 lies within ``reach_t`` steps of a whole number of slots (``step_slot`` steps each) back -- an even number, the same
    sender again: ``? B ?``, ``A B ?`` and, if it was a CQ, ``CQ B ?`` and the CQ's own text, which comes back bit for
    bit; an odd number, the partner answering on the same frequency: ``B A ?``.  A frame more than ``hold`` slot pairs back
    is forgotten.  All in absolute steps: nothing depends on how the stream is cut."""
    CAP = 8

    def __init__(self, reach_f=2, hold=4, step_slot=375, reach_t=8):
        self.reach_f, self.hold, self.step_slot, self.reach_t = int(reach_f), int(hold), int(step_slot), int(reach_t)
        self.heard = []                                                  # (t0, F, A, B, cq, text), in the order noted

    def _age_max(self):
        return 2 * self.hold * self.step_slot + self.reach_t

    def note(self, rec):
        """-> whether the record was remembered"""
        if not rec.get("ok"):
            return False
        got = calls_of(rec.get("text"))
        if got is None:
            return False
        entry = (int(rec["t0"]), int(rec["F"]), got[0], got[1], got[2], " ".join(str(rec["text"]).upper().split()))
        if entry not in self.heard:
            self.heard.append(entry)
        newest = max(e[0] for e in self.heard)
        self.heard = [e for e in self.heard if newest - e[0] <= self._age_max()]
        return True

    def hypotheses(self, F, t0):
        out, seen = [], set()

        def offer(kind, h):
            key = (h[0].tobytes(), h[1].tobytes())
            if key not in seen and len(out) < self.CAP:
                seen.add(key)
                out.append((kind, h))

        offer(KIND_CQ, hyp_cq())
        order = sorted(range(len(self.heard)), key=lambda i: (-self.heard[i][0], -i))
        for i in order:
            te, Fe, A, B, cq, text = self.heard[i]
            d = int(t0) - te
            k = int(round(d / self.step_slot))
            if abs(int(F) - Fe) > self.reach_f or k < 1 or d > self._age_max() or abs(d - k * self.step_slot) > self.reach_t:
                continue
            if k % 2 == 0:
                offer(KIND_FROM, hyp_from(B))
                if A is not None:
                    offer(KIND_PAIR, hyp_pair(A, B))
                if cq:
                    offer(KIND_CQ_FROM, hyp_cq_from(B))
                    offer(KIND_TEXT, hyp_text(text))
            elif A is not None:
                offer(KIND_PAIR, hyp_pair(B, A))
        return out


class FT8_AP_Skimmer(FT8_Skimmer):
    """An ``FT8_Skimmer`` with the keyword ``ap`` (a ``params()``; needs ``decode=True``; ``report=True`` and ``passes=2`` are
    refused with it).  Every release sends the records min-sum (and ``osd``) left without a message, with the hypotheses
    ``history`` (a ``History``) has for their place, through ``decode`` while their frames are still in the ring.  A rescued
    record gets ``ok``, ``status``, ``bits77``, ``i3``, ``n3``, ``text``, ``nerr`` and ``iterations`` from the pick; every
    record gains ``ap``: 0 not tried, -1 tried in vain, else the kind 1 to 5 of the hypothesis that decoded it.  Then every
    ``ok`` record is noted.  With ``ap=None`` it is an ``FT8_Skimmer``."""

    def __init__(self, *args, ap=None, **kw):
        self.ap = ap
        if ap is not None:
            given = inspect.signature(FT_Skimmer.__init__).bind(self, *args, **kw)
            given.apply_defaults()
            if not given.arguments["decode"]:
                raise ValueError(f"{type(self).__name__}: ap rescues frames the decoder failed on: it needs decode=True")
            if given.arguments["report"] or int(given.arguments["passes"]) != 1:
                raise ValueError(f"{type(self).__name__}: ap does not go together with report=True or passes=2: a rescued frame is "
                                 f"neither measured nor subtracted")
            plan(ap)                                                     # a bad setting fails here, with or without a device
        self.history = History()
        super().__init__(*args, **kw)

    def reset(self):
        super().reset()
        self.history = History(self.history.reach_f, self.history.hold, self.history.step_slot, self.history.reach_t)

    def _release(self):
        recs = super()._release()
        if self.ap is None or not recs:
            return recs
        hyps, kinds, pairs, tried = [], [], [], []
        index = {}
        for rec in recs:
            rec["ap"] = 0
            if rec["ok"]:
                continue
            c = len(tried)
            mine = []
            for kind, h in self.history.hypotheses(rec["F"], rec["t0"]):
                key = (h[0].tobytes(), h[1].tobytes())
                if key not in index:
                    index[key] = len(hyps)
                    hyps.append(h)
                    kinds.append(kind)
                mine.append(index[key])
            pairs += [(c, h) for h in sorted(mine)]
            tried.append(rec)
        if tried:
            got = decode(self.dec, [r["F"] for r in tried], [r["t0"] for r in tried], pairs, hyps, self.ap, self.ldpc)
            m = self.DECODERS.MODE
            for c, rec in enumerate(tried):
                if got["pair"][c] < 0:
                    rec["ap"] = -1
                    continue
                b77 = got["bits"][c, :MSG].copy()
                i3, n3 = _msg.types(b77)
                rec.update(ok=True, status=_ldpc.STATUS_OK, bits77=b77, i3=i3, n3=n3, text=m.UNPACK(b77), nerr=int(got["nerr"][c]),
                           iterations=int(got["iterations"][c]), ap=kinds[int(got["hyp"][c])])
        for rec in recs:
            self.history.note(rec)
        return recs
