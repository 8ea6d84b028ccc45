"""The 77-bit message of FT8: ``unpack77`` and ``pack77`` for the standard message (types 1 and 2:
two calls and a grid, a report or a sign-off) and free text (type 0.0).  Every other type unpacks to None; the record of a
frame keeps its bits, ``i3`` and ``n3`` beside the text.  The layout follows the published protocol description; this
repository holds no on-air frame to pin it (the LDPC tables are the part that has a proof)."""
from __future__ import annotations

import re

import numpy as np

NTOKENS = 2063592                                # c28 below this: DE, QRZ, CQ and the directed CQs
MAX22 = 1 << 22                                  # c28 from NTOKENS on: that many hashed calls, then the standard calls
MAXGRID4 = 32400
A1 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"     # a standard call's six characters, the digit in third place
A2 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
A3 = "0123456789"
A4 = " ABCDEFGHIJKLMNOPQRSTUVWXYZ"
FREE = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ+-./?"
SIGN_OFF = {1: "", 2: "RRR", 3: "RR73", 4: "73"}  # g15 - 32400
REPORT_MIN, REPORT_MAX = -30, 99                 # what pack77 takes; unpack77 prints whatever the bits say


def _int(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def _bits(v, n):
    return [(int(v) >> (n - 1 - i)) & 1 for i in range(n)]


def types(bits77):
    """-> (i3, n3): the last three bits, and the three before them (meaningful for i3 = 0)"""
    b = [int(v) & 1 for v in np.asarray(bits77).reshape(-1)]
    if len(b) != 77:
        raise ValueError(f"{len(b)} bits, 77 expected")
    return _int(b[74:77]), _int(b[71:74])


# ---- c28: a call, or what stands in a call's place ------------------------------------------------------------------------

def unpack_call(c28):
    """-> text, or None for a value that means nothing"""
    if c28 < 3:
        return ("DE", "QRZ", "CQ")[c28]
    if c28 < 1003:
        return f"CQ {c28 - 3:03d}"
    if c28 < 1003 + 27 ** 4:
        n, s = c28 - 1003, ""
        for _ in range(4):
            n, r = divmod(n, 27)
            s = A4[r] + s
        t = s.lstrip()                            # one to four letters, right-aligned
        return "CQ " + t if t and " " not in t else None
    if c28 < NTOKENS:
        return None
    if c28 < NTOKENS + MAX22:
        return "<...>"
    n = c28 - NTOKENS - MAX22
    n, i6 = divmod(n, 27)
    n, i5 = divmod(n, 27)
    n, i4 = divmod(n, 27)
    n, i3 = divmod(n, 10)
    i1, i2 = divmod(n, 36)
    if i1 >= 37:
        return None
    return (A1[i1] + A2[i2] + A3[i3] + A4[i4] + A4[i5] + A4[i6]).strip()


def pack_call(call):
    """a standard call of up to six characters with its digit in second or third place -> c28 (ValueError otherwise)"""
    c = call.upper()
    if len(c) >= 3 and c[2] in A3 and len(c) <= 6:
        six = c.ljust(6)
    elif len(c) >= 2 and c[1] in A3 and len(c) <= 5:
        six = (" " + c).ljust(6)
    else:
        raise ValueError(f"not a standard call: {call!r}")
    try:
        i = [A1.index(six[0]), A2.index(six[1]), A3.index(six[2]), A4.index(six[3]), A4.index(six[4]), A4.index(six[5])]
    except ValueError:
        raise ValueError(f"not a standard call: {call!r}") from None
    if " " in six.strip():
        raise ValueError(f"not a standard call: {call!r}")
    n = ((((i[0] * 36 + i[1]) * 10 + i[2]) * 27 + i[3]) * 27 + i[4]) * 27 + i[5]
    return NTOKENS + MAX22 + n


def _pack_first(tokens):
    """the tokens that stand in the first call's place -> (c28, tokens used)"""
    t = tokens[0]
    if t in ("DE", "QRZ"):
        return ("DE", "QRZ").index(t), 1
    if t == "CQ":
        if len(tokens) >= 3 and re.fullmatch(r"\d{3}", tokens[1]):
            return 3 + int(tokens[1]), 2
        if len(tokens) >= 3 and re.fullmatch(r"[A-Z]{1,4}", tokens[1]) and _is_call(tokens[2]):
            n = 0
            for ch in tokens[1].rjust(4):
                n = 27 * n + A4.index(ch)
            return 1003 + n, 2
        return 2, 1
    return None, 0


def _split_suffix(call):
    for suf in ("/R", "/P"):
        if call.endswith(suf):
            return call[:-2], suf
    return call, ""


def _is_call(t):
    try:
        pack_call(_split_suffix(t)[0])
        return True
    except ValueError:
        return False


# ---- g15: grid, report or sign-off ------------------------------------------------------------------------------------------

def unpack_g15(g15, r1):
    if g15 <= MAXGRID4:
        n, d = divmod(g15, 10)
        n, c = divmod(n, 10)
        a, b = divmod(n, 18)
        return ("R " if r1 else "") + chr(65 + a) + chr(65 + b) + str(c) + str(d)
    k = g15 - MAXGRID4
    if k in SIGN_OFF:
        return SIGN_OFF[k]
    return ("R" if r1 else "") + f"{k - 35:+03d}"


def pack_g15(tokens):
    """the tokens behind the two calls -> (g15, R1)"""
    if not tokens:
        return MAXGRID4 + 1, 0
    r1 = 0
    if len(tokens) == 2 and tokens[0] == "R":
        r1, tokens = 1, tokens[1:]
    if len(tokens) != 1:
        raise ValueError(f"not a grid, report or sign-off: {tokens}")
    t = tokens[0]
    if not r1 and t in ("RRR", "RR73", "73"):
        return MAXGRID4 + {"RRR": 2, "RR73": 3, "73": 4}[t], 0
    if re.fullmatch(r"[A-R]{2}\d{2}", t):
        return ((ord(t[0]) - 65) * 18 + ord(t[1]) - 65) * 100 + int(t[2:]), r1
    m = re.fullmatch(r"(R?)([+-]\d{2})", t)
    if m and not r1 and REPORT_MIN <= int(m.group(2)) <= REPORT_MAX:
        return MAXGRID4 + 35 + int(m.group(2)), 1 if m.group(1) else 0
    raise ValueError(f"not a grid, report or sign-off: {t!r}")


# ---- the message ------------------------------------------------------------------------------------------------------------

def unpack77(bits77):
    """77 bits -> text, or None for a type that is not unpacked here (or a value that means nothing)"""
    b = [int(v) & 1 for v in np.asarray(bits77).reshape(-1)]
    i3, n3 = types(b)
    if i3 in (1, 2):
        suf = "/R" if i3 == 1 else "/P"
        c1, c2 = unpack_call(_int(b[0:28])), unpack_call(_int(b[29:57]))
        if c1 is None or c2 is None or c2.split()[0] in ("DE", "QRZ", "CQ"):
            return None
        if b[28]:
            c1 += suf
        if b[57]:
            c2 += suf
        return " ".join(t for t in (c1, c2, unpack_g15(_int(b[59:74]), b[58])) if t)
    if i3 == 0 and n3 == 0:
        n, s = _int(b[0:71]), ""
        for _ in range(13):
            n, r = divmod(n, 42)
            s = FREE[r] + s
        return s.strip() if n == 0 else None
    return None


def pack77(text):
    """text -> uint8 [77]: a standard message where the text is one, else free text of at most 13 characters; ValueError
    for anything else"""
    text = " ".join(str(text).upper().split())
    tokens = text.split()
    try:
        if len(tokens) < 2:
            raise ValueError("too few words")
        c1, used = _pack_first(tokens)
        rest = tokens[used:]
        s1 = ""
        if c1 is None:
            call, s1 = _split_suffix(tokens[0])
            c1, rest = pack_call(call), tokens[1:]
        if not rest:
            raise ValueError("no second call")
        call, s2 = _split_suffix(rest[0])
        c2 = pack_call(call)
        if s1 and s2 and s1 != s2:
            raise ValueError("/R and /P in one message")
        g15, r1 = pack_g15(rest[1:])
        i3 = 2 if "/P" in (s1, s2) else 1
        bits = _bits(c1, 28) + [1 if s1 else 0] + _bits(c2, 28) + [1 if s2 else 0] + [r1] + _bits(g15, 15) + _bits(i3, 3)
        return np.array(bits, np.uint8)
    except ValueError:
        pass
    if len(text) > 13 or any(ch not in FREE for ch in text):
        raise ValueError(f"neither a standard message nor free text of at most 13 characters: {text!r}")
    n = 0
    for ch in text.rjust(13):
        n = 42 * n + FREE.index(ch)
    return np.array(_bits(n, 71) + [0] * 6, np.uint8)
