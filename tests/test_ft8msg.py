"""The 77-bit message of FT8 (pysdr_amd/ft8msg.py): pack77 / unpack77 round trips of the standard message
and of free text, every boundary value of c28 and g15, and None for every type that is not unpacked.  No GPU."""
import numpy as np
import pytest

from pysdr_amd import ft8msg as fm

ROUND_TRIPS = ["CQ K1ABC FN42", "K1ABC W9XYZ -12", "W9XYZ K1ABC R+07", "K1ABC W9XYZ RR73", "K1ABC W9XYZ RRR", "K1ABC W9XYZ 73",
               "K1ABC W9XYZ", "CQ DX K1ABC FN42", "CQ 123 K1ABC FN42", "CQ 000 K1ABC AA00", "CQ 999 KA1ABC RR99", "CQ TEST K1A FN42",
               "CQ A K1ABC FN42", "K1ABC/R W9XYZ FN42", "K1ABC W9XYZ/R R FN42", "CQ K1ABC/P FN42", "K1ABC/P W9XYZ/P -01", "K1A W9XYZ -30",
               "W9XYZ K1A +99", "DE K1ABC FN42", "QRZ K1ABC", "K1ABC W9XYZ R FN42", "K1ABC W9XYZ R-30", "9A1A 3D2AG +00",
               "HELLO WORLD", "TNX BOB 73 GL", "+-./?", "A", "0123456789ABC"]


def field(bits, lo, hi):
    return int("".join(str(int(b)) for b in bits[lo:hi]), 2)


def standard(c1, c2, g15, r1a=0, r1b=0, R1=0, i3=1):
    return np.array(fm._bits(c1, 28) + [r1a] + fm._bits(c2, 28) + [r1b] + [R1] + fm._bits(g15, 15) + fm._bits(i3, 3), np.uint8)


@pytest.mark.parametrize("text", ROUND_TRIPS)
def test_round_trip(text):
    bits = fm.pack77(text)
    assert bits.dtype == np.uint8 and bits.shape == (77,) and set(bits) <= {0, 1}
    assert fm.unpack77(bits) == text
    assert np.array_equal(fm.pack77(fm.unpack77(bits)), bits)
    assert fm.pack77(text.lower() + "  ").tolist() == bits.tolist()


def test_the_fields_are_where_the_layout_puts_them():
    b = fm.pack77("CQ K1ABC FN42")
    assert fm.types(b)[0] == 1 and field(b, 0, 28) == 2 and b[28] == 0 and b[57] == 0 and b[58] == 0
    n = 0
    for ch, alphabet in zip(" K1ABC", (fm.A1, fm.A2, fm.A3, fm.A4, fm.A4, fm.A4)):
        n = n * len(alphabet) + alphabet.index(ch)
    assert field(b, 29, 57) == fm.NTOKENS + (1 << 22) + n
    assert field(b, 59, 74) == ((5 * 18 + 13) * 10 + 4) * 10 + 2                 # F N 4 2
    b = fm.pack77("K1ABC/P W9XYZ R-12")
    assert fm.types(b)[0] == 2 and b[28] == 1 and b[57] == 0 and b[58] == 1 and field(b, 59, 74) == 32400 + 35 - 12
    assert field(fm.pack77("CQ DX K1ABC FN42"), 0, 28) == 1003 + 4 * 27 + 24
    assert field(fm.pack77("CQ 123 K1ABC FN42"), 0, 28) == 3 + 123
    assert [field(fm.pack77(f"K1ABC W9XYZ {t}".strip()), 59, 74) for t in ("", "RRR", "RR73", "73")] == [32401, 32402, 32403, 32404]
    b = fm.pack77("HELLO WORLD")
    assert fm.types(b) == (0, 0)
    n = 0
    for ch in "  HELLO WORLD":
        n = 42 * n + fm.FREE.index(ch)
    assert field(b, 0, 71) == n


def test_every_boundary_of_c28():
    k1abc = field(fm.pack77("CQ K1ABC FN42"), 29, 57)
    text = lambda c28: fm.unpack77(standard(c28, k1abc, 32401))                  # noqa: E731
    assert [text(v) for v in (0, 1, 2)] == ["DE K1ABC", "QRZ K1ABC", "CQ K1ABC"]
    assert text(3) == "CQ 000 K1ABC" and text(1002) == "CQ 999 K1ABC"
    assert text(1003) is None                                                   # no letter at all
    assert text(1004) == "CQ A K1ABC" and text(1003 + 26) == "CQ Z K1ABC" and text(1003 + 27 + 1) == "CQ AA K1ABC"
    assert text(1003 + 27) is None                                              # "A " is not right-aligned
    assert text(532443) == "CQ ZZZZ K1ABC" and 532443 == 1003 + 27 ** 4 - 1
    assert text(532444) is None and text(fm.NTOKENS - 1) is None
    assert text(fm.NTOKENS) == "<...> K1ABC" and text(fm.NTOKENS + (1 << 22) - 1) == "<...> K1ABC"
    first = fm.NTOKENS + (1 << 22)
    assert fm.unpack_call(first) == "00" and fm.unpack_call((1 << 28) - 1) == "ZZ9ZZZ"
    assert first + 37 * 36 * 10 * 27 ** 3 == 1 << 28
    assert fm.pack_call("ZZ9ZZZ") == (1 << 28) - 1 and fm.pack_call("K1A") == fm.pack_call("k1a") and fm.unpack_call(fm.pack_call("K1A")) == "K1A"
    for bad in ("K1ABCD", "ABC", "K", "", "K1AB-C", "1", "KABC1", "K1 A"):
        with pytest.raises(ValueError):
            fm.pack_call(bad)
    # the second place holds a call, never a token
    assert fm.unpack77(standard(k1abc, 2, 32401)) is None


def test_every_boundary_of_g15():
    a, b = field(fm.pack77("CQ K1ABC FN42"), 29, 57), field(fm.pack77("CQ W9XYZ FN42"), 29, 57)
    text = lambda g, R1=0: fm.unpack77(standard(a, b, g, R1=R1))                  # noqa: E731
    assert text(0) == "K1ABC W9XYZ AA00" and text(32399) == "K1ABC W9XYZ RR99" and text(32399, 1) == "K1ABC W9XYZ R RR99"
    assert text(32400) == "K1ABC W9XYZ SA00"                                    # the last value the grid's range holds
    assert text(32401) == "K1ABC W9XYZ" and text(32402) == "K1ABC W9XYZ RRR" and text(32403) == "K1ABC W9XYZ RR73" and text(32404) == "K1ABC W9XYZ 73"
    assert text(32405) == "K1ABC W9XYZ -30" and text(32405, 1) == "K1ABC W9XYZ R-30"
    assert text(32435) == "K1ABC W9XYZ +00" and text(32442, 1) == "K1ABC W9XYZ R+07" and text(32423) == "K1ABC W9XYZ -12"
    assert text(32767) == "K1ABC W9XYZ +332"
    for bad in ("K1ABC W9XYZ SA00", "K1ABC W9XYZ -31", "K1ABC W9XYZ R R-12", "K1ABC W9XYZ FN4", "K1ABC/R W9XYZ/P FN42"):
        assert len(bad) > 13                                                    # nothing here is free text either
        with pytest.raises(ValueError):
            fm.pack77(bad)


def test_an_unknown_type_gives_none():
    rng = np.random.default_rng(3)
    for i3 in range(8):
        for n3 in range(8):
            bits = np.concatenate((rng.integers(0, 2, 71), fm._bits(n3, 3), fm._bits(i3, 3))).astype(np.uint8)
            got = fm.unpack77(bits)
            assert fm.types(bits) == (i3, n3)
            if i3 in (1, 2) or (i3 == 0 and n3 == 0):
                assert got is None or isinstance(got, str)
            else:
                assert got is None, (i3, n3)
    top = np.array([1] * 71 + [0] * 6, np.uint8)                                 # 2^71 - 1 is beyond 42^13
    assert fm.unpack77(top) is None and fm.unpack77(np.zeros(77, np.uint8)) == ""
    with pytest.raises(ValueError):
        fm.unpack77(np.zeros(76))
    with pytest.raises(ValueError):
        fm.pack77("THIS TEXT IS TOO LONG")
    with pytest.raises(ValueError):
        fm.pack77("NO_UNDERSCORE")
