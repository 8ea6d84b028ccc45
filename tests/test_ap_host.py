"""The host policy of a-priori decoding (pysdr_amd/ap.py), which needs no device: the hypothesis makers
against ``ft8msg.pack77`` on the masked bits, the calls a text names, and ``History`` -- same sender and partner by the
parity of the slots between, the reach in fine rows and in steps, the cap of eight, expiry, and that nothing depends on how
the stream was cut into calls."""
import numpy as np
import pytest

from tests import ap_oracle as ao

FIRST, SECOND, I3 = list(range(0, 29)), list(range(29, 58)), list(range(74, 77))


def bits_of(h):
    """a hypothesis -> (the mask's set positions, the value's 77 bits)"""
    assert ao.hyp_ok(*h) and h[0].dtype == np.uint8 and h[0].shape == (12,) and h[1].shape == (12,)
    return list(np.flatnonzero(ao.unword(h[0])[:77])), ao.unword(h[1])[:77]


def test_the_makers_name_the_bits_pack77_gives():
    from pysdr_amd import ap
    from pysdr_amd.ft8msg import pack77
    for text, h, where in (("CQ K1ABC FN42", ap.hyp_cq(), FIRST + I3), ("CQ W9XYZ EN37", ap.hyp_cq(), FIRST + I3),
                           ("CQ K1ABC FN42", ap.hyp_from("K1ABC"), SECOND + I3), ("W9XYZ K1ABC -12", ap.hyp_from("K1ABC"), SECOND + I3),
                           ("W9XYZ K1ABC R-07", ap.hyp_from("k1abc"), SECOND + I3), ("K1ABC W9XYZ RR73", ap.hyp_pair("K1ABC", "W9XYZ"), FIRST + SECOND + I3),
                           ("K1ABC W9XYZ EN37", ap.hyp_pair("K1ABC", "W9XYZ"), FIRST + SECOND + I3), ("CQ DL1ABC JO62", ap.hyp_cq_from("DL1ABC"), FIRST + SECOND + I3),
                           ("K1ABC/R W9XYZ R FN42", ap.hyp_pair("K1ABC/R", "W9XYZ"), FIRST + SECOND + I3), ("CQ G4ABC/P IO91", ap.hyp_from("G4ABC/P"), SECOND + I3),
                           ("CQ K1ABC FN42", ap.hyp_text("CQ K1ABC FN42"), list(range(77))), ("TNX BOB 73 GL", ap.hyp_text("TNX BOB 73 GL"), list(range(77)))):
        at, value = bits_of(h)
        msg = pack77(text)
        assert at == sorted(where), (text, at)
        assert np.array_equal(value[at], msg[at]), text
        assert not np.delete(value, at).any()
    assert [len(bits_of(h)[0]) for h in (ap.hyp_cq(), ap.hyp_from("K1ABC"), ap.hyp_pair("K1ABC", "W9XYZ"), ap.hyp_cq_from("K1ABC"), ap.hyp_text("CQ K1ABC FN42"))] \
        == [32, 32, 61, 61, 77]
    # a hypothesis that is wrong for a message differs from it somewhere under its mask
    at, value = bits_of(ap.hyp_from("W9XYZ"))
    assert not np.array_equal(value[at], pack77("CQ K1ABC FN42")[at])
    for bad in ("HELLO", "", "K1ABC W9XYZ", "<...>"):
        with pytest.raises(ValueError):
            ap.hyp_from(bad)
    with pytest.raises(ValueError):
        ap.hyp_text("THIS TEXT IS TOO LONG")
    with pytest.raises(ValueError):
        ap.hyp_bits(np.zeros(77, np.uint8), np.zeros(77, np.uint8))
    tab = ap.table([ap.hyp_cq(), ap.hyp_from("K1ABC")])
    assert tab.shape == (2, 24) and tab.dtype == np.uint8 and np.array_equal(tab[1, :12], ap.hyp_from("K1ABC")[0]) and np.array_equal(tab[0, 12:], ap.hyp_cq()[1])


def test_the_calls_a_text_names():
    from pysdr_amd import ap
    assert ap.calls_of("CQ K1ABC FN42") == (None, "K1ABC", True)
    assert ap.calls_of("CQ DX K1ABC FN42") == (None, "K1ABC", False) and ap.calls_of("CQ 017 K1ABC") == (None, "K1ABC", False)
    assert ap.calls_of("QRZ K1ABC") == (None, "K1ABC", False) and ap.calls_of("DE K1ABC FN42") == (None, "K1ABC", False)
    assert ap.calls_of("k1abc w9xyz -12") == ("K1ABC", "W9XYZ", False) and ap.calls_of("W9XYZ K1ABC/R R FN42") == ("W9XYZ", "K1ABC/R", False)
    for text in (None, "", "TNX BOB 73 GL", "<...> K1ABC -01", "HELLO"):
        assert ap.calls_of(text) is None, text


def rec(text, t0, F, ok=True):
    return dict(ok=ok, text=text, t0=t0, F=F)


def kinds(h, F, t0):
    return [k for k, _ in h.hypotheses(F, t0)]


def test_history_same_sender_partner_reach_cap_and_expiry():
    from pysdr_amd import ap
    h = ap.History()
    assert (h.reach_f, h.hold, h.step_slot, h.reach_t) == (2, 4, 375, 8)
    assert kinds(h, 50, 1000) == [1] and np.array_equal(h.hypotheses(50, 1000)[0][1][0], ap.hyp_cq()[0])       # CQ ? ? is always offered
    assert not h.note(rec("CQ K1ABC FN42", 100, 50, ok=False)) and not h.note(rec(None, 100, 50)) and not h.note(rec("TNX BOB 73 GL", 100, 50))
    assert kinds(h, 50, 850) == [1]
    assert h.note(rec("K1ABC W9XYZ -12", 100, 50))
    # two slots later, the same sender again: ? B ?, A B ?
    got = h.hypotheses(50, 850)
    assert [k for k, _ in got] == [1, 2, 3]
    for (_, a), b in zip(got, (ap.hyp_cq(), ap.hyp_from("W9XYZ"), ap.hyp_pair("K1ABC", "W9XYZ"))):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # one slot later, the partner answering: B A ?
    got = h.hypotheses(50, 475)
    assert [k for k, _ in got] == [1, 3] and np.array_equal(got[1][1][1], ap.hyp_pair("W9XYZ", "K1ABC")[1])
    assert kinds(h, 50, 100 + 3 * 375) == [1, 3] and kinds(h, 50, 100 + 4 * 375) == [1, 2, 3]
    # the reach in steps and in fine rows, and nothing for the same slot or an earlier one
    assert kinds(h, 50, 850 + 8) == [1, 2, 3] and kinds(h, 50, 850 - 8) == [1, 2, 3] and kinds(h, 50, 850 + 9) == [1] and kinds(h, 50, 850 - 9) == [1]
    assert kinds(h, 52, 850) == [1, 2, 3] and kinds(h, 48, 850) == [1, 2, 3] and kinds(h, 53, 850) == [1] and kinds(h, 47, 850) == [1]
    assert kinds(h, 50, 100) == [1] and kinds(h, 50, 104) == [1] and kinds(h, 50, 100 - 375) == [1]
    # a CQ: ? B ?, CQ B ? and its own text; to the partner of a CQ nothing is known
    c = ap.History()
    assert c.note(rec("CQ K1ABC FN42", 100, 50))
    got = c.hypotheses(50, 850)
    assert [k for k, _ in got] == [1, 2, 4, 5] and np.array_equal(got[3][1][1], ap.hyp_text("CQ K1ABC FN42")[1])
    assert np.array_equal(got[2][1][1], ap.hyp_cq_from("K1ABC")[1]) and kinds(c, 50, 475) == [1]
    assert c.note(rec("CQ DX W9XYZ EN37", 100, 60)) and kinds(c, 60, 850) == [1, 2]
    # expiry: hold = 4 slot pairs
    assert kinds(h, 50, 100 + 8 * 375) == [1, 2, 3] and kinds(h, 50, 100 + 9 * 375) == [1] and kinds(h, 50, 100 + 10 * 375) == [1]
    assert h.note(rec("CQ JA1XYZ PM95", 100 + 12 * 375, 10)) and len(h.heard) == 1              # noting drops what is too old
    short = ap.History(hold=1)
    short.note(rec("K1ABC W9XYZ -12", 100, 50))
    assert kinds(short, 50, 850) == [1, 2, 3] and kinds(short, 50, 100 + 3 * 375) == [1]
    # the cap of eight, in order, the newest remembered frame first; a hypothesis is offered once
    m = ap.History()
    m.note(rec("JA1XYZ OH8X KP20", 100, 52))                                     # the oldest and first noted: the cap cuts it off
    m.note(rec("K1ABC W9XYZ -12", 100, 50))
    m.note(rec("DL1ABC G4ABC JO62", 100, 51))
    m.note(rec("W9XYZ K1ABC R-07", 475, 50))
    m.note(rec("CQ VK2DEF QF56", 850, 49))
    m.note(rec("K1ABC W9XYZ RR73", 850, 50))
    got = m.hypotheses(50, 100 + 4 * 375)
    # (the frame of step 475, an odd number of slots back, offers B A ? = K1ABC W9XYZ ?, which the newest frame offered already)
    want = [ap.hyp_cq(), ap.hyp_from("W9XYZ"), ap.hyp_pair("K1ABC", "W9XYZ"), ap.hyp_from("VK2DEF"), ap.hyp_cq_from("VK2DEF"),
            ap.hyp_text("CQ VK2DEF QF56"), ap.hyp_from("G4ABC"), ap.hyp_pair("DL1ABC", "G4ABC")]
    assert len(got) == 8 and [k for k, _ in got] == [1, 2, 3, 2, 4, 5, 2, 3]
    for (_, a), b in zip(got, want):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len(m.hypotheses(52, 100 + 4 * 375)) == 7                             # fine row 49 is out of reach there, JA1XYZ's is in


def test_history_does_not_depend_on_how_the_stream_is_cut():
    """the same records noted in one go, one by one with questions between, and in another order of equal steps give the same
    hypotheses: everything is in absolute steps"""
    from pysdr_amd import ap
    recs = [rec("CQ K1ABC FN42", 13, 10), rec("W9XYZ K1ABC -05", 388, 11), rec("K1ABC W9XYZ R-11", 763, 10), rec("CQ DL1ABC JO62", 763, 40),
            rec("W9XYZ K1ABC RR73", 1138, 11)]
    asks = [(10, 763), (11, 1138), (10, 1513), (40, 1513), (12, 1888), (10, 13 + 9 * 375)]

    def answers(h):
        return [[(k, a[0].tobytes(), a[1].tobytes()) for k, a in h.hypotheses(F, t0)] for F, t0 in asks]

    whole = ap.History()
    for r in recs:
        whole.note(r)
    piecewise = ap.History()
    seen = []
    for r in recs:
        piecewise.note(r)
        seen.append(answers(piecewise))                                          # asking changes nothing
    swapped = ap.History()
    for r in (recs[0], recs[1], recs[3], recs[2], recs[4]):                      # the two records of step 763 in the other order
        swapped.note(r)
        swapped.note(r)                                                          # and noted twice
    assert answers(whole) == answers(piecewise) == seen[-1]
    assert [sorted(a) for a in answers(swapped)] == [sorted(a) for a in answers(whole)]
    assert any(len(a) > 1 for a in answers(whole))
