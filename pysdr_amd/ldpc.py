"""LDPC(174,91) of FT8 and FT4 (kernel ``ldpc.hip``, pure half ``ldpc_plan.h``): the generator, the
sparse parity checks, CRC-14, the encoder and the codeword test, in NumPy, and the settings of the device decoder.  The
code is systematic: 77 message bits, 14 CRC bits, 83 parity bits, in transmission order -- the order of the skimmers' soft
bits.  The tables are protocol constants; the sparse checks are the 83 words of weight at most 7 in the generator's dual
code (tests/test_ldpc_oracle.py derives them again), every column in exactly three of them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import LdpcCfg, OsdCfg

N, K, M, MSG, CRC_BITS, EDGES = 174, 91, 83, 77, 14, 522
OSD_PATTERNS = (1, 92, 4187)                     # error patterns the second stage scores at order 0, 1, 2
CRC_POLY = 0x2757                                # x^14 + these terms; zero initial value, no reflection, no final XOR
ITERS_MAX, DECODE_MAX = 200, 4096
STATUS_NONE, STATUS_CODEWORD, STATUS_OK = 0, 1, 2   # no codeword; a codeword with a wrong CRC or an all-zero message; a message

# Parity bit j (codeword bit 91 + j) is the XOR of the message bits i < 91 whose bit is set in row j: the 23 hex digits are
# a 92-bit number whose lowest bit is dropped; the remaining 91, most significant first, are i = 0 .. 90.
GENERATOR_HEX = """
8329ce11bf31eaf509f27fc 761c264e25c259335493132 dc265902fb277c6410a1bdc 1b3f417858cd2dd33ec7f62
09fda4fee04195fd034783a 077cccc11b8873ed5c3d48a 29b62afe3ca036f4fe1a9da 6054faf5f35d96d3b0c8c3e
e20798e4310eed27884ae90 775c9c08e80e26ddae56318 b0b811028c2bf997213487c 18a0c9231fc60adf5c5ea32
76471e8302a0721e01b12b8 ffbccb80ca8341fafb47b2e 66a72a158f9325a2bf67170 c4243689fe85b1c51363a18
0dff739414d1a1b34b1c270 15b48830636c8b99894972e 29a89c0d3de81d665489b0e 4f126f37fa51cbe61bd6b94
99c47239d0d97d3c84e0940 1919b75119765621bb4f1e8 09db12d731faee0b86df6b8 488fc33df43fbdeea4eafb4
827423ee40b675f756eb5fe abe197c484cb74757144a9a 2b500e4bc0ec5a6d2bdbdd0 c474aa53d70218761669360
8eba1a13db3390bd6718cec 753844673a27782cc42012e 06ff83a145c37035a5c1268 3b37417858cc2dd33ec3f62
9a4a5a28ee17ca9c324842c bc29f465309c977e89610a4 2663ae6ddf8b5ce2bb29488 46f231efe457034c1814418
3fb2ce85abe9b0c72e06fbe de87481f282c153971a0a2e fcd7ccf23c69fa99bba1412 f0261447e9490ca8e474cec
4410115818196f95cdd7012 088fc31df4bfbde2a4eafb4 b8fef1b6307729fb0a078c0 5afea7acccb77bbc9d99a90
49a7016ac653f65ecdc9076 1944d085be4e7da8d6cc7d0 251f62adc4032f0ee714002 56471f8702a0721e00b12b8
2b8e4923f2dd51e2d537fa0 6b550a40a66f4755de95c26 a18ad28d4e27fe92a4f6c84 10c2e586388cb82a3d80758
ef34a41817ee02133db2eb0 7e9c0c54325a9c15836e000 3693e572d1fde4cdf079e86 bfb2cec5abe1b0c72e07fbe
7ee18230c583cccc57d4b08 a066cb2fedafc9f52664126 bb23725abc47cc5f4cc4cd2 ded9dba3bee40c59b5609b4
d9a7016ac653e6decdc9036 9ad46aed5f707f280ab5fc4 e5921c77822587316d7d3c2 4f14da8242a8b86dca73352
8b8b507ad467d4441df770e 22831c9cf1169467ad04b68 213b838fe2ae54c38ee7180 5d926b6dd71f085181a4e12
66ab79d4b29ee6e69509e56 958148682d748a38dd68baa b8ce020cf069c32a723ab14 f4331d6d461607e95752746
6da23ba424b9596133cf9c8 a636bcbc7b30c5fbeae67fe 5cb0d86a07df654a9089a20 f11f106848780fc9ecdd80a
1fbb5364fb8d2c9d730d5ba fcb86bc70a50c9d02a5d034 a534433029eac15f322e34c c989d9c7c3d3b8c55d75130
7bb38b2f0186d46643ae962 2644ebadeb44b9467d1f42c 608cc857594bfbb55d69600
""".split()

# Check m is row m; edge numbers run row-major over this list.
CHECKS_TEXT = (
    "0 3 51 56 85 135 151; 0 25 44 79 127 146; 0 32 71 105 106 156; 1 26 40 60 61 114 132; 1 47 73 112 127 159; "
    "1 53 85 100 134 163; 2 12 47 77 94 122; 2 23 29 71 103 138; 2 43 79 123 126 168; 3 28 67 119 133 172; "
    "3 30 58 90 91 95 152; 4 31 59 92 114 145; 4 33 64 77 97 106 153; 4 38 74 101 135 166; 5 23 60 93 121 150; "
    "5 31 63 96 125 137; 5 32 84 107 115 155; 6 32 61 94 95 142; 6 48 57 89 99 104 167; 6 49 80 98 131 172; "
    "7 24 62 82 92 95 147; 7 39 69 81 103 113 144; 7 45 70 111 118 165; 8 34 65 98 138 145; 8 39 89 105 133 150; "
    "8 53 62 130 146 154; 9 35 66 99 106 125; 9 43 81 90 110 143 148; 9 52 65 83 111 127 164; 10 36 66 86 100 138 157; "
    "10 43 74 109 120 165; 10 48 87 91 141 156; 11 37 67 101 104 154; 11 42 65 88 96 134 158; 11 49 60 117 118 143; "
    "12 38 68 102 148 161; 12 50 63 113 117 156; 13 29 82 112 124 169; 13 30 78 97 131 163; 13 40 70 87 101 122 155; "
    "14 41 58 105 122 158; 14 55 86 107 118 170; 14 57 59 73 110 149 162; 15 38 61 111 133 157; 15 42 72 107 140 159; "
    "15 46 75 129 136 153; 16 26 88 102 115 152; 16 36 73 80 108 130 153; 16 41 74 128 169 171; 17 35 75 88 112 113 142; "
    "17 41 78 143 145 151; 17 48 54 123 140 166; 18 34 58 72 109 124 160; 18 37 76 103 115 162; 18 45 80 116 134 166; "
    "19 35 62 93 135 160; 19 45 64 79 119 139 169; 19 46 69 91 137 164; 20 36 72 137 151 168; 20 44 77 82 116 120 150; "
    "20 53 76 99 139 170; 21 46 57 117 126 163; 21 52 67 108 120 173; 21 56 84 92 139 158; 22 33 70 93 126 152; "
    "22 42 78 119 130 144; 22 54 66 94 171 173; 23 51 75 128 147 148; 24 37 64 98 121 159; 24 52 68 89 100 129 155; "
    "25 40 76 108 140 147; 25 50 55 90 121 136 167; 26 39 55 123 124 125; 27 28 83 87 116 142 149; 27 31 71 102 131 165; "
    "27 47 69 84 104 128 157; 28 33 86 96 146 161; 29 49 59 85 136 141 161; 30 68 132 149 154 168; 34 81 132 141 170 173; "
    "44 54 63 110 129 160 172; 50 56 97 162 164 171; 51 83 109 114 144 167")

CHECKS = tuple(tuple(int(v) for v in row.split()) for row in CHECKS_TEXT.split(";"))


def _generator():
    g = np.zeros((M, K), np.uint8)
    for j, word in enumerate(GENERATOR_HEX):
        v = int(word, 16) >> 1
        for i in range(K):
            g[j, i] = (v >> (K - 1 - i)) & 1
    return g


GENERATOR = _generator()                          # uint8 [83][91]: parity j = GENERATOR[j] . message mod 2
GENERATOR.setflags(write=False)


def _edges():
    """-> (check -> its first edge [84], edge -> column [522], column -> its three edges [174][3] in ascending check order)"""
    base = np.concatenate(([0], np.cumsum([len(r) for r in CHECKS]))).astype(np.int32)
    col = np.array([n for r in CHECKS for n in r], np.int32)
    of = [[] for _ in range(N)]
    for e, n in enumerate(col):
        of[n].append(e)
    return base, col, np.array(of, np.int32)


CHECK_BASE, EDGE_COL, COL_EDGES = _edges()
EDGE_CHECK = np.repeat(np.arange(M, dtype=np.int32), np.diff(CHECK_BASE))
H = np.zeros((M, N), np.uint8)                    # the parity checks as a dense matrix
H[EDGE_CHECK, EDGE_COL] = 1
for _a in (CHECK_BASE, EDGE_COL, COL_EDGES, EDGE_CHECK, H):
    _a.setflags(write=False)


def crc14(bits77):
    """The 14 CRC bits (most significant first, uint8 [14]) of 77 message bits: polynomial 0x2757, zero initial value, no
    reflection, no final XOR, over 82 bits -- the message and five zeros."""
    bits = np.asarray(bits77).astype(np.int64).reshape(-1)
    if len(bits) != MSG:
        raise ValueError(f"crc14: {len(bits)} bits, 77 expected")
    r = 0
    for b in list(bits) + [0] * 5:
        top = ((r >> 13) & 1) ^ int(b & 1)
        r = (r << 1) & 0x3FFF
        if top:
            r ^= CRC_POLY
    return np.array([(r >> (13 - i)) & 1 for i in range(CRC_BITS)], np.uint8)


def encode91(bits91):
    """91 systematic bits (message and CRC) -> the 174-bit codeword"""
    b = np.asarray(bits91).astype(np.uint8).reshape(-1) & 1
    if len(b) != K:
        raise ValueError(f"encode91: {len(b)} bits, 91 expected")
    return np.concatenate((b, (GENERATOR.astype(np.int64) @ b.astype(np.int64) % 2).astype(np.uint8)))


def encode(bits77):
    """77 message bits -> uint8 [174] in transmission order: the message, its CRC-14, 83 parity bits"""
    b = np.asarray(bits77).astype(np.uint8).reshape(-1) & 1
    return encode91(np.concatenate((b, crc14(b))))


def check(bits174):
    """True where every one of the 83 parity checks is even"""
    b = np.asarray(bits174).astype(np.int64).reshape(-1)
    if len(b) != N:
        raise ValueError(f"check: {len(b)} bits, 174 expected")
    return not ((H.astype(np.int64) @ b) % 2).any()


def crc_ok(bits91):
    b = np.asarray(bits91).astype(np.uint8).reshape(-1)
    return bool(np.array_equal(crc14(b[:MSG]), b[MSG:K]))


def unpack_bits(packed):
    """uint8 [..][12] as the decoder packs them (MSB first, 5 bits of padding) -> uint8 [..][91]"""
    return np.unpackbits(np.asarray(packed, np.uint8), axis=-1)[..., :K]


def params(iters=30, alpha=0.8125):
    """The decoder's settings as the ``_lib.LdpcCfg`` the C ABI takes."""
    return LdpcCfg(iters=int(iters), alpha=float(np.float32(alpha)))


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in LdpcCfg._fields_}


def plan(cfg):
    """What one decode call launches (no device needed): dict of threads per candidate, LDS bytes, candidates per call,
    iterations.  Raises PysdrError for a cfg outside the rules (iters in [1, 200], alpha finite and in (0, 1])."""
    v = _lib.plan_call("pysdr_ldpc_plan", 4, C.byref(cfg) if cfg is not None else None)
    return {"threads": v[0], "lds_bytes": v[1], "max_candidates": v[2], "iters": v[3]}


def osd_params(order=2):
    """The setting of ordered-statistics decoding behind min-sum as the ``_lib.OsdCfg`` the C ABI
    takes: ``order`` rows of the most reliable basis' generator are flipped at once, 0 to 2.  The CRC-14 is the stage's
    only guard: a candidate that reaches it comes out as a false message with probability about 2^-14."""
    return OsdCfg(order=int(order))


def osd_cfg(osd):
    """None, an order or an ``OsdCfg`` -> None or the ``OsdCfg``"""
    if osd is None or isinstance(osd, OsdCfg):
        return osd
    if isinstance(osd, bool) or not isinstance(osd, (int, np.integer)):
        raise ValueError(f"osd: None, an order 0 to 2 or an OsdCfg, not {osd!r}")
    return osd_params(osd)


def osd_plan(cfg):
    """What the second launch of a decode call with ``osd`` is (no device needed): dict of threads per candidate, LDS
    bytes, patterns scored, candidates per call.  Raises PysdrError for an order outside [0, 2]."""
    v = _lib.plan_call("pysdr_osd_plan", 4, C.byref(cfg) if cfg is not None else None)
    return {"threads": v[0], "lds_bytes": v[1], "patterns": v[2], "max_candidates": v[3]}
