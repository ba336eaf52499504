"""Punctured rates of the K = 7 code (PUNCTURING in include/qpsk_hip.h: qpsk_punct_ntx, qpsk_conv_encode_punct_batch,
qpsk_viterbi_punct_batch, qpsk_deframer_reset_coded_punct): what can be checked without a GPU.

The restatements below are the header's definition in numpy, in integers.  A punctured decode IS the existing decoder on the zero-filled
row, so viterbi_punct_ref is viterbi_ref (test_viterbi_cpu) behind depuncture_ref, and deframe_coded_punct_ref is deframe_coded_ref's loop
(test_deframe_coded_cpu) with the shorter body; everything they are made of is imported, not copied.  The GPU tests (test_punct_gpu.py,
test_deframe_coded_punct_gpu.py) compare the kernels with them bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_deframe_coded_cpu import cut, deframe_coded_ref, dibits_to_costas, first_word, flat, push_gain, same_packets
from test_deframe_cpu import crc16, keystream, turn
from test_rx_data_cpu import data_rule
from test_rx_ext_cpu import declared
from test_soft_cpu import quantise
from test_viterbi_cpu import OPEN_END, OPEN_START, conv_encode_ref, dibits_to_soft, pack_bits, unpack_bits, viterbi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUNCT_SYMBOLS = ("qpsk_punct_ntx", "qpsk_conv_encode_punct_batch", "qpsk_viterbi_punct_batch", "qpsk_deframer_reset_coded_punct")
QPSK_ERR_ARG = -2
NAMED = {"1/2": (1, 0x1, 0x1), "2/3": (2, 0x1, 0x3), "3/4": (3, 0x5, 0x3), "5/6": (5, 0x15, 0x0B), "7/8": (7, 0x51, 0x2F)}
PERIOD32 = (32, 0x9E3779B9, 0x7F4A7C15)              # every position of the longest period, bit 31 of keep0 set; K = 20 + 18 = 38
DELETED_STEP = (4, 0b1101, 0b1001)                  # step 1 of the period sends nothing at all; K = 5 (odd)
ALL_PATTERNS = dict(NAMED, period32=PERIOD32, deleted=DELETED_STEP)
BAD_PATTERNS = [(0, 1, 1), (33, 1, 1), (3, 0x8, 0x1), (3, 0x1, 0x8), (32, 0, 0), (5, 0, 0), (-1, 1, 1)]
ALL_FLAGS = (0, OPEN_START, OPEN_END, OPEN_START | OPEN_END)


def popc(v):
    return bin(int(v)).count("1")


# ------------------------------------------------------------------- the numpy restatement
def punct_index(t, pattern):
    """the header's formula: (idx(t, 0), idx(t, 1)) for an int or an array of steps"""
    period, keep0, keep1 = pattern
    t = np.asarray(t, np.int64)
    r = t % period
    pc0 = np.array([popc(keep0 & ((1 << k) - 1)) for k in range(period)], np.int64)
    pc1 = np.array([popc(keep1 & ((1 << k) - 1)) for k in range(period)], np.int64)
    i0 = (t // period) * (popc(keep0) + popc(keep1)) + pc0[r] + pc1[r]
    return i0, i0 + ((keep0 >> r) & 1)


def punct_nsent(nsteps, pattern):
    return int(punct_index(nsteps, pattern)[0])


def punct_ntx(nsteps, pattern):
    return (punct_nsent(nsteps, pattern) + 1) // 2


def sent_mask(nsteps, pattern):
    """(nsteps, 2) bool: is coded bit j of step t sent"""
    period, keep0, keep1 = pattern
    r = np.arange(nsteps) % period
    return np.stack([(keep0 >> r) & 1, (keep1 >> r) & 1], axis=1).astype(bool)


def sent_positions(nsteps, pattern):
    """(nsteps, 2) int64: idx(t, j), meaningful where sent_mask is set"""
    return np.stack(punct_index(np.arange(nsteps), pattern), axis=1)


def puncture_ref(dibits, pattern):
    """coded dibits (R, nsteps) c0 | c1 << 1 -> transmitted dibits (R, ntx): sent bit k on bit k & 1 of dibit k >> 1, the pad bit 0"""
    d = np.atleast_2d(np.asarray(dibits, np.uint8))
    n = d.shape[1]
    m, at = sent_mask(n, pattern), sent_positions(n, pattern)
    flat_bits = np.zeros((d.shape[0], 2 * punct_ntx(n, pattern)), np.uint8)
    c = np.stack([d & 1, d >> 1], axis=-1)
    flat_bits[:, at[m]] = c[:, m]
    return (flat_bits[:, 0::2] | (flat_bits[:, 1::2] << 1)).astype(np.uint8)


def depuncture_ref(soft, nsteps, pattern, flip=None):
    """soft (R, ntx or more, 2) int8 as transmitted -> (R, nsteps, 2) int8: -128 taken as -127, v(k) negated iff bit k & 1 of
    flip[k >> 1], and 0 wherever nothing was sent"""
    s = np.asarray(soft, np.int8)
    v = np.maximum(s.reshape(s.shape[0], -1).astype(np.int64), -127)
    if flip is not None:
        f = np.asarray(flip, np.uint8).astype(np.int64)
        fb = np.stack([f & 1, (f >> 1) & 1], axis=-1).reshape(-1)
        v = v.copy()
        v[:, :len(fb)] = np.where(fb, -v[:, :len(fb)], v[:, :len(fb)])
    m, at = sent_mask(nsteps, pattern), sent_positions(nsteps, pattern)
    out = np.zeros((s.shape[0], nsteps, 2), np.int8)
    out[:, m] = v[:, at[m]]
    return out


def conv_encode_punct_ref(bits_packed, nbits, pattern, tail=True):
    return puncture_ref(conv_encode_ref(bits_packed, nbits, tail=tail), pattern)


def viterbi_punct_ref(soft, nsteps, pattern, flip=None, flags=0):
    """the definition: the existing decoder, d_flip NULL, on the zero-filled row"""
    return viterbi_ref(depuncture_ref(soft, nsteps, pattern, flip), flip=None, flags=flags)


def coded_punct_steps(nbytes):
    return 8 * (nbytes + 2) + 6


def deframe_coded_punct_ref(pushes, gains, sync, min_score, nbytes, pattern, mode="unit", scale=64.0):
    """deframe_coded_ref with a punctured body: Nc = ntx(8 (nbytes + 2) + 6) dibits on air, HUNT / SOFT / GAIN with that Nc, DECODE =
    viterbi_punct_ref on the Nc soft pairs with the keystream over the transmitted dibits.  One stream; arguments and result as
    deframe_coded_ref's (soft is (Nc, 2))"""
    pushes = [np.asarray(p, np.float32).reshape(-1, 2) for p in pushes]
    z = np.concatenate(pushes)
    D = data_rule(z)
    ends = np.cumsum([len(p) for p in pushes])
    g_push = np.array([push_gain(p, mode, scale) if gains is None else np.float32(gains[k]) for k, p in enumerate(pushes)], np.float32)
    g_sym = np.repeat(g_push, [len(p) for p in pushes])
    nsteps = coded_punct_steps(nbytes)
    n, Nc = len(sync), punct_ntx(nsteps, pattern)
    ks = keystream(Nc)
    out = [[] for _ in pushes]
    h = 0
    while True:
        w = first_word(D, h, sync, min_score)
        if w is None or w[0] + n + Nc > len(D):
            break
        p, r, score = w
        x, g = z[p + n:p + n + Nc], g_sym[p + n:p + n + Nc]
        a, b = x[:, 0], x[:, 1]
        u, v = ((a, b), (b, -a), (-a, -b), (-b, a))[r]
        soft = np.stack([quantise(u, g), quantise(v, g)], axis=1)
        dec = viterbi_punct_ref(soft[None], nsteps, pattern, flip=ks)
        byts = dec["bits"][0][:nbytes + 2]
        ok = crc16(byts[:nbytes]) == (int(byts[nbytes]) << 8 | int(byts[nbytes + 1]))
        h = p + n + Nc
        out[int(np.searchsorted(ends, h))].append(dict(pos=p, rot=r, score=score, bytes=byts, crc_ok=bool(ok), info=dec["info"][0], end=h,
                                                       soft=soft))
    return out


def make_coded_punct_packet(rng, sync, nbytes, pattern, corrupt=False):
    """[sync][keystream xor conv_encode_punct(payload + CRC-16 big-endian, tail)] as dibits -> (dibits, payload)"""
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
    crc = crc16(payload) ^ (1 if corrupt else 0)
    packet = np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])
    body = conv_encode_punct_ref(packet[None, :], 8 * len(packet), pattern, tail=True)[0]
    return np.concatenate([np.asarray(sync, np.uint8), body ^ keystream(len(body))]).astype(np.uint8), payload


# ------------------------------------------------------------------- 1. the numbering
def brute_force_positions(nsteps, pattern):
    """the sent bits enumerated in the order (t, j): {(t, j): k}, and their number"""
    period, keep0, keep1 = pattern
    pos, k = {}, 0
    for t in range(nsteps):
        for j, keep in ((0, keep0), (1, keep1)):
            if (keep >> (t % period)) & 1:
                pos[(t, j)] = k
                k += 1
    return pos, k


@pytest.mark.parametrize("name", sorted(ALL_PATTERNS))
def test_punct_index_equals_a_brute_force_enumeration(name):
    pattern = ALL_PATTERNS[name]
    pos, _ = brute_force_positions(200, pattern)
    i0, i1 = punct_index(np.arange(201), pattern)
    for (t, j), k in pos.items():
        assert (i0, i1)[j][t] == k, (name, t, j)
    for nsteps in range(1, 201):
        want = sum(1 for (t, _) in pos if t < nsteps)
        assert punct_nsent(nsteps, pattern) == want and punct_ntx(nsteps, pattern) == (want + 1) // 2, (name, nsteps)
    m = sent_mask(200, pattern)
    assert {(t, j) for t in range(200) for j in range(2) if m[t, j]} == set(pos)
    if name == "deleted":
        assert not m[1].any() and m[0].all()                             # a step with nothing sent, and the pattern's K is odd
    if name == "1/2":
        assert np.array_equal(i0, 2 * np.arange(201)) and np.array_equal(i1, i0 + 1)


def test_named_rates_are_what_their_names_say():
    for name, (period, keep0, keep1) in NAMED.items():
        num, den = (int(v) for v in name.split("/"))
        assert period == num and popc(keep0) + popc(keep1) == den, name
    # the header's macros and the Python dict carry the same numbers
    import re
    import qpsk_amd
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    for name, pattern in NAMED.items():
        m = re.search(r"#define QPSK_PUNCT_%s\s+(\w+),\s*(\w+),\s*(\w+)" % name.replace("/", "_"), header)
        assert m and tuple(int(v.rstrip("uU"), 0) for v in m.groups()) == pattern, name
        assert tuple(qpsk_amd.PUNCTURE[name]) == pattern, name
    assert sorted(qpsk_amd.PUNCTURE) == sorted(NAMED)


# ------------------------------------------------------------------- 2. ABI (fails without the feature)
def test_punct_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import torch
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in PUNCT_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "PUNCTURING" in header and "NOT reproduced" in header          # the DVB I/Q mapping is not the definition, and it says so
    assert callable(getattr(qpsk_amd.Modem, "punct_ntx", None))
    import inspect
    for name in ("conv_encode", "viterbi", "deframer_reset_coded"):
        assert inspect.signature(getattr(qpsk_amd.Modem, name)).parameters["puncture"].default is None, name
    buf = (C.c_uint8 * 64)()
    assert qpsk_lib.qpsk_conv_encode_punct_batch(None, buf, 1, 8, 1, 3, 5, 3, buf) == QPSK_ERR_ARG
    assert b"qpsk_conv_encode_punct_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_viterbi_punct_batch(None, buf, 0, 1, 8, 3, 5, 3, None, 0, buf, None) == QPSK_ERR_ARG
    assert b"qpsk_viterbi_punct_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_deframer_reset_coded_punct(None, 1, buf, 16, 16, 4, 1, 0, 64.0, 3, 5, 3) == QPSK_ERR_ARG
    assert b"qpsk_deframer_reset_coded_punct" in qpsk_lib.qpsk_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(qpsk_amd.QpskError):
            qpsk_amd.Modem().viterbi(np.zeros((1, 6, 2), np.int8), nsteps=8, puncture="3/4")


def test_qpsk_punct_ntx_equals_the_formula_and_refuses_bad_patterns(qpsk_lib):
    for name, pattern in ALL_PATTERNS.items():
        for nsteps in list(range(1, 201)) + [8200, 131072]:
            assert qpsk_lib.qpsk_punct_ntx(nsteps, *pattern) == punct_ntx(nsteps, pattern), (name, nsteps)
    for bad in BAD_PATTERNS:
        assert qpsk_lib.qpsk_punct_ntx(100, *bad) == QPSK_ERR_ARG, bad
        assert b"qpsk_punct_ntx" in qpsk_lib.qpsk_last_error()
    for nsteps in (0, -5, 131073):
        assert qpsk_lib.qpsk_punct_ntx(nsteps, 3, 5, 3) == QPSK_ERR_ARG, nsteps
    assert qpsk_lib.qpsk_punct_ntx(1, 2, 0x2, 0x2) == 0                  # step 0 sends nothing: a legal pattern, and nothing on air


# ------------------------------------------------------------------- 3. the restatement on hand cases
def test_puncture_and_depuncture_hand_cases():
    # rate 3/4: X 101, Y 110 -> of steps 0, 1, 2 the bits c0(0) c1(0) c1(1) c0(2) are sent, in that order
    d = np.array([[0b01, 0b10, 0b01, 0b11]], np.uint8)                    # (c0, c1) = (1,0) (0,1) (1,0) (1,1)
    tx = puncture_ref(d, NAMED["3/4"])
    assert punct_nsent(4, NAMED["3/4"]) == 6 and tx.shape == (1, 3)
    sent = [1, 0, 1, 1, 1, 1]                                           # c0(0) c1(0) c1(1) c0(2) | c0(3) c1(3)
    assert tx[0].tolist() == [sent[0] | sent[1] << 1, sent[2] | sent[3] << 1, sent[4] | sent[5] << 1]
    # an odd number of sent bits: the pad bit is 0 and its soft value is never read
    assert punct_nsent(3, NAMED["2/3"]) == 5
    tx = puncture_ref(np.array([[3, 3, 3]], np.uint8), NAMED["2/3"])
    assert tx[0].tolist() == [3, 3, 1]
    soft = np.array([[[10, -20], [30, -128], [-50, 99]]], np.int8)
    z = depuncture_ref(soft, 3, NAMED["2/3"])
    assert z[0].tolist() == [[10, -20], [0, 30], [-127, -50]]
    z = depuncture_ref(soft, 3, NAMED["2/3"], flip=np.array([1, 2, 3], np.uint8))
    assert z[0].tolist() == [[-10, -20], [0, 30], [127, 50]]
    other = soft.copy()
    other[0, 2, 1] = -7
    assert np.array_equal(depuncture_ref(other, 3, NAMED["2/3"]), depuncture_ref(soft, 3, NAMED["2/3"]))
    # (1, 1, 1) is no puncturing at all
    rng = np.random.default_rng(1)
    s = rng.integers(-128, 128, (3, 50, 2)).astype(np.int8)
    key = rng.integers(0, 4, 50).astype(np.uint8)
    a, b = viterbi_punct_ref(s, 50, NAMED["1/2"], flip=key, flags=OPEN_END), viterbi_ref(s, flip=key, flags=OPEN_END)
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["info"], b["info"])
    assert np.array_equal(puncture_ref(key[None], NAMED["1/2"]), key[None])


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("name", sorted(NAMED))
def test_noise_free_rows_decode_to_themselves(name, flags, oracle):
    """every named pattern, with and without d_flip, all four flag values.  As in test_viterbi_cpu, an open start takes the longer rows
    only and rows without a tail need the open end"""
    pattern = NAMED[name]
    rng = np.random.default_rng(70 + flags)
    for nbits in (63, 64, 65, 200) if flags & OPEN_START else (1, 2, 7, 8, 63, 64, 65, 200):
        bits = rng.integers(0, 2, (5, nbits), dtype=np.uint8)
        for tail in (True, False):
            if not tail and not flags & OPEN_END:
                continue
            n = nbits + (6 if tail else 0)
            tx = conv_encode_punct_ref(pack_bits(bits), nbits, pattern, tail=tail)
            assert tx.shape[1] == punct_ntx(n, pattern)
            key = oracle.scramble_stream(np.zeros(tx.shape[1], np.uint8))
            for flip in (None, key):
                sent = tx if flip is None else tx ^ key[None, :]
                got = viterbi_punct_ref(dibits_to_soft(sent), n, pattern, flip=flip, flags=flags)
                if tail or nbits >= 63:                                  # a short row without a tail: its last bits have too few sent bits behind them
                    assert np.array_equal(unpack_bits(got["bits"], n)[:, :nbits], bits), (name, nbits, tail, flip is None)
                assert np.all(got["info"][:, 0] == 64 * punct_nsent(n, pattern)) and not got["info"][:, 3].any()


# ------------------------------------------------------------------- 4. the deframer's restatement
def punct_stream(rng, sync, nbytes, pattern, npackets, amp=0.8, noise=0.2, bad=()):
    """dibit stream with packets at random gaps (every third back to back) and rotations -> (costas (n, 2) float32, [position])"""
    parts, at = [], []
    for q in range(npackets):
        parts.append(rng.integers(0, 4, 0 if q % 3 == 1 else int(rng.integers(1, 50)), dtype=np.uint8))
        pkt, _ = make_coded_punct_packet(rng, sync, nbytes, pattern, corrupt=q in bad)
        at.append(sum(len(p) for p in parts))
        parts.append(turn(pkt, q & 3))
    parts.append(rng.integers(0, 4, 9, dtype=np.uint8))
    return dibits_to_costas(np.concatenate(parts), amp=amp, noise=noise, rng=rng), at


def test_deframe_coded_punct_ref_with_1_1_1_equals_deframe_coded_ref_on_a_random_cut_stream():
    rng = np.random.default_rng(31)
    nbytes, sync = 5, rng.integers(0, 4, 24, dtype=np.uint8)
    z, at = punct_stream(rng, sync, nbytes, NAMED["1/2"], 7, noise=0.3, bad=(2,))
    sizes = []
    while sum(sizes) < len(z):
        sizes.append(int(rng.choice([1, 3, 50, 170, int(rng.integers(1, 300))])))
    rows = cut(z, sizes[:-1])
    for gains in (None, rng.uniform(20.0, 90.0, len(rows)).astype(np.float32)):
        a = deframe_coded_punct_ref(rows, gains, sync, 21, nbytes, NAMED["1/2"])
        b = deframe_coded_ref(rows, gains, sync, 21, nbytes)
        assert [len(p) for p in a] == [len(p) for p in b]
        assert same_packets(flat(a), flat(b)) and [p["pos"] for p in flat(a)] == at
        assert [p["crc_ok"] for p in flat(a)] == [q != 2 for q in range(7)]


@pytest.mark.parametrize("name", ["2/3", "3/4", "5/6", "7/8"])
def test_punctured_packets_come_back_whatever_the_cuts(name):
    """with a constant gain the packets do not depend on the cuts; nbytes = 5 gives 62 steps, an odd nsent = 93 at rate 2/3"""
    pattern = NAMED[name]
    rng = np.random.default_rng(32)
    nbytes, sync = 5, rng.integers(0, 4, 20, dtype=np.uint8)
    Nc = punct_ntx(coded_punct_steps(nbytes), pattern)
    assert (name, Nc) in (("2/3", 47), ("3/4", 42), ("5/6", 38), ("7/8", 36))
    z, at = punct_stream(rng, sync, nbytes, pattern, 5, noise=0.12, bad=(3,))
    whole = deframe_coded_punct_ref([z], [70.0], sync, 18, nbytes, pattern)[0]
    assert [p["pos"] for p in whole] == at and [p["crc_ok"] for p in whole] == [True, True, True, False, True]
    assert [p["end"] - p["pos"] for p in whole] == [20 + Nc] * 5
    for sizes in ([1] * len(z), [17] * 40, [7, 1, 1, 100, 2, 64]):
        rows = cut(z, sizes)
        assert same_packets(flat(deframe_coded_punct_ref(rows, [70.0] * len(rows), sync, 18, nbytes, pattern)), whole), sizes


# ------------------------------------------------------------------- 5. it still corrects what hard decisions cannot
LINK = dict(rows=16, nbits=528, amp=64.0, sigma=28.0, seed=2054)


def punct_link(name):
    """16 rows of 528 random bits + tail, coded and punctured, sent at +-64 with Gaussian noise of sigma 28, clipped and rounded to int8
    -> (bits, soft (16, ntx, 2), the sent values' signs as 0 / 1, nsteps)"""
    k, pattern = LINK, NAMED[name]
    rng = np.random.default_rng(k["seed"])
    bits = rng.integers(0, 2, (k["rows"], k["nbits"]), dtype=np.uint8)
    tx = conv_encode_punct_ref(pack_bits(bits), k["nbits"], pattern)
    sent = np.stack([tx & 1, tx >> 1], axis=-1)
    x = k["amp"] * (1.0 - 2.0 * sent) + k["sigma"] * rng.standard_normal(sent.shape)
    return bits, np.clip(np.rint(x), -127, 127).astype(np.int8), sent, k["nbits"] + 6


@pytest.mark.parametrize("name", ["2/3", "3/4", "5/6", "7/8"])
def test_punctured_rows_decode_clean_where_hard_decisions_fail(name):
    """16 rows of 528 bits + tail at +-64 with Gaussian noise sigma = 28 (seed 2054; the same bits and one noise draw per rate).
    Asserted: every coded row decodes to its bits, while hard decisions on the first 528 sent values -- what an uncoded link of the
    same payload would have to get right -- are wrong somewhere in at least half of the rows.
    Observed with this seed (rows decoded clean / rows whose hard decisions fail, of 16): 2/3 -> 16 / 16, 3/4 -> 16 / 16,
    5/6 -> 16 / 16, 7/8 -> 16 / 16; the decoder counts 4 .. 11, 4 .. 12, 4 .. 10 and 1 .. 9 channel bit errors per row of 801, 712, 641 and
    611 sent bits."""
    bits, soft, sent, nsteps = punct_link(name)
    got = viterbi_punct_ref(soft, nsteps, NAMED[name])
    clean = int((unpack_bits(got["bits"], nsteps)[:, :LINK["nbits"]] == bits).all(axis=1).sum())
    flat_soft, flat_sent = soft.reshape(len(soft), -1)[:, :LINK["nbits"]], sent.reshape(len(sent), -1)[:, :LINK["nbits"]]
    hard_fail = int((((flat_soft < 0).astype(np.uint8) != flat_sent) | (flat_soft == 0)).any(axis=1).sum())
    print("rate %s sigma %g: clean %d / %d, hard failures %d / %d, channel bit errors %d .. %d of %d"
          % (name, LINK["sigma"], clean, LINK["rows"], hard_fail, LINK["rows"], got["info"][:, 3].min(), got["info"][:, 3].max(),
             punct_nsent(nsteps, NAMED[name])))
    assert clean == LINK["rows"], clean
    assert hard_fail >= LINK["rows"] // 2, hard_fail
    assert not got["info"][:, 1].any() and not got["info"][:, 2].any()
