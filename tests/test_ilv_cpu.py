"""The bit interleaver of the coded packet path (INTERLEAVING in include/qpsk_hip.h: qpsk_ilv_stride, qpsk_conv_encode_ilv_batch,
qpsk_viterbi_ilv_batch, qpsk_frame_batch_ilv, qpsk_deframer_reset_coded_ilv): what can be checked without a GPU.

The restatements below are the header's definition in numpy, in integers, on top of the ones the punctured code already has: an
interleaved decode IS the punctured decoder on the row gathered through pi, so viterbi_ilv_ref is viterbi_ref behind depuncture_ref
behind one gather, and frame_ilv_ref / deframe_coded_ilv_ref are frame_ref / deframe_coded_punct_ref with the body permuted; everything
they are made of is imported, not copied.  The GPU tests (test_ilv_gpu.py) compare the kernels with them bit for bit.
"""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from test_deframe_coded_cpu import cut, dibits_to_costas, flat, same_packets
from test_deframe_cpu import crc16, turn
from test_frame_cpu import HALF, body_len, frame_ref, ks_prefix, starts
from test_punct_cpu import (ALL_FLAGS, DELETED_STEP, NAMED, PERIOD32, coded_punct_steps, conv_encode_punct_ref, deframe_coded_punct_ref,
                            depuncture_ref, punct_nsent, punct_ntx, viterbi_punct_ref)
from test_rx_ext_cpu import declared
from test_viterbi_cpu import OPEN_END, OPEN_START, dibits_to_soft, pack_bits, unpack_bits, viterbi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILV_SYMBOLS = ("qpsk_ilv_stride", "qpsk_conv_encode_ilv_batch", "qpsk_viterbi_ilv_batch", "qpsk_frame_batch_ilv", "qpsk_deframer_reset_coded_ilv")
QPSK_ERR_ARG = -2
ILV_PATTERNS = dict(NAMED, period32=PERIOD32)


# ------------------------------------------------------------------- the numpy restatement
def ilv_valid(n, s):
    """STRIDE: 1 <= s < max(n, 2) and gcd(s, n) = 1"""
    return n >= 2 and n % 2 == 0 and 1 <= s < max(n, 2) and math.gcd(s, n) == 1


def ilv_perm(n, s):
    """pi: (n,) int64, pi[k] = (k s) mod n, the on-air place of sent bit k"""
    if not ilv_valid(n, s):
        raise ValueError("stride %d is not a stride of %d bits" % (s, n))
    return (np.arange(n, dtype=np.int64) * int(s)) % n


def ilv_stride(nbits, want):
    """qpsk_ilv_stride: the smallest s >= min(want, nbits - 1) coprime to nbits"""
    s = min(want, nbits - 1)
    while math.gcd(s, nbits) != 1:
        s += 1
    return s


def strides_for(n):
    """the strides the tests take for a row of n bits: 1, 3 (the next coprime one where 3 divides n), the recommended one, n - 1"""
    return sorted({1, ilv_stride(n, 3), ilv_stride(n, max(1, n // 16)), n - 1} if n > 2 else {1})


def flat_bits(dibits):
    """(R, ntx) dibits -> (R, 2 ntx) bits, bit k on bit k & 1 of dibit k >> 1"""
    d = np.atleast_2d(np.asarray(dibits, np.uint8))
    return np.stack([d & 1, d >> 1], axis=-1).reshape(d.shape[0], -1)


def interleave_ref(tx, nsent, s):
    """ENCODER: transmitted dibits (R, ntx) in sent order -> on-air dibits (R, ntx): on-air bit pi(k) = sent bit k for k < nsent, every
    other on-air bit -- the pad's place pi(nsent) of an odd nsent -- 0"""
    b = flat_bits(tx)
    pi = ilv_perm(b.shape[1], s)
    air = np.zeros_like(b)
    air[:, pi[:nsent]] = b[:, :nsent]
    return (air[:, 0::2] | (air[:, 1::2] << 1)).astype(np.uint8)


def gather_ref(soft, ntx, s, flip=None):
    """the host's gather of identity (1): soft (R, ntx or more, 2) as on air -> (row' (R, ntx, 2) with row'[k] = row[pi(k)] over the flat
    numbers, flip' (ntx,) with the flip bits gathered the same way, or None)"""
    q = np.asarray(soft, np.int8)
    pi = ilv_perm(2 * ntx, s)
    rows = q.reshape(q.shape[0], -1)[:, pi].reshape(q.shape[0], ntx, 2)
    if flip is None:
        return rows, None
    fb = flat_bits(np.asarray(flip, np.uint8)[None, :ntx])[0][pi]
    return rows, (fb[0::2] | (fb[1::2] << 1)).astype(np.uint8)


def conv_encode_ilv_ref(bits_packed, nbits, pattern, s, tail=True):
    nsteps = nbits + (6 if tail else 0)
    return interleave_ref(conv_encode_punct_ref(bits_packed, nbits, pattern, tail=tail), punct_nsent(nsteps, pattern), s)


def viterbi_ilv_ref(soft, nsteps, pattern, s, flip=None, flags=0):
    """DECODER INPUT, literally: v(a) after the -128 rule, negated by flip over the on-air dibits; s_j = sent ? v(pi(idx(t, j))) : 0; then
    the existing decoder with d_flip NULL"""
    q = np.asarray(soft, np.int8)
    ntx = punct_ntx(nsteps, pattern)
    v = np.maximum(q.reshape(q.shape[0], -1)[:, :2 * ntx].astype(np.int64), -127)
    if flip is not None:
        v = np.where(flat_bits(np.asarray(flip, np.uint8)[None, :ntx])[0], -v, v)
    g = v[:, ilv_perm(2 * ntx, s)].astype(np.int8).reshape(q.shape[0], ntx, 2)
    return viterbi_ref(depuncture_ref(g, nsteps, pattern), flip=None, flags=flags)


def frame_ilv_ref(payloads, sync, coded, pattern, per_row, lead, gap, row_len, stride, plain=None):
    """frame_ref with the coded body's bits spread by the stride (uncoded: stride 1 only); plain: what frame_ref returns for the same
    arguments, where the caller has it already (it is left as it is)"""
    rows, crcs = frame_ref(payloads, sync, coded, pattern, per_row, lead, gap, row_len) if plain is None else (plain[0].copy(), plain[1])
    if not coded:
        assert stride == 1
        return rows, crcs
    pattern = HALF if pattern is None else pattern
    nbytes = np.asarray(payloads).shape[1]
    B, nsent = body_len(nbytes, True, pattern), punct_nsent(coded_punct_steps(nbytes), pattern)
    ks = ks_prefix(B)
    for r in range(rows.shape[0]):
        for at in starts(len(sync), nbytes, True, pattern, per_row, lead, gap):
            body = rows[r, at + len(sync):at + len(sync) + B]
            body[:] = interleave_ref((body ^ ks)[None], nsent, stride)[0] ^ ks
    return rows, crcs


def deframe_coded_ilv_ref(pushes, gains, sync, min_score, nbytes, pattern, stride, mode="unit", scale=64.0):
    """deframe_coded_punct_ref with DECODE = viterbi_ilv_ref: the hunt, the soft rows and the gains never look at a decoder's result, so
    its packets are taken as they are and decoded again through the stride"""
    out = deframe_coded_punct_ref(pushes, gains, sync, min_score, nbytes, pattern, mode=mode, scale=scale)
    nsteps = coded_punct_steps(nbytes)
    ks = ks_prefix(punct_ntx(nsteps, pattern))
    for p in flat(out):
        dec = viterbi_ilv_ref(p["soft"][None], nsteps, pattern, stride, flip=ks)
        byts = dec["bits"][0][:nbytes + 2]
        p.update(bytes=byts, info=dec["info"][0], crc_ok=bool(crc16(byts[:nbytes]) == (int(byts[nbytes]) << 8 | int(byts[nbytes + 1]))))
    return out


def make_coded_ilv_packet(rng, sync, nbytes, pattern, stride, corrupt=False):
    """[sync][keystream xor conv_encode_ilv(payload + CRC-16 big-endian, tail)] as dibits -> (dibits, payload)"""
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
    crc = crc16(payload) ^ (1 if corrupt else 0)
    packet = np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])
    body = conv_encode_ilv_ref(packet[None, :], 8 * len(packet), pattern, stride, tail=True)[0]
    return np.concatenate([np.asarray(sync, np.uint8), body ^ ks_prefix(len(body))]).astype(np.uint8), payload


def ilv_stream(rng, sync, nbytes, pattern, stride, npackets, amp=0.8, noise=0.2, bad=()):
    """test_punct_cpu.punct_stream with interleaved bodies: packets at random gaps (every third back to back) and rotations"""
    parts, at = [], []
    for q in range(npackets):
        parts.append(rng.integers(0, 4, 0 if q % 3 == 1 else int(rng.integers(1, 50)), dtype=np.uint8))
        pkt, _ = make_coded_ilv_packet(rng, sync, nbytes, pattern, stride, corrupt=q in bad)
        at.append(sum(len(p) for p in parts))
        parts.append(turn(pkt, q & 3))
    parts.append(rng.integers(0, 4, 9, dtype=np.uint8))
    return dibits_to_costas(np.concatenate(parts), amp=amp, noise=noise, rng=rng), at


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_ilv_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in ILV_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "INTERLEAVING" in header
    not_built = header[header.index("Not built: a"):]
    assert "interleaving" not in not_built[:not_built.index(";")]            # FRAMER no longer lists it among what is missing
    assert callable(getattr(qpsk_amd, "ilv_stride", None))
    for name in ("conv_encode", "viterbi", "deframer_reset_coded", "frame"):
        assert inspect.signature(getattr(qpsk_amd.Modem, name)).parameters["interleave"].default is None, name
    buf = (C.c_uint8 * 64)()
    assert qpsk_lib.qpsk_conv_encode_ilv_batch(None, buf, 1, 8, 1, 1, 1, 1, 3, buf) == QPSK_ERR_ARG
    assert b"qpsk_conv_encode_ilv_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_viterbi_ilv_batch(None, buf, 0, 1, 8, 1, 1, 1, 3, None, 0, buf, None) == QPSK_ERR_ARG
    assert b"qpsk_viterbi_ilv_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_frame_batch_ilv(None, buf, 0, 1, 1, 4, buf, 16, 1, 1, 1, 1, 3, 0, 0, 200, buf, None) == QPSK_ERR_ARG
    assert b"qpsk_frame_batch_ilv" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_deframer_reset_coded_ilv(None, 1, buf, 16, 16, 4, 1, 0, 64.0, 1, 1, 1, 3) == QPSK_ERR_ARG
    assert b"qpsk_deframer_reset_coded_ilv" in qpsk_lib.qpsk_last_error()


# ------------------------------------------------------------------- 2. strides and the permutation
def test_qpsk_ilv_stride_equals_a_brute_force_search_and_refuses_bad_arguments(qpsk_lib):
    import qpsk_amd
    for nbits in range(2, 601):
        for want in (1, 2, 3, nbits // 16 + 1, nbits // 2, nbits - 1, nbits, nbits + 7, 10 ** 6):
            brute = next(s for s in range(min(want, nbits - 1), nbits) if math.gcd(s, nbits) == 1)
            got = qpsk_lib.qpsk_ilv_stride(nbits, want)
            assert got == brute == ilv_stride(nbits, want), (nbits, want, got)
            assert nbits % 2 or ilv_valid(nbits, got), (nbits, want)
    assert qpsk_lib.qpsk_ilv_stride(524, 32) == 33 and qpsk_lib.qpsk_ilv_stride(1 << 18, 1 << 17) == (1 << 17) + 1
    assert qpsk_amd.ilv_stride(524, 524 // 16) == 33
    for nbits, want in ((1, 1), (0, 1), (-4, 1), (8, 0), (8, -1)):
        assert qpsk_lib.qpsk_ilv_stride(nbits, want) == QPSK_ERR_ARG, (nbits, want)
        assert b"qpsk_ilv_stride" in qpsk_lib.qpsk_last_error()
    with pytest.raises(qpsk_amd.QpskError):
        qpsk_amd.ilv_stride(1, 1)


def test_ilv_perm_is_a_permutation_for_every_valid_stride_and_each_bad_class_is_refused():
    for n in list(range(2, 130, 2)) + [524, 1 << 18]:
        for s in (range(1, n) if n < 130 else (1, 33, n // 2 + 1, n - 1)):
            if not ilv_valid(n, s):
                continue
            pi = ilv_perm(n, s)
            assert np.array_equal(np.sort(pi), np.arange(n)), (n, s)
            assert pi[0] == 0 and (n == 2 or pi[1] == s)
            if s == 1:
                assert np.array_equal(pi, np.arange(n))
    pi = ilv_perm(1 << 18, (1 << 18) - 1)                                     # the product needs more than 32 bits
    assert pi[(1 << 18) - 1] == 1 and pi[1 << 17] == 1 << 17
    for n, s in ((524, 0), (524, -3), (524, 2), (524, 524), (524, 525), (524, 131), (6, 3), (2, 2), (2, 3), (0, 1)):   # 0, negative, even, >= n, not coprime
        with pytest.raises(ValueError):
            ilv_perm(n, s)
    assert ilv_perm(2, 1).tolist() == [0, 1]


# ------------------------------------------------------------------- 3. hand cases
def test_hand_cases_six_bits_stride_five_and_an_odd_nsent_with_its_pad_written_out():
    # n = 6, s = 5: pi = 0 5 4 3 2 1, so the row on air is sent bits 0 5 4 3 2 1
    assert ilv_perm(6, 5).tolist() == [0, 5, 4, 3, 2, 1]
    sent = [1, 0, 0, 1, 1, 1]
    tx = np.array([[sent[0] | sent[1] << 1, sent[2] | sent[3] << 1, sent[4] | sent[5] << 1]], np.uint8)
    air = interleave_ref(tx, 6, 5)
    on_air = [sent[0], sent[5], sent[4], sent[3], sent[2], sent[1]]
    assert air[0].tolist() == [on_air[0] | on_air[1] << 1, on_air[2] | on_air[3] << 1, on_air[4] | on_air[5] << 1]
    soft = np.array([[[10, -20], [30, -128], [-50, 99]]], np.int8)
    rows, key = gather_ref(soft, 3, 5, flip=np.array([1, 2, 0], np.uint8))      # flip bits on air: 1 0 | 0 1 | 0 0
    assert rows[0].reshape(-1).tolist() == [10, 99, -50, -128, 30, -20]
    assert flat_bits(key[None])[0].tolist() == [1, 0, 0, 1, 0, 0]
    # DELETED_STEP over four steps: the sent bits are c0(0) c1(0) c0(2) c0(3) c1(3) = k 0 .. 4, nsent = 5, ntx = 3, n = 6
    assert punct_nsent(4, DELETED_STEP) == 5 and punct_ntx(4, DELETED_STEP) == 3
    bits = np.array([[1, 0, 1, 1]], np.uint8)
    tx = conv_encode_punct_ref(pack_bits(bits), 4, DELETED_STEP, tail=False)
    k = flat_bits(tx)[0].tolist()
    assert k[5] == 0                                                         # in sent order the pad is the last bit
    air = flat_bits(conv_encode_ilv_ref(pack_bits(bits), 4, DELETED_STEP, 5, tail=False))[0].tolist()
    assert air == [k[0], 0, k[4], k[3], k[2], k[1]]                          # pi(5) = 25 mod 6 = 1: the pad rides on on-air bit 1
    full = np.array([[3, 3, 3]], np.uint8)
    assert flat_bits(interleave_ref(full, 5, 5))[0].tolist() == [1, 0, 1, 1, 1, 1]      # a set bit in the pad's place is not sent
    # the decoder never reads on-air number 1
    soft = np.array([[[64, 17], [-64, 64], [-64, 64]]], np.int8)
    other = soft.copy()
    other[0, 0, 1] = -128
    a, b = (viterbi_ilv_ref(q, 4, DELETED_STEP, 5, flags=OPEN_END) for q in (soft, other))
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["info"], b["info"])
    changed = soft.copy()
    changed[0, 0, 0] = -64                                                   # on-air number 0 = sent bit 0 is read
    assert not np.array_equal(viterbi_ilv_ref(changed, 4, DELETED_STEP, 5, flags=OPEN_END)["info"], a["info"])


# ------------------------------------------------------------------- 4. the round trip, noise-free
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("name", sorted(ILV_PATTERNS))
def test_noise_free_rows_decode_to_themselves_through_every_stride(name, flags):
    """every named pattern and PERIOD32, with and without d_flip, all four flag values, the strides of strides_for().  As in test_punct_cpu
    an open start takes the longer rows only and rows without a tail need the open end.  Asserted for every case: the interleaved round
    trip gives, in bits and in all four info words, what the punctured round trip of the same bits gives (stride 1 IS that twin), the
    end metric is 64 nsent and no channel error is counted.  Asserted for the named patterns: that is the sent bits.  PERIOD32 is a
    pattern chosen for its bit positions, not a code: behind an open start its first bits, and without a tail its last ones, are not
    determined by a noise-free row (the punctured decoder of test_punct_cpu returns other bits of equal metric there), so for it the
    sent bits are asserted for rows with a tail from the closed start only"""
    pattern = ILV_PATTERNS[name]
    rng = np.random.default_rng(170 + flags)
    for nbits in (63, 200) if flags & OPEN_START else (8, 63, 200):
        bits = rng.integers(0, 2, (3, nbits), dtype=np.uint8)
        for tail in (True, False):
            if not tail and not flags & OPEN_END:
                continue
            n = nbits + (6 if tail else 0)
            ntx, nsent = punct_ntx(n, pattern), punct_nsent(n, pattern)
            key = ks_prefix(ntx)
            plain = conv_encode_punct_ref(pack_bits(bits), nbits, pattern, tail=tail)
            twin = viterbi_punct_ref(dibits_to_soft(plain), n, pattern, flags=flags)
            if (tail or nbits >= 63) and (name in NAMED or (tail and not flags & OPEN_START)):
                assert np.array_equal(unpack_bits(twin["bits"], n)[:, :nbits], bits), (name, nbits, tail)
            assert np.all(twin["info"][:, 0] == 64 * nsent) and not twin["info"][:, 3].any(), (name, nbits, tail)
            for s in strides_for(2 * ntx):
                tx = conv_encode_ilv_ref(pack_bits(bits), nbits, pattern, s, tail=tail)
                assert tx.shape == (3, ntx) and (s > 1 or np.array_equal(tx, plain))
                for flip in (None, key):
                    sent = tx if flip is None else tx ^ key[None, :]
                    got = viterbi_ilv_ref(dibits_to_soft(sent), n, pattern, s, flip=flip, flags=flags)
                    assert np.array_equal(got["bits"], twin["bits"]) and np.array_equal(got["info"], twin["info"]), (name, nbits, tail, s, flip is None)


# ------------------------------------------------------------------- 5. the two identities
@pytest.mark.parametrize("name", ["1/2", "3/4", "7/8", "deleted", "period32"])
def test_identity_1_gathered_on_the_host_and_identity_2_stride_one(name):
    pattern = dict(ILV_PATTERNS, deleted=DELETED_STEP)[name]
    rng = np.random.default_rng(len(name))
    for n in (6, 65, 150):
        ntx = punct_ntx(n, pattern)
        soft = rng.integers(-128, 128, (3, ntx + 2, 2)).astype(np.int8)          # two dibits of pitch behind every row
        soft[:, 0, 0] = -128
        key = rng.integers(0, 4, ntx).astype(np.uint8)
        for flip in (None, key):
            for flags in (0, OPEN_START | OPEN_END):
                for s in strides_for(2 * ntx):
                    a = viterbi_ilv_ref(soft, n, pattern, s, flip=flip, flags=flags)
                    rows, fk = gather_ref(soft, ntx, s, flip)
                    b = viterbi_punct_ref(rows, n, pattern, flip=fk, flags=flags)
                    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["info"], b["info"]), (name, n, s, flip is None, flags)
                one = viterbi_ilv_ref(soft, n, pattern, 1, flip=flip, flags=flags)
                twin = viterbi_punct_ref(soft[:, :ntx], n, pattern, flip=flip, flags=flags)
                assert np.array_equal(one["bits"], twin["bits"]) and np.array_equal(one["info"], twin["info"])
    packed = rng.integers(0, 256, (4, 19), dtype=np.uint8)
    assert np.array_equal(conv_encode_ilv_ref(packed, 150, pattern, 1), conv_encode_punct_ref(packed, 150, pattern))


# ------------------------------------------------------------------- 6. the framer's and the deframer's restatements
def test_frame_ilv_ref_at_stride_one_is_frame_ref_and_its_body_is_conv_encode_ilv_ref():
    rng = np.random.default_rng(7)
    sync = rng.integers(0, 4, 16, dtype=np.uint8)
    for nbytes, pattern in ((1, HALF), (30, NAMED["3/4"]), (5, DELETED_STEP)):
        payloads = rng.integers(0, 256, (6, nbytes), dtype=np.uint8)
        a = frame_ilv_ref(payloads, sync, True, pattern, 3, 5, 7, None, 1)
        b = frame_ref(payloads, sync, True, pattern, 3, 5, 7, None)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        B = body_len(nbytes, True, pattern)
        s = ilv_stride(2 * B, max(1, 2 * B // 16))
        rows, crcs = frame_ilv_ref(payloads, sync, True, pattern, 3, 5, 7, None, s)
        assert np.array_equal(crcs, b[1]) and not np.array_equal(rows, b[0])
        for k, at in enumerate(starts(16, nbytes, True, pattern, 3, 5, 7)):
            pkt, _ = make_coded_ilv_packet(np.random.default_rng(0), sync, nbytes, pattern, s)
            crc = int(crcs[k])
            whole = np.concatenate([payloads[k], np.array([crc >> 8, crc & 255], np.uint8)])
            body = conv_encode_ilv_ref(whole[None], 8 * (nbytes + 2), pattern, s)[0] ^ ks_prefix(B)
            assert np.array_equal(rows[0, at + 16:at + 16 + B], body) and len(pkt) == 16 + B
        outside = np.ones(rows.shape[1], bool)
        for at in starts(16, nbytes, True, pattern, 3, 5, 7):
            outside[at + 16:at + 16 + B] = False
        assert np.array_equal(rows[:, outside], b[0][:, outside])              # the sync words and the idle fill are untouched
    up = rng.integers(0, 256, (2, 9), dtype=np.uint8)
    assert np.array_equal(frame_ilv_ref(up, sync, False, None, 1, 0, 0, None, 1)[0], frame_ref(up, sync, False, None, 1, 0, 0, None)[0])


@pytest.mark.parametrize("name", ["1/2", "3/4", "deleted"])
def test_rows_of_frame_ilv_ref_come_back_through_deframe_coded_ilv_ref_whatever_the_cuts(name):
    pattern = dict(NAMED, deleted=DELETED_STEP)[name]
    rng = np.random.default_rng(33)
    nbytes, sync = 5, rng.integers(0, 4, 20, dtype=np.uint8)
    B = body_len(nbytes, True, pattern)
    s = ilv_stride(2 * B, 2 * B // 16)
    payloads = rng.integers(0, 256, (3, nbytes), dtype=np.uint8)
    rows, crcs = frame_ilv_ref(payloads, sync, True, pattern, 3, 11, 13, None, s)
    z = dibits_to_costas(rows[0], amp=0.8, noise=0.1, rng=rng)
    whole = deframe_coded_ilv_ref([z], [70.0], sync, 18, nbytes, pattern, s)[0]
    assert [p["pos"] for p in whole] == starts(20, nbytes, True, pattern, 3, 11, 13)
    assert all(p["crc_ok"] for p in whole) and [p["bytes"][:nbytes].tolist() for p in whole] == payloads.tolist()
    assert [int(p["bytes"][nbytes]) << 8 | int(p["bytes"][nbytes + 1]) for p in whole] == crcs.tolist()
    plain = deframe_coded_punct_ref([z], [70.0], sync, 18, nbytes, pattern)[0]
    assert [p["pos"] for p in plain] == [p["pos"] for p in whole] and not any(p["crc_ok"] for p in plain)      # the stride matters
    for sizes in ([1] * len(z), [17] * 40, [7, 1, 1, 100, 2, 64]):
        pushes = cut(z, sizes)
        assert same_packets(flat(deframe_coded_ilv_ref(pushes, [70.0] * len(pushes), sync, 18, nbytes, pattern, s)), whole), sizes
    one = deframe_coded_ilv_ref([z], [70.0], sync, 18, nbytes, pattern, 1)
    assert same_packets(flat(one), plain)


# ------------------------------------------------------------------- 7. the burst link: the reason for the feature
BURST = dict(rows=64, nbytes=30, dibits=16, amp=64, seed=524)


def burst_link(stride):
    """64 rows of a 30-byte packet's 256 bits + tail at rate 1/2 (n = 524 bits on air), sent through the stride at +-64 without noise; in
    every row 16 consecutive on-air dibits are inverted at a random place (the same places for every stride) -> rows decoded wrongly"""
    k = BURST
    rng = np.random.default_rng(k["seed"])
    nbits = 8 * (k["nbytes"] + 2)
    bits = rng.integers(0, 2, (k["rows"], nbits), dtype=np.uint8)
    at = rng.integers(0, nbits + 6 - k["dibits"] + 1, k["rows"])
    soft = dibits_to_soft(conv_encode_ilv_ref(pack_bits(bits), nbits, HALF, stride), amp=k["amp"])
    for r, a in enumerate(at):
        soft[r, a:a + k["dibits"]] = -soft[r, a:a + k["dibits"]]
    got = viterbi_ilv_ref(soft, nbits + 6, HALF, stride)
    return int((unpack_bits(got["bits"], nbits + 6)[:, :nbits] != bits).any(axis=1).sum())


def test_a_burst_of_16_dibits_is_corrected_through_the_interleaver_and_not_without_it():
    """30-byte packets at rate 1/2, n = 524, s = ilv_stride(524, 32) = 33, soft values +-64, otherwise noise-free; 16 consecutive on-air
    dibits inverted at a random place per row.  Asserted: every interleaved row decodes to the sent bits, and at least 48 of the 64 plain
    (stride 1) rows do not -- the 48 is a cap against a vacuous test, not a tolerance.  Observed with this seed: 0 of 64 interleaved rows
    and 64 of 64 plain rows decode wrongly."""
    n = 2 * punct_ntx(8 * (BURST["nbytes"] + 2) + 6, HALF)
    s = ilv_stride(n, 32)
    assert (n, s) == (524, 33)
    wrong_ilv, wrong_plain = burst_link(s), burst_link(1)
    print("burst of %d dibits on %d rows: wrong with stride %d: %d, wrong with stride 1: %d" % (BURST["dibits"], BURST["rows"], s, wrong_ilv, wrong_plain))
    assert wrong_ilv == 0, wrong_ilv
    assert wrong_plain >= 48, wrong_plain
