"""The K = 7, rate-1/2 convolutional code and its Viterbi decoder (qpsk_conv_encode_batch, qpsk_viterbi_batch): what can be checked
without a GPU.

conv_encode_ref() and viterbi_ref() below restate the definition of include/qpsk_hip.h in numpy, in integers; the GPU tests
(test_viterbi_gpu.py) compare the kernels with them bit for bit.  The reference has no FEC, so the tests here pin the restatement to a
second, naive one (exhaustive search over all codewords of short rows), check the header's statement about a finite start penalty, and
show on the CPU oracle's own costas_frame[] that the decoder corrects what hard decisions cannot.
"""
import os

import numpy as np
import pytest

from oracle.pyoracle import TAU
from test_rx_data_cpu import bytes_to_dibits, data_rule, dibits_to_bytes, sync_ref, transmit
from test_rx_ext_cpu import declared, oracle_ext
from test_soft_cpu import soft_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G0, G1 = 0x79, 0x5B                       # 171, 133 octal
NEG = -(1 << 30)
CONV_TAIL, OPEN_START, OPEN_END = 1, 1, 2
VITERBI_SYMBOLS = ("qpsk_conv_encode_batch", "qpsk_viterbi_batch", "qpsk_test_viterbi_launches", "qpsk_test_deframer_advance")
PAR = np.array([bin(v).count("1") & 1 for v in range(128)], np.int64)
C0, C1 = PAR[np.arange(128) & G0], PAR[np.arange(128) & G1]      # the coded pair of register value r


# ------------------------------------------------------------------- the numpy restatement
def pack_bits(bits):
    """(..., n) 0/1 -> (..., ceil(n/8)) uint8, bit t in byte t >> 3 at position t & 7"""
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="little")


def unpack_bits(packed, n):
    return np.unpackbits(np.asarray(packed, np.uint8), axis=-1, bitorder="little")[..., :n]


def conv_encode_ref(bits_packed, nbits, tail=True):
    """(R, ceil(nbits/8)) uint8 -> (R, nsteps) uint8 dibits c0 | c1 << 1"""
    b = unpack_bits(np.atleast_2d(bits_packed), nbits).astype(np.int64)
    if tail:
        b = np.concatenate([b, np.zeros((b.shape[0], 6), np.int64)], axis=1)
    r = np.zeros(b.shape[0], np.int64)
    out = np.zeros(b.shape, np.uint8)
    for t in range(b.shape[1]):
        r = ((r << 1) | b[:, t]) & 127
        out[:, t] = C0[r] | (C1[r] << 1)
    return out


def prepare_soft(soft, flip):
    """int8 (R, n, 2) -> int64 after the -128 rule and d_flip"""
    s = np.maximum(np.asarray(soft, np.int8).astype(np.int64), -127)
    if flip is not None:
        f = np.asarray(flip, np.uint8).astype(np.int64)
        s = s.copy()
        s[:, :, 0] = np.where(f & 1, -s[:, :, 0], s[:, :, 0])
        s[:, :, 1] = np.where(f & 2, -s[:, :, 1], s[:, :, 1])
    return s


def viterbi_ref(soft, flip=None, flags=0, penalty=NEG):
    """soft (R, nsteps, 2) int8 -> dict(bits (R, ceil(nsteps/8)) uint8, info (R, 4) int32), every row at once; penalty: the start value of
    the 63 other states (the definition's NEG; the header states that any finite penalty below -3048 gives the same outputs)"""
    s = prepare_soft(np.asarray(soft, np.int8).reshape(-1, np.shape(soft)[-2], 2), flip)
    R, n = s.shape[0], s.shape[1]
    ns = np.arange(64)
    p0, p1 = ns >> 1, (ns >> 1) | 32
    sg = lambda c: 1 - 2 * c      # noqa: E731
    a0, a1 = sg(C0[ns]), sg(C1[ns])                       # bm(ns)
    b0, b1 = sg(C0[ns | 64]), sg(C1[ns | 64])             # bm(ns | 64)
    pm = np.full((R, 64), penalty, np.int64)
    pm[:, 0] = 0
    if flags & OPEN_START:
        pm[:] = 0
    dec = np.zeros((n, R), np.uint64)
    weights = (np.uint64(1) << np.arange(64, dtype=np.uint64))
    for t in range(n):
        s0, s1 = s[:, t, 0:1], s[:, t, 1:2]
        m0 = pm[:, p0] + a0 * s0 + a1 * s1
        m1 = pm[:, p1] + b0 * s0 + b1 * s1
        d = m1 > m0                                        # a tie keeps p0
        pm = np.where(d, m1, m0)
        dec[t] = (d.astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)
    assert np.abs(pm).max() < 2 ** 31                      # int32 on the device
    end = np.argmax(pm, axis=1) if flags & OPEN_END else np.zeros(R, np.int64)      # argmax: the first (lowest) of equal maxima
    rows = np.arange(R)
    st = end.astype(np.int64)
    bits = np.zeros((R, n), np.uint8)
    for t in range(n - 1, -1, -1):
        bits[:, t] = st & 1
        st = (st >> 1) | ((((dec[t] >> st.astype(np.uint64)) & np.uint64(1)).astype(np.int64)) << 5)
    coded = conv_encode_from_state(bits, st)
    c = np.stack([coded & 1, coded >> 1], axis=-1).astype(np.int64)
    errs = ((s != 0) & ((s < 0).astype(np.int64) != c)).sum(axis=(1, 2))
    info = np.stack([pm[rows, end], end, st, errs], axis=1).astype(np.int32)
    return dict(bits=pack_bits(bits), info=info)


def conv_encode_from_state(bits, state):
    """the path's coded dibits: the encoder started in `state` (the state the trace-back arrives at; 0 unless open start)"""
    r = np.asarray(state, np.int64).copy()
    out = np.zeros(bits.shape, np.uint8)
    for t in range(bits.shape[1]):
        r = ((r << 1) | bits[:, t]) & 127
        out[:, t] = C0[r] | (C1[r] << 1)
    return out


def dibits_to_soft(d, amp=64):
    """coded dibits -> noise-free soft values: positive <=> the bit is 0"""
    d = np.asarray(d, np.uint8)
    return np.stack([np.where(d & 1, -amp, amp), np.where(d & 2, -amp, amp)], axis=-1).astype(np.int8)


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_viterbi_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import ctypes as C
    import torch
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in VITERBI_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    for word in ("QPSK_CONV_TAIL = 1", "QPSK_VITERBI_OPEN_START = 1", "QPSK_VITERBI_OPEN_END = 2"):
        assert word in header, word
    assert '"QPSK_VITERBI_CHUNK_ROWS"' in header and "none of them can change a result" in header
    for name in ("conv_encode", "viterbi", "viterbi_launches", "deframer_advance"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    # no context, no work: without a GPU no context can exist (test_abi.py::test_no_gpu_means_error_not_fallback), and the entry points
    # refuse a NULL one with QPSK_ERR_ARG on any machine
    buf = (C.c_uint8 * 64)()
    assert qpsk_lib.qpsk_conv_encode_batch(None, buf, 1, 8, 1, buf) == -2
    assert qpsk_lib.qpsk_viterbi_batch(None, buf, 0, 1, 8, None, 0, buf, None) == -2
    assert b"qpsk_viterbi_batch" in qpsk_lib.qpsk_last_error()
    n = C.c_int(-9)
    assert qpsk_lib.qpsk_test_viterbi_launches(None, C.byref(n)) == -2 and n.value == -9
    assert b"qpsk_test_viterbi_launches" in qpsk_lib.qpsk_last_error()
    for delta in (0, 1 << 40, -1):
        assert qpsk_lib.qpsk_test_deframer_advance(None, delta) == -2
    assert b"qpsk_test_deframer_advance" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_ctx_set_tuning(None, b"QPSK_VITERBI_CHUNK_ROWS", 1) == -2
    if not torch.cuda.is_available():
        with pytest.raises(qpsk_amd.QpskError):
            qpsk_amd.Modem().viterbi(np.zeros((1, 8, 2), np.int8))


def test_viterbi_kernel_is_built_and_writes_no_scalar_memory():
    src = open(os.path.join(ROOT, "qpsk_amd", "csrc", "viterbi.hip")).read().lower()
    assert "viterbi.o" in open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_d" + "cache_"):
        assert word not in src, word


# ------------------------------------------------------------------- 3. the restatement is pinned
def test_encoder_hand_cases():
    # one 1 bit, then the tail: the register walks 1, 2, 4, ... 64: the impulse responses 171 and 133 octal, newest bit in bit 0
    d = conv_encode_ref(pack_bits([[1]]), 1, tail=True)[0]
    assert [int(v) & 1 for v in d] == [(G0 >> k) & 1 for k in range(7)]
    assert [int(v) >> 1 for v in d] == [(G1 >> k) & 1 for k in range(7)]
    assert conv_encode_ref(pack_bits([[0] * 9]), 9, tail=False).tolist() == [[0] * 9]
    # bits beyond nbits in the last byte are not read
    assert np.array_equal(conv_encode_ref(np.array([[0xFF]], np.uint8), 3), conv_encode_ref(np.array([[0x07]], np.uint8), 3))


def naive_best(s, nbits, tail):
    """exhaustive: the largest correlation over all 2^nbits codewords from state 0, and the set of maximising inputs"""
    words = np.arange(1 << nbits)
    bits = ((words[:, None] >> np.arange(nbits)) & 1).astype(np.uint8)
    d = conv_encode_ref(pack_bits(bits), nbits, tail=tail) if nbits else np.zeros((1, 0), np.uint8)
    corr = (np.where(d & 1, -1, 1) * s[None, :, 0] + np.where(d >> 1, -1, 1) * s[None, :, 1]).sum(axis=1)
    return int(corr.max()), set(words[corr == corr.max()].tolist()), d


@pytest.mark.parametrize("nbits", list(range(1, 11)))
def test_viterbi_ref_finds_a_maximum_correlation_codeword(nbits):
    rng = np.random.default_rng(100 + nbits)
    n = nbits + 6
    rows = [rng.integers(-128, 128, (n, 2)) for _ in range(24)]
    rows += [rng.integers(-1, 2, (n, 2)) for _ in range(12)]                      # ties all the time
    rows += [rng.choice([-127, 127], (n, 2)) for _ in range(6)]                   # saturated
    rows += [np.zeros((n, 2), np.int64), np.full((n, 2), -128), np.full((n, 2), 127)]
    soft = np.stack(rows).astype(np.int8)
    got = viterbi_ref(soft)
    s = prepare_soft(soft, None)
    for i in range(len(soft)):
        best, argbest, coded = naive_best(s[i], nbits, True)
        bits = unpack_bits(got["bits"][i], n)
        word = int((bits[:nbits].astype(np.int64) << np.arange(nbits)).sum())
        assert got["info"][i, 0] == best, (nbits, i)
        assert word in argbest and not bits[nbits:].any(), (nbits, i)
        assert got["info"][i, 1] == 0 and got["info"][i, 2] == 0
        c = np.stack([coded[word] & 1, coded[word] >> 1], axis=-1)
        assert got["info"][i, 3] == int(((s[i] != 0) & ((s[i] < 0) != c.astype(bool))).sum()), (nbits, i)


@pytest.mark.parametrize("flags", [0, OPEN_START, OPEN_END, OPEN_START | OPEN_END])
def test_noise_free_rows_decode_to_themselves(flags, oracle):
    """with the start open a row shorter than a few constraint lengths is ambiguous by construction (another start state emits the same
    few pairs), so those flag combinations take the rows of 63 bits and more; the closed start takes every length from 1"""
    rng = np.random.default_rng(7 + flags)
    for nbits in (63, 64, 65, 200) if flags & OPEN_START else (1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 200):
        bits = rng.integers(0, 2, (5, nbits), dtype=np.uint8)
        for tail in (True, False):
            if not tail and not flags & OPEN_END:
                continue                                   # without a tail the path does not end in state 0
            d = conv_encode_ref(pack_bits(bits), nbits, tail=tail)
            n = d.shape[1]
            key = oracle.scramble_stream(np.zeros(n, np.uint8))
            for flip in (None, key):
                sent = d if flip is None else d ^ key[None, :]                   # the scrambler on the dibits, undone on the soft values
                got = viterbi_ref(dibits_to_soft(sent), flip=flip, flags=flags)
                assert np.array_equal(unpack_bits(got["bits"], n)[:, :nbits], bits), (nbits, tail, flip is None)
                assert np.all(got["info"][:, 0] == 128 * n) and not got["info"][:, 3].any()
                assert not got["info"][:, 2].any()         # the path starts in state 0 although every start was allowed


def test_rows_shorter_than_the_register():
    """nsteps 1 .. 7 without a tail, open end: the decoded bits are the sent ones"""
    for n in range(1, 8):
        bits = ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.uint8)
        d = conv_encode_ref(pack_bits(bits), n, tail=False)
        got = viterbi_ref(dibits_to_soft(d), flags=OPEN_END)
        assert np.array_equal(unpack_bits(got["bits"], n), bits), n
        assert np.array_equal(got["info"][:, 1], (bits.astype(np.int64) << np.arange(n)[::-1]).sum(axis=1) & 63), n


# ------------------------------------------------------------------- 4. a finite start penalty above the spread changes nothing
def test_start_penalty_3049_equals_neg():
    rng = np.random.default_rng(4)
    for soft in (rng.integers(-128, 128, (64, 600, 2)), rng.integers(-1, 2, (16, 300, 2)), rng.choice([-127, 127], (16, 300, 2))):
        for flags in (0, OPEN_END):
            a, b = viterbi_ref(soft.astype(np.int8), flags=flags), viterbi_ref(soft.astype(np.int8), flags=flags, penalty=-3049)
            assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["info"], b["info"])


# ------------------------------------------------------------------- 5. it corrects what hard decisions cannot
LINK = dict(fs=19200.0, rs=2400.0, C=8, L=16384, nbytes=64, prefix=100, nsync=64, frames=16, noise=0.26, seed=51)


def make_coded_frame(orc, rng, nsym, prefix, sync, nbytes):
    """[prefix random dibits][sync][coded (payload + CRC-16, big-endian) + tail, scrambled][the same packet UNCODED, scrambled][random
    fill] -> (symbols, payload, nsteps): the uncoded copy meets the same channel and is what hard decisions alone can deliver"""
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
    crc = orc.crc16(payload.tobytes())
    packet = np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])
    body = orc.scramble_stream(conv_encode_ref(packet[None, :], 8 * len(packet), tail=True)[0])
    plain = orc.scramble_stream(bytes_to_dibits(packet))
    sym = rng.integers(0, 4, nsym, dtype=np.uint8)
    at = prefix
    for part in (sync, body, plain):
        sym[at:at + len(part)] = part
        at += len(part)
    return sym, payload, len(body)


def coded_link(orc, noise=None):
    """the frames of LINK through the CPU oracle: dict with x (the transmitted frames), costas, sync's outputs (payload = the coded body and
    the uncoded copy behind it), the keystream of the coded body, the payloads"""
    k = LINK
    noise = k["noise"] if noise is None else noise
    nsym = k["L"] // k["C"]
    taps = orc.rrc_make(np.float32(k["fs"]), np.float32(k["rs"]), np.float32(0.35))
    rng = np.random.default_rng(k["seed"])
    sync = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    frames, payloads = [], []
    for f in range(k["frames"]):
        sym, pl, nsteps = make_coded_frame(orc, rng, nsym, k["prefix"], sync, k["nbytes"])
        frames.append(transmit(sym, k["L"], k["C"], taps, k["fs"], offset_hz=30.0, phase=0.3 + f * np.pi / 2, noise=noise, seed=f))
        payloads.append(pl)
    x = np.stack(frames)
    got = oracle_ext(orc, x, k["fs"], k["rs"], np.full(len(x), 126 % k["C"], np.int32), None, loop_bw=np.float32(TAU / 100.0), want_costas=True)
    s = sync_ref(data_rule(got["costas"]), sync, 0, 255, nsteps + 4 * (k["nbytes"] + 2))
    return dict(x=x, costas=got["costas"], sync=sync, s=s, nsteps=nsteps, key=orc.scramble_stream(np.zeros(nsteps, np.uint8)),
                payloads=np.stack(payloads))


def crc_ok(orc, packet, nbytes):
    return (int(packet[nbytes]) << 8 | int(packet[nbytes + 1])) == orc.crc16(packet[:nbytes].tobytes())


def link_verdicts(orc, lk):
    """-> (frames whose UNCODED copy fails its CRC on data_rule's hard decisions, frames whose Viterbi output passes its CRC and equals the
    payload, the decoder's outputs)"""
    k, s, nsteps, nbytes = LINK, lk["s"], lk["nsteps"], LINK["nbytes"]
    soft = soft_ref(lk["costas"], skip=256, lag=s["lag"], rot=s["rot"], first=k["nsync"], nout=nsteps)["soft"]
    got = viterbi_ref(soft, flip=lk["key"])
    hard_fail = good = 0
    for f in range(k["frames"]):
        plain = dibits_to_bytes(orc.scramble_stream(s["out"][f, nsteps:]))      # the uncoded copy: descrambled hard decisions, packed
        hard_fail += not crc_ok(orc, plain, nbytes)
        out = got["bits"][f][:nbytes + 2]
        good += bool(np.array_equal(out[:nbytes], lk["payloads"][f]) and crc_ok(orc, out, nbytes))
    return hard_fail, good, got, soft


def test_coded_packets_through_the_oracle_pass_where_hard_decisions_fail(oracle):
    """Each of 16 frames carries, behind a 64-dibit sync word, a packet of 64 payload bytes + CRC-16 twice: coded (K = 7, rate 1/2, tail)
    and scrambled, and behind it uncoded and scrambled, so both meet the same channel.  Transmitted with additive noise 0.26 per
    component (sigutil's units, seed 51), received by the CPU oracle at the matched decimation offset; data rule -> sync_ref -> for the coded copy soft_ref
    (UNIT, scale 64, sync's lag and rot) -> viterbi_ref with the keystream as d_flip; for the uncoded copy sync's de-rotated hard decisions,
    descrambled and packed.  Asserted: the hard decisions give a failing CRC in at least half of the frames, and every frame's Viterbi
    output passes its CRC and equals the payload.
    The noise level was found on the CPU with these seeds (16 frames each): 0.20 -> 0 hard failures, 16 decoded; 0.24 -> 6, 16;
    0.26 -> 9, 16 (the decoder counts 0 .. 5 channel bit errors of 1068 per frame in the coded copy); 0.28 -> 14, 15 (one frame's Costas
    loop slips: 95 bit errors, beyond the code); 0.30 -> 15, 15.  Behind the Costas loop the errors are not the ideal AWGN channel's of
    the issue's table: they come with the loop's phase jitter, in bursts."""
    k = LINK
    lk = coded_link(oracle)
    assert np.all(lk["s"]["lag"] == k["prefix"] + 126 // k["C"]), lk["s"]["lag"]
    hard_fail, good, got, _ = link_verdicts(oracle, lk)
    flips = got["info"][:, 3]
    print("noise %g: hard CRC failures %d / %d, Viterbi good %d / %d, channel bit errors per frame %d .. %d of %d"
          % (k["noise"], hard_fail, k["frames"], good, k["frames"], flips.min(), flips.max(), 2 * lk["nsteps"]))
    assert hard_fail >= k["frames"] // 2, hard_fail
    assert good == k["frames"], good
    assert np.all(got["info"][:, 1] == 0) and np.all(got["info"][:, 2] == 0)
