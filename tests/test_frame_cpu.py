"""The batched packet framer (qpsk_frame_len / qpsk_frame_batch, FRAMER in include/qpsk_hip.h): what can be checked without a GPU.

frame_ref() below restates the definition in numpy, composed from the restatements the receive side already has (crc16 and the keystream of
test_deframe_cpu, bytes_to_dibits, conv_encode_ref, conv_encode_punct_ref, punct_ntx); the GPU tests (test_frame_gpu.py) compare the
kernel with it bit for bit.  Here: frame_ref against the three packet builders the deframer tests use, its rows through the three numpy
deframers, and the noise-free link transmitter -> rx_frame() -> deframers on the CPU oracle.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_deframe_coded_cpu import deframe_coded_ref, dibits_to_costas, flat, make_coded_packet
from test_deframe_cpu import crc16, deframe_ref, keystream, make_packet
from test_punct_cpu import BAD_PATTERNS, NAMED, PERIOD32, conv_encode_punct_ref, deframe_coded_punct_ref, make_coded_punct_packet, punct_ntx
from test_rx_data_cpu import bytes_to_dibits, data_rule
from test_rx_ext_cpu import declared
from test_viterbi_cpu import conv_encode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SYMBOLS = ("qpsk_frame_len", "qpsk_frame_batch")
QPSK_ERR_ARG = -2
UNCODED, CODED = 0, 1                # QPSK_FRAME_UNCODED, QPSK_FRAME_CODED
HALF = (1, 1, 1)                     # the pattern of the rate-1/2 format


# ------------------------------------------------------------------- the numpy restatement
def ks_prefix(n):
    """keystream(n) as a prefix of one long keystream (test_the_keystream_of_a_longer_frame_extends_a_shorter_one): test_deframe_cpu's
    keystream() asks the oracle anew for every new length"""
    size = 16384
    while size < n:
        size *= 2
    return keystream(size)[:n]


def body_len(nbytes, coded, pattern=HALF):
    """B: the dibits of a body on air"""
    return punct_ntx(8 * (nbytes + 2) + 6, pattern) if coded else 4 * (nbytes + 2)


def packet_ref(payload, sync, coded, pattern=HALF):
    """one packet [sync & 3][body] -> (dibits (nsync + B,), the CRC sent)"""
    payload = np.asarray(payload, np.uint8)
    crc = crc16(payload)
    pkt = np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])
    if not coded:
        body = bytes_to_dibits(pkt)
    elif tuple(pattern) == HALF:
        body = conv_encode_ref(pkt[None, :], 8 * len(pkt), tail=True)[0]
    else:
        body = conv_encode_punct_ref(pkt[None, :], 8 * len(pkt), pattern, tail=True)[0]
    assert len(body) == body_len(len(payload), coded, pattern)
    return np.concatenate([np.asarray(sync, np.uint8) & 3, body ^ ks_prefix(len(body))]).astype(np.uint8), crc


def frame_ref(payloads, sync, coded, pattern, per_row, lead, gap, row_len):
    """payloads (nrows * per_row, nbytes) uint8 -> (dibits (nrows, row_len) uint8, crc (nrows * per_row,) uint16); row_len None = the exact
    fit.  Packet j of a row starts at column lead + j (P + gap); every other column i is idle fill keystream[i]"""
    payloads = np.asarray(payloads, np.uint8)
    pattern = HALF if pattern is None else pattern
    npk, nbytes = payloads.shape
    assert npk % per_row == 0
    P = len(sync) + body_len(nbytes, coded, pattern)
    need = lead + per_row * P + (per_row - 1) * gap
    row_len = need if row_len is None else row_len
    assert need <= row_len
    rows = np.tile(ks_prefix(row_len), (npk // per_row, 1)).astype(np.uint8)
    crcs = np.zeros(npk, np.uint16)
    for k in range(npk):
        pkt, crcs[k] = packet_ref(payloads[k], sync, coded, pattern)
        at = lead + (k % per_row) * (P + gap)
        rows[k // per_row, at:at + P] = pkt
    return rows, crcs


def starts(nsync, nbytes, coded, pattern, per_row, lead, gap):
    P = nsync + body_len(nbytes, coded, HALF if pattern is None else pattern)
    return [lead + j * (P + gap) for j in range(per_row)]


# ------------------------------------------------------------------- ABI (fails without the feature)
def test_framer_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import inspect
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in FRAME_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "FRAMER" in header and "QPSK_FRAME_UNCODED = 0" in header and "QPSK_FRAME_CODED = 1" in header
    assert callable(getattr(qpsk_amd.Modem, "frame", None)) and callable(getattr(qpsk_amd, "frame_len", None))
    par = inspect.signature(qpsk_amd.Modem.frame).parameters
    assert [(k, par[k].default) for k in ("coded", "puncture", "per_row", "lead", "gap", "row_len")] == \
        [("coded", True), ("puncture", None), ("per_row", 1), ("lead", 0), ("gap", 0), ("row_len", None)]
    mk = open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    assert "frame.o" in mk and "frame.hip" in mk
    buf = (C.c_uint8 * 64)()
    assert qpsk_lib.qpsk_frame_batch(None, buf, 0, 1, 1, 4, buf, 16, CODED, 1, 1, 1, 0, 0, 200, buf, None) == QPSK_ERR_ARG
    assert b"qpsk_frame_batch" in qpsk_lib.qpsk_last_error()


# ------------------------------------------------------------------- qpsk_frame_len, host only
CODINGS = [("uncoded", False, HALF), ("1/2", True, HALF)] + [(k, True, v) for k, v in sorted(NAMED.items()) if k != "1/2"]


def test_qpsk_frame_len_equals_the_formula_and_refuses_out_of_range_arguments(qpsk_lib):
    import qpsk_amd
    for nsync in (1, 16, 128):
        for nbytes in (1, 5, 64, 1024):
            for name, coded, pattern in CODINGS:
                want = nsync + body_len(nbytes, coded, pattern)
                assert qpsk_lib.qpsk_frame_len(nsync, nbytes, CODED if coded else UNCODED, *pattern) == want, (nsync, nbytes, name)
                assert qpsk_amd.frame_len(nsync, nbytes, coded=coded, puncture=pattern if coded else None) == want
            assert qpsk_amd.frame_len(nsync, nbytes) == nsync + 8 * (nbytes + 2) + 6            # coded, no pattern: rate 1/2
    assert qpsk_lib.qpsk_frame_len(16, 5, UNCODED, 0, 0, 0) == 16 + 28                          # the pattern is ignored when uncoded
    for bad in BAD_PATTERNS:
        assert qpsk_lib.qpsk_frame_len(16, 5, CODED, *bad) == QPSK_ERR_ARG, bad
        assert b"qpsk_frame_len" in qpsk_lib.qpsk_last_error()
    for nsync, nbytes, coding in ((0, 5, CODED), (129, 5, CODED), (-1, 5, UNCODED), (16, 0, CODED), (16, 1025, CODED), (16, 1025, UNCODED),
                                  (16, -3, UNCODED), (16, 5, 2), (16, 5, -1)):
        assert qpsk_lib.qpsk_frame_len(nsync, nbytes, coding, 1, 1, 1) == QPSK_ERR_ARG, (nsync, nbytes, coding)
    with pytest.raises(qpsk_amd.QpskError):
        qpsk_amd.frame_len(16, 5, puncture=(3, 0x8, 0x1))
    with pytest.raises(ValueError):
        qpsk_amd.frame_len(16, 5, puncture="4/5")


# ------------------------------------------------------------------- frame_ref against the packet builders of the deframer tests
def test_frame_ref_of_one_packet_equals_the_three_packet_builders():
    rng = np.random.default_rng(11)
    for nsync, nbytes in ((32, 5), (128, 16)):
        sync = rng.integers(0, 4, nsync, dtype=np.uint8)
        pkt, payload = make_packet(rng, sync, nbytes, keystream(4 * (nbytes + 2)))
        rows, crc = frame_ref(payload[None, :], sync, False, None, 1, 0, 0, None)
        assert np.array_equal(rows[0], pkt) and crc[0] == crc16(payload)
        pkt, payload = make_coded_packet(rng, sync, nbytes)
        rows, crc = frame_ref(payload[None, :], sync, True, None, 1, 0, 0, None)
        assert np.array_equal(rows[0], pkt) and crc[0] == crc16(payload)
        for name, pattern in sorted(NAMED.items()):
            pkt, payload = make_coded_punct_packet(rng, sync, nbytes, pattern)
            rows, crc = frame_ref(payload[None, :], sync, True, pattern, 1, 0, 0, None)
            assert np.array_equal(rows[0], pkt) and crc[0] == crc16(payload), (nsync, nbytes, name)
    # the pattern (1, 1, 1) through the punctured encoder is the rate-1/2 body, and sync dibits are taken & 3
    payload = rng.integers(0, 256, (1, 7), dtype=np.uint8)
    sync = rng.integers(0, 4, 16, dtype=np.uint8)
    a = frame_ref(payload, sync, True, HALF, 1, 3, 0, None)[0]
    b = np.concatenate([keystream(3), sync, conv_encode_punct_ref(
        np.concatenate([payload[0], np.array([crc16(payload[0]) >> 8, crc16(payload[0]) & 255], np.uint8)])[None, :], 72, HALF)[0] ^ keystream(78)])
    assert np.array_equal(a[0], b)
    assert np.array_equal(frame_ref(payload, sync | 0xA4, True, HALF, 1, 3, 0, None)[0], a)


def test_the_keystream_of_a_longer_frame_extends_a_shorter_one():
    for n in (1, 28, 62, 535, 4104):
        assert np.array_equal(keystream(n), ks_prefix(n)), n
    assert np.array_equal(keystream(16384), keystream(32768)[:16384])


# ------------------------------------------------------------------- rows through the numpy deframers
PER_ROW, TRAIL = 3, 9
PLACES = ((0, 0), (5, 7), (64, 1))


def planted_row(rng, nsync, nbytes, coded, pattern, lead, gap):
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    payloads = rng.integers(0, 256, (PER_ROW, nbytes), dtype=np.uint8)
    at = starts(nsync, nbytes, coded, pattern, PER_ROW, lead, gap)
    need = at[-1] + nsync + body_len(nbytes, coded, HALF if pattern is None else pattern)
    rows, crc = frame_ref(payloads, sync, coded, pattern, PER_ROW, lead, gap, need + TRAIL)
    assert rows.shape == (1, need + TRAIL) and rows.max() <= 3
    return sync, payloads, at, rows[0], crc


def assert_planted(got, at, payloads, crc, nbytes):
    assert [p["pos"] for p in got] == at
    for p, payload, c in zip(got, payloads, crc):
        assert p["crc_ok"] and p["rot"] == 0 and np.array_equal(p["bytes"][:nbytes], payload)
        assert (int(p["bytes"][nbytes]) << 8 | int(p["bytes"][nbytes + 1])) == int(c)


@pytest.mark.parametrize("nbytes", [1, 5, 16, 64, 200])
@pytest.mark.parametrize("nsync", [16, 32, 128])
def test_rows_come_back_through_the_numpy_deframers(nsync, nbytes):
    """three packets per row at (lead, gap) = (0, 0), (5, 7), (64, 1) and nine trailing idle columns, min_score = nsync: deframe_ref and
    deframe_coded_ref report exactly the three planted positions -- no false word in the idle fill -- all crc_ok, payloads equal"""
    rng = np.random.default_rng(1000 * nsync + nbytes)
    for lead, gap in PLACES:
        sync, payloads, at, row, crc = planted_row(rng, nsync, nbytes, False, None, lead, gap)
        got = deframe_ref(row, sync, nsync, nbytes, ks=ks_prefix(4 * (nbytes + 2)))
        assert [p["score"] for p in got] == [nsync] * PER_ROW
        assert_planted(got, at, payloads, crc, nbytes)
        sync, payloads, at, row, crc = planted_row(rng, nsync, nbytes, True, None, lead, gap)
        got = flat(deframe_coded_ref([dibits_to_costas(row, amp=0.7)], [np.float32(90.0)], sync, nsync, nbytes))
        assert_planted(got, at, payloads, crc, nbytes)
        assert all(p["info"][3] == 0 for p in got)                          # no channel bit errors


@pytest.mark.parametrize("name", sorted(NAMED))
@pytest.mark.parametrize("nbytes", [5, 16])
@pytest.mark.parametrize("nsync", [16, 32, 128])
def test_punctured_rows_come_back_through_the_numpy_deframer(nsync, nbytes, name):
    rng = np.random.default_rng(1000 * nsync + nbytes + 7)
    for lead, gap in PLACES:
        sync, payloads, at, row, crc = planted_row(rng, nsync, nbytes, True, NAMED[name], lead, gap)
        got = flat(deframe_coded_punct_ref([dibits_to_costas(row, amp=0.7)], [np.float32(90.0)], sync, nsync, nbytes, NAMED[name]))
        assert_planted(got, at, payloads, crc, nbytes)


def test_a_period_32_pattern_comes_back_too():
    rng = np.random.default_rng(32)
    sync, payloads, at, row, crc = planted_row(rng, 32, 16, True, PERIOD32, 5, 7)
    got = flat(deframe_coded_punct_ref([dibits_to_costas(row, amp=0.7)], [np.float32(90.0)], sync, 32, 16, PERIOD32))
    assert_planted(got, at, payloads, crc, 16)


# ------------------------------------------------------------------- the noise-free link on the CPU oracle
LINK = dict(fs=9600.0, rs=2400.0, L=512, tx_hz=1550.0, mixer_hz=1500.0, nsync=32, nbytes=16, min_score=28, per_row=3, lead=150, gap=37,
            spare_blocks=3, seed=2061)
LINK_CODINGS = {"uncoded": (False, None), "1/2": (True, None), "3/4": (True, NAMED["3/4"]), "7/8": (True, NAMED["7/8"])}


def link_shape(coding, nstreams=1):
    """-> dict(sync, payloads (nstreams * per_row, nbytes), row_len = whole blocks + spare_blocks, at = the packets' start columns, delay)"""
    k = LINK
    coded, pattern = LINK_CODINGS[coding]
    Cy = int(k["fs"] / k["rs"])
    nsym = k["L"] // Cy
    rng = np.random.default_rng(k["seed"])
    sync = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    payloads = rng.integers(0, 256, (nstreams * k["per_row"], k["nbytes"]), dtype=np.uint8)
    at = starts(k["nsync"], k["nbytes"], coded, pattern, k["per_row"], k["lead"], k["gap"])
    need = at[-1] + k["nsync"] + body_len(k["nbytes"], coded, HALF if pattern is None else pattern)
    row_len = (-(-need // nsym) + k["spare_blocks"]) * nsym
    return dict(coded=coded, pattern=pattern, sync=sync, payloads=payloads, row_len=row_len, at=at, nsym=nsym, cycles=Cy,
                delay=nsym + 126 // Cy)


def link_receive(oracle, row):
    """one row of dibits -> the oracle's transmitter (tx_hz) -> rx_frame() block by block at the shipped configuration, fixed index
    126 % CYCLES -> the costas_frame[] of every block"""
    from oracle.pyoracle import TIMING_FIXED
    k = LINK
    Cy = int(k["fs"] / k["rs"])
    tx = oracle.tx(k["fs"], k["rs"], np.float32(0.35), k["tx_hz"])
    pcm = tx.symbols(np.stack([row >> 1, row & 1], axis=1).reshape(-1).astype(np.int32))
    m = oracle.modem(k["fs"], k["rs"], k["L"], timing_mode=TIMING_FIXED, fixed_index=126 % Cy)
    m.set_mixer_hz(k["mixer_hz"])
    blocks = []
    for b in range(len(pcm) // k["L"]):
        m.rx_pcm(pcm[b * k["L"]:(b + 1) * k["L"]])
        blocks.append(np.array(m.costas_frame, np.float32).reshape(-1, 2).copy())
    return pcm, blocks


def link_deframe(shape, blocks):
    """the numpy deframer of the shape's coding on the blocks of one stream, a push per block -> the packets in order"""
    k = LINK
    if not shape["coded"]:
        return deframe_ref(data_rule(np.concatenate(blocks)), shape["sync"], k["min_score"], k["nbytes"])
    if shape["pattern"] is None:
        return flat(deframe_coded_ref(blocks, None, shape["sync"], k["min_score"], k["nbytes"]))
    return flat(deframe_coded_punct_ref(blocks, None, shape["sync"], k["min_score"], k["nbytes"], shape["pattern"]))


@pytest.mark.parametrize("coding", sorted(LINK_CODINGS))
def test_noise_free_link_through_the_oracle(oracle, coding):
    """frame_ref's row -> PCM -> rx_frame() block by block -> the numpy deframer: every packet comes back crc_ok with its payload at
    column + one block + 126 // CYCLES = column + 128 + 31, and nothing else is reported"""
    k = LINK
    shape = link_shape(coding)
    rows, crc = frame_ref(shape["payloads"], shape["sync"], shape["coded"], shape["pattern"], k["per_row"], k["lead"], k["gap"], shape["row_len"])
    assert shape["delay"] == 128 + 31 and rows.shape[1] % shape["nsym"] == 0
    _, blocks = link_receive(oracle, rows[0])
    got = link_deframe(shape, blocks)
    assert [p["pos"] for p in got] == [c + 159 for c in shape["at"]]
    for p, payload in zip(got, shape["payloads"]):
        assert p["crc_ok"] and np.array_equal(p["bytes"][:k["nbytes"]], payload)
    print("%s: rot %s, score %s" % (coding, [p["rot"] for p in got], [p["score"] for p in got]))
