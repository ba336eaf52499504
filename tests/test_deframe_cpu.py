"""Sync-word packet deframing of continuous streams (qpsk_deframer_reset / qpsk_deframer_push): what can be checked without a GPU.

deframe_ref() below restates the contract of include/qpsk_hip.h (DEFRAMER) in numpy; the GPU tests (test_deframe_gpu.py) compare the
kernel with it.  The link test runs the reference's own shape on the CPU oracle: continuous PCM with packets at random gaps ->
rx_frame() block by block -> the data rule of costas_frame[] -> deframe_ref.
"""
import os

import numpy as np

from test_rx_data_cpu import RING, bytes_to_dibits, data_rule, dibits_to_bytes, sync_ref
from test_rx_ext_cpu import declared

DEFRAME_SYMBOLS = ("qpsk_deframer_reset", "qpsk_deframer_push")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crc16(data):
    """crc16.c: init 0xFFFF, polynomial 0x1021, no reflection, no final xor"""
    crc = 0xFFFF
    for b in np.asarray(data, np.uint8).tolist():
        x = ((crc >> 8) ^ b) & 0xFF
        x ^= x >> 4
        crc = ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFF
    return crc


_KS = {}


def keystream(n):
    """the scrambler's keystream over n dibits from SEED 0x4A80: the oracle's scramble() of zeros (the scrambler is additive)"""
    if n not in _KS:
        from oracle.pyoracle import Oracle, build_oracle
        build_oracle()
        _KS[n] = Oracle().scramble_stream(np.zeros(n, np.uint8))
    return _KS[n]


def deframe_ref(D, sync, min_score, nbytes, ks=None):
    """-> list of dict(pos, rot, score, bytes (nbytes + 2) uint8, crc_ok, end) for every packet COMPLETE within D, in order"""
    d = RING[np.asarray(D, np.uint8) & 3].astype(np.int64)
    rs = RING[np.asarray(sync, np.uint8)].astype(np.int64)
    n, N = len(rs), 4 * (nbytes + 2)
    ks = keystream(N) if ks is None else ks
    out = []
    if len(d) < n:
        return out
    diff = (np.lib.stride_tricks.sliding_window_view(d, n) - rs) & 3
    sc = np.stack([(diff == r).sum(axis=1) for r in range(4)], axis=1)       # (positions, 4)
    best, rot = sc.max(axis=1), sc.argmax(axis=1)                            # argmax: the smallest rotation of a tie
    h = 0
    for p in np.nonzero(best >= min_score)[0].tolist():
        if p < h:
            continue
        if p + n + N > len(d):
            break
        r = int(rot[p])
        u = RING[(d[p + n:p + n + N] - r) & 3] ^ ks
        b = dibits_to_bytes(u)
        ok = crc16(b[:nbytes]) == (int(b[nbytes]) << 8 | int(b[nbytes + 1]))
        out.append(dict(pos=p, rot=r, score=int(best[p]), bytes=b, crc_ok=bool(ok), end=p + n + N))
        h = p + n + N
    return out


def make_packet(rng, sync, nbytes, ks, corrupt=False):
    """[sync][scrambled payload + CRC-16 big-endian] as dibits -> (dibits, payload)"""
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
    crc = crc16(payload) ^ (1 if corrupt else 0)
    body = bytes_to_dibits(np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])) ^ ks
    return np.concatenate([np.asarray(sync, np.uint8), body]).astype(np.uint8), payload


def turn(dibits, q):
    """the dibits as a loop settled q quarter turns off reads them"""
    return RING[(RING[np.asarray(dibits, np.uint8) & 3] + q) & 3].astype(np.uint8)


# ------------------------------------------------------------------- ABI (fails without the feature)
def test_deframer_entry_points_are_declared_bound_and_exported(qpsk_lib):
    from qpsk_amd.lib import API_SYMBOLS
    for name in DEFRAME_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    import qpsk_amd
    for name in ("deframer_reset", "deframe"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name


def test_deframe_kernel_is_built_and_writes_no_scalar_memory():
    src = open(os.path.join(ROOT, "qpsk_amd", "csrc", "deframe.hip")).read().lower()
    assert "deframe.o" in open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_d" + "cache_"):
        assert word not in src, word


# ------------------------------------------------------------------- the numpy restatement, on hand cases
def test_crc16_is_the_oracle_crc(oracle):
    b = np.random.default_rng(2).integers(0, 256, 77, dtype=np.uint8)
    assert crc16(b) == oracle.crc16(b.tobytes())


def test_threshold_exactly_at_min_score():
    rng = np.random.default_rng(1)
    nbytes, sync = 4, rng.integers(0, 4, 16, dtype=np.uint8)
    ks = keystream(4 * (nbytes + 2))
    pkt, payload = make_packet(rng, sync, nbytes, ks)
    hit = sync_ref(np.concatenate([np.zeros(40, np.uint8), pkt]), sync, 0, 40, 0)
    assert hit["lag"][0] == 40 and hit["score"][0] == 16
    for errors in (2, 3):
        bad = pkt.copy()
        for i in (1, 5, 9)[:errors]:
            bad[i] = RING[(RING[bad[i]] + 1) & 3]                       # a wrong dibit in the word
        D = np.concatenate([np.full(40, 0, np.uint8), bad, np.zeros(10, np.uint8)])
        at = deframe_ref(D, sync, 16 - errors, nbytes)                  # exactly min_score
        assert [p["pos"] for p in at if p["crc_ok"]] == [40], errors
        assert at[-1]["score"] == 16 - errors and np.array_equal(at[-1]["bytes"][:nbytes], payload)
        below = deframe_ref(D, sync, 16 - errors + 1, nbytes)           # min_score - 1: not a candidate
        assert 40 not in [p["pos"] for p in below]


def test_rotation_tie_takes_the_smallest_rotation():
    # a word of one repeated dibit against a row of two kinds: two rotations score the same, the smaller one wins
    sync = np.zeros(4, np.uint8)
    D = np.array([0, 1, 0, 1] + [0] * 30, np.uint8)                     # ring: 0 1 0 1 -> rotations 0 and 1 score 2 each
    p = deframe_ref(D, sync, 2, 1)[0]
    assert (p["pos"], p["rot"], p["score"]) == (0, 0, 2)
    D = np.array([1, 3, 1, 3] + [0] * 30, np.uint8)                     # ring: 1 2 1 2 -> rotations 1 and 2
    p = deframe_ref(D, sync, 2, 1)[0]
    assert (p["pos"], p["rot"], p["score"]) == (0, 1, 2)


def test_candidates_inside_a_packet_are_ignored_and_packets_run_back_to_back():
    rng = np.random.default_rng(3)
    nbytes, sync = 8, rng.integers(0, 4, 24, dtype=np.uint8)
    N = 4 * (nbytes + 2)
    ks = keystream(N)
    a, pa = make_packet(rng, sync, nbytes, ks)
    b, pb = make_packet(rng, sync, nbytes, ks)
    # a second word planted INSIDE a's payload (its CRC then fails): the hunt does not see it; b follows a with no gap
    a_bad = a.copy()
    a_bad[24 + 10:24 + 34] = sync
    D = np.concatenate([rng.integers(0, 4, 7, dtype=np.uint8), a_bad, b, rng.integers(0, 4, 5, dtype=np.uint8)])
    got = deframe_ref(D, sync, 24, nbytes)
    assert [(p["pos"], p["crc_ok"]) for p in got] == [(7, False), (7 + 24 + N, True)]
    assert got[0]["end"] == got[1]["pos"] and np.array_equal(got[1]["bytes"][:nbytes], pb)
    D = np.concatenate([a, b])
    got = deframe_ref(D, sync, 24, nbytes)
    assert [(p["pos"], p["crc_ok"]) for p in got] == [(0, True), (24 + N, True)]
    assert np.array_equal(got[0]["bytes"][:nbytes], pa)


def test_crc_pass_and_fail_and_the_hunt_resumes_behind_a_failed_packet():
    rng = np.random.default_rng(4)
    nbytes, sync = 16, rng.integers(0, 4, 32, dtype=np.uint8)
    ks = keystream(4 * (nbytes + 2))
    good, pg = make_packet(rng, sync, nbytes, ks)
    bad, _ = make_packet(rng, sync, nbytes, ks, corrupt=True)
    D = np.concatenate([rng.integers(0, 4, 50, dtype=np.uint8), bad, rng.integers(0, 4, 9, dtype=np.uint8), turn(good, 2)])
    got = deframe_ref(D, sync, 30, nbytes)
    assert [(p["crc_ok"], p["rot"]) for p in got][-2:] == [(False, 0), (True, 2)]
    assert np.array_equal(got[-1]["bytes"][:nbytes], pg)


def test_result_does_not_depend_on_the_cuts():
    """a word and a payload straddling a cut: the packets of the prefixes grow as the concatenation's, each reported once complete"""
    rng = np.random.default_rng(5)
    nbytes, sync = 8, rng.integers(0, 4, 20, dtype=np.uint8)
    ks = keystream(4 * (nbytes + 2))
    parts = []
    for q in range(4):
        parts += [rng.integers(0, 4, int(rng.integers(0, 30)), dtype=np.uint8), turn(make_packet(rng, sync, nbytes, ks)[0], q)]
    D = np.concatenate(parts)
    whole = deframe_ref(D, sync, 18, nbytes)
    assert sum(p["crc_ok"] for p in whole) == 4
    for cut in range(0, len(D) + 1, 7):
        head = deframe_ref(D[:cut], sync, 18, nbytes)
        want = [p for p in whole if p["end"] <= cut]
        assert [(p["pos"], p["rot"], p["crc_ok"]) for p in head] == [(p["pos"], p["rot"], p["crc_ok"]) for p in want], cut


def test_deframe_ref_agrees_with_sync_ref():
    """rows with one planted word and min_score above every other position's best score: p*, r* and the de-rotated dibits before
    descrambling are sync_ref's lag, rot and out"""
    rng = np.random.default_rng(6)
    nbytes, n = 6, 40
    N = 4 * (nbytes + 2)
    zero_ks = np.zeros(N, np.uint8)
    for trial in range(20):
        sync = rng.integers(0, 4, n, dtype=np.uint8)
        row = rng.integers(0, 4, 400, dtype=np.uint8)
        lag = int(rng.integers(0, 400 - n - N))
        row[lag:lag + n] = turn(sync, int(rng.integers(0, 4)))
        s = sync_ref(row, sync, 0, 400 - n - N, N)
        # the best score of any other position
        d = RING[row].astype(np.int64)
        diff = (np.lib.stride_tricks.sliding_window_view(d, n) - RING[sync]) & 3
        best = np.stack([(diff == r).sum(axis=1) for r in range(4)], axis=1).max(axis=1)
        best[lag] = 0
        got = deframe_ref(row, sync, int(best.max()) + 1, nbytes, ks=zero_ks)
        assert len(got) == 1 and got[0]["pos"] == s["lag"][0] == lag and got[0]["rot"] == s["rot"][0]
        assert np.array_equal(bytes_to_dibits(got[0]["bytes"]), s["out"][0]), trial


# ------------------------------------------------------------------- the reference's own shape on the oracle
def link_pcm(oracle, rng, fs, rs, L, nblocks, sync, nbytes, mixer_hz=1500.0, noise=30.0, first=0):
    """continuous PCM at tx_hz = mixer_hz + 50 (qpsk.c:320) carrying packets at random gaps -> (pcm, [(symbol index of the word,
    payload)])"""
    C = int(fs / rs)
    nsym = L // C
    total = nblocks * nsym
    ks = keystream(4 * (nbytes + 2))
    sym = rng.integers(0, 4, total, dtype=np.uint8)
    sent, t = [], first + int(rng.integers(0, 40))
    while True:
        pkt, payload = make_packet(rng, sync, nbytes, ks)
        if t + len(pkt) > total:
            break
        sym[t:t + len(pkt)] = pkt
        sent.append((t, payload))
        t += len(pkt) + int(rng.integers(0, 200))
    tx = oracle.tx(fs, rs, np.float32(0.35), mixer_hz + 50.0)
    pcm = tx.symbols(np.stack([sym >> 1, sym & 1], axis=1).reshape(-1).astype(np.int32)).astype(np.float64)
    pcm = np.clip(np.round(pcm + noise * rng.standard_normal(pcm.size)), -32768, 32767).astype(np.int16)
    return pcm, sent


def test_link_through_the_oracle_stream(oracle):
    """rx_frame() block by block on the shipped configuration (512-sample blocks: a packet is longer than a block): every packet
    comes back with its CRC at symbol t + one block + 126 // CYCLES, and no other packet passes its CRC"""
    from oracle.pyoracle import TIMING_FIXED
    fs, rs, L = 9600.0, 2400.0, 512
    C = int(fs / rs)
    nsym = L // C
    rng = np.random.default_rng(7)
    sync = rng.integers(0, 4, 32, dtype=np.uint8)
    nbytes, nblocks = 64, 30
    pcm, sent = link_pcm(oracle, rng, fs, rs, L, nblocks, sync, nbytes)
    m = oracle.modem(fs, rs, L, timing_mode=TIMING_FIXED, fixed_index=126 % C)
    m.set_mixer_hz(1500.0)
    rows = []
    for b in range(nblocks):
        m.rx_pcm(pcm[b * L:(b + 1) * L])
        rows.append(data_rule(m.costas_frame))
    got = deframe_ref(np.concatenate(rows), sync, 28, nbytes)
    ok = [(p["pos"], p["bytes"][:nbytes].tobytes()) for p in got if p["crc_ok"]]
    want = [(t + nsym + 126 // C, pl.tobytes()) for t, pl in sent if t + nsym + 126 // C + 32 + 4 * (nbytes + 2) <= nblocks * nsym]
    assert len(want) >= 5 and ok == want
