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


# ------------------------------------------------------------------- inputs the GPU tests and the port's CPU test share
def want_of(D, cuts, sync, min_score, nbytes):
    """deframe_ref over the concatenation, each packet tagged with the push that completes it"""
    ends = np.cumsum(cuts)
    out = []
    for p in deframe_ref(D, sync, min_score, nbytes):
        k = int(np.searchsorted(ends, p["end"]))            # the first push whose cumulative length reaches the packet's end
        out.append((k, p["pos"], p["rot"], p["score"], p["bytes"].tobytes(), p["crc_ok"]))
    return out


def planted_streams(rng, S, total, sync, nbytes, max_err=3):
    """S rows of random dibits with packets at random gaps and rotations, 0..max_err dibit errors in each word"""
    ks = keystream(4 * (nbytes + 2))
    D = rng.integers(0, 4, (S, total), dtype=np.uint8)
    for s in range(S):
        t = int(rng.integers(0, 300))
        while True:
            pkt, _ = make_packet(rng, sync, nbytes, ks, corrupt=bool(rng.integers(0, 8) == 0))
            pkt = turn(pkt, int(rng.integers(0, 4)))
            for i in rng.choice(len(sync), int(rng.integers(0, max_err + 1)), replace=False):
                pkt[i] = (pkt[i] + 1 + rng.integers(0, 3)) & 3
            if t + len(pkt) > total:
                break
            D[s, t:t + len(pkt)] = pkt
            t += len(pkt) + int(rng.integers(0, 400))
    return D


EDGE_CUTTINGS = ([1] * 200 + [1300], [97] * 15 + [45])


def edge_case(nsync, nbytes):
    """6 streams of 1500 dibits for a word of nsync dibits, and per cutting the reference's records.  The seed is chosen so that the
    reference, before anything is compared with it, shows two packets in every stream and, under either cutting, a packet that ends in
    a later push than the one that completed its sync word"""
    rng = np.random.default_rng(101 + nsync)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    D = planted_streams(rng, 6, 1500, sync, nbytes, max_err=1)
    wants = []
    for cuts in EDGE_CUTTINGS:
        ends = np.cumsum(cuts)
        want = [want_of(D[s], cuts, sync, nsync - 1, nbytes) for s in range(6)]
        assert all(len(w) >= 2 for w in want), [len(w) for w in want]
        assert any(r[0] > np.searchsorted(ends, r[1] + nsync) for w in want for r in w)
        wants.append(want)
    return sync, D, wants


def cuttings_of_test_1(rng, total):
    """the five cuttings of test_deframe_gpu's test 1, the last one drawn from the generator that made the streams"""
    mixed = []
    while sum(mixed) < total:
        mixed.append(int(rng.choice([1, 7, 128, 2048, int(rng.integers(1, 700))])))
    mixed[-1] -= sum(mixed) - total
    mixed = [c for c in mixed if c > 0]
    return [[c for c in cuts if c > 0] for cuts in ([1] * 300 + [total - 300], [7] * (total // 7) + [total % 7],
                                                    [128] * (total // 128) + [total % 128], [2048, 2048, total - 4096], mixed)]


# The hunt's own sets (deframe_hunt.h): S = 6 streams -- two workgroups of HUNT_WAVES = 4, the second one ragged -- of 1500 dibits, under
# four cuttings.  Where min_score lies far below nsync a candidate is no planted word any more: every step holds several, hx lands inside a
# step, a chunk restarts behind every packet, and two rotations can reach the same count.
HUNT_S, HUNT_TOTAL = 6, 1500
HUNT_CUTTINGS = ([1] * 200 + [1300], [97] * 15 + [45], [1500], [64] * 23 + [28])
DENSE_NOISE = ((7, 1, 2), (7, 1, 4), (16, 1, 6), (65, 2, 20), (128, 1, 40), (64, 1, 16), (1, 1, 1), (2, 1, 1))      # (nsync, nbytes, min_score)
DENSE_NOISE_CODED = ((16, 1, 6), (65, 2, 20))
TIE_NSYNC = (8, 64, 66, 128)
B2B_K = 3
HUNT_SET_NAMES = tuple(["dense noise (%d, %d, %d)" % t for t in DENSE_NOISE] + ["ties of %s, nsync %d" % (w, n) for n in TIE_NSYNC for w in ("two", "four")]
                       + ["back to back, max_packets %d" % M for M in (B2B_K + 1, B2B_K, 64)])
HUNT_CODED_SET_NAMES = {kind: tuple(["%s dense noise (%d, %d, %d)" % ((kind,) + t) for t in DENSE_NOISE_CODED if kind != "ilv"]
                                    + ["%s back to back, max_packets %d" % (kind, M) for M in (B2B_K + 1, B2B_K, 64)]) for kind in ("plain", "punct", "ilv")}


def rotation_scores(D, sync):
    """(positions, 4): the dibits of the word at each position that match under each rotation"""
    d = RING[np.asarray(D, np.uint8) & 3].astype(np.int64)
    diff = (np.lib.stride_tricks.sliding_window_view(d, len(sync)) - RING[np.asarray(sync, np.uint8)].astype(np.int64)) & 3
    return np.stack([(diff == r).sum(axis=1) for r in range(4)], axis=1)


def written(want, npush, max_packets):
    """records tagged with their push -> (count per push, the records a push writes: its first max_packets)"""
    count = [sum(1 for r in want if r[0] == k) for k in range(npush)]
    seen, out = [0] * npush, []
    for r in want:
        if seen[r[0]] < max_packets:
            out.append(r)
        seen[r[0]] += 1
    return count, out


def _check_dense(s):
    """every stream completes packets in most pushes' steps; at nsync = 7, 1 and 2 the one push of 1500 overflows max_packets"""
    n, _, ms = s["nsync"], s["nbytes"], s["min_score"]
    for k in range(HUNT_S):
        sc = rotation_scores(s["D"][k], s["sync"]).max(axis=1)
        if ms <= -(-n // 4):
            assert (sc >= ms).all()                                     # every position is a candidate
        else:
            assert (sc >= ms).mean() > 0.02                             # and elsewhere a 64-position step holds more than one
        whole = want_of(s["D"][k], [HUNT_TOTAL], s["sync"], ms, s["nbytes"])
        if n in (1, 2, 7):
            assert len(whole) > s["max_packets"], (n, ms, len(whole))
        assert len(whole) >= 5


def _check_ties(s):
    """at every position the reference reports, `ways` rotations share the largest count (two of them at nsync = 66 of the period-4
    streams) and the smallest of them is reported; over the streams every rotation is reported, 0 for the pair (3, 0)"""
    rots = set()
    for k in range(HUNT_S):
        sc = rotation_scores(s["D"][k], s["sync"])
        whole = want_of(s["D"][k], [HUNT_TOTAL], s["sync"], s["min_score"], s["nbytes"])
        assert len(whole) >= 10
        for _, pos, rot, score, _, _ in whole:
            tied = np.nonzero(sc[pos] == sc[pos].max())[0].tolist()
            assert len(tied) == (2 if s["ways"] == 4 and s["nsync"] % 4 else s["ways"]) and rot == tied[0] and score == sc[pos].max()
            if s["ways"] == 2:
                a = s["pair"][k]
                assert tied == sorted((a, (a + 1) & 3)) and rot == (0 if a == 3 else a)
            rots.add(rot)
    assert rots == ({0, 1, 2} if s["ways"] == 2 else {0} if s["nsync"] % 4 == 0 else {0, 1, 2})


def _check_b2b(s):
    """in every even stream the push of k period + 1 dibits begins with the last dibit of a pending packet and completes k + 1 packets,
    nsym // period + 1; the odd streams lie one dibit later and complete k"""
    n, N = s["nsync"], 4 * (s["nbytes"] + 2)
    for cuts in s["cuttings"]:
        big = cuts.index(B2B_K * (n + N) + 1)
        assert cuts[big] // (n + N) + 1 == B2B_K + 1
        for k in range(HUNT_S):
            want = want_of(s["D"][k], cuts, s["sync"], s["min_score"], s["nbytes"])
            here = [r for r in want if r[0] == big]
            assert len(here) == (B2B_K + 1 if k % 2 == 0 else B2B_K), (k, len(here))
            if k % 2 == 0:
                assert here[0][1] + n + N == sum(cuts[:big]) + 1         # its last dibit is the push's first
            assert len(want) == 6 and all(r[5] for r in want)


def b2b_cuttings(lead, period, nsync):
    """[.., k period + 1, ..]: the big push begins at the last dibit of the packet planted at `lead`; the push behind it ends 5 dibits into
    the next packet's payload (an odd have), or 6 (an even one)"""
    out = []
    for into in (5, 6):
        head = [lead + period - 1, B2B_K * period + 1, nsync + into]
        out.append(head + [lead + 6 * period + 20 - sum(head)])
    return out


_SETS = {}


def hunt_sets():
    """the uncoded sets (built once; nothing changes them): dicts of what, sync, nsync, nbytes, min_score, max_packets, D (6, total) dibits, cuttings, check (asserts on the
    reference alone what the set is there for)"""
    if "uncoded" in _SETS:
        return _SETS["uncoded"]
    sets = []
    for n, nbytes, ms in DENSE_NOISE:
        rng = np.random.default_rng(1000 * n + ms)
        sets.append(dict(what="dense noise (%d, %d, %d)" % (n, nbytes, ms), sync=rng.integers(0, 4, n, dtype=np.uint8), nbytes=nbytes, min_score=ms,
                         D=rng.integers(0, 4, (HUNT_S, HUNT_TOTAL), dtype=np.uint8), cuttings=HUNT_CUTTINGS, check=_check_dense))
    t = np.arange(HUNT_TOTAL)
    for n in TIE_NSYNC:
        # a constant word (ring value 0) against ring values a, a + 1, a, ...: rotations a and a + 1 tie at every position
        pair = [0, 1, 2, 3, 3, 1]
        D = np.stack([RING[(a + ((t + (k >= 4)) & 1)) & 3] for k, a in enumerate(pair)]).astype(np.uint8)
        sets.append(dict(what="ties of two, nsync %d" % n, sync=np.zeros(n, np.uint8), nbytes=1, min_score=n // 2, D=D, cuttings=HUNT_CUTTINGS,
                         check=_check_ties, ways=2, pair=pair))
        # and against ring values of period 4: all four rotations tie (at nsync = 66 the two that hold the window's two extra values)
        D = np.stack([RING[(t + k) & 3] for k in range(HUNT_S)]).astype(np.uint8)
        sets.append(dict(what="ties of four, nsync %d" % n, sync=np.zeros(n, np.uint8), nbytes=1, min_score=n // 4, D=D, cuttings=HUNT_CUTTINGS,
                         check=_check_ties, ways=4))
    n, nbytes, lead = 16, 2, 37
    N = 4 * (nbytes + 2)
    rng = np.random.default_rng(77)
    sync = rng.integers(0, 4, n, dtype=np.uint8)
    ks = keystream(N)
    D = rng.integers(0, 4, (HUNT_S, lead + 6 * (n + N) + 20), dtype=np.uint8)
    for k in range(HUNT_S):
        pk = np.concatenate([turn(make_packet(rng, sync, nbytes, ks)[0], int(rng.integers(0, 4))) for _ in range(6)])
        D[k, lead + (k & 1):lead + (k & 1) + len(pk)] = pk
    for M in (B2B_K + 1, B2B_K, 64):
        sets.append(dict(what="back to back, max_packets %d" % M, sync=sync, nbytes=nbytes, min_score=n, max_packets=M, D=D,
                         cuttings=b2b_cuttings(lead, n + N, n), check=_check_b2b))
    for s in sets:
        s.setdefault("max_packets", 64)
        s["nsync"] = len(s["sync"])
    assert tuple(s["what"] for s in sets) == HUNT_SET_NAMES
    _SETS["uncoded"] = sets
    return sets


def set_of_test_1(nsync, nbytes, streams=None):
    """what test_deframe_gpu's test 1 pushes at one parameter pair, in hunt_sets' form: 300 streams of 6000 dibits (or the given ones of them)
    under five cuttings"""
    rng = np.random.default_rng(nsync)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    D = planted_streams(rng, 300, 6000, sync, nbytes)
    cuttings = cuttings_of_test_1(rng, 6000)
    return dict(what="test 1 (%d, %d)" % (nsync, nbytes), sync=sync, nsync=nsync, nbytes=nbytes, min_score=nsync - 3, max_packets=64,
                D=D if streams is None else D[streams], cuttings=cuttings, check=None)


COSTAS_CASE_CUTS = [100, 1, 900, 1999]


def costas_case():
    """what test_deframe_gpu's test 2 pushes: 64 streams of 3000 complex values with -0.0, +0.0 and NaN components sprinkled in, and their
    data rule -> (sync, nbytes, min_score, z (64, 3000, 2) float32, data (64, 3000) uint8)"""
    rng = np.random.default_rng(11)
    S, total, nsync, nbytes = 64, 3000, 40, 12
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    D = planted_streams(rng, S, total, sync, nbytes, max_err=2)
    re = np.where(D & 1, -1.0, 1.0).astype(np.float32) * rng.uniform(0.1, 2.0, D.shape).astype(np.float32)
    im = np.where(D & 2, -1.0, 1.0).astype(np.float32) * rng.uniform(0.1, 2.0, D.shape).astype(np.float32)
    z = np.stack([re, im], axis=-1)
    special = np.array([-0.0, 0.0, np.nan, -np.nan], np.float32)
    sel = rng.random(z.shape) < 0.05
    z[sel] = special[rng.integers(0, 4, int(sel.sum()))]
    return sync, nbytes, nsync - 2, z, data_rule(z)


def old_sets(streams=None):
    """what test_deframe_gpu's tests 1, 1b and 2 push, in hunt_sets' form (tests 1 and 2 cut to the given streams; test 2 as the data rule of
    its costas input, the dibits its special values turn into included)"""
    sets = [set_of_test_1(nsync, nbytes, streams) for nsync, nbytes in ((32, 16), (64, 64), (100, 5))]
    for nsync, nbytes in ((7, 1), (65, 2), (128, 5)):
        sync, D, _ = edge_case(nsync, nbytes)
        sets.append(dict(what="test 1b (%d, %d)" % (nsync, nbytes), sync=sync, nbytes=nbytes, min_score=nsync - 1, D=D, cuttings=EDGE_CUTTINGS))
    sync, nbytes, min_score, _, data = costas_case()
    sets.append(dict(what="test 2", sync=sync, nbytes=nbytes, min_score=min_score, D=data if streams is None else data[streams], cuttings=[COSTAS_CASE_CUTS]))
    for s in sets:
        s.update(max_packets=64, nsync=len(s["sync"]), check=None)
    return sets


def overflow_set():
    """what test_deframe_gpu's test 3 pushes, in hunt_sets' form: ten packets back to back in one push at max_packets = 3"""
    rng = np.random.default_rng(12)
    S, nsync, nbytes, M = 5, 16, 2, 3
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    ks = keystream(4 * (nbytes + 2))
    D = np.concatenate([make_packet(rng, sync, nbytes, ks)[0] for _ in range(10)] + [np.zeros(5, np.uint8)])
    D = np.tile(D, (S, 1))
    return dict(what="test 3", sync=sync, nsync=nsync, nbytes=nbytes, min_score=nsync, max_packets=M, D=D, cuttings=[[D.shape[1]]], check=None)


def hunt_coded_sets(kind):
    """the coded sets of one kind ("plain", "punct", "ilv"): dicts of what, kind, sync, nsync, nbytes, min_score, max_packets, pattern,
    stride, nbody (Nc), z (6, total, 2) float32 rows of costas_frame[], cuttings, gain (6,) float32, the caller's per stream at every push,
    check.  Dense noise (plain and punct) at DENSE_NOISE_CODED: every completion is a decode of garbage.  Back to back at the per-push
    bound per_stream = min(max_packets, nsym / (nsync + Nc) + 1): nbytes = 5 behind the pattern 2/3 has Nc = 47, odd, so the staging rows'
    pitch is rounded up"""
    from test_deframe_coded_cpu import dibits_to_costas, make_coded_packet
    from test_ilv_cpu import ilv_stride, make_coded_ilv_packet
    from test_punct_cpu import NAMED, coded_punct_steps, make_coded_punct_packet, punct_ntx
    if kind in _SETS:
        return _SETS[kind]
    pattern = {"plain": NAMED["1/2"], "punct": NAMED["2/3"], "ilv": NAMED["3/4"]}[kind]
    sets = []

    def costas(rng, d, noise):
        amp = rng.uniform(0.3, 2.0, HUNT_S)
        return np.stack([dibits_to_costas(d[k], amp=float(amp[k]), noise=noise * float(amp[k]), rng=rng) for k in range(HUNT_S)]).astype(np.float32)

    for n, nbytes, ms in DENSE_NOISE_CODED if kind != "ilv" else ():
        rng = np.random.default_rng(2000 * n + ms + len(kind))
        z = costas(rng, rng.integers(0, 4, (HUNT_S, HUNT_TOTAL), dtype=np.uint8), 0.5)
        sets.append(dict(what="%s dense noise (%d, %d, %d)" % (kind, n, nbytes, ms), sync=rng.integers(0, 4, n, dtype=np.uint8), nbytes=nbytes, min_score=ms,
                         max_packets=64, z=z, cuttings=HUNT_CUTTINGS, gain=rng.uniform(20.0, 90.0, HUNT_S).astype(np.float32), check=_check_dense_coded))
    n, nbytes, lead = 16, 2 if kind == "plain" else 5, 37
    Nc = punct_ntx(coded_punct_steps(nbytes), pattern)
    stride = ilv_stride(2 * Nc, 2 * Nc // 16) if kind == "ilv" else None
    if kind == "punct":
        assert Nc == 47
    rng = np.random.default_rng(88 + len(kind))
    sync = rng.integers(0, 4, n, dtype=np.uint8)
    d = rng.integers(0, 4, (HUNT_S, lead + 6 * (n + Nc) + 20), dtype=np.uint8)
    for k in range(HUNT_S):
        make = {"plain": lambda: make_coded_packet(rng, sync, nbytes), "punct": lambda: make_coded_punct_packet(rng, sync, nbytes, pattern),
                "ilv": lambda: make_coded_ilv_packet(rng, sync, nbytes, pattern, stride)}[kind]
        pk = np.concatenate([turn(make()[0], int(rng.integers(0, 4))) for _ in range(6)])
        d[k, lead + (k & 1):lead + (k & 1) + len(pk)] = pk
    z = costas(rng, d, 0.1)
    gain = rng.uniform(40.0, 90.0, HUNT_S).astype(np.float32)
    for M in (B2B_K + 1, B2B_K, 64):
        sets.append(dict(what="%s back to back, max_packets %d" % (kind, M), sync=sync, nbytes=nbytes, min_score=n, max_packets=M, z=z,
                         cuttings=b2b_cuttings(lead, n + Nc, n), gain=gain, check=_check_b2b_coded))
    for s in sets:
        s.update(kind=kind, pattern=pattern, stride=stride, nsync=len(s["sync"]), nbody=punct_ntx(coded_punct_steps(s["nbytes"]), pattern))
    assert tuple(s["what"] for s in sets) == HUNT_CODED_SET_NAMES[kind]
    _SETS[kind] = sets
    return sets


def coded_reference(s, cuts):
    """per stream the reference's packets of a coded set under one cutting, push by push (deframe_coded_ref's form, `soft` included)"""
    from test_deframe_coded_cpu import deframe_coded_ref
    from test_ilv_cpu import deframe_coded_ilv_ref
    from test_punct_cpu import deframe_coded_punct_ref
    at = np.cumsum([0] + list(cuts))
    out = []
    for k in range(HUNT_S):
        rows, gains = [s["z"][k, a:b] for a, b in zip(at[:-1], at[1:])], [s["gain"][k]] * len(cuts)
        if s["kind"] == "plain":
            out.append(deframe_coded_ref(rows, gains, s["sync"], s["min_score"], s["nbytes"]))
        elif s["kind"] == "punct":
            out.append(deframe_coded_punct_ref(rows, gains, s["sync"], s["min_score"], s["nbytes"], s["pattern"]))
        else:
            out.append(deframe_coded_ilv_ref(rows, gains, s["sync"], s["min_score"], s["nbytes"], s["pattern"], s["stride"]))
    return out


def _check_dense_coded(s, refs):
    """refs: coded_reference per cutting.  Every stream completes packets by the dozen, and no decode of noise passes its CRC by design"""
    from test_rx_data_cpu import data_rule as rule
    for k in range(HUNT_S):
        sc = rotation_scores(rule(s["z"][k]), s["sync"]).max(axis=1)
        assert (sc >= s["min_score"]).mean() > 0.02
    for ref in refs:
        assert all(sum(len(push) for push in ref[k]) >= 10 for k in range(HUNT_S))


def _check_b2b_coded(s, refs):
    n, Nc = s["nsync"], s["nbody"]
    for cuts, ref in zip(s["cuttings"], refs):
        big = cuts.index(B2B_K * (n + Nc) + 1)
        assert cuts[big] // (n + Nc) + 1 == B2B_K + 1
        for k in range(HUNT_S):
            assert len(ref[k][big]) == (B2B_K + 1 if k % 2 == 0 else B2B_K), (k, len(ref[k][big]))
            if k % 2 == 0:
                assert ref[k][big][0]["end"] == sum(cuts[:big]) + 1
            assert sum(len(push) for push in ref[k]) == 6 and all(p["crc_ok"] for push in ref[k] for p in push)


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
