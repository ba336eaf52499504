"""Stream positions beyond 32 bits, both deframers.

The deframers keep len, h and ppos as 64-bit values and do a push's arithmetic in int after taking base0 off; d_pos is long long because
the streams are continuous.  No test can push 2^31 symbols, so qpsk_test_deframer_advance moves the counters: push 600 symbols, advance,
push the rest in cuts of 97.  Every record of a later push must be the reference's with pos + delta and nothing else changed -- the packets
that were pending across the advance included.  The references are deframe_ref, deframe_coded_ref and deframe_coded_punct_ref on the
unmoved stream, computed once per deframer; everything is bit for bit.
"""
import functools

import numpy as np
import pytest

from test_deframe_coded_cpu import coded_steps, dibits_to_costas
from test_deframe_coded_gpu import planted_costas, rows_of
from test_deframe_coded_gpu import push_all as push_coded
from test_deframe_coded_gpu import want_all as want_half
from test_deframe_coded_punct_gpu import want_all as want_punct
from test_deframe_cpu import turn
from test_deframe_gpu import modem, planted_streams, push_all, want_of
from test_punct_cpu import NAMED, make_coded_punct_packet, punct_nsent, punct_ntx

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
S, NSYNC, TOTAL, FIRST, CUT = 4, 32, 3000, 600, 97
CUTS = [FIRST] + [CUT] * ((TOTAL - FIRST) // CUT) + [(TOTAL - FIRST) % CUT]
DELTAS = {"2^31": (1 << 31) - 700, "2^32": (1 << 32) - 700, "2^40": (1 << 40) + 1}
SEEDS = {"plain": 1, "coded": 1, "2/3": 5}


def punct_streams(rng, sync, nbytes, pattern, noise=0.08):
    """S streams of TOTAL symbols: punctured packets at random gaps and rotations between random dibits, at a random amplitude plus noise"""
    d = rng.integers(0, 4, (S, TOTAL), dtype=np.uint8)
    for s in range(S):
        t = int(rng.integers(0, 150))
        while True:
            pkt = turn(make_coded_punct_packet(rng, sync, nbytes, pattern, corrupt=bool(rng.integers(0, 8) == 0))[0], int(rng.integers(0, 4)))
            if t + len(pkt) > TOTAL:
                break
            d[s, t:t + len(pkt)] = pkt
            t += len(pkt) + int(rng.integers(0, 150))
    return np.stack([dibits_to_costas(d[s], amp=float(rng.uniform(0.3, 2.0)), noise=0.0) for s in range(S)]) \
        + (noise * rng.standard_normal((S, TOTAL, 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scenario(kind):
    """the streams, their pushes and the reference's records (push, pos, rot, score, bytes, crc_ok[, info]) per stream; asserts what the
    test is about from the reference alone: in every stream a packet completes in the first push, in two streams or more a packet is
    pending at symbol FIRST, and later records start on both sides of symbol 700, where the first two deltas put 2^31 and 2^32"""
    rng = np.random.default_rng(SEEDS[kind])
    sync = rng.integers(0, 4, NSYNC, dtype=np.uint8)
    min_score = NSYNC - 3
    c = dict(kind=kind, sync=sync, min_score=min_score)
    if kind == "plain":
        c["nbytes"], body = 16, 4 * 18
        D = planted_streams(rng, S, TOTAL, sync, 16)
        c["rows"] = [np.ascontiguousarray(D[:, a:a + n]) for a, n in zip(np.cumsum([0] + CUTS[:-1]), CUTS)]
        c["want"] = [want_of(D[s], CUTS, sync, min_score, 16) for s in range(S)]
    elif kind == "coded":
        c["nbytes"], body = 16, coded_steps(16)
        z = planted_costas(rng, S, TOTAL, sync, 16, gap=150)
        c["rows"] = rows_of(z, CUTS)
        c["gains"] = rng.uniform(30.0, 90.0, (len(CUTS), S)).astype(np.float32)
        c["want"] = want_half(c["rows"], c["gains"], sync, min_score, 16)
    else:
        pattern = NAMED[kind]
        c["nbytes"], body = 5, punct_ntx(coded_steps(5), pattern)
        assert punct_nsent(coded_steps(5), pattern) & 1                  # the odd-nsent shape
        z = punct_streams(rng, sync, 5, pattern)
        c["rows"] = rows_of(z, CUTS)
        c["gains"] = None                                                # every push takes its row's own
        c["want"] = want_punct(c["rows"], None, sync, min_score, 5, pattern)
    assert [r.shape[1] for r in c["rows"]] == CUTS
    want = c["want"]
    assert all(any(r[0] == 0 for r in w) for w in want), [sum(r[0] == 0 for r in w) for w in want]
    pending = [s for s in range(S) if any(r[1] + NSYNC <= FIRST < r[1] + NSYNC + body for r in want[s])]
    assert len(pending) >= 2, pending
    later = [r[1] for w in want for r in w if r[0] > 0]
    assert min(later) < 700 <= max(later)
    assert sum(len(w) for w in want) >= 3 * S
    return c


def reset(m, c):
    if c["kind"] == "plain":
        m.deframer_reset(S, c["sync"], c["nbytes"], c["min_score"], max_packets=8)
    else:
        m.deframer_reset_coded(S, c["sync"], c["nbytes"], c["min_score"], max_packets=8, puncture=None if c["kind"] == "coded" else c["kind"])


def push(m, c, first, last):
    """pushes [first, last) -> the records per stream, numbered by push as the reference's"""
    if c["kind"] == "plain":
        got = push_all(m, c["rows"][first:last])
    else:
        got = push_coded(m, c["rows"][first:last], None if c["gains"] is None else c["gains"][first:last])
    return [[(r[0] + first,) + r[1:] for r in g] for g in got]


def moved(want, delta):
    return [[(r[0], r[1] + (delta if r[0] > 0 else 0)) + r[2:] for r in w] for w in want]


@pytest.mark.parametrize("delta", sorted(DELTAS))
@pytest.mark.parametrize("kind", ["plain", "coded", "2/3"])
def test_records_behind_an_advance_are_the_reference_s_with_the_position_moved(kind, delta):
    c = scenario(kind)
    d = DELTAS[delta]
    want = moved(c["want"], d)
    if delta != "2^40":                                                  # positions on both sides of the power of two
        at = [r[1] for w in want for r in w if r[0] > 0]
        assert min(at) < (1 << int(delta[2:])) <= max(at)
    m = modem()
    reset(m, c)
    got = push(m, c, 0, 1)
    m.deframer_advance(d)
    later = push(m, c, 1, len(c["rows"]))
    m.sync()
    for s in range(S):
        assert got[s] == [r for r in want[s] if r[0] == 0], (s, got[s][:1])
        assert later[s] == [r for r in want[s] if r[0] > 0], (s, later[s][:2], [r for r in want[s] if r[0] > 0][:2])
    m.close()


@pytest.mark.parametrize("kind", ["plain", "coded"])
def test_a_refused_advance_changes_nothing(kind):
    c = scenario(kind)
    m = modem()
    adv = lambda delta: m.L.qpsk_test_deframer_advance(m.h, delta)      # noqa: E731
    assert adv(5) == QPSK_ERR_STATE                                      # before a reset
    assert b"qpsk_test_deframer_advance" in m.L.qpsk_last_error()
    reset(m, c)
    assert adv(5) == QPSK_ERR_STATE                                      # len = 0: no carried tail yet
    assert adv(-1) == QPSK_ERR_ARG
    got = push(m, c, 0, 1)
    assert adv(-1) == QPSK_ERR_ARG and adv((1 << 62) + 1) == QPSK_ERR_ARG
    later = push(m, c, 1, len(c["rows"]))
    m.sync()
    for s in range(S):
        assert got[s] + later[s] == c["want"][s], s
    # a stream that has seen fewer than nsync - 1 dibits: refused; with nsync - 1 the tail is whole and the call goes through
    reset(m, c)
    short = [r[:, :NSYNC - 2] for r in c["rows"][:1]] + [r[:, NSYNC - 2:NSYNC - 1] for r in c["rows"][:1]]
    for k, r in enumerate(short):
        if kind == "plain":
            m.deframe(data=np.ascontiguousarray(r))
        else:
            m.deframe_coded(np.ascontiguousarray(r), c["gains"][0])
        assert adv(7) == (QPSK_ERR_STATE if k == 0 else 0), k
    m.sync()
    m.close()
