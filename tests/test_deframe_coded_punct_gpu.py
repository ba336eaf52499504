"""qpsk_deframer_reset_coded_punct + qpsk_deframer_push_coded on the GPU against deframe_coded_punct_ref (test_punct_cpu.py), which restates
include/qpsk_hip.h.  Everything is bit for bit; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_cpu import dibits_to_costas
from test_deframe_coded_gpu import hunt_set_on_the_device, modem, push_all, rec, rows_of
from test_deframe_cpu import HUNT_CODED_SET_NAMES, hunt_coded_sets, turn
from test_punct_cpu import NAMED, coded_punct_steps, deframe_coded_punct_ref, make_coded_punct_packet, punct_nsent, punct_ntx

pytestmark = pytest.mark.gpu

QPSK_ERR_STATE = -5
S = 3


def want_all(rows, gains, sync, min_score, nbytes, pattern):
    out = []
    for s in range(rows[0].shape[0]):
        ref = deframe_coded_punct_ref([r[s] for r in rows], None if gains is None else [g[s] for g in gains], sync, min_score, nbytes, pattern)
        out.append([rec(k, p) for k, push in enumerate(ref) for p in push])
    return out


def planted(rng, sync, nbytes, pattern, total):
    """S streams of `total` symbols: six packets each at random rotations -- packets 1 and 2 and packets 4 and 5 back to back, packet 3
    with a wrong CRC -- between random dibits, on the diagonals at a random amplitude plus Gaussian noise"""
    d = rng.integers(0, 4, (S, total), dtype=np.uint8)
    for s in range(S):
        t = int(rng.integers(0, 30))
        for q in range(6):
            pkt, _ = make_coded_punct_packet(rng, sync, nbytes, pattern, corrupt=q == 3)
            pkt = turn(pkt, int(rng.integers(0, 4)))
            assert t + len(pkt) <= total
            d[s, t:t + len(pkt)] = pkt
            t += len(pkt) + (0 if q in (1, 4) else int(rng.integers(1, 40)))
    return np.stack([dibits_to_costas(d[s], amp=float(rng.uniform(0.3, 2.0)), noise=0.0) for s in range(S)]) \
        + (0.08 * rng.standard_normal((S, total, 2))).astype(np.float32)


def random_cuts(rng, total):
    """3 to 6 pushes of random sizes"""
    k = int(rng.integers(3, 7))
    at = np.sort(rng.choice(np.arange(1, total), k - 1, replace=False))
    return np.diff(np.concatenate([[0], at, [total]])).tolist()


@pytest.mark.parametrize("with_gain", [True, False])
@pytest.mark.parametrize("name", sorted(NAMED))
@pytest.mark.parametrize("nbytes", [5, 16])
def test_punctured_packets_bit_for_bit_for_random_cuts(nbytes, name, with_gain):
    """nbytes = 5: 62 steps, so nsent = 93 is odd at rate 2/3 and the staged rows are an odd number of dibits long"""
    pattern = NAMED[name]
    rng = np.random.default_rng(100 * nbytes + len(name) + sorted(NAMED).index(name))
    nsync = 24
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    Nc = punct_ntx(coded_punct_steps(nbytes), pattern)
    if (nbytes, name) == (5, "2/3"):
        assert punct_nsent(62, pattern) == 93 and Nc == 47
    total = 6 * (nsync + Nc) + 250
    z = planted(rng, sync, nbytes, pattern, total).astype(np.float32)
    m = modem()
    seen, straddled = [], 0
    for trial in range(2):
        rows = rows_of(z, random_cuts(rng, total))
        assert 3 <= len(rows) <= 6
        gains = np.tile(rng.uniform(40.0, 90.0, (1, S)), (len(rows), 1)).astype(np.float32)
        gains = gains if with_gain else None
        m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=8, puncture=name)
        got = push_all(m, rows, gains)
        assert "deframe_coded_decode_punct_kernel" in m.last_kernel(), m.last_kernel()
        want = want_all(rows, gains, sync, nsync - 3, nbytes, pattern)
        for s in range(S):
            assert got[s] == want[s], (trial, s, got[s][:1], want[s][:1])
        edges = np.cumsum([r.shape[1] for r in rows])[:-1]
        straddled += sum(bool(((edges > r[1]) & (edges < r[1] + nsync + Nc)).any()) for g in want for r in g)
        seen.append(got)
    assert straddled >= 1                                                 # some packet's symbols came in more than one push
    good = [[r for r in g if r[5]] for g in seen[0]]
    assert all(len(g) >= 5 for g in good) and any(not r[5] for g in seen[0] for r in g)      # the payloads come back; the bad CRC shows
    m.close()


@pytest.mark.parametrize("what", HUNT_CODED_SET_NAMES["punct"])
def test_the_hunt_on_dense_candidates_and_at_the_per_push_bound_behind_the_pattern_2_3(what):
    """test_deframe_coded_gpu's cases behind a pattern: the back-to-back sets have nbytes = 5, so Nc = 47 is odd, the staging rows lie
    stage_pitch = 48 dibits apart, and the pending body is copied with an odd and an even number of pairs"""
    hunt_set_on_the_device(next(s for s in hunt_coded_sets("punct") if s["what"] == what))


@pytest.mark.parametrize("route", [0, 1])
def test_the_pattern_1_1_1_equals_the_unpunctured_reset_and_both_routes_agree(route):
    rng = np.random.default_rng(7)
    nbytes, nsync = 16, 24
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    total = 6 * (nsync + coded_punct_steps(nbytes)) + 250
    z = planted(rng, sync, nbytes, NAMED["1/2"], total).astype(np.float32)
    rows = rows_of(z, random_cuts(rng, total))
    m = modem()
    m.tune(viterbi_lds=route)
    for gains in (np.full((len(rows), S), 60.0, np.float32), None):
        m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=8)
        a = push_all(m, rows, gains)
        ka = m.last_kernel()
        m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=8, puncture=(1, 1, 1))
        b = push_all(m, rows, gains)
        kb = m.last_kernel()
        word = "<lds>" if route else "<global>"
        assert "punct" not in ka and "punct" in kb and word in ka and word in kb, (ka, kb)
        assert a == b and sum(len(x) for x in a) >= 5 * S
    m.close()


def test_an_uncoded_push_after_the_punctured_reset_is_refused():
    import torch
    m = modem()
    sw = (C.c_uint8 * 16)(*([1, 2, 3, 0] * 4))
    z = torch.zeros((2, 100, 2), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert m.L.qpsk_deframer_reset_coded_punct(m.h, 2, sw, 16, 14, 4, 4, 0, 64.0, 3, 5, 3) == 0
    assert m.L.qpsk_deframer_push(m.h, P(z), None, 100, P(cnt), None, None, None, None, None) == QPSK_ERR_STATE
    assert m.L.qpsk_deframer_push_coded(m.h, P(z), 100, None, P(cnt), None, None, None, None, None, None) == 0
    m.sync()
    m.close()
