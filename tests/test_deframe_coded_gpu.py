"""qpsk_deframer_reset_coded / qpsk_deframer_push_coded on the GPU against deframe_coded_ref (test_deframe_coded_cpu.py), which restates
include/qpsk_hip.h.  Everything is bit for bit; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_cpu import (LINK, coded_link_pcm, coded_steps, cut, deframe_coded_ref, dibits_to_costas, link_rows,
                                    make_coded_packet)
from test_deframe_cpu import HUNT_CODED_SET_NAMES, HUNT_S, coded_reference, deframe_ref, hunt_coded_sets, keystream, turn
from test_rx_data_cpu import data_rule

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE, QPSK_ERR_RANGE = -2, -5, -6
KEYS = ("pos", "rot", "score", "bytes", "crc_ok", "info")


def modem(**kw):
    import qpsk_amd
    return qpsk_amd.Modem(**kw)


def rec(k, p):
    return (k, int(p["pos"]), int(p["rot"]), int(p["score"]), np.asarray(p["bytes"], np.uint8).tobytes(), bool(p["crc_ok"]),
            tuple(int(v) for v in p["info"]))


def push_all(m, rows, gains=None):
    """rows: list of (S, nsym, 2); gains: None or (npush, S) -> per stream the records (push, pos, rot, score, bytes, crc_ok, info)"""
    S = rows[0].shape[0]
    got = [[] for _ in range(S)]
    for k, r in enumerate(rows):
        o = m.deframe_coded(np.ascontiguousarray(r), None if gains is None else np.ascontiguousarray(gains[k], np.float32))
        h = {key: o[key].cpu().numpy() for key in KEYS + ("count",)}
        assert (h["count"] <= h["pos"].shape[1]).all(), "more packets in one push than the test's max_packets"
        for s in range(S):
            got[s] += [rec(k, {key: h[key][s, j] for key in KEYS}) for j in range(h["count"][s])]
    m.sync()
    return got


def want_all(rows, gains, sync, min_score, nbytes, mode="unit", scale=64.0):
    S = rows[0].shape[0]
    out = []
    for s in range(S):
        ref = deframe_coded_ref([r[s] for r in rows], None if gains is None else [g[s] for g in gains], sync, min_score, nbytes, mode, scale)
        out.append([rec(k, p) for k, push in enumerate(ref) for p in push])
    return out


def planted_costas(rng, S, total, sync, nbytes, max_err=3, noise=0.3, gap=300, burst=40):
    """S streams of dibits on the diagonals at a random amplitude plus Gaussian noise; packets at random gaps and rotations with
    0..max_err dibit errors in the word, one in eight with a wrong CRC, one in eight with a stretch of `burst` dibits of its body
    replaced by random dibits (beyond the code)"""
    d = rng.integers(0, 4, (S, total), dtype=np.uint8)
    for s in range(S):
        t = int(rng.integers(0, gap))
        while True:
            pkt, _ = make_coded_packet(rng, sync, nbytes, corrupt=bool(rng.integers(0, 8) == 0))
            if rng.integers(0, 8) == 0:
                a = len(sync) + int(rng.integers(0, len(pkt) - len(sync) - burst))
                pkt[a:a + burst] = rng.integers(0, 4, burst, dtype=np.uint8)
            pkt = turn(pkt, int(rng.integers(0, 4)))
            for i in rng.choice(len(sync), int(rng.integers(0, max_err + 1)), replace=False):
                pkt[i] = (pkt[i] + 1 + rng.integers(0, 3)) & 3
            if t + len(pkt) > total:
                break
            d[s, t:t + len(pkt)] = pkt
            t += len(pkt) + int(rng.integers(0, gap))
    amp = rng.uniform(0.2, 3.0, (S, 1))
    z = np.stack([amp * (1.0 - 2.0 * (d & 1)), amp * (1.0 - 2.0 * (d >> 1))], axis=-1)
    return (z + noise * amp[..., None] * rng.standard_normal(z.shape)).astype(np.float32)


def rows_of(z, cuts):
    return [np.ascontiguousarray(z[:, a:b]) for a, b in zip(np.cumsum([0] + cuts[:-1]), np.cumsum(cuts)) if b > a]


# ------------------------------------------------------------------- 1. synthetic streams, all seven outputs, any cuts, caller's gains
@pytest.mark.parametrize("nsync,nbytes,S,total", [(32, 16, 24, 1500), (64, 64, 16, 3000), (100, 5, 24, 900), (128, 1024, 5, 20000)])
def test_planted_packets_bit_for_bit_for_every_cut_with_the_caller_s_gains(nsync, nbytes, S, total):
    rng = np.random.default_rng(nsync)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    min_score = nsync - 3
    z = planted_costas(rng, S, total, sync, nbytes)
    m = modem()
    mixed = []
    while sum(mixed) < total:
        mixed.append(int(rng.choice([1, 7, 128, 2048, int(rng.integers(1, 700))])))
    mixed[-1] -= sum(mixed) - total
    seen = []
    for cuts, vary in (([total], False), ([97] * (total // 97) + [total % 97], True), ([total // 3 + 1] * 3, False), (mixed, True)):
        rows = rows_of(z, [c for c in cuts if c > 0])
        gains = (rng.uniform(20.0, 90.0, (len(rows), S)) if vary else np.tile(rng.uniform(20.0, 90.0, (1, S)), (len(rows), 1))).astype(np.float32)
        m.deframer_reset_coded(S, sync, nbytes, min_score, max_packets=64)
        got = push_all(m, rows, gains)
        want = want_all(rows, gains, sync, min_score, nbytes)
        for s in range(S):
            assert got[s] == want[s], (cuts[:4], s, got[s][:1], want[s][:1])
        seen.append(sum(len(g) for g in got))
        assert "deframe_coded_decode_kernel" in m.last_kernel()
    assert min(seen) >= S and len(set(seen)) == 1
    assert any(r[5] for g in got for r in g) and any(not r[5] for g in got for r in g)      # CRC passes and failures both occur
    m.close()


def test_one_symbol_per_push_on_a_short_stream():
    rng = np.random.default_rng(2)
    nsync, nbytes, S, total = 32, 16, 8, 520
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = planted_costas(rng, S, total, sync, nbytes, gap=60)
    g = np.tile(rng.uniform(30.0, 80.0, (1, S)).astype(np.float32), (total, 1))
    m = modem()
    m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=4)
    rows = rows_of(z, [1] * total)
    got = push_all(m, rows, g)
    assert got == want_all(rows, g, sync, nsync - 3, nbytes) and sum(len(x) for x in got) >= S
    m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=4)
    whole = push_all(m, [z], g[:1])
    assert [[r[1:] for r in x] for x in whole] == [[r[1:] for r in x] for x in got]      # a constant gain: the cuts do not show
    m.close()


EDGE_CUTTINGS = ([1] * 200 + [1300], [97] * 15 + [45])


def edge_case(nsync, nbytes):
    """6 streams of 1500 symbols for a word of nsync dibits, and per cutting the rows, the caller's gains and the reference's records.
    The seed is chosen so that the reference, before anything is compared with it, shows two packets in every stream and, under either
    cutting, a packet that ends in a later push than the one that completed its sync word"""
    rng = np.random.default_rng(200 + nsync)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = planted_costas(rng, 6, 1500, sync, nbytes, max_err=1, burst=10)
    cases = []
    for cuts in EDGE_CUTTINGS:
        ends = np.cumsum(cuts)
        rows = rows_of(z, cuts)
        gains = rng.uniform(20.0, 90.0, (len(rows), 6)).astype(np.float32)
        want = want_all(rows, gains, sync, nsync - 1, nbytes)
        assert all(len(w) >= 2 for w in want), [len(w) for w in want]
        assert any(r[0] > np.searchsorted(ends, r[1] + nsync) for w in want for r in w)
        cases.append((rows, gains, want))
    return sync, cases


@pytest.mark.parametrize("nsync,nbytes", [(7, 1), (65, 2)])
def test_words_of_7_and_65_dibits_with_the_caller_s_gains(nsync, nbytes):
    sync, cases = edge_case(nsync, nbytes)
    m = modem()
    for rows, gains, want in cases:
        m.deframer_reset_coded(6, sync, nbytes, nsync - 1, max_packets=64)
        assert push_all(m, rows, gains) == want, (nsync, len(rows))
    m.close()


# ------------------------------------------------------------------- 2. no gain given: the row's own, both modes, both soft routes
@pytest.mark.parametrize("mode", ["unit", "llr"])
def test_without_a_gain_every_push_takes_its_row_s_own(mode):
    rng = np.random.default_rng(3)
    nsync, nbytes, S, total = 48, 32, 12, 9000
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = planted_costas(rng, S, total, sync, nbytes, noise=0.25)
    z[:, 4000:] *= np.float32(1.6)
    rows = rows_of(z, [3000, 5000, 100, 900])                            # rows on both sides of 4096 symbols
    m = modem()
    m.deframer_reset_coded(S, sync, nbytes, nsync - 4, max_packets=32, mode=mode, scale=40.0)
    got = push_all(m, rows)
    assert got == want_all(rows, None, sync, nsync - 4, nbytes, mode, 40.0) and sum(len(x) for x in got) > 3 * S
    m.close()


# ------------------------------------------------------------------- 3. the decoder's two routes
def test_decision_words_in_lds_and_in_the_scratch_buffer_give_equal_outputs():
    rng = np.random.default_rng(4)
    nsync, nbytes, S, total = 40, 200, 10, 8000
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = planted_costas(rng, S, total, sync, nbytes)
    rows = rows_of(z, [2500, 2500, 3000])
    g = np.full((3, S), 55.0, np.float32)
    m = modem()
    outs = []
    for lds, name in ((1, "<lds>"), (0, "<global>")):
        m.tune(viterbi_lds=lds)
        m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=8)
        outs.append(push_all(m, rows, g))
        assert name in m.last_kernel(), m.last_kernel()
    assert outs[0] == outs[1] == want_all(rows, g, sync, nsync - 3, nbytes) and sum(len(x) for x in outs[0]) >= S
    m.close()


# ------------------------------------------------------------------- 4. overflow; each output alone
def back_to_back(rng, sync, nbytes, npk, S):
    d = np.concatenate([make_coded_packet(rng, sync, nbytes)[0] for _ in range(npk)] + [np.zeros(5, np.uint8)])
    return np.tile(dibits_to_costas(d, amp=0.8, noise=0.2, rng=rng), (S, 1, 1))


def raw_push(m, z, gain, M, nbytes, which=KEYS, guard=1):
    """the C call with guarded buffers of M + guard rows per stream; outputs not in `which` are passed as NULL -> dict of numpy arrays"""
    import torch
    S = z.shape[0]
    shapes = dict(bytes=((nbytes + 2,), torch.uint8, 0xA5), pos=((), torch.int64, -7), rot=((), torch.int32, -7), score=((), torch.int32, -7),
                  crc_ok=((), torch.uint8, 0xA5), info=((4,), torch.int32, -7))
    bufs = {k: torch.full((S * (M + guard),) + shapes[k][0], shapes[k][2], dtype=shapes[k][1], device="cuda") for k in KEYS}
    cnt = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    zt = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    gt = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, np.float32)).cuda()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    rc = m.L.qpsk_deframer_push_coded(m.h, P(zt), z.shape[1], P(gt), P(cnt), *[P(bufs[k]) if k in which else None for k in
                                                                               ("bytes", "pos", "rot", "score", "crc_ok", "info")])
    assert rc == 0, m.L.qpsk_last_error()
    m.sync()
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    out["count"] = cnt.cpu().numpy()
    return out


def test_overflow_counts_everything_and_writes_only_max_packets():
    """even streams hold ten packets, odd streams none: in the [S][M] packed outputs every overflowing stream's rows are followed
    directly by rows that must stay untouched (the next stream's, then the guard behind the last stream)"""
    rng = np.random.default_rng(5)
    S, nsync, nbytes, M = 6, 16, 2, 3
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = back_to_back(rng, sync, nbytes, 10, S)
    z[1::2] = dibits_to_costas(np.zeros(z.shape[1], np.uint8), amp=0.8)
    g = np.full(S, 70.0, np.float32)
    m = modem()
    m.deframer_reset_coded(S, sync, nbytes, nsync, max_packets=M)
    o = raw_push(m, z, g, M, nbytes)
    want = [p for p in deframe_coded_ref([z[0]], [70.0], sync, nsync, nbytes)[0]]
    assert len(want) == 10 and deframe_coded_ref([z[1]], [70.0], sync, nsync, nbytes) == [[]]
    assert o["count"].tolist() == [10, 0] * (S // 2)
    canary = dict(bytes=0xA5, pos=-7, rot=-7, score=-7, crc_ok=0xA5, info=-7)
    for s in range(0, S, 2):
        for j in range(M):
            assert rec(0, {k: o[k][s * M + j] for k in KEYS}) == rec(0, want[j]), (s, j)
        for k in KEYS:
            assert (o[k][(s + 1) * M:(s + 2) * M] == canary[k]).all(), (s, k)      # the rows right behind stream s's
    for k in KEYS:
        assert (o[k][S * M:] == canary[k]).all(), k                      # and the guard behind the whole block
    m.close()


# ------------------------------------------------------------------- 4b. the hunt where candidates are dense, and at the per-push bound
def hunt_set_on_the_device(s):
    """one set of test_deframe_cpu.hunt_coded_sets (any kind: the reset follows the set's) under each of its cuttings, push by push through
    raw_push's guarded buffers: count, and pos, rot, score, bytes, crc_ok, info of every row a push writes against the set's reference,
    with the push; the rows of a stream beyond min(count, max_packets) and the guard rows come back as they went in"""
    M, nbytes = s["max_packets"], s["nbytes"]
    canary = dict(bytes=0xA5, pos=-7, rot=-7, score=-7, crc_ok=0xA5, info=-7)
    refs = [coded_reference(s, cuts) for cuts in s["cuttings"]]
    s["check"](s, refs)
    m = modem()
    for cuts, ref in zip(s["cuttings"], refs):
        m.deframer_reset_coded(HUNT_S, s["sync"], nbytes, s["min_score"], max_packets=M, puncture=None if s["kind"] == "plain" else s["pattern"],
                               interleave=s["stride"])
        at = 0
        for k, c in enumerate(cuts):
            o = raw_push(m, s["z"][:, at:at + c], s["gain"], M, nbytes)
            at += c
            for j in range(HUNT_S):
                want = ref[j][k]
                assert o["count"][j] == len(want), (s["what"], cuts[:2], k, j)
                w = min(len(want), M)
                for q in range(w):
                    assert o["crc_ok"][j * M + q] in (0, 1)
                    assert rec(k, {key: o[key][j * M + q] for key in KEYS}) == rec(k, want[q]), (s["what"], cuts[:2], k, j, q)
                for key in KEYS:
                    assert (o[key][j * M + w:(j + 1) * M] == canary[key]).all(), (s["what"], k, j, key)
            for key in KEYS:
                assert (o[key][HUNT_S * M:] == canary[key]).all(), (s["what"], k, key)
        word = {"plain": "deframe_coded_decode_kernel", "punct": "deframe_coded_decode_punct_kernel", "ilv": "deframe_coded_decode_ilv_kernel"}[s["kind"]]
        assert word in m.last_kernel(), m.last_kernel()
    m.close()


@pytest.mark.parametrize("what", HUNT_CODED_SET_NAMES["plain"])
def test_the_hunt_on_dense_candidates_and_at_the_per_push_bound(what):
    """rate 1/2.  Dense noise: every completion is a Viterbi decode of garbage, compared bit for bit all the same.  Back to back: a push of
    k (nsync + Nc) + 1 symbols that begins with the last symbol of a pending body completes k + 1 packets, per_stream's nsym term at
    equality; at max_packets = k the cap bites (count k + 1, k rows written)"""
    hunt_set_on_the_device(next(s for s in hunt_coded_sets("plain") if s["what"] == what))


def test_each_output_alone_equals_all_together_and_null_outputs_are_never_written():
    rng = np.random.default_rng(6)
    S, nsync, nbytes, M = 7, 24, 9, 4
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = back_to_back(rng, sync, nbytes, 3, S)
    m = modem()
    for gain in (np.full(S, 50.0, np.float32), None):
        m.deframer_reset_coded(S, sync, nbytes, nsync - 1, max_packets=M)
        full = raw_push(m, z, gain, M, nbytes, guard=0)
        assert (full["count"] == 3).all() and full["crc_ok"].reshape(S, M)[:, :3].all()
        for only in KEYS + (None,):
            m.deframer_reset_coded(S, sync, nbytes, nsync - 1, max_packets=M)
            o = raw_push(m, z, gain, M, nbytes, which=() if only is None else (only,), guard=0)
            assert np.array_equal(o["count"], full["count"])
            for k in KEYS:
                if k == only:
                    assert np.array_equal(o[k], full[k]), k
                else:
                    assert (o[k] == (0xA5 if o[k].dtype == np.uint8 else -7)).all(), (only, k)      # never handed over, never written
    m.close()


# ------------------------------------------------------------------- 5. errors and state
def test_errors_state_and_rereset():
    import torch
    m = modem()
    L, h = m.L, m.h
    d = torch.zeros((4, 100), dtype=torch.uint8, device="cuda")
    z = torch.zeros((4, 100, 2), dtype=torch.float32, device="cuda")
    g = torch.ones(4, dtype=torch.float32, device="cuda")
    cnt = torch.full((4,), -3, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    push = lambda *a: L.qpsk_deframer_push_coded(h, *a)  # noqa: E731
    plain = lambda: L.qpsk_deframer_push(h, P(z), None, 100, P(cnt), None, None, None, None, None)  # noqa: E731
    none7 = (None,) * 6
    assert push(P(z), 100, P(g), P(cnt), *none7) == QPSK_ERR_STATE                                   # before any reset
    sw = (C.c_uint8 * 130)(*([1, 2, 3, 0] * 32 + [1, 2]))
    bad_resets = [(0, 16, 8, 4, 8, 0, 64.0), (4, 0, 1, 4, 8, 0, 64.0), (4, 129, 8, 4, 8, 0, 64.0), (4, 16, 0, 4, 8, 0, 64.0),
                  (4, 16, 17, 4, 8, 0, 64.0), (4, 16, 8, 0, 8, 0, 64.0), (4, 16, 8, 1025, 8, 0, 64.0), (4, 16, 8, 4, 0, 0, 64.0),
                  (4, 16, 8, 4, 65, 0, 64.0), (4, 16, 8, 4, 8, 2, 64.0), (4, 16, 8, 4, 8, -1, 64.0), (4, 16, 8, 4, 8, 0, 0.0),
                  (4, 16, 8, 4, 8, 1, float("inf")), (4, 16, 8, 4, 8, 1, float("nan"))]
    for a in bad_resets:
        assert L.qpsk_deframer_reset_coded(h, a[0], sw, *a[1:]) == QPSK_ERR_ARG, a
    assert L.qpsk_deframer_reset_coded(h, 4, None, 16, 8, 4, 8, 0, 64.0) == QPSK_ERR_ARG
    assert push(P(z), 100, P(g), P(cnt), *none7) == QPSK_ERR_STATE                                   # a refused reset resets nothing
    # a context holds one deframer, in one mode
    assert L.qpsk_deframer_reset(h, 4, sw, 16, 8, 4, 8) == 0
    assert push(P(z), 100, P(g), P(cnt), *none7) == QPSK_ERR_STATE and plain() == 0
    assert L.qpsk_deframer_reset_coded(h, 4, sw, 16, 8, 4, 8, 0, 64.0) == 0
    assert plain() == QPSK_ERR_STATE and push(P(z), 100, P(g), P(cnt), *none7) == 0
    m.sync()
    # argument errors launch nothing
    cnt.fill_(-3)
    assert push(None, 100, P(g), P(cnt), *none7) == QPSK_ERR_ARG                                      # no input
    assert push(P(z), 100, P(g), None, *none7) == QPSK_ERR_ARG                                        # no count
    assert push(P(z), 0, P(g), P(cnt), *none7) == QPSK_ERR_ARG
    assert push(P(z), (1 << 21) + 1, P(g), P(cnt), *none7) == QPSK_ERR_ARG
    assert push(C.c_void_p(z.data_ptr() + 4), 99, P(g), P(cnt), *none7) == QPSK_ERR_ARG               # not 8-byte aligned
    assert push(P(z), 100, P(g), C.c_void_p(z.data_ptr() + 8), *none7) == QPSK_ERR_ARG                # count overlaps the input
    assert push(P(z), 100, P(g), P(cnt), None, None, None, None, None, C.c_void_p(z.data_ptr() + 64)) == QPSK_ERR_ARG
    m.sync()
    assert (cnt.cpu().numpy() == -3).all()
    # a re-reset with other sizes replaces everything
    rng = np.random.default_rng(7)
    sync = rng.integers(0, 4, 70, dtype=np.uint8)
    zz = planted_costas(rng, 9, 2500, sync, 30, max_err=1)
    rows = rows_of(zz, [1000, 1500])
    gg = np.full((2, 9), 60.0, np.float32)
    m.deframer_reset_coded(9, sync, 30, 68, max_packets=16)
    assert push_all(m, rows, gg) == want_all(rows, gg, sync, 68, 30)
    m.close()


def test_outputs_that_touch_the_input_are_accepted_and_the_least_shared_bytes_are_refused():
    """2 streams, 100 symbols of costas_frame[] a push (1600 bytes), 4 slots of 2 + 2 bytes; all seven outputs are given"""
    import torch
    from test_deframe_gpu import boundary_pushes
    rng = np.random.default_rng(22)
    S, M, nsym, nbytes, total = 2, 4, 100, 2, 1500
    sync = rng.integers(0, 4, 16, dtype=np.uint8)
    z = planted_costas(rng, S, total + nsym, sync, nbytes, max_err=1, noise=0.1, gap=150, burst=8)      # a push more than is made: what the last refused calls are handed
    gain = np.full(S, 60.0, np.float32)
    d_gain = torch.from_numpy(gain).cuda()
    sizes = dict(d_count=S * 4, d_bytes=S * M * (nbytes + 2), d_pos=S * M * 8, d_rot=S * M * 4, d_score=S * M * 4, d_crc_ok=S * M, d_info=S * M * 16)
    steps = dict(d_count=4, d_bytes=1, d_pos=8, d_rot=4, d_score=4, d_crc_ok=1, d_info=4)
    shapes = dict(pos=(np.int64, (S, M)), rot=(np.int32, (S, M)), score=(np.int32, (S, M)), bytes=(np.uint8, (S, M, nbytes + 2)),
                  crc_ok=(np.uint8, (S, M)), info=(np.int32, (S, M, 4)))
    m = modem()
    m.deframer_reset_coded(S, sync, nbytes, 15, max_packets=M)
    got = [[] for _ in range(S)]

    def parse(host, where, k):
        cut = lambda name, dtype, shape: host[where[name]:where[name] + sizes[name]].view(dtype).reshape(shape)      # noqa: E731
        cnt = cut("d_count", np.int32, (S,))
        h = {key: cut("d_" + key, *shapes[key]) for key in KEYS}
        assert (cnt <= M).all()
        for s in range(S):
            got[s] += [rec(k, {key: h[key][s, j] for key in KEYS}) for j in range(cnt[s])]

    call = lambda d_in, n, p: m.L.qpsk_deframer_push_coded(m.h, d_in, n, C.c_void_p(d_gain.data_ptr()), p["d_count"], p["d_bytes"], p["d_pos"],  # noqa: E731
                                                           p["d_rot"], p["d_score"], p["d_crc_ok"], p["d_info"])
    put = lambda k: np.ascontiguousarray(z[:, k * nsym:(k + 1) * nsym]).view(np.uint8).reshape(-1)      # noqa: E731
    pushes = boundary_pushes(m, call, S, M, nsym, S * nsym * 8, put, sizes, steps, parse, "qpsk_deframer_push_coded")
    assert pushes == 15 == total // nsym
    rows = rows_of(z[:, :total], [nsym] * pushes)
    assert got == want_all(rows, np.tile(gain, (pushes, 1)), sync, 15, nbytes) and all(got)
    m.sync()
    m.close()


def nan_case(where):
    """one stream pair: stream 0 carries a packet, stream 1 none (abandoned); a NaN is put `where` -> the synchronisation's verdict"""
    import qpsk_amd
    rng = np.random.default_rng(8)
    nsync, nbytes = 24, 6
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    pkt, _ = make_coded_packet(rng, sync, nbytes)
    z = np.stack([dibits_to_costas(np.concatenate([np.zeros(50, np.uint8), pkt, np.zeros(30, np.uint8)]), amp=1.0, noise=0.1, rng=rng),
                  dibits_to_costas(np.zeros(50 + len(pkt) + 30, np.uint8), amp=1.0)])
    gain = np.full(2, 60.0, np.float32)
    if where == "body":
        z[0, 50 + nsync + 17, 1] = np.nan
    elif where == "outside":
        z[1, 33, 0] = np.nan                                            # no body there: data_rule reads a NaN as dibit bit 0
        z[0, 10, 1] = np.inf
    elif where == "gain":
        gain[1] = np.nan
    elif where == "outside, no gain":
        z[1, 33, 0] = np.nan
        gain = None
    m = modem()
    m.deframer_reset_coded(2, sync, nbytes, nsync, max_packets=2)
    o = m.deframe_coded(z, gain)
    try:
        m.sync()
        verdict = 0
    except qpsk_amd.QpskError as e:
        verdict = int(str(e).split("error")[1].split(":")[0])
    cnt = o["count"].cpu().numpy().tolist()
    m.close()
    return verdict, cnt


def test_nan_in_a_body_or_a_gain_is_reported_and_a_nan_outside_every_body_is_not():
    assert nan_case("none") == (0, [1, 0])
    assert nan_case("body")[0] == QPSK_ERR_RANGE
    assert nan_case("gain")[0] == QPSK_ERR_RANGE
    assert nan_case("outside") == (0, [1, 0])
    assert nan_case("outside, no gain")[0] == QPSK_ERR_RANGE             # the summed row holds it


# ------------------------------------------------------------------- 6. isolation
def test_coded_deframer_and_receive_streams_do_not_disturb_each_other():
    fs, rs, L, S = 9600.0, 2400.0, 512, 40
    rng = np.random.default_rng(14)
    pcm = (5000 * rng.standard_normal((4, S, L))).astype(np.int16)
    a, b = modem(fs=fs, rs=rs, frame_size=L), modem(fs=fs, rs=rs, frame_size=L)
    frames = (0.3 * rng.standard_normal((32, L, 2))).astype(np.float32)
    a.streams_reset(S, 1500.0)
    b.streams_reset(S, 1500.0)
    sync = rng.integers(0, 4, 20, dtype=np.uint8)
    b.deframer_reset_coded(S, sync, 8, 12)
    rows = []
    for k in range(4):
        oa, ob = a.streams_rx_pcm(pcm[k]), b.streams_rx_pcm(pcm[k])
        got = b.deframe_coded(ob)
        ra, rb = a.rx_batch(frames, want_costas=True), b.rx_batch(frames, want_costas=True)      # the histogram mode's guess, the batch paths
        for key in ("sym", "costas", "phase", "freq", "index"):
            assert np.array_equal(oa[key].cpu().numpy().view(np.uint8), ob[key].cpu().numpy().view(np.uint8)), (k, key)
            assert np.array_equal(ra[key].cpu().numpy().view(np.uint8), rb[key].cpu().numpy().view(np.uint8)), (k, key)
        rows.append(ob["costas"].cpu().numpy())
        want = want_all(rows, None, sync, 12, 8)
        assert got["count"].cpu().numpy().tolist() == [sum(1 for r in want[s] if r[0] == k) for s in range(S)]
    a.sync()
    b.sync()
    a.close()
    b.close()


# ------------------------------------------------------------------- 7. the link on the device
def test_link_on_the_stream_path(oracle):
    """the CPU test's PCM through qpsk_streams_rx_pcm block by block, each block's d_costas pushed with no gain: the packet records equal
    deframe_coded_ref on the oracle's costas_frame[] bit for bit, and every payload comes back"""
    from oracle.pyoracle import TIMING_FIXED
    k = LINK
    Cy = int(k["fs"] / k["rs"])
    lk = coded_link_pcm(oracle)
    rows = link_rows(oracle, lk)
    m = modem(fs=k["fs"], rs=k["rs"], frame_size=k["L"], timing_mode=TIMING_FIXED, fixed_index=126 % Cy)
    m.streams_reset(3, 1500.0)
    m.deframer_reset_coded(3, lk["sync_c"], k["nbytes"], k["min_score"], max_packets=4)
    got = [[] for _ in range(3)]
    for b in range(lk["nblocks"]):
        blk = np.tile(lk["pcm"][b * k["L"]:(b + 1) * k["L"]], (3, 1))
        o = m.streams_rx_pcm(np.ascontiguousarray(blk))
        assert np.array_equal(o["costas"].cpu().numpy()[1].view(np.uint32), rows[b].view(np.uint32)), b
        r = m.deframe_coded(o)
        h = {key: r[key].cpu().numpy() for key in KEYS + ("count",)}
        for s in range(3):
            got[s] += [rec(b, {key: h[key][s, j] for key in KEYS}) for j in range(h["count"][s])]
    m.sync()
    want = want_all([r[None] for r in rows], None, lk["sync_c"], k["min_score"], k["nbytes"])[0]
    assert got[0] == got[1] == got[2] == want
    delay = k["L"] // Cy + 126 // Cy
    good = {r[1]: r[4][:k["nbytes"]] for r in want if r[5]}
    assert all(good.get(tc + delay) == pl.tobytes() for tc, _, pl in lk["sent"])
    m.close()


# ------------------------------------------------------------------- 8. against the batch calls
def test_packets_inside_one_push_equal_soft_then_viterbi():
    rng = np.random.default_rng(9)
    nsync, nbytes, S, total = 64, 64, 20, 1200
    Nc = coded_steps(nbytes)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    z = planted_costas(rng, S, total, sync, nbytes, gap=250)
    g = rng.uniform(30.0, 90.0, S).astype(np.float32)
    m = modem()
    m.deframer_reset_coded(S, sync, nbytes, nsync - 3, max_packets=2)
    o = m.deframe_coded(z, g)
    cnt = o["count"].cpu().numpy()
    assert (cnt >= 1).all()
    lag, rot = o["pos"].cpu().numpy()[:, 0].astype(np.int32), o["rot"].cpu().numpy()[:, 0].astype(np.int32)
    soft = m.soft(z, gain=g, lag=lag, rot=rot, first=nsync, nout=Nc)
    v = m.viterbi(soft, flip=keystream(Nc))
    m.sync()
    assert np.array_equal(o["bytes"].cpu().numpy()[:, 0], v["bits"].cpu().numpy()[:, :nbytes + 2])
    assert np.array_equal(o["info"].cpu().numpy()[:, 0], v["info"].cpu().numpy())
    assert o["crc_ok"].cpu().numpy()[:, 0].sum() >= S // 2
    # and the uncoded deframer on the same context afterwards is the uncoded deframer
    m.deframer_reset(S, sync, nbytes, nsync - 3, max_packets=4)
    u = m.deframe(costas=z)
    want = [len(deframe_ref(data_rule(z[s]), sync, nsync - 3, nbytes)) for s in range(S)]
    assert u["count"].cpu().numpy().tolist() == want
    m.close()
