"""qpsk_deframer_reset / qpsk_deframer_push on the GPU against deframe_ref (test_deframe_cpu.py), which restates include/qpsk_hip.h."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_cpu import (COSTAS_CASE_CUTS, EDGE_CUTTINGS, HUNT_SET_NAMES, costas_case, cuttings_of_test_1, deframe_ref, edge_case, hunt_sets,
                              link_pcm, overflow_set, planted_streams, want_of, written)
from test_rx_data_cpu import data_rule

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5


def modem(**kw):
    import qpsk_amd
    return qpsk_amd.Modem(**kw)


def push_all(m, rows, costas=False):
    """push a list of (S, nsym[, 2]) rows; -> per stream the list of reported packets (push index, pos, rot, score, bytes, crc_ok)"""
    S = rows[0].shape[0]
    got = [[] for _ in range(S)]
    for k, r in enumerate(rows):
        o = m.deframe(costas=r) if costas else m.deframe(data=r)
        cnt = o["count"].cpu().numpy()
        pos, rot, sc = o["pos"].cpu().numpy(), o["rot"].cpu().numpy(), o["score"].cpu().numpy()
        by, ok = o["bytes"].cpu().numpy(), o["crc_ok"].cpu().numpy()
        assert (cnt <= pos.shape[1]).all(), "more packets in one push than the test's max_packets"
        for s in range(S):
            for j in range(cnt[s]):
                got[s].append((k, int(pos[s, j]), int(rot[s, j]), int(sc[s, j]), by[s, j].tobytes(), bool(ok[s, j])))
    return got


# ------------------------------------------------------------------- 1. planted words, bit for bit, any cuts
@pytest.mark.parametrize("nsync,nbytes", [(32, 16), (64, 64), (100, 5)])
def test_planted_words_bit_for_bit_for_every_cut(nsync, nbytes):
    rng = np.random.default_rng(nsync)
    S, total = 300, 6000
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    min_score = nsync - 3
    D = planted_streams(rng, S, total, sync, nbytes)
    m = modem()
    lists = []
    for cuts in cuttings_of_test_1(rng, total):
        m.deframer_reset(S, sync, nbytes, min_score, max_packets=64)
        rows, at = [], 0
        for c in cuts:
            rows.append(np.ascontiguousarray(D[:, at:at + c]))
            at += c
        got = push_all(m, rows)
        for s in range(S):
            want = want_of(D[s], cuts, sync, min_score, nbytes)
            assert got[s] == want, (cuts[:4], s, got[s][:2], want[:2])
        lists.append([[g[1:] for g in got[s]] for s in range(S)])
    assert all(x == lists[0] for x in lists)
    assert sum(len(x) for x in lists[0]) > 3 * S
    m.close()


# ------------------------------------------------------------------- 1b. one and two plane words, on both inputs
@pytest.mark.parametrize("nsync,nbytes", [(7, 1), (65, 2), (128, 5)])
def test_words_of_7_65_and_128_dibits_on_data_rows_and_on_costas_input(nsync, nbytes):
    sync, D, wants = edge_case(nsync, nbytes)
    z = np.stack([np.where(D & 1, -1.0, 1.0), np.where(D & 2, -0.5, 0.5)], axis=-1).astype(np.float32)
    assert np.array_equal(data_rule(z), D)
    m = modem()
    for cuts, want in zip(EDGE_CUTTINGS, wants):
        at = np.cumsum([0] + cuts)
        for costas, x in ((False, D), (True, z)):
            m.deframer_reset(6, sync, nbytes, nsync - 1, max_packets=64)
            got = push_all(m, [np.ascontiguousarray(x[:, a:b]) for a, b in zip(at[:-1], at[1:])], costas=costas)
            assert got == want, (nsync, cuts[:2], costas)
    m.close()


# ------------------------------------------------------------------- 2. costas input = its data rule
def test_costas_input_equals_its_data_rule():
    # complex values with -0.0, +0.0 and NaN components sprinkled in (test_deframe_cpu.costas_case: the port's CPU test runs `data` too)
    sync, nbytes, min_score, z, data = costas_case()
    S, nsync = z.shape[0], len(sync)
    assert min_score == nsync - 2
    m = modem()
    cuts = COSTAS_CASE_CUTS
    rows_z, rows_d, at = [], [], 0
    for c in cuts:
        rows_z.append(np.ascontiguousarray(z[:, at:at + c]))
        rows_d.append(np.ascontiguousarray(data[:, at:at + c]))
        at += c
    m.deframer_reset(S, sync, nbytes, nsync - 2, max_packets=64)
    gz = push_all(m, rows_z, costas=True)
    m.deframer_reset(S, sync, nbytes, nsync - 2, max_packets=64)
    gd = push_all(m, rows_d)
    assert gz == gd and sum(len(x) for x in gz) > S
    for s in range(S):
        assert gd[s] == want_of(data[s], cuts, sync, nsync - 2, nbytes), s
    m.close()


# ------------------------------------------------------------------- 3. overflow
def test_overflow_counts_everything_and_writes_only_max_packets():
    import torch
    t3 = overflow_set()
    sync, nsync, nbytes, M, D = t3["sync"], t3["nsync"], t3["nbytes"], t3["max_packets"], t3["D"]
    S = D.shape[0]
    m = modem()
    m.deframer_reset(S, sync, nbytes, nsync, max_packets=M)
    d = torch.from_numpy(D).cuda()
    cnt = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    by = torch.full((S, M + 1, nbytes + 2), 0xA5, dtype=torch.uint8, device="cuda")   # one canary row per stream beyond max_packets
    pos = torch.full((S, M + 1), -7, dtype=torch.int64, device="cuda")
    rot = torch.full((S, M + 1), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((S, M + 1), -7, dtype=torch.int32, device="cuda")
    ok = torch.full((S, M + 1), 0xA5, dtype=torch.uint8, device="cuda")
    # the outputs are [S][M] packed: the last S rows of each buffer are the canary
    flat = [t.reshape(-1) for t in (by, pos, rot, sc, ok)]
    rc = m.L.qpsk_deframer_push(m.h, None, C.c_void_p(d.data_ptr()), D.shape[1], C.c_void_p(cnt.data_ptr()),
                                *[C.c_void_p(t.data_ptr()) for t in flat])
    assert rc == 0, m.L.qpsk_last_error()
    m.sync()
    want = deframe_ref(D[0], sync, nsync, nbytes)
    assert len(want) == 10
    assert (cnt.cpu().numpy() == 10).all()
    n_b, n_p = S * M * (nbytes + 2), S * M
    fb, fp, fr, fs_, fo = [t.cpu().numpy() for t in flat]
    for s in range(S):
        for j in range(M):
            assert fb[(s * M + j) * (nbytes + 2):(s * M + j + 1) * (nbytes + 2)].tobytes() == want[j]["bytes"].tobytes()
            assert (fp[s * M + j], fr[s * M + j], fs_[s * M + j], fo[s * M + j]) == (want[j]["pos"], want[j]["rot"], want[j]["score"], 1)
    assert (fb[n_b:] == 0xA5).all() and (fp[n_p:] == -7).all() and (fr[n_p:] == -7).all() and (fs_[n_p:] == -7).all()
    assert (fo[n_p:] == 0xA5).all()
    m.close()


# ------------------------------------------------------------------- 3b. the hunt where candidates are dense and rotations tie
def push_guarded(m, x, cuts, M, nbytes, costas=False):
    """the C call push by push over x (S, total[, 2]), every output poisoned before each push and one canary row per stream behind the
    [S][M] block (test 3's layout) -> per stream (count per push, the records written: push, pos, rot, score, bytes, crc_ok).  The rows of
    a stream beyond min(count, M) and the canary rows must come back as they went in"""
    import torch
    S = x.shape[0]
    xs = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cnt = torch.empty((S,), dtype=torch.int32, device="cuda")
    by = torch.empty((S * (M + 1), nbytes + 2), dtype=torch.uint8, device="cuda")
    pos = torch.empty((S * (M + 1),), dtype=torch.int64, device="cuda")
    rot, sc = torch.empty_like(pos, dtype=torch.int32), torch.empty_like(pos, dtype=torch.int32)
    ok = torch.empty_like(pos, dtype=torch.uint8)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    counts, got, at = [[] for _ in range(S)], [[] for _ in range(S)], 0
    for k, c in enumerate(cuts):
        row = xs[:, at:at + c].contiguous()
        at += c
        cnt.fill_(-1)
        for t, v in ((by, 0xA5), (pos, -7), (rot, -7), (sc, -7), (ok, 0xA5)):
            t.fill_(v)
        rc = m.L.qpsk_deframer_push(m.h, P(row) if costas else None, None if costas else P(row), c, P(cnt), P(by), P(pos), P(rot), P(sc), P(ok))
        assert rc == 0, m.L.qpsk_last_error()
        m.sync()
        hc, hb, hp, hr, hs, ho = [t.cpu().numpy() for t in (cnt, by, pos, rot, sc, ok)]
        if not hc.any():
            assert (hb == 0xA5).all() and (hp == -7).all() and (hr == -7).all() and (hs == -7).all() and (ho == 0xA5).all(), k
            for s in range(S):
                counts[s].append(0)
            continue
        for s in range(S):
            w = min(int(hc[s]), M)
            counts[s].append(int(hc[s]))
            got[s] += [(k, int(hp[s * M + j]), int(hr[s * M + j]), int(hs[s * M + j]), hb[s * M + j].tobytes(), bool(ho[s * M + j])) for j in range(w)]
            assert all(int(ho[s * M + j]) in (0, 1) for j in range(w))
            idle = slice(s * M + w, (s + 1) * M)
            assert (hb[idle] == 0xA5).all() and (hp[idle] == -7).all() and (hr[idle] == -7).all() and (hs[idle] == -7).all() and (ho[idle] == 0xA5).all(), (k, s)
        assert (hb[S * M:] == 0xA5).all() and (hp[S * M:] == -7).all() and (hr[S * M:] == -7).all() and (hs[S * M:] == -7).all() and (ho[S * M:] == 0xA5).all(), k
    return [(counts[s], got[s]) for s in range(S)]


@pytest.mark.parametrize("what", HUNT_SET_NAMES)
def test_the_hunt_on_dense_candidates_tied_rotations_and_the_per_push_bound(what):
    """test_deframe_cpu.hunt_sets: low thresholds on noise (every step holds candidates, hx lands inside a step, the [1500] push of the
    short words overflows max_packets), constant words against alternating and period-4 ring values (two and four rotations tie: the
    smallest wins), packets back to back with a push of k periods + 1 dibits at max_packets = k + 1, k and 64.  test_hunt_port_cpu.py has
    run the same bytes through the scalar port of the hunt; here the kernel, on data rows and on costas input: count, pos, rot, score,
    bytes, crc_ok and the push, bit for bit"""
    s = next(t for t in hunt_sets() if t["what"] == what)
    s["check"](s)
    D = s["D"]
    z = np.stack([np.where(D & 1, -1.0, 1.0), np.where(D & 2, -0.5, 0.5)], axis=-1).astype(np.float32)
    assert np.array_equal(data_rule(z), D)
    m = modem()
    for cuts in s["cuttings"]:
        want = [written(want_of(D[k], cuts, s["sync"], s["min_score"], s["nbytes"]), len(cuts), s["max_packets"]) for k in range(D.shape[0])]
        for costas, x in ((False, D), (True, z)):
            m.deframer_reset(D.shape[0], s["sync"], s["nbytes"], s["min_score"], max_packets=s["max_packets"])
            got = push_guarded(m, x, cuts, s["max_packets"], s["nbytes"], costas=costas)
            for k in range(D.shape[0]):
                assert got[k][0] == want[k][0], (what, cuts[:2], costas, k, "count")
                assert got[k][1] == want[k][1], (what, cuts[:2], costas, k)
    m.close()


# ------------------------------------------------------------------- 4. errors and state
def test_errors_and_rereset():
    import torch
    m = modem()
    L, h = m.L, m.h
    d = torch.zeros((4, 100), dtype=torch.uint8, device="cuda")
    z = torch.zeros((4, 100, 2), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.qpsk_deframer_push(h, None, P(d), 100, P(cnt), None, None, None, None, None) == QPSK_ERR_STATE
    sw = (C.c_uint8 * 130)(*([1, 2, 3, 0] * 32 + [1, 2]))
    bad_resets = [(0, 16, 8, 4, 8), (4, 0, 1, 4, 8), (4, 129, 8, 4, 8), (4, 16, 0, 4, 8), (4, 16, 17, 4, 8), (4, 16, 8, 0, 8),
                  (4, 16, 8, 1025, 8), (4, 16, 8, 4, 0), (4, 16, 8, 4, 65)]
    for S, n, ms, nb, M in bad_resets:
        assert L.qpsk_deframer_reset(h, S, sw, n, ms, nb, M) == QPSK_ERR_ARG, (S, n, ms, nb, M)
    assert L.qpsk_deframer_reset(h, 4, None, 16, 8, 4, 8) == QPSK_ERR_ARG
    notdibit = (C.c_uint8 * 4)(1, 2, 4, 0)
    assert L.qpsk_deframer_reset(h, 4, notdibit, 4, 2, 4, 8) == QPSK_ERR_ARG
    assert L.qpsk_deframer_push(h, None, P(d), 100, P(cnt), None, None, None, None, None) == QPSK_ERR_STATE
    assert L.qpsk_deframer_reset(h, 4, sw, 16, 8, 4, 8) == 0
    ok = lambda *a: L.qpsk_deframer_push(h, *a)  # noqa: E731
    assert ok(None, P(d), 100, P(cnt), None, None, None, None, None) == 0
    assert ok(None, None, 100, P(cnt), None, None, None, None, None) == QPSK_ERR_ARG                 # no input
    assert ok(P(z), P(d), 100, P(cnt), None, None, None, None, None) == QPSK_ERR_ARG                 # both
    assert ok(None, P(d), 100, None, None, None, None, None, None) == QPSK_ERR_ARG                   # no count
    assert ok(None, P(d), 0, P(cnt), None, None, None, None, None) == QPSK_ERR_ARG
    assert ok(None, P(d), (1 << 21) + 1, P(cnt), None, None, None, None, None) == QPSK_ERR_ARG
    assert ok(None, P(d), 100, C.c_void_p(d.data_ptr() + 8), None, None, None, None, None) == QPSK_ERR_ARG   # count overlaps the input
    big = torch.zeros(4 * 8 * 6 + 64, dtype=torch.uint8, device="cuda")
    assert ok(None, P(big), 16, P(cnt), C.c_void_p(big.data_ptr() + 32), None, None, None, None) == QPSK_ERR_ARG
    assert ok(P(z), None, 100, P(cnt), None, None, None, None, C.c_void_p(z.data_ptr() + 100)) == QPSK_ERR_ARG
    m.sync()
    # a re-reset with other sizes replaces everything
    rng = np.random.default_rng(13)
    sync = rng.integers(0, 4, 70, dtype=np.uint8)
    D = planted_streams(rng, 9, 2500, sync, 30, max_err=1)
    m.deframer_reset(9, sync, 30, 68, max_packets=16)
    got = push_all(m, [np.ascontiguousarray(D[:, :1000]), np.ascontiguousarray(D[:, 1000:])])
    for s in range(9):
        assert got[s] == want_of(D[s], [1000, 1500], sync, 68, 30), s
    m.close()


def boundary_pushes(m, call, S, M, nsym, in_bytes, put_input, sizes, steps, parse, who):
    """what the overlap tests of both pushes share: the input of in_bytes bytes at byte 1024 of one allocation, every output at a home of its
    own; then each output in turn ends where the input begins and begins where it ends (accepted; parse(host, where, push index) compares
    the push), and lies one step of its alignment further in (refused: "<who>: <output> overlaps the input").  -> the pushes made"""
    import torch
    arena = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    home = {name: 256 * ((1024 + in_bytes + 255) // 256 + 1 + i) for i, name in enumerate(sizes)}      # behind the input, apart from each other
    pushes = 0
    for name in [None] + list(sizes):
        for shift, accepted in ((0, True),) if name is None else ((-sizes[name], True), (in_bytes, True), (-sizes[name] + steps[name], False), (in_bytes - steps[name], False)):
            where = dict(home) if name is None else {**home, name: 1024 + shift}
            host = np.zeros(8192, np.uint8)
            host[1024:1024 + in_bytes] = put_input(pushes)
            arena.copy_(torch.from_numpy(host))
            rc = call(C.c_void_p(arena.data_ptr() + 1024), nsym, {k: C.c_void_p(arena.data_ptr() + v) for k, v in where.items()})
            torch.cuda.synchronize()
            if not accepted:
                assert rc == QPSK_ERR_ARG and ("%s: %s overlaps the input" % (who, name)).encode() in m.L.qpsk_last_error(), (name, shift, rc, m.L.qpsk_last_error())
                continue
            assert rc == 0, (name, shift, m.L.qpsk_last_error())
            parse(arena.cpu().numpy(), where, pushes)
            pushes += 1
    return pushes


def test_outputs_that_touch_the_input_are_accepted_and_the_least_shared_bytes_are_refused():
    """2 streams, 100 dibits a push on the data input (200 bytes), 4 slots of 4 + 2 bytes; every optional output is given"""
    rng = np.random.default_rng(21)
    S, M, nsym, nbytes, total = 2, 4, 100, 4, 1300
    sync = rng.integers(0, 4, 16, dtype=np.uint8)
    D = planted_streams(rng, S, total + nsym, sync, nbytes, max_err=1)      # a push more than is made: what the last refused calls are handed
    sizes = dict(d_count=S * 4, d_bytes=S * M * (nbytes + 2), d_pos=S * M * 8, d_rot=S * M * 4, d_score=S * M * 4, d_crc_ok=S * M)
    steps = dict(d_count=4, d_bytes=1, d_pos=8, d_rot=4, d_score=4, d_crc_ok=1)
    m = modem()
    m.deframer_reset(S, sync, nbytes, 15, max_packets=M)
    got = [[] for _ in range(S)]

    def parse(host, where, k):
        cut = lambda name, dtype, shape: host[where[name]:where[name] + sizes[name]].view(dtype).reshape(shape)      # noqa: E731
        cnt, by, pos = cut("d_count", np.int32, (S,)), cut("d_bytes", np.uint8, (S, M, nbytes + 2)), cut("d_pos", np.int64, (S, M))
        rot, sc, ok = cut("d_rot", np.int32, (S, M)), cut("d_score", np.int32, (S, M)), cut("d_crc_ok", np.uint8, (S, M))
        assert (cnt <= M).all()
        for s in range(S):
            for j in range(cnt[s]):
                got[s].append((k, int(pos[s, j]), int(rot[s, j]), int(sc[s, j]), by[s, j].tobytes(), bool(ok[s, j])))

    call = lambda d_in, n, p: m.L.qpsk_deframer_push(m.h, None, d_in, n, p["d_count"], p["d_bytes"], p["d_pos"], p["d_rot"], p["d_score"], p["d_crc_ok"])  # noqa: E731
    pushes = boundary_pushes(m, call, S, M, nsym, S * nsym, lambda k: D[:, k * nsym:(k + 1) * nsym].reshape(-1), sizes, steps, parse, "qpsk_deframer_push")
    assert pushes == 13 == total // nsym
    for s in range(S):
        assert got[s] == want_of(D[s, :total], [nsym] * pushes, sync, 15, nbytes) and got[s], s
    m.sync()
    m.close()


def test_deframer_and_receive_streams_do_not_disturb_each_other():
    fs, rs, L, S = 9600.0, 2400.0, 512, 40
    rng = np.random.default_rng(14)
    pcm = (5000 * rng.standard_normal((4, S, L))).astype(np.int16)
    a, b = modem(fs=fs, rs=rs, frame_size=L), modem(fs=fs, rs=rs, frame_size=L)
    a.streams_reset(S, 1500.0)
    b.streams_reset(S, 1500.0)
    sync = rng.integers(0, 4, 20, dtype=np.uint8)
    b.deframer_reset(S, sync, 8, 12)
    rows = []
    for k in range(4):
        oa = a.streams_rx_pcm(pcm[k])
        ob = b.streams_rx_pcm(pcm[k])
        got = b.deframe(ob)
        for key in ("sym", "costas", "phase", "freq", "index"):
            assert np.array_equal(oa[key].cpu().numpy().view(np.uint8), ob[key].cpu().numpy().view(np.uint8)), (k, key)
        rows.append(data_rule(ob["costas"].cpu().numpy()))
        # a stream reset leaves the deframer alone; the deframer's output matches the reference on what it was given
        assert got["count"].cpu().numpy().tolist() == [sum(1 for p in deframe_ref(np.concatenate([r[s] for r in rows]), sync, 12, 8)
                                                            if p["end"] > sum(len(r[s]) for r in rows[:-1])) for s in range(S)]
    a.close()
    b.close()


# ------------------------------------------------------------------- 5. the link on the stream path
@pytest.mark.parametrize("fs,L,S", [(9600.0, 512, 96), (19200.0, 2048, 64)])
def test_link_on_the_stream_path(oracle, fs, L, S):
    """qpsk_tx_symbols-shaped PCM (the oracle's transmitter, bit for bit the library's) with packets at random gaps, at tx_hz =
    mixer_hz + 50 with noise; qpsk_streams_rx_pcm block by block, each block's d_costas pushed.  (a) on sampled streams the packet
    records equal deframe_ref on the oracle's costas_frame[]; (b) every packet whose word starts after W warm-up blocks comes back
    with its CRC at t + nsym + 126 // CYCLES, and no other packet passes its CRC.  W is the number of blocks the oracle's loop needs
    before its data rule matches the transmitted dibits on every checked stream (measured below, not assumed)."""
    from oracle.pyoracle import TIMING_FIXED
    rs, nbytes, nsync, nblocks = 2400.0, 64, 48, 24
    C_ = int(fs / rs)
    nsym = L // C_
    delay = nsym + 126 // C_
    rng = np.random.default_rng(int(fs) + L)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    pcms, sents = [], []
    for s in range(S):
        p, sent = link_pcm(oracle, rng, fs, rs, L, nblocks, sync, nbytes, noise=20.0)
        pcms.append(p)
        sents.append(sent)
    pcm = np.stack(pcms)                                              # (S, nblocks * L)
    m = modem(fs=fs, rs=rs, frame_size=L, timing_mode=TIMING_FIXED, fixed_index=126 % C_)
    m.streams_reset(S, 1500.0)
    m.deframer_reset(S, sync, nbytes, nsync - 6, max_packets=16)
    got = [[] for _ in range(S)]
    for b in range(nblocks):
        o = m.streams_rx_pcm(np.ascontiguousarray(pcm[:, b * L:(b + 1) * L]))
        r = m.deframe(o)
        cnt, pos = r["count"].cpu().numpy(), r["pos"].cpu().numpy()
        by, ok, rot = r["bytes"].cpu().numpy(), r["crc_ok"].cpu().numpy(), r["rot"].cpu().numpy()
        for s in range(S):
            assert cnt[s] <= 16
            got[s] += [(int(pos[s, j]), int(rot[s, j]), by[s, j].tobytes(), bool(ok[s, j])) for j in range(cnt[s])]
    check = sorted(set([0, 1, S // 2, S - 1]))
    warm = 0
    for s in check:
        om = oracle.modem(fs, rs, L, timing_mode=TIMING_FIXED, fixed_index=126 % C_)
        om.set_mixer_hz(1500.0)
        rows = []
        for b in range(nblocks):
            om.rx_pcm(pcm[s, b * L:(b + 1) * L])
            rows.append(data_rule(om.costas_frame))
        D = np.concatenate(rows)
        want = [(p["pos"], p["rot"], p["bytes"].tobytes(), p["crc_ok"]) for p in deframe_ref(D, sync, nsync - 6, nbytes)]
        assert got[s] == want, s                                     # (a)
        # W: one block behind the last expected packet the oracle's own decisions do not bring back
        for t, payload in sents[s]:
            if t + delay + nsync + 4 * (nbytes + 2) > nblocks * nsym:
                continue                                              # not complete within the run
            ok_here = any(p[0] == t + delay and p[3] for p in want)
            if not ok_here:
                warm = max(warm, (t + delay) // nsym + 1)
    assert warm <= 4, warm                                            # the loop locks within a few blocks at a 50 Hz offset
    total = 0
    for s in range(S):
        ok = sorted((p, pl[:nbytes]) for p, _, pl, good in got[s] if good)
        want = sorted((t + delay, payload.tobytes()) for t, payload in sents[s]
                      if (t + delay) // nsym >= warm and t + delay + nsync + 4 * (nbytes + 2) <= nblocks * nsym)
        assert [x for x in ok if x[0] // nsym >= warm] == want, s    # (b)
        assert all(x[0] // nsym >= warm or x in [(t + delay, pl.tobytes()) for t, pl in sents[s]] for x in ok), s
        total += len(want)
    assert total >= 3 * S
