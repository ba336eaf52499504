"""qpsk_synth_reset / qpsk_synth_push and Modem.synth_reset / Modem.synth on the GPU, bit for bit (as uint32) against the numpy restatement
of test_synth_cpu.py (SYNTHESIS BANK of include/qpsk_hip.h): both instantiations of synth_transform_kernel and the three of
synth_filter_kernel at push lengths around the transform's tile of every geometry and around the filter's run, samples over sixty decades
with signed zeros, the carried history, the scratch that grows, selections and pitches, the refusals, the independence of the channeliser
and the receive streams, and the link of the CPU test on the device with library calls only.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_channel_cpu import LINK, bits, channel_ref, link_shape, twiddles
from test_synth_cpu import synth_link_result, synth_ref

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
POISON = 12345.0
KERNEL = "synth_filter_kernel"
RUN = 16                             # the times a lane of synth_filter_kernel takes (SYNTH_RUN in kernels.h)
MAX_SAMPLES = 1 << 27                # T M of one push


def tile(M):
    """the times a workgroup of synth_transform_kernel takes (channel_tile in kernels.h): 256 threads below M = 1024, 1024 from there on"""
    return 16384 // M if M >= 1024 else 8192 // M if M >= 64 else 128


@pytest.fixture(scope="module")
def m():
    import qpsk_amd
    md = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"], timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=link_shape()["index"])
    yield md
    md.close()


def proto(M, P, seed=0):
    """taps with no symmetry and no zero among them: a wrong branch or a wrong order shows"""
    rng = np.random.default_rng(1000 * M + P + seed)
    return (rng.standard_normal(M * P) / np.sqrt(P)).astype(np.float32)


def rows(nsel, T, seed):
    return np.random.default_rng(seed).standard_normal((nsel, T, 2)).astype(np.float32)


def run_pushes(m, M, P, g, pushes, chan=None):
    """reset, then the pushes one after the other -> for each the device's capture (T M, 2) and the restatement's with the carried history"""
    m.synth_reset(M, P, g, chan)
    hist, out = None, []
    for c in pushes:
        got = m.synth(c).cpu().numpy()
        assert m.last_kernel() == KERNEL
        want, hist = synth_ref(c, chan, hist, g, M, P, twiddles(M))
        out.append((got, want))
    m.sync()
    return out


# ------------------------------------------------------------------- 1. shapes: every instantiation, lengths around every tile and the run
# (M, P, the transform's kernel, the filter's kernel, the pushes' lengths).  The filter's instantiations are P = 8 and P = 16, every other P
# takes its generic path; the transform's are the two geometries
SHAPES = [
    (2, 1, "<256>", "<0>", (1, 127, 128, 129, 300)),
    (4, 2, "<256>", "<0>", (1, 15, 16, 17, 3 * 16 + 5)),
    (64, 8, "<256>", "<8>", (1, 15, 16, 17, 127, 128, 129, 3 * 128 + 5)),
    (64, 16, "<256>", "<16>", (1, 17, 129, 2 * 128 + 44)),
    (128, 5, "<256>", "<0>", (63, 64, 65, 200)),
    (256, 32, "<256>", "<0>", (31, 32, 33, 100)),
    (512, 8, "<256>", "<8>", (1, 15, 16, 17, 50)),
    (1024, 8, "<1024>", "<8>", (1, 15, 16, 17, 70)),
    (1024, 16, "<1024>", "<16>", (16, 17, 37)),
    (2048, 5, "<1024>", "<0>", (7, 8, 9, 30)),
    (4096, 8, "<1024>", "<8>", (1, 3, 4, 5, 23)),
    (4096, 32, "<1024>", "<0>", (4, 9)),
]


def test_the_shapes_cover_every_kernel_and_the_lengths_around_the_tile_and_the_run_of_both_geometries():
    assert {s[2:4] for s in SHAPES} == {(t, f) for t in ("<256>", "<1024>") for f in ("<0>", "<8>", "<16>")}
    for M, P, transform, filt, _ in SHAPES:
        assert transform == ("<1024>" if M >= 1024 else "<256>") and filt == ("<%d>" % P if P in (8, 16) else "<0>")
    for big in (False, True):
        tiles, runs = set(), set()
        for M, P, _, _, lengths in SHAPES:
            if (M >= 1024) == big:
                tb = tile(M)
                tiles |= {{1: "1", tb - 1: "tile - 1", tb: "tile", tb + 1: "tile + 1"}.get(T, "tiles + rest" if T > 2 * tb and T % tb else "") for T in lengths}
                runs |= {{1: "1", RUN - 1: "run - 1", RUN: "run", RUN + 1: "run + 1"}.get(T, "runs + rest" if T > 2 * RUN and T % RUN else "") for T in lengths}
        assert {"1", "tile - 1", "tile", "tile + 1", "tiles + rest"} <= tiles, (big, tiles)
        assert {"1", "run - 1", "run", "run + 1", "runs + rest"} <= runs, (big, runs)
    assert max(s[0] for s in SHAPES) == 4096


@pytest.mark.parametrize("M,P,transform,filt,lengths", SHAPES, ids=["M%d-P%d" % s[:2] for s in SHAPES])
def test_pushes_around_the_tile_and_the_run_equal_synth_ref(m, M, P, transform, filt, lengths):
    g = proto(M, P)
    chan = None if M != 128 else np.random.default_rng(M).permutation(M)[:77]
    nsel = M if chan is None else len(chan)
    pushes = [rows(nsel, T, 7 * M + T) for T in lengths]
    for T, (got, want) in zip(lengths, run_pushes(m, M, P, g, pushes, chan)):      # the history is carried through the sequence
        assert got.shape == (T * M, 2)
        assert np.array_equal(bits(got), bits(want)), (transform, filt, T)


# ------------------------------------------------------------------- 2. inputs
@pytest.mark.parametrize("M,P", [(64, 8), (1024, 5), (2, 1)])
def test_sixty_decades_and_signed_zeros_come_out_as_the_restatement_says(m, M, P):
    """magnitudes from 1e-30 to 1e30 in both signs (no sum reaches the overflow: M values below 1e30 and taps below 1), runs of +0.0 and
    -0.0, whole times of -0.0 -- a -0.0 at the output where the operations give one (e - z with z = +0.0)"""
    rng = np.random.default_rng(M + 31 * P)
    T = 2 * tile(M) + 3 if M > 2 else 40
    mag = 10.0 ** rng.uniform(-30.0, 30.0, (M, T, 2))
    c = (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
    c[rng.random((M, T)) < 0.1] = 0.0
    c[rng.random((M, T)) < 0.1] = -0.0
    c[:, :P + 2] = -0.0                                           # whole vectors of -0.0: outputs that are sums of zeros alone
    g = np.minimum(np.abs(proto(M, P)), np.float32(0.9))
    (got, want), = run_pushes(m, M, P, g, [c])
    assert np.isfinite(want).all() and (bits(want) == 0x80000000).any() and (bits(want) == 0).any()
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------- 3. carry
@pytest.mark.parametrize("M,P", [(64, 8), (32, 5), (1024, 8)])
def test_history_is_carried_shifted_by_short_pushes_and_cleared_by_a_reset(m, M, P):
    g = proto(M, P)
    lengths = [1, 1, P - 2, P - 1, P, 40]
    c = rows(M, sum(lengths), 99 + M)
    cuts = np.cumsum([0] + lengths)
    parts = run_pushes(m, M, P, g, [c[:, cuts[i]:cuts[i + 1]] for i in range(len(lengths))])
    (whole, want), = run_pushes(m, M, P, g, [c])                   # the reset in front of it clears the history
    assert np.array_equal(bits(whole), bits(want))
    assert np.array_equal(bits(np.concatenate([got for got, _ in parts])), bits(whole))
    for got, w in parts:
        assert np.array_equal(bits(got), bits(w))
    # a reset to another (M, P), and back
    M2, P2 = 16, 3
    (g2, w2), = run_pushes(m, M2, P2, proto(M2, P2), [rows(M2, 9, 5)])
    assert np.array_equal(bits(g2), bits(w2))
    (g3, w3), = run_pushes(m, M, P, g, [c[:, :3]])
    assert np.array_equal(bits(g3), bits(want[:3 * M])) and np.array_equal(bits(g3), bits(w3))


# ------------------------------------------------------------------- 4. the scratch grows with the largest push
def test_a_small_a_large_and_a_small_push_on_a_new_context_equal_the_restatement():
    import qpsk_amd
    fresh = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"])
    M, P = 64, 8
    g = proto(M, P)
    lengths = (3, 500, 2, 501, 1)
    for T, (got, want) in zip(lengths, run_pushes(fresh, M, P, g, [rows(M, T, T) for T in lengths])):
        assert np.array_equal(bits(got), bits(want)), T
    fresh.close()


# ------------------------------------------------------------------- 5. selection, pitch, and what is written
@pytest.mark.parametrize("M,P", [(64, 8), (2048, 2)])
def test_selections_in_any_order_a_lone_channel_and_rows_at_a_pitch(m, M, P):
    import torch
    rng = np.random.default_rng(M)
    g, T = proto(M, P), tile(M) + 3
    for chan in (rng.permutation(M), rng.permutation(M)[:M // 3], np.array([M - 2]), None):
        nsel = M if chan is None else len(chan)
        c = rows(nsel, T, 3 + nsel)
        (got, want), = run_pushes(m, M, P, g, [c], chan=chan)
        assert np.array_equal(bits(got), bits(want))
        if chan is not None and nsel < M:
            # a channel nobody names contributes exact zeros: the same bits as all M channels with +0.0 rows in the others' places
            every = np.zeros((M, T, 2), np.float32)
            every[chan] = c
            (got_all, want_all), = run_pushes(m, M, P, g, [every])
            assert np.array_equal(bits(want_all), bits(want)) and np.array_equal(bits(got_all), bits(got))
    # rows at a pitch with poison between them; poison where d_x will lie and behind it
    chan = np.array([3, M - 1, 0])
    c = rows(len(chan), T, 17)
    want, _ = synth_ref(c, chan, None, g, M, P, twiddles(M))
    pitch = T + 5
    buf = torch.full((len(chan), pitch, 2), POISON, dtype=torch.float32, device=m.dev)
    buf[:, :T] = torch.from_numpy(c).to(m.dev)
    before = buf.clone()
    x = torch.full((T * M + 64, 2), POISON, dtype=torch.float32, device=m.dev)
    m.synth_reset(M, P, g, chan)
    m._check(m.L.qpsk_synth_push(m.h, C.c_void_p(buf.data_ptr()), pitch, T, C.c_void_p(x.data_ptr())))
    m.sync()
    got = x.cpu().numpy()
    assert np.array_equal(bits(got[:T * M]), bits(want))          # every sample of d_x is written
    assert np.all(got[T * M:] == POISON)
    assert torch.equal(buf, before)
    m.synth_reset(M, P, g, chan)
    assert np.array_equal(bits(m.synth(buf[:, :T], pitch=pitch).cpu().numpy()), bits(want))
    assert torch.equal(buf, before)


# ------------------------------------------------------------------- 6. refusals
def test_every_refusal_launches_nothing_and_leaves_the_bank_and_the_last_kernel():
    import qpsk_amd
    import torch
    fresh = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"])
    M, P, T = 16, 4, 6
    g = proto(M, P)
    cin = torch.from_numpy(rows(M, 3 * T, 1)).to(fresh.dev)              # (M, 3 T, 2): rows 3 T apart
    x = torch.full((2 * T * M, 2), POISON, dtype=torch.float32, device=fresh.dev)
    pc, px = cin.data_ptr(), x.data_ptr()
    gp = g.ctypes.data_as(C.c_void_p)
    ptr = lambda v: C.c_void_p(v) if v else None      # noqa: E731
    push = lambda cc, pitch, TT, xx: fresh.L.qpsk_synth_push(fresh.h, ptr(cc), pitch, TT, ptr(xx))      # noqa: E731
    fresh.rrc_fir(np.zeros((1, LINK["L"], 2), np.float32))
    before = fresh.last_kernel()
    assert before != KERNEL
    # a push before any reset
    assert push(pc, 3 * T, T, px) == QPSK_ERR_STATE and b"qpsk_synth_push" in fresh.L.qpsk_last_error()
    # resets
    reset = lambda MM, PP, taps, chan, nsel: fresh.L.qpsk_synth_reset(fresh.h, MM, PP, taps, chan, nsel)      # noqa: E731
    big = np.zeros(8192 * 2, np.float32).ctypes.data_as(C.c_void_p)
    for MM in (1, 3, 8192, 0, -16):
        assert reset(MM, 2, big, None, 0) == QPSK_ERR_ARG, MM
    for PP in (0, 33, -1):
        assert reset(M, PP, big, None, 0) == QPSK_ERR_ARG, PP
    assert reset(M, P, None, None, 0) == QPSK_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        gb = g.copy()
        gb[M * P - 1] = bad
        assert reset(M, P, gb.ctypes.data_as(C.c_void_p), None, 0) == QPSK_ERR_ARG, bad
    for chan in ([0, M], [-1, 2], [3, 1 << 30], [5, 1, 5], [2, 2], list(range(M)) + [0]):      # outside, named twice, nsel > M
        ch = np.array(chan, np.int32)
        assert reset(M, P, gp, ch.ctypes.data_as(C.c_void_p), len(ch)) == QPSK_ERR_ARG, chan
    ch = np.array([1, 2], np.int32)
    assert reset(M, P, gp, ch.ctypes.data_as(C.c_void_p), 0) == QPSK_ERR_ARG
    assert reset(M, P, gp, ch.ctypes.data_as(C.c_void_p), -2) == QPSK_ERR_ARG
    assert reset(M, P, gp, ch.ctypes.data_as(C.c_void_p), M + 1) == QPSK_ERR_ARG
    assert fresh.L.qpsk_synth_reset(None, M, P, gp, None, 0) == QPSK_ERR_ARG
    # none of them made a bank
    assert push(pc, 3 * T, T, px) == QPSK_ERR_STATE
    assert fresh.last_kernel() == before
    # pushes on a good one
    fresh.synth_reset(M, P, g)
    assert push(None, 3 * T, T, px) == QPSK_ERR_ARG and push(pc, 3 * T, T, None) == QPSK_ERR_ARG
    assert push(pc, 3 * T, 0, px) == QPSK_ERR_ARG and push(pc, 3 * T, -3, px) == QPSK_ERR_ARG
    assert push(pc, T - 1, T, px) == QPSK_ERR_ARG and push(pc, -1, T, px) == QPSK_ERR_ARG      # a pitch below T
    assert push(pc, MAX_SAMPLES // M + 1, MAX_SAMPLES // M + 1, px) == QPSK_ERR_ARG            # T M beyond the bound
    assert b"samples in one push" in fresh.L.qpsk_last_error()
    assert fresh.L.qpsk_synth_push(None, ptr(pc), 3 * T, T, ptr(px)) == QPSK_ERR_ARG
    assert push(pc, 3 * T, T, pc) == QPSK_ERR_ARG                                              # d_x is d_in
    assert push(pc, 3 * T, T, pc + 8 * ((M - 1) * 3 * T + T - 1)) == QPSK_ERR_ARG              # d_x begins in the last row's last sample
    assert push(px + 8 * T, T, T, px) == QPSK_ERR_ARG                                          # the rows begin inside d_x
    assert b"overlaps" in fresh.L.qpsk_last_error()
    fresh.sync()
    assert fresh.last_kernel() == before
    assert torch.all(x == POISON).item()
    # the refused resets and pushes left the bank and its zero history: the next push is the first
    cs = cin.cpu().numpy()
    got = fresh.synth(cs[:, :T]).cpu().numpy()
    want, hist = synth_ref(cs[:, :T], None, None, g, M, P, twiddles(M))
    assert fresh.last_kernel() == KERNEL and np.array_equal(bits(got), bits(want))
    assert reset(3, P, gp, None, 0) == QPSK_ERR_ARG                                            # a refused reset leaves the one the context has
    dup = np.array([4, 4], np.int32)
    assert reset(M, P, gp, dup.ctypes.data_as(C.c_void_p), 2) == QPSK_ERR_ARG
    got = fresh.synth(cs[:, T:2 * T]).cpu().numpy()
    want, _ = synth_ref(cs[:, T:2 * T], None, hist, g, M, P, twiddles(M))
    assert np.array_equal(bits(got), bits(want))
    fresh.close()


# ------------------------------------------------------------------- 7. independence
def test_synth_pushes_and_channel_pushes_and_stream_calls_leave_each_other_as_they_are(m):
    S, L = 3, LINK["L"]
    rng = np.random.default_rng(66)
    blocks = (0.5 * rng.standard_normal((4, S, L, 2))).astype(np.float32)
    wide = [rng.standard_normal((37 * 16, 2)).astype(np.float32) for _ in blocks]
    narrow = [rows(5, 11 + i, 70 + i) for i in range(len(blocks))]
    chan = np.array([7, 0, 2, 31, 12])
    keys = ("sym", "freq", "phase", "costas", "index")
    as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8)      # noqa: E731

    def run(with_synth, with_others):
        if with_others:
            m.streams_reset(S, 1500.0)
            m.channel_reset(16, 4, proto(16, 4))
        if with_synth:
            m.synth_reset(32, 6, proto(32, 6), chan)
        out = []
        for b, x, c in zip(blocks, wide, narrow):
            o = {}
            if with_others:
                o["channel"] = m.channel(x).cpu().numpy()
            if with_synth:
                o["synth"] = m.synth(c).cpu().numpy()
            if with_others:
                rx = m.streams_rx_cplx(b, want_costas=True)
                o.update({k: rx[k].cpu().numpy() for k in keys})
            if with_synth:
                o["synth2"] = m.synth(c[:, :3]).cpu().numpy()
            out.append(o)
        m.sync()
        return out

    others, synth, mixed = run(False, True), run(True, False), run(True, True)
    for a, b, ab in zip(others, synth, mixed):
        for k in a:
            assert np.array_equal(as_bytes(a[k]), as_bytes(ab[k])), k
        for k in b:
            assert np.array_equal(as_bytes(b[k]), as_bytes(ab[k])), k
    hist = None
    for c, o in zip(narrow, mixed):
        want, hist = synth_ref(c, chan, hist, proto(32, 6), 32, 6, twiddles(32))
        assert np.array_equal(bits(o["synth"]), bits(want))
        want, hist = synth_ref(c[:, :3], chan, hist, proto(32, 6), 32, 6, twiddles(32))
        assert np.array_equal(bits(o["synth2"]), bits(want))


# ------------------------------------------------------------------- 8. the link on the device
def test_three_rows_to_packets_through_both_banks_with_library_calls_only_equal_the_cpu_chain(m, oracle):
    """test_synth_cpu's link with library calls only: frame -> tx_symbols (baseband) -> synth -> channel -> streams_rx_cplx -> deframe, a
    block at a time, both banks live in one context.  The baseband, the capture and every channel row equal the CPU chain's bit for bit;
    the packets' counts, payloads and crc_ok equal the CPU chain's, which the CPU test has pinned to what was sent"""
    k, shape = LINK, link_shape()
    M, P, L = k["M"], k["P"], k["L"]
    r = synth_link_result(oracle)
    chans = sorted(k["carriers"])
    o = m.frame(shape["payloads"], shape["sync"], coded=False, per_row=k["per_row"], lead=k["lead"], gap=k["gap"], row_len=shape["row_len"])
    assert np.array_equal(o["dibits"].cpu().numpy(), r["rows"])
    m.tx_reset(len(chans), 1550.0)
    bb = m.tx_symbols(o["dibits"], want_pcm=True, want_baseband=True)["baseband"]
    assert np.array_equal(bits(bb.cpu().numpy()), bits(r["basebands"]))
    n = bb.shape[1]
    m.synth_reset(M, P, r["g"], chans)
    m.channel_reset(M, P, r["proto"])
    m.streams_reset(M, 1500.0)
    m.deframer_reset(M, shape["sync"], k["nbytes"], k["min_score"], max_packets=4)
    got = [[] for _ in range(M)]
    nblocks = n // L
    assert nblocks * L == n and n * M == len(r["capture"])
    for b in range(nblocks):
        x = m.synth(bb[:, b * L:(b + 1) * L], pitch=n)
        assert np.array_equal(bits(x.cpu().numpy()), bits(r["capture"][b * L * M:(b + 1) * L * M]))
        y = m.channel(x)
        assert np.array_equal(bits(y.cpu().numpy()), bits(r["y"][:, b * L:(b + 1) * L]))
        rx = m.streams_rx_cplx(y.contiguous(), want_costas=True)
        d = m.deframe(costas=rx)
        h = {key: d[key].cpu().numpy() for key in ("count", "bytes", "crc_ok")}
        for s in range(M):
            got[s] += [(h["bytes"][s, j].tobytes(), bool(h["crc_ok"][s, j])) for j in range(h["count"][s])]
    m.sync()
    for s in range(M):
        assert got[s] == [(g[3], g[4]) for g in r["records"][s]], s
        assert len(got[s]) == (k["per_row"] if s in chans else 0)
