"""qpsk_channel_reset / qpsk_channel_push and Modem.channel_reset / Modem.channel on the GPU, bit for bit (as uint32) against the numpy
restatement of test_channel_cpu.py (CHANNELISER of include/qpsk_hip.h): every instantiation of channel_push_kernel and its generic path
at push lengths around the tile of every geometry, samples over sixty decades with signed zeros, the carried history, selections and
pitches, the refusals, the independence of the receive streams, and the link of the CPU test on the device with library calls only.  There
is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_channel_cpu import LINK, bits, channel_ref, link_result, link_shape, link_wideband, twiddles

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
POISON = 12345.0
KERNEL = "channel_push_kernel"


def tile(M):
    """the output times a workgroup takes (channel_tile in kernels.h): 256 threads below M = 1024, 1024 threads from there on"""
    return 16384 // M if M >= 1024 else 8192 // M if M >= 64 else 128


# the tile of every M the tests use; the two geometries are M < 1024 (256 threads) and M >= 1024 (1024 threads)
TILES = {2: 128, 4: 128, 16: 128, 32: 128, 64: 128, 128: 64, 256: 32, 512: 16, 1024: 16, 2048: 8, 4096: 4}


@pytest.fixture(scope="module")
def m():
    import qpsk_amd
    md = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"], timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=link_shape()["index"])
    yield md
    md.close()


def proto(M, P, seed=0):
    """taps with no symmetry and no zero among them: a wrong branch or a wrong order shows"""
    rng = np.random.default_rng(1000 * M + P + seed)
    return (rng.standard_normal(M * P) / np.sqrt(M * P)).astype(np.float32)


def samples(M, T, seed):
    return np.random.default_rng(seed).standard_normal((T * M, 2)).astype(np.float32)


def run_pushes(m, M, P, h, pushes, chan=None):
    """reset, then the pushes one after the other -> for each the device's rows (nsel, T, 2) and the restatement's with the carried history"""
    m.channel_reset(M, P, h, chan)
    sel = np.arange(M) if chan is None else np.asarray(chan)
    hist, out = None, []
    for x in pushes:
        got = m.channel(x).cpu().numpy()
        assert m.last_kernel() == KERNEL
        want, hist = channel_ref(x, hist, h, M, P, twiddles(M))
        out.append((got, want[sel]))
    m.sync()
    return out


# ------------------------------------------------------------------- 1. shapes: every instantiation, lengths around every tile
# (M, P, kernel, the pushes' lengths).  The instantiations are P = 8 and P = 16 at 256 threads and P = 8 at 1024 threads; every other pair
# takes the generic path of its geometry (P = 16 from M = 1024 on included)
SHAPES = [
    (2, 1, "<0, 256>", (1, 127, 128, 129, 300)),
    (4, 2, "<0, 256>", (1, 127, 128, 129)),
    (64, 8, "<8, 256>", (1, 127, 128, 129, 3 * 128 + 5)),
    (64, 16, "<16, 256>", (1, 129, 2 * 128 + 44)),
    (128, 5, "<0, 256>", (63, 64, 65, 200)),
    (256, 32, "<0, 256>", (31, 32, 33, 100)),
    (512, 8, "<8, 256>", (1, 15, 16, 17, 50)),
    (1024, 8, "<8, 1024>", (1, 15, 16, 17, 70)),
    (1024, 5, "<0, 1024>", (16, 17)),
    (2048, 16, "<0, 1024>", (7, 8, 9, 30)),
    (4096, 8, "<8, 1024>", (1, 3, 4, 5, 23)),
    (4096, 32, "<0, 1024>", (4, 9)),
]


def test_the_shapes_cover_every_kernel_and_the_lengths_around_the_tile_of_both_geometries():
    assert {s[2] for s in SHAPES} == {"<0, 256>", "<8, 256>", "<16, 256>", "<0, 1024>", "<8, 1024>"}
    for big in (False, True):
        seen = set()
        for M, P, kernel, lengths in SHAPES:
            if (M >= 1024) == big:
                tb = tile(M)
                seen |= {{1: "1", tb - 1: "tile - 1", tb: "tile", tb + 1: "tile + 1"}.get(T, "tiles + rest" if T > 2 * tb and T % tb else "") for T in lengths}
        assert {"1", "tile - 1", "tile", "tile + 1", "tiles + rest"} <= seen, (big, seen)


@pytest.mark.parametrize("M,P,kernel,lengths", SHAPES, ids=["M%d-P%d" % s[:2] for s in SHAPES])
def test_pushes_of_one_less_than_a_tile_a_tile_one_more_and_several_equal_channel_ref(m, M, P, kernel, lengths):
    tb = tile(M)
    assert TILES[M] == tb
    h = proto(M, P)
    pushes = [samples(M, T, 7 * M + T) for T in lengths]
    for T, (got, want) in zip(lengths, run_pushes(m, M, P, h, pushes)):
        assert got.shape == (M, T, 2)
        assert np.array_equal(bits(got), bits(want)), (kernel, T)


# ------------------------------------------------------------------- 2. inputs
@pytest.mark.parametrize("M,P", [(64, 8), (1024, 5), (2, 1)])
def test_sixty_decades_and_signed_zeros_come_out_as_the_restatement_says(m, M, P):
    """magnitudes from 1e-30 to 1e30 in both signs (no sum reaches the overflow: the taps are below 1), runs of +0.0 and -0.0 -- a -0.0
    at the output where the operations give one, which the restatement does at least once here"""
    rng = np.random.default_rng(M + 31 * P)
    T = 2 * tile(M) + 3 if M > 2 else 40
    mag = 10.0 ** rng.uniform(-30.0, 30.0, (T * M, 2))
    x = (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
    x[rng.random(len(x)) < 0.1] = 0.0
    x[rng.random(len(x)) < 0.1] = -0.0
    x[:(P + 2) * M] = -0.0                                        # whole blocks of -0.0: outputs that are sums of zeros alone
    h = np.abs(proto(M, P))
    (got, want), = run_pushes(m, M, P, h, [x])
    assert np.isfinite(want).all() and (bits(want) == 0x80000000).any() and (bits(want) == 0).any()
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------- 3. carry
@pytest.mark.parametrize("M,P", [(64, 8), (32, 5), (1024, 8)])
def test_history_is_carried_shifted_by_short_pushes_and_cleared_by_a_reset(m, M, P):
    h = proto(M, P)
    lengths = [1, 1, P - 2, P - 1, P, 40]
    x = samples(M, sum(lengths), 99 + M)
    cuts = np.cumsum([0] + lengths) * M
    parts = run_pushes(m, M, P, h, [x[cuts[i]:cuts[i + 1]] for i in range(len(lengths))])
    (whole, want), = run_pushes(m, M, P, h, [x])                   # the reset in front of it clears the history
    assert np.array_equal(bits(whole), bits(want))
    assert np.array_equal(bits(np.concatenate([g for g, _ in parts], axis=1)), bits(whole))
    for g, w in parts:
        assert np.array_equal(bits(g), bits(w))
    # a reset to another (M, P), and back
    M2, P2 = (16, 3) if M != 16 else (8, 3)
    (g2, w2), = run_pushes(m, M2, P2, proto(M2, P2), [samples(M2, 9, 5)])
    assert np.array_equal(bits(g2), bits(w2))
    (g3, w3), = run_pushes(m, M, P, h, [x[:3 * M]])
    assert np.array_equal(bits(g3), bits(want[:, :3]))


# ------------------------------------------------------------------- 4. selection and pitch
@pytest.mark.parametrize("M,P", [(64, 8), (2048, 2)])
def test_selections_in_any_order_with_repeats_and_rows_at_a_pitch_leave_the_gaps_alone(m, M, P):
    import torch
    rng = np.random.default_rng(M)
    h, T = proto(M, P), tile(M) + 3
    x = samples(M, T, 3)
    full, _ = channel_ref(x, None, h, M, P, twiddles(M))
    for chan in (rng.permutation(M), np.array([5, 1, 5, M - 1, 0, 5]), np.array([M - 2])):
        (got, want), = run_pushes(m, M, P, h, [x], chan=chan)
        assert got.shape == (len(chan), T, 2) and np.array_equal(bits(want), bits(full[chan]))
        assert np.array_equal(bits(got), bits(want))
    chan = np.array([3, M - 1, 0])
    m.channel_reset(M, P, h, chan)
    pitch = T + 5
    buf = torch.full((len(chan), pitch, 2), POISON, dtype=torch.float32, device=m.dev)
    xd = torch.from_numpy(x).to(m.dev)
    m._check(m.L.qpsk_channel_push(m.h, C.c_void_p(xd.data_ptr()), T, C.c_void_p(buf.data_ptr()), pitch))
    m.sync()
    got = buf.cpu().numpy()
    assert np.array_equal(bits(got[:, :T]), bits(full[chan])) and np.all(got[:, T:] == POISON)
    m.channel_reset(M, P, h, chan)
    view = m.channel(x, pitch=pitch)
    assert view.shape == (len(chan), T, 2) and view.stride(0) == 2 * pitch and np.array_equal(bits(view.cpu().numpy()), bits(full[chan]))


# ------------------------------------------------------------------- 5. refusals
def test_every_refusal_launches_nothing_and_leaves_the_channeliser_and_the_last_kernel(m):
    import qpsk_amd
    import torch
    fresh = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"])
    M, P, T = 16, 4, 6
    h = proto(M, P)
    x = torch.from_numpy(samples(M, 3 * T, 1)).to(fresh.dev)
    out = torch.full((M, 2 * T, 2), POISON, dtype=torch.float32, device=fresh.dev)
    px, po = x.data_ptr(), out.data_ptr()
    hp = h.ctypes.data_as(C.c_void_p)
    ptr = lambda v: C.c_void_p(v) if v else None      # noqa: E731
    push = lambda xx, TT, oo, pitch: fresh.L.qpsk_channel_push(fresh.h, ptr(xx), TT, ptr(oo), pitch)      # noqa: E731
    fresh.rrc_fir(np.zeros((1, LINK["L"], 2), np.float32))
    before = fresh.last_kernel()
    assert before != KERNEL
    # a push before any reset
    assert push(px, T, po, 0) == QPSK_ERR_STATE and b"qpsk_channel_push" in fresh.L.qpsk_last_error()
    # resets
    reset = lambda MM, PP, taps, chan, nsel: fresh.L.qpsk_channel_reset(fresh.h, MM, PP, taps, chan, nsel)      # noqa: E731
    big = np.zeros(8192 * 2, np.float32).ctypes.data_as(C.c_void_p)
    for MM in (1, 3, 8192, 0, -16):
        assert reset(MM, 2, big, None, 0) == QPSK_ERR_ARG, MM
    for PP in (0, 33, -1):
        assert reset(M, PP, big, None, 0) == QPSK_ERR_ARG, PP
    assert reset(M, P, None, None, 0) == QPSK_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        hb = h.copy()
        hb[M * P - 1] = bad
        assert reset(M, P, hb.ctypes.data_as(C.c_void_p), None, 0) == QPSK_ERR_ARG, bad
    for chan in ([0, M], [-1, 2], [3, 1 << 30]):
        ch = np.array(chan, np.int32)
        assert reset(M, P, hp, ch.ctypes.data_as(C.c_void_p), len(ch)) == QPSK_ERR_ARG, chan
    ch = np.array([1, 2], np.int32)
    assert reset(M, P, hp, ch.ctypes.data_as(C.c_void_p), 0) == QPSK_ERR_ARG
    assert reset(M, P, hp, ch.ctypes.data_as(C.c_void_p), -2) == QPSK_ERR_ARG
    assert fresh.L.qpsk_channel_reset(None, M, P, hp, None, 0) == QPSK_ERR_ARG
    # none of them made a channeliser
    assert push(px, T, po, 0) == QPSK_ERR_STATE
    assert fresh.last_kernel() == before
    # pushes on a good one
    fresh.channel_reset(M, P, h)
    assert push(None, T, po, 0) == QPSK_ERR_ARG and push(px, T, None, 0) == QPSK_ERR_ARG
    assert push(px, 0, po, 0) == QPSK_ERR_ARG and push(px, -3, po, 0) == QPSK_ERR_ARG
    assert push(px, T, po, T - 1) == QPSK_ERR_ARG and push(px, T, po, -1) == QPSK_ERR_ARG
    assert push(px, (1 << 30) // M + 1, po, 0) == QPSK_ERR_ARG
    assert fresh.L.qpsk_channel_push(None, ptr(px), T, ptr(po), 0) == QPSK_ERR_ARG
    assert push(px, T, px, 0) == QPSK_ERR_ARG                                      # d_out is d_x
    assert push(px, T, px + 8 * (T * M - 1), 0) == QPSK_ERR_ARG                    # d_out begins in d_x's last sample
    assert push(px + 8 * T, T, px, T) == QPSK_ERR_ARG                              # d_x begins inside d_out's first row
    assert b"overlaps" in fresh.L.qpsk_last_error()
    fresh.sync()
    assert fresh.last_kernel() == before
    assert torch.all(out == POISON).item()
    # the refused resets and pushes left the channeliser and its zero history: the next push is the first
    xs = x.cpu().numpy()
    got = fresh.channel(xs[:T * M]).cpu().numpy()
    want, hist = channel_ref(xs[:T * M], None, h, M, P, twiddles(M))
    assert fresh.last_kernel() == KERNEL and np.array_equal(bits(got), bits(want))
    assert reset(3, P, hp, None, 0) == QPSK_ERR_ARG                                # a refused reset leaves the one the context has
    got = fresh.channel(xs[T * M:2 * T * M]).cpu().numpy()
    want, _ = channel_ref(xs[T * M:2 * T * M], hist, h, M, P, twiddles(M))
    assert np.array_equal(bits(got), bits(want))
    fresh.close()


# ------------------------------------------------------------------- 6. independence
def test_channel_pushes_between_stream_calls_leave_the_streams_as_they_are(m):
    S, L = 3, LINK["L"]
    rng = np.random.default_rng(66)
    blocks = (0.5 * rng.standard_normal((4, S, L, 2))).astype(np.float32)
    keys = ("sym", "freq", "phase", "costas", "index")

    def run(between):
        m.streams_reset(S, 1500.0)
        if between:
            m.channel_reset(16, 4, proto(16, 4))
        out = []
        for b in blocks:
            if between:
                m.channel(samples(16, 37, 8))
            o = m.streams_rx_cplx(b, want_costas=True)
            out.append({k: o[k].cpu().numpy() for k in keys})
        m.sync()
        return out

    plain, mixed = run(False), run(True)
    for a, b in zip(plain, mixed):
        for k in keys:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ------------------------------------------------------------------- 7. the link on the device
def test_three_carriers_of_one_capture_to_packets_with_library_calls_equals_the_cpu_chain(m, oracle):
    """test_channel_cpu's link with library calls only: frame -> tx_symbols (baseband) -> the same numpy interpolation -> channel ->
    streams_rx_cplx -> deframe, a block at a time.  The baseband and every channel row equal the CPU chain's bit for bit; the packets'
    counts, payloads and crc_ok equal the CPU chain's, which the CPU test has pinned to what was sent"""
    k, shape = LINK, link_shape()
    M, P, L = k["M"], k["P"], k["L"]
    r = link_result(oracle)
    chans = sorted(k["carriers"])
    o = m.frame(shape["payloads"], shape["sync"], coded=False, per_row=k["per_row"], lead=k["lead"], gap=k["gap"], row_len=shape["row_len"])
    assert np.array_equal(o["dibits"].cpu().numpy(), r["rows"])
    m.tx_reset(len(chans), 1550.0)
    bb = m.tx_symbols(o["dibits"], want_pcm=True, want_baseband=True)["baseband"].cpu().numpy()
    capture = link_wideband({ch: bb[i] for i, ch in enumerate(chans)})
    assert np.array_equal(bits(capture), bits(r["capture"]))
    m.channel_reset(M, P, r["proto"])
    m.streams_reset(M, 1500.0)
    m.deframer_reset(M, shape["sync"], k["nbytes"], k["min_score"], max_packets=4)
    got = [[] for _ in range(M)]
    nblocks = len(capture) // (L * M)
    for b in range(nblocks):
        y = m.channel(capture[b * L * M:(b + 1) * L * M])
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
