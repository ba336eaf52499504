"""qpsk_resample_reset / qpsk_resample_need / qpsk_resample_push and Modem.resample_reset / resample_need / resample on the GPU, bit for bit
(as uint32) against the numpy restatement of test_resample_cpu.py (RESAMPLER of include/qpsk_hip.h): every instantiation of
resample_push_kernel on the staged and on the direct path at push lengths around the tile, samples over sixty decades with signed zeros,
the carried history and position, rows and pitches, the refusals, the independence of the other stateful stages, and the link of the CPU
test on the device with library calls only.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_channel_cpu import channel_ref, twiddles
from test_resample_cpu import LINK, bits, link_result, link_shape, need_ref, resample_ref, taps, total_in, up_blocks

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
POISON = 12345.0
KERNEL = "resample_push_kernel"
TILE = 256                            # RESAMPLE_TILE in kernels.h: the outputs a workgroup takes
WIN_MAX = 4096                        # RESAMPLE_WIN_MAX: the largest window of samples a workgroup stages in LDS


def path(L, D, P):
    """resample_staged in kernels.h: a tile's window of (TILE - 1) D / L + 1 + P samples is staged where it fits"""
    return "staged" if (TILE - 1) * D // L + 1 + P <= WIN_MAX else "direct"


def kernel(L, D, P):
    return "<%d, %s>" % (P if P in (8, 16) else 0, path(L, D, P))


@pytest.fixture(scope="module")
def m():
    import qpsk_amd
    md = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"], timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=link_shape()["index"])
    yield md
    md.close()


def samples(S, n, seed):
    return np.random.default_rng(seed).standard_normal((S, n, 2)).astype(np.float32)


def run_pushes(m, S, L, D, P, h, nouts, x, reset=True, state=None, at=0):
    """reset, then pushes of nouts outputs, each fed the samples it needs from x (S, n, 2) in turn -> (for each push the device's rows
    (S, nout, 2) and the restatement's, the state, the samples consumed).  The library's need is checked against the restatement's"""
    if reset:
        m.resample_reset(S, L, D, P, h)
    out = []
    for nout in nouts:
        K = m.resample_need(nout)
        assert K == need_ref(0 if state is None else state[1], L, D, nout)
        assert at + K <= x.shape[1]
        got = m.resample(x[:, at:at + K], nout).cpu().numpy()
        assert m.last_kernel() == KERNEL
        want, state = resample_ref(x[:, at:at + K], state, h, L, D, P, nout)
        out.append((got, want))
        at += K
    m.sync()
    return out, state, at


# ------------------------------------------------------------------- 1. shapes: every instantiation on both paths, lengths around the tile
# (L, D, P, kernel, the pushes' lengths).  The instantiations are P = 8 and P = 16, every other P takes the generic path; a ratio is staged
# or direct by its window
AROUND = (1, 255, 256, 257, 3 * 256 + 5)
SHAPES = [
    (5, 4, 8, "<8, staged>", AROUND),
    (4, 5, 16, "<16, staged>", AROUND),
    (1, 1, 1, "<0, staged>", AROUND),
    (2, 1, 3, "<0, staged>", (1, 256, 257, 515)),
    (1, 3, 4, "<0, staged>", (255, 256, 257, 900)),
    (160, 147, 2, "<0, staged>", AROUND),
    (160, 147, 16, "<16, staged>", (300, 1, 256)),
    (512, 511, 32, "<0, staged>", (1, 257, 600)),           # the taps fill their 64 KiB of LDS
    (4, 6, 5, "<0, staged>", (256, 1, 300)),                # gcd > 1
    (7, 3, 5, "<0, staged>", (1, 1, 1, 255, 2, 600)),       # L > D: pushes that consume nothing
    (1, 16, 8, "<8, staged>", (257, 255)),                  # the largest staged window there is at L = 1, P = 8: 4089 samples
    (3, 512, 2, "<0, direct>", AROUND),
    (1, 4096, 2, "<0, direct>", (1, 255, 256, 257, 520)),
    (1, 64, 8, "<8, direct>", AROUND),
    (1, 32, 16, "<16, direct>", (255, 257, 3 * 256 + 1)),
    (1, 17, 8, "<8, direct>", (256, 300)),                  # the smallest direct window: 4344 samples
]


def test_the_shapes_cover_every_kernel_on_both_paths_and_the_lengths_around_the_tile():
    assert {s[3] for s in SHAPES} == {"<%d, %s>" % (p, w) for p in (0, 8, 16) for w in ("staged", "direct")}
    for L, D, P, k, _ in SHAPES:
        assert kernel(L, D, P) == k, (L, D, P)
    assert {(5, 4), (4, 5), (1, 1), (2, 1), (1, 3), (160, 147), (512, 511), (3, 512), (1, 4096), (4, 6)} <= {s[:2] for s in SHAPES}
    assert (512, 511, 32) in {s[:3] for s in SHAPES} and {(3, 512, 2), (1, 4096, 2)} <= {s[:3] for s in SHAPES}
    for way in ("staged", "direct"):
        seen = set()
        for L, D, P, k, lengths in SHAPES:
            if way in k:
                seen |= {{1: "1", TILE - 1: "tile - 1", TILE: "tile", TILE + 1: "tile + 1"}.get(n, "tiles + rest" if n > 2 * TILE and n % TILE else "")
                         for n in lengths}
        assert {"1", "tile - 1", "tile", "tile + 1", "tiles + rest"} <= seen, (way, seen)
    # the two paths meet between D = 16 and D = 17 at L = 1, P = 8
    assert path(1, 16, 8) == "staged" and path(1, 17, 8) == "direct"


@pytest.mark.parametrize("L,D,P,k,lengths", SHAPES, ids=["%d/%d-P%d" % s[:3] for s in SHAPES])
def test_pushes_of_one_less_than_a_tile_a_tile_one_more_and_several_equal_resample_ref(m, L, D, P, k, lengths):
    S = 2
    h = taps(L, P)
    x = samples(S, total_in(L, D, sum(lengths)) + 1, 7 * L + D)
    out, state, _ = run_pushes(m, S, L, D, P, h, lengths, x)
    for nout, (got, want) in zip(lengths, out):
        assert got.shape == (S, nout, 2)
        assert np.array_equal(bits(got), bits(want)), (k, nout)
    assert state[1] == 0 or D - L <= state[1] < D


# ------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("L,D,P", [(5, 4, 8), (4, 5, 16), (3, 512, 2), (7, 3, 5)])
def test_sixty_decades_and_signed_zeros_come_out_as_the_restatement_says(m, L, D, P):
    """magnitudes from 1e-30 to 1e30 in both signs (no sum reaches the overflow: the taps are below 1), runs of +0.0 and -0.0 -- a -0.0
    at the output where the operations give one, which the restatement does at least once here"""
    rng = np.random.default_rng(L + 31 * P)
    nout, S = 2 * TILE + 3, 2
    n = total_in(L, D, nout)
    mag = 10.0 ** rng.uniform(-30.0, 30.0, (S, n, 2))
    x = (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
    x[rng.random((S, n)) < 0.1] = 0.0
    x[rng.random((S, n)) < 0.1] = -0.0
    x[:, :min(n // 2, 3 * P + 40 * D // L)] = -0.0                      # a run of -0.0: outputs that are sums of zeros alone
    h = np.abs(taps(L, P))
    h = (h / max(1.0, 1.01 * float(h.max()))).astype(np.float32)
    assert h.max() < 1.0 and np.all(h > 0.0) and not np.array_equal(h, h[::-1])
    ((got, want),), _, _ = run_pushes(m, S, L, D, P, h, [nout], x)
    assert np.isfinite(want).all() and (bits(want) == 0x80000000).any() and (bits(want) == 0).any()
    assert np.array_equal(bits(got), bits(want))


def test_nan_and_inf_propagate_as_ieee_arithmetic_says(m):
    L, D, P, S, nout = 5, 4, 8, 1, 300
    x = samples(S, total_in(L, D, nout), 77)
    x[0, 50, 0], x[0, 120, 1], x[0, 200, 0] = np.inf, np.nan, -np.inf
    ((got, want),), _, _ = run_pushes(m, S, L, D, P, taps(L, P), [nout], x)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    assert np.array_equal(bits(got)[keep], bits(want)[keep])


# ------------------------------------------------------------------- 3. carry
def nouts_for(L, D, wanted):
    """from a reset, for every K of `wanted` in turn the smallest nout whose push consumes exactly K inputs at the position then reached;
    where no push does (K = 0 needs r < 0), single outputs go in between until one does -> (the nouts, the K of every push)"""
    r, nouts, Ks = 0, [], []
    for K in wanted:
        for _ in range(2 * L):
            fit = [n for n in range(1, 4 * (K + 2) * L // D + 8) if need_ref(r, L, D, n) == K]
            nout = fit[0] if fit else 1
            got = need_ref(r, L, D, nout)
            nouts.append(nout)
            Ks.append(got)
            r += nout * D - got * L
            if fit:
                break
        else:
            raise AssertionError((L, D, K))
    return nouts, Ks


@pytest.mark.parametrize("L,D,P", [(7, 3, 5), (5, 4, 8), (2, 1, 16), (160, 147, 2)])
def test_history_and_position_are_carried_through_pushes_that_consume_none_few_and_many(m, L, D, P):
    S = 3
    h = taps(L, P)
    nouts, Ks = nouts_for(L, D, [1, 0, P - 1, 0, P, P + 1, 1, 0, 40, 0])
    assert {0, 1, P - 1, P, P + 1, 40} <= set(Ks)
    x = samples(S, sum(Ks) + 2, 99 + L)
    parts, state, used = run_pushes(m, S, L, D, P, h, nouts, x)
    assert used == sum(Ks)
    total = sum(nouts)
    assert total_in(L, D, total) == used
    (whole,), state_whole, _ = run_pushes(m, S, L, D, P, h, [total], x)              # the reset in front of it clears history and position
    assert np.array_equal(bits(whole[0]), bits(whole[1]))
    assert np.array_equal(bits(np.concatenate([g for g, _ in parts], axis=1)), bits(whole[0]))
    for g, w in parts:
        assert np.array_equal(bits(g), bits(w))
    assert state[1] == state_whole[1] and np.array_equal(bits(state[0]), bits(state_whole[0]))
    # a reset to another shape, and back
    L2, D2, P2 = 3, 7, 2
    x2 = samples(2, total_in(L2, D2, 9), 5)
    ((g2, w2),), _, _ = run_pushes(m, 2, L2, D2, P2, taps(L2, P2), [9], x2)
    assert np.array_equal(bits(g2), bits(w2))
    ((g3, _),), _, _ = run_pushes(m, S, L, D, P, h, nouts[:1], x)
    assert np.array_equal(bits(g3), bits(whole[0][:, :nouts[0]]))


# ------------------------------------------------------------------- 4. rows
@pytest.mark.parametrize("S", [1, 3, 70])
def test_rows_at_pitches_leave_the_gaps_alone(m, S):
    import torch
    L, D, P = 4, 5, 16
    h = taps(L, P)
    nouts = (TILE + 3, 40)
    x = samples(S, total_in(L, D, sum(nouts)), 3 + S)
    (a, b), _, _ = run_pushes(m, S, L, D, P, h, nouts, x)                            # tight rows through Modem.resample
    assert np.array_equal(bits(a[0]), bits(a[1])) and np.array_equal(bits(b[0]), bits(b[1]))
    # the C call at pitches, poison between the rows
    m.resample_reset(S, L, D, P, h)
    at = 0
    for nout, (_, want) in zip(nouts, (a, b)):
        K = m.resample_need(nout)
        ip, op = K + 7, nout + 5
        src = torch.full((S, ip, 2), POISON, dtype=torch.float32, device=m.dev)
        src[:, :K] = torch.from_numpy(x[:, at:at + K]).to(m.dev)
        dst = torch.full((S, op, 2), POISON, dtype=torch.float32, device=m.dev)
        m._check(m.L.qpsk_resample_push(m.h, C.c_void_p(src.data_ptr()), ip, K, nout, C.c_void_p(dst.data_ptr()), op))
        m.sync()
        got = dst.cpu().numpy()
        assert np.array_equal(bits(got[:, :nout]), bits(want)) and np.all(got[:, nout:] == POISON)
        assert np.all(src.cpu().numpy()[:, K:] == POISON)
        at += K
    # Modem.resample with both pitches: a view in, a view out
    m.resample_reset(S, L, D, P, h)
    K = m.resample_need(nouts[0])
    src = torch.full((S, K + 7, 2), POISON, dtype=torch.float32, device=m.dev)
    src[:, :K] = torch.from_numpy(x[:, :K]).to(m.dev)
    view = m.resample(src[:, :K], nouts[0], pitch=K + 7, out_pitch=nouts[0] + 5)
    assert view.shape == (S, nouts[0], 2) and (S == 1 or view.stride(0) == 2 * (nouts[0] + 5))
    assert np.array_equal(bits(view.cpu().numpy()), bits(a[1]))
    with pytest.raises(ValueError):
        m.resample(x[:, :K + 1], nouts[1])                                           # not the need


def test_a_channeliser_push_written_at_a_pitch_is_read_where_it_lies(m):
    import qpsk_amd
    M, PC, L, D, P, nout = 8, 4, 5, 4, 8, 300
    T = total_in(L, D, nout)
    hc = qpsk_amd.channel_prototype(M, PC)
    x = np.random.default_rng(12).standard_normal((T * M, 2)).astype(np.float32)
    rows, _ = channel_ref(x, None, hc, M, PC, twiddles(M))
    h = taps(L, P)
    want, _ = resample_ref(rows, None, h, L, D, P, nout)
    m.channel_reset(M, PC, hc)
    m.resample_reset(M, L, D, P, h)
    assert m.resample_need(nout) == T
    y = m.channel(x, pitch=T + 9)
    assert y.shape == (M, T, 2) and y.stride(0) == 2 * (T + 9)
    got = m.resample(y, nout, pitch=T + 9).cpu().numpy()
    m.sync()
    assert np.array_equal(bits(y.cpu().numpy()), bits(rows))
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------- 5. refusals
def test_every_refusal_launches_nothing_and_leaves_the_resampler_and_the_last_kernel(m):
    import qpsk_amd
    import torch
    fresh = qpsk_amd.Modem(fs=LINK["fs"], rs=LINK["rs"], frame_size=LINK["L"])
    S, L, D, P, nout = 3, 5, 4, 4, 10
    K = total_in(L, D, nout)
    h = taps(L, P)
    xs = samples(S, 3 * K, 1)
    x = torch.from_numpy(xs).to(fresh.dev)
    out = torch.full((S, 4 * nout, 2), POISON, dtype=torch.float32, device=fresh.dev)
    px, po = x.data_ptr(), out.data_ptr()
    hp = h.ctypes.data_as(C.c_void_p)
    ptr = lambda v: C.c_void_p(v) if v else None      # noqa: E731
    push = lambda xx, ip, nin, nn, oo, op: fresh.L.qpsk_resample_push(fresh.h, ptr(xx), ip, nin, nn, ptr(oo), op)      # noqa: E731
    err = lambda: fresh.L.qpsk_last_error()      # noqa: E731
    fresh.rrc_fir(np.zeros((1, LINK["L"], 2), np.float32))
    before = fresh.last_kernel()
    assert before != KERNEL
    # before any reset
    assert push(px, 3 * K, K, nout, po, 4 * nout) == QPSK_ERR_STATE and b"qpsk_resample_push" in err()
    assert fresh.L.qpsk_resample_need(fresh.h, nout) == QPSK_ERR_STATE and b"qpsk_resample_need" in err()
    # resets
    reset = lambda SS, LL, DD, PP, tp: fresh.L.qpsk_resample_reset(fresh.h, SS, LL, DD, PP, tp)      # noqa: E731
    big = np.zeros(512 * 32, np.float32).ctypes.data_as(C.c_void_p)
    for SS in (0, -1, 65537):
        assert reset(SS, L, D, P, big) == QPSK_ERR_ARG, SS
    for LL in (0, -1, 513):
        assert reset(S, LL, D, 1, big) == QPSK_ERR_ARG, LL
    for DD in (0, -1, 4097):
        assert reset(S, L, DD, P, big) == QPSK_ERR_ARG, DD
    for PP in (0, -1, 33):
        assert reset(S, 1, D, PP, big) == QPSK_ERR_ARG, PP
    assert reset(S, L, D, P, None) == QPSK_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        hb = h.copy()
        hb[L * P - 1] = bad
        assert reset(S, L, D, P, hb.ctypes.data_as(C.c_void_p)) == QPSK_ERR_ARG, bad
    assert fresh.L.qpsk_resample_reset(None, S, L, D, P, hp) == QPSK_ERR_ARG
    # none of them made a resampler
    assert push(px, 3 * K, K, nout, po, 4 * nout) == QPSK_ERR_STATE
    assert fresh.last_kernel() == before
    # pushes on a good one
    fresh.resample_reset(S, L, D, P, h)
    assert fresh.resample_need(nout) == K
    good = (px, 3 * K, K, nout, po, 4 * nout)
    assert push(None, 3 * K, K, nout, po, 4 * nout) == QPSK_ERR_ARG and push(px, 3 * K, K, nout, None, 4 * nout) == QPSK_ERR_ARG
    for nn in (0, -3, (1 << 24) + 1):
        assert push(px, 3 * K, K, nn, po, 0) == QPSK_ERR_ARG, nn
        assert fresh.L.qpsk_resample_need(fresh.h, nn) == QPSK_ERR_ARG, nn
    for nin in (K - 1, K + 1, 0, -1):
        assert push(px, 3 * K, nin, nout, po, 4 * nout) == QPSK_ERR_ARG, nin
    assert b"qpsk_resample_need" in err() or b"nin" in err()
    assert push(px, K - 1, K, nout, po, 4 * nout) == QPSK_ERR_ARG and push(px, -1, K, nout, po, 4 * nout) == QPSK_ERR_ARG
    assert push(px, 3 * K, K, nout, po, nout - 1) == QPSK_ERR_ARG and push(px, 3 * K, K, nout, po, -1) == QPSK_ERR_ARG
    assert push(px, (1 << 62), K, nout, po, 4 * nout) == QPSK_ERR_ARG                 # an extent that leaves the address space
    assert push(px, 3 * K, K, nout, po, (1 << 62)) == QPSK_ERR_ARG
    assert fresh.L.qpsk_resample_push(None, ptr(px), 3 * K, K, nout, ptr(po), 4 * nout) == QPSK_ERR_ARG
    assert push(px, 3 * K, K, nout, px, 4 * nout) == QPSK_ERR_ARG                    # d_out is d_in
    assert b"overlaps" in err()
    last_in = 8 * ((S - 1) * 3 * K + K - 1)
    assert push(px, 3 * K, K, nout, px + last_in, 4 * nout) == QPSK_ERR_ARG          # d_out begins in d_in's last sample
    assert push(px + 8 * nout, 3 * K, K, nout, px, 3 * K) == QPSK_ERR_ARG            # d_in begins between d_out's first two rows
    assert b"overlaps" in err()
    fresh.sync()
    assert fresh.last_kernel() == before
    assert torch.all(out == POISON).item()
    # the refused resets and pushes left the resampler, its zero history and its position: the next push is the first
    assert fresh.resample_need(nout) == K
    assert push(*good) == 0
    fresh.sync()
    want, state = resample_ref(xs[:, :K], None, h, L, D, P, nout)
    got = out.cpu().numpy()
    assert fresh.last_kernel() == KERNEL and np.array_equal(bits(got[:, :nout]), bits(want)) and np.all(got[:, nout:] == POISON)
    assert reset(S, 0, D, P, hp) == QPSK_ERR_ARG                                     # a refused reset leaves the one the context has
    K2 = fresh.resample_need(nout)
    assert K2 == need_ref(state[1], L, D, nout)
    got = fresh.resample(xs[:, K:K + K2], nout).cpu().numpy()
    want, _ = resample_ref(xs[:, K:K + K2], state, h, L, D, P, nout)
    assert np.array_equal(bits(got), bits(want))
    # nout D + L must stay below 2^31: decided with the resampler's D
    fresh.resample_reset(1, 1, 4096, 2, taps(1, 2))
    assert fresh.L.qpsk_resample_need(fresh.h, 1 << 19) == QPSK_ERR_ARG and b"2^31" in err()
    assert fresh.L.qpsk_resample_need(fresh.h, (1 << 19) - 1) == ((1 << 19) - 2) * 4096 + 1
    fresh.close()


# ------------------------------------------------------------------- 6. independence
def test_resample_pushes_between_the_other_stages_calls_leave_them_as_they_are(m):
    """a streams_rx_cplx sequence, a channeliser sequence and a synthesis sequence with resample pushes between their calls give the
    sequences' own results -- and the resampler, with all of those between its pushes, its own"""
    import qpsk_amd
    S, Lf = 3, LINK["L"]
    rng = np.random.default_rng(66)
    blocks = (0.5 * rng.standard_normal((4, S, Lf, 2))).astype(np.float32)
    keys = ("sym", "freq", "phase", "costas", "index")
    M, PC = 16, 4
    hc = qpsk_amd.channel_prototype(M, PC)
    wide = rng.standard_normal((4, 37 * M, 2)).astype(np.float32)
    rows = rng.standard_normal((4, M, 21, 2)).astype(np.float32)
    L, D, P, nout = 7, 3, 5, 50
    h = taps(L, P)
    x = samples(2, total_in(L, D, 4 * nout), 8)

    def run(between):
        m.streams_reset(S, 1500.0)
        m.channel_reset(M, PC, hc)
        m.synth_reset(M, PC, hc)
        state, at = None, 0
        if between:
            m.resample_reset(2, L, D, P, h)
        out = []
        for i, b in enumerate(blocks):
            if between:
                (pair,), state, at = run_pushes(m, 2, L, D, P, h, [nout], x, reset=False, state=state, at=at)
                assert np.array_equal(bits(pair[0]), bits(pair[1])), i
            o = m.streams_rx_cplx(b, want_costas=True)
            rec = {k: o[k].cpu().numpy() for k in keys}
            rec["channel"] = m.channel(wide[i]).cpu().numpy()
            rec["synth"] = m.synth(rows[i]).cpu().numpy()
            out.append(rec)
        m.sync()
        return out

    plain, mixed = run(False), run(True)
    for a, b in zip(plain, mixed):
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ------------------------------------------------------------------- 7. the link on the device
def test_the_link_through_five_fourths_and_four_fifths_with_library_calls_equals_the_cpu_chain(m, oracle):
    """test_resample_cpu's link with library calls only, two Modems for the two rates: frame -> tx_symbols (baseband at 9600 Hz) -> the
    12 kS/s Modem's resampler 5 / 4 in the CPU chain's irregular blocks -> the 9600 Hz Modem's resampler 4 / 5 -> its streams_rx_cplx ->
    deframe, a frame at a time.  The baseband, the 12 kS/s rows and the 9600 Hz rows equal the CPU chain's bit for bit; the packets'
    counts, payloads and crc_ok equal the CPU chain's, which the CPU test has pinned to what was sent"""
    import qpsk_amd
    import torch
    k, shape = LINK, link_shape()
    (L1, D1, P1), (L2, D2, P2) = k["up"], k["down"]
    S, Lf = k["nstreams"], k["L"]
    r = link_result(oracle)
    m12 = qpsk_amd.Modem(fs=k["fs"] * L1 / D1, rs=k["rs"], frame_size=Lf * L1 // D1)
    assert m12.cycles == 5 and m.cycles == 4
    o = m.frame(shape["payloads"], shape["sync"], coded=False, per_row=k["per_row"], lead=k["lead"], gap=k["gap"], row_len=shape["row_len"])
    assert np.array_equal(o["dibits"].cpu().numpy(), r["rows"])
    m.tx_reset(S, 1550.0)
    bb = m.tx_symbols(o["dibits"], want_pcm=True, want_baseband=True)["baseband"]
    assert np.array_equal(bits(bb.cpu().numpy()), bits(r["baseband"]))
    n = bb.shape[1]
    # up, at the 12 kS/s Modem
    m12.resample_reset(S, L1, D1, P1, r["h1"])
    ups, at = [], 0
    for nout, K1 in zip(up_blocks(n * L1 // D1), r["K1"]):
        assert m12.resample_need(nout) == K1
        ups.append(m12.resample(bb[:, at:at + K1], nout))
        at += K1
    up = torch.cat(ups, dim=1)
    assert at == n and np.array_equal(bits(up.cpu().numpy()), bits(r["up"]))
    # down, at the 9600 Hz Modem, into its receiver
    m.resample_reset(S, L2, D2, P2, r["h2"])
    m.streams_reset(S, 1500.0)
    m.deframer_reset(S, shape["sync"], k["nbytes"], k["min_score"], max_packets=4)
    got = [[] for _ in range(S)]
    at = 0
    for b, K2 in enumerate(r["K2"]):
        assert m.resample_need(Lf) == K2
        y = m.resample(up[:, at:at + K2], Lf)
        at += K2
        assert y.is_contiguous() and np.array_equal(bits(y.cpu().numpy()), bits(r["down"][:, b * Lf:(b + 1) * Lf]))
        rx = m.streams_rx_cplx(y, want_costas=True)
        d = m.deframe(costas=rx)
        hh = {key: d[key].cpu().numpy() for key in ("count", "bytes", "crc_ok")}
        for s in range(S):
            got[s] += [(hh["bytes"][s, j].tobytes(), bool(hh["crc_ok"][s, j])) for j in range(hh["count"][s])]
    m.sync()
    m12.close()
    for s in range(S):
        assert got[s] == [(g[3], g[4]) for g in r["records"][s]], s
        assert len(got[s]) == k["per_row"]
