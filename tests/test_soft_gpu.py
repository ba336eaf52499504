"""qpsk_soft_batch / Modem.soft / Modem.quality on the GPU: sums, quality figures and soft decisions bit for bit against
test_soft_cpu.soft_ref (the definition of include/qpsk_hip.h restated in numpy), on random rows, on the library's own costas_frame[]
and through the whole chain with qpsk_sync_batch, and the error contract."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TIMING_FIXED
from sigutil import bits_equal, make_frames
from test_rx_data_cpu import make_packet_frame, transmit
from test_soft_cpu import MODES, soft_ref

pytestmark = pytest.mark.gpu

FS, RS, L2 = 19200.0, 2400.0, 16384
QPSK_ERR_ARG, QPSK_ERR_RANGE = -2, -6
ONE_PASS_MAX = 4096                     # kernels.h, SOFT_ONE_PASS_MAX: rows up to this many symbols are read once
ONE_PASS, TWO_PASS = "soft_onepass_kernel", "soft_sums_kernel + soft_apply_kernel"
GUARD = 64                              # elements behind every output that must stay untouched


def modem(**kw):
    import qpsk_amd
    kw.setdefault("fs", FS)
    kw.setdefault("rs", RS)
    kw.setdefault("frame_size", L2)
    return qpsk_amd.Modem(**kw)


def dev(a, dtype=None):
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw(m, z, pitch, R, N, skip, mode, scale, gain, lag, rot, first, nout, soft, quality, sums):
    return m.L.qpsk_soft_batch(m.h, ptr(z) if hasattr(z, "data_ptr") else z, pitch, R, N, skip, mode, scale, ptr(gain), ptr(lag), ptr(rot),
                               first, nout, ptr(soft) if hasattr(soft, "data_ptr") or soft is None else soft, ptr(quality), ptr(sums))


def run(m, z, skip=0, mode="unit", scale=64.0, gain=None, lag=None, rot=None, first=0, nout=None, want=("soft", "quality", "sums"),
        pitch=0, nsym=None):
    """the raw call with guarded outputs; z: numpy (R, N, 2) or a device tensor of pitched rows (then nsym is given).  -> host arrays"""
    import torch
    zt = z if hasattr(z, "data_ptr") else dev(z, np.float32)
    R = zt.shape[0]
    N = zt.shape[1] if nsym is None else nsym
    nout = N - first if nout is None else nout
    bufs = {}
    if "soft" in want:
        bufs["soft"] = torch.full((R * nout * 2 + GUARD,), 0x55, dtype=torch.int8, device="cuda")
    if "quality" in want:
        bufs["quality"] = torch.full((R * 4 + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    if "sums" in want:
        bufs["sums"] = torch.full((R * 4 + GUARD,), 7.0, dtype=torch.float64, device="cuda")
    keep = [dev(gain, np.float32), dev(lag, np.int32), dev(rot, np.int32)]
    m._check(raw(m, zt, pitch, R, N, skip, MODES[mode], scale, keep[0], keep[1], keep[2], first, nout, bufs.get("soft"), bufs.get("quality"),
                 bufs.get("sums")))
    kernel = m.last_kernel()
    torch.cuda.synchronize()
    out = {"kernel": kernel}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        n = h.size - GUARD
        assert np.all(h[n:] == (0x55 if k == "soft" else 7.0)), "guard behind %s overwritten" % k
        out[k] = h[:n].reshape((R, nout, 2) if k == "soft" else (R, 4))
    return out


def assert_equal(got, want, what=""):
    for k in ("sums", "quality", "soft"):
        if k in got:
            bad = np.nonzero((got[k].reshape(len(got[k]), -1) != want[k].reshape(len(want[k]), -1)).any(axis=1))[0]
            assert bits_equal(got[k], want[k]), (what, k, "rows", bad[:8])


def random_rows(R, N, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal((R, N, 2))).astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. random rows, every shape
@pytest.mark.parametrize("amp", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("N", [64, 256, 257, 2048, 2049, ONE_PASS_MAX, ONE_PASS_MAX + 1])
def test_random_rows_bit_for_bit(amp, N):
    """sums, quality and soft output; every skip, mode and rotation; lags at 0, in the middle and at the last legal value; soft scales that
    saturate (scale 1e3 in UNIT mode: everything at +-127) and that resolve the noise"""
    m = modem()
    R = 3
    z = random_rows(R, N, N + int(amp * 10), amp)
    first, nout = 5, N // 2 + 1                                   # odd and even nout: the rows' outputs start on odd / even 2-byte boundaries
    lag = np.array([0, (N - first - nout) // 2, N - first - nout], np.int32)
    for i, skip in enumerate(sorted({0, 1, 255 % N, 256 % N, N - 1})):
        for mode, scale in (("unit", 64.0), ("unit", 1e3), ("llr", 0.125), ("llr", 4.0)):
            rot = np.array([i, i + 1, i + 2 + 4 * i], np.int32)
            got = run(m, z, skip=skip, mode=mode, scale=scale, lag=lag, rot=rot, first=first, nout=nout)
            assert got["kernel"] == (ONE_PASS if N <= ONE_PASS_MAX else TWO_PASS)
            assert_equal(got, soft_ref(z, skip=skip, mode=mode, scale=scale, lag=lag, rot=rot, first=first, nout=nout), (skip, mode, scale))
    m.sync()
    m.close()


@pytest.mark.parametrize("R,N", [(1, 131072), (4096, 2048), (1, 1 << 21), (5, 1), (2, 3)])
def test_batch_shapes_bit_for_bit(R, N):
    m = modem()
    z = random_rows(R, N, R + N)
    rng = np.random.default_rng(R)
    skip = min(256, N - 1)
    nout = N - N // 3
    lag = rng.integers(0, N - nout + 1, R).astype(np.int32)
    rot = rng.integers(0, 4, R).astype(np.int32)
    got = run(m, z, skip=skip, mode="llr", scale=0.5, lag=lag, rot=rot, nout=nout)
    assert got["kernel"] == (ONE_PASS if N <= ONE_PASS_MAX else TWO_PASS)
    assert_equal(got, soft_ref(z, skip=skip, mode="llr", scale=0.5, lag=lag, rot=rot, nout=nout))
    m.sync()
    m.close()


def test_ties_round_to_even_and_zero_rows():
    m = modem()
    N = 512
    rng = np.random.default_rng(8)
    # components are odd integers around 128 with mean |component| exactly 128: UNIT scale 64 gives g = 0.5 and every product is k + 0.5
    mag = np.tile(np.array([127, 129, 125, 131, 1, 255, 63, 193], np.float32), N * 2 // 8)
    z = (mag * rng.choice([-1.0, 1.0], N * 2)).astype(np.float32).reshape(1, N, 2)
    want = soft_ref(z)
    assert want["gain"][0] == 0.5 and set(np.abs(want["soft"]).reshape(-1).tolist()) == {64, 62, 66, 0, 127, 32, 96}
    assert_equal(run(m, z), want)
    # the caller's gain: products at k + 0.5 for every k that fits, and far beyond saturation
    z2 = np.arange(-600, 600, dtype=np.float32).reshape(1, 600, 2)
    for rot in range(4):
        g = run(m, z2, gain=[0.5], rot=[rot], want=("soft",))
        assert g["kernel"] == "soft_apply_kernel"
        assert_equal(g, soft_ref(z2, gain=[0.5], rot=[rot]))
    # all-zero rows: gain 0, quality 0, soft 0 -- in both modes, next to rows that are not
    z3 = random_rows(4, 300, 3)
    z3[1] = 0.0
    z3[3] = -0.0
    for mode in MODES:
        got = run(m, z3, mode=mode, scale=2.0, skip=9)
        assert_equal(got, soft_ref(z3, mode=mode, scale=2.0, skip=9))
        assert not got["quality"][[1, 3]].any() and not got["soft"][[1, 3]].any() and not got["sums"][[1, 3]].any()
    m.sync()
    m.close()


def test_pitched_rows_never_read_the_gap():
    import torch
    m = modem()
    for N, pitch in ((2048, 2053), (ONE_PASS_MAX + 1, ONE_PASS_MAX + 2)):
        R = 5
        z = random_rows(R, N, N)
        buf = np.full((R, pitch, 2), np.nan, np.float32)
        buf[:, :N] = z
        bt = torch.from_numpy(buf).cuda()
        lag = np.array([0, 3, N - 100, 1, 50], np.int32)
        for want in (("soft", "quality", "sums"), ("quality",), ("soft",)):
            gain = [0.25] * R if want == ("soft",) else None
            got = run(m, bt, skip=256, mode="llr", scale=0.5, lag=lag, first=0, nout=100, pitch=pitch, nsym=N, want=want, gain=gain)
            assert_equal(got, soft_ref(z, skip=256, mode="llr", scale=0.5, lag=lag, first=0, nout=100, gain=gain))
        m.sync()                                                   # no QPSK_ERR_RANGE: the NaNs were not read
    m.close()


@pytest.mark.parametrize("N", [700, ONE_PASS_MAX + 700])
def test_each_output_alone_equals_all_together(N):
    m = modem()
    R = 7
    z = random_rows(R, N, 70 + N, 0.3)
    rng = np.random.default_rng(N)
    kw = dict(skip=100, mode="unit", scale=50.0, lag=rng.integers(0, 50, R).astype(np.int32), rot=rng.integers(0, 4, R).astype(np.int32),
              first=32, nout=N - 32 - 50)
    want = soft_ref(z, **kw)
    kernels = set()
    for outs in (("soft", "quality", "sums"), ("soft",), ("quality",), ("sums",), ("soft", "sums"), ("quality", "sums")):
        got = run(m, z, want=outs, **kw)
        kernels.add(got["kernel"])
        assert_equal(got, want, outs)
    assert kernels == {ONE_PASS if N <= ONE_PASS_MAX else TWO_PASS, "soft_sums_kernel"}
    # the caller's gain with and without the quality figures: the same soft output, the row's own quality
    gain = rng.uniform(0.5, 90.0, R).astype(np.float32)
    want = soft_ref(z, gain=gain, **kw)
    for outs in (("soft",), ("soft", "quality"), ("soft", "quality", "sums")):
        assert_equal(run(m, z, want=outs, gain=gain, **kw), want, outs)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. the library's own costas_frame[]
def test_batch_costas_rows_and_the_python_front_end(oracle):
    m = modem(timing_mode=TIMING_FIXED, fixed_index=6)
    F = 40
    x = np.concatenate([make_frames(F // 2, L2, 8, m.taps, FS, offset_hz=20.0, noise=n, base_seed=s)[0] for n, s in ((0.05, 1), (0.2, 2))])
    rx = m.rx_batch_ext(x, want_costas=True)
    z = rx["costas"].cpu().numpy()
    for kw in (dict(skip=256), dict(skip=256, mode="llr", scale=0.25, first=300, nout=1000), dict(scale=20.0, want_sums=True)):
        got = m.soft(rx, **kw)
        m.sync()
        assert m.last_kernel() == ONE_PASS
        ref_kw = {k: v for k, v in kw.items() if k != "want_sums"}
        want = soft_ref(z, **ref_kw)
        assert ("sums" in got) == bool(kw.get("want_sums"))
        assert_equal({k: got[k].cpu().numpy() for k in ("soft", "quality", "sums") if k in got}, want, kw)
    q = m.quality(rx, skip=256)
    m.sync()
    assert m.last_kernel() == "soft_sums_kernel" and "soft" not in q
    qh = q["quality"].cpu().numpy()
    assert bits_equal(qh, soft_ref(z, skip=256)["quality"])
    # the figures read as the CPU tests say: locked frames, and the noisier half reads the lower SNR
    assert np.all(qh[:, 2] > 0.5) and qh[:F // 2, 1].min() > qh[F // 2:, 1].max()
    m.close()


def test_stream_costas_rows(oracle):
    fs, L, S = 9600.0, 512, 70
    m = modem(fs=fs, frame_size=L)
    m.streams_reset(S, 1500.0)
    rng = np.random.default_rng(5)
    pcm = (5000 * rng.standard_normal((3, S, L))).astype(np.int16)
    for b in range(3):
        o = m.streams_rx_pcm(pcm[b])
        got = m.soft(o, skip=16, mode="llr", scale=0.5, want_sums=True)
        m.sync()
        want = soft_ref(o["costas"].cpu().numpy(), skip=16, mode="llr", scale=0.5)
        assert_equal({k: got[k].cpu().numpy() for k in ("soft", "quality", "sums")}, want, b)
    m.close()


def test_chain_with_sync_gives_the_payloads_hard_decisions(oracle):
    """carrier_est -> rx_batch_ext (costas_frame[]) and rx_batch_data (decisions) -> sync -> soft with sync's lag and rot: the sign of
    every non-zero soft value is the de-rotated dibit's bit, at all four rotations, and the values equal soft_ref"""
    import torch
    F, C8, nbytes, prefix, nsync = 64, 8, 64, 120, 64
    nsym = L2 // C8
    taps = oracle.rrc_make(np.float32(FS), np.float32(RS), np.float32(0.35))
    rng = np.random.default_rng(77)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    x = np.stack([transmit(make_packet_frame(oracle, rng, nsym, prefix, sync, nbytes)[0], L2, C8, taps, FS, offset_hz=float(rng.uniform(-250, 250)),
                           phase=float(rng.uniform(0, 2 * np.pi)), noise=0.03, seed=f) for f in range(F)])
    m = modem(timing_mode=TIMING_FIXED, fixed_index=126 % C8)
    xt = torch.from_numpy(x).cuda()
    est = m.carrier_est(xt)
    idx = torch.full((F,), 126 % C8, dtype=torch.int32)
    rx = m.rx_batch_ext(xt, index=idx, seed=est["seed"], want_costas=True)
    data = m.rx_batch_data(xt, index=idx, seed=est["seed"])["data"]
    nout = 4 * (nbytes + 2)
    s = m.sync(data, sync, 0, 255, nout)
    got = m.soft(rx, skip=256, lag=s["lag"], rot=s["rot"], first=nsync, nout=nout)
    m.sync()
    q, out = got["soft"].cpu().numpy(), s["out"].cpu().numpy()
    lag, rot = s["lag"].cpu().numpy(), s["rot"].cpu().numpy()
    assert np.all(lag == prefix + 126 // C8) and set(rot.tolist()) == {0, 1, 2, 3}
    for bit in (0, 1):
        nz = q[:, :, bit] != 0
        assert nz.mean() > 0.99
        assert np.array_equal((q[:, :, bit] < 0)[nz], ((out >> bit) & 1).astype(bool)[nz]), bit
    assert_equal({"soft": q, "quality": got["quality"].cpu().numpy()},
                 soft_ref(rx["costas"].cpu().numpy(), skip=256, lag=lag, rot=rot, first=nsync, nout=nout))
    m.close()


# ------------------------------------------------------------------------------------------ 3. the error contract
def test_argument_errors_launch_nothing():
    import torch
    m = modem()
    R, N = 4, 100
    z = torch.zeros((R, N, 2), dtype=torch.float32, device="cuda")
    soft = torch.full((R * N * 2,), 0x55, dtype=torch.int8, device="cuda")
    qual = torch.full((R, 4), 7.0, dtype=torch.float32, device="cuda")
    sums = torch.full((R, 4), 7.0, dtype=torch.float64, device="cuda")
    inf, nan = float("inf"), float("nan")
    ok = dict(z=z, pitch=0, R=R, N=N, skip=0, mode=0, scale=64.0, gain=None, lag=None, rot=None, first=10, nout=90, soft=soft, quality=qual,
              sums=sums)
    assert raw(m, **ok) == 0
    m.sync()
    soft.fill_(0x55)
    qual.fill_(7.0)
    sums.fill_(7.0)
    cases = [dict(skip=-1), dict(skip=N), dict(first=11), dict(nout=-1), dict(first=-1, nout=5), dict(soft=None, quality=None, sums=None),
             dict(mode=2), dict(mode=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=inf), dict(scale=nan), dict(pitch=N - 1), dict(pitch=-5),
             dict(z=None), dict(R=0), dict(N=0), dict(N=(1 << 21) + 1, skip=0), dict(z=C.c_void_p(z.data_ptr() + 4)),
             dict(soft=C.c_void_p(soft.data_ptr() + 1)),
             dict(soft=C.c_void_p(z.data_ptr() + 8 * R * N - 2)), dict(z=C.c_void_p(soft.data_ptr() + 8), R=1, N=10, first=0, nout=10)]
    for i, c in enumerate(cases):
        assert raw(m, **{**ok, **c}) == QPSK_ERR_ARG, (i, c)
    assert m.L.qpsk_soft_batch(None, ptr(z), 0, R, N, 0, 0, 64.0, None, None, None, 0, N, ptr(soft), None, None) == QPSK_ERR_ARG
    # with d_soft NULL, first and nout are ignored
    assert raw(m, **{**ok, "soft": None, "first": 1000, "nout": -7}) == 0
    m.sync()
    assert torch.all(soft == 0x55) and torch.all(sums != 7.0)
    m.close()


def test_a_soft_output_that_touches_the_input_is_accepted_and_a_shared_pair_is_refused():
    """2 rows of 16 symbols at pitch 20 inside one allocation: the input spans 8 (20 + 16) = 288 bytes -- the 32 bytes of padding behind the
    last row are not the buffer -- and d_soft 64.  d_soft is 2-byte aligned, so the least the two can share is one int8 pair.  An empty
    d_soft (nout = 0) that points inside the input is refused as it always was; on either end of it, it is accepted"""
    import torch
    m = modem()
    R, N, P = 2, 16, 20
    z = random_rows(R, N, 77)
    want = soft_ref(z, first=0, nout=N)
    arena = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    at = lambda off: C.c_void_p(arena.data_ptr() + off)      # noqa: E731
    rows = np.zeros((R, P, 2), np.float32)
    rows[:, :N] = z
    for off, nout, accepted in ((544, N, True), (192, N, True), (542, N, False), (194, N, False), (256, 0, True), (544, 0, True), (300, 0, False)):
        arena.zero_()
        arena[256:256 + rows.nbytes] = torch.from_numpy(rows.view(np.uint8).reshape(-1)).cuda()
        rc = raw(m, at(256), P, R, N, 0, 0, 64.0, None, None, None, 0, nout, at(off), None, None)
        if not accepted:
            assert rc == QPSK_ERR_ARG and b"qpsk_soft_batch: d_soft overlaps d_costas" in m.L.qpsk_last_error(), (off, nout, rc)
            continue
        assert rc == 0, (off, nout, m.L.qpsk_last_error())
        m.sync()
        if nout:
            assert np.array_equal(arena[off:off + 2 * R * N].cpu().numpy().view(np.int8).reshape(R, N, 2), want["soft"]), off
    m.close()


@pytest.mark.parametrize("N", [600, ONE_PASS_MAX + 600])
def test_bad_device_lag_gives_zeros_for_that_row_only(N):
    import qpsk_amd
    m = modem()
    R, first, nout = 6, 16, 200
    z = random_rows(R, N, N + 1)
    last = N - first - nout
    lag = np.array([0, last + 1, last, -1, 2 ** 31 - 1, -2 ** 31], np.int32)
    for gain in (None, np.full(R, 3.0, np.float32)):
        got = run(m, z, lag=lag, first=first, nout=nout, gain=gain, want=("soft", "quality") if gain is None else ("soft",))
        with pytest.raises(qpsk_amd.QpskError) as e:
            m.sync()
        assert "error %d" % QPSK_ERR_ARG in str(e.value)
        want = soft_ref(z, lag=lag, first=first, nout=nout, gain=gain)
        assert_equal(got, want)
        assert not got["soft"][[1, 3, 4, 5]].any() and got["soft"][0].any() and got["soft"][2].any()
        # the context works again
        lag_ok = np.clip(lag, 0, last).astype(np.int32)
        assert_equal(run(m, z, lag=lag_ok, first=first, nout=nout, gain=gain), soft_ref(z, lag=lag_ok, first=first, nout=nout, gain=gain))
        m.sync()
    m.close()


@pytest.mark.parametrize("N", [600, ONE_PASS_MAX + 600])
def test_nonfinite_input_is_a_range_error(N):
    import qpsk_amd
    m = modem()
    R, skip, first, nout = 3, 100, 300, 200
    z0 = random_rows(R, N, N + 2)

    def expect_range_error(z, **kw):
        run(m, z, skip=skip, first=first, nout=nout, **kw)
        with pytest.raises(qpsk_amd.QpskError) as e:
            m.sync()
        assert "error %d" % QPSK_ERR_RANGE in str(e.value), kw

    for pos, bad in ((skip, np.nan), (N - 1, np.inf), (first + 7, -np.inf)):
        z = z0.copy()
        z[1, pos, pos & 1] = bad
        expect_range_error(z)
        expect_range_error(z, want=("quality",))
    # the caller's gain and no quality output: only the payload is read
    z = z0.copy()
    z[2, first + nout - 1, 0] = np.nan
    expect_range_error(z, gain=[1.0, 1.0, 1.0], want=("soft",))
    expect_range_error(z0, gain=[1.0, np.inf, 1.0], want=("soft",))
    expect_range_error(z0, gain=[np.nan, 1.0, 1.0])
    # not read: before skip (sums) and outside the payload (soft) -- the call succeeds and equals the reference on the clean rows
    z = z0.copy()
    z[0, :skip] = np.nan
    got = run(m, z, skip=skip, want=("quality", "sums"))
    m.sync()
    assert_equal(got, soft_ref(z0, skip=skip))
    z = z0.copy()
    z[0, :first] = np.inf
    z[0, first + nout:] = np.nan
    got = run(m, z, first=first, nout=nout, gain=[2.0] * R, want=("soft",))
    m.sync()
    assert_equal(got, soft_ref(z0, first=first, nout=nout, gain=[2.0] * R))
    m.close()


def test_other_state_is_left_alone():
    """stream-ordered on the context's stream; the histogram mode's guess and the receive streams are neither read nor updated"""
    import torch
    from oracle.pyoracle import TIMING_HIST
    L, F = 2048, 1024
    m = modem(frame_size=L, timing_mode=TIMING_HIST)
    x, _ = make_frames(F, L, 8, m.taps, FS, offset_hz=40.0, base_seed=21, noise=0.01)
    xt = torch.from_numpy(x).cuda()
    m.rx_batch(xt)
    rx = m.rx_batch(xt, want_costas=True)
    st0, st1 = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    m._check(m.L.qpsk_test_hist_state(m.h, st0))
    got = m.soft(rx, skip=32)
    m.sync()
    m._check(m.L.qpsk_test_hist_state(m.h, st1))
    assert list(st0) == list(st1)
    assert_equal({k: got[k].cpu().numpy() for k in ("soft", "quality")}, soft_ref(rx["costas"].cpu().numpy(), skip=32))
    m.close()
