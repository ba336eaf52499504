"""qpsk_carrier_est_batch / Modem.carrier_est on the GPU: bit for bit against test_carrier_est_cpu.oracle_carrier_est (the definition
of include/qpsk_hip.h restated on the oracle), end to end through qpsk_rx_batch_ext, and the error contract."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TAU, TIMING_FIXED, TIMING_HIST
from sigutil import bits_equal, make_frames, random_frames
from test_carrier_est_cpu import oracle_carrier_est, quadrant_errors, search_set
from test_rx_ext_cpu import oracle_ext

pytestmark = pytest.mark.gpu

RS, L2 = 2400.0, 16384                      # config 2: 2400 baud, 16384 samples per frame (FS 19200 at CYCLES 8)
QPSK_ERR_ARG, QPSK_ERR_RANGE = -2, -6


def modem(C_, L=L2, **kw):
    import qpsk_amd
    return qpsk_amd.Modem(fs=RS * C_, rs=RS, frame_size=L, **kw)


def host(o):
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_") and v is not None}


def assert_bits(got, want, rows=None):
    """seed, freq, bin and the bits of line, on the listed rows of got (want holds exactly those rows)"""
    for key in ("seed", "freq", "bin", "line"):
        if key not in got:
            continue
        g = got[key] if rows is None else got[key][rows]
        assert bits_equal(g, want[key]), (key, np.nonzero(g.reshape(len(g), -1) != want[key].reshape(len(g), -1))[0][:8])


def stimulus(C_, L, taps, n, seed):
    """offset frames at +-(RS/8 - half a bin) and inside, noise-only, zero and partly zero frames"""
    fs = RS * C_
    edge = RS / 8 - 0.5 * RS * C_ / (4.0 * n)
    frames = []
    for i, df in enumerate((edge, -edge, 37.0, -211.0)):
        frames.append(make_frames(1, L, C_, taps, fs, offset_hz=df, base_seed=seed + i, noise=0.05)[0][0])
    frames.append(random_frames(1, L, seed=seed + 9)[0])
    frames.append(np.zeros((L, 2), np.float32))
    part = make_frames(1, L, C_, taps, fs, offset_hz=120.0, base_seed=seed + 7, noise=0.02)[0][0]
    part[: L // 2] = 0.0
    frames.append(part)
    return np.stack(frames)


# ------------------------------------------------------------------------------------------ 1. shapes, bit for bit
@pytest.mark.parametrize("C_", [4, 8])
@pytest.mark.parametrize("n", [64, 512, 1024, 8192])
def test_every_window_bit_for_bit(oracle, C_, n):
    m = modem(C_, timing_mode=TIMING_FIXED)
    x = stimulus(C_, L2, m.taps, n, 40 + n + C_)
    for start in (0, 1, 128, L2 - n):
        got = host(m.carrier_est(x, n=n, start=start, want_line=True))
        want = oracle_carrier_est(oracle, x, m.taps, C_, n, start)
        assert_bits(got, want)
        assert m.last_kernel() == "carrier_est_kernel"
    m.sync()
    m.close()


def test_edge_offsets_are_found_within_a_bin(oracle):
    """+-(RS/8 - half a bin) lands on the edge bins of S, not on a sideband"""
    m = modem(8, timing_mode=TIMING_FIXED)
    n = 1024
    x = stimulus(8, L2, m.taps, n, 77)
    got = host(m.carrier_est(x[:2], n=n))
    true_w = TAU * (RS / 8 - 0.5 * RS * 8 / (4.0 * n)) / RS
    bw = TAU * 8 / (4.0 * n)
    assert abs(got["freq"][0] - true_w) <= bw and abs(got["freq"][1] + true_w) <= bw
    m.close()


def test_pitched_and_unaligned_input(oracle):
    import torch
    C_, n, F = 8, 1024, 7
    m = modem(C_, timing_mode=TIMING_FIXED)
    x = stimulus(C_, L2, m.taps, n, 5)
    pitch = L2 + 6
    buf = np.zeros((F, pitch, 2), np.float32)
    buf[:, :L2] = x
    buf[:, L2:] = np.nan                                       # never read: past every frame's end
    for start in (0, 3, L2 - n):
        got = host(m.carrier_est(buf, n=n, start=start, pitch=pitch, want_line=True))
        assert_bits(got, oracle_carrier_est(oracle, x, m.taps, C_, n, start))
    # one sample (8 bytes) off a 16-byte boundary, pitched
    flat = torch.zeros(F * pitch * 2 + 2, dtype=torch.float32)
    flat[2:].view(F, pitch, 2)[:] = torch.from_numpy(buf)
    flat = flat.cuda()
    out = {k: torch.empty(s, dtype=d, device="cuda") for k, s, d in
           (("seed", (F, 2), torch.float32), ("freq", (F,), torch.float32), ("bin", (F,), torch.int32), ("line", (F, 2), torch.float64))}
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    m._check(m.L.qpsk_carrier_est_batch(m.h, C.c_void_p(flat.data_ptr() + 8), pitch, F, 1, n, p(out["seed"]), p(out["freq"]),
                                        p(out["bin"]), p(out["line"])))
    assert_bits(host(out), oracle_carrier_est(oracle, x, m.taps, C_, n, 1))
    m.sync()
    m.close()


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [64, 512, 1024, 2048])
def test_custom_taps(oracle, symmetric, n):
    """set_taps: a symmetric set (the stream with the taps in SGPRs) and an asymmetric one (taps in LDS), at every n that selects a
    different number of waves per workgroup (1, 1, 2, 4)"""
    C_ = 8
    m = modem(C_, timing_mode=TIMING_FIXED)
    t = oracle.rrc_make(np.float32(RS * C_), np.float32(RS), np.float32(0.5))
    if not symmetric:
        t = (t * np.linspace(0.8, 1.2, 127)).astype(np.float32)
    m.set_taps(t)
    x = stimulus(C_, L2, t, n, 11)
    for start in (0, 129):
        got = host(m.carrier_est(x, n=n, start=start, want_line=True))
        assert_bits(got, oracle_carrier_est(oracle, x, t, C_, n, start))
    # QPSK_FIR_GENERIC = 1 takes the taps-in-LDS stream also for the symmetric set
    m.tune(fir_generic=1)
    got = host(m.carrier_est(x, n=n, start=1, want_line=True))
    assert_bits(got, oracle_carrier_est(oracle, x, t, C_, n, 1))
    m.sync()
    m.close()


def test_narrowed_clamp(oracle):
    C_, n = 8, 1024
    m = modem(C_, timing_mode=TIMING_FIXED)
    a, b = m.gains
    x = stimulus(C_, L2, m.taps, n, 21)
    for lo, hi in ((-0.2, 0.3), (0.05, 0.5), (-0.6, -0.55)):
        m.set_loop(a, b, lo, hi)
        got = host(m.carrier_est(x, n=n, want_line=True))
        want = oracle_carrier_est(oracle, x, m.taps, C_, n, 128, min_freq=lo, max_freq=hi)
        assert_bits(got, want)
        assert np.all(got["freq"] >= np.float32(lo)) and np.all(got["freq"] <= np.float32(hi))
    m.sync()
    m.close()


@pytest.mark.parametrize("F", [1, 63, 65, 4097])
def test_ragged_batches(oracle, F):
    import torch
    C_, n = 8, 1024
    m = modem(C_, timing_mode=TIMING_FIXED)
    xu = stimulus(C_, L2, m.taps, n, 31)
    fid = np.arange(F) % len(xu)
    xt = torch.from_numpy(xu).cuda()[torch.from_numpy(fid).cuda()]
    got = host(m.carrier_est(xt, n=n, want_line=True))
    want = oracle_carrier_est(oracle, xu, m.taps, C_, n, 128)
    rows = sorted(set(range(min(F, 8))) | set(range(max(0, F - 8), F)) | set(range(0, F, 97)))
    assert_bits(got, {k: v[fid[rows]] for k, v in want.items()}, rows)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. end to end
@pytest.fixture(scope="module")
def doppler(oracle):
    """400 config-2 frames, offsets drawn in +-0.97 RS/8, noise 0.05 (calibrated on the oracle: every seeded frame decodes)"""
    fs, C_, F = RS * 8, 8, 400
    taps = oracle.rrc_make(np.float32(fs), np.float32(RS), np.float32(0.35))
    dfs = np.random.default_rng(2024).uniform(-0.97 * RS / 8, 0.97 * RS / 8, F)
    x = np.zeros((F, L2, 2), np.float32)
    tx = np.zeros((F, L2 // C_), np.uint8)
    for f in range(F):
        x[f:f + 1], tx[f:f + 1] = make_frames(1, L2, C_, taps, fs, offset_hz=float(dfs[f]), base_seed=9000 + f, noise=0.05)
    return dict(x=x, tx=tx, dfs=dfs)


def test_estimate_then_ext_decodes_every_frame(oracle, doppler):
    import torch
    C_, F = 8, len(doppler["x"])
    m = modem(C_, timing_mode=TIMING_FIXED, fixed_index=126 % C_)
    xt = torch.from_numpy(doppler["x"]).cuda()
    idx = torch.full((F,), 126 % C_, dtype=torch.int32)
    est = m.carrier_est(xt)
    got = m.rx_batch_ext(xt, index=idx, seed=est["seed"], want_costas=True)
    seeds = est["seed"].cpu().numpy()
    gh = host(got)
    want = oracle_ext(oracle, doppler["x"], RS * C_, RS, idx.numpy(), seeds, want_costas=True)
    for key in ("sym", "freq", "phase", "hz", "costas"):
        assert bits_equal(gh[key], want[key]), key
    errs = [quadrant_errors(gh["costas"][f], doppler["tx"][f], C_) for f in range(F)]
    assert max(errs) == 0, [(f, e) for f, e in enumerate(errs) if e][:8]
    # the unseeded control: the same frames through rx_batch fail on most frames beyond 150 Hz
    plain = host(m.rx_batch(xt, want_costas=True))
    big = np.nonzero(np.abs(doppler["dfs"]) > 150.0)[0]
    fails = sum(quadrant_errors(plain["costas"][f], doppler["tx"][f], C_) > 0 for f in big)
    assert fails > 0.9 * len(big), (fails, len(big))
    m.sync()
    m.close()


def test_doppler_estimates_bit_for_bit(oracle, doppler):
    C_ = 8
    m = modem(C_, timing_mode=TIMING_FIXED)
    rows = list(range(0, len(doppler["x"]), 13))
    got = host(m.carrier_est(doppler["x"], want_line=True))
    assert_bits(got, oracle_carrier_est(oracle, doppler["x"], m.taps, C_, 1024, 128, frames_to_check=rows), rows)
    bw = TAU * C_ / (4.0 * 1024)
    assert np.max(np.abs(got["freq"] - TAU * doppler["dfs"] / RS)) <= bw
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. error contract
def raw(m, x, pitch, F, start, n, outs):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    return m.L.qpsk_carrier_est_batch(m.h, p(x), pitch, F, start, n, *[p(t) for t in outs])


def test_argument_errors_enqueue_nothing():
    import torch
    m = modem(8, L=4096, timing_mode=TIMING_FIXED)
    F = 4
    x = torch.zeros((F, 4096, 2), device="cuda")
    seed = torch.full((F, 2), 7.0, device="cuda")
    freq = torch.full((F,), 7.0, device="cuda")
    b = torch.full((F,), 7, dtype=torch.int32, device="cuda")
    line = torch.full((F, 2), 7.0, dtype=torch.float64, device="cuda")
    outs = (seed, freq, b, line)
    cases = [
        (x, 0, F, 0, 1000, outs), (x, 0, F, 0, 32, outs), (x, 0, F, 0, 16384, outs), (x, 0, F, 0, 96, outs),
        (x, 0, F, -1, 1024, outs), (x, 0, F, 3073, 1024, outs), (x, 0, F, 0, 8192, outs),
        (x, 0, 0, 0, 1024, outs), (x, 0, -3, 0, 1024, outs), (None, 0, F, 0, 1024, outs), (x, 0, F, 0, 1024, (None,) * 4),
        (x, 4095, F, 0, 1024, outs), (x, 4097, F, 0, 1024, outs), (x, -2, F, 0, 1024, outs),
    ]
    for i, (xi, pitch, nf, start, n, o) in enumerate(cases):
        assert raw(m, xi, pitch, nf, start, n, o) == QPSK_ERR_ARG, i
    m.set_loop(*m.gains, 0.9, 1.0)                             # beyond pi / 4: S is empty
    assert raw(m, x, 0, F, 0, 1024, outs) == QPSK_ERR_ARG
    m.sync()
    assert torch.all(seed == 7.0) and torch.all(freq == 7.0) and torch.all(b == 7) and torch.all(line == 7.0)
    m.close()


def test_nonfinite_sample_inside_the_window_is_a_range_error(oracle):
    import torch
    import qpsk_amd
    C_, n, start, L = 8, 1024, 512, 4096
    m = modem(C_, L=L, timing_mode=TIMING_FIXED)
    x0, _ = make_frames(3, L, C_, m.taps, RS * C_, offset_hz=90.0, noise=0.05)
    for pos, bad in ((start + n // 2, np.nan), (start - 126, np.inf), (start + n - 1, -np.inf)):
        x = x0.copy()
        x[1, pos, 1] = bad
        m.carrier_est(x, n=n, start=start)
        with pytest.raises(qpsk_amd.QpskError) as e:
            m.sync()
        assert "error %d" % QPSK_ERR_RANGE in str(e.value), pos
    # outside the window: before start - 126 and from start + n on -- the call succeeds and the estimate is the clean frame's
    x = x0.copy()
    x[1, 0] = np.nan
    x[1, start - 127] = np.inf
    x[1, start + n:] = np.nan
    got = host(m.carrier_est(torch.from_numpy(x), n=n, start=start, want_line=True))
    m.sync()
    assert_bits(got, oracle_carrier_est(oracle, x0, m.taps, C_, n, start))
    m.close()


def test_nothing_written_past_nframes():
    import torch
    F, extra = 65, 16
    m = modem(8, L=4096, timing_mode=TIMING_FIXED)
    x = torch.from_numpy(make_frames(F, 4096, 8, m.taps, RS * 8, offset_hz=60.0, noise=0.05)[0]).cuda()
    seed = torch.full((F + extra, 2), 7.0, device="cuda")
    freq = torch.full((F + extra,), 7.0, device="cuda")
    b = torch.full((F + extra,), 7, dtype=torch.int32, device="cuda")
    line = torch.full((F + extra, 2), 7.0, dtype=torch.float64, device="cuda")
    for n in (64, 1024, 4096):
        m._check(raw(m, x, 0, F, 0, n, (seed, freq, b, line)))
        m.sync()
        assert torch.all(seed[F:] == 7.0) and torch.all(freq[F:] == 7.0) and torch.all(b[F:] == 7) and torch.all(line[F:] == 7.0)
        assert torch.all(seed[:F, 0] == 0.0) and torch.equal(seed[:F, 1], freq[:F])
    # each output alone
    for k in range(4):
        o = [None] * 4
        o[k] = (seed, freq, b, line)[k]
        m._check(raw(m, x, 0, F, 0, 512, o))
    m.sync()
    m.close()


def test_histogram_guess_is_left_alone():
    import torch
    L, F = 2048, 1024
    m = modem(8, L=L, timing_mode=TIMING_HIST)
    x, _ = make_frames(F, L, 8, m.taps, RS * 8, offset_hz=40.0, base_seed=21, noise=0.01)
    xt = torch.from_numpy(x).cuda()
    m.rx_batch(xt)
    m.rx_batch(xt)
    st0, st1 = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    m._check(m.L.qpsk_test_hist_state(m.h, st0))
    m.carrier_est(torch.from_numpy(np.ascontiguousarray(x[:, ::-1])).cuda(), n=1024)
    m.sync()
    m._check(m.L.qpsk_test_hist_state(m.h, st1))
    assert list(st0) == list(st1) and st0[0] >= 0
    assert search_set(8, 1024)                                  # (the default clamp's S is the whole band)
    m.close()
