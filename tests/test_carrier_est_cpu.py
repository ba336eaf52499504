"""The fourth-power carrier estimate (qpsk_carrier_est_batch): what can be checked without a GPU.

oracle_carrier_est() restates the definition of include/qpsk_hip.h step by step on the oracle: the filter and the transform are the
oracle's rrc_fir() and fftn() (reference-pinned code), the fourth power, the search set and the argmax are numpy fp64.  The GPU tests
(test_carrier_est_gpu.py) compare the kernel with it bit for bit; the tests here check that the definition does what it is for: the
estimate lands within a bin of the true offset inside the range, and a loop seeded with it decodes where the unseeded loop does not.
"""
import os

import numpy as np
import pytest

from oracle.pyoracle import TAU
from sigutil import make_frames
from test_rx_ext_cpu import declared, oracle_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def omega(k, C, n):
    """w(k) = (float)(TAU * (double)(k*C) / (double)(4*n)) rad/symbol"""
    return np.float32(TAU * float(k * C) / float(4 * n))


def search_set(C, n, min_freq=-1.0, max_freq=1.0):
    """S = { k : |k| < n / (2C), min_freq <= w(k) <= max_freq } in increasing k"""
    lo, hi = np.float32(min_freq), np.float32(max_freq)
    return [k for k in range(-(n // (2 * C)), n // (2 * C) + 1) if abs(k) * 2 * C < n and lo <= omega(k, C, n) <= hi]


def oracle_carrier_est(orc, frames, taps, C, n, start, min_freq=-1.0, max_freq=1.0, frames_to_check=None):
    """Steps 1-6 of the definition per frame -> dict(seed (F, 2) f32, freq (F,) f32, bin (F,) i32, line (F, 2) f64) over
    frames_to_check (default: all), in that order"""
    frames = np.asarray(frames, np.float32)
    sel = list(range(frames.shape[0])) if frames_to_check is None else list(frames_to_check)
    S = search_set(C, n, min_freq, max_freq)
    assert S, "empty search set"
    taps = np.ascontiguousarray(taps, np.float32)
    out = dict(seed=np.zeros((len(sel), 2), np.float32), freq=np.zeros(len(sel), np.float32), bin=np.zeros(len(sel), np.int32),
               line=np.zeros((len(sel), 2), np.float64))
    ks = np.array(S, np.int64)
    for i, f in enumerate(sel):
        y = np.array(frames[f, :start + n], np.float32, copy=True)
        orc.rrc_fir(taps, np.zeros((127, 2), np.float32), y)                      # 1: fresh delay line
        a = y[start:start + n, 0].astype(np.float64)
        b = y[start:start + n, 1].astype(np.float64)
        s_re = a * a - b * b                                                      # 2: fp64, unfused, in this order
        s_im = 2.0 * (a * b)
        z_re = s_re * s_re - s_im * s_im
        z_im = 2.0 * (s_re * s_im)
        X = orc.fftn(z_re + 1j * z_im)                                            # 3: fft.c:110-120 (complex construction is exact)
        Xs = X[ks % n]                                                            # 4: bin k is X[k mod n]
        P = Xs.real * Xs.real + Xs.imag * Xs.imag                                 # 5
        best = None
        for j in range(len(S)):
            if np.isnan(P[j]):
                continue
            key = (-P[j], abs(S[j]), S[j])
            if best is None or key < best[0]:
                best = (key, j)
        if best is None:                                                          # every power NaN: the member of S nearest 0
            j = min(range(len(S)), key=lambda q: (abs(S[q]), S[q]))
        else:
            j = best[1]
        k = S[j]
        w = omega(k, C, n)                                                        # 6
        out["seed"][i] = (0.0, w)
        out["freq"][i] = w
        out["bin"][i] = k
        out["line"][i] = (Xs[j].real, Xs[j].imag)
    return out


def quadrant_errors(costas, tx, C, skip=8):
    """costas_frame[] quadrant decisions against the transmitted symbols after symbol `skip`, modulo the loop's 4-fold ambiguity (the
    fewest errors over the four rotations).  Transmit and receive filters delay the signal by 126 samples, so decimated symbol j at
    offset 126 % C carries transmitted symbol j - 126 // C."""
    lag = 126 // C
    z = costas[skip + lag:, 0].astype(np.float64) + 1j * costas[skip + lag:, 1].astype(np.float64)
    q = np.floor(np.angle(z) / (np.pi / 2)).astype(np.int64) % 4                  # the quadrant: the loop locks on the diagonals
    want = np.array([0, 1, 3, 2], np.int64)[tx[skip:skip + len(z)]]               # CONSTELLATION of sigutil: 1, j, -j, -1
    return min(int(np.sum((q + r) % 4 != want)) for r in range(4))


def bin_width(C, n):
    return TAU * C / (4.0 * n)


# ------------------------------------------------------------------- ABI (fails without the feature)
def test_carrier_est_is_declared_bound_and_exported(qpsk_lib):
    from qpsk_amd.lib import API_SYMBOLS
    assert "qpsk_carrier_est_batch" in declared("qpsk_hip.h")
    assert "qpsk_carrier_est_batch" in API_SYMBOLS
    assert hasattr(qpsk_lib, "qpsk_carrier_est_batch")


def test_python_front_end_exists():
    import qpsk_amd
    assert callable(getattr(qpsk_amd.Modem, "carrier_est", None))


def test_kernel_source_is_built_and_writes_no_scalar_memory():
    src = open(os.path.join(ROOT, "qpsk_amd", "csrc", "carrier_est.hip")).read().lower()
    assert "carrier_est.o" in open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_d" + "cache_"):
        assert word not in src, word


# ------------------------------------------------------------------- properties of the restatement
def test_search_set_is_the_band_inside_the_clamp():
    for C in (4, 8):
        for n in (64, 512, 1024, 8192):
            S = search_set(C, n)
            assert S == list(range(-(n // (2 * C)) + 1, n // (2 * C)))          # |w| < pi/4 lies inside the default [-1, 1] clamp
            assert all(abs(float(omega(k, C, n))) < np.pi / 4 for k in S)
    full = search_set(8, 1024)
    narrow = search_set(8, 1024, -0.2, 0.3)
    assert set(narrow) < set(full) and narrow[0] == 1 - 17 and narrow[-1] == 24
    assert all(-0.2 <= omega(k, 8, 1024) <= 0.3 for k in narrow)
    assert search_set(8, 1024, 0.9, 1.0) == []                                    # beyond pi/4: empty (the call refuses it)


def test_zero_frame_gives_zero(oracle):
    taps = oracle.rrc_make(np.float32(19200.0), np.float32(2400.0), np.float32(0.35))
    for C, n, start in ((8, 1024, 128), (4, 64, 0)):
        r = oracle_carrier_est(oracle, np.zeros((1, 2048, 2), np.float32), taps, C, n, start)
        assert r["bin"][0] == 0 and r["freq"][0] == 0.0 and tuple(r["seed"][0]) == (0.0, 0.0)
    r = oracle_carrier_est(oracle, np.zeros((1, 2048, 2), np.float32), taps, 8, 1024, 128, min_freq=0.1, max_freq=0.5)
    assert r["bin"][0] == search_set(8, 1024, 0.1, 0.5)[0]                         # 0 outside S: the member nearest 0


def test_narrowed_clamp_narrows_the_search(oracle):
    """A line outside a narrowed clamp is not found; the estimate stays inside [min_freq, max_freq]"""
    fs, rs = 19200.0, 2400.0
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    x, _ = make_frames(2, 4096, 8, taps, fs, offset_hz=200.0, noise=0.02)
    wide = oracle_carrier_est(oracle, x, taps, 8, 1024, 128)
    true_w = TAU * 200.0 / rs
    assert np.all(np.abs(wide["freq"] - true_w) <= bin_width(8, 1024))
    narrow = oracle_carrier_est(oracle, x, taps, 8, 1024, 128, min_freq=-0.1, max_freq=0.1)
    assert np.all(np.abs(narrow["freq"]) <= 0.1)
    assert np.all(narrow["bin"] != wide["bin"])


@pytest.mark.parametrize("C,fs,L,n", [(8, 19200.0, 4096, 1024), (8, 19200.0, 16384, 2048), (4, 9600.0, 4096, 1024),
                                      (4, 9600.0, 8192, 512)])
def test_estimate_within_one_bin_over_the_range(oracle, C, fs, L, n):
    """24 seeded random offsets with |df| < 0.97 RS/8 per shape, noise 0.05: |w_hat - w_true| <= one bin"""
    rs = 2400.0
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    rng = np.random.default_rng(1000 + C * 7 + n)
    for i, df in enumerate(rng.uniform(-0.97 * rs / 8, 0.97 * rs / 8, 24)):
        x, _ = make_frames(1, L, C, taps, fs, offset_hz=float(df), base_seed=500 + i, noise=0.05)
        r = oracle_carrier_est(oracle, x, taps, C, n, 128)
        assert abs(float(r["freq"][0]) - TAU * df / rs) <= bin_width(C, n), (df, r["freq"][0])


@pytest.mark.parametrize("L,n,bw,offsets", [(1024, 512, TAU / 100.0, (150.0, 250.0)), (4096, 2048, TAU / 200.0, (150.0, 250.0))])
def test_seeded_loop_decodes_where_the_unseeded_loop_fails(oracle, L, n, bw, offsets):
    """Through the ext composition (test_rx_ext_cpu.oracle_ext) at timing offset 126 % 8: unseeded, every frame has quadrant errors
    after symbol 8; seeded with (0, w_hat), none"""
    fs, rs, C = 19200.0, 2400.0, 8
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    bw = np.float32(bw)
    for df in offsets:
        x, tx = make_frames(4, L, C, taps, fs, offset_hz=df, base_seed=77, noise=0.05)
        idx = np.full(4, 126 % C, np.int32)
        est = oracle_carrier_est(oracle, x, taps, C, n, 128)
        plain = oracle_ext(oracle, x, fs, rs, idx, None, loop_bw=bw, want_costas=True)
        seeded = oracle_ext(oracle, x, fs, rs, idx, est["seed"], loop_bw=bw, want_costas=True)
        for f in range(4):
            assert quadrant_errors(plain["costas"][f], tx[f], C) > 0, (df, f)
            assert quadrant_errors(seeded["costas"][f], tx[f], C) == 0, (df, f)
