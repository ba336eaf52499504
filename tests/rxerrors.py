"""Fixtures for the receive calls' error verdicts (numpy + the CPU oracle; shared by test_rx_errors_cpu.py and test_rx_errors_gpu.py).

A receive kernel fails its call with QPSK_ERR_RANGE when a Costas loop's phase goes beyond the bounded 2 pi wrap (qpsk_device.h,
phase_wrap: more than WRAP_LIMIT turns) or ends on a NaN / Inf.  The oracle has no such flag -- its phase_wrap() is unbounded -- so
whether a (frame, decimation offset, loop bandwidth) overflows is DERIVED from what the oracle does give: the de-rotated symbols z_k of
a fixed-offset run, from which the detector e_k = sgn(re) im - sgn(im) re and so every step's phase follow.

With LIM = WRAP_LIMIT * 2 pi, and |phase| <= 2 pi, |freq| <= max_freq in front of a step whose phase is
phase + (freq + beta e) + alpha e (the frequency is clamped only BEHIND the step, costas_loop.c:56-74):

  stays clean   (alpha + beta) max_k(|re_k| + |im_k|) + 2 pi + max_freq < 0.9 LIM   (|e_k| <= |re_k| + |im_k|: no step can get there;
                                                                                    by induction the GPU's z_k are the oracle's)
  overflows     alpha |e_k| > 1.1 LIM for some k   (the first such step overflows on the GPU too: anything earlier that differed from the
                                                    oracle could only be an earlier overflow)

What lies between is not a fixture.  0.9 and 1.1 keep float rounding of the bound itself out of the question (2 pi + max_freq + beta |e| is
0.03 % of LIM against the 10 % margin): they are conditions on the fixtures, not tolerances on a kernel.

The oracle's loop must never see +-Inf nor a phase near 2^27 rad (it would not return): reach() refuses such frames.
"""
import ctypes as C
import os
import re

import numpy as np

from oracle.pyoracle import Costas, TAU, TIMING_FIXED, TIMING_HIST
from sigutil import make_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, RS, L, CYCLES = 19200.0, 2400.0, 1024, 8      # 128 symbols: the smallest frame the one-pass histogram route takes
BW = np.float32(TAU / 100.0)
MIN_FREQ, MAX_FREQ = -1.0, 1.0
SAFE_RAD = 1e7                                    # the oracle's unbounded wrap terminates well below 2^27 rad; stay an order under it
SWEEP_BWS = [np.float32(TAU / 1000.0), np.float32(TAU / 100.0), np.float32(3.0 * TAU / 100.0)]
SWEEP_INDEX = 6


def wrap_limit():
    """WRAP_LIMIT as the kernels compile it"""
    with open(os.path.join(ROOT, "qpsk_amd", "csrc", "qpsk_device.h")) as f:
        m = re.search(r"constexpr\s+int\s+WRAP_LIMIT\s*=\s*(\d+)\s*;", f.read())
    assert m, "WRAP_LIMIT not found in qpsk_device.h"
    return int(m.group(1))


LIM = wrap_limit() * TAU


def loop_gains(oracle, bw=BW):
    c = Costas()
    oracle.lib.qo_costas_create(C.byref(c), float(bw), MIN_FREQ, MAX_FREQ)
    return float(c.alpha), float(c.beta)


def taps_of(oracle):
    return oracle.rrc_make(FS, RS, 0.35)


def reach(oracle, frame, index, bw=BW):
    """One frame through the oracle's loop at a fixed decimation offset -> (clean, peak), both in units of LIM:
    clean = the bound no step's phase can exceed, peak = the largest alpha |e_k| (see the module docstring)."""
    frame = np.ascontiguousarray(frame, np.float32)
    assert np.isfinite(frame).all() and float(np.abs(frame).max()) < SAFE_RAD, "not a frame the oracle's unbounded wrap may see"
    out = oracle.rx_batch(frame[None], FS, RS, loop_bw=bw, min_freq=MIN_FREQ, max_freq=MAX_FREQ, timing_mode=TIMING_FIXED,
                          fixed_index=int(index), want_costas=True)
    z = out["costas"][0].astype(np.float64)
    re_, im_ = z[:, 0], z[:, 1]
    e = np.where(re_ > 0.0, 1.0, -1.0) * im_ - np.where(im_ > 0.0, 1.0, -1.0) * re_       # qo_phase_detector: sgn(0) = -1
    alpha, beta = loop_gains(oracle, bw)
    reach_sum = float(np.max(np.abs(re_) + np.abs(im_)))
    assert alpha * reach_sum < SAFE_RAD
    return ((alpha + beta) * reach_sum + TAU + MAX_FREQ) / LIM, alpha * float(np.max(np.abs(e))) / LIM


def stays_clean(oracle, frame, index, bw=BW):
    return reach(oracle, frame, index, bw)[0] < 0.9


def overflows(oracle, frame, index, bw=BW):
    return reach(oracle, frame, index, bw)[1] > 1.1


def hist_index(oracle, frame):
    """the reference's histogram timing estimate of one frame on a fresh delay line (no loop: safe on NaN / Inf)"""
    y = np.array(frame, np.float32, copy=True)
    oracle.rrc_fir(taps_of(oracle), np.zeros((127, 2), np.float32), y)
    return int(oracle.timing_hist(y, CYCLES)[0])


def fft_index(oracle, frame, frame_size=L):
    """the FFT timing estimate of one frame (no loop: safe on NaN / Inf)"""
    assert frame.shape[0] == frame_size
    return int(oracle.timing_fft_index(taps_of(oracle), np.ascontiguousarray(frame, np.float32), CYCLES))


def modem_frames(oracle, F, seed, delay=6, noise=0.0, offset_hz=40.0):
    """noise-free modem frames cut at `delay` from frames eight samples longer (the delay moves the histogram index)"""
    x, _ = make_frames(F, L + 8, CYCLES, taps_of(oracle), FS, offset_hz=offset_hz, base_seed=seed, noise=noise)
    return np.ascontiguousarray(x[:, delay:delay + L])


def majority(index):
    """index_majority_kernel's rule: the first maximum of the eight counts"""
    return int(np.bincount(np.asarray(index) & 7, minlength=8).argmax())


def tone_frame(amplitude, theta):
    """a tone at rs / 2 under a raised-cosine ramp of 256 samples at either end (band-limited): I = A s, Q = 0.37 A s.  Filtered, it
    crosses zero at one sample phase and peaks four samples away -- and the histogram index, a bin of envelope statistics, does not
    follow the peak: a frame whose loop is tame at its true index and violent at another"""
    n = np.arange(L, dtype=np.float64)
    env = np.ones(L)
    ramp = 0.5 * (1.0 - np.cos(np.pi * np.arange(256) / 256.0))
    env[:256] = ramp
    env[-256:] = ramp[::-1]
    s = env * np.cos(np.pi * n / 8.0 + theta)
    x = np.zeros((L, 2), np.float32)
    x[:, 0] = (amplitude * s).astype(np.float32)
    x[:, 1] = (0.37 * amplitude * s).astype(np.float32)
    return x


_cache = {}


def _cached(fn):
    def wrapper(oracle):
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn(oracle)
        return _cache[fn.__name__]
    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


@_cached
def priming(oracle):
    """the batch that leaves the guess: 37 noise-free modem frames -> dict(x, index (the oracle's), g (their one majority index))"""
    x = modem_frames(oracle, 37, seed=1234)
    index = oracle.rx_batch(x, FS, RS, loop_bw=BW, timing_mode=TIMING_HIST)["index"]
    counts = np.bincount(index, minlength=8)
    assert np.sum(counts == counts.max()) == 1, "the priming batch has no single majority index: %s" % counts
    return dict(x=x, index=index, g=majority(index))


def _tone_candidate(oracle, k, g):
    """theta = k pi / 64 -> the fixture's facts at the amplitude that puts the true index's clean bound at about half of LIM, or None"""
    theta = k * np.pi / 64.0
    unit = tone_frame(1.0, theta)
    t = hist_index(oracle, unit)
    # |z_k| is the decimated sample's magnitude, so the reach scales with the amplitude: measured at amplitude 1, set to LIM / 2
    unit_clean = reach(oracle, unit, t)[0] * LIM - TAU - MAX_FREQ
    if unit_clean <= 0.0:
        return None
    amplitude = 0.5 * LIM / unit_clean
    frame = tone_frame(amplitude, theta)
    if hist_index(oracle, frame) != t:
        return None
    clean_t, peak_t = reach(oracle, frame, t)
    clean_g, peak_g = reach(oracle, frame, g)
    return dict(k=k, theta=theta, amplitude=amplitude, frame=frame, t=t, g=g, clean_t=clean_t, peak_t=peak_t, clean_g=clean_g, peak_g=peak_g,
                ok=bool(t != g and clean_t < 0.9 and peak_g > 1.1))


@_cached
def tone_scan(oracle):
    """every theta = k pi / 64, k = 0..127, through the oracle -> the list of candidates (None where the amplitude changes the index)"""
    g = priming(oracle)["g"]
    return [_tone_candidate(oracle, k, g) for k in range(128)]


@_cached
def guess_only_overflow(oracle):
    """THE fixture of the one-pass route's defect: a frame whose loop stays clean at its true index t and overflows at the priming
    batch's majority index g != t (the first theta of the scan that gives both) -> the candidate's dict"""
    found = [c for c in tone_scan(oracle) if c and c["ok"]]
    assert found, "no theta = k pi / 64 gives a frame that is clean at its true index and overflows at the guess"
    return found[0]


@_cached
def both_overflow(oracle):
    """the same frame scaled until its true index overflows as well (and every phase stays below SAFE_RAD: the oracle terminates)
    -> dict(frame, scale, t, g, peak_t, peak_g)"""
    fx = guess_only_overflow(oracle)
    for scale in (8.0, 16.0, 32.0):
        frame = tone_frame(fx["amplitude"] * scale, fx["theta"])
        t = hist_index(oracle, frame)
        peak_t, peak_g = reach(oracle, frame, t)[1], reach(oracle, frame, fx["g"])[1]
        if peak_t > 1.1 and peak_g > 1.1:
            return dict(frame=frame, scale=scale, t=t, g=fx["g"], peak_t=peak_t, peak_g=peak_g)
    raise AssertionError("no scale up to 32 makes the true index overflow")


def mixed_batch(oracle, F, special, seed=500):
    """F clean modem frames with `special` at the first frame of a workgroup, the last frame of a workgroup, inside the ragged tail
    (where F is no multiple of 16) and at frame 0 -> (x, positions)"""
    x = modem_frames(oracle, F, seed=seed)
    positions = sorted({0, 16, 31, F - 3 if F % 16 else F - 1})
    for p in positions:
        x[p] = special
    return x, positions


@_cached
def bad_at_the_guess(oracle):
    """frames whose TRUE index equals the guess g and whose loop must fail there: a NaN sample (placed where the histogram index
    stays g), and an ordinary frame scaled until the loop at g overflows -> dict(g, base (the clean frame), nan, nan_at, big, big_peak)"""
    g = priming(oracle)["g"]
    base = modem_frames(oracle, 1, seed=900)[0]
    assert hist_index(oracle, base) == g
    nan, nan_at = None, None
    for at in (L - 5, L - 200, 300, 100):
        cand = base.copy()
        cand[at, 0] = np.float32("nan")
        if hist_index(oracle, cand) == g:
            nan, nan_at = cand, at
            break
    assert nan is not None, "every NaN position tried moves the histogram index off the guess"
    big = None
    for scale in (3e5, 1e6):
        cand = (base * np.float32(scale)).astype(np.float32)
        if hist_index(oracle, cand) == g and reach(oracle, cand, g)[1] > 1.1:
            big = cand
            break
    assert big is not None, "no scale up to 1e6 makes the loop at the guess overflow"
    return dict(g=g, base=base, nan=nan, nan_at=nan_at, big=big, big_peak=reach(oracle, big, g)[1])


def nonfinite_batch(x, bad):
    """a copy of x with `bad` at sample 300 of frame 3 (inside the FFT estimate's window of samples 2..639, I component) and at sample
    L - 5 of frame F // 2 + 1 (outside it, Q component) -> (xb, hit frames)"""
    F, n = x.shape[0], x.shape[1]
    hit = [3, F // 2 + 1]
    assert hit[0] != hit[1] and hit[1] < F
    xb = x.copy()
    xb[hit[0], 300, 0] = np.float32(bad)
    xb[hit[1], n - 5, 1] = np.float32(bad)
    return xb, hit


@_cached
def sweep_fixture(oracle):
    """a bandwidth sweep in which ONE loop of one frame stays clean while its two neighbours on the same frame overflow: an ordinary
    frame scaled so that the lowest bandwidth's clean bound sits at about 0.45 LIM -> dict(x (37 frames), at, scale, clean, peaks)"""
    x, _ = make_frames(37, L, CYCLES, taps_of(oracle), FS, offset_hz=20.0, base_seed=77, noise=0.02)
    at = 17
    unit_clean = reach(oracle, x[at], SWEEP_INDEX, SWEEP_BWS[0])[0] * LIM - TAU - MAX_FREQ
    scale = 0.45 * LIM / unit_clean
    x[at] = (x[at] * np.float32(scale)).astype(np.float32)
    r = [reach(oracle, x[at], SWEEP_INDEX, bw) for bw in SWEEP_BWS]
    return dict(x=x, at=at, scale=scale, clean=[c for c, _ in r], peaks=[p for _, p in r])
