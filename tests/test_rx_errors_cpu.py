"""The fixtures of tests/test_rx_errors_gpu.py, proved on the CPU: every "this loop stays clean" and "this loop overflows" the GPU tests rely
on is computed here through the oracle (rxerrors.py states the predicate), as are the timing indices the bad frames must get."""
import numpy as np

import rxerrors as R
from oracle.pyoracle import TAU, TIMING_FIXED, TIMING_HIST
from sigutil import bits_equal


def test_wrap_limit_is_read_from_the_kernels_header():
    assert R.wrap_limit() >= 1024                     # a limit the reference's own test signals stay far below (a few turns per step)
    assert R.LIM == R.wrap_limit() * TAU


def test_loop_gains_are_the_oracles(oracle):
    """alpha, beta of the predicate = update_gains() (costas_loop.c:76-81) for the three bandwidths of the sweep"""
    got = [R.loop_gains(oracle, bw)[0] for bw in R.SWEEP_BWS]
    for bw, alpha in zip(R.SWEEP_BWS, got):
        z, w = np.float32(np.sqrt(np.float32(2.0)) / np.float32(2.0)), np.float32(bw)
        denom = (np.float32(1.0) + np.float32(2.0) * z * w) + w * w
        assert abs(alpha - float(np.float32(4.0) * z * w / denom)) <= 1e-6 * alpha
    assert 0.017 < got[0] < 0.019 and 0.16 < got[1] < 0.17 and 0.40 < got[2] < 0.42


def test_predicate_on_ordinary_and_scaled_frames(oracle):
    """an ordinary modem frame is clean by five orders of magnitude; scaled by 1e6 it overflows; the detector restated in numpy is the
    oracle's (qo_phase_detector) on the very z_k it is applied to"""
    x = R.modem_frames(oracle, 1, seed=3)[0]
    clean, peak = R.reach(oracle, x, 6)
    assert clean < 1e-3 and peak < 1e-3 and R.stays_clean(oracle, x, 6) and not R.overflows(oracle, x, 6)
    big = (x * np.float32(1e6)).astype(np.float32)
    assert R.overflows(oracle, big, 6) and not R.stays_clean(oracle, big, 6)
    z = oracle.rx_batch(x[None], R.FS, R.RS, loop_bw=R.BW, timing_mode=TIMING_FIXED, fixed_index=6, want_costas=True)["costas"][0]
    z = np.concatenate([z, np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 0.0], [-0.0, -2.0]], np.float32)])      # sgn(0) = -1
    e = np.where(z[:, 0] > 0, 1.0, -1.0) * z[:, 1].astype(np.float64) - np.where(z[:, 1] > 0, 1.0, -1.0) * z[:, 0].astype(np.float64)
    want = np.array([oracle.lib.qo_phase_detector(float(a), float(b)) for a, b in z], np.float32)
    assert bits_equal(e.astype(np.float32), want)


def test_priming_batch_has_one_majority_index(oracle):
    p = R.priming(oracle)
    counts = np.bincount(p["index"], minlength=8)
    assert counts.sum() == 37 and np.sum(counts == counts.max()) == 1 and counts[p["g"]] == counts.max()
    # the helper's per-frame estimate (rrc_fir on a fresh delay line + the histogram scan) is what the batch call does
    assert [R.hist_index(oracle, f) for f in p["x"]] == list(p["index"])


def test_a_frame_that_overflows_at_the_guess_only(oracle):
    """the scan over theta = k pi / 64: at least one tone frame is clean at its true index t and overflows at the guess g != t, and the
    one the GPU tests take is such a frame"""
    scan = [c for c in R.tone_scan(oracle) if c]
    good = [c for c in scan if c["ok"]]
    print("theta = k pi / 64 with a clean true index and an overflowing guess: k =", [c["k"] for c in good])
    assert len(good) >= 1
    fx = R.guess_only_overflow(oracle)
    print("taken: k = %d, amplitude %.4g, true index %d (clean bound %.3f LIM), guess %d (peak %.3f LIM)" % (
        fx["k"], fx["amplitude"], fx["t"], fx["clean_t"], fx["g"], fx["peak_g"]))
    assert fx["g"] == R.priming(oracle)["g"] and fx["t"] != fx["g"]
    assert R.hist_index(oracle, fx["frame"]) == fx["t"]
    assert R.stays_clean(oracle, fx["frame"], fx["t"]) and fx["clean_t"] < 0.9
    assert R.overflows(oracle, fx["frame"], fx["g"]) and fx["peak_g"] > 1.1
    # the whole-batch oracle call the GPU test compares with sees the frame at its true index
    for F in (37, 64):
        x, positions = R.mixed_batch(oracle, F, fx["frame"])
        assert len(positions) == 4 and 0 in positions and 16 in positions and 31 in positions
        assert (F % 16 == 0) or any(p >= 16 * (F // 16) for p in positions)
        index = oracle.rx_batch(x, R.FS, R.RS, loop_bw=R.BW, timing_mode=TIMING_HIST)["index"]
        assert all(index[p] == fx["t"] for p in positions)


def test_the_same_frame_scaled_overflows_at_both_indices(oracle):
    b = R.both_overflow(oracle)
    print("scale %g: true index %d peak %.3f LIM, guess %d peak %.3f LIM" % (b["scale"], b["t"], b["peak_t"], b["g"], b["peak_g"]))
    assert R.hist_index(oracle, b["frame"]) == b["t"]
    assert R.overflows(oracle, b["frame"], b["t"]) and R.overflows(oracle, b["frame"], b["g"])
    assert max(b["peak_t"], b["peak_g"]) * R.LIM < R.SAFE_RAD


def test_bad_frames_whose_true_index_is_the_guess(oracle):
    fx = R.bad_at_the_guess(oracle)
    assert R.hist_index(oracle, fx["base"]) == fx["g"] and R.stays_clean(oracle, fx["base"], fx["g"])
    assert np.isnan(fx["nan"]).sum() == 1 and R.hist_index(oracle, fx["nan"]) == fx["g"]
    assert R.hist_index(oracle, fx["big"]) == fx["g"] and R.overflows(oracle, fx["big"], fx["g"])


def test_timing_indices_of_frames_with_a_non_finite_sample(oracle):
    """the oracle's timing functions (no loop in them: Inf is safe) give every bad frame an index, and the fixtures are ones where that
    index is worth pinning: in FFT mode a bad sample inside the estimate's window moves it off the clean frames' index"""
    xh = R.modem_frames(oracle, 16, seed=500)
    xf = R.modem_frames(oracle, 16, seed=600, delay=0, noise=0.02)
    for bad in ("nan", "inf", "-inf"):
        xb, hit = R.nonfinite_batch(xh, bad)
        assert (~np.isfinite(xb)).sum() == 2
        ih = [R.hist_index(oracle, xb[h]) for h in hit]
        assert all(0 <= i < 8 for i in ih)
        xb, hit = R.nonfinite_batch(xf, bad)
        fi = [R.fft_index(oracle, xb[h]) for h in hit]
        clean = [R.fft_index(oracle, xf[h]) for h in hit]
        print(bad, "histogram indices", ih, "FFT indices", fi, "clean", clean)
        assert clean == [126 % 8, 126 % 8]
        assert fi[0] != clean[0] and fi[1] == clean[1]      # sample 300 is inside the window of samples 2..639, sample L - 5 is not


def test_one_loop_of_a_sweep_overflows_alone(oracle):
    s = R.sweep_fixture(oracle)
    print("scale %.4g: clean bounds %s LIM, peaks %s LIM" % (s["scale"], np.round(s["clean"], 3), np.round(s["peaks"], 3)))
    f = s["x"][s["at"]]
    assert R.stays_clean(oracle, f, R.SWEEP_INDEX, R.SWEEP_BWS[0])
    assert R.overflows(oracle, f, R.SWEEP_INDEX, R.SWEEP_BWS[1]) and R.overflows(oracle, f, R.SWEEP_INDEX, R.SWEEP_BWS[2])
    for k in range(37):
        if k != s["at"]:
            assert all(R.reach(oracle, s["x"][k], R.SWEEP_INDEX, bw)[0] < 0.01 for bw in R.SWEEP_BWS)
    # the single-loop runs the predicate reads are the sweep's loops: same bits
    sweep = oracle.rx_batch_bw(s["x"], R.FS, R.RS, R.SWEEP_BWS, timing_mode=TIMING_FIXED, fixed_index=R.SWEEP_INDEX)
    for b, bw in enumerate(R.SWEEP_BWS):
        one = oracle.rx_batch(s["x"], R.FS, R.RS, loop_bw=bw, timing_mode=TIMING_FIXED, fixed_index=R.SWEEP_INDEX)
        assert bits_equal(sweep["sym"][:, b], one["sym"]) and bits_equal(sweep["phase"][:, b], one["phase"])
