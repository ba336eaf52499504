"""The receive calls' error verdicts outside TIMING_FIXED: a call with a bad frame returns, fails with QPSK_ERR_RANGE (-6) at the next
synchronisation, and every other frame of the call still carries the oracle's bits (include/qpsk_hip.h) -- on both histogram routes, on
the three placements of the FFT estimate and for one loop of a bandwidth sweep.  The fixtures and the proof that each one's loop
overflows / stays clean where the tests say so are in rxerrors.py and test_rx_errors_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import rxerrors as R
from oracle.pyoracle import TIMING_FFT, TIMING_FIXED, TIMING_HIST
from sigutil import bits_equal

pytestmark = pytest.mark.gpu

ONEPASS = "rx_hist_kernel (one pass on the guessed index) + rx_fused_kernel (fall-back list)"
INLINE = " (FFT timing estimate inside the launch)"
KEYS = ("sym", "phase", "freq", "index", "hz")


def modem(mode, **kw):
    import qpsk_amd
    return qpsk_amd.Modem(fs=R.FS, rs=R.RS, frame_size=R.L, loop_bw=R.BW, min_freq=R.MIN_FREQ, max_freq=R.MAX_FREQ, timing_mode=mode, **kw)


def cpu(t):
    return t.cpu().numpy()


def sync_fails_with_range_error(m):
    import qpsk_amd
    with pytest.raises(qpsk_amd.QpskError, match="-6"):
        m.sync()


def hist_state(m):
    """[the guess the next call takes, misses not yet counted, majority, frames, frames off the majority or missed] (synchronises)"""
    st = (C.c_int32 * 5)()
    m._check(m.L.qpsk_test_hist_state(m.h, st))
    return list(st)


def assert_rows_equal(got, want, rows, keys=KEYS, what=""):
    for k in keys:
        g = cpu(got[k])[rows]
        w = np.asarray(want[k] if isinstance(want[k], np.ndarray) else cpu(want[k]))[rows].astype(g.dtype)
        assert bits_equal(g, w), "%s%s differs in %d elements" % (what, k, int(np.sum(g != w)))


def primed_onepass_modem(oracle):
    """a histogram-mode context whose guess is the priming batch's majority index, with the one-pass route forced"""
    prime = R.priming(oracle)
    m = modem(TIMING_HIST)
    got = m.rx_batch(prime["x"])
    m.sync()
    assert m.last_kernel() != ONEPASS                 # no guess yet: two launches
    assert bits_equal(cpu(got["index"]), prime["index"])
    assert hist_state(m)[0] == prime["g"]
    m.tune(hist_onepass=1)
    return m


def hist_oracle(oracle, x):
    return oracle.rx_batch(x, R.FS, R.RS, loop_bw=R.BW, min_freq=R.MIN_FREQ, max_freq=R.MAX_FREQ, timing_mode=TIMING_HIST)


# ------------------------------------------------------------------ 3. the one-pass histogram route
@pytest.mark.parametrize("F", [37, 64])
def test_return_code_does_not_depend_on_the_route(oracle, F):
    """A frame whose loop overflows at the GUESSED index but is clean at its true one (rxerrors.guess_only_overflow) at the first and the
    last frame of a workgroup, in the ragged tail and at frame 0.  rx_hist_kernel's serial wave runs it on the guess, the scan wave then
    puts it on the list and the fall-back pass redoes it at its true index: the call is as good as the two-launch route's, so it returns
    what that returns -- OK -- with the same bits.  (Until the flags of the run on the guess were held back per frame, the one-pass call
    failed with -6 here: seen on the parent commit.)"""
    fx = R.guess_only_overflow(oracle)
    x, positions = R.mixed_batch(oracle, F, fx["frame"])
    want = hist_oracle(oracle, x)
    assert all(want["index"][p] == fx["t"] for p in positions)
    m1 = modem(TIMING_HIST)
    m1.tune(hist_onepass=0)
    got1 = m1.rx_batch(x)
    m1.sync()
    assert m1.last_kernel() != ONEPASS
    assert_rows_equal(got1, want, slice(None))
    m2 = primed_onepass_modem(oracle)
    got2 = m2.rx_batch(x)
    assert m2.last_kernel() == ONEPASS
    m2.sync()
    assert_rows_equal(got2, got1, slice(None), what="one-pass route against the two-launch route: ")
    st = hist_state(m2)
    missed = int(np.sum(want["index"] != fx["g"]))
    assert missed >= len(positions)
    assert st[0] == R.majority(want["index"]) and st[1] == 0 and st[3] == F and st[4] == max(missed, F - int(np.sum(want["index"] == st[0])))


@pytest.mark.parametrize("F", [37, 64])
def test_overflow_at_the_true_index_fails_on_both_routes(oracle, F):
    """the same frame scaled until its loop overflows at the true index too: both routes fail with -6 (on the one-pass route through
    the fall-back pass: the true index is not the guess), every other frame equals the oracle, every index does, and the next clean call
    on the context is fine -- on the one-pass route"""
    b = R.both_overflow(oracle)
    x, positions = R.mixed_batch(oracle, F, b["frame"])
    others = [f for f in range(F) if f not in positions]
    want = hist_oracle(oracle, x)                     # (terminates: every phase below rxerrors.SAFE_RAD)
    assert all(want["index"][p] == b["t"] for p in positions) and b["t"] != b["g"]
    xc = R.modem_frames(oracle, F, seed=501)
    wantc = hist_oracle(oracle, xc)
    m1 = modem(TIMING_HIST)
    m1.tune(hist_onepass=0)
    m2 = primed_onepass_modem(oracle)
    for m, onepass in ((m1, False), (m2, True)):
        got = m.rx_batch(x)
        assert (m.last_kernel() == ONEPASS) == onepass
        sync_fails_with_range_error(m)
        assert_rows_equal(got, want, others)
        assert_rows_equal(got, want, slice(None), keys=("index",))
        got = m.rx_batch(xc)
        assert (m.last_kernel() == ONEPASS) == onepass
        m.sync()                                      # the failed synchronisation cleared the flag
        assert_rows_equal(got, wantc, slice(None))


@pytest.mark.parametrize("F", [37, 64])
@pytest.mark.parametrize("kind", ["nan", "big"])
def test_bad_frame_at_the_guessed_index_is_still_an_error(oracle, kind, F):
    """frames whose TRUE index is the guess -- the run on the guess is their result, nothing redoes them -- with a NaN sample, or scaled
    until the loop at that index overflows: the flags held back for the run on the guess must still fail the call, on both routes"""
    fx = R.bad_at_the_guess(oracle)
    x, positions = R.mixed_batch(oracle, F, fx["base"])
    want = hist_oracle(oracle, x)                     # the clean batch: the bad frames' indices are the base frame's (test_rx_errors_cpu)
    assert all(want["index"][p] == fx["g"] for p in positions)
    xb = x.copy()
    xb[positions] = fx[kind]
    others = [f for f in range(F) if f not in positions]
    m1 = modem(TIMING_HIST)
    m1.tune(hist_onepass=0)
    m2 = primed_onepass_modem(oracle)
    for m, onepass in ((m1, False), (m2, True)):
        got = m.rx_batch(xb)
        assert (m.last_kernel() == ONEPASS) == onepass
        sync_fails_with_range_error(m)
        assert_rows_equal(got, want, others)
        assert_rows_equal(got, want, slice(None), keys=("index",))
        got = m.rx_batch(x)
        assert (m.last_kernel() == ONEPASS) == onepass
        m.sync()
        assert_rows_equal(got, want, slice(None))


# ------------------------------------------------------------------ 4. non-finite input on the histogram and FFT routes
# F: the smallest whole workgroup of the named kernel (16 frames: rx_hist_kernel, rx_fused_pipe_kernel with four FIR waves; 8: rx_lean_kernel
# under QPSK_PIPE_G = 8) and a ragged size.  The in-launch FFT routes are reached with test_fft_timing_under_every_geometry_key's keys
ROUTES = {
    "hist_two_launch": dict(mode=TIMING_HIST, tune=dict(hist_onepass=0), kernel="rx_fused_pipe_kernel"),
    "hist_one_pass": dict(mode=TIMING_HIST, tune=dict(), kernel=ONEPASS),
    "fft_in_front": dict(mode=TIMING_FFT, tune=dict(fft_fused=0), kernel="rx_fused_pipe_kernel"),
    "fft_in_fused_pipe": dict(mode=TIMING_FFT, tune=dict(pipe_v=1, pipe_nf=4), kernel="rx_fused_pipe_kernel" + INLINE),
    "fft_in_lean": dict(mode=TIMING_FFT, tune=dict(pipe_g=8), kernel="rx_lean_kernel" + INLINE),
}
ROUTE_CASES = [(r, F) for r in ROUTES for F in ((8, 21) if r == "fft_in_lean" else (16, 37))]


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
@pytest.mark.parametrize("route,F", ROUTE_CASES)
def test_nonfinite_input_on_histogram_and_fft_routes(oracle, route, F, bad):
    """a NaN / Inf sample in two frames (sample 300: inside the FFT estimate's window; sample L - 5: outside it): the call returns and
    fails with -6; every frame without one equals the oracle, the index included; a bad frame's INDEX is what the oracle's timing
    function gives for that frame alone (on the one-pass route it goes into the next call's guess); the next clean call is fine"""
    r = ROUTES[route]
    hist = r["mode"] == TIMING_HIST
    x = R.modem_frames(oracle, F, seed=500) if hist else R.modem_frames(oracle, F, seed=600, delay=0, noise=0.02)
    want = oracle.rx_batch(x, R.FS, R.RS, loop_bw=R.BW, timing_mode=r["mode"])
    xb, hit = R.nonfinite_batch(x, bad)
    index = want["index"].copy()
    index[hit] = [R.hist_index(oracle, xb[h]) if hist else R.fft_index(oracle, xb[h]) for h in hit]
    clean = [f for f in range(F) if f not in hit]
    m = primed_onepass_modem(oracle) if route == "hist_one_pass" else modem(r["mode"])
    m.tune(**r["tune"])
    guess = hist_state(m)[0]
    got = m.rx_batch(xb)
    assert m.last_kernel() == r["kernel"], m.last_kernel()
    sync_fails_with_range_error(m)
    assert_rows_equal(got, want, clean)
    assert bits_equal(cpu(got["index"]), index), (cpu(got["index"])[hit], index[hit])
    if route == "hist_one_pass":
        st = hist_state(m)
        maj = R.majority(index)
        missed = int(np.sum(index != guess))
        assert st == [maj, 0, maj, F, max(missed, F - int(np.sum(index == maj)))], st
    got = m.rx_batch(x)
    assert m.last_kernel() == r["kernel"], m.last_kernel()
    m.sync()
    assert_rows_equal(got, want, slice(None))


# ------------------------------------------------------------------ 5. one loop of a bandwidth sweep overflows alone
@pytest.mark.parametrize("pipe_v,pipe_g,kernel", [(1, None, "rx_fused_pipe_kernel"), (2, None, "rx_pipe2_kernel"), (2, 7, "rx_pipe2_kernel")])
def test_one_loop_of_a_sweep_overflows_alone(oracle, pipe_v, pipe_g, kernel):
    """one lane of the serial wave per (frame, loop): of three bandwidths on one scaled frame the two higher overflow, the lowest stays
    clean (test_rx_errors_cpu).  The call fails with -6; every loop of every other frame, and the scaled frame's lowest-bandwidth loop,
    equal the oracle"""
    s = R.sweep_fixture(oracle)
    x, at = s["x"], s["at"]
    want = oracle.rx_batch_bw(x, R.FS, R.RS, R.SWEEP_BWS, timing_mode=TIMING_FIXED, fixed_index=R.SWEEP_INDEX)
    m = modem(TIMING_FIXED, fixed_index=R.SWEEP_INDEX)
    m.tune(pipe_v=pipe_v, pipe_g=pipe_g)
    got = m.rx_batch_bw(x, R.SWEEP_BWS)
    assert m.last_kernel() == kernel, m.last_kernel()
    sync_fails_with_range_error(m)
    others = [f for f in range(x.shape[0]) if f != at]
    assert_rows_equal(got, want, others, keys=("sym", "phase", "freq"))
    for k in ("sym", "phase", "freq"):
        assert bits_equal(cpu(got[k])[at, 0], want[k][at, 0]), "the scaled frame's lowest-bandwidth loop: %s" % k
