"""Batched receive with the acquisition from outside (qpsk_rx_batch_ext): what can be checked without a GPU.

The ext call is defined per frame as a composition of reference code -- rx_frame(frame) with the caller's index at qpsk.c:190,
set_phase() / set_frequency() (costas_loop.c:117-132), rx_frame(zeros) -- and oracle_ext() below is that composition on the
oracle.  The `ref` test pins it to the compiled reference's real setters; the GPU tests (test_rx_ext_gpu.py) compare against it.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.pyoracle import TAU, TIMING_FIXED, TIMING_HIST, OracleModem, ref_available
from sigutil import bits_equal, make_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_SYMBOLS = ("qpsk_rx_batch_ext", "qpsk_rx_batch_bw_ext", "qpsk_multi_set_acquisition")


def oracle_ext(orc, frames, fs, rs, index, seed=None, loop_bw=np.float32(TAU / 100.0), min_freq=-1.0, max_freq=1.0,
               want_costas=False, frames_to_check=None):
    """Per frame: a fresh TIMING_FIXED OracleModem with fixed_index = index[f]; rx_cplx(frame); the loop state written and put
    through qo_phase_wrap / qo_frequency_limit (set_phase / set_frequency); rx_cplx(zeros).  -> dict(sym, freq, phase, index, hz
    [, costas]) over frames_to_check (default: all), in that order."""
    frames = np.ascontiguousarray(frames, np.float32)
    F, L = frames.shape[0], frames.shape[1]
    sel = list(range(F)) if frames_to_check is None else list(frames_to_check)
    nsym = L // int(fs / rs)
    out = dict(sym=np.zeros((len(sel), nsym), np.uint8), freq=np.zeros(len(sel), np.float32),
               phase=np.zeros(len(sel), np.float32), index=np.zeros(len(sel), np.int32), hz=np.zeros(len(sel), np.float32))
    if want_costas:
        out["costas"] = np.zeros((len(sel), nsym, 2), np.float32)
    zeros = np.zeros((L, 2), np.float32)
    modems = {}
    for i, f in enumerate(sel):
        k = int(index[f])
        m = modems.get(k)
        if m is None:
            m = modems[k] = OracleModem(orc, fs, rs, L, loop_bw=loop_bw, min_freq=min_freq, max_freq=max_freq,
                                        timing_mode=TIMING_FIXED, fixed_index=k)
        m.reset()
        m.rx_cplx(frames[f])
        if seed is not None:
            m.s.loop.phase = float(seed[f][0])
            m.s.loop.freq = float(seed[f][1])
            orc.lib.qo_phase_wrap(C.byref(m.s.loop))
            orc.lib.qo_frequency_limit(C.byref(m.s.loop))
        m.rx_cplx(zeros)
        out["sym"][i] = m.symbols
        out["freq"][i] = m.freq
        out["phase"][i] = m.phase
        out["index"][i] = k
        out["hz"][i] = m.offset_hz
        if want_costas:
            out["costas"][i] = m.costas_frame
    return out


def declared(header):
    import re
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(qpsk_\w+)\s*\(", text))


def test_ext_entry_points_are_declared_bound_and_exported(qpsk_lib):
    from qpsk_amd.lib import API_SYMBOLS
    for name in EXT_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name


def test_python_front_ends_exist():
    import qpsk_amd
    for name in ("rx_batch_ext", "rx_batch_bw_ext"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    assert callable(getattr(qpsk_amd.MultiJob, "set_acquisition", None))


def test_oracle_composition_with_zero_seed_is_the_fixed_batch(oracle):
    """A zero seed (or none) leaves the composition equal to the oracle's own fixed-index batch, for every index"""
    fs, rs, L = 19200.0, 2400.0, 1024
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    x, _ = make_frames(16, L, 8, taps, fs, offset_hz=40.0, noise=0.05)
    idx = np.arange(16, dtype=np.int32) % 8
    for seed in (None, np.zeros((16, 2), np.float32)):
        got = oracle_ext(oracle, x, fs, rs, idx, seed)
        for k in range(8):
            rows = np.nonzero(idx == k)[0]
            want = oracle.rx_batch(x[rows], fs, rs, timing_mode=TIMING_FIXED, fixed_index=k)
            for key in ("sym", "freq", "phase", "hz"):
                assert bits_equal(got[key][rows], want[key]), (k, key)


def test_oracle_seed_wraps_and_clamps_like_the_setters(oracle):
    """The seed goes through phase_wrap (float against the double 2 pi) and the [min, max] clamp before the second call"""
    from oracle.pyoracle import Costas
    c = Costas()
    oracle.lib.qo_costas_create(C.byref(c), np.float32(TAU / 100.0), -1.0, 1.0)
    for p, f in [(9.5, 1.5), (-9.5, -2.0), (3.0, 0.25), (-0.0, -0.0), (20.0, 0.0)]:
        c.phase, c.freq = p, f
        oracle.lib.qo_phase_wrap(C.byref(c))
        oracle.lib.qo_frequency_limit(C.byref(c))
        q = np.float32(p)
        while q > TAU:
            q = np.float32(np.float64(q) - TAU)
        while q < -TAU:
            q = np.float32(np.float64(q) + TAU)
        assert bits_equal(np.float32(c.phase), q)
        assert bits_equal(np.float32(c.freq), np.float32(min(max(f, -1.0), 1.0)) if f != 0.0 else np.float32(f))


@pytest.mark.ref
@pytest.mark.skipif(not ref_available("shipped"), reason="oracle/_ref not built (needs the reference sources)")
def test_oracle_composition_matches_the_reference_setters(oracle):
    """oracle_ext() against the reference itself: rx_frame(frame); set_phase(); set_frequency(); rx_frame(zeros) on a fresh
    process state.  The reference has no fixed index, so each frame's index is the one its histogram picks (the oracle's
    histogram equals the reference's: test_oracle_vs_ref.py), fed to the composition as a fixed index."""
    from oracle.pyoracle import Reference
    ref = Reference("shipped")
    fs, rs, L = ref.fs, ref.rs, ref.frame_size
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    x, _ = make_frames(6, L, ref.cycles, taps, fs, offset_hz=50.0, noise=0.05)
    x[5, 100:300] = 0.0
    seeds = np.array([[9.3, 0.4], [-8.1, 1.7], [-0.0, -0.0], [0.0, -0.0], [2.5, -3.0], [-4.0, 0.05]], np.float32)
    hist = OracleModem(oracle, fs, rs, L, timing_mode=TIMING_HIST)
    idx = np.zeros(6, np.int32)
    for f in range(6):
        hist.reset()
        hist.rx_cplx(x[f])
        idx[f] = hist.index
    got = oracle_ext(oracle, x, fs, rs, idx, seeds, want_costas=True)
    zeros = np.zeros((L, 2), np.float32)
    for f in range(6):
        ref.reset()
        ref.rx_cplx(x[f])
        ref.lib.set_phase(seeds[f, 0])
        ref.lib.set_frequency(seeds[f, 1])
        ref.rx_cplx(zeros)
        assert bits_equal(ref.phase, got["phase"][f]), f
        assert bits_equal(ref.freq, got["freq"][f]), f
        assert bits_equal(ref.symbols, got["sym"][f]), f
        assert bits_equal(ref.costas_frame, got["costas"][f]), f
        assert bits_equal(ref.offset_hz, got["hz"][f]), f
