"""The serial wave's ring stream in chunk-long groups (costas_asm.h, costas_asm_run_ring*: one group = one 64-symbol ring chunk):
entry, hand-over and exit at every chunk count, every stream build (one lane per loop, paired lanes, rx_hist_kernel's low-register
copy), and every way out of a group -- a 2 pi wrap at each of the 64 step positions and in the tail, an abandoned chunk (exact-zero
detector input, the double-wrap flag), lanes excused from the zero test, a first chunk kept away from the stream.  Everything is
compared with the oracle bit for bit: symbols, frequency, phase."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TAU, TIMING_FIXED, TIMING_HIST, Costas
from sigutil import bits_equal, make_frames
from test_rx_ext_cpu import oracle_ext

pytestmark = pytest.mark.gpu

FS, RS, CYCLES = 19200.0, 2400.0, 8
BW = np.float32(TAU / 100.0)
INDEX = 6
CHUNK = 64                                   # symbols per ring chunk = steps per group of the ring stream
LEAN = "rx_lean_kernel"
KEYS = ("sym", "freq", "phase")
# frames per workgroup, lean_pair: one workgroup of 8 on either stream, 32 per workgroup = every lane of the one-lane stream busy
STREAMS = [(8, 0), (8, 1), (32, 0)]


def cpu(t):
    return t.cpu().numpy()


def lean_modem(L, G, pair, **kw):
    import qpsk_amd
    m = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_FIXED, fixed_index=INDEX, **kw)
    m.tune(pipe_v=3, pipe_g=G, lean_pair=pair)
    return m


def assert_equal(got, want, what):
    for k in KEYS:
        g = cpu(got[k])
        w = np.asarray(want[k]).astype(g.dtype)
        assert bits_equal(g, w), "%s: %s differs in %d elements (first frame %d)" % (
            what, k, int(np.sum(g != w)), int(np.argwhere((g != w).reshape(len(g), -1).any(axis=1))[0, 0]))


def run_lean(x, want, G, pair, what):
    m = lean_modem(x.shape[1], G, pair)
    try:
        got = m.rx_batch(x)
        m.sync()
        assert m.last_kernel().startswith(LEAN), m.last_kernel()
        assert_equal(got, want, "%s, %d frames per workgroup, lean_pair %d" % (what, G, pair))
    finally:
        m.close()


def fixed_oracle(oracle, x):
    return oracle.rx_batch(x, FS, RS, loop_bw=BW, timing_mode=TIMING_FIXED, fixed_index=INDEX, want_costas=True)


def taps(oracle):
    return oracle.rrc_make(FS, RS, np.float32(0.35))


def loop_trace(oracle, frame):
    """One frame through the oracle's filter and loop, step by step -> (phase after each step, final (phase, freq))"""
    y = np.array(frame, np.float32, copy=True)
    oracle.rrc_fir(taps(oracle), np.zeros((127, 2), np.float32), y)
    d = y[INDEX::CYCLES]
    c = Costas()
    oracle.lib.qo_costas_create(C.byref(c), BW, -1.0, 1.0)
    zr, zi = C.c_float(), C.c_float()
    ph = np.empty(len(d), np.float64)
    for i in range(len(d)):
        oracle.lib.qo_costas_step(C.byref(c), float(d[i, 0]), float(d[i, 1]), C.byref(zr), C.byref(zi))
        ph[i] = c.phase
    return ph, (np.float32(c.phase), np.float32(c.freq))


# ------------------------------------------------------------------ shapes
@pytest.fixture(scope="module")
def shape_batches(oracle):
    """per frame size: 64 noisy modem frames and the oracle's results (computed once; the smaller batches are its first frames)"""
    out = {}
    for L in (1024, 1536, 2048):
        x, _ = make_frames(64, L, CYCLES, taps(oracle), FS, offset_hz=50.0, base_seed=7000 + L, noise=0.02)
        out[L] = (x, fixed_oracle(oracle, x))
    return out


def first(want, n):
    return {k: v[:n] for k, v in want.items()}


@pytest.mark.parametrize("L", [1024, 1536, 2048])
@pytest.mark.parametrize("G,pair", [(8, 0), (8, 1)])
def test_one_workgroup_of_eight(shape_batches, L, G, pair):
    """128 symbols: entry, one hand-over, the exit at kend; 192: an odd chunk count; 256: the two-chunk ring round twice"""
    x, want = shape_batches[L]
    run_lean(x[:8], first(want, 8), G, pair, "%d symbols" % (L // CYCLES))


@pytest.mark.parametrize("L", [1024, 1536, 2048])
def test_every_lane_of_the_one_lane_stream(shape_batches, L):
    x, want = shape_batches[L]
    run_lean(x, want, 32, 0, "%d symbols, 64 frames" % (L // CYCLES))


@pytest.mark.parametrize("L", [1024, 1536, 2048])
@pytest.mark.parametrize("G,pair", STREAMS)
def test_ragged_batch_of_nine(shape_batches, L, G, pair):
    x, want = shape_batches[L]
    run_lean(x[:9], first(want, 9), G, pair, "%d symbols, 9 frames" % (L // CYCLES))


def test_histogram_mode_runs_the_low_register_copy(oracle):
    """16 frames in histogram timing mode: once a first call has left a guess, rx_hist_kernel serves the batch (its serial wave runs
    costas_asm_lo.h's copy of the stream)"""
    import qpsk_amd
    L = 2048
    x, _ = make_frames(16, L, CYCLES, taps(oracle), FS, offset_hz=-35.0, base_seed=4242, noise=0.02)
    want = oracle.rx_batch(x, FS, RS, loop_bw=BW, timing_mode=TIMING_HIST)
    m = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_HIST)
    try:
        got = m.rx_batch(x)
        m.sync()
        assert_equal(got, want, "histogram mode, first call")
        m.tune(hist_onepass=1)
        got = m.rx_batch(x)
        m.sync()
        assert m.last_kernel().startswith("rx_hist_kernel"), m.last_kernel()
        assert_equal(got, want, "histogram mode, rx_hist_kernel")
        assert bits_equal(cpu(got["index"]), want["index"])
    finally:
        m.close()


# ------------------------------------------------------------------ exits
@pytest.fixture(scope="module")
def wrap_batch(oracle):
    """64 clean modem frames of 2048 symbols, carrier offsets -315 .. +315 Hz in 10 Hz steps"""
    L = 2048 * CYCLES
    t = taps(oracle)
    x = np.concatenate([make_frames(1, L, CYCLES, t, FS, offset_hz=-315.0 + 10.0 * f, base_seed=900, first_frame=f)[0] for f in range(64)])
    return x, fixed_oracle(oracle, x)


def test_wrap_batch_wraps_at_every_step_position(oracle, wrap_batch):
    """CPU side of the fixture: the phase a step leaves is wrapped by the NEXT step's head -- step (i + 1) % 64 of its group, or the
    group's tail when that is 0 -- so the residues of i + 1 over all wraps of the batch must cover 0 .. 63.  The per-step trace is the
    oracle's own loop: it ends on the state oracle.rx_batch() reports."""
    x, want = wrap_batch
    seen = np.zeros(CHUNK, np.int64)
    for f in range(len(x)):
        ph, (p_end, f_end) = loop_trace(oracle, x[f])
        assert bits_equal(np.array([p_end, f_end]), np.array([want["phase"][f], want["freq"][f]], np.float32)), f
        before = np.concatenate([[0.0], ph[:-1]])
        wrapped = np.abs(ph - before) > np.pi                 # a step moves the phase by |freq| <= 1 plus alpha e, far below pi here
        seen += np.bincount((np.nonzero(wrapped)[0] + 1) % CHUNK, minlength=CHUNK)
    print("wraps per step position (0 = the tail):", seen.tolist())
    assert (seen > 0).all(), "no wrap at positions %s" % np.nonzero(seen == 0)[0].tolist()


@pytest.mark.parametrize("G,pair", STREAMS)
def test_wrap_at_every_step_position(wrap_batch, G, pair):
    x, want = wrap_batch
    run_lean(x, want, G, pair, "wraps at every step position")


@pytest.fixture(scope="module")
def exit_batch(oracle):
    """16 frames of 256 symbols: live modem frames, and among them frames on an axis (imaginary or real part exactly zero: the
    detector input of the first step has an exact zero, the C++ step takes the whole chunk), an all-zero frame (excused from the
    zero test), a frame that is silent from a chunk boundary on and one that falls silent inside a chunk, and one frame at a level
    that puts the phase beyond 4 pi in one step (the double-wrap flag)"""
    L = 2048
    x, _ = make_frames(16, L, CYCLES, taps(oracle), FS, offset_hz=40.0, base_seed=333, noise=0.02)
    x[1, :, 1] = 0.0          # real axis
    x[2, :, 0] = 0.0          # imaginary axis
    x[3] = 0.0
    x[5, 512 * 2 - 130:] = 0.0      # zero symbols from the start of the third chunk on
    x[6, 700:] = 0.0
    x[9, :, 1] = 0.0
    x[9, :, 0] *= -1.0
    x[12] *= 400.0
    want = fixed_oracle(oracle, x)
    return x, want


def test_exit_batch_has_what_it_claims(oracle, exit_batch):
    x, want = exit_batch
    z = want["costas"]
    for f in (1, 9):
        assert z[f, 0, 1] == 0.0 and z[f, 0, 0] != 0.0          # T of the first step: (a, 0)
    assert z[2, 0, 0] == 0.0 and z[2, 0, 1] != 0.0
    assert not z[3].any()
    c = Costas()
    oracle.lib.qo_costas_create(C.byref(c), BW, -1.0, 1.0)
    t = z[12].astype(np.float64)
    e = np.where(t[:, 0] > 0.0, 1.0, -1.0) * t[:, 1] - np.where(t[:, 1] > 0.0, 1.0, -1.0) * t[:, 0]
    # the phase in front of the update is within 2 pi, the frequency within 1: alpha |e| > 6 pi + 1 leaves it beyond 4 pi
    assert float(c.alpha) * float(np.abs(e).max()) > 6.0 * np.pi + 1.0


@pytest.mark.parametrize("G,pair", STREAMS)
def test_abandoned_chunks_zero_frames_and_double_wraps(exit_batch, G, pair):
    x, want = exit_batch
    run_lean(x, want, G, pair, "exits")


@pytest.mark.parametrize("G,pair", STREAMS)
def test_loaded_phase_of_minus_zero_keeps_the_first_chunk_off_the_stream(oracle, shape_batches, G, pair):
    """qpsk_rx_batch_ext with a seed phase of -0 in one frame: first_ring_chunk is 1 for its whole workgroup; a -0 frequency is kept
    away from the stream group by group"""
    L = 2048
    x = shape_batches[L][0][:12]
    seed = np.zeros((12, 2), np.float32)
    seed[2] = (-0.0, 0.0)
    seed[5] = (0.5, -0.0)
    seed[7] = (-0.0, -0.0)
    seed[10] = (3.0, 0.9)
    idx = np.full(12, INDEX, np.int32)
    want = oracle_ext(oracle, x, FS, RS, idx, seed)
    m = lean_modem(L, G, pair)
    try:
        got = m.rx_batch_ext(x, index=idx, seed=seed)
        m.sync()
        assert m.last_kernel().startswith(LEAN), m.last_kernel()
        assert_equal(got, want, "seeded, %d frames per workgroup, lean_pair %d" % (G, pair))
    finally:
        m.close()


def test_exact_zero_symbols_at_chunk_edges_costas_batch(oracle):
    """decimated symbols straight into the ring (costas_pipe_kernel): single exact-zero symbols at the first, an inner and the last
    step of a chunk, in the first and the last chunk, and a run across a hand-over -- each abandons its whole chunk"""
    import qpsk_amd
    import torch
    N, F = 256, 12
    rng = np.random.default_rng(64)
    d = rng.standard_normal((F, N, 2)).astype(np.float32)
    zero_at = {0: [0], 1: [63], 2: [64], 3: [100], 4: [127, 128], 5: [191], 6: [192], 7: [255], 8: list(range(120, 136)), 9: [5, 70, 133, 250]}
    for f, where in zero_at.items():
        d[f, where] = 0.0
    st0 = np.zeros((F, 2), np.float32)
    st0[10] = [3.0, 0.9]
    st0[11] = [-6.2, -0.99]
    m = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=N * CYCLES)
    try:
        st = torch.from_numpy(st0.copy()).cuda()
        sym, z = m.costas(d, st)
        m.sync()
        sym, z, st = cpu(sym), cpu(z), cpu(st)
    finally:
        m.close()
    for f in range(F):
        c = Costas()
        oracle.lib.qo_costas_create(C.byref(c), BW, -1.0, 1.0)
        c.phase, c.freq = float(st0[f, 0]), float(st0[f, 1])
        zr, zi = C.c_float(), C.c_float()
        want = np.empty((N, 2), np.float32)
        wsym = np.empty(N, np.uint8)
        for i in range(N):
            wsym[i] = oracle.lib.qo_costas_step(C.byref(c), float(d[f, i, 0]), float(d[f, i, 1]), C.byref(zr), C.byref(zi))
            want[i] = zr.value, zi.value
        assert np.array_equal(sym[f], wsym), f
        assert bits_equal(z[f], want), f
        assert bits_equal(st[f], np.array([c.phase, c.freq], np.float32)), f
