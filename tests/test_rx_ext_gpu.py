"""qpsk_rx_batch_ext / qpsk_rx_batch_bw_ext / qpsk_multi_set_acquisition on the GPU: the caller's per-frame timing offsets and loop
seeds, bit for bit against the oracle composition of test_rx_ext_cpu.oracle_ext (rx_frame(frame) at the given index, set_phase /
set_frequency, rx_frame(zeros)), on every receive kernel that can take the batch."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.pyoracle import TAU, TIMING_FFT, TIMING_FIXED, TIMING_HIST
from sigutil import bits_equal, make_frames, random_frames
from test_rx_ext_cpu import oracle_ext

pytestmark = pytest.mark.gpu

BW = np.float32(TAU / 100.0)
FS, RS, L2 = 19200.0, 2400.0, 16384          # config 2: 2400 baud, 8x oversample, 16384 samples per frame
QPSK_ERR_ARG, QPSK_ERR_RANGE = -2, -6
KEYS = ("sym", "freq", "phase", "hz")


def modem(**kw):
    import qpsk_amd
    return qpsk_amd.Modem(**kw)


def distinct_frames(n, L, taps, fs, seed):
    """n frames: clean and noisy transmissions, noise, a zero frame and frames with zero stretches (the loop's exact-zero shortcut)"""
    x, _ = make_frames(n, L, 8, taps, fs, offset_hz=45.0, base_seed=seed, noise=0.02)
    x[1::7] = random_frames(len(x[1::7]), L, seed=seed + 1)
    x[2] = 0.0
    x[3, : L // 3] = 0.0
    x[4, L // 2:] = 0.0
    x[5, 1000:5000] = 0.0
    return x


def tiled(xu, F):
    fid = np.arange(F) % len(xu)
    return np.ascontiguousarray(xu[fid]), fid


def wg_indices(F, G, rng):
    """per workgroup of G frames: all even, all odd or mixed offsets 0..7"""
    idx = np.zeros(F, np.int32)
    for w in range(0, F, G):
        n = min(G, F - w)
        kind = (w // G) % 3
        if kind == 0:
            idx[w:w + n] = 2 * rng.integers(0, 4, n)
        elif kind == 1:
            idx[w:w + n] = 2 * rng.integers(0, 4, n) + 1
        else:
            idx[w:w + n] = rng.integers(0, 8, n)
    return idx


def random_seeds(F, rng):
    """phases in +-3 pi (some wrap at the load), frequencies inside and outside the [-1, 1] clamp, signed zeros"""
    s = np.zeros((F, 2), np.float32)
    s[:, 0] = rng.uniform(-3 * np.pi, 3 * np.pi, F)
    s[:, 1] = rng.uniform(-1.5, 1.5, F) * (rng.random(F) < 0.3) + rng.uniform(-0.02, 0.02, F) * (rng.random(F) >= 0.3)
    s[0] = (-0.0, -0.0)
    s[1 % F] = (0.0, -0.0)
    s[2 % F, 1] = 0.01          # the zero frame seeded with freq != 0: the phase advances every step, wraps included
    s[3 % F, 1] = -0.3
    s[4 % F, 1] = 0.7
    return s


def check_rows(F, G=16):
    rows = set(range(min(F, 3 * G))) | set(range(max(0, F - 2 * G), F)) | set(range(0, F, 37))
    return sorted(rows)


def oracle_rows(orc, xu, fid, idx, seed, rows, fs=FS, rs=RS, want_costas=False, memo=None):
    """oracle_ext on the listed rows of a tiled batch, memoised by (distinct frame, index, seed)"""
    memo = {} if memo is None else memo
    out = {}
    for r in rows:
        key = (int(fid[r]), int(idx[r]), None if seed is None else seed[r].tobytes(), want_costas)
        if key not in memo:
            one = oracle_ext(orc, xu[fid[r]][None], fs, rs, [idx[r]], None if seed is None else seed[r][None], want_costas=want_costas)
            memo[key] = {k: v[0] for k, v in one.items()}
        out[r] = memo[key]
    return out


def assert_rows(got, want, keys=KEYS):
    for k in keys:
        g = got[k].cpu().numpy()
        for r, w in want.items():
            assert bits_equal(g[r], w[k]), (k, r)


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert bits_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k


# ---------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("mode", [TIMING_FIXED, TIMING_HIST, TIMING_FFT])
def test_both_null_equals_pitched(oracle, mode):
    import torch
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=mode, fixed_index=5)
    xu = distinct_frames(32, L2, m.taps, FS, 100)
    for F in (4096, 40):
        x, _ = tiled(xu, F)
        xt = torch.from_numpy(x).cuda()
        want = m.rx_batch(xt)
        m.sync()
        got = m.rx_batch_ext(xt)
        m.sync()
        assert_same(got, want, KEYS + ("index",))
    m.close()


@pytest.mark.parametrize("k", range(8))
def test_uniform_index_equals_fixed_context(k):
    import torch
    mf = modem(fs=FS, rs=RS, frame_size=2048, timing_mode=TIMING_FIXED, fixed_index=k)
    mh = modem(fs=FS, rs=RS, frame_size=2048, timing_mode=TIMING_HIST)
    xu = distinct_frames(64, 2048, mf.taps, FS, 200 + k)
    x, _ = tiled(xu, 1024)
    xt = torch.from_numpy(x).cuda()
    want = mf.rx_batch(xt, want_costas=True)
    got = mh.rx_batch_ext(xt, index=torch.full((1024,), k, dtype=torch.int32), seed=torch.zeros((1024, 2)), want_costas=True)
    mf.sync(); mh.sync()
    assert_same(got, want, KEYS + ("index", "costas"))
    mf.close(); mh.close()


# ---------------------------------------------------------------------------- 2. histogram round trip
def test_histogram_indices_fed_back(oracle):
    import torch
    L, F = 2048, 1000
    mh = modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_HIST)
    mf = modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_FIXED, fixed_index=0)
    x, _ = make_frames(F, L, 8, mh.taps, FS, offset_hz=40.0, base_seed=7, noise=0.03)
    x[1::5] = random_frames(len(x[1::5]), L, seed=8)          # a fifth of the frames off the majority index
    xt = torch.from_numpy(x).cuda()
    h = mh.rx_batch(xt)
    mh.sync()
    idx = h["index"].clone()
    assert len(np.unique(idx.cpu().numpy())) > 1
    got = mf.rx_batch_ext(xt, index=idx)
    mf.sync()
    assert_same(got, h, KEYS + ("index",))
    want = oracle.rx_batch(x, FS, RS, loop_bw=BW, timing_mode=TIMING_HIST, threads=min(16, os.cpu_count() or 1))
    for k in KEYS + ("index",):
        assert bits_equal(got[k].cpu().numpy(), want[k]), k
    mh.close(); mf.close()


# ---------------------------------------------------------------------------- 3 + 4. per-frame indices and seeds on every kernel
ROUTES = [
    # (frames, want_costas, tuning, expected kernel prefix)
    (4096, False, {}, "rx_lean_kernel"),
    (4097, False, {}, "rx_lean_kernel"),
    (4095, False, {}, "rx_lean_kernel"),
    (40, False, {}, "rx_fused_pipe_kernel"),
    (40, True, {}, "rx_fused_pipe_kernel"),
    (600, False, {"pipe_v": 2}, "rx_pipe2_kernel"),
    (48, True, {"fused_generic": 1}, "rx_fused_kernel"),
]


@pytest.fixture(scope="module")
def stim(oracle):
    import torch
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    xu = distinct_frames(24, L2, m.taps, FS, 300)
    m.close()
    x, fid = tiled(xu, 4097)
    return dict(xu=xu, x=torch.from_numpy(x).cuda(), fid=fid, memo={})


@pytest.mark.parametrize("F,want_costas,tuning,kernel", ROUTES)
@pytest.mark.parametrize("use_index,use_seed", [(True, False), (True, True), (False, True)])
def test_per_frame_index_and_seed(oracle, stim, F, want_costas, tuning, kernel, use_index, use_seed):
    import torch
    rng = np.random.default_rng(F * 7 + use_index * 3 + use_seed)
    idx = wg_indices(F, 16, rng) if use_index else np.full(F, 3, np.int32)
    seed = random_seeds(F, rng) if use_seed else None
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED, fixed_index=3)
    x = stim["x"][:F]
    rows = check_rows(F)
    want = oracle_rows(oracle, stim["xu"], stim["fid"], idx, seed, rows, want_costas=want_costas, memo=stim["memo"])
    lean = kernel == "rx_lean_kernel"
    for dma in ((0, 1, 2) if lean else (None,)):
        for pair in ((0, 1, 2) if lean else (None,)):
            m.tune(lean_dma=dma, lean_pair=pair, **tuning)
            got = m.rx_batch_ext(x, index=torch.from_numpy(idx) if use_index else None,
                                 seed=None if seed is None else torch.from_numpy(seed), want_costas=want_costas)
            m.sync()
            assert m.last_kernel().startswith(kernel), (m.last_kernel(), kernel)
            assert_rows(got, want, KEYS + (("costas",) if want_costas else ()))
            assert bits_equal(got["index"].cpu().numpy(), idx)
    m.close()


def test_config2_seeded_ext_call_is_the_lean_kernel(oracle, stim):
    import torch
    rng = np.random.default_rng(5)
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    idx = torch.from_numpy(wg_indices(4096, 16, rng))
    seed = torch.from_numpy(random_seeds(4096, rng))
    m.rx_batch_ext(stim["x"][:4096], index=idx, seed=seed)
    m.sync()
    assert m.last_kernel() == "rx_lean_kernel"
    m.close()


# ---------------------------------------------------------------------------- 5. several loops per frame
def test_bw_ext_seeds_per_loop(oracle):
    import torch
    fs, rs, L, F = 9600.0, 1200.0, 4096, 24
    bws = [np.float32(TAU / 50.0), np.float32(TAU / 100.0), np.float32(TAU / 400.0)]
    m = modem(fs=fs, rs=rs, frame_size=L, timing_mode=TIMING_FIXED)
    x, _ = make_frames(F, L, 8, m.taps, fs, offset_hz=20.0, base_seed=11, noise=0.02)
    x[2] = 0.0
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 8, F).astype(np.int32)
    seed = np.stack([random_seeds(F, rng) for _ in bws], axis=1)      # (F, nbw, 2)
    for use_index in (True, False):
        ix = idx if use_index else np.zeros(F, np.int32)
        got = m.rx_batch_bw_ext(torch.from_numpy(x), bws, index=torch.from_numpy(ix) if use_index else None, seed=torch.from_numpy(seed))
        m.sync()
        for b, bw in enumerate(bws):
            want = oracle_ext(oracle, x, fs, rs, ix, seed[:, b], loop_bw=bw)
            assert bits_equal(got["sym"][:, b].cpu().numpy(), want["sym"]), b
            assert bits_equal(got["freq"][:, b].cpu().numpy(), want["freq"]), b
            assert bits_equal(got["phase"][:, b].cpu().numpy(), want["phase"]), b
    m.close()


# ---------------------------------------------------------------------------- 6. CYCLES = 4
def test_cycles4_index6_generic_path(oracle):
    import torch
    fs, rs, L, F = 9600.0, 2400.0, 512, 64
    m = modem(fs=fs, rs=rs, frame_size=L, timing_mode=TIMING_HIST)
    x, _ = make_frames(F, L, 4, m.taps, fs, offset_hz=50.0, base_seed=13, noise=0.02)
    x[3] = 0.0
    rng = np.random.default_rng(13)
    seed = random_seeds(F, rng)
    idx = np.full(F, 6, np.int32)
    idx[::5] = rng.integers(0, 8, len(idx[::5]))
    for s in (None, seed):
        got = m.rx_batch_ext(torch.from_numpy(x), index=torch.from_numpy(idx), seed=None if s is None else torch.from_numpy(s),
                             want_costas=True)
        m.sync()
        want = oracle_ext(oracle, x, fs, rs, idx, s, want_costas=True)
        for k in KEYS + ("costas",):
            assert bits_equal(got[k].cpu().numpy(), want[k]), k
    m.close()


# ---------------------------------------------------------------------------- 7. errors
@pytest.mark.parametrize("F,tuning", [(4096, {}), (40, {}), (600, {"pipe_v": 2}), (48, {"fused_generic": 1})])
def test_bad_index_is_reported_and_the_next_call_is_clean(oracle, stim, F, tuning):
    import torch
    import qpsk_amd
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    m.tune(**tuning)
    x = stim["x"][:F]
    rows = check_rows(F)
    good = np.full(F, 2, np.int32)
    want = oracle_rows(oracle, stim["xu"], stim["fid"], good, None, rows, memo=stim["memo"])
    for bad in (-1, 8, 2 ** 31 - 1, -2 ** 31):
        idx = good.copy()
        idx[F // 2 + 1] = bad
        m.rx_batch_ext(x, index=torch.from_numpy(idx))
        with pytest.raises(qpsk_amd.QpskError) as e:
            m.sync()
        assert "error %d" % QPSK_ERR_ARG in str(e.value) and "timing offset" in str(e.value)
        got = m.rx_batch_ext(x, index=torch.from_numpy(good))
        m.sync()
        assert_rows(got, want)
    m.close()


@pytest.mark.parametrize("F", [4096, 40])
def test_bad_seed_is_a_range_error(stim, F):
    import torch
    import qpsk_amd
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    x = stim["x"][:F]
    for bad in ((np.nan, 0.0), (0.0, np.nan), (1e30, 0.0), (np.inf, 0.0), (-np.inf, 0.1)):
        seed = np.zeros((F, 2), np.float32)
        seed[F // 3] = bad
        m.rx_batch_ext(x, seed=torch.from_numpy(seed))
        with pytest.raises(qpsk_amd.QpskError) as e:
            m.sync()
        assert "error %d" % QPSK_ERR_RANGE in str(e.value), bad
        m.rx_batch_ext(x, seed=torch.zeros((F, 2)))
        m.sync()
    m.close()


def test_ext_calls_leave_the_histogram_guess_alone():
    import torch
    L, F = 2048, 1024
    m = modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_HIST)
    x, _ = make_frames(F, L, 8, m.taps, FS, offset_hz=40.0, base_seed=21, noise=0.01)
    xt = torch.from_numpy(x).cuda()
    m.rx_batch(xt)
    m.rx_batch(xt)
    st0, st1 = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    m._check(m.L.qpsk_test_hist_state(m.h, st0))
    other = torch.from_numpy(np.ascontiguousarray(x[:, ::-1])).cuda()
    for ix in (None, torch.full((F,), 5, dtype=torch.int32)):
        got = m.rx_batch_ext(other, index=ix, seed=torch.full((F, 2), 0.1))
        assert "rx_hist_kernel" not in m.last_kernel()
        m.sync()
        m._check(m.L.qpsk_test_hist_state(m.h, st1))
        assert list(st0) == list(st1)
        assert got["sym"].shape == (F, m.nsym)
    m.close()


# ---------------------------------------------------------------------------- 8. multi
def test_multi_acquisition(oracle):
    import qpsk_amd
    L, F = 2048, 301
    mj = qpsk_amd.MultiJob([0, 0, 0], fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_FIXED, fixed_index=4)
    taps = oracle.rrc_make(np.float32(FS), np.float32(RS), np.float32(0.35))
    x = distinct_frames(F, L, taps, FS, 400)
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 8, F).astype(np.int32)
    seed = random_seeds(F, rng)
    mj.load(x)
    mj.set_acquisition(idx, seed)
    want = oracle_ext(oracle, x, FS, RS, idx, seed)
    outs = [mj.outputs(), mj.outputs()]
    mj.begin(0)
    mj.begin(1)
    mj.end(0, *outs[0])
    mj.begin(0)
    mj.end(1, *outs[1])
    mj.end(0, *outs[0])
    for o in outs:
        assert bits_equal(o[0], want["sym"]) and bits_equal(o[1], want["freq"]) and bits_equal(o[2], want["phase"])
    # index only, then back to the contexts' timing
    mj.set_acquisition(idx, None)
    mj.begin(0); mj.end(0, *outs[0])
    w2 = oracle_ext(oracle, x, FS, RS, idx, None)
    assert bits_equal(outs[0][0], w2["sym"]) and bits_equal(outs[0][2], w2["phase"])
    fixed = oracle.rx_batch(x, FS, RS, loop_bw=BW, timing_mode=TIMING_FIXED, fixed_index=4)
    mj.set_acquisition(None, None)
    mj.begin(1); mj.end(1, *outs[1])
    assert bits_equal(outs[1][0], fixed["sym"]) and bits_equal(outs[1][2], fixed["phase"])
    # a later load clears it
    mj.set_acquisition(idx, seed)
    mj.load(x)
    mj.begin(0); mj.end(0, *outs[0])
    assert bits_equal(outs[0][0], fixed["sym"]) and bits_equal(outs[0][1], fixed["freq"]) and bits_equal(outs[0][2], fixed["phase"])
    mj.close()
