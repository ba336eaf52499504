"""qpsk_rx_batch_data / qpsk_sync_batch / qpsk_multi_set_data on the GPU: the data rule bit for bit against the oracle's costas_frame[]
(test_rx_ext_cpu.oracle_ext) and against qpsk_rx_batch_ext with a costas_frame[] dump, on every route; the sync search against its numpy
restatement (test_rx_data_cpu.sync_ref); a whole link from baseband to checked CRCs with the library's own calls."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TIMING_FFT, TIMING_FIXED, TIMING_HIST
from sigutil import bits_equal
from test_rx_data_cpu import data_rule, make_packet_frame, sync_ref, transmit
from test_rx_ext_gpu import FS, KEYS, L2, RS, check_rows, distinct_frames, oracle_rows, random_seeds, tiled, wg_indices

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_RANGE = -2, -6


def modem(**kw):
    import qpsk_amd
    return qpsk_amd.Modem(**kw)


@pytest.fixture(scope="module")
def stim(oracle):
    import torch
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    xu = distinct_frames(24, L2, m.taps, FS, 500)
    m.close()
    x, fid = tiled(xu, 4097)
    return dict(xu=xu, x=torch.from_numpy(x).cuda(), fid=fid, memo={})


def t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def check_against_ext(m, x, idx, seed, want_sym=False, pitch=0):
    """rx_batch_data against rx_batch_ext(want_costas) on the same arguments: data = the rule on its costas_frame[], every other output
    equal.  Returns (data result, the kernel rx_batch_data ran on)"""
    got = m.rx_batch_data(x, index=t(idx), seed=t(seed), want_sym=want_sym, pitch=pitch)
    m.sync()
    kernel = m.last_kernel()
    ref = m.rx_batch_ext(x, index=t(idx), seed=t(seed), want_costas=True, pitch=pitch)
    m.sync()
    assert bits_equal(got["data"].cpu().numpy(), data_rule(ref["costas"].cpu().numpy()))
    for k in KEYS[1:] + ("index",):
        assert bits_equal(got[k].cpu().numpy(), ref[k].cpu().numpy()), k
    if want_sym:
        assert bits_equal(got["sym"].cpu().numpy(), ref["sym"].cpu().numpy())
    return got, kernel


# ---------------------------------------------------------------------------- 1. the lean route
@pytest.mark.parametrize("F", [4096, 4097, 4095, 40])
def test_lean_route_bit_for_bit(oracle, stim, F):
    """data only: rx_lean_kernel wherever rx_batch_ext takes it (whole and ragged batches, odd / even / mixed offsets, seeds, every staging
    and serial-wave variant); the data rule against the oracle's costas_frame[] on sampled rows"""
    rng = np.random.default_rng(F)
    idx = wg_indices(F, 16, rng)
    seed = random_seeds(F, rng)
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED, fixed_index=3)
    x = stim["x"][:F]
    rows = check_rows(F)[::3]
    want = oracle_rows(oracle, stim["xu"], stim["fid"], idx, seed, rows, want_costas=True, memo=stim["memo"])
    for dma in (0, 1, 2):
        for pair in (0, 1):
            m.tune(lean_dma=dma, lean_pair=pair)
            m.rx_batch_ext(x, index=t(idx), seed=t(seed))
            m.sync()
            ext_kernel = m.last_kernel()
            got, kernel = check_against_ext(m, x, idx, seed)
            assert kernel == ext_kernel
            if F >= 4095:
                assert kernel == "rx_lean_kernel", kernel
            d = got["data"].cpu().numpy()
            for r, w in want.items():
                assert bits_equal(d[r], data_rule(w["costas"])), r
                assert bits_equal(got["freq"].cpu().numpy()[r], w["freq"]) and bits_equal(got["phase"].cpu().numpy()[r], w["phase"])
    m.close()


@pytest.mark.parametrize("mode,kernel", [(TIMING_FFT, "rx_lean_kernel (FFT timing estimate inside the launch)"), (TIMING_HIST, "rx_lean_kernel")])
def test_lean_route_with_the_contexts_timing(stim, mode, kernel):
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=mode)
    x = stim["x"][:4096]
    m.rx_batch_ext(x)
    m.sync()
    assert m.last_kernel() == kernel
    _, k = check_against_ext(m, x, None, random_seeds(4096, np.random.default_rng(1)))
    assert k == kernel
    _, k = check_against_ext(m, x, None, None)
    assert k == kernel
    m.close()


def test_config2_batch_once(oracle, stim):
    """the whole 4096 x 16384 config-2 batch at offset 6, against the oracle on a spread of rows"""
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED, fixed_index=6)
    idx = np.full(4096, 6, np.int32)
    got, kernel = check_against_ext(m, stim["x"][:4096], idx, None)
    assert kernel == "rx_lean_kernel"
    rows = list(range(0, 4096, 257)) + [4095]
    want = oracle_rows(oracle, stim["xu"], stim["fid"], idx, None, rows, want_costas=True, memo=stim["memo"])
    d = got["data"].cpu().numpy()
    for r, w in want.items():
        assert bits_equal(d[r], data_rule(w["costas"])), r
    m.close()


# ---------------------------------------------------------------------------- 2. the other routes
@pytest.mark.parametrize("F,tuning,kernel", [(40, {}, "rx_fused_pipe_kernel"), (600, {"pipe_v": 2}, "rx_pipe2_kernel"),
                                             (64, {"pipe_v": 1}, "rx_fused_pipe_kernel"), (48, {"fused_generic": 1}, "rx_fused_kernel")])
def test_other_kernels(oracle, stim, F, tuning, kernel):
    rng = np.random.default_rng(F + 1)
    idx = wg_indices(F, 16, rng)
    seed = random_seeds(F, rng)
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    m.tune(**tuning)
    got, k = check_against_ext(m, stim["x"][:F], idx, seed)
    assert k.startswith(kernel), k
    rows = check_rows(F)[::4]
    want = oracle_rows(oracle, stim["xu"], stim["fid"], idx, seed, rows, want_costas=True, memo=stim["memo"])
    for r, w in want.items():
        assert bits_equal(got["data"].cpu().numpy()[r], data_rule(w["costas"])), r
    m.close()


def test_sym_requested_as_well(stim):
    rng = np.random.default_rng(7)
    for F in (4096, 41):
        m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
        check_against_ext(m, stim["x"][:F], wg_indices(F, 16, rng), random_seeds(F, rng), want_sym=True)
        m.close()


def test_asymmetric_taps(stim):
    rng = np.random.default_rng(8)
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    taps = np.array(m.taps, np.float32)
    taps[3] *= np.float32(1.01)
    m.set_taps(taps)
    check_against_ext(m, stim["x"][:512], wg_indices(512, 16, rng), random_seeds(512, rng))
    m.close()


def test_default_cycles4_modem(oracle):
    from sigutil import make_frames
    fs, rs, L, F = 9600.0, 2400.0, 512, 64
    m = modem(fs=fs, rs=rs, frame_size=L, timing_mode=TIMING_HIST)
    x, _ = make_frames(F, L, 4, m.taps, fs, offset_hz=50.0, base_seed=17, noise=0.02)
    x[3] = 0.0
    rng = np.random.default_rng(17)
    idx = rng.integers(0, 8, F).astype(np.int32)
    seed = random_seeds(F, rng)
    from test_rx_ext_cpu import oracle_ext
    for ix in (idx, None):
        got, _ = check_against_ext(m, t(x), ix, seed)
        if ix is not None:
            want = oracle_ext(oracle, x, fs, rs, idx, seed, want_costas=True)
            assert bits_equal(got["data"].cpu().numpy(), data_rule(want["costas"]))
    m.close()


# ---------------------------------------------------------------------------- 3. errors
def test_errors(stim):
    import torch
    import qpsk_amd
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED)
    x = stim["x"][:64]
    F = 64
    fl = m.empty((F,), torch.float32)
    rc = m.L.qpsk_rx_batch_data(m.h, C.c_void_p(x.data_ptr()), 0, F, None, None, None, None, C.c_void_p(fl.data_ptr()), None, None, None)
    assert rc == QPSK_ERR_ARG
    bad = x.clone()
    bad[5, 4000, 0] = float("nan")
    m.rx_batch_data(bad)
    with pytest.raises(qpsk_amd.QpskError) as e:
        m.sync()
    assert "error %d" % QPSK_ERR_RANGE in str(e.value)
    idx = np.full(F, 2, np.int32)
    idx[9] = 9
    m.rx_batch_data(x, index=t(idx))
    with pytest.raises(qpsk_amd.QpskError) as e:
        m.sync()
    assert "error %d" % QPSK_ERR_ARG in str(e.value)
    check_against_ext(m, x, np.full(F, 2, np.int32), None)      # the next call is clean
    m.close()


# ---------------------------------------------------------------------------- 4. sync
def planted(F, nsym, nsync, rng, lag_lo, lag_hi, errors=0):
    data = rng.integers(0, 256, (F, nsym), dtype=np.uint8)      # high bits set: only the low two may be read
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    lags = rng.integers(lag_lo, lag_hi + 1, F)
    rots = rng.integers(0, 4, F)
    ring = np.array([0, 1, 3, 2], np.uint8)
    for f in range(F):
        w = ring[(ring[sync] + rots[f]) & 3].copy()
        for e in rng.choice(nsync, errors, replace=False) if errors else []:
            w[e] = (w[e] + 1 + rng.integers(0, 3)) & 3
        data[f, lags[f]:lags[f] + nsync] = w | (rng.integers(0, 64, nsync, dtype=np.uint8) << 2)
    return data, sync, lags, rots


def check_sync(m, data, sync, lag_min, lag_max, nout):
    got = m.sync(data, sync, lag_min, lag_max, nout)
    m.sync()
    want = sync_ref(data, sync, lag_min, lag_max, nout)
    for k in ("lag", "rot", "score", "out"):
        assert bits_equal(got[k].cpu().numpy(), want[k]), k
    return want


@pytest.mark.parametrize("F,nsym,nsync,window,nout,errors", [(4096, 2048, 64, 256, 1024, 0), (300, 2048, 64, 256, 1024, 6),
                                                             (65, 1000, 128, 300, 17, 20), (7, 130, 1, 129, 0, 0), (33, 700, 37, 663, 0, 3)])
def test_sync_planted_words(F, nsym, nsync, window, nout, errors):
    m = modem(fs=FS, rs=RS, frame_size=L2)
    rng = np.random.default_rng(F * 31 + nsync)
    lag_max = min(window - 1, nsym - nsync - nout)
    data, sync, lags, rots = planted(F, nsym, nsync, rng, 0, lag_max, errors)
    want = check_sync(m, data, sync, 0, lag_max, nout)
    if errors <= 6 and nsync >= 32:
        assert np.array_equal(want["lag"], lags) and np.array_equal(want["rot"], rots)
    m.close()


def test_sync_ties_and_whole_frame_window():
    m = modem(fs=FS, rs=RS, frame_size=L2)
    # exact ties everywhere: constant data, a constant word
    check_sync(m, np.full((5, 300), 2, np.uint8), [1, 1, 1], 0, 290, 7)
    check_sync(m, np.zeros((3, 64), np.uint8), [0, 1, 3, 2], 4, 60, 0)
    # a window as large as the whole frame (no LDS-sized limit)
    rng = np.random.default_rng(3)
    data, sync, _, _ = planted(9, 16384, 128, rng, 0, 16384 - 128)
    check_sync(m, data, sync, 0, 16384 - 128, 0)
    data, sync, _, _ = planted(9, 16384, 64, rng, 100, 8000)
    check_sync(m, data, sync, 37, 16384 - 64 - 1000, 1000)
    m.close()


def test_sync_argument_errors():
    import torch
    m = modem(fs=FS, rs=RS, frame_size=L2)
    data = torch.zeros((4, 100), dtype=torch.uint8, device="cuda")
    buf = torch.zeros((4, 200), dtype=torch.uint8, device="cuda")
    lag = torch.zeros(4, dtype=torch.int32, device="cuda")
    sw = (C.c_uint8 * 129)(*([1] * 129))
    bad = (C.c_uint8 * 4)(0, 1, 4, 2)
    p = lambda a: C.c_void_p(a.data_ptr())      # noqa: E731
    call = lambda d, n, s, ns, lo, hi, no, out, lg: m.L.qpsk_sync_batch(m.h, d, 4, n, s, ns, lo, hi, no, out, lg, None, None)  # noqa: E731
    assert call(p(data), 100, sw, 8, 0, 10, 10, p(buf), p(lag)) == 0
    for args in [(None, 100, sw, 8, 0, 10, 10, p(buf), p(lag)), (p(data), 100, None, 8, 0, 10, 10, p(buf), p(lag)),
                 (p(data), 100, sw, 0, 0, 10, 10, p(buf), p(lag)), (p(data), 100, sw, 129, 0, 10, 10, p(buf), p(lag)),
                 (p(data), 100, sw, 8, -1, 10, 10, p(buf), p(lag)), (p(data), 100, sw, 8, 11, 10, 10, p(buf), p(lag)),
                 (p(data), 100, sw, 8, 0, 83, 10, p(buf), p(lag)), (p(data), 100, sw, 8, 0, 10, -1, p(buf), p(lag)),
                 (p(data), 100, sw, 8, 0, 10, 10, None, None), (p(data), 100, bad, 4, 0, 10, 10, p(buf), p(lag)),
                 (p(data), 100, sw, 8, 0, 10, 10, C.c_void_p(data.data_ptr() + 50), p(lag)),
                 (p(buf), 100, sw, 8, 0, 10, 10, C.c_void_p(buf.data_ptr() + 399), p(lag))]:
        assert call(*args) == QPSK_ERR_ARG, args
    assert call(p(data), 100, sw, 8, 0, 82, 10, p(buf), p(lag)) == 0      # lag_max + nsync + nout == nsym
    assert call(p(data), 100, sw, 8, 0, 10, 0, C.c_void_p(data.data_ptr() + 50), p(lag)) == 0      # nout = 0: d_out is not looked at
    # the 400 bytes of data and the 40 of d_out inside one allocation: touching on either side (accepted, the reference's output), one byte shared
    rows, word, _, _ = planted(4, 100, 8, np.random.default_rng(5), 0, 10)
    want = sync_ref(rows, word, 0, 10, 10)
    arena, d_word = torch.zeros(1024, dtype=torch.uint8, device="cuda"), (C.c_uint8 * 8)(*word.tolist())
    for off, accepted in ((500, True), (60, True), (499, False), (61, False)):
        arena.zero_()
        arena[100:500] = torch.from_numpy(rows.reshape(-1)).cuda()
        rc = call(C.c_void_p(arena.data_ptr() + 100), 100, d_word, 8, 0, 10, 10, C.c_void_p(arena.data_ptr() + off), p(lag))
        if not accepted:
            assert rc == QPSK_ERR_ARG and b"qpsk_sync_batch: d_out overlaps d_data" in m.L.qpsk_last_error(), (off, rc)
            continue
        assert rc == 0, (off, m.L.qpsk_last_error())
        m.sync()
        assert bits_equal(arena[off:off + 40].cpu().numpy().reshape(4, 10), want["out"]) and bits_equal(lag.cpu().numpy(), want["lag"])
        assert np.array_equal(arena[100:500].cpu().numpy(), rows.reshape(-1))
    m.sync()
    m.close()


# ---------------------------------------------------------------------------- 5. end to end
def test_link_end_to_end(oracle):
    """256 config-2 frames, carrier offsets up to 0.9 RS/8 and random phases, small noise: carrier_est -> rx_batch_data with the seeds ->
    sync -> descramble -> pack -> CRC, every call the library's"""
    import torch
    F, C8, nbytes, prefix = 256, 8, 64, 120
    nsym = L2 // C8
    taps = oracle.rrc_make(np.float32(FS), np.float32(RS), np.float32(0.35))
    rng = np.random.default_rng(99)
    sync = rng.integers(0, 4, 64, dtype=np.uint8)
    dfs = rng.uniform(-0.9 * RS / 8, 0.9 * RS / 8, F)
    phases = rng.uniform(0, 2 * np.pi, F)
    x = np.zeros((F, L2, 2), np.float32)
    payloads = np.zeros((F, nbytes), np.uint8)
    for f in range(F):
        sym, payloads[f] = make_packet_frame(oracle, rng, nsym, prefix, sync, nbytes)
        x[f] = transmit(sym, L2, C8, taps, FS, offset_hz=float(dfs[f]), phase=float(phases[f]), noise=0.03, seed=f)
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED, fixed_index=126 % C8)
    xt = torch.from_numpy(x).cuda()
    est = m.carrier_est(xt)
    idx = torch.full((F,), 126 % C8, dtype=torch.int32)
    got = m.rx_batch_data(xt, index=idx, seed=est["seed"])
    nout = 4 * (nbytes + 2)
    s = m.sync(got["data"], sync, 0, 255, nout)
    body = m.scramble(s["out"])
    packed = torch.empty((F, nout // 4), dtype=torch.uint8, device="cuda")
    m._check(m.L.qpsk_pack_symbols(m.h, C.c_void_p(body.data_ptr()), F, nout, C.c_void_p(packed.data_ptr())))
    crc = m.crc16(packed[:, :nbytes].contiguous())
    m.sync()
    pk = packed.cpu().numpy()
    assert np.array_equal(pk[:, :nbytes], payloads)
    stored = (pk[:, nbytes].astype(np.uint16) << 8) | pk[:, nbytes + 1]
    assert np.array_equal(crc, stored)
    assert np.all(s["lag"].cpu().numpy() == prefix + 126 // C8)
    assert set(s["rot"].cpu().numpy().tolist()) == {0, 1, 2, 3}
    # the sync search over the data rule restated on the host agrees
    want = sync_ref(got["data"].cpu().numpy(), sync, 0, 255, nout)
    assert bits_equal(s["out"].cpu().numpy(), want["out"])
    m.close()


# ---------------------------------------------------------------------------- 6. multi
@pytest.mark.parametrize("packed", [False, True])
def test_multi_data_mode(stim, packed):
    import qpsk_amd
    L, F = 2048, 301
    mj = qpsk_amd.MultiJob([0, 0, 0], fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_FIXED, fixed_index=4)
    from test_rx_ext_gpu import distinct_frames as frames_of
    m = modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_FIXED, fixed_index=4)
    x = frames_of(F, L, m.taps, FS, 600)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 8, F).astype(np.int32)
    seed = random_seeds(F, rng)
    mj.load(x)
    mj.set_packed(packed)
    mj.set_data(True)
    for acq in (False, True):
        if acq:
            mj.set_acquisition(idx, seed)
        outs = [mj.outputs(), mj.outputs()]
        mj.begin(0)
        mj.begin(1)
        with pytest.raises(qpsk_amd.QpskError):
            mj.set_data(False)
        mj.end(0, *outs[0])
        mj.end(1, *outs[1])
        want = {"data": [], "freq": [], "phase": []}
        for r in range(3):
            sh = mj.shard(r)
            sl = slice(sh["first"], sh["first"] + sh["count"])
            g = m.rx_batch_data(t(x[sl]), index=t(idx[sl]) if acq else None, seed=t(seed[sl]) if acq else None)
            m.sync()
            for k in want:
                want[k].append(g[k].cpu().numpy())
        wd = np.concatenate(want["data"])
        for o in outs:
            rows = mj.unpack(o[0]) if packed else o[0]
            assert bits_equal(rows, wd)
            assert bits_equal(o[1], np.concatenate(want["freq"])) and bits_equal(o[2], np.concatenate(want["phase"]))
    # off again: the slicer's rows
    mj.set_data(False)
    mj.set_acquisition(None, None)
    o = mj.outputs()
    mj.begin(0); mj.end(0, *o)
    plain = m.rx_batch(t(x))
    m.sync()
    assert bits_equal(mj.unpack(o[0]) if packed else o[0], plain["sym"].cpu().numpy())
    mj.close()
    m.close()
