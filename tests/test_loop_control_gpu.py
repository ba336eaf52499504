"""qpsk_ctx_set_loop in front of every kernel that runs a Costas loop, bit for bit against the oracle with the gains and limits in force.

The gains live in device memory (d_gains), which has three writers -- the context's configuration upload, use_context_gains() and
qpsk_rx_batch_bw, which replaces them with a sweep's -- and the limits travel as kernel arguments.  Every single-loop entry must see
the context's own gains whatever ran before it, and a change enqueued behind an unsynchronised call must leave that call alone.
One sequence (drive()) for qpsk_costas_batch, qpsk_rx_batch on each receive kernel and qpsk_streams_rx_cplx on each stream route."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import Costas, TAU, TIMING_FIXED
from sigutil import bits_equal, make_frames, random_frames

pytestmark = pytest.mark.gpu

FS, RS = 19200.0, 2400.0
BW0 = np.float32(TAU / 100.0)                     # the context's own
BW1 = np.float32(TAU / 40.0)
LO1, HI1 = -0.02, 0.05                            # the stimuli sit 30 to 45 Hz off centre, ~0.1 rad/symbol: the clamp acts
SWEEP = [np.float32(TAU / 1000.0), np.float32(TAU / 200.0), np.float32(3.0 * TAU / 100.0)]


def modem(**kw):
    import qpsk_amd
    return qpsk_amd.Modem(**kw)


def cpu(t):
    return t.cpu().numpy()


def gains(oracle, bw):
    """set_loop_bandwidth()'s (alpha, beta) at the default damping; bandwidth 0 gives exactly (0, 0)"""
    c = Costas()
    oracle.lib.qo_costas_create(C.byref(c), float(bw), -1.0, 1.0)
    return float(c.alpha), float(c.beta)


def drive(m, oracle, call):
    """The sequence under test -> [(what call() returned, (bandwidth, min_freq, max_freq) in force)] for its steps; the two sweeps it
    runs in between are checked here"""
    import torch
    g0, g1 = gains(oracle, BW0), gains(oracle, BW1)
    assert gains(oracle, 0.0) == (0.0, 0.0) and g0 != g1
    one, two = (BW0, -1.0, 1.0), (BW1, LO1, HI1)
    runs = [(call(), one)]                                  # 1. the context's gains
    m.set_loop(*g1, LO1, HI1)                               # 2. NO synchronisation in between: the first call keeps bw0's results
    runs.append((call(), two))
    m.sync()
    xs = random_frames(2, m.frame_size, seed=5)
    x = torch.from_numpy(xs).to(m.dev)
    sweeps = [(m.rx_batch_bw(x, SWEEP), (LO1, HI1))]        # 3. a sweep overwrites d_gains; the context's own must be back
    runs.append((call(), two))
    m.set_loop(*g1, LO1, HI1)                               # 4. the same four values: no upload
    runs.append((call(), two))
    m.set_loop(0.0, 0.0, LO1, HI1)                          # 5. the loop is frozen
    runs.append((call(), (np.float32(0.0), LO1, HI1)))
    m.set_loop(*g0, -1.0, 1.0)                              # 6. back
    runs.append((call(), one))
    assert m.gains == (np.float32(g0[0]), np.float32(g0[1]))
    # 7. (beyond the six) the same two hazards with the sweep as the unsynchronised call: its own gains are in d_gains when a change of
    # the context's is enqueued right behind it, and the limits it runs with are those of step 6
    sweeps.append((m.rx_batch_bw(x, SWEEP), (-1.0, 1.0)))
    m.set_loop(*g1, LO1, HI1)
    runs.append((call(), two))
    m.sync()
    for got, (lo, hi) in sweeps:
        want = oracle.rx_batch_bw(xs, m.params.fs, m.params.rs, SWEEP, min_freq=lo, max_freq=hi, timing_mode=m.params.timing_mode,
                                  fixed_index=m.params.fixed_index)
        for k in ("sym", "freq", "phase", "index"):
            assert bits_equal(cpu(got[k]), want[k]), ("sweep", lo, hi, k)
    return runs


# ---------------------------------------------------------------------------- qpsk_costas_batch
def oracle_costas_rows(oracle, d, setting):
    """rows of decimated symbols through the oracle's loop from (0, 0) -> sym (R, N), z (R, N, 2), end state (R, 2)"""
    bw, lo, hi = setting
    R, N = d.shape[0], d.shape[1]
    sym, z, st = np.zeros((R, N), np.uint8), np.zeros((R, N, 2), np.float32), np.zeros((R, 2), np.float32)
    zr, zi = C.c_float(), C.c_float()
    for r in range(R):
        c = Costas()
        oracle.lib.qo_costas_create(C.byref(c), float(bw), lo, hi)
        for i in range(N):
            sym[r, i] = oracle.lib.qo_costas_step(C.byref(c), float(d[r, i, 0]), float(d[r, i, 1]), C.byref(zr), C.byref(zi))
            z[r, i] = (zr.value, zi.value)
        st[r] = (c.phase, c.freq)
    return sym, z, st


@pytest.fixture(scope="module")
def costas_rows(oracle):
    """70 distinct rows of 70 symbols turning at 0.1 rad/symbol, and the oracle's answers per loop setting"""
    rng = np.random.default_rng(21)
    n = np.arange(70)
    s = np.exp(1j * (0.1 * n[None] + np.pi / 2 * rng.integers(0, 4, (70, 70)) + np.pi / 4)) + 0.1 * (rng.standard_normal((70, 70)) + 1j * rng.standard_normal((70, 70)))
    d = np.stack([s.real, s.imag], -1).astype(np.float32)
    return dict(d=d, memo={})


@pytest.mark.parametrize("rows", ["70", "4 CUs + 6"])
def test_costas_batch_follows_set_loop(oracle, costas_rows, rows):
    """70 rows, and 4 CUs + 6: costas_pipe_kernel workgroups with two loader waves and a ragged last one"""
    import torch
    F = 70 if rows == "70" else 4 * torch.cuda.get_device_properties(0).multi_processor_count + 6
    fid = np.arange(F) % 70
    m = modem(fs=FS, rs=RS, frame_size=1024)
    d = torch.from_numpy(costas_rows["d"][fid]).to(m.dev)

    def call():
        st = torch.zeros((F, 2), dtype=torch.float32, device=m.dev)
        sym, z = m.costas(d, st)
        return sym, z, st

    runs = drive(m, oracle, call)
    for step, ((sym, z, st), setting) in enumerate(runs):
        if setting not in costas_rows["memo"]:
            costas_rows["memo"][setting] = oracle_costas_rows(oracle, costas_rows["d"], setting)
        wsym, wz, wst = costas_rows["memo"][setting]
        assert bits_equal(cpu(sym), wsym[fid]) and bits_equal(cpu(z), wz[fid]) and bits_equal(cpu(st), wst[fid]), step
    a, b, c = (costas_rows["memo"][s][2] for s in ((BW0, -1.0, 1.0), (BW1, LO1, HI1), (np.float32(0.0), LO1, HI1)))
    assert not bits_equal(a, b) and not bits_equal(b, c) and (b[:, 1] == np.float32(HI1)).any() and not c.any()      # the settings do differ
    m.close()


# ---------------------------------------------------------------------------- qpsk_rx_batch on its receive kernels
L2 = 16384
ROUTES = [      # test_rx_ext_gpu.ROUTES at its smallest frame counts: (frames, want_costas, tuning, expected kernel prefix)
    (4095, False, {}, "rx_lean_kernel"),
    (40, True, {}, "rx_fused_pipe_kernel"),
    (600, False, {"pipe_v": 2}, "rx_pipe2_kernel"),
    (48, True, {"fused_generic": 1}, "rx_fused_kernel"),
]
KEYS = ("sym", "freq", "phase", "hz")


@pytest.fixture(scope="module")
def frames(oracle):
    """24 distinct frames tiled to the largest batch, on the device, and the oracle's answers per loop setting (frames are independent)"""
    import torch
    taps = oracle.rrc_make(np.float32(FS), np.float32(RS), np.float32(.35))
    xu, _ = make_frames(24, L2, 8, taps, FS, offset_hz=45.0, base_seed=300, noise=0.02)
    xu[1::7] = random_frames(len(xu[1::7]), L2, seed=301)
    xu[2] = 0.0
    xu[3, : L2 // 3] = 0.0
    fid = np.arange(4095) % 24
    return dict(xu=xu, fid=fid, x=torch.from_numpy(np.ascontiguousarray(xu[fid])).cuda(), memo={})


@pytest.mark.parametrize("F,want_costas,tuning,kernel", ROUTES)
def test_rx_batch_follows_set_loop(oracle, frames, F, want_costas, tuning, kernel):
    m = modem(fs=FS, rs=RS, frame_size=L2, timing_mode=TIMING_FIXED, fixed_index=3)
    m.tune(**tuning)
    x, fid = frames["x"][:F], frames["fid"][:F]
    kernels = []

    def call():
        o = m.rx_batch(x, want_costas=want_costas)
        kernels.append(m.last_kernel())
        return o

    runs = drive(m, oracle, call)
    assert all(k.startswith(kernel) for k in kernels), kernels
    for step, (got, setting) in enumerate(runs):
        if setting not in frames["memo"]:
            bw, lo, hi = setting
            frames["memo"][setting] = oracle.rx_batch(frames["xu"], FS, RS, loop_bw=bw, min_freq=lo, max_freq=hi, timing_mode=TIMING_FIXED,
                                                      fixed_index=3, want_costas=True, threads=8)
        want = frames["memo"][setting]
        for k in KEYS + (("costas",) if want_costas else ()):
            assert bits_equal(cpu(got[k]), want[k][fid]), (step, k)
    for k in KEYS:      # 6 equals 1
        assert bits_equal(cpu(runs[5][0][k]), cpu(runs[0][0][k])), k
    one, two = frames["memo"][(BW0, -1.0, 1.0)], frames["memo"][(BW1, LO1, HI1)]
    assert not bits_equal(one["sym"], two["sym"]) and (two["freq"] == np.float32(HI1)).any()      # the settings do differ, the clamp acts
    m.close()


# ---------------------------------------------------------------------------- qpsk_streams_rx_cplx on its routes
STREAM_ROUTES = {"block": dict(stream_block=1, stream_scan=0), "apart": dict(stream_block=0, stream_scan=0),
                 "scan": dict(stream_block=0, stream_scan=1)}      # as test_streams_pcm_golden tunes them


@pytest.mark.parametrize("route", sorted(STREAM_ROUTES))
def test_streams_follow_set_loop(oracle, route):
    """9 streams, three blocks per step of the sequence; the oracle's modems run on with the same gains and limits written into their loops"""
    import torch
    L, S, PER = 1024, 9, 3
    m = modem(fs=FS, rs=RS, frame_size=L)
    m.tune(**STREAM_ROUTES[route])
    m.streams_reset(S)
    x, _ = make_frames(S, L * PER * 7, 8, m.taps, FS, offset_hz=30.0, base_seed=17, noise=0.02)
    blocks = np.ascontiguousarray(x.reshape(S, PER * 7, L, 2).transpose(1, 0, 2, 3))
    xd = torch.from_numpy(blocks).to(m.dev)
    at = [0]
    kernels = []

    def call():
        out = []
        for _ in range(PER):
            out.append(m.streams_rx_cplx(xd[at[0]]))
            kernels.append(m.last_kernel())
            at[0] += 1
        return out

    runs = drive(m, oracle, call)
    assert all((k == "stream_block_kernel") == (route == "block") for k in kernels), kernels
    assert any("stream_scan_kernel" in k for k in kernels) == (route == "scan"), kernels
    om = [oracle.modem(FS, RS, L, loop_bw=BW0) for _ in range(S)]
    k = 0
    for step, (outs, (bw, lo, hi)) in enumerate(runs):
        a, b = gains(oracle, bw)
        for s in range(S):
            om[s].s.loop.alpha, om[s].s.loop.beta, om[s].s.loop.min_freq, om[s].s.loop.max_freq = a, b, lo, hi
        for o in outs:
            sym, costas, phase, freq, index = (cpu(o[n]) for n in ("sym", "costas", "phase", "freq", "index"))
            for s in range(S):
                om[s].rx_cplx(blocks[k, s])
                assert index[s] == om[s].index, (step, k, s)
                assert bits_equal(sym[s], om[s].symbols) and bits_equal(costas[s], om[s].costas_frame), (step, k, s)
                assert phase[s].tobytes() == om[s].phase.tobytes() and freq[s].tobytes() == om[s].freq.tobytes(), (step, k, s)
            k += 1
    m.close()
