"""rrc_fir_stream_kernel (firstream.hip) where one wave owns a RUN of two or three 512-output tiles, and the FFT sizes test_fft_batch skips.

The launcher cuts a frame into up to 16 * compute-units runs, so a run is longer than one tile only when nframes * ceil(length / 512) exceeds
that: no other shape of the suite gets there with a sample compared.  Inside such a run the next tile's history is carried in
registers, the next tile is prefetched, the LDS image is reused and the last run of a frame may be shorter.  Every case below derives its
frame count from the device's compute units and asserts the geometry it is about through qpsk_test_fir_runs (Modem.fir_runs): a premise that
does not hold fails the test.  Every comparison is on the raw bits."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TAU, TIMING_HIST
from sigutil import bits_equal, make_frames

pytestmark = pytest.mark.gpu
BW = np.float32(TAU / 100.0)
FS, RS = 19200.0, 2400.0
TILE = 512
STREAM, GENERIC = "rrc_fir_stream_kernel", "rrc_fir_kernel"

# name: (length, F from S = 16 * compute units, (ntiles, parts, tpp), the tile whose last 128 samples are planted: never the last of its run)
CASES = {
    "A": (1025, lambda S: S // 2 + 2, (3, 2, 2), 0),      # runs {0,1} {2}: the last run is one tile holding one sample; odd length
    "B": (1030, lambda S: S + 4, (3, 1, 3), 1),           # one wave per frame: two whole tiles, then a partial third
    "C": (2085, lambda S: S // 4 + 76, (5, 3, 2), 2),     # runs {0,1} {2,3} {4}: workgroups of four waves mix runs of different frames
    "D": (1536, lambda S: S, (3, 1, 3), 0),               # whole tiles only
}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def wave_slots():
    import torch
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    """two float32 device tensors, every element, as int32"""
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def modems():
    import qpsk_amd
    ms = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=1024)
    mg = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=1024)
    mg.tune(fir_generic=1)
    yield ms, mg
    ms.close()
    mg.close()


def boundary_frames(F, parts):
    """the frames on either side of a workgroup boundary near the middle of the batch (a workgroup: four units f * parts + part)"""
    u = (F * parts // 2) // 4 * 4
    while (u - 1) // parts == u // parts:
        u += 4
    return (u - 1) // parts, u // parts


_DATA = {}


@pytest.fixture(scope="module")
def case_data(modems, oracle):
    """per case, built once and only read afterwards: the stimulus, what the run-less rrc_fir_kernel makes of every frame, and the oracle's
    output for the sampled frames"""
    import torch
    ms, mg = modems

    def get(name):
        if name in _DATA:
            return _DATA[name]
        n, f_of, geom, carry_tile = CASES[name]
        F = f_of(wave_slots())
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1000 + ord(name))
        x = torch.randn((F, n, 2), generator=gen, device="cuda", dtype=torch.float32)
        mem = torch.randn((F, 127, 2), generator=gen, device="cuda", dtype=torch.float32)
        # the samples the register carry hands on: exact zeros of both signs, values whose products with the taps are tiny (1e-30) or
        # subnormal (2e-38: the path has no flush to zero), and large ones
        planted = (F // 5, 2 * F // 5 + 1, 3 * F // 5 + 2, 4 * F // 5 + 3)
        b = carry_tile * TILE + TILE - 128
        assert b + 128 <= n and (carry_tile + 1) % geom[2] != 0 and carry_tile + 1 < geom[0]
        seg = x[list(planted), b:b + 128].cpu().numpy()
        seg[0, 0:48] = np.float32(0.0)
        seg[0, 48:96] = np.float32(-0.0)
        seg[1] *= np.float32(1e-30)
        seg[2] *= np.float32(300.0)
        seg[3] *= np.float32(2e-38)
        assert np.signbit(seg[0, 48:96]).all() and not np.signbit(seg[0, 0:48]).any() and (seg[0, 0:96] == 0).all()
        assert np.any((seg[3] != 0) & (np.abs(seg[3]) < np.finfo(np.float32).tiny))
        x[list(planted), b:b + 128] = torch.from_numpy(seg).cuda()
        rng = np.random.default_rng(ord(name))
        fa, fb = boundary_frames(F, geom[1])
        assert fa != fb and (fa * geom[1] + geom[1] - 1) // 4 + 1 == (fb * geom[1]) // 4
        sample = np.unique(np.concatenate([[0, F - 1, fa, fb], planted, rng.choice(F, 8, replace=False)]))
        # the kernel without runs, every frame: carried delay lines and fresh ones
        mem_ref = mem.clone()
        y_ref = mg.rrc_fir(x, mem_ref)
        assert mg.last_kernel() == GENERIC
        y_ref0 = mg.rrc_fir(x, None)
        mg.sync()
        # the oracle on the sample
        taps = ms.taps
        pick = torch.from_numpy(sample).cuda()
        xs, mems = x[pick].cpu().numpy(), mem[pick].cpu().numpy()
        want_y, want_mem, want_y0 = xs.copy(), mems.copy(), xs.copy()
        for i in range(len(sample)):
            oracle.rrc_fir(taps, want_mem[i], want_y[i])
            oracle.rrc_fir(taps, np.zeros((127, 2), np.float32), want_y0[i])
        _DATA[name] = dict(F=F, n=n, geom=geom, x=x, mem=mem, y_ref=y_ref, mem_ref=mem_ref, y_ref0=y_ref0, sample=sample, pick=pick,
                           want_y=want_y, want_mem=want_mem, want_y0=want_y0)
        return _DATA[name]

    yield get
    _DATA.clear()


VARIANTS = [(c, v) for c in "ABCD" for v in ("carried", "fresh", "offset8")] + [("B", "inplace"), ("C", "inplace")]


@pytest.mark.parametrize("case,variant", VARIANTS)
def test_multi_tile_runs(modems, case_data, case, variant):
    """rrc_fir_stream_kernel in runs of two or three tiles: every frame against rrc_fir_kernel (which has no runs), a sample of at least 12
    frames -- first, last, both sides of a workgroup boundary, the planted ones, a seeded draw -- against the oracle; output and delay line.
    Variants: a carried delay line, none (fresh, no write-back), input 8 bytes off a 16-byte boundary (no 16-byte path on any tile), and
    in place (the library filters from a copy)"""
    import torch
    ms, _ = modems
    d = case_data(case)
    F, n = d["F"], d["n"]
    assert ms.fir_runs(F, n) == d["geom"], (case, F, n, ms.fir_runs(F, n))      # the premise, from the library
    assert d["geom"][2] >= 2
    x = d["x"]
    d_mem = None if variant == "fresh" else d["mem"].clone()
    if variant == "offset8":
        buf = torch.zeros((F * n + 1, 2), dtype=torch.float32, device="cuda")
        buf[1:] = x.reshape(-1, 2)
        xin = buf[1:].reshape(F, n, 2)
        assert xin.data_ptr() % 16 == 8 and xin.is_contiguous()
        y = ms.rrc_fir(xin, d_mem)
    elif variant == "inplace":
        y = x.clone()
        ms._check(ms.L.qpsk_rrc_fir_batch(ms.h, ptr(d_mem), ptr(y), ptr(y), F, n))
    else:
        assert x.data_ptr() % 16 == 0
        y = ms.rrc_fir(x, d_mem)
    assert ms.last_kernel() == STREAM, ms.last_kernel()
    ms.sync()
    y_ref = d["y_ref0"] if variant == "fresh" else d["y_ref"]
    if not same_bits(y, y_ref):
        bad = torch.nonzero((y.view(torch.int32) != y_ref.view(torch.int32)).any(dim=2))
        raise AssertionError("%s/%s: %d samples differ from rrc_fir_kernel, first (frame, sample) %s" % (case, variant, len(bad), bad[:6].tolist()))
    if d_mem is not None:
        assert same_bits(d_mem, d["mem_ref"]), (case, variant, "delay lines differ from rrc_fir_kernel")
    sample, pick = d["sample"], d["pick"]
    assert len(sample) >= 12
    ys = y[pick].cpu().numpy()
    want = d["want_y0"] if variant == "fresh" else d["want_y"]
    for i, f in enumerate(sample):
        assert bits_equal(ys[i], want[i]), (case, variant, int(f), np.flatnonzero((ys[i].view(np.uint32) != want[i].view(np.uint32)).any(axis=1))[:8])
    if d_mem is not None:
        assert bits_equal(d_mem[pick].cpu().numpy(), d["want_mem"]), (case, variant, "delay lines differ from the oracle")


def test_fir_runs_hook_contract(modems):
    """qpsk_test_fir_runs: bad arguments are QPSK_ERR_ARG and touch nothing; and the shapes test_rrc_fir_batch_with_delay_lines filters all run
    one tile per wave -- why this file exists"""
    ms, _ = modems
    ms.rrc_fir(np.zeros((2, 600, 2), np.float32))
    ms.sync()
    before = ms.last_kernel()
    assert before == STREAM
    out = (C.c_int * 3)(-7, -7, -7)
    fn = ms.L.qpsk_test_fir_runs
    for args in ((None, 5, 5, out), (ms.h, 5, 5, None), (ms.h, 0, 5, out), (ms.h, -1, 5, out), (ms.h, 5, 0, out), (ms.h, 5, -3, out)):
        assert fn(*args) == -2, args[1:3]
        assert b"qpsk_test_fir_runs" in ms.L.qpsk_last_error()
    assert list(out) == [-7, -7, -7] and ms.last_kernel() == before
    for F, n in ((5, 1), (5, 4097), (1, 70000), (2, 33333), (700, 640)):
        ntiles, parts, tpp = ms.fir_runs(F, n)
        assert ntiles == -(-n // TILE) and tpp == 1 and parts == ntiles, (F, n, ntiles, parts, tpp)
    assert ms.last_kernel() == before


def test_three_kernel_histogram_route_in_runs_of_two(oracle):
    """the receive path's three-kernel histogram route (QPSK_HIST_GENERIC = 1: rrc_fir -> scan -> receive kernel) on S + 1 frames of 1024
    samples at an ODD pitch: the filter runs two tiles per wave with in_pitch != length and no 16-byte path.  Every frame's index equals the
    fused scan's (packed frames, another context); 16 frames against the oracle in every output"""
    import torch
    import qpsk_amd
    L = 1024
    F = wave_slots() + 1
    m = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_HIST)
    m.tune(hist_generic=1)
    assert m.fir_runs(F, L) == (2, 1, 2), m.fir_runs(F, L)
    base, _ = make_frames(64, L, m.cycles, m.taps, FS, offset_hz=50.0, base_seed=77, noise=0.02)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    x = torch.from_numpy(base).cuda()[torch.arange(F, device="cuda") % 64]
    x = (x + 0.05 * torch.randn(x.shape, generator=gen, device="cuda", dtype=torch.float32)).contiguous()
    xp = torch.zeros((F, L + 1, 2), dtype=torch.float32, device="cuda")
    xp[:, :L] = x
    outs = []
    for mm, src, pitch in ((m, xp, L + 1), (qpsk_amd.Modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_HIST), x, 0)):
        o = dict(sym=mm.empty((F, mm.nsym), torch.uint8), freq=mm.empty((F,), torch.float32), phase=mm.empty((F,), torch.float32),
                 index=mm.empty((F,), torch.int32))
        mm.rx_batch_raw(src, F, o["sym"], o["freq"], o["phase"], pitch=pitch, index=o["index"])
        mm.sync()
        outs.append(o)
        if mm is not m:
            assert "rx_hist_kernel" not in mm.last_kernel(), mm.last_kernel()       # no guess yet: the fused scan, then the receive kernel
            mm.close()
    assert m.last_kernel() == "rx_fused_kernel", m.last_kernel()      # an odd pitch: the generic receive kernel behind the three-kernel estimate
    assert torch.equal(outs[0]["index"], outs[1]["index"])
    rng = np.random.default_rng(11)
    sample = np.unique(np.concatenate([[0, 1, 3, 4, F - 2, F - 1], rng.choice(F, 12, replace=False)]))      # 3 | 4: a workgroup boundary of the filter
    assert len(sample) >= 16
    pick = torch.from_numpy(sample).cuda()
    want = oracle.rx_batch(x[pick].cpu().numpy(), FS, RS, loop_bw=BW, timing_mode=TIMING_HIST)
    for k in ("sym", "freq", "phase", "index"):
        assert bits_equal(outs[0][k][pick].cpu().numpy(), want[k]), k
    m.close()


# ------------------------------------------------------------------ the FFT sizes test_fft_batch leaves out
@pytest.mark.parametrize("log2n", [2, 4, 5, 6, 7, 8, 10, 12, 15, 17, 18, 19])
def test_fft_remaining_sizes(oracle, log2n):
    """fft_kernel at 4, 16 .. 256, 1024, 4096 and fft_big_late_kernel with 3, 5, 6 and 7 remaining stages (2^15, 2^17 .. 2^19): forward and
    inverse, every row against the oracle's fftn / ifftn (the same host libm builds both twiddle sets)"""
    import qpsk_amd
    m = qpsk_amd.Modem()
    n, nb = 1 << log2n, 3 if log2n <= 12 else 2
    rng = np.random.default_rng(100 + log2n)
    x = rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))
    X = m.fft(x).cpu().numpy()
    Xi = m.fft(x, inverse=True).cpu().numpy()
    m.sync()
    for b in range(nb):
        assert bits_equal(X[b], oracle.fftn(x[b])), (n, b)
        assert bits_equal(Xi[b], oracle.ifftn(x[b])), (n, b)
    m.close()


@pytest.mark.parametrize("log2n,nb", [(15, 2), (12, 3)])
def test_fft_in_place_rows(oracle, log2n, nb):
    """in place with more than one row: 2^15 goes through the two-pass path's staging copy (row 1 must not read row 0's result), 4096 is the
    LDS kernel, which the in-place check of test_fft_batch (2^21) never reaches.  Equal to the out-of-place result and to the oracle"""
    import torch
    import qpsk_amd
    m = qpsk_amd.Modem()
    n = 1 << log2n
    rng = np.random.default_rng(200 + log2n)
    x = rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))
    for inverse in (0, 1):
        X = m.fft(x, inverse=bool(inverse)).cpu().numpy()
        xin = torch.from_numpy(x).cuda()
        m._check(m.L.qpsk_fft_batch(m.h, ptr(xin), ptr(xin), nb, n, inverse))
        m.sync()
        got = xin.cpu().numpy()
        assert bits_equal(got, X), (n, inverse)
        for b in range(nb):
            assert bits_equal(got[b], oracle.ifftn(x[b]) if inverse else oracle.fftn(x[b])), (n, inverse, b)
    m.close()
