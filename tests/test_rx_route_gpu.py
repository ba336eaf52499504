"""Which kernel serves which receive call: a table from (entry point, batch size, timing mode, tuning keys) to the exact string
qpsk_ctx_last_kernel() gives afterwards.  No result is compared here -- every route's bits are held against the oracle by
test_gpu_parity.py, test_rx_ext_gpu.py and test_rx_data_gpu.py -- this file pins the ROUTING of rx_batch_common (api_rx.cpp), so that a
change to the host code that moves a shape to another kernel, or to another error text, shows as a changed string.

The expected strings are a record: they were taken from the library as it stood before the routing was rewritten as a side-effect-free
plan, and the rewritten code has to reproduce them.  Shapes: frame_size 1024 at 19200 / 2400 (CYCLES 8, 128 symbols = two chunks, the
smallest frame rx_lean_kernel serves), batch sizes at which a branch flips on a 256-CU device.  The input is noise: no route but the
histogram mode's one-pass route depends on content, and that one gets copies of one clean frame."""
import numpy as np
import pytest

from oracle.pyoracle import TIMING_FFT, TIMING_FIXED, TIMING_HIST
from sigutil import make_frames

pytestmark = pytest.mark.gpu

FS, RS, L = 19200.0, 2400.0, 1024
FMAX = 8192
BW = 0.0628
MODES = {"fixed": TIMING_FIXED, "fft": TIMING_FFT, "hist": TIMING_HIST}
LEAN, PIPE, PIPE2, GENERIC = "rx_lean_kernel", "rx_fused_pipe_kernel", "rx_pipe2_kernel", "rx_fused_kernel"
INLINE = " (FFT timing estimate inside the launch)"
ONEPASS = "rx_hist_kernel (one pass on the guessed index) + rx_fused_kernel (fall-back list)"


def make_noise():
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    return torch.randn(FMAX * L * 2 + 4096, generator=g, device="cuda", dtype=torch.float32)


@pytest.fixture(scope="module")
def noise():
    """FMAX frames of noise in device memory (and room for one odd pitch and an 8-byte offset); read-only, shared by every row"""
    return make_noise()


def observe(noise, call, F, mode="fixed", tune=None, frame_size=L, fs=FS, offset=0, pitch=0, **kw):
    """One receive call on a fresh context; the kernel string afterwards, or the text of the library's refusal (return code and message)."""
    import qpsk_amd
    import torch
    m = qpsk_amd.Modem(fs=fs, rs=RS, frame_size=frame_size, timing_mode=MODES[mode], fixed_index=3)
    try:
        m.tune(**(tune or {}))
        row = pitch or frame_size
        assert 2 * offset + F * row * 2 <= noise.numel()
        x = noise[2 * offset:2 * offset + F * row * 2].view(F, row, 2)
        try:
            if call == "rx":
                m.rx_batch(x, **kw)
            elif call == "raw":      # a frame pitch of its own
                m.rx_batch_raw(x, F, m.empty((F, m.nsym), torch.uint8), m.empty((F,), torch.float32), m.empty((F,), torch.float32), pitch=pitch)
            elif call == "bw":
                m.rx_batch_bw(x, [BW * (1.0 + b / 64.0) for b in range(kw["loops"])])
            elif call == "ext":
                m.rx_batch_ext(x, index=torch.full((F,), 5, dtype=torch.int32) if kw.get("index") else None,
                               seed=torch.zeros((F, 2), dtype=torch.float32) if kw.get("seed") else None)
            elif call == "data":
                m.rx_batch_data(x, want_sym=kw.get("want_sym", False))
            else:
                raise AssertionError(call)
        except qpsk_amd.QpskError as e:
            return str(e)
        m.sync()
        return m.last_kernel()
    finally:
        m.close()


def fixed(F, pipe_v, expected):
    return ("fixed-%d-v%s" % (F, pipe_v), dict(call="rx", F=F, tune=dict(pipe_v=pipe_v)), expected)


TABLE = [
    # ---- fixed timing, nothing set: the pipeline kernel of 16-frame workgroups below four frames per workgroup, rx_lean_kernel from there on
    fixed(40, None, PIPE), fixed(512, None, PIPE), fixed(513, None, LEAN), fixed(1024, None, LEAN),
    fixed(1023, None, LEAN),            # odd and ragged: pad rows and the last-row copy
    fixed(4097, None, LEAN), fixed(8192, None, LEAN),
    # ---- QPSK_PIPE_V names a kernel: 1 and 2 the older pipeline kernels, 3 rx_lean_kernel at any batch size
    fixed(40, 1, PIPE), fixed(512, 1, PIPE), fixed(513, 1, PIPE), fixed(1024, 1, PIPE), fixed(1023, 1, PIPE), fixed(4097, 1, PIPE), fixed(8192, 1, PIPE),
    fixed(40, 2, PIPE2), fixed(512, 2, PIPE2), fixed(513, 2, PIPE2), fixed(1024, 2, PIPE2), fixed(1023, 2, PIPE2), fixed(4097, 2, PIPE2), fixed(8192, 2, PIPE2),
    fixed(40, 3, LEAN), fixed(512, 3, LEAN), fixed(513, 3, LEAN), fixed(1024, 3, LEAN), fixed(1023, 3, LEAN), fixed(4097, 3, LEAN), fixed(8192, 3, LEAN),
    ("fixed-4096-g32", dict(call="rx", F=4096, tune=dict(pipe_g=32)), LEAN),
    ("fixed-4096-g20", dict(call="rx", F=4096, tune=dict(pipe_g=20)), LEAN),
    # ---- FFT timing: the estimate inside the launch, and in front of it where the LDS is full (32 frames per workgroup) or the caller says so
    ("fft-1024", dict(call="rx", F=1024, mode="fft"), LEAN + INLINE),
    ("fft-4096", dict(call="rx", F=4096, mode="fft"), LEAN + INLINE),
    ("fft-8192", dict(call="rx", F=8192, mode="fft"), LEAN),
    ("fft-1024-unfused", dict(call="rx", F=1024, mode="fft", tune=dict(fft_fused=0)), LEAN),
    # ---- a costas_frame[] dump leaves rx_lean_kernel
    ("costas-1024", dict(call="rx", F=1024, want_costas=True), PIPE),
    # ---- several loops per frame
    ("bw4-64", dict(call="bw", F=64, loops=4), PIPE),
    ("bw4-4097", dict(call="bw", F=4097, loops=4), PIPE2),
    ("bw16-64", dict(call="bw", F=64, loops=16), PIPE),
    ("bw16-4097-v2", dict(call="bw", F=4097, loops=16, tune=dict(pipe_v=2)), PIPE2),
    ("bw64-64", dict(call="bw", F=64, loops=64), GENERIC),
    # ---- acquisition from outside, FFT mode: offsets given = no estimate at all
    ("ext-index", dict(call="ext", F=1024, mode="fft", index=True), LEAN),
    ("ext-seed", dict(call="ext", F=1024, mode="fft", seed=True), LEAN + INLINE),
    ("ext-both", dict(call="ext", F=1024, mode="fft", index=True, seed=True), LEAN),
    # ---- data decisions: inside rx_lean_kernel, or from a costas_frame[] dump behind any other launch
    ("data-1024", dict(call="data", F=1024), LEAN),
    ("data-1024-sym", dict(call="data", F=1024, want_sym=True), PIPE),
    ("data-40", dict(call="data", F=40), PIPE),
    # ---- 125 symbols are not whole chunks: not rx_lean_kernel; then the shapes no pipeline kernel takes
    ("frame-1000", dict(call="rx", F=1024, frame_size=1000), PIPE),
    ("align-8", dict(call="rx", F=1024, offset=1), GENERIC),
    ("pitch-odd", dict(call="raw", F=1024, pitch=L + 1), GENERIC),
    ("cycles-4", dict(call="rx", F=1024, fs=9600.0), GENERIC),
    ("generic-key", dict(call="rx", F=1024, tune=dict(fused_generic=1)), GENERIC),
    # ---- a geometry the library refuses: the return code and the text
    ("layout-mismatch", dict(call="rx", F=1024, tune=dict(pipe_layout_lo=0x2, pipe_g=8, pipe_v=2)), "libqpsk_hip error -2: QPSK_PIPE_LAYOUT_*: 2 units on 1 waves do not match 8 frames per workgroup"),
]


@pytest.mark.parametrize("spec,expected", [pytest.param(s, e, id=i) for i, s, e in TABLE])
def test_route(noise, spec, expected):
    assert observe(noise, **spec) == expected


def histogram_sequence(tune):
    """two histogram-mode calls on one context over 1024 copies of one clean frame (every frame on one index: the guess holds)"""
    import qpsk_amd
    import torch
    m = qpsk_amd.Modem(fs=FS, rs=RS, frame_size=L, timing_mode=TIMING_HIST)
    try:
        m.tune(**tune)
        one, _ = make_frames(1, L, m.cycles, m.taps, FS, offset_hz=40.0, base_seed=80)
        x = torch.from_numpy(np.ascontiguousarray(np.tile(one, (1024, 1, 1)))).cuda()
        seen = []
        for _ in range(2):
            m.rx_batch(x)
            m.sync()
            seen.append(m.last_kernel())
        return seen
    finally:
        m.close()


def test_histogram_route_follows_the_guess():
    """the first call has no guess and takes the two launches; it leaves its majority index behind, and the second call runs in one pass"""
    assert histogram_sequence({}) == [LEAN, ONEPASS]


def test_histogram_route_switched_off():
    assert histogram_sequence(dict(hist_onepass=0)) == [LEAN, LEAN]
