"""Which kernel serves which block of the running streams: a table from (entry point, rates, frame_size, stream count, timing mode, tuning
keys, pointer alignment) to the exact string qpsk_ctx_last_kernel() gives after one call.  No result is compared here -- every route's
bits are held against the oracle by test_gpu_parity.py and test_abi.py, which force the routes with tuning keys -- this file pins the
ROUTING of the three stream entries (stream_route() in api_streams.cpp) at the library's OWN thresholds: 1.4 M, 3.5 M and 0.4 M samples per block
of all streams, 1024, 2560 and 3584 streams, a row on either side of each.  The thresholds are constants; none depends on the CU count.

The expected strings are a record: they were taken from the library as it stood before the routing was rewritten as a side-effect-free
plan, and the rewritten code has to reproduce them.  Each row is one fresh context: tune(), streams_reset() -- the reset reads the tuning:
it decides whether the streams share one carrier table -- one call, sync(), the string.  The input is noise: no route depends on content."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TIMING_FFT, TIMING_FIXED, TIMING_HIST

pytestmark = pytest.mark.gpu

RS = 2400.0
MODES = {"fixed": TIMING_FIXED, "fft": TIMING_FFT, "hist": TIMING_HIST}
B = "stream_block_kernel"
S = "stream_scan_kernel + costas_pipe_kernel"
A = "filter, timing, costas_pipe_kernel"
GENERIC = "filter, timing, costas_kernel, decimate_kernel"
PCM_MAX = 3584 * 2304      # the largest PCM row, in samples
CPLX_MAX = 3584 * 512      # the largest complex row


@pytest.fixture(scope="module")
def noise():
    """PCM and complex noise in device memory, and the PCM's first samples on the host; read-only, shared by every row.  Each buffer has
    room for a view that starts one element (PCM) or one complex sample (8 bytes) into it."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    pcm = (3000.0 * torch.randn(PCM_MAX + 8, generator=g, device="cuda", dtype=torch.float32)).to(torch.int16)
    cplx = torch.randn(2 * CPLX_MAX + 8, generator=g, device="cuda", dtype=torch.float32)
    assert pcm.data_ptr() % 16 == 0 and cplx.data_ptr() % 16 == 0
    return dict(pcm=pcm, cplx=cplx, host=np.ascontiguousarray(pcm[:2735 * 512].cpu().numpy()))


def call(m, noise, entry, n, offset=0):
    """one block of n streams through the entry point; offset: elements (PCM) or complex samples the input starts into its buffer"""
    import torch
    L = m.frame_size
    if entry == "pcm":
        x = noise["pcm"][offset:offset + n * L].view(n, L)
        assert x.data_ptr() % 4 == 2 * (offset % 2)
        m.streams_rx_pcm(x, want_costas=False)
    elif entry == "pcm-nosym":      # the raw binding: no symbols wanted
        x = noise["pcm"][offset:offset + n * L]
        f, p = m.empty((n,), torch.float32), m.empty((n,), torch.float32)
        m._check(m.L.qpsk_streams_rx_pcm(m.h, C.c_void_p(x.data_ptr()), None, C.c_void_p(f.data_ptr()), C.c_void_p(p.data_ptr()), None, None))
    elif entry == "cplx":
        x = noise["cplx"][2 * offset:2 * offset + 2 * n * L].view(n, L, 2)
        assert x.data_ptr() % 16 == 8 * (offset % 2)
        m.streams_rx_cplx(x, want_costas=False)
    elif entry == "host":
        h = noise["host"][:n * L]
        sym = np.zeros((n, m.nsym), np.uint8)
        m._check(m.L.qpsk_streams_rx_pcm_host(m.h, C.c_void_p(h.ctypes.data), None, C.c_void_p(sym.ctypes.data), None, None))
    else:
        raise AssertionError(entry)


def observe(noise, entry, L, n, fs=19200.0, rs=RS, mode="hist", tune=None, offset=0, skew_taps=False):
    """One stream call on a fresh context; the kernel string afterwards"""
    import qpsk_amd
    m = qpsk_amd.Modem(fs=fs, rs=rs, frame_size=L, timing_mode=MODES[mode], fixed_index=3)
    try:
        m.tune(**(tune or {}))
        if skew_taps:      # taps[k] != taps[126 - k]: not the filter stream_scan_kernel keeps in registers
            t = m.taps
            t[3] *= np.float32(1.25)
            m.set_taps(t)
        m.streams_reset(n)
        call(m, noise, entry, n, offset)
        m.sync()
        return m.last_kernel()
    finally:
        m.close()


def row(name, entry, L, n, expected, **kw):
    return ("%s-%dx%d" % (name, n, L), dict(entry=entry, L=L, n=n, **kw), expected)


TABLE = [
    # ---- PCM, 19200 / 2400 (CYCLES 8), histogram timing, nothing tuned: the streams share one carrier table.  1.4 M samples between the
    # one-launch kernel and stream_scan_kernel; blocks longer than the one-launch kernel's 2048 samples: stream_scan_kernel from 1024 streams
    row("pcm", "pcm", 512, 2734, B), row("pcm", "pcm", 512, 2735, S), row("pcm", "pcm", 2048, 683, B), row("pcm", "pcm", 2048, 684, S),
    row("pcm", "pcm", 4096, 1023, A), row("pcm", "pcm", 4096, 1024, S), row("pcm", "pcm", 512, 1, B),
    # ---- every stream its own carrier: stream_scan_kernel from 2560 streams
    row("pcm-carrier0", "pcm", 512, 2559, B, tune=dict(stream_carrier=0)), row("pcm-carrier0", "pcm", 512, 2560, S, tune=dict(stream_carrier=0)),
    # ---- no stream_scan_kernel: the one-launch kernel up to 3.5 M samples
    row("pcm-scan0", "pcm", 512, 6835, B, tune=dict(stream_scan=0)), row("pcm-scan0", "pcm", 512, 6836, A, tune=dict(stream_scan=0)),
    # ---- the keys name a kernel (shapes both kernels take)
    row("pcm-block1", "pcm", 512, 2735, B, tune=dict(stream_block=1)),
    row("pcm-block0", "pcm", 512, 16, A, tune=dict(stream_block=0)),
    row("pcm-block0-scan1", "pcm", 512, 16, S, tune=dict(stream_block=0, stream_scan=1)),
    row("pcm-generic", "pcm", 512, 16, GENERIC, tune=dict(fused_generic=1)),
    # ---- complex input, CYCLES 8: the one-launch kernel up to 0.4 M samples, stream_scan_kernel from 3584 streams on a 16-byte boundary
    row("cplx", "cplx", 512, 781, B), row("cplx", "cplx", 512, 782, A), row("cplx", "cplx", 512, 3583, A), row("cplx", "cplx", 512, 3584, S),
    row("cplx-align8", "cplx", 512, 3584, A, offset=1),
    # ---- complex input, CYCLES 4 (9600 / 2400): the PCM rule's 3.5 M samples
    row("cplx-cycles4", "cplx", 512, 3583, B, fs=9600.0), row("cplx-cycles4", "cplx", 512, 3584, S, fs=9600.0),
    # ---- shapes stream_scan_kernel refuses: not whole 256-sample tiles, a filter that is not symmetric, CYCLES 16
    row("tile", "pcm", 520, 16, B), row("tile", "pcm", 520, 3000, B),
    row("skew-taps", "pcm", 512, 2735, B, skew_taps=True),
    row("cycles16", "pcm", 512, 2735, B, rs=1200.0),
    # ---- timing modes: the FFT estimate takes neither kernel, fixed timing both
    row("fft", "pcm", 1024, 16, A, mode="fft"), row("fixed", "pcm", 512, 2735, S, mode="fixed"),
    # ---- PCM one int16 off a 4-byte boundary: not stream_scan_kernel on the PCM.  A block the one-launch kernel does not take either goes
    # through mixer_kernel and is routed again as complex input in the context's own buffer -- to the kernels apart below 3584 streams, to
    # stream_scan_kernel on the mixed block from there on
    row("pcm-align2", "pcm", 512, 2735, B, offset=1), row("pcm-align2", "pcm", 4096, 1024, A, offset=1),
    row("pcm-align2", "pcm", 2304, 3584, S, offset=1),
    # ---- no symbols wanted: never the one-launch kernel
    row("nosym", "pcm-nosym", 512, 16, A), row("nosym", "pcm-nosym", 512, 2735, S),
    # ---- the host entry (9600 / 2400, 512-sample blocks: the drop-in's call): the one-launch kernel on the staging buffer -- arguments inline
    # up to 8 streams, completion polled or not -- or the device arena and the same routes
    row("host", "host", 512, 1, B, fs=9600.0), row("host", "host", 512, 8, B, fs=9600.0), row("host", "host", 512, 9, B, fs=9600.0),
    row("host-poll0", "host", 512, 1, B, fs=9600.0, tune=dict(stream_poll=0)),
    row("host", "host", 512, 2735, S),
    row("host-block0", "host", 512, 4, A, fs=9600.0, tune=dict(stream_block=0)),
]


@pytest.mark.parametrize("spec,expected", [pytest.param(s, e, id=i) for i, s, e in TABLE])
def test_route(noise, spec, expected):
    assert observe(noise, **spec) == expected


def test_route_follows_the_carrier_and_the_keys(noise):
    """one context, 2400 streams x 1024 samples of PCM (2.46 M samples): the shared carrier's stream_scan_kernel; with both kernels
    switched off the kernels apart, and the carrier goes back to the streams; keys unset again: no shared carrier any more and fewer
    than 2560 streams, so the one-launch kernel; a reset shares the carrier again"""
    import qpsk_amd
    n = 2400
    m = qpsk_amd.Modem(fs=19200.0, rs=RS, frame_size=1024)
    try:
        m.streams_reset(n)
        seen = []

        def block():
            call(m, noise, "pcm", n)
            m.sync()
            seen.append(m.last_kernel())

        block()
        m.tune(stream_block=0, stream_scan=0)
        block()
        m.tune(stream_block=None, stream_scan=None)
        block()
        m.streams_reset(n)
        block()
        assert seen == [S, A, B, S]
    finally:
        m.close()


ENTRIES = {"pcm": "qpsk_streams_rx_pcm", "cplx": "qpsk_streams_rx_cplx", "host": "qpsk_streams_rx_pcm_host"}


def refusal(m, noise, entry, n):
    import qpsk_amd
    with pytest.raises(qpsk_amd.QpskError) as e:
        call(m, noise, entry, n)
    return str(e.value)


def test_stream_call_before_any_reset_is_refused(noise):
    import qpsk_amd
    m = qpsk_amd.Modem(fs=9600.0, rs=RS, frame_size=512)
    try:
        for entry in ENTRIES:
            assert refusal(m, noise, entry, 4) == "libqpsk_hip error -5: call qpsk_streams_reset() first"
    finally:
        m.close()


def test_stream_call_on_poisoned_streams_is_refused(noise):
    """a kernel's word that it gave up (qpsk_test_inject_status) fails the stream call that reads it with QPSK_ERR_HIP; every entry then
    refuses by name until the reset"""
    import qpsk_amd
    m = qpsk_amd.Modem(fs=9600.0, rs=RS, frame_size=512)
    try:
        m.streams_reset(4)
        m._check(m.L.qpsk_test_inject_status(m.h, 1))
        assert refusal(m, noise, "host", 4) == ("libqpsk_hip error -3: pipeline kernel: producer/consumer wait timed out; results of the calls "
                                                "since the last synchronisation are invalid")
        for entry, who in ENTRIES.items():
            assert refusal(m, noise, entry, 4) == ("libqpsk_hip error -5: %s: an earlier stream call failed between its launches; the streams' "
                                                   "carried state is undefined until qpsk_streams_reset()" % who)
        m.streams_reset(4)
        call(m, noise, "host", 4)
        assert m.last_kernel() == B
    finally:
        m.close()
