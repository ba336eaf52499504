"""The polyphase channeliser (CHANNELISER in include/qpsk_hip.h: qpsk_channel_twiddles, qpsk_channel_reset, qpsk_channel_push): what can be
checked without a GPU.

channel_ref() below restates the header's definition in numpy float32, vectorised over the output times: the branch sums in the stated
order, the bit reversal, then the radix-2 stages one by one (the kernel keeps two stages in registers per pass; the operations and their
operands are these).  It takes the library's own table from qpsk_channel_twiddles, which is part of the definition.  Here: the table, the
restatement against the direct fp64 sum, split pushes, the prototype helper, and a noise-free link of three carriers in one wideband
capture through channel_ref, the oracle's stream receiver and the numpy deframer.  The GPU tests (test_channel_gpu.py) compare the kernel
with channel_ref bit for bit.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_deframe_cpu import deframe_ref
from test_frame_cpu import HALF, body_len, frame_ref, starts
from test_rx_data_cpu import data_rule
from test_rx_ext_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNEL_SYMBOLS = ("qpsk_channel_twiddles", "qpsk_channel_reset", "qpsk_channel_push")
QPSK_ERR_ARG = -2
U = 2.0 ** -24                       # the unit roundoff of fp32


# ------------------------------------------------------------------- the numpy restatement
_TW = {}


def twiddles(M):
    """the library's table (M / 2, 2) float32, once per M"""
    if M not in _TW:
        import qpsk_amd
        _TW[M] = qpsk_amd.channel_twiddles(M)
    return _TW[M]


def bitrev(M):
    n = M.bit_length() - 1
    return np.array([int(format(p, "0%db" % n)[::-1], 2) for p in range(M)])


def channel_ref(x, hist, h, M, P, tw):
    """x (T M, 2) float32, hist ((P - 1) M, 2) float32 or None (zeros), h (M P,) float32, tw (M / 2, 2) float32 ->
    (y (M, T, 2) float32: y[k, m] = y_k[m], the history after the push ((P - 1) M, 2))"""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    h = np.asarray(h, np.float32).reshape(P, M)
    tw = np.asarray(tw, np.float32)
    hist = np.zeros(((P - 1) * M, 2), np.float32) if hist is None else np.asarray(hist, np.float32).reshape(-1, 2)
    assert len(x) % M == 0 and len(x) >= M and len(hist) == (P - 1) * M and M & (M - 1) == 0
    T = len(x) // M
    s = np.concatenate([hist, x])
    rev = s.reshape(T + P - 1, M, 2)[:, ::-1, :]               # rev[b, p] = block(b)[M - 1 - p]; the push's block m is b = m + P - 1
    with np.errstate(all="ignore"):
        acc = h[0][None, :, None] * rev[P - 1:P - 1 + T]           # fl(h x) for q = 0
        for q in range(1, P):
            acc = acc + h[q][None, :, None] * rev[P - 1 - q:P - 1 - q + T]
        v = np.empty_like(acc)
        v[:, bitrev(M)] = acc
        for st in range(1, M.bit_length()):
            half = 1 << (st - 1)
            lo = np.array([i for i in range(M) if not i & half])
            hi = lo + half
            w = tw[(lo & (half - 1)) * (M >> st)]
            wr, wi = w[None, :, 0], w[None, :, 1]
            e, o = v[:, lo], v[:, hi]
            z = np.stack([wr * o[..., 0] - wi * o[..., 1], wr * o[..., 1] + wi * o[..., 0]], axis=-1)
            v[:, lo] = e + z
            v[:, hi] = e - z
    assert v.dtype == np.float32
    return np.ascontiguousarray(v.transpose(1, 0, 2)), s[len(s) - (P - 1) * M:].copy()


def channel_direct(x, h, M, P):
    """the direct fp64 sum y_k[m] = sum_r h[r] s[(m + P) M - 1 - r] e^{j 2 pi k (r mod M) / M} from a zero history -> (M, T) complex128"""
    xc = np.asarray(x, np.float64).reshape(-1, 2)
    s = np.concatenate([np.zeros((P - 1) * M, np.complex128), xc[:, 0] + 1j * xc[:, 1]])
    T = len(xc) // M
    r = np.arange(M * P)
    rot = np.exp(2j * np.pi * np.outer(np.arange(M), r % M) / M)           # (k, r)
    hh = np.asarray(h, np.float64)
    return np.stack([rot @ (hh * s[(m + P) * M - 1 - r]) for m in range(T)], axis=1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_channel_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in CHANNEL_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "CHANNELISER" in header and "channel_push_kernel" in header
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(qpsk_amd.Modem.channel_reset) == ["self", "M", "P", "proto", "chan"]
    assert sig(qpsk_amd.Modem.channel)[:2] == ["self", "x"]
    assert inspect.signature(qpsk_amd.Modem.channel_reset).parameters["chan"].default is None
    assert callable(qpsk_amd.channel_twiddles) and callable(qpsk_amd.channel_prototype)
    tw, taps = (C.c_float * 8)(), (C.c_float * 16)(*([0.25] * 16))
    for M in (0, 1, 3, 6, 8192, -4):
        assert qpsk_lib.qpsk_channel_twiddles(M, tw) == QPSK_ERR_ARG, M
    assert qpsk_lib.qpsk_channel_twiddles(8, None) == QPSK_ERR_ARG
    assert b"qpsk_channel_twiddles" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_channel_reset(None, 4, 4, taps, None, 0) == QPSK_ERR_ARG
    assert b"qpsk_channel_reset" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_channel_push(None, taps, 1, tw, 0) == QPSK_ERR_ARG
    assert b"qpsk_channel_push" in qpsk_lib.qpsk_last_error()


# ------------------------------------------------------------------- 3. the twiddle table
@pytest.mark.parametrize("M", [2, 4, 8, 64, 1024, 4096])
def test_the_twiddle_table_is_cos_and_sin_rounded_to_float32_within_one_ulp(M):
    """the library rounds libm's double cos / sin of TAU j / M, numpy its own: two doubles that differ in the last place round to
    neighbouring floats at worst"""
    tw = twiddles(M)
    assert tw.shape == (M // 2, 2) and tw.dtype == np.float32
    assert bits(tw[0]).tolist() == bits(np.array([1.0, 0.0], np.float32)).tolist()
    ang = 2.0 * np.pi * np.arange(M // 2) / M
    want = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    assert np.all(np.abs(tw - want) <= np.spacing(np.abs(want)))


# ------------------------------------------------------------------- 4. the restatement against the direct fp64 sum
@pytest.mark.parametrize("M,P", [(2, 1), (4, 5), (16, 12), (64, 8), (256, 2), (1024, 3)])
def test_channel_ref_equals_the_direct_fp64_sum_within_the_bound_of_its_operation_count(M, P):
    """The bound, in complex modulus, with A = sum |h| max |x| and u = 2^-24.  Branch sums: P products and P - 1 adds on each part, at most
    P roundings on any path, so an error of at most P u sum_q |h_q| |x_q| per branch.  A stage: the table entry is a rounded double
    (u |w|), the complex product is four products and two adds (Higham: 2 sqrt(2) u |w| |o|), the add or subtract rounds each part
    (u |e +- z|) -- together below 5 u times the modulus bound of the node, and the modulus bounds of the nodes of one stage that feed one
    output add up to A (a node is a partial sum over its own branches, |w| = 1).  Hence n = P + 5 log2 M roundings' worth, and
    n u / (1 - n u) A with the higher orders"""
    import qpsk_amd
    rng = np.random.default_rng(100 * M + P)
    T = 5
    h = qpsk_amd.channel_prototype(M, P) if P > 1 else np.full(M, 1.0 / M, np.float32)
    x = rng.standard_normal((T * M, 2)).astype(np.float32)
    y, _ = channel_ref(x, None, h, M, P, twiddles(M))
    want = channel_direct(x, h, M, P)
    err = np.abs((y[..., 0].astype(np.float64) + 1j * y[..., 1]) - want).max()
    n = P + 5 * (M.bit_length() - 1)
    A = np.abs(h.astype(np.float64)).sum() * np.hypot(x[:, 0].astype(np.float64), x[:, 1]).max()
    bound = n * U / (1 - n * U) * A
    print("M %d P %d: error %.3g, bound %.3g" % (M, P, err, bound))
    assert err <= bound


def test_three_carriers_come_back_with_gain_one_in_their_channels():
    """M = 16, P = 12: tones at the centres of channels 3, 4 and 13 -> those rows have modulus 1 once the filter has filled, every other row
    stays at the prototype's stop band"""
    import qpsk_amd
    M, P, T = 16, 12, 40
    h = qpsk_amd.channel_prototype(M, P)
    n = np.arange(T * M)
    rows = []
    for k in (3, 4, 13):
        z = np.exp(2j * np.pi * k * n / M)
        y, _ = channel_ref(np.stack([z.real, z.imag], axis=1).astype(np.float32), None, h, M, P, twiddles(M))
        rows.append(np.hypot(y[:, P:, 0], y[:, P:, 1]))
        assert np.abs(rows[-1][k] - 1.0).max() < 1e-5, k
        assert np.delete(rows[-1], k, axis=0).max() < 1e-3, k


# ------------------------------------------------------------------- 5. split pushes
@pytest.mark.parametrize("M,P", [(8, 6), (64, 1), (32, 16)])
def test_a_push_split_anywhere_equals_the_single_push_bit_for_bit(M, P):
    import qpsk_amd
    rng = np.random.default_rng(M + P)
    T = 3 * P + 7
    h = rng.standard_normal(M * P).astype(np.float32) if P == 1 else qpsk_amd.channel_prototype(M, P)
    x = rng.standard_normal((T * M, 2)).astype(np.float32)
    whole, hist_whole = channel_ref(x, None, h, M, P, twiddles(M))
    cuttings = [[1] * T, [1, 1, max(P - 2, 1), max(P - 1, 1), P, T - 2 - max(P - 2, 1) - max(P - 1, 1) - P], [T - 1, 1], [2, T - 2], [P, P, T - 2 * P]]
    for cuts in cuttings:
        assert sum(cuts) == T and min(cuts) >= 1
        hist, parts, at = None, [], 0
        for c in cuts:                                            # several of these are shorter than the history: T < P - 1
            y, hist = channel_ref(x[at * M:(at + c) * M], hist, h, M, P, twiddles(M))
            parts.append(y)
            at += c
        assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(whole)), cuts
        assert np.array_equal(bits(hist), bits(hist_whole)), cuts
    assert np.array_equal(hist_whole, x[len(x) - (P - 1) * M:])


# ------------------------------------------------------------------- 6. the prototype helper
@pytest.mark.parametrize("M,P,beta", [(2, 1, 8.0), (8, 32, 16.0), (16, 12, 8.0), (64, 16, 10.0), (4096, 8, 8.0)])
def test_channel_prototype_is_symmetric_float32_with_unit_gain_at_dc(M, P, beta):
    import qpsk_amd
    h = qpsk_amd.channel_prototype(M, P, beta=beta)
    assert h.dtype == np.float32 and h.shape == (M * P,) and np.isfinite(h).all()
    assert np.array_equal(bits(h), bits(h[::-1]))
    # every tap is rounded once: the sum moves by at most u times sum |h|
    assert abs(h.astype(np.float64).sum() - 1.0) <= U * np.abs(h.astype(np.float64)).sum() + 1e-12


# ------------------------------------------------------------------- 7. the link on the restatements
# P and beta: the images the interpolator leaves of a carrier lie in the CENTRE of every other channel, attenuated by the prototype's
# stop band alone, and the receiver has no squelch -- noise-free, an empty channel is silent only while those images stay at the level of
# the fp32 rounding of the capture (2^-24 of full scale, -144 dB).  Kaiser beta = 16 over M P = 256 taps: the stop band of the float32
# taps, measured from 0.75 channel spacings on, is -152.4 dB (stopband_db below; the test asserts < -145), the pass band reaches past
# the carrier's edge at (1 + 0.35) rs / 2 = 0.17 spacings.  (P = 16, beta = 10, measured -99.9 dB, also kept the empty channels silent
# here, but only because the images of three carriers overlap there at equal level; one carrier alone would come through.)
LINK = dict(fs=9600.0, rs=2400.0, L=512, M=8, P=32, beta=16.0, carriers={2: 11.0, 3: -17.0, 6: 23.0}, nsync=32, nbytes=16, min_score=28,
            per_row=3, lead=150, gap=37, spare_blocks=3, seed=4018)


def stopband_db(h, M, start=0.75):
    H = np.abs(np.fft.fft(np.asarray(h, np.float64), 64 * len(h)))
    f = np.fft.fftfreq(len(H)) * M                                 # in channel spacings
    return 20.0 * np.log10(H[np.abs(f) >= start].max() / H[0])


def link_shape():
    """-> dict: the sync word, payloads (carriers * per_row, nbytes), the rows' length in dibits (whole blocks), the packets' columns, the
    receiver's fixed index and the delay in symbols: tx and rx filter (126 samples) and the two banks (M P - 1 + M P - 1 wideband samples
    less the M - 1 the analysis bank's output time already counts: P - 1 channel samples, exactly)"""
    k = LINK
    Cy = int(k["fs"] / k["rs"])
    nsym = k["L"] // Cy
    rng = np.random.default_rng(k["seed"])
    sync = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    payloads = rng.integers(0, 256, (len(k["carriers"]) * k["per_row"], k["nbytes"]), dtype=np.uint8)
    at = starts(k["nsync"], k["nbytes"], False, None, k["per_row"], k["lead"], k["gap"])
    need = at[-1] + k["nsync"] + body_len(k["nbytes"], False)
    row_len = (-(-need // nsym) + k["spare_blocks"]) * nsym
    lag = 126 + k["P"] - 1
    return dict(sync=sync, payloads=payloads, row_len=row_len, at=at, nsym=nsym, cycles=Cy, index=lag % Cy, delay=nsym + lag // Cy)


def link_wideband(basebands):
    """basebands {channel: (n, 2) float32 at fs} -> the capture (n M, 2) float32: every carrier turned by its offset, interpolated by M with
    the link's prototype (zero stuffing, M h, fp64) and moved to its channel's centre; then the sum"""
    import qpsk_amd
    k = LINK
    M = k["M"]
    h = qpsk_amd.channel_prototype(M, k["P"], beta=k["beta"]).astype(np.float64)
    total = None
    for ch, bb in sorted(basebands.items()):
        bb = np.asarray(bb, np.float64)
        n = len(bb)
        z = (bb[:, 0] + 1j * bb[:, 1]) * np.exp(2j * np.pi * k["carriers"][ch] * np.arange(n) / k["fs"])
        up = np.zeros(n * M, np.complex128)
        up[::M] = z
        w = np.convolve(up, M * h)[:n * M] * np.exp(2j * np.pi * ch * np.arange(n * M) / M)
        total = w if total is None else total + w
    return np.stack([total.real, total.imag], axis=1).astype(np.float32)


def link_baseband_ref(oracle, row):
    """a row of dibits through the oracle's transmit chain up to the shaped baseband: Gray map, zero stuffing, tx filter"""
    k = LINK
    Cy = int(k["fs"] / k["rs"])
    taps = oracle.rrc_make(np.float32(k["fs"]), np.float32(k["rs"]), np.float32(0.35))
    cre, cim = np.array([1.0, 0.0, 0.0, -1.0], np.float32), np.array([0.0, 1.0, -1.0, 0.0], np.float32)
    sig = np.zeros((len(row) * Cy, 2), np.float32)
    sig[::Cy, 0], sig[::Cy, 1] = cre[row], cim[row]
    oracle.rrc_fir(taps, np.zeros((127, 2), np.float32), sig)
    return sig


def link_records(packets):
    return [(p["pos"], p["rot"], p["score"], np.asarray(p["bytes"], np.uint8).tobytes(), bool(p["crc_ok"])) for p in packets]


_LINK = {}


def link_result(oracle):
    """the CPU chain, computed once -> dict(shape, rows, capture, records: per channel the deframer's packets)"""
    if _LINK:
        return _LINK
    import qpsk_amd
    from oracle.pyoracle import TIMING_FIXED
    k, shape = LINK, link_shape()
    M, P = k["M"], k["P"]
    chans = sorted(k["carriers"])
    rows, _ = frame_ref(shape["payloads"], shape["sync"], False, HALF, k["per_row"], k["lead"], k["gap"], shape["row_len"])
    capture = link_wideband({ch: link_baseband_ref(oracle, rows[i]) for i, ch in enumerate(chans)})
    h = qpsk_amd.channel_prototype(M, P, beta=k["beta"])
    y, _ = channel_ref(capture, None, h, M, P, twiddles(M))
    records = []
    for ch in range(M):
        m = oracle.modem(k["fs"], k["rs"], k["L"], timing_mode=TIMING_FIXED, fixed_index=shape["index"])
        costas = []
        for b in range(y.shape[1] // k["L"]):
            m.rx_cplx(y[ch, b * k["L"]:(b + 1) * k["L"]])
            costas.append(np.array(m.costas_frame, np.float32).reshape(-1, 2).copy())
        records.append(link_records(deframe_ref(data_rule(np.concatenate(costas)), shape["sync"], k["min_score"], k["nbytes"])))
    _LINK.update(shape=shape, rows=rows, capture=capture, proto=h, y=y, records=records)
    return _LINK


def test_three_carriers_of_one_capture_come_back_as_packets_and_the_empty_channels_stay_silent(oracle, qpsk_lib):
    """frame_ref's rows -> the oracle's transmit chain -> three carriers (two adjacent, each off its centre) in one capture -> channel_ref
    -> the oracle's stream receiver on every channel -> deframe_ref: every packet of an occupied channel comes back crc_ok with its payload
    where it was sent, and no empty channel reports a packet"""
    assert all(hasattr(qpsk_lib, name) for name in CHANNEL_SYMBOLS)
    k = LINK
    r = link_result(oracle)
    shape, chans = r["shape"], sorted(k["carriers"])
    level = stopband_db(r["proto"], k["M"])
    print("stop band of the float32 prototype from 0.75 spacings: %.1f dB" % level)
    assert level < -145.0
    assert chans == [2, 3, 6] and shape["index"] == 1 and shape["delay"] == 128 + 39
    for ch in range(k["M"]):
        got = r["records"][ch]
        if ch not in chans:
            assert got == [], ch
            continue
        i = chans.index(ch)
        assert [g[0] for g in got] == [c + shape["delay"] for c in shape["at"]], ch
        for g, payload in zip(got, shape["payloads"][i * k["per_row"]:(i + 1) * k["per_row"]]):
            assert g[4] and g[3][:k["nbytes"]] == payload.tobytes(), ch
