"""The polyphase synthesis bank (SYNTHESIS BANK in include/qpsk_hip.h: qpsk_synth_reset, qpsk_synth_push), the channeliser's transmit twin:
what can be checked without a GPU.

synth_ref() below restates the header's definition in numpy float32, vectorised over the times: the rows into the bit-reversed places of
a zero vector, the radix-2 stages one by one with the library's own table (test_channel_cpu's, the analysis bank's), then the branch
filter in the stated order over the history and the push.  Here: the ABI, the restatement against the direct fp64 sum, split pushes, the
identity that ties the bank to the analysis bank behind it, and a noise-free link of three carriers -- frame_ref's rows through the
oracle's transmit chain, synth_ref, channel_ref, the oracle's stream receiver and the numpy deframer.  The GPU tests (test_synth_gpu.py)
compare the kernels with synth_ref bit for bit.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_channel_cpu import (LINK, bitrev, bits, channel_direct, channel_ref, link_baseband_ref, link_records, link_shape, stopband_db,
                              twiddles)
from test_deframe_cpu import deframe_ref
from test_frame_cpu import HALF, frame_ref
from test_rx_data_cpu import data_rule
from test_rx_ext_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH_SYMBOLS = ("qpsk_synth_reset", "qpsk_synth_push")
QPSK_ERR_ARG = -2
U = 2.0 ** -24                       # the unit roundoff of fp32
U64 = 2.0 ** -53                     # and of fp64


# ------------------------------------------------------------------- the numpy restatement
def synth_ref(c, chan, hist, g, M, P, tw):
    """c (nsel, T, 2) float32, row i for channel chan[i] (None: all M in order), hist ((P - 1) M, 2) float32 or None (zeros): the last
    P - 1 transformed vectors, g (M P,) float32, tw (M / 2, 2) float32 -> (x (T M, 2) float32, the history after the push ((P - 1) M, 2))"""
    c = np.asarray(c, np.float32)
    g = np.asarray(g, np.float32).reshape(P, M)
    tw = np.asarray(tw, np.float32)
    chan = np.arange(M) if chan is None else np.asarray(chan)
    hist = np.zeros(((P - 1) * M, 2), np.float32) if hist is None else np.asarray(hist, np.float32).reshape(-1, 2)
    assert c.ndim == 3 and c.shape[0] == len(chan) and c.shape[1] >= 1 and c.shape[2] == 2 and M & (M - 1) == 0
    assert len(set(chan.tolist())) == len(chan) and chan.min() >= 0 and chan.max() < M and len(hist) == (P - 1) * M
    T = c.shape[1]
    v = np.zeros((T, M, 2), np.float32)                            # +0.0: a channel nobody names
    v[:, bitrev(M)[chan]] = c.transpose(1, 0, 2)
    with np.errstate(all="ignore"):
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
        s = np.concatenate([hist.reshape(P - 1, M, 2), v])         # s[b] = V_{b - (P - 1)}
        acc = g[0][None, :, None] * s[P - 1:P - 1 + T]                # fl(g V) for q = 0
        for q in range(1, P):
            acc = acc + g[q][None, :, None] * s[P - 1 - q:P - 1 - q + T]
    assert acc.dtype == np.float32
    return np.ascontiguousarray(acc.reshape(T * M, 2)), s[T:].reshape(-1, 2).copy()


def synth_direct(c, chan, g, M, P):
    """the direct fp64 sum x[n] = sum_k sum_m c_k[m] g[n - m M] e^{j 2 pi k (n - m M) / M} from a zero history -> (T M,) complex128"""
    c = np.asarray(c, np.float64)
    cc = c[..., 0] + 1j * c[..., 1]                                 # (nsel, T)
    chan = np.arange(M) if chan is None else np.asarray(chan)
    T = cc.shape[1]
    gg = np.asarray(g, np.float64).reshape(P, M)
    r = np.arange(M)
    rot = np.exp(2j * np.pi * (np.outer(chan, r) % M) / M)           # (i, r): e^{j 2 pi k n / M}, n = r mod M
    x = np.zeros((T, M), np.complex128)
    for q in range(P):                                                # n - m M = q M + r
        x[q:] += gg[q][None, :] * (cc[:, :T - q].T @ rot)
    return x.reshape(-1)


def pairs(z):
    return np.stack([z.real, z.imag], axis=-1)


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_synth_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in SYNTH_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "SYNTHESIS BANK" in header and "synth_filter_kernel" in header
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(qpsk_amd.Modem.synth_reset) == ["self", "M", "P", "proto", "chan"]
    assert sig(qpsk_amd.Modem.synth) == ["self", "rows", "pitch"]
    assert inspect.signature(qpsk_amd.Modem.synth_reset).parameters["chan"].default is None
    assert inspect.signature(qpsk_amd.Modem.synth).parameters["pitch"].default == 0
    taps, buf = (C.c_float * 16)(*([0.25] * 16)), (C.c_float * 8)()
    assert qpsk_lib.qpsk_synth_reset(None, 4, 4, taps, None, 0) == QPSK_ERR_ARG
    assert b"qpsk_synth_reset" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_synth_push(None, taps, 0, 1, buf) == QPSK_ERR_ARG
    assert b"qpsk_synth_push" in qpsk_lib.qpsk_last_error()
    # what the arguments alone decide is refused without a context too, a channel named twice among it
    twice = (C.c_int32 * 3)(1, 2, 1)
    assert qpsk_lib.qpsk_synth_reset(None, 4, 4, taps, twice, 3) == QPSK_ERR_ARG
    assert b"second time" in qpsk_lib.qpsk_last_error()


def test_the_gain_keyword_of_the_prototype_helper_is_exact():
    import qpsk_amd
    for M, P in ((8, 32), (64, 16), (4096, 8)):
        h = qpsk_amd.channel_prototype(M, P, beta=16.0)
        g = qpsk_amd.channel_prototype(M, P, beta=16.0, gain=M)
        assert g.dtype == np.float32 and np.array_equal(g.astype(np.float64), M * h.astype(np.float64))
        assert np.array_equal(bits(qpsk_amd.channel_prototype(M, P, beta=16.0, gain=1.0)), bits(h))


# ------------------------------------------------------------------- 2. the restatement against the direct fp64 sum
@pytest.mark.parametrize("full", [False, True], ids=["sparse", "full"])
@pytest.mark.parametrize("M,P", [(2, 1), (4, 5), (16, 12), (64, 8), (256, 2), (1024, 3)])
def test_synth_ref_equals_the_direct_fp64_sum_within_the_bound_of_its_operation_count(M, P, full):
    """The bound, in complex modulus, with B = max_m sum_k |c_k[m]|, G = max_r sum_q |g[q M + r]| and u = 2^-24.  A stage of the transform:
    the table entry is a rounded double (u |w|), the complex product is four products and two adds (Higham: 2 sqrt(2) u |w| |o|), the add
    or subtract rounds each part (u |e +- z|) -- together below 5 u times the modulus bound of the node, and the modulus bounds of the
    nodes of one stage that feed one output add up to B (a node is a partial sum over its own channels, |w| = 1): V_m[r] is off by at most
    5 log2 M u B, and |V_m[r]| <= B.  The branch filter: P products and P - 1 adds on each part, at most P roundings on any path, so P u
    sum_q |g_q| |V_{m - q}| <= P u G B, and the transform's error comes through times G.  Hence n = P + 5 log2 M roundings' worth, and
    n u / (1 - n u) G B with the higher orders"""
    import qpsk_amd
    rng = np.random.default_rng(100 * M + P + 7 * full)
    T = P + 4
    g = qpsk_amd.channel_prototype(M, P, gain=M) if P > 1 else np.ones(M, np.float32)
    chan = None if full else rng.permutation(M)[:max(1, M // 4)]
    nsel = M if full else len(chan)
    c = rng.standard_normal((nsel, T, 2)).astype(np.float32)
    x, _ = synth_ref(c, chan, None, g, M, P, twiddles(M))
    want = synth_direct(c, chan, g, M, P)
    err = np.abs((x[:, 0].astype(np.float64) + 1j * x[:, 1]) - want).max()
    n = P + 5 * (M.bit_length() - 1)
    B = np.hypot(c[..., 0].astype(np.float64), c[..., 1]).sum(axis=0).max()
    G = np.abs(g.astype(np.float64)).reshape(P, M).sum(axis=0).max()
    bound = n * U / (1 - n * U) * G * B
    print("M %d P %d nsel %d: error %.3g, bound %.3g, ratio %.3g" % (M, P, nsel, err, bound, err / bound))
    assert err <= bound


def test_an_unselected_channel_contributes_exact_zeros_and_a_lone_channel_is_its_tone():
    """one row on channel k of M = 16: every V_m[r] is c[m] times a product of table entries, and with c = 1 the output is g[n] times the
    tone of channel k to the table's precision; with no input at all every sample is +0.0"""
    import qpsk_amd
    M, P, T, k = 16, 4, 9, 5
    g = qpsk_amd.channel_prototype(M, P, gain=M)
    x, hist = synth_ref(np.zeros((2, T, 2), np.float32), [3, k], None, g, M, P, twiddles(M))
    assert not bits(x).any() and not bits(hist).any()
    one = np.zeros((1, T, 2), np.float32)
    one[0, 0, 0] = 1.0
    x, _ = synth_ref(one, [k], None, g, M, P, twiddles(M))
    n = np.arange(M * P)
    want = g.astype(np.float64) * np.exp(2j * np.pi * k * n / M)
    assert np.abs((x[:M * P, 0] + 1j * x[:M * P, 1]) - want).max() <= 5 * 4 * U * np.abs(g).max()
    assert not bits(x[M * P:]).any()


# ------------------------------------------------------------------- 3. split pushes
@pytest.mark.parametrize("M,P", [(8, 6), (64, 1), (32, 16)])
def test_a_push_split_anywhere_equals_the_single_push_bit_for_bit(M, P):
    import qpsk_amd
    rng = np.random.default_rng(M + P)
    T = 3 * P + 7
    g = rng.standard_normal(M * P).astype(np.float32) if P == 1 else qpsk_amd.channel_prototype(M, P, gain=M)
    chan = rng.permutation(M)[:M // 2 + 1]
    c = rng.standard_normal((len(chan), T, 2)).astype(np.float32)
    whole, hist_whole = synth_ref(c, chan, None, g, M, P, twiddles(M))
    cuttings = [[1] * T, [1, 1, max(P - 2, 1), max(P - 1, 1), P, T - 2 - max(P - 2, 1) - max(P - 1, 1) - P], [T - 1, 1], [2, T - 2], [P, P, T - 2 * P]]
    for cuts in cuttings:
        assert sum(cuts) == T and min(cuts) >= 1
        hist, parts, at = None, [], 0
        for n in cuts:                                            # several of these are shorter than the history: T < P - 1
            x, hist = synth_ref(c[:, at:at + n], chan, hist, g, M, P, twiddles(M))
            parts.append(x)
            at += n
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)), cuts
        assert np.array_equal(bits(hist), bits(hist_whole)), cuts
    assert hist_whole.shape == ((P - 1) * M, 2)


# ------------------------------------------------------------------- 4. the twin identity
@pytest.mark.parametrize("M,P,k", [(8, 6, 3), (16, 4, 0), (16, 4, 15), (64, 3, 33)])
def test_the_analysis_of_the_synthesis_is_the_closed_form_of_the_header(M, P, k):
    """fp64, one row on channel k: the direct analysis of the direct synthesis is
        y_k[m'] = e^{j 2 pi k (M - 1) / M} sum_m c_k[m] (h * g)[(m' - m) M + M - 1]
    and for symmetric prototypes (h * g) is symmetric about M P - 1, so the samples (h * g)[j M + M - 1] are symmetric about j = P - 1:
    a delay of exactly P - 1 channel samples, and e^{j 2 pi k (M - 1) / M} = e^{-j 2 pi k / M}, a turn of -k / M.
    The bound is fp64's rounding over the operation count, times sum |h| sum |g| max |c|: both sides are sums of at most M P + P terms
    (M P in the analysis or the convolution, P in the synthesis or the closed form's sum), each term a product of at most four factors
    (3 roundings), and two rotations whose arguments reach 2 pi M before the reduction (an error of u 2 pi M each, plus 2 for exp):
    n = 2 (M P + P) + 6 + 2 (2 pi M + 2)"""
    import qpsk_amd
    rng = np.random.default_rng(M * P + k)
    T = 3 * P + 2
    h = qpsk_amd.channel_prototype(M, P).astype(np.float64)
    g = qpsk_amd.channel_prototype(M, P, gain=M).astype(np.float64)
    c = rng.standard_normal((1, T, 2))
    x = synth_direct(c, [k], g, M, P)
    y = channel_direct(pairs(x), h, M, P)[k]                         # (T,)
    hg = np.convolve(h, g)
    taps = np.array([hg[j * M + M - 1] for j in range(2 * P - 1)])    # (h * g)[j M + M - 1], j = m' - m
    cc = c[0, :, 0] + 1j * c[0, :, 1]
    want = np.exp(2j * np.pi * k * (M - 1) / M) * np.convolve(cc, taps)[:T]
    n = 2 * (M * P + P) + 6 + 2 * (2 * np.pi * M + 2)
    bound = n * U64 / (1 - n * U64) * np.abs(h).sum() * np.abs(g).sum() * np.abs(cc).max()
    err = np.abs(y - want).max()
    print("M %d P %d k %d: error %.3g, bound %.3g, ratio %.3g" % (M, P, k, err, bound, err / bound))
    assert err <= bound
    assert np.argmax(np.abs(taps)) == P - 1 and np.allclose(taps, taps[::-1], rtol=0, atol=bound)
    assert abs(np.exp(2j * np.pi * k * (M - 1) / M) - np.exp(-2j * np.pi * k / M)) <= 4 * np.pi * M * U64
    # measured, no criterion: the fp32 round trip of a narrow-band row through synth_ref and channel_ref against the row delayed P - 1 and
    # turned by e^{-j 2 pi k / M} -- the deviation is the prototypes' pass-band droop
    t = np.arange(8 * P)
    row = np.exp(2j * np.pi * 0.01 * t)
    xs, _ = synth_ref(pairs(row)[None].astype(np.float32), [k], None, g.astype(np.float32), M, P, twiddles(M))
    ys, _ = channel_ref(xs, None, h.astype(np.float32), M, P, twiddles(M))
    back = (ys[k, 2 * P:, 0] + 1j * ys[k, 2 * P:, 1]) * np.exp(2j * np.pi * k / M)
    print("  fp32 round trip of a narrow-band row: deviation %.3g of full scale" % np.abs(back - row[P + 1:len(row) - P + 1]).max())


# ------------------------------------------------------------------- 5. the link on the restatements
_LINK = {}


def synth_link_result(oracle):
    """the CPU chain, computed once -> dict(shape, rows, basebands (3, n, 2), gain prototype g, analysis prototype proto, capture, y,
    records: per channel the deframer's packets).  LINK's shape with the carriers at their channels' centres: the bank places them"""
    if _LINK:
        return _LINK
    import qpsk_amd
    from oracle.pyoracle import TIMING_FIXED
    k, shape = LINK, link_shape()
    M, P = k["M"], k["P"]
    chans = sorted(k["carriers"])
    rows, _ = frame_ref(shape["payloads"], shape["sync"], False, HALF, k["per_row"], k["lead"], k["gap"], shape["row_len"])
    basebands = np.stack([link_baseband_ref(oracle, rows[i]) for i in range(len(chans))])
    h = qpsk_amd.channel_prototype(M, P, beta=k["beta"])
    g = qpsk_amd.channel_prototype(M, P, beta=k["beta"], gain=M)
    capture, _ = synth_ref(basebands, chans, None, g, M, P, twiddles(M))
    y, _ = channel_ref(capture, None, h, M, P, twiddles(M))
    records = []
    for ch in range(M):
        m = oracle.modem(k["fs"], k["rs"], k["L"], timing_mode=TIMING_FIXED, fixed_index=shape["index"])
        costas = []
        for b in range(y.shape[1] // k["L"]):
            m.rx_cplx(y[ch, b * k["L"]:(b + 1) * k["L"]])
            costas.append(np.array(m.costas_frame, np.float32).reshape(-1, 2).copy())
        records.append(link_records(deframe_ref(data_rule(np.concatenate(costas)), shape["sync"], k["min_score"], k["nbytes"])))
    _LINK.update(shape=shape, rows=rows, basebands=basebands, proto=h, g=g, capture=capture, y=y, records=records)
    return _LINK


def test_three_rows_through_both_banks_come_back_as_packets_where_they_were_sent(oracle, qpsk_lib):
    """frame_ref's rows -> the oracle's transmit chain -> synth_ref on channels 2, 3 and 6 of M = 8 with g = M h -> channel_ref -> the
    oracle's stream receiver on every channel -> deframe_ref.  All nine packets come back crc_ok at `at + 167` -- link_shape()'s delay,
    which already counts the two banks' P - 1 channel samples, with its index 1 -- every sync word matches in 32 of 32 dibits, the
    rotations are the banks' turn of -k / M (-1/4, -3/8, -3/4 of a circle for k = 2, 3, 6) as the loop settles on it: 3, 2 and 1; the
    five empty channels deliver nothing"""
    assert all(hasattr(qpsk_lib, name) for name in SYNTH_SYMBOLS)
    k = LINK
    r = synth_link_result(oracle)
    shape, chans = r["shape"], sorted(k["carriers"])
    assert np.array_equal(r["g"].astype(np.float64), k["M"] * r["proto"].astype(np.float64))
    assert stopband_db(r["proto"], k["M"]) < -145.0
    assert chans == [2, 3, 6] and shape["index"] == 1 and shape["delay"] == 167
    assert len(r["capture"]) == k["M"] * r["basebands"].shape[1]
    rotations = {2: 3, 3: 2, 6: 1}
    for ch in range(k["M"]):
        got = r["records"][ch]
        if ch not in chans:
            assert got == [], ch
            continue
        i = chans.index(ch)
        assert [g[0] for g in got] == [c + 167 for c in shape["at"]], ch
        assert [g[1] for g in got] == [rotations[ch]] * k["per_row"], ch
        assert [g[2] for g in got] == [32] * k["per_row"], ch
        for g, payload in zip(got, shape["payloads"][i * k["per_row"]:(i + 1) * k["per_row"]]):
            assert g[4] and g[3][:k["nbytes"]] == payload.tobytes(), ch
