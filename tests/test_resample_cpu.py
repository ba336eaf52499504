"""The batched rational resampler (RESAMPLER in include/qpsk_hip.h: qpsk_resample_reset, qpsk_resample_need, qpsk_resample_push): what can
be checked without a GPU.

resample_ref() below restates the header's definition in numpy float32, vectorised over the outputs and over any leading stream axes:
the position arithmetic with floor division, then the P products and P - 1 additions one operation at a time in the stated order.  Here:
the restatement against the direct fp64 sum (zero stuffing, convolution, decimation) within a bound derived from its operation count, runs
cut at many places, the host's position arithmetic against a brute-force count, the prototype helper and its pass and stop band, tones, and
a noise-free link: frame_ref's rows through the oracle's transmit chain at 9600 Hz, up to 12 kS/s by 5 / 4, back by 4 / 5, through the
oracle's stream receiver and the numpy deframer.  The GPU tests (test_resample_gpu.py) compare the kernel with resample_ref bit for bit.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_channel_cpu import LINK as CHANNEL_LINK, link_baseband_ref, link_records
from test_deframe_cpu import deframe_ref
from test_frame_cpu import HALF, body_len, frame_ref, starts
from test_rx_data_cpu import data_rule
from test_rx_ext_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLE_SYMBOLS = ("qpsk_resample_reset", "qpsk_resample_need", "qpsk_resample_push")
QPSK_ERR_ARG = -2
U = 2.0 ** -24                       # the unit roundoff of fp32
# the ratios of the cuts, and their taps per branch
RATIOS = [(5, 4, 4), (4, 5, 3), (3, 7, 2), (7, 3, 5), (1, 1, 1), (1, 1, 3), (2, 1, 1), (1, 3, 4), (160, 147, 2)]


# ------------------------------------------------------------------- the numpy restatement
def need_ref(r, L, D, nout):
    """K: the inputs the next nout outputs consume at the position r (Python's // is the floor division of the definition)"""
    return (r + (nout - 1) * D) // L + 1


def resample_ref(x, state, h, L, D, P, nout):
    """x (..., K, 2) float32, the next K = need_ref(r, L, D, nout) samples of every stream; state = (history (..., P, 2) float32, r) or None
    (after a reset: zeros, 0); h (L P,) float32 -> (y (..., nout, 2) float32, the state after the push)"""
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float32).reshape(-1)
    assert x.ndim >= 2 and x.shape[-1] == 2 and len(h) == L * P and nout >= 1
    hist, r = (np.zeros(x.shape[:-2] + (P, 2), np.float32), 0) if state is None else state
    assert hist.shape == x.shape[:-2] + (P, 2) and (r == 0 or D - L <= r < D)      # 0: after a reset
    K = need_ref(r, L, D, nout)
    assert x.shape[-2] == K, (x.shape, K)
    s = np.concatenate([np.asarray(hist, np.float32), x], axis=-2)          # sample i of the push is s[P + i]; the history is i = -P .. -1
    t = r + np.arange(nout, dtype=np.int64) * D
    i, b = t // L, t % L                                                     # floor division: i >= -1
    assert i.min() >= -1 and i.max() == K - 1
    with np.errstate(all="ignore"):
        acc = h[b][:, None] * s[..., P + i, :]                               # fl(h x) for q = 0
        for q in range(1, P):
            acc = acc + h[q * L + b][:, None] * s[..., P + i - q, :]
    assert acc.dtype == np.float32
    return acc, (s[..., K:, :].copy(), r + nout * D - K * L)


def run_ref(x, h, L, D, P, nouts, state=None):
    """x (..., n, 2): consecutive pushes of nouts outputs, each fed the samples it needs from x in turn -> (y (..., sum nouts, 2), the
    state, the K of every push)"""
    at, parts, Ks = 0, [], []
    for nout in nouts:
        K = need_ref(0 if state is None else state[1], L, D, nout)
        y, state = resample_ref(x[..., at:at + K, :], state, h, L, D, P, nout)
        parts.append(y)
        Ks.append(K)
        at += K
    return np.concatenate(parts, axis=-2), state, Ks


def resample_direct(x, h, L, D, nout, absolute=False):
    """the definition's other form in fp64, from a zero history: v = h * (s zero-stuffed by L), y[n] = v[n D] -> (nout,) complex128;
    absolute: sum |h| |s| part by part instead, the scale of the rounding bound -> (nout, 2)"""
    z = np.asarray(x, np.float64)
    hh = np.asarray(h, np.float64)
    if absolute:
        z, hh = np.abs(z), np.abs(hh)
    up = np.zeros((len(z) * L, 2))
    up[::L] = z
    v = np.stack([np.convolve(up[:, c], hh) for c in (0, 1)], axis=1)
    y = v[np.arange(nout) * D]
    return y if absolute else y[:, 0] + 1j * y[:, 1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def taps(L, P, seed=0):
    """taps with no symmetry and no zero among them: a wrong branch or a wrong order shows"""
    rng = np.random.default_rng(1000 * L + P + seed)
    h = (rng.standard_normal(L * P) / np.sqrt(P)).astype(np.float32)
    assert np.all(h != 0.0)
    return h


def total_in(L, D, nout):
    """the inputs nout outputs consume from a reset"""
    return need_ref(0, L, D, nout)


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_resample_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in RESAMPLE_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "RESAMPLER" in header and "resample_push_kernel" in header
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(qpsk_amd.Modem.resample_reset) == ["self", "nstreams", "L", "D", "P", "proto"]
    assert sig(qpsk_amd.Modem.resample_need) == ["self", "nout"]
    assert sig(qpsk_amd.Modem.resample) == ["self", "rows", "nout", "pitch", "out_pitch"]
    assert sig(qpsk_amd.resample_prototype) == ["L", "D", "P", "beta", "gain"]
    L = qpsk_lib
    err = lambda: L.qpsk_last_error()      # noqa: E731
    h = (C.c_float * 64)(*([0.25] * 64))
    buf, out = (C.c_float * 64)(), (C.c_float * 64)()
    reset = lambda S, LL, D, P, hp: L.qpsk_resample_reset(None, S, LL, D, P, hp)      # noqa: E731
    push = lambda i, ip, nin, nout, o, op: L.qpsk_resample_push(None, i, ip, nin, nout, o, op)      # noqa: E731
    # a NULL context is refused last: good arguments reach it ...
    assert reset(3, 5, 4, 4, h) == QPSK_ERR_ARG and b"qpsk_resample_reset: null context" in err()
    assert L.qpsk_resample_need(None, 7) == QPSK_ERR_ARG and b"qpsk_resample_need: null context" in err()
    assert push(buf, 0, 4, 5, out, 0) == QPSK_ERR_ARG and b"qpsk_resample_push: null context" in err()
    assert push(None, 0, 0, 1, out, 0) == QPSK_ERR_ARG and b"null context" in err()             # nin = 0 with a NULL d_in is legal
    # ... and what the arguments alone decide is refused before it
    for S in (0, -1, 65537):
        assert reset(S, 5, 4, 4, h) == QPSK_ERR_ARG and b"nstreams" in err(), S
    for LL in (0, -5, 513):
        assert reset(3, LL, 4, 1, h) == QPSK_ERR_ARG and b"L = " in err(), LL
    for D in (0, -4, 4097):
        assert reset(3, 5, D, 4, h) == QPSK_ERR_ARG and b"D = " in err(), D
    for P in (0, -1, 33):
        assert reset(3, 1, 4, P, h) == QPSK_ERR_ARG and b"P = " in err(), P
    assert reset(3, 5, 4, 4, None) == QPSK_ERR_ARG and b"null h_proto" in err()
    for bad in (np.nan, np.inf, -np.inf):
        hb = (C.c_float * 64)(*([0.25] * 64))
        hb[19] = bad
        assert reset(3, 5, 4, 4, hb) == QPSK_ERR_ARG and b"h_proto[19]" in err(), bad
        hb[19], hb[20] = 0.25, bad                                                               # beyond the L P = 20 taps: not looked at
        assert reset(3, 5, 4, 4, hb) == QPSK_ERR_ARG and b"null context" in err(), bad
    for nout in (0, -1, (1 << 24) + 1):
        assert L.qpsk_resample_need(None, nout) == QPSK_ERR_ARG and b"nout" in err(), nout
        assert push(buf, 0, 4, nout, out, 0) == QPSK_ERR_ARG and b"nout" in err(), nout
    assert push(buf, 0, 4, 5, None, 0) == QPSK_ERR_ARG and b"null d_out" in err()
    assert push(None, 0, 4, 5, out, 0) == QPSK_ERR_ARG and b"null d_in" in err()
    assert push(buf, 0, -1, 5, out, 0) == QPSK_ERR_ARG and b"nin" in err()
    for ip in (3, -1):
        assert push(buf, ip, 4, 5, out, 0) == QPSK_ERR_ARG and b"in_pitch" in err(), ip
    for op in (4, -1):
        assert push(buf, 0, 4, 5, out, op) == QPSK_ERR_ARG and b"out_pitch" in err(), op
    assert push(buf, 4, 4, 5, out, 5) == QPSK_ERR_ARG and b"null context" in err()               # pitches equal to the rows are good


# ------------------------------------------------------------------- 3. the restatement against the direct fp64 sum
@pytest.mark.parametrize("L,D,P", [(5, 4, 4), (4, 5, 16), (3, 7, 2), (7, 3, 5), (1, 1, 1), (2, 1, 8), (1, 3, 32), (160, 147, 2), (4, 6, 7)])
def test_resample_ref_equals_the_direct_fp64_sum_within_the_bound_of_its_operation_count(L, D, P):
    """Per part, y = sum of P products: every product is rounded once and takes part in at most P - 1 rounded additions, the first product
    in P - 1 as well -- at most P roundings on any path from a product to the result, so (Higham, inner products)
    |fl(y) - y| <= gamma_P sum_q |h_q| |s_q|, gamma_P = P u / (1 - P u), u = 2^-24.  The fp64 sums on the right add below 2^-29 of that
    (P 2^-53 relative): a factor 1 + 2^-20 covers them"""
    rng = np.random.default_rng(100 * L + 10 * D + P)
    nout = 300
    x = rng.standard_normal((total_in(L, D, nout), 2)).astype(np.float32)
    h = taps(L, P)
    y, _ = resample_ref(x, None, h, L, D, P, nout)
    want = resample_direct(x, h, L, D, nout)
    scale = resample_direct(x, h, L, D, nout, absolute=True)
    gamma = P * U / (1 - P * U)
    err = np.abs(np.stack([y[:, 0] - want.real, y[:, 1] - want.imag], axis=1))
    bound = gamma * scale * (1 + 2.0 ** -20)
    print("L %d D %d P %d: largest error %.3g, its bound %.3g, largest error / bound %.3f" % (L, D, P, err.max(), bound[np.unravel_index(err.argmax(), err.shape)], (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert np.abs(want).max() > 0.1                                # the comparison is not of zeros


# ------------------------------------------------------------------- 4. cuts
@pytest.mark.parametrize("L,D,P", RATIOS, ids=["%d/%d-P%d" % r for r in RATIOS])
def test_a_run_cut_anywhere_equals_the_single_push_bit_for_bit(L, D, P):
    rng = np.random.default_rng(L + 7 * D + 31 * P)
    total = 6 * P * max(L, D) // min(L, D) + 97
    x = rng.standard_normal((2, total_in(L, D, total) + 3, 2)).astype(np.float32)      # two streams; three samples stay unconsumed
    h = taps(L, P)
    whole, state_whole, _ = run_ref(x, h, L, D, P, [total])
    cuttings = [[1] * total, [total - 1, 1], [1, total - 1], [2, 3, total - 5]]
    for _ in range(12):
        cuts = []
        while sum(cuts) < total:
            cuts.append(int(min(rng.choice([1, 1, 2, 3, P, 2 * P + 1, 40]), total - sum(cuts))))
        cuttings.append(cuts)
    seen_K = set()
    for cuts in cuttings:
        assert sum(cuts) == total and min(cuts) >= 1
        y, state, Ks = run_ref(x, h, L, D, P, cuts)
        seen_K |= set(Ks)
        assert np.array_equal(bits(y), bits(whole)), cuts
        assert np.array_equal(bits(state[0]), bits(state_whole[0])) and state[1] == state_whole[1], cuts
    # the pieces that matter: nout = 1 (above, in every cutting), K < P where P > 1, and K = 0 where L > D
    assert (0 in seen_K) == (L > D), seen_K
    assert P == 1 or any(0 < K < P for K in seen_K), seen_K
    consumed = total_in(L, D, total)
    assert np.array_equal(state_whole[0], np.concatenate([np.zeros((2, P, 2), np.float32), x[:, :consumed]], axis=1)[:, -P:])


# ------------------------------------------------------------------- 5. the host's position arithmetic
def c_div(a, b):
    """C's division, which truncates towards zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def need_host(r, L, D, nout):
    """qpsk_resample_need's arithmetic as api_resample.cpp writes it, with C's truncating division: floor(a / L) for a negative a is
    -((-a + L - 1) / L)"""
    a = r + (nout - 1) * D
    return (c_div(a, L) if a >= 0 else -c_div(-a + L - 1, L)) + 1


@pytest.mark.parametrize("L,D", [(5, 4), (4, 5), (3, 7), (7, 3), (1, 1), (2, 1), (1, 3), (160, 147), (512, 1), (1, 4096), (512, 511), (4, 6), (511, 4096)])
def test_the_need_equals_a_brute_force_count_and_r_stays_in_its_interval(L, D):
    """brute force: output n reads up to input (n D) div L, counted from the reset with counters that grow; the carried r never does"""
    rng = np.random.default_rng(L * 4099 + D)
    n0 = c0 = r = 0
    seen = set()
    for _ in range(3000):
        nout = int(rng.choice([1, 1, 2, 3, 5, 17, 512, 4097]))
        last = ((n0 + nout - 1) * D) // L                      # the input index of the push's last output
        K = last + 1 - c0
        assert need_ref(r, L, D, nout) == K and need_host(r, L, D, nout) == K
        assert K >= 0
        n0, c0, r = n0 + nout, c0 + K, r + nout * D - K * L
        assert r == n0 * D - c0 * L and D - L <= r < D
        seen.add(r)
    assert (0 in {need_ref(rr, L, D, 1) for rr in seen}) == (L > D)
    g = np.gcd(L, D)
    assert all(rr % g == 0 for rr in seen) and len(seen) <= L // g


# ------------------------------------------------------------------- 6. the prototype helper
def response(h, f):
    """|H(f)| / |H(0)| of the taps in fp64 at the frequencies f, cycles per interpolated sample"""
    hh = np.asarray(h, np.float64)
    H = np.exp(-2j * np.pi * np.outer(np.asarray(f, np.float64), np.arange(len(hh)))) @ hh
    return np.abs(H) / abs(hh.sum())


def band_edges(L, D, P, beta):
    """what resample_prototype's docstring says: the cut-off and the half width of the transition band, cycles per interpolated sample"""
    return 1.0 / (2.0 * max(L, D)), np.sqrt(1.0 + (beta / np.pi) ** 2) / (L * P)


def band_levels(h, L, D, P, beta, points=4000):
    """measured from the taps on a dense grid: the pass band's largest deviation from gain 1 (up to cut-off - width), the stop band's
    largest gain (from cut-off + width to half the interpolated rate)"""
    fc, w = band_edges(L, D, P, beta)
    ripple = np.abs(response(h, np.linspace(0.0, max(fc - w, 0.0), points)) - 1.0).max()
    stop = response(h, np.linspace(fc + w, 0.5, points)).max() if fc + w < 0.5 else 0.0
    return ripple, stop


@pytest.mark.parametrize("L,D,P,beta,gain", [(5, 4, 16, 10.0, None), (4, 5, 18, 10.0, None), (160, 147, 16, 10.0, None), (1, 3, 32, 10.0, None),
                                             (2, 1, 8, 6.0, 1.0), (1, 8, 16, 8.0, 3.0), (1, 1, 1, 10.0, None), (512, 511, 32, 10.0, None)])
def test_resample_prototype_is_symmetric_float32_with_its_gain_and_the_stop_band_the_docstring_says(L, D, P, beta, gain):
    """The stop band: Kaiser's rule puts a window of shape beta at A = beta / 0.1102 + 8.7 dB (the rule's own fit is good to about a dB; 3 dB
    are allowed here), and the docstring says it begins one main-lobe half width beyond the cut-off, where the response -- the window's
    spectrum integrated over the ideal pass band -- has just left its main lobe.  At the cut-off itself an ideal low-pass through any
    symmetric window stands at one half.  The float32 rounding of the taps lies at 2^-24 sqrt(L P) of the gain at worst, 40 dB below"""
    import qpsk_amd
    h = qpsk_amd.resample_prototype(L, D, P, beta=beta) if gain is None else qpsk_amd.resample_prototype(L, D, P, beta=beta, gain=gain)
    want = float(L if gain is None else gain)
    assert h.dtype == np.float32 and h.shape == (L * P,) and np.isfinite(h).all()
    assert np.array_equal(bits(h), bits(h[::-1]))
    # every tap is rounded once: the sum moves by at most u times sum |h|
    assert abs(h.astype(np.float64).sum() - want) <= U * np.abs(h.astype(np.float64)).sum() + 1e-12 * want
    if L * P < 32:
        return                                                     # too few taps for a band structure
    fc, w = band_edges(L, D, P, beta)
    A = beta / 0.1102 + 8.7
    ripple, stop = band_levels(h, L, D, P, beta)
    half = response(h, [fc])[0]
    inside = response(h, [fc + 0.5 * w])[0]
    print("L %d D %d P %d beta %g: cut-off %.5f, width %.5f, stop band %.1f dB (Kaiser %.1f), ripple %.2e, at the cut-off %.4f, half way %.1f dB"
          % (L, D, P, beta, fc, w, 20 * np.log10(stop), -A, ripple, half, 20 * np.log10(inside)))
    assert 20 * np.log10(stop) <= -(A - 3.0)                      # the stop band has begun at cut-off + width
    assert 20 * np.log10(inside) > -(A - 3.0)                     # ... and not half a width sooner
    assert abs(half - 0.5) < 0.01


# ------------------------------------------------------------------- 7. tones
def tone(f, n):
    z = np.exp(2j * np.pi * f * np.arange(n))
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


@pytest.mark.parametrize("L,D,P", [(5, 4, 16), (4, 5, 18), (2, 5, 32), (1, 3, 32), (160, 147, 16)])
def test_tones_in_the_pass_band_come_back_with_gain_one_and_tones_in_the_stop_band_stay_below_its_level(L, D, P):
    """A tone of f cycles per input sample, zero-stuffed by L, is L images of amplitude 1 / L at (f + k) / L cycles per interpolated
    sample; the filter (gain L at 0) weighs image k by |H((f + k) / L)| / H(0), and the decimation only moves them.  With the tone in the
    pass band (|f| / L below cut-off - width) the image k = 0 has gain within the pass band's ripple of 1 and the L - 1 others lie in the
    stop band: | |y| - 1 | <= ripple + (L - 1) stop.  With every image in the stop band |y| <= L stop.  Both levels are measured from the
    taps above; the fp32 arithmetic adds at most gamma_P max_b sum_q |h[q L + b]| per part, the float32 tone itself u of that"""
    import qpsk_amd
    beta = 10.0
    h = qpsk_amd.resample_prototype(L, D, P, beta=beta)
    fc, w = band_edges(L, D, P, beta)
    ripple, stop = band_levels(h, L, D, P, beta)
    rounding = (P * U / (1 - P * U) + U) * np.abs(h.astype(np.float64)).reshape(P, L).sum(axis=0).max() * np.sqrt(2.0)
    nout = 40 * P
    settle = P * L // D + 2                                        # outputs before it reach back before the tone's start: i = n D div L < P
    passed = [s * L * (fc - w) * frac for frac in (0.05, 0.5, 0.98) for s in (1.0, -1.0)]
    worst = 0.0
    for f in passed:
        y, _ = resample_ref(tone(f, total_in(L, D, nout)), None, h, L, D, P, nout)
        mod = np.hypot(y[settle:, 0].astype(np.float64), y[settle:, 1])
        worst = max(worst, np.abs(mod - 1.0).max())
    print("L %d D %d P %d: pass band ripple %.2e, stop band %.2e, rounding %.2e; tones off gain one by %.2e at most" % (L, D, P, ripple, stop, rounding, worst))
    assert worst <= ripple + (L - 1) * stop + rounding
    assert ripple + (L - 1) * stop + rounding < 1e-2              # the check means something: L - 1 = 159 images at -100 dB are 1.5e-3
    # the stop band: only where it begins below half the INPUT rate, i.e. with enough decimation
    lo = L * (fc + w)
    if lo < 0.5:
        for f in (lo, 0.5 * (lo + 0.5), 0.5, -0.5 * (lo + 0.5)):
            images = ((f + np.arange(L)) / L + 0.5) % 1.0 - 0.5    # cycles per interpolated sample, wrapped to [-0.5, 0.5)
            assert np.all(np.abs(images) >= fc + w - 1e-12), f
            y, _ = resample_ref(tone(f, total_in(L, D, nout)), None, h, L, D, P, nout)
            mod = np.hypot(y[settle:, 0].astype(np.float64), y[settle:, 1])
            assert mod.max() <= L * stop + rounding, f
    else:
        assert (L, D, P) in [(5, 4, 16), (4, 5, 18), (160, 147, 16)]


# ------------------------------------------------------------------- 8. the link on the restatements
# 9600 Hz -> 12 kS/s by 5 / 4 (P1 taps per branch) -> 9600 Hz by 4 / 5 (P2): both filters run at 48 kS/s, are symmetric of 5 P1 and 4 P2
# taps, so the round trip delays by ((5 P1 - 1) + (4 P2 - 1)) / 2 samples at 48 kS/s: 75 = exactly 15 modem samples.  The carrier's edge
# lies at (1 + 0.35) 2400 / 2 = 1620 Hz, both pass bands reach beyond 2500 Hz (cut-off 4800 Hz less 3.34 / 80 and 3.34 / 72 of 48 kHz)
LINK = dict(fs=9600.0, rs=2400.0, L=512, up=(5, 4, 16), down=(4, 5, 18), beta=10.0, nstreams=3, nsync=32, nbytes=16, min_score=28, per_row=3,
            lead=150, gap=37, spare_blocks=3, seed=4020, up_blocks=(333, 1, 640, 77, 2, 1200))


def link_shape():
    """-> dict: the sync word, payloads (nstreams * per_row, nbytes), the rows' length in dibits (whole blocks), the packets' columns, the
    receiver's fixed index and the delay in symbols: tx and rx filter (126 samples) and the two resamplers' round trip, derived here"""
    k = LINK
    assert (k["fs"], k["rs"]) == (CHANNEL_LINK["fs"], CHANNEL_LINK["rs"])      # link_baseband_ref shapes at these
    Cy = int(k["fs"] / k["rs"])
    nsym = k["L"] // Cy
    (L1, D1, P1), (L2, D2, P2) = k["up"], k["down"]
    assert L1 * L2 == D1 * D2                                      # the two ratios undo each other
    assert L1 * D2 == L1 * L1                                      # ... and both filters run at L1 times the modem's rate (48 kS/s)
    common = L1
    both = (L1 * P1 - 1) + (L2 * P2 - 1)                           # twice the round trip, samples at the interpolated rate
    assert both % (2 * common) == 0                                # a whole number of modem samples
    resampled = both // (2 * common)
    rng = np.random.default_rng(k["seed"])
    sync = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    payloads = rng.integers(0, 256, (k["nstreams"] * k["per_row"], k["nbytes"]), dtype=np.uint8)
    at = starts(k["nsync"], k["nbytes"], False, None, k["per_row"], k["lead"], k["gap"])
    need = at[-1] + k["nsync"] + body_len(k["nbytes"], False)
    row_len = (-(-need // nsym) + k["spare_blocks"]) * nsym
    lag = 126 + resampled
    return dict(sync=sync, payloads=payloads, row_len=row_len, at=at, nsym=nsym, cycles=Cy, resampled=resampled, index=lag % Cy,
                delay=nsym + lag // Cy)


def up_blocks(n_up):
    """the outputs of the pushes at 12 kS/s: LINK's irregular lengths over and over, so that K varies from push to push"""
    out, j = [], 0
    while sum(out) < n_up:
        out.append(min(LINK["up_blocks"][j % len(LINK["up_blocks"])], n_up - sum(out)))
        j += 1
    return out


_LINK = {}


def link_result(oracle):
    """the CPU chain, computed once -> dict(shape, rows, baseband (S, n, 2), up (S, n 5 / 4, 2), down (S, n, 2), the K of every push,
    records: per stream the deframer's packets)"""
    if _LINK:
        return _LINK
    import qpsk_amd
    from oracle.pyoracle import TIMING_FIXED
    k, shape = LINK, link_shape()
    (L1, D1, P1), (L2, D2, P2) = k["up"], k["down"]
    rows, _ = frame_ref(shape["payloads"], shape["sync"], False, HALF, k["per_row"], k["lead"], k["gap"], shape["row_len"])
    bb = np.stack([link_baseband_ref(oracle, row) for row in rows])
    n = bb.shape[1]
    assert n % D1 == 0 and n % k["L"] == 0
    h1 = qpsk_amd.resample_prototype(L1, D1, P1, beta=k["beta"])
    h2 = qpsk_amd.resample_prototype(L2, D2, P2, beta=k["beta"])
    n_up = n * L1 // D1
    assert total_in(L1, D1, n_up) == n and total_in(L2, D2, n) <= n_up
    up, _, K1 = run_ref(bb, h1, L1, D1, P1, up_blocks(n_up))
    down, _, K2 = run_ref(up, h2, L2, D2, P2, [k["L"]] * (n // k["L"]))
    records = []
    for s in range(k["nstreams"]):
        m = oracle.modem(k["fs"], k["rs"], k["L"], timing_mode=TIMING_FIXED, fixed_index=shape["index"])
        costas = []
        for b in range(n // k["L"]):
            m.rx_cplx(down[s, b * k["L"]:(b + 1) * k["L"]])
            costas.append(np.array(m.costas_frame, np.float32).reshape(-1, 2).copy())
        records.append(link_records(deframe_ref(data_rule(np.concatenate(costas)), shape["sync"], k["min_score"], k["nbytes"])))
    _LINK.update(shape=shape, rows=rows, baseband=bb, h1=h1, h2=h2, up=up, down=down, K1=K1, K2=K2, records=records)
    return _LINK


def test_packets_come_back_through_five_fourths_and_four_fifths_where_the_delay_predicts(oracle, qpsk_lib):
    """frame_ref's rows -> the oracle's transmit chain at 9600 Hz -> resample_ref 5 / 4 in irregular blocks -> resample_ref 4 / 5 a frame at
    a time -> the oracle's stream receiver at the fixed index the delay gives -> deframe_ref: every packet comes back crc_ok with its
    payload at the column the delay predicts"""
    assert all(hasattr(qpsk_lib, name) for name in RESAMPLE_SYMBOLS)
    k = LINK
    r = link_result(oracle)
    shape = r["shape"]
    assert shape["resampled"] == 15 and shape["index"] == 1 and shape["delay"] == 128 + 35
    assert len(set(r["K1"])) > 4 and len(set(r["K2"])) > 1       # K varies from push to push
    # the round trip is the baseband delayed by 15 samples, to the filters' ripple: measured and printed, not a limit of this test
    d = shape["resampled"]
    diff = np.abs(r["down"][:, d:] - r["baseband"][:, :-d]).max()
    print("round trip against the baseband delayed by %d samples: largest difference %.3g, amplitude %.3g" % (d, diff, np.abs(r["baseband"]).max()))
    for s in range(k["nstreams"]):
        got = r["records"][s]
        assert [g[0] for g in got] == [c + shape["delay"] for c in shape["at"]], s
        for g, payload in zip(got, shape["payloads"][s * k["per_row"]:(s + 1) * k["per_row"]]):
            assert g[4] and g[3][:k["nbytes"]] == payload.tobytes(), s
