"""Soft decisions and per-row signal quality (qpsk_soft_batch): what can be checked without a GPU.

soft_ref() below restates the definition of include/qpsk_hip.h in numpy -- the order of the fp64 sums included -- and the GPU tests
(test_soft_gpu.py) compare the kernels with it bit for bit.  The reference has no counterpart, so the tests here pin the restatement
to a second, naive one, tie the soft values' signs to qpsk_sync_batch's de-rotated dibits on oracle output, and check on the CPU
oracle that the quality figures mean what the header says they mean.
"""
import math
import os

import numpy as np
import pytest

from oracle.pyoracle import TAU, TIMING_FIXED
from sigutil import make_frames
from test_rx_data_cpu import data_rule, make_packet_frame, sync_ref, transmit
from test_rx_ext_cpu import declared, oracle_ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
NPART = 256                      # partial sums of the definition
MODES = {"unit": 0, "llr": 1}    # QPSK_SOFT_UNIT, QPSK_SOFT_LLR


# ------------------------------------------------------------------- the numpy restatement
def row_sums(z, skip):
    """(nsym, 2) float32 -> (S1, S2, S4, SQ) float64 in the defined order, and m = nsym - skip"""
    z = np.asarray(z, np.float32)[skip:].astype(np.float64)
    a, b = z[:, 0], z[:, 1]
    aa, bb = a * a, b * b
    p = aa + bb
    sr = aa - bb
    si = 2.0 * (a * b)
    terms = np.stack([np.abs(a) + np.abs(b), p, p * p, sr * sr - si * si], axis=1)
    m = len(terms)
    P = np.zeros((NPART, 4), np.float64)
    for j in range(0, m, NPART):                  # P[l] takes its terms k = l, l + 256, ... in increasing k
        c = terms[j:j + NPART]
        P[:len(c)] += c
    h = NPART // 2
    while h:
        P[:h] += P[h:2 * h]
        h //= 2
    return P[0].copy(), m


def row_finish(S, m, mode, scale):
    """the sums of one row -> (quality (4,) float32, gain float32)"""
    S1, S2, S4, SQ = (float(v) for v in S)
    M2, M4 = S2 / m, S4 / m
    D = 2.0 * M2 * M2 - M4
    Ps = math.sqrt(D) if D > 0.0 else 0.0
    Pn = M2 - Ps
    amp = S1 / (2.0 * m)
    with np.errstate(over="ignore"):
        q = np.array([amp, Ps / Pn if Pn > 0.0 else 0.0, -SQ / S4 if S4 > 0.0 else 0.0, max(Pn, 0.0) / 2.0]).astype(np.float32)
    sc = float(np.float32(scale))

    def unit(target):
        return np.float32(min(target / amp, FLT_MAX)) if amp > 0.0 else np.float32(0.0)

    if MODES[mode] == 1:
        g = np.float32(min(2.0 * math.sqrt(Ps / 2.0) / (Pn / 2.0) / sc, FLT_MAX)) if Pn > 0.0 else unit(127.0)
    else:
        g = unit(sc)
    return q, g


def quantise(x, g):
    """float32 array, float32 gain -> int8: fp32 multiply, round half to even, limited to +-127"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.clip(np.rint(np.asarray(x, np.float32) * np.float32(g)), -127, 127).astype(np.int8)


def soft_ref(costas, skip=0, mode="unit", scale=64.0, gain=None, lag=None, rot=None, first=0, nout=None):
    """costas (R, nsym, 2) float32 -> dict(soft (R, nout, 2) int8, quality (R, 4) float32, sums (R, 4) float64, gain (R,) float32);
    gain / lag / rot: per-row arrays or None.  A row whose lag leaves the row has zeros in soft."""
    z = np.asarray(costas, np.float32)
    if z.ndim == 2:
        z = z[None]
    R, nsym = z.shape[0], z.shape[1]
    nout = nsym - first if nout is None else nout
    out = dict(soft=np.zeros((R, nout, 2), np.int8), quality=np.zeros((R, 4), np.float32), sums=np.zeros((R, 4), np.float64),
               gain=np.zeros(R, np.float32))
    for r in range(R):
        S, m = row_sums(z[r], skip)
        out["sums"][r] = S
        out["quality"][r], g = row_finish(S, m, mode, scale)
        if gain is not None:
            g = np.float32(gain[r])
        out["gain"][r] = g
        L = 0 if lag is None else int(lag[r])
        if L < 0 or L + first + nout > nsym:
            continue
        x = z[r, L + first:L + first + nout]
        a, b = x[:, 0], x[:, 1]
        u, v = ((a, b), (b, -a), (-a, -b), (-b, a))[(0 if rot is None else int(rot[r])) & 3]
        out["soft"][r, :, 0] = quantise(u, g)
        out["soft"][r, :, 1] = quantise(v, g)
    return out


def naive_sums(z, skip):
    """the same sums symbol by symbol in Python floats: one loop over the symbols, then the tree"""
    P = [[0.0] * 4 for _ in range(NPART)]
    for k, (a, b) in enumerate(np.asarray(z, np.float32)[skip:].tolist()):
        p = a * a + b * b
        sr, si = a * a - b * b, 2.0 * (a * b)
        t = (abs(a) + abs(b), p, p * p, sr * sr - si * si)
        for q in range(4):
            P[k % NPART][q] += t[q]
    h = NPART // 2
    while h:
        for l in range(h):
            for q in range(4):
                P[l][q] += P[l + h][q]
        h //= 2
    return np.array(P[0], np.float64)


# ------------------------------------------------------------------- ABI (fails without the feature)
def test_soft_entry_point_is_declared_bound_and_exported(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    assert "qpsk_soft_batch" in declared("qpsk_hip.h")
    assert "qpsk_soft_batch" in API_SYMBOLS
    assert hasattr(qpsk_lib, "qpsk_soft_batch")
    for name in ("soft", "quality"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "QPSK_SOFT_UNIT" in header and "QPSK_SOFT_LLR" in header


def test_soft_kernel_is_built_and_writes_no_scalar_memory():
    src = open(os.path.join(ROOT, "qpsk_amd", "csrc", "soft.hip")).read().lower()
    assert "soft.o" in open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_d" + "cache_",
                 "atomic" + "add"):
        assert word not in src, word


# ------------------------------------------------------------------- the restatement is pinned
@pytest.mark.parametrize("nsym,skip", [(1, 0), (64, 0), (255, 3), (256, 0), (257, 0), (257, 256), (513, 1), (1000, 255), (2049, 256),
                                       (2049, 2048)])
def test_soft_ref_sums_equal_the_naive_loop(nsym, skip):
    rng = np.random.default_rng(nsym * 7 + skip)
    z = (rng.standard_normal((nsym, 2)) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
    S, m = row_sums(z, skip)
    assert m == nsym - skip
    assert np.array_equal(S.view(np.uint64), naive_sums(z, skip).view(np.uint64))


def test_soft_ref_hand_cases():
    # the constellation on the diagonals at amplitude A: amp = A, lock = +1, no noise; UNIT puts it at +-scale
    A = np.float32(0.75)
    z = np.array([[A, A], [-A, A], [-A, -A], [A, -A]] * 16, np.float32)
    r = soft_ref(z, scale=64.0)
    assert r["quality"][0, 0] == A and r["quality"][0, 2] == 1.0 and r["quality"][0, 1] == 0.0 and r["quality"][0, 3] == 0.0
    assert set(np.abs(r["soft"]).reshape(-1).tolist()) == {64}
    assert np.array_equal(r["soft"][0, :4, 0] < 0, [False, True, True, False]) and np.array_equal(r["soft"][0, :4, 1] < 0, [False, False, True, True])
    # LLR with no measurable noise falls back to the UNIT rule with 127
    assert set(np.abs(soft_ref(z, mode="llr", scale=0.5)["soft"]).reshape(-1).tolist()) == {127}
    # on the axes (45 degrees off) the lock figure is -1
    z2 = np.array([[A, 0], [0, A], [-A, 0], [0, -A]] * 16, np.float32)
    assert soft_ref(z2)["quality"][0, 2] == -1.0
    # all zeros: gain 0, quality 0, soft 0
    r = soft_ref(np.zeros((2, 70, 2), np.float32), skip=5, mode="llr")
    assert not r["quality"].any() and not r["gain"].any() and not r["soft"].any()
    # rotations: exact swaps and sign flips; ties round to even; saturation at +-127
    z3 = np.array([[0.5, -1.5], [2.5, 300.0], [-0.5, 1.5], [-2.5, -300.0]], np.float32)
    s = [soft_ref(z3, gain=[1.0], rot=[k])["soft"][0].tolist() for k in range(4)]
    assert s[0] == [[0, -2], [2, 127], [0, 2], [-2, -127]]
    assert s[1] == [[-2, 0], [127, -2], [2, 0], [-127, 2]]
    assert s[2] == [[0, 2], [-2, -127], [0, -2], [2, 127]]
    assert s[3] == [[2, 0], [-127, 2], [-2, 0], [127, -2]]
    # a lag that leaves the row: zeros for that row only
    r = soft_ref(np.ones((3, 10, 2), np.float32), gain=[1, 1, 1], lag=[0, 7, -1], first=2, nout=2)
    assert r["soft"][0].tolist() == [[1, 1], [1, 1]] and not r["soft"][1].any() and not r["soft"][2].any()
    # the gain never becomes infinite
    tiny = np.full((1, 8, 2), np.float32(1e-45), np.float32)
    assert soft_ref(tiny, scale=1e30)["gain"][0] == np.float32(FLT_MAX)


# ------------------------------------------------------------------- signs against the sync search, on oracle output
def test_soft_signs_equal_the_derotated_dibits_at_every_rotation(oracle):
    """packets transmitted at four carrier quarter turns (as test_rx_data_cpu's link), received on the oracle; data rule -> sync_ref gives
    lag, rot and the de-rotated dibits; wherever a soft value is non-zero its sign bit is the dibit's bit, and next to none are zero"""
    fs, rs, C, L = 19200.0, 2400.0, 8, 16384
    nsym, nbytes, prefix = L // C, 64, 100
    taps = oracle.rrc_make(np.float32(fs), np.float32(rs), np.float32(0.35))
    rng = np.random.default_rng(41)
    sync = rng.integers(0, 4, 64, dtype=np.uint8)
    nout = nsym - 64 - prefix - 126 // C                       # the whole row behind the word
    zero = total = 0
    rots = set()
    for noise in (0.02, 0.05):
        x = np.stack([transmit(make_packet_frame(oracle, rng, nsym, prefix, sync, nbytes)[0], L, C, taps, fs, offset_hz=30.0,
                               phase=0.3 + f * np.pi / 2, noise=noise, seed=f) for f in range(4)])
        got = oracle_ext(oracle, x, fs, rs, np.full(4, 126 % C, np.int32), None, loop_bw=np.float32(TAU / 100.0), want_costas=True)
        s = sync_ref(data_rule(got["costas"]), sync, 0, 255, nout)
        assert np.all(s["lag"] == prefix + 126 // C) and np.all(s["score"] == len(sync))
        rots |= set(s["rot"].tolist())
        for mode, scale in (("unit", 64.0), ("llr", 0.25)):
            q = soft_ref(got["costas"], skip=256, mode=mode, scale=scale, lag=s["lag"], rot=s["rot"], first=len(sync), nout=nout)["soft"]
            for bit in (0, 1):
                nz = q[:, :, bit] != 0
                assert np.array_equal((q[:, :, bit] < 0)[nz], ((s["out"] >> bit) & 1).astype(bool)[nz]), (noise, mode, bit)
                zero += int((~nz).sum())
                total += nz.size
    assert rots == {0, 1, 2, 3}, rots
    print("soft values equal to zero: %d of %d" % (zero, total))
    assert zero < 0.01 * total


# ------------------------------------------------------------------- the quality figures mean what they say
FS, RS, L2, C8, IDX, SKIP, NF = 19200.0, 2400.0, 16384, 8, 6, 256, 48      # fixed_index 6: the matched instant for make_frames stimulus


@pytest.fixture(scope="module")
def batches(oracle):
    """quality and UNIT soft values of 48 oracle frames per stimulus"""
    taps = oracle.rrc_make(np.float32(FS), np.float32(RS), np.float32(0.35))

    def run(x):
        z = oracle.rx_batch(x, FS, RS, timing_mode=TIMING_FIXED, fixed_index=IDX, want_costas=True)["costas"]
        return soft_ref(z, skip=SKIP, scale=64.0, first=SKIP)

    out = {}
    for noise in (0.0, 0.02, 0.05, 0.1, 0.2, 0.4):
        out[noise] = run(make_frames(NF, L2, C8, taps, FS, offset_hz=20.0, noise=noise)[0])
    out["noise only"] = run((0.3 * np.random.default_rng(1).standard_normal((NF, L2, 2))).astype(np.float32))
    out["1000 Hz"] = run(make_frames(NF, L2, C8, taps, FS, offset_hz=1000.0, noise=0.05)[0])
    return out


def test_lock_reads_high_on_locked_frames_and_low_otherwise(batches):
    for noise in (0.0, 0.05, 0.1):
        lock = batches[noise]["quality"][:, 2]
        print("noise %g: lock min %.5f" % (noise, lock.min()))
        assert np.all(lock > 0.8), (noise, lock.min())
    for key in ("noise only", "1000 Hz"):
        lock = batches[key]["quality"][:, 2]
        print("%s: |lock| max %.4f" % (key, np.abs(lock).max()))
        assert np.all(np.abs(lock) < 0.4), (key, np.abs(lock).max())


def test_snr_falls_with_noise_and_reads_below_one_on_noise(batches):
    means = [float(batches[n]["quality"][:, 1].astype(np.float64).mean()) for n in (0.02, 0.05, 0.1, 0.2, 0.4)]
    print("mean snr at noise 0.02 .. 0.4:", means)
    assert all(a > b for a, b in zip(means, means[1:])), means
    snr = batches["noise only"]["quality"][:, 1]
    print("noise only: snr max %.3f" % snr.max())
    assert np.all(snr < 1.0), snr.max()


def test_unit_mode_lands_on_scale(batches):
    for noise in (0.0, 0.02, 0.05, 0.1):
        mean = np.abs(batches[noise]["soft"].astype(np.float64)).mean(axis=(1, 2))
        print("noise %g: mean |q| %.3f .. %.3f" % (noise, mean.min(), mean.max()))
        assert np.all(np.abs(mean - 64.0) < 1.0), (noise, mean.min(), mean.max())
