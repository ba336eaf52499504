"""The streaming Viterbi decoder with a sliding trace-back window (qpsk_viterbi_stream_*, VITERBI STREAM in include/qpsk_hip.h) and the
encoder that carries its register (qpsk_conv_encode_stream_batch): what can be checked without a GPU.

viterbi_stream_ref and conv_encode_stream_ref below restate the header in numpy, in integers; the GPU tests (test_viterbi_stream_gpu.py)
compare the kernels with them bit for bit.  The restatement keeps every decision word and every soft pair since the reset -- no ring, no
pending pairs, no blocks: it is the definition, not the kernel.  It is pinned here to the row decoder's restatement (viterbi_ref /
viterbi_punct_ref) through the three properties the header states.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_punct_cpu import NAMED, conv_encode_punct_ref, depuncture_ref, popc, puncture_ref, viterbi_punct_ref
from test_rx_ext_cpu import declared
from test_viterbi_cpu import C0, C1, NEG, OPEN_END, conv_encode_from_state, dibits_to_soft, pack_bits, unpack_bits, viterbi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QPSK_ERR_ARG = -2
TERMINATED = 1
MAX_STEPS = 131072
STREAM_SYMBOLS = ("qpsk_viterbi_stream_reset", "qpsk_viterbi_stream_emits", "qpsk_viterbi_stream_push", "qpsk_viterbi_stream_flush",
                  "qpsk_conv_encode_stream_batch", "qpsk_test_viterbi_stream_advance")

_NS = np.arange(64)
_P0, _P1 = _NS >> 1, (_NS >> 1) | 32
_A0, _A1 = 1 - 2 * C0[_NS], 1 - 2 * C1[_NS]                  # bm(ns)
_B0, _B1 = 1 - 2 * C0[_NS | 64], 1 - 2 * C1[_NS | 64]        # bm(ns | 64)
_WEIGHTS = np.uint64(1) << np.arange(64, dtype=np.uint64)


# ------------------------------------------------------------------- the numpy restatement
def viterbi_step(pm, s0, s1):
    """viterbi_ref's step: pm (S, 64) int64, s0 / s1 (S, 1) -> (pm', the decision words (S,) uint64)"""
    m0 = pm[:, _P0] + _A0 * s0 + _A1 * s1
    m1 = pm[:, _P1] + _B0 * s0 + _B1 * s1
    d = m1 > m0                                               # a tie keeps p0
    return np.where(d, m1, m0), (d.astype(np.uint64) * _WEIGHTS).sum(axis=1, dtype=np.uint64)


def push_steps(ntx, pattern):
    """the trellis steps of a push of ntx dibits, or None where the header refuses it"""
    period, keep0, keep1 = pattern
    K = popc(keep0) + popc(keep1)
    if ntx < 1 or (2 * ntx) % K:
        return None
    n = 2 * ntx // K * period
    return n if 1 <= n <= MAX_STEPS else None


class viterbi_stream_ref:
    """S streams pushed together.  push(soft (S, ntx, 2) int8) and flush(flags) return dict(bits (S, nbits / 8) uint8, nbits, info (S, 4))"""

    def __init__(self, nstreams, depth=128, window=256, pattern=(1, 1, 1)):
        assert nstreams >= 1 and depth >= 64 and window >= 64 and depth % 64 == 0 and window % 64 == 0 and depth + window <= 8192
        self.S, self.D, self.W, self.pattern = nstreams, depth, window, tuple(pattern)
        self._start()

    def _start(self):
        self.pm = np.full((self.S, 64), NEG, np.int64)
        self.pm[:, 0] = 0
        self.t = 0                                            # steps since the reset
        self.dec, self.soft = [], []                          # per step: (S,) uint64, (S, 2) int64
        self.out = np.zeros((self.S, 0), np.uint8)            # every bit emitted since the reset

    def emits(self, ntx):
        n = push_steps(ntx, self.pattern)
        assert n is not None
        return self._emitted(self.t + n) - self._emitted(self.t)

    def _emitted(self, total):
        return 0 if total < self.W else max(0, total // self.W * self.W - self.D)

    def _decide(self, st, lo, hi, call):
        """trace back from state st (S,) after step self.t - 1 down to step lo; emit bits [lo, hi) into the call's books"""
        first = st.copy()
        spread = self.pm.max(axis=1) - self.pm.min(axis=1)
        call["info"][:, 2], call["info"][:, 3] = first, spread
        if hi <= lo:
            return
        bits = np.zeros((self.S, self.t - lo), np.uint8)
        for t in range(self.t - 1, lo - 1, -1):
            bits[:, t - lo] = st & 1
            st = (st >> 1) | ((((self.dec[t] >> st.astype(np.uint64)) & np.uint64(1)).astype(np.int64)) << 5)
        new = bits[:, :hi - lo]
        assert self.out.shape[1] == lo                        # the emitted ranges abut
        # re-encode: the register is fed by all earlier emitted bits, zeros before bit 0
        before = np.concatenate([np.zeros((self.S, 6), np.uint8), self.out], axis=1)[:, -6:].astype(np.int64)
        state = sum(before[:, 5 - k] << k for k in range(6))
        coded = conv_encode_from_state(new, state)
        c = np.stack([coded & 1, coded >> 1], axis=-1).astype(np.int64)
        s = np.stack(self.soft[lo:hi], axis=1)
        call["info"][:, 0] += ((s != 0) & ((s < 0).astype(np.int64) != c)).sum(axis=(1, 2))
        call["info"][:, 1] += (s != 0).sum(axis=(1, 2))
        call["new"].append(new)
        self.out = np.concatenate([self.out, new], axis=1)

    def _result(self, call):
        new = np.concatenate(call["new"], axis=1) if call["new"] else np.zeros((self.S, 0), np.uint8)
        return dict(bits=pack_bits(new) if new.shape[1] else np.zeros((self.S, 0), np.uint8), nbits=new.shape[1],
                    info=call["info"].astype(np.int32))

    def push(self, soft):
        soft = np.asarray(soft, np.int8)
        assert soft.ndim == 3 and soft.shape[0] == self.S and soft.shape[2] == 2
        n = push_steps(soft.shape[1], self.pattern)
        assert n is not None, "a push carries whole pattern periods"
        s = depuncture_ref(soft, n, self.pattern).astype(np.int64)      # the -128 rule, and 0 where nothing was sent
        call = dict(new=[], info=np.zeros((self.S, 4), np.int64))
        call["info"][:, 2] = -1
        for u in range(n):
            if self.t % 64 == 0:
                self.pm = self.pm - self.pm.max(axis=1, keepdims=True)
            self.pm, d = viterbi_step(self.pm, s[:, u, 0:1], s[:, u, 1:2])
            assert np.abs(self.pm).max() < 2 ** 31            # int32 on the device
            self.dec.append(d)
            self.soft.append(s[:, u])
            self.t += 1
            if self.t % self.W == 0:
                T = self.t
                self._decide(np.argmax(self.pm, axis=1).astype(np.int64), max(0, T - self.D - self.W), T - self.D, call)
        return self._result(call)

    def flush(self, flags=0):
        call = dict(new=[], info=np.zeros((self.S, 4), np.int64))
        st = np.zeros(self.S, np.int64) if flags & TERMINATED else np.argmax(self.pm, axis=1).astype(np.int64)
        self._decide(st, self._emitted(self.t), self.t, call)
        r = self._result(call)
        self._start()
        return r


def conv_encode_stream_ref(bits_packed, nbits, pattern=(1, 1, 1), state=None):
    """(R, ceil(nbits / 8)) uint8, state (R,) = the register's low six bits before the row (None = 0) -> (transmitted dibits (R, ntx), the
    register's low six bits behind the row)"""
    period, keep0, keep1 = pattern
    b = unpack_bits(np.atleast_2d(bits_packed), nbits)
    assert nbits % period == 0 and (nbits // period * (popc(keep0) + popc(keep1))) % 2 == 0
    r = np.zeros(b.shape[0], np.int64) if state is None else np.asarray(state, np.int64) & 63
    out = puncture_ref(conv_encode_from_state(b, r), pattern)
    for t in range(nbits):
        r = ((r << 1) | b[:, t]) & 127
    return out, (r & 63).astype(np.uint8)


def run_ref(dec, soft, cuts, flags=0):
    """push soft (S, ntx, 2) cut at the dibit positions `cuts`, then flush: (all bits (S, total), summed info[:, :2], the calls)"""
    calls = [dec.push(soft[:, a:b]) for a, b in zip([0] + list(cuts), list(cuts) + [soft.shape[1]]) if b > a]
    calls.append(dec.flush(flags))
    bits = np.concatenate([unpack_bits(c["bits"], c["nbits"]) for c in calls], axis=1)
    return bits, sum(c["info"][:, :2].astype(np.int64) for c in calls), calls


def random_soft(rng, S, ntx):
    """int8 over the whole range, with zeros (erasures) and -128 sprinkled in"""
    s = rng.integers(-128, 128, (S, ntx, 2)).astype(np.int8)
    s[rng.random(s.shape) < 0.05] = 0
    s[rng.random(s.shape) < 0.03] = -128
    return s


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_viterbi_stream_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import inspect
    import torch
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in STREAM_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    for word in ("VITERBI STREAM", "QPSK_VITERBI_STREAM_TERMINATED = 1", "NOTHING DEPENDS ON HOW THE STEPS WERE CUT INTO PUSHES", "Not built: d_flip"):
        assert word in header, word
    for name in ("viterbi_stream_reset", "viterbi_stream", "viterbi_stream_flush", "viterbi_stream_emits", "conv_encode_stream",
                 "viterbi_stream_advance"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    sig = inspect.signature(qpsk_amd.Modem.viterbi_stream_reset).parameters
    assert (sig["depth"].default, sig["window"].default, sig["puncture"].default) == (128, 256, None)
    assert "viterbi_stream.o" in open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    # no context, no work: the entry points refuse a NULL one with QPSK_ERR_ARG on any machine
    buf = (C.c_uint8 * 64)()
    n = C.c_int(-9)
    assert qpsk_lib.qpsk_viterbi_stream_reset(None, 1, 128, 256, 1, 1, 1) == QPSK_ERR_ARG
    assert b"qpsk_viterbi_stream_reset" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_viterbi_stream_emits(None, 64) == QPSK_ERR_ARG
    assert b"qpsk_viterbi_stream_emits" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_viterbi_stream_push(None, buf, 0, 8, buf, 0, None, C.byref(n)) == QPSK_ERR_ARG and n.value == -9
    assert b"qpsk_viterbi_stream_push" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_viterbi_stream_flush(None, 0, buf, 0, None, C.byref(n)) == QPSK_ERR_ARG and n.value == -9
    assert b"qpsk_viterbi_stream_flush" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_conv_encode_stream_batch(None, buf, 1, 8, 1, 1, 1, None, None, buf) == QPSK_ERR_ARG
    assert b"qpsk_conv_encode_stream_batch" in qpsk_lib.qpsk_last_error()
    for delta in (0, 1 << 40, -1):
        assert qpsk_lib.qpsk_test_viterbi_stream_advance(None, delta) == QPSK_ERR_ARG
    assert b"qpsk_test_viterbi_stream_advance" in qpsk_lib.qpsk_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(qpsk_amd.QpskError):
            qpsk_amd.Modem().viterbi_stream_reset(1)


# ------------------------------------------------------------------- 2. the restatement is pinned to the row decoder's
# property 2: floor(N / W) W <= D, so nothing is emitted before the flush, which is then the row decoder on the whole row.  N = 700 at rate
# 1/2; behind 3/4 a push holds whole periods of 3 steps, so the row is the next whole number of periods, 702 steps
@pytest.mark.parametrize("name,N", [("1/2", 700), ("3/4", 702)])
@pytest.mark.parametrize("flags", [0, TERMINATED])
def test_a_flush_before_anything_was_emitted_is_the_row_decoder(name, N, flags):
    pattern = NAMED[name]
    rng = np.random.default_rng(701 + flags)
    ntx = N * (popc(pattern[1]) + popc(pattern[2])) // pattern[0] // 2
    assert push_steps(ntx, pattern) == N
    soft = random_soft(rng, 3, ntx)
    dec = viterbi_stream_ref(3, depth=512, window=512, pattern=pattern)
    cut = 12 * 20
    first = dec.push(soft[:, :cut])
    second = dec.push(soft[:, cut:])
    for c in (first, second):
        assert c["nbits"] == 0 and c["bits"].shape == (3, 0) and not c["info"][:, :2].any()
    assert (first["info"][:, 2] == -1).all() and (second["info"][:, 2] >= 0).all()      # step 512 is a decision point that emits nothing
    got = dec.flush(flags)
    want = viterbi_punct_ref(soft, N, pattern, flags=0 if flags & TERMINATED else OPEN_END)
    assert got["nbits"] == N
    np.testing.assert_array_equal(got["bits"], want["bits"])
    np.testing.assert_array_equal(got["info"][:, 0], want["info"][:, 3])
    np.testing.assert_array_equal(got["info"][:, 2], want["info"][:, 1])
    if name == "1/2":
        np.testing.assert_array_equal(got["bits"], viterbi_ref(soft, flags=0 if flags & TERMINATED else OPEN_END)["bits"])
    assert dec.t == 0 and dec.push(soft[:, :cut])["nbits"] == 0                            # as after a reset


# property 3: noise-free input decodes to the data at the shortest depth and window
@pytest.mark.parametrize("name", sorted(NAMED))
def test_noise_free_streams_decode_to_the_data(name):
    pattern = NAMED[name]
    rng = np.random.default_rng(64)
    nbits = 840 * 2                                           # whole periods of every named pattern, whole dibits
    data = rng.integers(0, 2, (4, nbits)).astype(np.uint8)
    dibits, _ = conv_encode_stream_ref(pack_bits(data), nbits, pattern)
    soft = dibits_to_soft(dibits)
    dec = viterbi_stream_ref(4, depth=64, window=64, pattern=pattern)
    bits, counts, calls = run_ref(dec, soft, [12, 36, 48 * 5, 48 * 11])
    np.testing.assert_array_equal(bits, data)
    assert not counts[:, 0].any() and (counts[:, 1] == 2 * soft.shape[1]).all()
    assert sum(c["nbits"] for c in calls[:-1]) > 0           # decisions fell inside the pushes, not only in the flush


# property 1: partition independence, on values that include erasures and -128
@pytest.mark.parametrize("name,depth,window", [("1/2", 64, 64), ("1/2", 192, 128), ("7/8", 64, 192)])
def test_the_cuts_between_pushes_change_nothing(name, depth, window):
    pattern = NAMED[name]
    rng = np.random.default_rng(depth + window)
    ntx = 12 * 70
    soft = random_soft(rng, 3, ntx)
    whole_bits, whole_counts, whole_calls = run_ref(viterbi_stream_ref(3, depth, window, pattern), soft, [])
    unit = 1 if name == "1/2" else 4                          # 7/8: whole periods are multiples of 4 dibits
    cuts = sorted(set(unit * int(c) for c in rng.integers(1, ntx // unit, 9)))
    bits, counts, calls = run_ref(viterbi_stream_ref(3, depth, window, pattern), soft, cuts)
    np.testing.assert_array_equal(bits, whole_bits)
    np.testing.assert_array_equal(counts, whole_counts)
    assert bits.shape[1] == push_steps(ntx, pattern)
    np.testing.assert_array_equal(calls[-1]["info"], whole_calls[-1]["info"])      # the flush emits the same steps from the same metrics
    for c in calls[:-1]:
        assert c["nbits"] % 64 == 0


def test_emits_counts_what_the_pushes_emit():
    dec = viterbi_stream_ref(1, depth=128, window=192)
    rng = np.random.default_rng(5)
    for ntx in (1, 190, 1, 192, 500, 63, 64):
        want = dec.emits(ntx)
        assert dec.push(random_soft(rng, 1, ntx))["nbits"] == want
    assert dec.flush()["nbits"] == dec_total_minus_emitted(1011, 128, 192)


def dec_total_minus_emitted(total, depth, window):
    return total - max(0, total // window * window - depth)


# the transmit twin
@pytest.mark.parametrize("name", sorted(NAMED))
def test_chunked_stream_encoding_equals_the_row_encoder(name):
    pattern = NAMED[name]
    rng = np.random.default_rng(9)
    nbits = 1680                                              # chunks of 420 bits: whole periods and whole dibits of every named pattern
    data = rng.integers(0, 2, (3, nbits)).astype(np.uint8)
    want = conv_encode_punct_ref(pack_bits(data), nbits, pattern, tail=False)
    state, parts = None, []
    for a, b in ((0, 420), (420, 1260), (1260, 1680)):
        d, state = conv_encode_stream_ref(pack_bits(data[:, a:b]), b - a, pattern, state)
        parts.append(d)
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), want)
    for k in range(6):
        np.testing.assert_array_equal((state >> k) & 1, data[:, nbits - 1 - k])
