"""Convolutionally coded packets out of continuous streams (qpsk_deframer_reset_coded / qpsk_deframer_push_coded): what can be checked
without a GPU.

deframe_coded_ref() below restates the contract of include/qpsk_hip.h (CODED DEFRAMER) in numpy.  It is composed of restatements that
are pinned elsewhere and imported, not copied: data_rule (test_rx_data_cpu), the hunt of deframe_ref (test_deframe_cpu: asked for the
first word at or behind h, once per packet), quantise / row_sums / row_finish (test_soft_cpu), viterbi_ref (test_viterbi_cpu), crc16
and keystream (test_deframe_cpu).  The GPU tests (test_deframe_coded_gpu.py) compare the kernels with it bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_deframe_cpu import crc16, deframe_ref, keystream, turn
from test_rx_data_cpu import bytes_to_dibits, data_rule
from test_rx_ext_cpu import declared
from test_soft_cpu import quantise, row_finish, row_sums, soft_ref
from test_viterbi_cpu import conv_encode_ref, viterbi_ref

CODED_SYMBOLS = ("qpsk_deframer_reset_coded", "qpsk_deframer_push_coded")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PROBE_KS = np.zeros(12, np.uint8)


def coded_steps(nbytes):
    """Nc: the dibits of a coded body"""
    return 8 * (nbytes + 2) + 6


def first_word(D, h, sync, min_score):
    """the hunt of deframe_ref: (p*, r*, score) of the first word at or behind h whose sync word is complete in D, or None.  A probe
    deframer of one-byte packets is asked for its FIRST packet only, so its own payload length never matters (a coded body is longer)"""
    got = deframe_ref(np.asarray(D)[h:], sync, min_score, 1, ks=_PROBE_KS)
    return (h + got[0]["pos"], got[0]["rot"], got[0]["score"]) if got else None


def push_gain(row, mode, scale):
    """the gain qpsk_soft_batch defines for one pushed row with skip = 0"""
    S, m = row_sums(row, 0)
    return row_finish(S, m, mode, scale)[1]


def deframe_coded_ref(pushes, gains, sync, min_score, nbytes, mode="unit", scale=64.0):
    """one stream.  pushes: list of (nsym_k, 2) float32 rows of costas_frame[]; gains: None (every push takes its row's own gain) or one
    float32 per push.  -> list over pushes of the packets that push reports, each dict(pos, rot, score, bytes (nbytes + 2) uint8, crc_ok,
    info (4,) int32, end, soft (Nc, 2) int8)"""
    pushes = [np.asarray(p, np.float32).reshape(-1, 2) for p in pushes]
    z = np.concatenate(pushes)
    D = data_rule(z)
    ends = np.cumsum([len(p) for p in pushes])
    g_push = np.array([push_gain(p, mode, scale) if gains is None else np.float32(gains[k]) for k, p in enumerate(pushes)], np.float32)
    g_sym = np.repeat(g_push, [len(p) for p in pushes])
    n, Nc = len(sync), coded_steps(nbytes)
    ks = keystream(Nc)
    out = [[] for _ in pushes]
    h = 0
    while True:
        w = first_word(D, h, sync, min_score)
        if w is None or w[0] + n + Nc > len(D):
            break
        p, r, score = w
        x, g = z[p + n:p + n + Nc], g_sym[p + n:p + n + Nc]
        a, b = x[:, 0], x[:, 1]
        u, v = ((a, b), (b, -a), (-a, -b), (-b, a))[r]
        soft = np.stack([quantise(u, g), quantise(v, g)], axis=1)
        dec = viterbi_ref(soft[None], flip=ks)
        byts = dec["bits"][0][:nbytes + 2]
        ok = crc16(byts[:nbytes]) == (int(byts[nbytes]) << 8 | int(byts[nbytes + 1]))
        h = p + n + Nc
        out[int(np.searchsorted(ends, h))].append(dict(pos=p, rot=r, score=score, bytes=byts, crc_ok=bool(ok), info=dec["info"][0], end=h,
                                                       soft=soft))
    return out


def make_coded_packet(rng, sync, nbytes, corrupt=False, payload=None):
    """[sync][keystream xor conv_encode(payload + CRC-16 big-endian, tail)] as dibits -> (dibits, payload)"""
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8) if payload is None else payload
    crc = crc16(payload) ^ (1 if corrupt else 0)
    packet = np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])
    body = conv_encode_ref(packet[None, :], 8 * len(packet), tail=True)[0] ^ keystream(coded_steps(nbytes))
    return np.concatenate([np.asarray(sync, np.uint8), body]).astype(np.uint8), payload


def dibits_to_costas(d, amp=1.0, q=0, noise=0.0, rng=None):
    """dibits on the diagonals at amplitude amp per component, turned q quarter turns, plus Gaussian noise -> (n, 2) float32"""
    d = np.asarray(d, np.uint8)
    zc = (amp * (1.0 - 2.0 * (d & 1)) + 1j * amp * (1.0 - 2.0 * (d >> 1))) * (1j ** q)
    z = np.stack([zc.real, zc.imag], axis=1)
    if noise:
        z = z + noise * rng.standard_normal(z.shape)
    return z.astype(np.float32)


def cut(z, sizes):
    """rows of the given sizes, then the rest"""
    out, at = [], 0
    for s in sizes:
        if at >= len(z):
            break
        out.append(z[at:at + s])
        at += s
    if at < len(z):
        out.append(z[at:])
    return out


def flat(reported):
    return [p for push in reported for p in push]


def same_packets(a, b):
    key = lambda p: (p["pos"], p["rot"], p["score"], p["bytes"].tobytes(), p["crc_ok"], p["info"].tobytes())      # noqa: E731
    return [key(p) for p in a] == [key(p) for p in b]


# ------------------------------------------------------------------- ABI (fails without the feature)
def test_coded_deframer_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in CODED_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    for name in ("deframer_reset_coded", "deframe_coded"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    buf = (C.c_uint8 * 64)()
    assert qpsk_lib.qpsk_deframer_reset_coded(None, 1, buf, 16, 16, 4, 1, 0, 64.0) == -2
    assert b"qpsk_deframer_reset_coded" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_deframer_push_coded(None, buf, 8, None, buf, None, None, None, None, None, None) == -2
    assert b"qpsk_deframer_push_coded" in qpsk_lib.qpsk_last_error()


def test_coded_deframer_sources_are_built_and_write_no_scalar_memory():
    mk = open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    assert "deframe_coded.o" in mk
    for name in ("deframe_coded.hip", "viterbi_row.h", "deframe_bits.h", "soft_quant.h"):
        src = open(os.path.join(ROOT, "qpsk_amd", "csrc", name)).read().lower()
        assert name in mk, name
        for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_d" + "cache_"):
            assert word not in src, (name, word)


# ------------------------------------------------------------------- the restatement, on hand cases
def test_threshold_exactly_at_min_score():
    rng = np.random.default_rng(11)
    nbytes, sync = 4, rng.integers(0, 4, 16, dtype=np.uint8)
    pkt, payload = make_coded_packet(rng, sync, nbytes)
    for errors in (2, 3):
        bad = pkt.copy()
        for i in (1, 5, 9)[:errors]:
            bad[i] = turn(bad[i:i + 1], 1)[0]                           # a wrong dibit in the word
        z = dibits_to_costas(np.concatenate([np.zeros(40, np.uint8), bad, np.zeros(10, np.uint8)]), amp=0.7)
        at = flat(deframe_coded_ref([z], [90.0], sync, 16 - errors, nbytes))
        assert [(p["pos"], p["score"], p["crc_ok"]) for p in at if p["pos"] == 40] == [(40, 16 - errors, True)], errors
        assert np.array_equal([p for p in at if p["pos"] == 40][0]["bytes"][:nbytes], payload)
        below = flat(deframe_coded_ref([z], [90.0], sync, 16 - errors + 1, nbytes))
        assert 40 not in [p["pos"] for p in below]


def test_hunt_resumes_behind_a_failed_packet_and_packets_run_back_to_back():
    rng = np.random.default_rng(12)
    nbytes, sync = 8, rng.integers(0, 4, 24, dtype=np.uint8)
    n, Nc = 24, coded_steps(nbytes)
    a, _ = make_coded_packet(rng, sync, nbytes, corrupt=True)
    b, pb = make_coded_packet(rng, sync, nbytes)
    c, pc = make_coded_packet(rng, sync, nbytes)
    a_bad = a.copy()
    a_bad[n + 10:n + 10 + n] = sync                                     # a second word INSIDE a's body: the hunt does not see it
    d = np.concatenate([rng.integers(0, 4, 7, dtype=np.uint8), a_bad, turn(b, 3), c, rng.integers(0, 4, 5, dtype=np.uint8)])
    got = flat(deframe_coded_ref([dibits_to_costas(d)], [64.0], sync, n, nbytes))
    assert [(p["pos"], p["crc_ok"], p["rot"]) for p in got] == [(7, False, 0), (7 + n + Nc, True, 3), (7 + 2 * (n + Nc), True, 0)]
    assert got[0]["end"] == got[1]["pos"] and got[1]["end"] == got[2]["pos"]
    assert np.array_equal(got[1]["bytes"][:nbytes], pb) and np.array_equal(got[2]["bytes"][:nbytes], pc)
    assert np.all(got[1]["info"] == [2 * 64 * Nc, 0, 0, 0])             # noise free at +-64: every soft value agrees with the path


def noisy_stream(rng, sync, nbytes, npackets, amp, noise):
    parts, sent = [], []
    for q in range(npackets):
        parts.append(rng.integers(0, 4, int(rng.integers(0, 50)), dtype=np.uint8))
        pkt, pl = make_coded_packet(rng, sync, nbytes)
        sent.append((sum(len(p) for p in parts), pl))
        parts.append(turn(pkt, q & 3))
    parts.append(rng.integers(0, 4, 9, dtype=np.uint8))
    return dibits_to_costas(np.concatenate(parts), amp=amp, noise=noise, rng=rng), sent


def test_a_constant_gain_gives_a_result_independent_of_the_cuts():
    """cuts of one symbol per push, of sizes that put one packet over three and more pushes, and no cut at all: the packets are the
    same, each reported by the push that brings its last symbol"""
    rng = np.random.default_rng(13)
    nbytes, sync = 5, rng.integers(0, 4, 20, dtype=np.uint8)
    Nc = coded_steps(nbytes)
    z, sent = noisy_stream(rng, sync, nbytes, 4, amp=0.8, noise=0.35)
    g = np.float32(80.0)
    whole = deframe_coded_ref([z], [g], sync, 18, nbytes)
    assert [p["pos"] for p in whole[0]] == [t for t, _ in sent] and all(p["crc_ok"] for p in whole[0])
    assert any(p["info"][3] > 0 for p in whole[0])                      # the noise did flip channel bits
    thirds = [Nc // 3] * (len(z) // (Nc // 3) + 1)                      # rows shorter than a third of a body: every body over >= 3 pushes
    assert max(len(r) for r in cut(z, thirds)) * 3 <= Nc
    for sizes in ([1] * len(z), [17] * 40, thirds, [7, 1, 1, 300, 2, 64]):
        rows = cut(z, sizes)
        got = deframe_coded_ref(rows, [g] * len(rows), sync, 18, nbytes)
        assert same_packets(flat(got), whole[0]), sizes
        ends = np.cumsum([len(r) for r in rows])
        for k, push in enumerate(got):
            for p in push:
                assert (ends[k - 1] if k else 0) < p["end"] <= ends[k]


def test_a_per_push_gain_applies_to_exactly_that_push_s_symbols():
    rng = np.random.default_rng(14)
    nbytes, sync = 3, rng.integers(0, 4, 16, dtype=np.uint8)
    n, Nc = 16, coded_steps(nbytes)
    pkt, _ = make_coded_packet(rng, sync, nbytes)
    z = dibits_to_costas(np.concatenate([np.zeros(5, np.uint8), pkt, np.zeros(4, np.uint8)]), amp=0.5, noise=0.05, rng=rng)
    rows = cut(z, [5 + n + 10, 20, 7])                                  # body symbols 0..9 | 10..29 | 30..36 | the rest
    gains = np.array([40.0, 100.0, 10.0, 64.0], np.float32)
    got = flat(deframe_coded_ref(rows, gains, sync, n, nbytes))
    assert len(got) == 1 and got[0]["pos"] == 5
    body = z[5 + n:5 + n + Nc]
    for lo, hi, g in ((0, 10, 40.0), (10, 30, 100.0), (30, 37, 10.0), (37, Nc, 64.0)):
        assert np.array_equal(got[0]["soft"][lo:hi, 0], quantise(body[lo:hi, 0], np.float32(g))), (lo, hi)
        assert np.array_equal(got[0]["soft"][lo:hi, 1], quantise(body[lo:hi, 1], np.float32(g))), (lo, hi)
    assert not np.array_equal(got[0]["soft"], flat(deframe_coded_ref(rows, [64.0] * 4, sync, n, nbytes))[0]["soft"])


@pytest.mark.parametrize("mode", ["unit", "llr"])
def test_without_a_gain_every_push_takes_the_gain_soft_ref_defines_for_its_row(mode):
    rng = np.random.default_rng(15)
    nbytes, sync = 6, rng.integers(0, 4, 24, dtype=np.uint8)
    n, Nc = 24, coded_steps(nbytes)
    pkt, payload = make_coded_packet(rng, sync, nbytes)
    z = dibits_to_costas(np.concatenate([rng.integers(0, 4, 300, dtype=np.uint8), turn(pkt, 1), rng.integers(0, 4, 400, dtype=np.uint8)]),
                         amp=0.6, noise=0.12, rng=rng)
    z[500:] *= np.float32(1.7)                                          # the level changes between the pushes
    rows = cut(z, [340, 160])                                           # the body starts at 324: 16 symbols in push 0, 160 in push 1, the rest in push 2
    got = flat(deframe_coded_ref(rows, None, sync, 22, nbytes, mode=mode, scale=32.0))
    assert len(got) == 1 and (got[0]["pos"], got[0]["rot"]) == (300, 1) and got[0]["crc_ok"]
    assert np.array_equal(got[0]["bytes"][:nbytes], payload)
    at = 0
    for k, row in enumerate(rows):
        want = soft_ref(row[None], skip=0, mode=mode, scale=32.0)["gain"][0]
        assert push_gain(row, mode, 32.0) == want
        lo, hi = max(at, 324) - 324, min(at + len(row), 324 + Nc) - 324
        if hi > lo:
            x = z[324 + lo:324 + hi]
            assert np.array_equal(got[0]["soft"][lo:hi, 0], quantise(x[:, 1], want)), k      # r = 1: (u, v) = (b, -a)
            assert np.array_equal(got[0]["soft"][lo:hi, 1], quantise(-x[:, 0], want)), k
        at += len(row)
    assert len({float(push_gain(r, mode, 32.0)) for r in rows}) == 3


@pytest.mark.parametrize("gain", [None, 71.5])
def test_a_packet_inside_one_push_equals_soft_ref_then_viterbi_ref(gain):
    rng = np.random.default_rng(16)
    nbytes, sync = 16, rng.integers(0, 4, 32, dtype=np.uint8)
    n, Nc = 32, coded_steps(nbytes)
    pkt, payload = make_coded_packet(rng, sync, nbytes)
    lag = 77
    z = dibits_to_costas(np.concatenate([rng.integers(0, 4, lag, dtype=np.uint8), turn(pkt, 2), rng.integers(0, 4, 30, dtype=np.uint8)]),
                         amp=0.9, noise=0.4, rng=rng)
    got = flat(deframe_coded_ref([z], None if gain is None else [gain], sync, 28, nbytes))
    assert len(got) == 1 and (got[0]["pos"], got[0]["rot"]) == (lag, 2)
    s = soft_ref(z[None], skip=0, gain=None if gain is None else np.array([gain], np.float32), lag=[lag], rot=[2], first=n, nout=Nc)
    v = viterbi_ref(s["soft"], flip=keystream(Nc))
    assert np.array_equal(got[0]["soft"], s["soft"][0])
    assert np.array_equal(got[0]["bytes"], v["bits"][0][:nbytes + 2]) and np.array_equal(got[0]["info"], v["info"][0])
    assert got[0]["crc_ok"] and np.array_equal(got[0]["bytes"][:nbytes], payload) and got[0]["info"][3] > 0


# ------------------------------------------------------------------- the kernels' own formulations, restated
def test_per_byte_crc_shares_sum_to_crc16():
    """deframe_coded_decode_kernel's CRC: byte k of nbytes contributes crc_byte(b) x^(8 (nbytes - 1 - k)) modulo the polynomial, the
    register's start value contributes 0xFFFF x^(8 nbytes) (the table and crc_init of qpsk_deframer_reset_coded); the xor is crc16()"""
    def step(r):
        return ((r << 1) ^ (0x1021 if r & 0x8000 else 0)) & 0xFFFF

    def mulmod(a, m):
        r = 0
        for i in range(15, -1, -1):
            r = step(r)
            if (m >> i) & 1:
                r ^= a
        return r

    def crc_byte(b):
        x = b ^ (b >> 4)
        return ((x << 12) ^ (x << 5) ^ x) & 0xFFFF

    rng = np.random.default_rng(17)
    for n in (1, 2, 5, 64, 1023, 1024):
        adv, a, init = [], 1, 0xFFFF
        for _ in range(n):
            adv.append(a)
            for _ in range(8):
                a, init = step(a), step(init)
        d = rng.integers(0, 256, n).tolist()
        share = 0
        for k, b in enumerate(d):
            share ^= mulmod(crc_byte(b), adv[n - 1 - k])
        assert share ^ init == crc16(d), n


class HuntEmulation:
    """Pins the DESIGN, not the kernel: a hand-written mirror of deframe_coded_hunt_kernel's bookkeeping, which shows that the scheme
    (what is carried, where a body's pairs go, how many staging rows a push needs) yields the contract; only the GPU tests compare the
    kernel itself.  For one stream, push by push, in the kernel's own terms: the carried tail of n - 1 ring
    values, X = [tail][row], positions p_x in [0, P), the pending buffer of int8 pairs, staging rows by slot with per_stream =
    min(max_packets, nsym // (n + Nc) + 1), packets beyond max_packets counted only; then the decode of every staged row.  Scores are
    taken directly (the bit planes are deframe_kernel's, pinned by test_deframe_gpu.py)."""

    def __init__(self, sync, min_score, nbytes, max_packets):
        from test_deframe_cpu import RING
        self.RING = RING
        self.rs = RING[np.asarray(sync)].astype(np.int64)
        self.n, self.N, self.ms, self.nb, self.M = len(sync), coded_steps(nbytes), min_score, nbytes, max_packets
        self.len = self.h = self.pending = self.have = 0
        self.tail = np.zeros(0, np.int64)
        self.pend = np.zeros((self.N, 2), np.int8)

    @staticmethod
    def pairs(x, r, g):
        a, b = x[:, 0], x[:, 1]
        u, v = ((a, b), (b, -a), (-a, -b), (-b, a))[r]
        return np.stack([quantise(u, g), quantise(v, g)], axis=1)

    def push(self, row, g):
        n, N, nsym = self.n, self.N, len(row)
        ring = self.RING[data_rule(row)].astype(np.int64)
        per = min(self.M, nsym // (n + N) + 1)
        stage, found, count = {}, [], 0
        T = min(self.len, n - 1)
        if self.pending:
            need = N - self.have
            if nsym >= need:
                assert count < per
                stage[count] = np.concatenate([self.pend[:self.have], self.pairs(row[:need], self.prot, g)])
                found.append((self.ppos, self.prot, self.pscore))
                count += 1
                self.pending = 0
            else:
                self.pend[self.have:self.have + nsym] = self.pairs(row, self.prot, g)
                self.have += nsym
        base0, Xv = self.len - T, np.concatenate([self.tail, ring])
        X = T + nsym
        P = X - n + 1
        if not self.pending and P > 0 and self.h < base0 + P:
            hx, moved = max(self.h - base0, 0), False
            diff = (np.lib.stride_tricks.sliding_window_view(Xv, n) - self.rs) & 3
            sc = np.stack([(diff == r).sum(axis=1) for r in range(4)], axis=1)
            best, rot = sc.max(axis=1), sc.argmax(axis=1)
            while True:
                cand = np.nonzero(best[hx:P] >= self.ms)[0]
                if not len(cand):
                    break
                px = hx + int(cand[0])
                hx, moved, row0 = px + n + N, True, px + n - T
                assert row0 >= 0                                         # the body starts in the row
                if hx > X:
                    got = nsym - row0
                    assert 0 <= got < N
                    self.pend[:got] = self.pairs(row[row0:], int(rot[px]), g)
                    self.pending, self.have = 1, got
                    self.ppos, self.prot, self.pscore = base0 + px, int(rot[px]), int(best[px])
                    break
                if count < per:
                    assert row0 + N <= nsym
                    stage[count] = self.pairs(row[row0:row0 + N], int(rot[px]), g)
                    found.append((base0 + px, int(rot[px]), int(best[px])))
                else:
                    assert count >= self.M                               # per_stream only ever cuts at max_packets
                count += 1
            if moved:
                self.h = base0 + hx
        self.tail = Xv[X - min(X, n - 1):].copy()
        self.len += nsym
        out = []
        for slot in range(min(count, per)):
            d = viterbi_ref(stage[slot][None], flip=keystream(N))
            b = d["bits"][0][:self.nb + 2]
            ok = crc16(b[:self.nb]) == (int(b[self.nb]) << 8 | int(b[self.nb + 1]))
            out.append(dict(pos=found[slot][0], rot=found[slot][1], score=found[slot][2], bytes=b, crc_ok=bool(ok), info=d["info"][0]))
        return count, out


def test_the_hunt_kernel_s_bookkeeping_equals_the_restatement_on_random_cuts():
    rng = np.random.default_rng(18)
    for trial in range(8):
        nsync, nbytes = [(32, 16), (64, 5), (100, 5), (20, 40)][trial % 4]
        sync = rng.integers(0, 4, nsync, dtype=np.uint8)
        parts = []
        while sum(len(p) for p in parts) < 2500:
            pkt, _ = make_coded_packet(rng, sync, nbytes, corrupt=bool(rng.integers(0, 6) == 0))
            parts += [rng.integers(0, 4, int(rng.integers(0, 120)), dtype=np.uint8), turn(pkt, int(rng.integers(0, 4)))]
        z = dibits_to_costas(np.concatenate(parts), amp=0.7, noise=0.2, rng=rng)
        sizes = []
        while sum(sizes) < len(z):
            sizes.append(int(rng.choice([1, 3, 50, 400, 1500, int(rng.integers(1, 300))])))
        rows = cut(z, sizes[:-1])
        gains = rng.uniform(20.0, 90.0, len(rows)).astype(np.float32)
        M = (64, 2)[trial % 2]
        ref = deframe_coded_ref(rows, gains, sync, nsync - 3, nbytes)
        emu = HuntEmulation(sync, nsync - 3, nbytes, M)
        total = 0
        for k, row in enumerate(rows):
            count, got = emu.push(row, gains[k])
            assert count == len(ref[k]), (trial, k)
            assert same_packets(got, ref[k][:M]), (trial, k)
            total += count
        assert total >= 5, trial


# ------------------------------------------------------------------- the reference's own shape on the oracle
LINK = dict(fs=9600.0, rs=2400.0, L=512, nbytes=64, nsync=32, min_score=28, pairs=16, noise=4600.0, seed=71)


def coded_link_pcm(oracle, noise=None):
    """test_deframe_cpu.link_pcm's pattern with coded packets: continuous PCM at tx_hz = mixer_hz + 50 carrying, at random gaps, pairs of
    [sync_c][coded body] and, right behind it, the same payload UNCODED as [sync_u][scrambled payload + CRC] (test_deframe_cpu.make_packet's layout),
    so both meet the same channel; two sync words, so that each deframer sees only its own packets.
    -> dict(pcm, nblocks, sync_c, sync_u, sent = [(symbol index of the coded word, symbol index of the uncoded word, payload)])"""
    k = LINK
    noise = k["noise"] if noise is None else noise
    Cy = int(k["fs"] / k["rs"])
    nsym = k["L"] // Cy
    rng = np.random.default_rng(k["seed"])
    sync_c = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    sync_u = rng.integers(0, 4, k["nsync"], dtype=np.uint8)
    ks_u = keystream(4 * (k["nbytes"] + 2))
    parts, sent, t = [], [], 0
    for _ in range(k["pairs"]):
        gap = rng.integers(0, 4, int(rng.integers(20, 200)), dtype=np.uint8)
        coded, payload = make_coded_packet(rng, sync_c, k["nbytes"])
        crc = crc16(payload)
        plain = np.concatenate([sync_u, bytes_to_dibits(np.concatenate([payload, np.array([crc >> 8, crc & 0xFF], np.uint8)])) ^ ks_u])
        sent.append((t + len(gap), t + len(gap) + len(coded), payload))
        parts += [gap, coded, plain]
        t += len(gap) + len(coded) + len(plain)
    nblocks = (t + 3 * nsym) // nsym + 1
    sym = np.concatenate(parts + [rng.integers(0, 4, nblocks * nsym - t, dtype=np.uint8)])
    tx = oracle.tx(k["fs"], k["rs"], np.float32(0.35), 1550.0)
    pcm = tx.symbols(np.stack([sym >> 1, sym & 1], axis=1).reshape(-1).astype(np.int32)).astype(np.float64)
    pcm = np.clip(np.round(pcm + noise * rng.standard_normal(pcm.size)), -32768, 32767).astype(np.int16)
    return dict(pcm=pcm, nblocks=nblocks, sync_c=sync_c, sync_u=sync_u, sent=sent)


def link_rows(oracle, lk):
    """rx_frame() block by block (the shipped configuration) -> the costas_frame[] of every block"""
    from oracle.pyoracle import TIMING_FIXED
    k = LINK
    Cy = int(k["fs"] / k["rs"])
    m = oracle.modem(k["fs"], k["rs"], k["L"], timing_mode=TIMING_FIXED, fixed_index=126 % Cy)
    m.set_mixer_hz(1500.0)
    rows = []
    for b in range(lk["nblocks"]):
        m.rx_pcm(lk["pcm"][b * k["L"]:(b + 1) * k["L"]])
        rows.append(np.array(m.costas_frame, np.float32).reshape(-1, 2).copy())
    return rows


def link_verdicts(lk, rows):
    """-> (coded packets that come back with crc_ok and the right payload at the right place, uncoded twins that fail their CRC or are
    missed, the coded packets)"""
    k = LINK
    Cy = int(k["fs"] / k["rs"])
    delay = k["L"] // Cy + 126 // Cy
    coded = flat(deframe_coded_ref(rows, None, lk["sync_c"], k["min_score"], k["nbytes"]))
    plain = deframe_ref(data_rule(np.concatenate(rows)), lk["sync_u"], k["min_score"], k["nbytes"])
    good_c = {p["pos"]: p["bytes"][:k["nbytes"]].tobytes() for p in coded if p["crc_ok"]}
    good_u = {p["pos"]: p["bytes"][:k["nbytes"]].tobytes() for p in plain if p["crc_ok"]}
    ok = sum(good_c.get(tc + delay) == pl.tobytes() for tc, _, pl in lk["sent"])
    lost = sum(good_u.get(tu + delay) != pl.tobytes() for _, tu, pl in lk["sent"])
    return ok, lost, coded


def test_coded_packets_through_the_oracle_stream_pass_where_their_uncoded_twins_fail(oracle):
    """16 pairs of packets (64 payload bytes, 32-dibit sync words, min_score 28) in continuous PCM with additive noise per PCM sample
    (link_pcm's units), received by the CPU oracle's rx_frame() in 512-sample blocks: a coded packet straddles five blocks, and every
    block takes its own gain (UNIT, scale 64, gain = None).  Asserted: every coded packet comes back with crc_ok and its payload at
    t + one block + 126 // CYCLES; at least half of the uncoded twins, through deframe_ref, fail their CRC or are missed.
    The noise level was found on the CPU with these seeds (coded good / 16, uncoded lost / 16, channel bit errors per good coded packet
    of 1068): 3000 -> 16, 0, 0..0;  4000 -> 16, 2, 0..1;  4200 -> 16, 4, 0..3;  4400 -> 16, 9, 0..3;  4600 -> 16, 12, 0..5;
    4800 -> 15, 13, 1..7;  5000 -> 14, 15, 2..8;  6000 -> 2, 16;  7000 and above -> 0, 16 (the word is no longer found).  The step from
    "the hard decisions mostly pass" to "the code no longer holds" is narrow here because rx_frame()'s loop runs at its shipped, wide
    bandwidth: the errors come with its phase jitter, in bursts, as in test_viterbi_cpu.py's batch link."""
    lk = coded_link_pcm(oracle)
    rows = link_rows(oracle, lk)
    ok, lost, coded = link_verdicts(lk, rows)
    errs = [int(p["info"][3]) for p in coded if p["crc_ok"]]
    print("noise %g: coded good %d / %d, uncoded lost %d / %d, channel bit errors per packet %d .. %d of %d"
          % (LINK["noise"], ok, LINK["pairs"], lost, LINK["pairs"], min(errs), max(errs), 2 * coded_steps(LINK["nbytes"])))
    assert ok == LINK["pairs"], ok
    assert lost >= LINK["pairs"] // 2, lost
    assert all(p["info"][1] == 0 and p["info"][2] == 0 for p in coded)
