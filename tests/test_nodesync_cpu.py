"""The node sync in front of the streaming Viterbi decoder (qpsk_nodesync_*, NODE SYNC in include/qpsk_hip.h): what can be checked without a
GPU.

nodesync_ref below restates the header in numpy, in integers; the GPU tests (test_nodesync_gpu.py) compare the kernel with it bit for bit.  The
restatement keeps every input dibit since the reset -- no tail buffer -- and a literal tick: it is the definition, not the kernel.  The closed
loops run it against viterbi_stream_ref, each push's `info` fed into the next tick, and are computed once and shared with the GPU tests.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_outer_cpu import POLARITY, bytes_to_bits, outer_ref, sync_words
from test_punct_cpu import BAD_PATTERNS, NAMED, popc
from test_rs_cpu import rs_decode_ref, rs_encode_ref
from test_rx_ext_cpu import declared
from test_soft_cpu import soft_ref
from test_viterbi_cpu import dibits_to_soft, pack_bits, unpack_bits
from test_viterbi_stream_cpu import conv_encode_stream_ref, random_soft, viterbi_stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QPSK_ERR_ARG = -2
NODESYNC_SYMBOLS = ("qpsk_nodesync_reset", "qpsk_nodesync_shifts", "qpsk_nodesync_push", "qpsk_nodesync_set")
SHIFTS = {"1/2": 1, "2/3": 3, "3/4": 2, "5/6": 3, "7/8": 4}
# The threshold per rate.  A right candidate has to read below thr / 2 and a wrong one above 2 thr, in the table's long run and in every span
# of the closed loops, which are a third as long and scatter more.  The table of the issue that asked for the node sync (right candidates
# 0.001 - 0.005 at every rate; wrong ones from 0.136 at rate 1/2 down to 0.032 at 7/8, because a punctured step offers fewer values to disagree
# with) leaves thr the range (2 x 0.005, wrong / 2) = (0.010, 0.068 / 0.043 / 0.031 / 0.021 / 0.016): each value below sits inside its range,
# nearer the lower end at the low rates, where a short span's few errors weigh more, and in the middle at 7/8, where there is no room to choose.
# (1/16, 1/32 and 1/64 for 1/2, 3/4 and 7/8 would put 2 thr at 0.125, 0.0625 and 0.031, on top of the wrong candidates' 0.136, 0.063 and 0.032.)
THRESHOLD = {"1/2": (1, 32), "2/3": (1, 48), "3/4": (1, 48), "5/6": (1, 64), "7/8": (1, 80)}


# ------------------------------------------------------------------- the numpy restatement
def minus128(x):
    """the -128 rule"""
    x = np.asarray(x, np.int8)
    return np.where(x == -128, np.int8(-127), x).astype(np.int8)


def turn_ref(x, r):
    """x (..., 2) int8 without -128 -> turn_r of every pair"""
    a, b = x[..., 0].astype(np.int16), x[..., 1].astype(np.int16)
    u, v = ((a, b), (b, -a), (-a, -b), (-b, a))[r & 3]
    return np.stack([u, v], axis=-1).astype(np.int8)


def shifts_ref(pattern):
    K = popc(pattern[1]) + popc(pattern[2])
    return K if K % 2 else K // 2


class nodesync_ref:
    """S links pushed together.  push(soft (S, ntx, 2) int8, vinfo (S, 4) or None) returns dict(soft (S, ntx, 2) int8, info (S, 8) int32)"""

    def __init__(self, nlinks, nrot=2, nshift=1, span=4096, settle=1024, threshold=(1, 32), drop=2):
        num, den = threshold
        assert nlinks >= 1 and nrot in (1, 2, 4) and 1 <= nshift <= 32 and 1 <= span <= 1 << 24 and 0 <= settle <= 1 << 24
        assert 0 <= num <= 65535 and 1 <= den <= 65535 and 1 <= drop <= 16
        self.S, self.nrot, self.nshift, self.C = nlinks, nrot, nshift, nrot * nshift
        self.span, self.settle, self.num, self.den, self.drop = span, settle, num, den, drop
        self.X = np.zeros((nlinks, 0, 2), np.int8)            # every input dibit since the reset, after the -128 rule
        self.st = [dict(c=0, locked=0, run=0, err=0, cnt=0, settle_left=0, switches=0) for _ in range(nlinks)]

    def set(self, cand=None):
        for l, s in enumerate(self.st):
            s.update(c=0 if cand is None else int(np.uint32(np.int32(cand[l]))) % self.C, err=0, cnt=0, run=0, locked=0, settle_left=self.settle)

    def tick(self, s, e, n):
        verdict = 0
        if n > 0:
            if s["settle_left"] > 0:
                s["settle_left"] = max(0, s["settle_left"] - n)
                verdict = 3
            else:
                s["err"] += e
                s["cnt"] += n
                assert abs(s["err"]) < 2 ** 31 and s["cnt"] < 2 ** 31      # int32 on the device
                if s["cnt"] >= self.span:
                    bad = s["err"] * self.den > self.num * s["cnt"]         # Python integers: the int64 products
                    s["err"] = s["cnt"] = 0
                    if not bad:
                        s["run"] = 0
                        s["locked"] = 1
                        verdict = 1
                    else:
                        verdict = 2
                        s["run"] += 1
                        if not s["locked"] or s["run"] >= self.drop:
                            s["c"] = (s["c"] + 1) % self.C
                            s["locked"] = 0
                            s["run"] = 0
                            s["settle_left"] = self.settle
                            s["switches"] += 1
        return verdict

    def push(self, soft, vinfo=None):
        soft = np.asarray(soft, np.int8)
        assert soft.ndim == 3 and soft.shape[0] == self.S and soft.shape[2] == 2
        ntx = soft.shape[1]
        assert max(1, self.nshift - 1) <= ntx <= 1 << 20
        total = self.X.shape[1]
        self.X = np.concatenate([self.X, minus128(soft)], axis=1)
        out, info = np.zeros((self.S, ntx, 2), np.int8), np.zeros((self.S, 8), np.int32)
        for l, s in enumerate(self.st):
            verdict = 0 if vinfo is None else self.tick(s, int(vinfo[l][0]), int(vinfo[l][1]))
            r, h = s["c"] % self.nrot, s["c"] // self.nrot
            i = total + np.arange(ntx) - h
            out[l, i >= 0] = turn_ref(self.X[l, i[i >= 0]], r)          # an erasure where the link has not seen the dibit
            info[l] = (r, h, s["locked"], s["switches"], verdict, s["run"], s["err"], s["cnt"])
        return dict(soft=out, info=info)


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_nodesync_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import torch
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in NODESYNC_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    for word in ("NODE SYNC", "-128 IS TAKEN AS -127", "NOTHING DEPENDS ON HOW THE DIBITS WERE CUT INTO PUSHES", "r = c mod nrot, h = c div nrot",
                 "Not built: fan-out of all candidates", "a transform fused into the stream decoder's loader"):
        assert word in header, word
    # the stream sections no longer hand the search to the caller
    assert "the caller does, with d_info[0]" not in header and "which stays with the error ratio" not in header
    for name in ("nodesync_reset", "nodesync", "nodesync_set"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    sig = inspect.signature(qpsk_amd.Modem.nodesync_reset).parameters
    assert [sig[k].default for k in ("nrot", "nshift", "drop")] == [2, 1, 2] and list(sig)[:2] == ["self", "nlinks"]
    assert list(inspect.signature(qpsk_amd.Modem.nodesync).parameters)[:4] == ["self", "soft", "vinfo", "pitch"]
    assert list(inspect.signature(qpsk_amd.Modem.nodesync_set).parameters) == ["self", "cand"]
    mk = open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    assert "nodesync.o" in mk and "api_nodesync.o" in mk
    # no context, no work: the entry points refuse a NULL one with QPSK_ERR_ARG on any machine
    buf, out = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    assert qpsk_lib.qpsk_nodesync_reset(None, 1, 2, 1, 1024, 1024, 1, 32, 2) == QPSK_ERR_ARG
    assert b"qpsk_nodesync_reset: null context" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_nodesync_push(None, buf, 0, 8, None, out, 0, None) == QPSK_ERR_ARG
    assert b"qpsk_nodesync_push" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_nodesync_set(None, None) == QPSK_ERR_ARG
    assert b"qpsk_nodesync_set" in qpsk_lib.qpsk_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(qpsk_amd.QpskError):
            qpsk_amd.Modem().nodesync_reset(1)


def test_every_reset_rule_is_decided_before_a_device_is_touched(qpsk_lib):
    """a reset checks its arguments before it looks at the context: with a NULL context the error text names the argument, and only a call
    whose arguments are in order gets as far as "null context" """
    L = qpsk_lib
    names = ("nlinks", "nrot", "nshift", "span", "settle", "thr_num", "thr_den", "drop")
    good = dict(nlinks=1, nrot=2, nshift=2, span=1024, settle=1024, thr_num=1, thr_den=32, drop=2)

    def refused(k, text):
        rc = L.qpsk_nodesync_reset(None, *[{**good, **k}[a] for a in names])
        assert rc == QPSK_ERR_ARG and text in L.qpsk_last_error(), (k, rc, L.qpsk_last_error())
    for k, text in ((dict(nlinks=0), b"nlinks = 0"), (dict(nlinks=-2), b"nlinks = -2"), (dict(nrot=0), b"nrot = 0"), (dict(nrot=3), b"nrot = 3"),
                    (dict(nrot=8), b"nrot = 8"), (dict(nshift=0), b"nshift = 0"), (dict(nshift=33), b"nshift = 33"), (dict(span=0), b"span = 0"),
                    (dict(span=(1 << 24) + 1), b"span = 16777217"), (dict(settle=-1), b"settle = -1"), (dict(settle=(1 << 24) + 1), b"settle = 16777217"),
                    (dict(thr_num=-1), b"threshold -1 / 32"), (dict(thr_num=65536), b"threshold 65536 / 32"), (dict(thr_den=0), b"threshold 1 / 0"),
                    (dict(thr_den=65536), b"threshold 1 / 65536"), (dict(drop=0), b"drop = 0"), (dict(drop=17), b"drop = 17")):
        refused(k, text)
    for k in (dict(), dict(nrot=1, nshift=1), dict(nrot=4, nshift=32), dict(span=1, settle=0), dict(span=1 << 24, settle=1 << 24),
              dict(thr_num=0, thr_den=1), dict(thr_num=65535, thr_den=65535), dict(drop=1), dict(drop=16)):      # the corners pass
        refused(k, b"null context")


def test_nodesync_shifts_are_the_delays_a_pattern_needs(qpsk_lib):
    import qpsk_amd
    for name, want in SHIFTS.items():
        assert qpsk_lib.qpsk_nodesync_shifts(*NAMED[name]) == want == shifts_ref(NAMED[name]) == qpsk_amd.nodesync_shifts(name)
        assert qpsk_amd.nodesync_shifts(NAMED[name]) == want
    assert qpsk_lib.qpsk_nodesync_shifts(4, 0b1101, 0b1001) == 5       # K = 5, odd: every phase needs its own delay
    assert qpsk_lib.qpsk_nodesync_shifts(32, 0xFFFFFFFF, 0xFFFFFFFF) == 32
    for bad in BAD_PATTERNS:
        assert qpsk_lib.qpsk_nodesync_shifts(*bad) == QPSK_ERR_ARG, bad
        assert b"qpsk_nodesync_shifts" in qpsk_lib.qpsk_last_error()
    with pytest.raises(qpsk_amd.QpskError):
        qpsk_amd.nodesync_shifts((0, 1, 1))


# ------------------------------------------------------------------- 2. the properties the header states
def test_one_candidate_is_the_input_after_the_minus_128_rule():
    rng = np.random.default_rng(1)
    soft = random_soft(rng, 3, 700)
    assert (soft == -128).any() and (soft == 0).any()
    ns = nodesync_ref(3, nrot=1, nshift=1)
    got = np.concatenate([ns.push(soft[:, :33])["soft"], ns.push(soft[:, 33:], vinfo=np.array([[900, 1000, 0, 0]] * 3))["soft"]], axis=1)
    np.testing.assert_array_equal(got, minus128(soft))
    assert not (got == -128).any()
    assert [s["c"] for s in ns.st] == [0, 0, 0] and [s["switches"] for s in ns.st] == [0, 0, 0]       # span 4096: nothing was judged


def test_the_cuts_between_pushes_change_nothing():
    rng = np.random.default_rng(2)
    soft = random_soft(rng, 6, 1200)
    cand = np.array([0, 5, 31 * 4 + 3, 7 * 4 + 2, 8 * 4 + 1, -1], np.int32)      # -1 = 2^32 - 1 = 127 mod 128: (3, 31)
    outs = []
    for cuts in ([], [31, 64, 580], [600], list(range(40, 1200, 40))):
        ns = nodesync_ref(6, nrot=4, nshift=32)
        ns.set(cand)
        outs.append(np.concatenate([ns.push(soft[:, a:b])["soft"] for a, b in zip([0] + cuts, cuts + [1200])], axis=1))
        assert [s["c"] for s in ns.st] == [0, 5, 127, 30, 33, 127]
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])
    x = minus128(soft)
    np.testing.assert_array_equal(outs[0][1, 1:], turn_ref(x[1, :-1], 1))      # c = 5: r = 1, h = 1
    assert not outs[0][1, 0].any() and not outs[0][2, :31].any()               # erasures where the link has seen nothing yet
    np.testing.assert_array_equal(outs[0][2, 31:], turn_ref(x[2, :-31], 3))


def test_the_turn_is_the_soft_decisions_rule():
    """turn_r on the soft pairs of rotation 0 equals soft_ref with rot = r on the same costas_frame[] rows (quantise() is odd and limited to
    +-127, so both are defined everywhere)"""
    rng = np.random.default_rng(3)
    costas = rng.standard_normal((4, 300, 2)).astype(np.float32)
    costas[0, :5] = [[0.0, 1.0], [1e9, -1e9], [0.5 / 64, -0.5 / 64], [1.5 / 64, 2.5 / 64], [-0.0, 3.0]]
    gain = np.full(4, 64.0, np.float32)
    plain = soft_ref(costas, gain=gain)["soft"]
    for r in range(4):
        ns = nodesync_ref(4, nrot=4, nshift=1)
        ns.set(np.full(4, r, np.int32))
        np.testing.assert_array_equal(ns.push(plain)["soft"], soft_ref(costas, gain=gain, rot=np.full(4, r))["soft"])


def test_the_tick_is_a_function_of_the_state_and_the_counts():
    """every branch on hand cases: settle, good, bad while hunting, bad while locked below and at drop, the wrap, n = 0, and products beyond
    32 bits"""
    x = np.zeros((1, 4, 2), np.int8)
    ns = nodesync_ref(1, nrot=2, nshift=2, span=100, settle=50, threshold=(1, 10), drop=2)
    ns.set(np.array([3], np.int32))
    step = lambda e, n: ns.push(x, np.array([[e, n, 0, 0]]))["info"][0].tolist()
    assert ns.push(x)["info"][0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]      # no tick
    assert step(5, 0) == [1, 1, 0, 0, 0, 0, 0, 0]                        # n = 0: nothing, settle_left stays
    assert step(30, 30)[4] == 3 and ns.st[0]["settle_left"] == 20
    assert step(30, 30)[4] == 3 and ns.st[0]["settle_left"] == 0
    assert step(4, 60) == [1, 1, 0, 0, 0, 0, 4, 60]                      # counted, not yet a span
    assert step(6, 40) == [1, 1, 1, 0, 1, 0, 0, 0]                       # 10 / 100 is not above 1 / 10: good, locked
    assert step(11, 100) == [1, 1, 1, 0, 2, 1, 0, 0]                     # bad while locked, below drop
    assert step(0, 100) == [1, 1, 1, 0, 1, 0, 0, 0]                      # a good span clears the run
    assert step(11, 100)[4:6] == [2, 1]
    assert step(11, 100) == [0, 0, 0, 1, 2, 0, 0, 0] and ns.st[0]["settle_left"] == 50      # at drop: the wrap C - 1 -> 0
    assert step(0, 50)[4] == 3
    assert step(50, 100) == [1, 0, 0, 2, 2, 0, 0, 0]                     # bad while hunting: one span moves on
    big = nodesync_ref(1, nrot=1, nshift=1, span=1 << 24, settle=0, threshold=(65535, 65535), drop=1)
    stepb = lambda e, n: big.push(x, np.array([[e, n, 0, 0]]))["info"][0].tolist()
    assert stepb(1 << 23, 1 << 23)[4] == 0
    assert stepb(1 << 23, 1 << 23) == [0, 0, 1, 0, 1, 0, 0, 0]           # 2^24 * 65535 on either side: equal is not above
    assert stepb((1 << 24) + 1, 1 << 24) == [0, 0, 0, 1, 2, 0, 0, 0]     # C = 1: the one candidate again


# ------------------------------------------------------------------- 3. the ratio table
TABLE = dict(depth=128, window=256, sigma=24.0, steps=1680 * 2, seed=2407)
_TABLE = {}


def noisy(rng, dibits, sigma):
    s = dibits_to_soft(dibits).astype(np.float64)
    return np.clip(np.rint(s + rng.normal(0.0, sigma, s.shape)), -127, 127).astype(np.int8)


def ratio_table():
    """per rate: the candidates (r, h) of nrot = 4 x nodesync_shifts and the ratio errors / counted of one push through viterbi_stream_ref,
    every candidate a stream of the same decoder"""
    if _TABLE:
        return _TABLE
    p = TABLE
    for name, pattern in sorted(NAMED.items()):
        rng = np.random.default_rng(p["seed"])
        data = rng.integers(0, 2, (1, p["steps"])).astype(np.uint8)
        soft = noisy(rng, conv_encode_stream_ref(pack_bits(data), p["steps"], pattern)[0], p["sigma"])
        nshift = shifts_ref(pattern)
        C4 = 4 * nshift
        ns = nodesync_ref(C4, nrot=4, nshift=nshift)
        ns.set(np.arange(C4, dtype=np.int32))
        dec = viterbi_stream_ref(C4, p["depth"], p["window"], pattern)
        info = dec.push(ns.push(np.repeat(soft, C4, axis=0))["soft"])["info"].astype(np.int64)
        assert (info[:, 1] > 1500).all()
        _TABLE[name] = [((c % 4, c // 4), info[c, 0] / info[c, 1]) for c in range(C4)]
    return _TABLE


@pytest.mark.parametrize("name", sorted(NAMED))
def test_right_and_wrong_candidates_stand_a_factor_of_two_either_side_of_the_threshold(name):
    num, den = THRESHOLD[name]
    thr = num / den
    rows = ratio_table()[name]
    print(name, " ".join("(%d,%d) %.4f" % (r, h, q) for (r, h), q in rows))
    for (r, h), q in rows:
        if h == 0 and r in (0, 2):
            assert q < thr / 2, (name, r, h, q)
        else:
            assert q > 2 * thr, (name, r, h, q)


# ------------------------------------------------------------------- 4. / 5. the closed loop on the restatements
# Words of RS (60, 44) with the sync byte as byte 0 -> bits -> the code at +-64 with noise -> the channel: a quarter turn (z j^3 = z (-j):
# turn_1 of the table, three quarter turns the other way round) and the first dibit lost -> blocks of 516 dibits through nodesync_ref ->
# viterbi_stream_ref, each push's info into the next tick.  At rate 3/4 with nrot = 2 the candidates are (0, 0), (1, 0), (0, 1), (1, 1): the
# last one stands a half turn off the transmitter -- the data inverted, at the right delay.  Mid-stream one more dibit is lost (a slip): two
# dibits are a whole period of the pattern, so the link has to come back on (1, 0), over the wrap, three data bits early.  The slip's place
# was chosen on these restatements so that it falls between two spans: one that straddles it reads half good and half bad, and no threshold
# judges that by a factor of two (check_spans asserts that none does).
LOOP = dict(n=60, k=44, sync=0x47, depth=128, window=256, block=516, span=1024, settle=1024, drop=2, sigma=24.0, quiet=20)
LOOPS = {"3/4": dict(nrot=2, nwords=88, nblocks=54, turn=1, lost=1, slip=(33, 300), seed=3404),
         "1/2": dict(nrot=4, nwords=20, nblocks=16, turn=3, lost=0, slip=None, seed=1202)}
_LOOP = {}


def loop_result(name):
    """computed once, shared with test_nodesync_gpu.py: the sent words and bits, the received blocks and every call's outputs"""
    if name in _LOOP:
        return _LOOP[name]
    p, q, pattern = LOOP, LOOPS[name], NAMED[name]
    rng = np.random.default_rng(q["seed"])
    sent = rs_encode_ref(sync_words(rng, (q["nwords"], p["k"]), p["sync"]), p["n"] - p["k"])
    data = bytes_to_bits(sent.reshape(1, -1))
    nbits = data.shape[1]
    soft = noisy(rng, conv_encode_stream_ref(pack_bits(data), nbits, pattern)[0], p["sigma"])
    rx = turn_ref(soft, q["turn"])[:, q["lost"]:]
    if q["slip"]:
        rx = np.delete(rx, q["slip"][0] * p["block"] + q["slip"][1], axis=1)
    B = p["block"]
    assert rx.shape[1] >= q["nblocks"] * B
    nshift = shifts_ref(pattern)
    ns = nodesync_ref(1, q["nrot"], nshift, p["span"], p["settle"], THRESHOLD[name], p["drop"])
    dec = viterbi_stream_ref(1, p["depth"], p["window"], pattern)
    blocks, ncalls, vcalls, judged, vinfo = [], [], [], [], None
    for k in range(q["nblocks"]):
        blocks.append(rx[:, k * B:(k + 1) * B])
        before = (ns.st[0]["err"], ns.st[0]["cnt"])
        n = ns.push(blocks[-1], vinfo)
        if n["info"][0, 4] in (1, 2):                         # a span was judged: on which figures
            judged.append((k, int(n["info"][0, 4]), before[0] + int(vinfo[0, 0]), before[1] + int(vinfo[0, 1])))
        v = dec.push(n["soft"])
        vinfo = v["info"]
        ncalls.append(n)
        vcalls.append(v)
    bits = np.concatenate([unpack_bits(v["bits"], v["nbits"]) for v in vcalls], axis=1)
    steps = dec.t // q["nblocks"]                            # trellis steps of a block
    _LOOP[name] = dict(sent=sent, data=data, blocks=blocks, ncalls=ncalls, vcalls=vcalls, judged=judged, bits=bits, steps=steps,
                       nshift=nshift, C=q["nrot"] * nshift, info=np.stack([n["info"][0] for n in ncalls]))
    return _LOOP[name]


def lock_calls(info):
    """the calls at which `locked` rises"""
    locked = info[:, 2]
    return [k for k in range(len(locked)) if locked[k] and (k == 0 or not locked[k - 1])]


def check_spans(name, res):
    """no verdict hangs on a coin flip: every judged span reads outside [thr / 2, 2 thr], and on the side its verdict says"""
    num, den = THRESHOLD[name]
    for k, verdict, err, cnt in res["judged"]:
        print("call %2d verdict %d: %d / %d = %.4f" % (k, verdict, err, cnt, err / cnt))
        assert cnt >= LOOP["span"]
        if verdict == 1:
            assert 2 * err * den < num * cnt, (k, err, cnt)
        else:
            assert err * den > 2 * num * cnt, (k, err, cnt)


def test_the_loop_at_rate_3_4_locks_on_the_half_turn_twin_and_comes_back_after_a_slip():
    p, q, res = LOOP, LOOPS["3/4"], loop_result("3/4")
    info, steps, C = res["info"], res["steps"], res["C"]
    K = 4
    assert C == 4 and steps == 774
    check_spans("3/4", res)
    first, second = lock_calls(info)
    # the first lock: on (1, 1), behind exactly the three wrong candidates, within the bound
    assert info[first, :4].tolist() == [1, 1, 1, 3]
    counted = sum(int(v["info"][0, 1]) for v in res["vcalls"][:first])          # what the ticks up to the locking call were handed
    bound = C * (p["settle"] + 2 * p["span"])
    assert counted <= bound
    # ... and in values pushed: the decoder's latency of depth + window steps and the block by which its info is handed over come on top
    assert 2 * p["block"] * first <= bound + (p["depth"] + p["window"]) * K // 3 + 2 * p["block"]
    # it never moves again over the quiet blocks, and the bits are the data inverted at the right delay from the lock on
    slip_call = q["slip"][0]
    assert slip_call >= first + p["quiet"]
    assert (info[first:slip_call + 1, :4] == [1, 1, 1, 3]).all() and not (info[first:slip_call + 1, 4] == 2).any()
    t0, t1 = steps * first, steps * slip_call - p["depth"] - p["window"]
    np.testing.assert_array_equal(res["bits"][0, t0:t1], 1 - res["data"][0, t0:t1])
    # the slip: exactly `drop` bad spans in a row, the second one unlocks; then the wrap 3 -> 0 (wrong) -> 1, which is right
    after = [(k, v) for k, v, _, _ in res["judged"] if k > slip_call]
    bad = [k for k, v in after if v == 2][:p["drop"]]
    assert [v for k, v in after if k <= bad[-1]][-p["drop"]:] == [2] * p["drop"]
    assert not [k for k, v in after if v == 2 and k < bad[0]] and info[bad[0], 2] == 1 and info[bad[0], 5] == 1
    assert info[bad[-1], :4].tolist() == [0, 0, 0, 4]
    assert info[second, :4].tolist() == [1, 0, 1, 5] and (info[second:, :4] == [1, 0, 1, 5]).all()
    assert sorted(set(info[bad[-1]:second, 0] + 2 * info[bad[-1]:second, 1])) == [0, 1]
    t2 = steps * second
    got = res["bits"][0, t2:]
    assert got.size > 2000
    np.testing.assert_array_equal(got, 1 - res["data"][0, t2 + 3:t2 + 3 + got.size])      # two dibits lost: one period, three bits


def test_the_loop_at_rate_1_2_locks_on_the_first_of_the_two_twins_it_meets():
    p, res = LOOP, loop_result("1/2")
    info, steps = res["info"], res["steps"]
    assert res["C"] == 4 and steps == p["block"]
    check_spans("1/2", res)
    (first,) = lock_calls(info)
    assert info[first, :4].tolist() == [1, 0, 1, 1] and (info[first:, :4] == [1, 0, 1, 1]).all()     # the channel's turn_3 and r = 1: a whole turn
    assert sum(int(v["info"][0, 1]) for v in res["vcalls"][:first]) <= 4 * (p["settle"] + 2 * p["span"])
    t0 = steps * first
    got = res["bits"][0, t0:]
    assert got.size > 1000
    np.testing.assert_array_equal(got, res["data"][0, t0:t0 + got.size])


# ------------------------------------------------------------------- the link behind the loop, on the restatements (shared with the GPU test)
def clean_words(res, pos):
    """which words of the outer link count: every bit decoded while the node sync stood locked on a right candidate -- from the first lock to
    the slip less the decoder's latency, and from the second lock on"""
    p, q = LOOP, LOOPS["3/4"]
    first, second = lock_calls(res["info"])
    t0, t1, t2 = res["steps"] * first, res["steps"] * q["slip"][0] - p["depth"] - p["window"], res["steps"] * second
    pos = np.asarray(pos)
    return ((pos >= t0) & (pos + 8 * p["n"] <= t1)) | (pos >= t2)


def loop_link():
    res = loop_result("3/4")
    if "ocalls" not in res:
        p = LOOP
        ref = outer_ref(1, p["n"], 1, p["sync"], 2, 3, POLARITY)
        res["ocalls"] = [ref.push(unpack_bits(v["bits"], v["nbits"])) if v["nbits"] else None for v in res["vcalls"]]
        oc = [c for c in res["ocalls"] if c is not None]
        res["words"] = np.concatenate([c["words"][0] for c in oc])
        res["pos"] = np.concatenate([c["pos"][0] for c in oc])
        res["flags"] = np.concatenate([c["flags"][0] for c in oc])
        res["decoded"], res["rsinfo"] = rs_decode_ref(res["words"], p["n"] - p["k"])
    return res


def test_every_word_behind_the_lock_decodes_clean():
    p, res = LOOP, loop_link()
    ok = clean_words(res, res["pos"])
    assert ok.sum() >= 40 and (res["flags"][ok] & 2).all()               # the half-turn twin: s = -1
    assert (res["rsinfo"][ok, 0] >= 0).all()
    second = lock_calls(res["info"])[1]
    late = res["pos"] >= res["steps"] * second
    assert late[ok].sum() >= 5
    index = np.where(late, (res["pos"] + 3) // (8 * p["n"]), res["pos"] // (8 * p["n"]))
    assert (res["pos"][ok & ~late] % (8 * p["n"]) == 0).all() and ((res["pos"][ok & late] + 3) % (8 * p["n"]) == 0).all()
    np.testing.assert_array_equal(res["decoded"][ok], res["sent"][index[ok]])
