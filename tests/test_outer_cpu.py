"""The outer link of a continuous stream (qpsk_outer_*, OUTER LINK in include/qpsk_hip.h): word sync, polarity resolution and the Forney byte
deinterleaver behind the stream decoder, and the interleaver that is its transmit twin -- what can be checked without a GPU.

outer_ref and outer_interleave_ref below restate the header in numpy, in integers; the GPU tests (test_outer_gpu.py) compare the kernels with
them bit for bit.  outer_ref keeps every bit since the reset -- no ring, no chunks: it is the definition, not the kernel.  V(u) is formed for
all u with array operations and the state machine loops over events only (a lock, a word, a drop).

What the arguments of qpsk_outer_reset, qpsk_outer_max_words and qpsk_outer_interleave_batch decide by themselves is decided before the
context is looked at, so every such QPSK_ERR_ARG is pinned here, by its error text, without a device; test_outer_gpu.py repeats them on a
context, with the refusals of the push.

The bits test_outer_gpu.py pushes through the device are built here too (outer_gpu_sets and the functions it calls), so that
test_outer_port_cpu.py can run the scalar port of the kernel over the same inputs and say what they would and would not notice.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_rs_cpu import rs_decode_ref, rs_encode_ref
from test_rx_ext_cpu import declared
from test_viterbi_cpu import dibits_to_soft, pack_bits, unpack_bits
from test_viterbi_stream_cpu import conv_encode_stream_ref, viterbi_stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QPSK_ERR_ARG = -2
POLARITY, MSB_FIRST = 1, 2
MAX_BITS = 1 << 20
OUTER_SYMBOLS = ("qpsk_outer_reset", "qpsk_outer_max_words", "qpsk_outer_push", "qpsk_outer_interleave_batch", "qpsk_test_outer_advance")
GEOMETRIES = ((4, 1), (4, 2), (4, 4), (6, 3), (60, 12), (204, 12))


# ------------------------------------------------------------------- the numpy restatement
def outer_interleave_ref(words, branches, history=None):
    """words (R, nwords, n) uint8, history (R, I - 1, n) = the last I - 1 source words before the call, oldest first (None = zeros)
    -> (Y (R, nwords, n) with Y[c][q] = X[c - q mod I][q], the history behind the call)"""
    x = np.asarray(words, np.uint8)
    R, nw, n = x.shape
    I = int(branches)
    assert 2 <= n <= 255 and 1 <= I <= 32 and n % I == 0
    h = np.zeros((R, I - 1, n), np.uint8) if history is None else np.asarray(history, np.uint8)
    assert h.shape == (R, I - 1, n)
    src = np.concatenate([h, x], axis=1)                      # source word c of the call is src[:, c + I - 1]
    q = np.arange(n)
    c = np.arange(nw)[:, None]
    return src[:, c + (I - 1) - q % I, q], src[:, nw:]


def word_bound(lock, n, nbits):
    return lock + -(-nbits // (8 * n))


class _Stream:
    """one stream of outer_ref: every bit since the reset, V(u) for every u that has its eight bits, and the header's state"""

    def __init__(self):
        self.B = np.zeros(0, np.uint8)
        self.V = np.zeros(0, np.int64)
        self.locked, self.h, self.u0, self.s, self.c, self.run = False, 0, 0, 0, 0, 0


class outer_ref:
    """S streams pushed together.  push(bits (S, nbits) of 0 / 1) returns dict(count (S,), words / pos / flags: one array per stream with
    `count` entries, info (S, 4))"""

    HUNT_BLOCK = 4096      # candidates examined at a time: a hunt that resumes after every drop stays linear

    def __init__(self, nstreams, n, branches=1, sync=0x47, lock=2, drop=3, flags=POLARITY):
        assert nstreams >= 1 and 2 <= n <= 255 and 1 <= branches <= 32 and n % branches == 0
        assert 0 <= sync <= 255 and 1 <= lock <= 16 and 0 <= drop <= 16 and not flags & ~(POLARITY | MSB_FIRST)
        self.S, self.n, self.I, self.sync, self.L, self.drop, self.flags = nstreams, n, branches, sync, lock, drop, flags
        self.streams = [_Stream() for _ in range(nstreams)]
        self.advanced = 0      # qpsk_test_outer_advance: added to every pos reported from then on
        self.weights = (1 << (7 - np.arange(8))) if flags & MSB_FIRST else (1 << np.arange(8))

    def max_words(self, nbits):
        assert 1 <= nbits <= MAX_BITS
        return word_bound(self.L, self.n, nbits)

    def advance(self, delta):
        assert delta >= 0 and delta % 8 == 0
        self.advanced += delta

    def _append(self, st, bits):
        old = len(st.V)
        st.B = np.concatenate([st.B, bits])
        if len(st.B) >= 8:
            win = np.lib.stride_tricks.sliding_window_view(st.B[old:], 8).astype(np.int64)
            st.V = np.concatenate([st.V, win @ self.weights])

    def _m(self, v):
        m = (v == self.sync).astype(np.int64)
        if self.flags & POLARITY:
            m -= v == (self.sync ^ 0xFF)
        return m

    def _hunt(self, st):
        """HUNT from st.h: True with the lock declared, False with st.h at the first candidate whose look-ahead has not arrived"""
        step = 8 * self.n
        last = len(st.B) - (step * (self.L - 1) + 8)          # the last candidate whose L bytes are all in
        while st.h <= last:
            a, b = st.h, min(last + 1, st.h + self.HUNT_BLOCK)
            m = self._m(st.V[a:b])
            ok = m != 0
            for i in range(1, self.L):
                ok &= self._m(st.V[a + step * i:b + step * i]) == m
            if ok.any():
                k = int(np.argmax(ok))
                st.locked, st.u0, st.s, st.c, st.run = True, a + k, int(m[k]), 0, 0
                return True
            st.h = b
        return False

    def push(self, bits):
        bits = np.asarray(bits, np.uint8)
        assert bits.ndim == 2 and bits.shape[0] == self.S and 1 <= bits.shape[1] <= MAX_BITS and bits.max() <= 1
        n, I, step = self.n, self.I, 8 * self.n
        q = np.arange(n)
        gather = 8 * q - step * (I - 1 - q % I)               # Z[q] = V(first bit of raw word c + gather[q])
        out = dict(count=np.zeros(self.S, np.int32), words=[], pos=[], flags=[], info=np.zeros((self.S, 4), np.int32))
        for i, st in enumerate(self.streams):
            self._append(st, bits[i])
            words, pos, flags = [], [], []
            while True:
                if not st.locked:
                    if not self._hunt(st):
                        break
                    out["info"][i, 2] += 1
                at = st.u0 + step * st.c
                if at + step > len(st.B):
                    break
                inv = 0xFF if st.s < 0 else 0
                miss = (int(st.V[at]) ^ inv) != self.sync
                st.run = st.run + 1 if miss else 0
                if self.drop > 0 and st.run == self.drop:
                    st.locked, st.h = False, at + 1
                    out["info"][i, 3] += 1
                    continue
                if st.c >= I - 1:
                    z = (st.V[at + gather] ^ inv).astype(np.uint8)
                    words.append(z)
                    pos.append(at + self.advanced)
                    flags.append((1 if z[0] != self.sync else 0) | (2 if st.s < 0 else 0))
                st.c += 1
            out["count"][i] = len(words)
            out["words"].append(np.array(words, np.uint8).reshape(len(words), n))
            out["pos"].append(np.array(pos, np.int64))
            out["flags"].append(np.array(flags, np.uint8))
            out["info"][i, 0], out["info"][i, 1] = int(st.locked), st.s if st.locked else 0
        return out


def bytes_to_bits(b, msb_first=False):
    """(..., k) uint8 -> (..., 8 k) bits in the order they are sent"""
    return np.unpackbits(np.asarray(b, np.uint8), axis=-1, bitorder="big" if msb_first else "little")


def split_sizes(n):
    """the repeating split of the partition tests"""
    return (1, 7, 8, 9, 63, 64, 65, 8 * n - 1, 8 * n, 8 * n + 1)


def cut(total, sizes):
    """[(a, b)] covering [0, total) in pushes of the repeating sizes"""
    spans, a, k = [], 0, 0
    while a < total:
        b = min(total, a + sizes[k % len(sizes)])
        spans.append((a, b))
        a, k = b, k + 1
    return spans


def run_outer(ref, bits, spans):
    """push bits (S, N) in the given spans: (the calls, per stream the concatenated words, pos, flags)"""
    calls = [ref.push(bits[:, a:b]) for a, b in spans]
    S = bits.shape[0]
    words = [np.concatenate([c["words"][i] for c in calls]) for i in range(S)]
    pos = [np.concatenate([c["pos"][i] for c in calls]) for i in range(S)]
    flags = [np.concatenate([c["flags"][i] for c in calls]) for i in range(S)]
    return calls, words, pos, flags


def sync_words(rng, shape, sync=0x47):
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    x[..., 0] = sync
    return x


def damaged_stream(rng, n, I, nwords, lead, kind, sync=0x47):
    """one stream: `lead` random bits, then nwords interleaved words with the sync byte; kind: "clean", "delete" / "insert" (one bit, in the
    middle), "invert" (from two thirds on), or a combination joined with +.  Returns the bits and the source words"""
    x = sync_words(rng, (1, nwords, n), sync)
    y, _ = outer_interleave_ref(x, I)
    b = np.concatenate([rng.integers(0, 2, lead, dtype=np.uint8), bytes_to_bits(y.reshape(-1))])
    for k in kind.split("+"):
        if k == "delete":
            b = np.delete(b, len(b) // 2)
        elif k == "insert":
            b = np.insert(b, len(b) // 2, 1)
        elif k == "invert":
            b = b.copy()
            b[len(b) * 2 // 3:] ^= 1
        else:
            assert k == "clean"
    return b, x[0]


# ------------------------------------------------------------------- what the GPU tests push
# Every input test_outer_gpu.py feeds the device is built here, so that test_outer_port_cpu.py runs the scalar port of the kernel
# (outer_port.py) over literally the same bits: the GPU tests call these functions, and outer_gpu_sets() calls them over the same parameter
# lists.  An input set is one link: the reset's arguments and its steps, ("push", bits (S, nbits), max_words or None) or ("advance", delta);
# "check", where a set has one, asserts on the reference's outputs alone what the case is there for.
LEADS = (0, 9, 18, 27, 36, 45, 54, 63)      # one lead-in per stream: every value of u0 & 7
GPU_GEOMETRIES = ((4, 1), (4, 2), (4, 4), (6, 3), (255, 1), (204, 12))
GPU_LOCKS = ((1, 0), (2, 1), (3, 2), (1, 2), (3, 0))
GPU_FLAGS = (POLARITY, 0, POLARITY | MSB_FIRST, MSB_FIRST)
GPU_SLIPS = ((4, 2), (6, 3))
GPU_PARTITIONS = ((4, 2, 2, 2), (6, 3, 3, 1), (204, 12, 2, 3))


def streams_of(rng, n, I, nwords, kinds, leads=LEADS, msb_first=False, sync=0x47):
    """one damaged_stream per lead-in, cut to a common length: (bits (S, N), the source words)"""
    made = [damaged_stream(rng, n, I, nwords, lead, kinds[i % len(kinds)], sync) for i, lead in enumerate(leads)]
    if msb_first:      # the same bytes sent high bit first: every byte of the bit stream is reversed in place
        made = [(np.concatenate([b[:lead], b[lead:lead + (len(b) - lead) // 8 * 8].reshape(-1, 8)[:, ::-1].reshape(-1)]), x)
                for (b, x), lead in zip(made, leads)]
    N = min(len(b) for b, _ in made)
    return np.stack([b[:N] for b, _ in made]), [x for _, x in made]


def input_set(what, n, I, L, drop, bits=None, spans=None, steps=None, flags=POLARITY, group=0, sync=0x47, check=None):
    if steps is None:
        steps = [("push", bits[:, a:b], None) for a, b in spans]
    S = next(x[1] for x in steps if x[0] == "push").shape[0]
    return dict(what=what, reset=dict(nstreams=S, n=n, branches=I, sync=sync, lock=L, drop=drop, flags=flags, group=group), steps=steps, check=check)


def geometry_inputs(n, I, L, drop):
    rng = np.random.default_rng(n * 1000 + I * 100 + L * 10 + drop)
    bits, _ = streams_of(rng, n, I, 2 * I + L + 8, ("clean", "delete", "insert"))
    N = bits.shape[1]
    return bits, [(0, N // 3 + 5), (N // 3 + 5, N)]


def polarity_inputs(flags):
    rng = np.random.default_rng(flags + 5)
    bits, x = streams_of(rng, 6, 3, 40, ("clean",), msb_first=bool(flags & MSB_FIRST), sync=0x47)
    bits[1::2] ^= 1                                           # every other stream inverted
    N = bits.shape[1]
    return bits, x, [(0, N // 2 + 3), (N // 2 + 3, N)]


def slip_inputs(n, I, across):
    rng = np.random.default_rng(n + I + across)
    bits, _ = streams_of(rng, n, I, 90, ("delete+invert", "insert+invert", "invert", "delete"))
    N = bits.shape[1]
    # the slips sit near N / 2, the inversion at 2 N / 3: inside one push, or with a push boundary on each
    return bits, [(0, N // 2), (N // 2, N * 2 // 3 + 30), (N * 2 // 3 + 30, N)] if across else [(0, N)]


def partition_inputs(n, I):
    rng = np.random.default_rng(n)
    return streams_of(rng, n, I, 2 * I + 14 if n > 100 else 70, ("delete", "clean", "insert+invert"))[0]


def big16_inputs():
    rng = np.random.default_rng(16)
    return streams_of(rng, 4, 2, (1 << 16) // 32 + 80, ("clean", "delete"), leads=(0, 13, 70))[0]


def big20_inputs():
    rng = np.random.default_rng(20)
    return streams_of(rng, 204, 12, (1 << 20) // 1632 + 2, ("clean", "delete+invert"), leads=(5, 62))[0][:, :1 << 20]


def layout_inputs():
    rng = np.random.default_rng(6)
    bits, _ = streams_of(rng, 6, 3, 60, ("clean", "insert"))
    return bits, cut(bits.shape[1], (301, 299, 403, 211, 97))


def positions_inputs():
    rng = np.random.default_rng(31)
    return streams_of(rng, 6, 3, 90, ("delete+invert", "insert"))[0]


def refusal_inputs():
    rng = np.random.default_rng(8)
    return streams_of(rng, 6, 3, 60, ("clean", "delete"))[0]


def replaced_link_inputs():
    rng = np.random.default_rng(88)
    bits, _ = streams_of(rng, 4, 2, 40, ("clean",))
    other, _ = streams_of(rng, 6, 3, 30, ("clean",), leads=LEADS[:3])
    return bits, other


def totals(wants):
    """per stream: words emitted, locks declared, locks lost, over all the calls of a link"""
    return (sum(w["count"].astype(np.int64) for w in wants), sum(w["info"][:, 2].astype(np.int64) for w in wants),
            sum(w["info"][:, 3].astype(np.int64) for w in wants))


# a. the limits of the geometry: I = 32 (the gather's lanes 32 .. 63 wrap twice), the longest word I = 32 allows, L = 16 and drop = 16
LIMITS = ((64, 32, 2, 3, False), (32, 32, 3, 2, True), (224, 32, 2, 3, False), (6, 3, 16, 16, False), (4, 1, 16, 3, True))      # n, I, L, drop, split
LIMIT_KINDS = ("clean", "delete", "insert")


def limit_inputs(n, I, L, drop, split):
    """eight streams at the eight lead-ins; a slip sits in the middle, so either half holds the words of a lock, of a drop and of I - 1
    words in flight with some to spare"""
    rng = np.random.default_rng(n * 1000 + I * 100 + L * 10 + drop)
    bits, _ = streams_of(rng, n, I, 2 * (I + L + drop) + 16, LIMIT_KINDS)
    N = bits.shape[1]
    return bits, cut(N, split_sizes(n)) if split else [(0, N // 3 + 5), (N // 3 + 5, N)]


def limit_set(n, I, L, drop, split):
    def check(wants):
        emitted, nlock, nlost = totals(wants)
        assert (emitted > 0).all(), emitted
        if drop == 16:                                        # the streams with a slip lose the lock sixteen misses later and find it again
            slipped = np.array([LIMIT_KINDS[i % 3] != "clean" for i in range(len(LEADS))])
            assert (nlost[slipped] >= 1).all() and (nlock[slipped] >= 2).all(), (nlock, nlost)
    bits, spans = limit_inputs(n, I, L, drop, split)
    return input_set("limits %s" % ((n, I, L, drop),), n, I, L, drop, bits, spans, check=check)


# c. the look-ahead edge: the push that ends on the last bit of a candidate's look-ahead declares the lock, the one a bit shorter does not
EDGES = ((4, 1, 3), (6, 3, 2))              # n, I, L
EDGE_LEADS = range(10)


def edge_stream(n, L, I, lead):
    """`lead` zero bits, then words of a sync byte and a zero body: no candidate but the true one"""
    x = np.zeros((L + I + 3, n), np.uint8)
    x[:, 0] = 0x47
    return np.concatenate([np.zeros(lead, np.uint8), bytes_to_bits(x.reshape(-1))])


def edge_sets(n, I, L):
    """HUNT: every lead-in of 0 .. 9 bits against a cut at lead + span - 2 .. lead + span + 2, the streams whose cut is the same bit
    sharing a link.  LOCKED: the cut on the last bit of raw word L + I - 1 and one bit before it"""
    span, step = 8 * n * (L - 1) + 8, 8 * n
    N = len(edge_stream(n, L, I, 0))
    sets = []
    for k in range(-2, 12):                                   # the cut at span + k: the leads within 2 of k
        leads = [l for l in EDGE_LEADS if abs(k - l) <= 2]
        bits = np.stack([edge_stream(n, L, I, l)[:N] for l in leads])

        def check(wants, leads=leads, k=k):
            for i, l in enumerate(leads):
                assert wants[0]["info"][i, 2] == (1 if k >= l else 0), (k, l, wants[0]["info"][i])
                assert wants[0]["info"][i, 2] + wants[1]["info"][i, 2] == 1 and wants[1]["count"][i] > 0
        sets.append(input_set("hunt edge %s cut at span + %d" % ((n, I, L), k), n, I, L, 3, bits, [(0, span + k), (span + k, N)], check=check))
    words = L + I                                             # raw words whole in the first push: emitted from word I - 1 on
    for j in range(-1, 10):                                   # the cut at step * words + j: on a stream's last bit (lead = j), or one before
        leads = [l for l in EDGE_LEADS if l - j in (0, 1)]
        bits = np.stack([edge_stream(n, L, I, l)[:N] for l in leads])

        def check(wants, leads=leads, j=j):
            for i, l in enumerate(leads):
                assert wants[0]["count"][i] == words - (I - 1) - (l - j), (j, l, wants[0]["count"])
                assert wants[0]["count"][i] + wants[1]["count"][i] == (N - l) // step - (I - 1)
        sets.append(input_set("word edge %s cut at %d words + %d" % ((n, I, L), words, j), n, I, L, 3, bits,
                              [(0, step * words + j), (step * words + j, N)], check=check))
    return sets


# e. hunting through chunks: at (255, 1) and L = 16 a candidate's look-ahead spans 30 608 bits, so four chunks of 8192 bits arrive before
# the first candidate is whole, and the window holds the most a hunt ever keeps
NOISE = dict(n=255, I=1, L=16, drop=3, nbits=6 * 8192, leads=(0, 5))


def noise_set(phase):
    """noise in one push (preceded by a push of `phase` bits, so that it is appended at that bit phase), then a clean stream"""
    p = NOISE
    rng = np.random.default_rng(255 + phase)
    noise = rng.integers(0, 2, (2, phase + p["nbits"]), dtype=np.uint8)
    clean, _ = streams_of(rng, p["n"], p["I"], p["L"] + 4, ("clean",), leads=p["leads"])
    steps = ([("push", noise[:, :phase], None)] if phase else []) + [("push", noise[:, phase:], None), ("push", clean, None)]

    def check(wants):
        for w in wants[:-1]:
            assert not w["count"].any() and not w["info"].any()
        last = wants[-1]
        assert np.array_equal(last["info"], [[1, 1, 1, 0]] * 2) and (last["count"] > 0).all()
        assert [int(x[0]) for x in last["pos"]] == [phase + p["nbits"] + lead for lead in p["leads"]]      # counted from the reset
    return input_set("noise at bit phase %d" % phase, p["n"], p["I"], p["L"], p["drop"], steps=steps, check=check)


# f. max_words = 0: the count is the true count and nothing else is written
def no_slots_set():
    bits, _ = streams_of(np.random.default_rng(60), 6, 3, 40, ("clean", "insert"))
    N = bits.shape[1]
    steps = [("push", bits[:, :N // 3], None), ("push", bits[:, N // 3:2 * N // 3], 0), ("push", bits[:, 2 * N // 3:], None)]

    def check(wants):
        assert (wants[1]["count"] > 0).all() and (wants[2]["count"] > 0).all()
    return input_set("max_words = 0", 6, 3, 2, 2, steps=steps, check=check)


def outer_gpu_sets(new=True):
    """every link test_outer_gpu.py pushes through the device (new=False: without the cases a and c above)"""
    sets = []
    if new:
        sets += [s for n, I, L in EDGES for s in edge_sets(n, I, L)]
        sets += [limit_set(*case) for case in LIMITS]
    sets += [no_slots_set(), noise_set(0), noise_set(3)]
    for n, I in GPU_GEOMETRIES:
        for L, drop in GPU_LOCKS:
            sets.append(input_set("geometry %s" % ((n, I, L, drop),), n, I, L, drop, *geometry_inputs(n, I, L, drop)))
    for flags in GPU_FLAGS:
        bits, _, spans = polarity_inputs(flags)
        sets.append(input_set("polarity and bit order %d" % flags, 6, 3, 2, 2, bits, spans, flags=flags))
    for n, I in GPU_SLIPS:
        for across in (False, True):
            sets.append(input_set("slips %s" % ((n, I, across),), n, I, 2, 2, *slip_inputs(n, I, across)))
    for n, I, L, drop in GPU_PARTITIONS:
        bits = partition_inputs(n, I)
        N = bits.shape[1]
        sets.append(input_set("the repeating split %s" % ((n, I, L, drop),), n, I, L, drop, bits, cut(N, split_sizes(n))))
        sets.append(input_set("one push %s" % ((n, I, L, drop),), n, I, L, drop, bits, [(0, N)]))
    bits = big16_inputs()
    sets.append(input_set("2^16 bits into three slots", 4, 2, 2, 2, steps=[("push", bits[:, :1 << 16], 3), ("push", bits[:, 1 << 16:], None)]))
    bits = big20_inputs()
    sets.append(input_set("2^20 bits", 204, 12, 2, 3, bits, [(0, 1 << 20)]))
    sets.append(input_set("layout", 6, 3, 2, 2, *layout_inputs()))
    bits = positions_inputs()
    N = bits.shape[1]
    for delta in (1 << 31, 1 << 40):
        sets.append(input_set("positions past %d" % delta, 6, 3, 2, 2, steps=[("push", bits[:, :N // 4], None), ("advance", delta),
                                                                                ("push", bits[:, N // 4:N // 2 + 9], None), ("push", bits[:, N // 2 + 9:], None)]))
    bits = refusal_inputs()
    sets.append(input_set("around the refused calls", 6, 3, 2, 2, bits, [(0, 400), (400, 901), (901, bits.shape[1])]))
    bits, other = replaced_link_inputs()
    sets.append(input_set("the link a reset replaces", 4, 2, 2, 2, bits, [(0, bits.shape[1] // 2)]))
    sets.append(input_set("the link that replaces it", 6, 3, 1, 0, other, [(0, other.shape[1])], flags=0, sync=0xB8))
    for I in (1, 12):
        pushes = [unpack_bits(c["bits"], c["nbits"]) for c in link_result()[I]["vcalls"] if c["nbits"]]
        sets.append(input_set("the link at I = %d" % I, LINK["n"], I, LINK["lock"], LINK["drop"], steps=[("push", b, None) for b in pushes], sync=LINK["sync"]))
    return sets


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_outer_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import torch
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in OUTER_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    for word in ("OUTER LINK", "QPSK_OUTER_POLARITY = 1, QPSK_OUTER_MSB_FIRST = 2", "THE RESULT DEPENDS ONLY ON B", "Forney's interleaver",
                 "the receiver's Z is then X delayed by I - 1 words", "BEFORE RS-encoding it", "DVB's inverted sync byte in every eighth word",
                 "energy dispersal", "cells other than n / I", "streams pushed with different\n * lengths", "quarter-turn (90 degrees) search"):
        assert word in header, word
    for name in ("outer_reset", "outer_max_words", "outer", "outer_interleave", "outer_advance"):
        assert callable(getattr(qpsk_amd.Modem, name, None)), name
    sig = inspect.signature(qpsk_amd.Modem.outer_reset).parameters
    assert [sig[k].default for k in ("branches", "sync", "lock", "drop", "polarity", "msb_first")] == [1, 0x47, 2, 3, True, False]
    assert list(inspect.signature(qpsk_amd.Modem.outer).parameters) == ["self", "bits", "nbits", "pitch", "max_words"]
    assert list(inspect.signature(qpsk_amd.Modem.outer_interleave).parameters) == ["self", "words", "branches", "history"]
    assert (qpsk_amd.lib.OUTER_POLARITY, qpsk_amd.lib.OUTER_MSB_FIRST) == (POLARITY, MSB_FIRST)
    assert "outer.o" in open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    # no context, no work: the entry points refuse a NULL one with QPSK_ERR_ARG on any machine
    buf, cnt = (C.c_uint8 * 64)(), (C.c_int32 * 4)()
    assert qpsk_lib.qpsk_outer_reset(None, 1, 4, 1, 0x47, 2, 3, POLARITY) == QPSK_ERR_ARG
    assert b"qpsk_outer_reset" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_outer_max_words(None, 64) == QPSK_ERR_ARG
    assert b"qpsk_outer_max_words" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_outer_push(None, buf, 0, 64, 1, cnt, buf, 0, None, None, None) == QPSK_ERR_ARG
    assert b"qpsk_outer_push" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_outer_interleave_batch(None, buf, 1, 2, 4, 2, None, None, buf) == QPSK_ERR_ARG
    assert b"qpsk_outer_interleave_batch" in qpsk_lib.qpsk_last_error()
    for delta in (0, 1 << 40, -8):
        assert qpsk_lib.qpsk_test_outer_advance(None, delta) == QPSK_ERR_ARG
    assert b"qpsk_test_outer_advance" in qpsk_lib.qpsk_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(qpsk_amd.QpskError):
            qpsk_amd.Modem().outer_reset(1, 4)


def test_every_argument_error_decided_before_a_device_is_touched(qpsk_lib):
    """reset, max_words and the interleaver check their arguments before they look at the context: with a NULL context the error text
    names the argument, and only a call whose arguments are in order gets as far as "null context" """
    L = qpsk_lib
    buf, out = (C.c_uint8 * 256)(), (C.c_uint8 * 256)()

    def refused(rc, text):
        assert rc == QPSK_ERR_ARG and text in L.qpsk_last_error(), (rc, text, L.qpsk_last_error())
    good = dict(nstreams=1, n=6, branches=3, sync=0x47, lock=2, drop=3, flags=POLARITY | MSB_FIRST)
    reset = lambda **k: L.qpsk_outer_reset(None, *[{**good, **k}[a] for a in ("nstreams", "n", "branches", "sync", "lock", "drop", "flags")])
    refused(reset(), b"null context")
    for k, text in ((dict(nstreams=0), b"nstreams = 0"), (dict(nstreams=-3), b"nstreams = -3"), (dict(n=1, branches=1), b"n = 1 outside"),
                    (dict(n=256, branches=1), b"n = 256 outside"), (dict(branches=0), b"branches = 0"), (dict(branches=4), b"branches = 4"),
                    (dict(n=66, branches=33), b"branches = 33"), (dict(sync=-1), b"sync = -1"), (dict(sync=256), b"sync = 256"),
                    (dict(lock=0), b"lock = 0"), (dict(lock=17), b"lock = 17"), (dict(drop=-1), b"drop = -1"), (dict(drop=17), b"drop = 17"),
                    (dict(flags=4), b"unknown flags 0x4")):
        refused(reset(**k), text)
    for n, I in GEOMETRIES + ((255, 1), (2, 2), (64, 32)):     # the corners of the ranges pass the argument checks
        refused(reset(n=n, branches=I, lock=16, drop=0, flags=0), b"null context")
    for nbits, text in ((0, b"nbits = 0"), (-1, b"nbits = -1"), (MAX_BITS + 1, b"nbits = 1048577"), (1, b"null context"), (MAX_BITS, b"null context")):
        refused(L.qpsk_outer_max_words(None, nbits), text)
    at = lambda b, off=0: C.c_void_p(C.addressof(b) + off)
    il = lambda words=at(buf), nrows=2, nwords=5, n=6, I=3, hin=None, hout=None, o=at(out): L.qpsk_outer_interleave_batch(None, words, nrows, nwords, n, I, hin, hout, o)
    refused(il(), b"null context")
    refused(il(hin=at(buf, 100), hout=at(out, 100)), b"null context")
    for k, text in ((dict(words=None), b"null d_words or d_out"), (dict(o=None), b"null d_words or d_out"), (dict(n=1, I=1), b"n = 1 outside"),
                    (dict(n=256, I=1), b"n = 256 outside"), (dict(I=0), b"branches = 0"), (dict(I=4), b"branches = 4"), (dict(n=66, I=33), b"branches = 33"),
                    (dict(nrows=0), b"nrows = 0"), (dict(nwords=0), b"nwords = 0"), (dict(nwords=(1 << 20) + 1), b"nwords = 1048577"),
                    (dict(o=at(buf)), b"d_out overlaps an input"), (dict(o=at(buf, 59)), b"d_out overlaps an input"),
                    (dict(hin=at(out, 59)), b"d_out overlaps an input"), (dict(hin=at(buf, 100), hout=at(buf, 123)), b"d_hist_out overlaps an input"),
                    (dict(hout=at(buf, 40)), b"d_hist_out overlaps an input"), (dict(hout=at(out, 59)), b"d_hist_out overlaps d_out")):
        refused(il(**k), text)
    refused(il(o=at(buf, 60)), b"null context")               # abutting, not overlapping
    # the boundary of every pair, a byte on either side: the words are 2 * 5 * 6 = 60 bytes, a history 2 * 2 * 6 = 24
    for k, text in ((dict(words=at(buf, 59), o=at(buf)), b"d_out overlaps an input"), (dict(hin=at(out, 23), o=at(out, 46)), b"d_out overlaps an input"),
                    (dict(hout=at(buf, 59)), b"d_hist_out overlaps an input"), (dict(words=at(buf, 23), hout=at(buf)), b"d_hist_out overlaps an input"),
                    (dict(hin=at(buf, 123), hout=at(buf, 100)), b"d_hist_out overlaps an input"), (dict(o=at(out, 23), hout=at(out)), b"d_hist_out overlaps d_out")):
        refused(il(**k), text)                                # one shared byte
    for k in (dict(words=at(buf, 60), o=at(buf)), dict(hin=at(out, 60)), dict(hin=at(out, 22), o=at(out, 46)), dict(hout=at(buf, 60)),
              dict(words=at(buf, 24), hout=at(buf)), dict(hin=at(buf, 100), hout=at(buf, 124)), dict(hin=at(buf, 124), hout=at(buf, 100)),
              dict(hout=at(out, 60)), dict(o=at(out, 24), hout=at(out)), dict(hin=at(buf, 100)), dict(hout=at(buf, 100))):
        refused(il(**k), b"null context")                     # touching on either side; one history without the other


# ------------------------------------------------------------------- 2. the interleaver is Forney's
def forney_fifo_bank(x, I, M):
    """the textbook: branch j is a FIFO of j M zero-filled cells, a commutator steps one branch per byte"""
    fifos = [[0] * (j * M) for j in range(I)]
    y = []
    for t, b in enumerate(x):
        f = fifos[t % I]
        f.append(int(b))
        y.append(f.pop(0))
    return np.array(y, np.uint8)


@pytest.mark.parametrize("n,I", GEOMETRIES)
def test_the_closed_form_is_a_bank_of_fifos_with_a_commutator(n, I):
    rng = np.random.default_rng(n * 100 + I)
    x = rng.integers(0, 256, (1, 3 * I + 5, n), dtype=np.uint8)
    y, hist = outer_interleave_ref(x, I)
    np.testing.assert_array_equal(y.reshape(-1), forney_fifo_bank(x.reshape(-1), I, n // I))
    np.testing.assert_array_equal(hist, x[:, x.shape[1] - (I - 1):])


@pytest.mark.parametrize("n,I", GEOMETRIES)
def test_a_history_carried_over_several_calls_equals_one_call(n, I):
    rng = np.random.default_rng(n + I)
    x = rng.integers(0, 256, (3, 2 * I + 7, n), dtype=np.uint8)
    whole, whole_hist = outer_interleave_ref(x, I)
    hist, parts = None, []
    for a, b in ((0, 1), (1, 3), (3, I + 4), (I + 4, x.shape[1])):      # calls shorter than the history among them
        y, hist = outer_interleave_ref(x[:, a:b], I, hist)
        parts.append(y)
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), whole)
    np.testing.assert_array_equal(hist, whole_hist)


# ------------------------------------------------------------------- 3. the receiver undoes it
@pytest.mark.parametrize("n,I", GEOMETRIES)
@pytest.mark.parametrize("flags", [POLARITY, POLARITY | MSB_FIRST])
def test_the_receiver_returns_the_words_delayed_by_the_branches(n, I, flags):
    rng = np.random.default_rng(n * 7 + I)
    S, nw = 3, 2 * I + 6
    x = sync_words(rng, (S, nw, n))
    # sync bytes only where they belong: a random 0x47 / 0xB8 in the lead-in or the data could lock the hunt on a false word (the GPU tests
    # are full of those); here the lock must fall on the first word
    body = x[:, :, 1:]
    body[(body == 0x47) | (body == 0xB8)] = 0
    y, _ = outer_interleave_ref(x, I)
    bits = bytes_to_bits(y.reshape(S, -1), bool(flags & MSB_FIRST))
    ref = outer_ref(S, n, I, 0x47, lock=2, drop=3, flags=flags)
    calls, words, pos, fl = run_outer(ref, bits, [(0, bits.shape[1])])
    for i in range(S):
        np.testing.assert_array_equal(words[i], x[i, :nw - (I - 1)])
        np.testing.assert_array_equal(pos[i], 8 * n * np.arange(I - 1, nw))
        assert not fl[i].any()
    np.testing.assert_array_equal(calls[0]["info"], [[1, 1, 1, 0]] * S)


# ------------------------------------------------------------------- 4. partition independence and the word bound
CASES = [(n, I, L, drop, kind) for (n, I) in ((4, 1), (4, 2), (4, 4), (6, 3), (12, 4)) for (L, drop, kind) in
         ((1, 0, "clean"), (2, 1, "delete+invert"), (3, 2, "insert"), (2, 3, "delete"), (1, 1, "invert"))]


@pytest.mark.parametrize("n,I,L,drop,kind", CASES)
def test_the_cuts_between_pushes_change_nothing_and_the_word_bound_holds(n, I, L, drop, kind):
    """The header's bound L + ceil(nbits / 8 n) must hold in every push.  It is never met with equality: the words a push emits have their
    last bits at least 8 n apart (within a lock by construction; across a drop and a relock the dropped word lies between), so at most
    ceil(nbits / 8 n) of them end inside the push, and only the lock the push declares can add words that ended before it: raw words
    0 .. L-2, that is L - 1.  The tightest a push comes is therefore L - 1 + ceil(nbits / 8 n), one below the bound, and
    test_a_push_that_completes_a_lock_comes_within_one_word_of_the_bound shows a push that reaches it."""
    rng = np.random.default_rng(n * 1000 + I * 100 + L * 10 + drop)
    streams = [damaged_stream(rng, n, I, 60, int(rng.integers(0, 71)), kind)[0] for _ in range(4)]
    N = min(len(b) for b in streams)
    bits = np.stack([b[:N] for b in streams])
    _, one_w, one_p, one_f = run_outer(outer_ref(4, n, I, 0x47, L, drop), bits, [(0, N)])
    assert sum(len(w) for w in one_w) > 40                    # the case does emit
    for sizes in ((1,), split_sizes(n), (1000,)):
        spans = cut(N, sizes)
        calls, w, p, f = run_outer(outer_ref(4, n, I, 0x47, L, drop), bits, spans)
        for (a, b), c in zip(spans, calls):
            assert (c["count"] <= word_bound(L, n, b - a) - 1).all(), (a, b, c["count"])
        for i in range(4):
            np.testing.assert_array_equal(w[i], one_w[i])
            np.testing.assert_array_equal(p[i], one_p[i])
            np.testing.assert_array_equal(f[i], one_f[i])


@pytest.mark.parametrize("L", [1, 2, 3, 16])
def test_a_push_that_completes_a_lock_comes_within_one_word_of_the_bound(L):
    n = 4
    x = np.zeros((1, L + 3, n), np.uint8)
    x[:, :, 0] = 0x47
    bits = bytes_to_bits(x.reshape(1, -1))
    lock_bit = 8 * n * (L - 1) + 7                            # the bit that declares the lock: L - 1 whole words lie behind it
    for k in (1, 2):                                          # the push ends with the last bit of raw word L - 2 + k
        ref = outer_ref(1, n, 1, 0x47, lock=L, drop=3)
        assert ref.push(bits[:, :lock_bit])["count"][0] == 0
        nbits = 8 * n * k - 7
        got = ref.push(bits[:, lock_bit:lock_bit + nbits])
        assert got["count"][0] == L - 1 + k == word_bound(L, n, nbits) - 1
        np.testing.assert_array_equal(got["info"], [[1, 1, 1, 0]])
        np.testing.assert_array_equal(got["pos"][0], 8 * n * np.arange(L - 1 + k))


def test_slips_drop_the_lock_and_an_inverted_stream_locks_with_the_other_sign():
    rng = np.random.default_rng(47)
    n, I = 6, 3
    b, x = damaged_stream(rng, n, I, 80, 13, "delete+invert")
    ref = outer_ref(1, n, I, 0x47, lock=2, drop=2)
    calls, w, p, f = run_outer(ref, b[None, :], cut(len(b), (97,)))
    info = np.array([c["info"][0] for c in calls])
    assert info[:, 2].sum() >= 3 and info[:, 3].sum() >= 2   # the slip and the inversion each cost the lock
    assert (f[0] & 2).any() and not (f[0][:10] & 2).any()     # s = -1 behind the inversion
    # every word emitted under the last lock is a source word, inverted stream or not
    tail = w[0][-10:]
    assert any((tail == x[k:k + 10]).all() for k in range(len(x) - 10 + 1))
    # without POLARITY the inverted part never locks
    ref = outer_ref(1, n, I, 0x47, lock=2, drop=2, flags=0)
    calls, w0, p0, f0 = run_outer(ref, b[None, :], [(0, len(b))])
    assert not (f0[0] & 2).any() and calls[0]["info"][0, 1] >= 0 and len(w0[0]) < len(w[0])


# ------------------------------------------------------------------- 5. a link on the restatements alone
# Words of RS (60, 44) with the sync byte as byte 0 of the data -> interleaver -> bits -> rate 1/2 at +-64 -> a half turn (both soft values
# negated) -> one run of RUN inverted dibits -> the stream decoder at (128, 256) -> outer_ref with POLARITY -> RS decode.  The code is
# transparent, so the half turn comes out as the inverted bit stream (s = -1) and the run as RUN inverted bits with a few errors at either
# end: RUN / 8 = 50 wrong bytes in a row.  Without interleaving they land in one or two words of 60 and exceed the radius of 8; behind
# I = 12 a source word gets ceil(50 / 12) = 5 of them.  RUN = 400 was chosen on these restatements; measured there: I = 1: 2 of the 39 emitted
# words fail their decode (the run straddles a word boundary; the 37 others are clean), I = 12: 0 of 28 fail, 13 are repaired, of at most 5
# bytes each (the figures are also in DESIGN.md 4.4.14).
LINK = dict(n=60, k=44, nwords=40, run=400, at=9000, depth=128, window=256, seed=6044, sync=0x47, lock=2, drop=3)
_LINK = {}


def link_result():
    """computed once, shared with test_outer_gpu.py: per I the sent words, every stage's output and the decode"""
    if _LINK:
        return _LINK
    p = LINK
    rng = np.random.default_rng(p["seed"])
    data = sync_words(rng, (p["nwords"], p["k"]), p["sync"])
    sent = rs_encode_ref(data, p["n"] - p["k"])              # systematic: byte 0 stays the sync byte
    for I in (1, 12):
        y, _ = outer_interleave_ref(sent[None], I)
        tx_bits = bytes_to_bits(y.reshape(1, -1))
        nbits = tx_bits.shape[1]
        dibits, _ = conv_encode_stream_ref(pack_bits(tx_bits), nbits)
        soft = -dibits_to_soft(dibits).astype(np.int16)      # the half turn
        soft[:, p["at"]:p["at"] + p["run"]] *= -1            # the run
        soft = soft.astype(np.int8)
        dec = viterbi_stream_ref(1, p["depth"], p["window"])
        cuts = [0, 4096, 4096 + 2048, 12288, nbits]
        vcalls = [dec.push(soft[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        vcalls.append(dec.flush())
        ref = outer_ref(1, p["n"], I, p["sync"], p["lock"], p["drop"], POLARITY)
        ocalls = [ref.push(unpack_bits(c["bits"], c["nbits"])) for c in vcalls if c["nbits"]]
        words = np.concatenate([c["words"][0] for c in ocalls])
        out, info = rs_decode_ref(words, p["n"] - p["k"])
        _LINK[I] = dict(sent=sent, interleaved=y[0], dibits=dibits, soft=soft, cuts=cuts, vcalls=vcalls, ocalls=ocalls, words=words,
                        flags=np.concatenate([c["flags"][0] for c in ocalls]), pos=np.concatenate([c["pos"][0] for c in ocalls]),
                        decoded=out, info=info)
    return _LINK


def test_a_burst_that_breaks_a_word_without_the_interleaver_is_repaired_behind_it():
    r = link_result()
    p = LINK
    one, twelve = r[1], r[12]
    # the half turn: s = -1 on every word, every byte right behind the decode
    for x in (one, twelve):
        assert (x["flags"] & 2).all()
        assert x["ocalls"][-1]["info"][0, 0] == 1 and x["ocalls"][-1]["info"][0, 1] == -1
        assert sum(c["info"][0, 3] for c in x["ocalls"]) == 0      # the burst costs a sync byte or two, never the lock
        np.testing.assert_array_equal(np.diff(x["pos"]), 8 * p["n"])
    # the decoder starts in state 0 and the inverted stream does not: the first bits are wrong, the hunt passes over word 0 and locks on word 1
    assert one["pos"][0] == 8 * p["n"] and twelve["pos"][0] == 8 * p["n"] * 12
    assert len(one["words"]) == 39 and len(twelve["words"]) == 28
    failed = one["info"][:, 0] < 0
    assert failed.sum() == 2 and (one["info"][~failed, 0] == 0).all()
    np.testing.assert_array_equal(one["decoded"][~failed], one["sent"][1:40][~failed])
    assert ((one["decoded"][failed] != one["sent"][1:40][failed]).sum(axis=1) > 8).all()
    # behind 12 branches: every emitted word decodes to what was sent, I - 1 words late
    assert (twelve["info"][:, 0] >= 0).all() and (twelve["info"][:, 0] > 0).sum() == 13
    assert twelve["info"][:, 0].max() == 5
    np.testing.assert_array_equal(twelve["decoded"], twelve["sent"][1:29])
