"""DVB-S transport framing (GROUP SYNC under OUTER LINK and DVB TRANSPORT in include/qpsk_hip.h): the inverted sync byte in every G-th word
and the energy dispersal -- what can be checked without a GPU.

outer_group_ref and dispersal_ref below restate the header in numpy, in integers; the GPU tests (test_dvb_gpu.py) compare the kernels with
them bit for bit.  outer_group_ref extends test_outer_cpu.outer_ref and, like it, keeps every bit since the reset: no ring, no chunks.  It
finds a candidate's (s, g) in a table of every legal sign mask built from the header's e(k), not by the kernel's shift of one mask.
dispersal_ref takes its keystream from a numpy restatement of the generator 1 + x^14 + x^15 as EN 300 421 draws it; the library's
sequence is pinned to the oracle's scrambler (the restatement of the reference's scramble()) and to the bytes the standard prints.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_outer_cpu import (CASES, MSB_FIRST, POLARITY, bytes_to_bits, cut, damaged_stream, input_set, outer_interleave_ref, outer_ref,
                            run_outer, split_sizes, word_bound)
from test_punct_cpu import NAMED
from test_rs_cpu import rs_decode_ref, rs_encode_ref
from test_rx_ext_cpu import declared
from test_viterbi_cpu import dibits_to_soft, pack_bits, unpack_bits
from test_viterbi_stream_cpu import conv_encode_stream_ref, viterbi_stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QPSK_ERR_ARG = -2
DISPERSAL_MSB_FIRST = 1
DVB_SYMBOLS = ("qpsk_outer_reset_group", "qpsk_dispersal_batch", "qpsk_dispersal_sequence")
STANDARD = bytes.fromhex("03F6083430B8A393")                 # EN 300 421: the first bytes of the PRBS, high bit first


# ------------------------------------------------------------------- the numpy restatements
def prbs_bits(nbits):
    """the standard's generator: 15 cells loaded with 100101010000000, the output is cell 14 xor cell 15 and is fed back into cell 1"""
    reg = [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    out = np.zeros(nbits, np.uint8)
    for j in range(nbits):
        out[j] = reg[13] ^ reg[14]
        reg = [int(out[j])] + reg[:14]
    return out


def dispersal_sequence_ref(length=188, group=8, msb_first=False):
    """PR[0 .. group length - 2] as a uint8 array"""
    k = prbs_bits(8 * (group * length - 1)).reshape(-1, 8)
    return np.packbits(k, axis=1, bitorder="big" if msb_first else "little")[:, 0]


def dispersal_ref(rows, group, index, msb_first=False):
    """rows (R, len) uint8, index (R,) = every row's group index (one >= group: the row is copied) -> (R, len)"""
    x = np.atleast_2d(np.asarray(rows, np.uint8))
    R, n = x.shape
    index = np.asarray(index, np.int64)
    assert 2 <= n <= 255 and 1 <= group <= 16 and index.shape == (R,)
    table = np.concatenate([[0xFF], dispersal_sequence_ref(n, group, msb_first)]).astype(np.uint8).reshape(group, n)
    table[1:, 0] = 0                                          # the generator runs through the other sync bytes and leaves them alone
    table = np.concatenate([table, np.zeros((1, n), np.uint8)])
    return x ^ table[np.where(index < group, index, group)]


def legal_masks(G, L, polarity=True):
    """{mask: (s, g)} with bit i of the mask = (s e((i + g) mod G) < 0), and whether no two (s, g) share a mask"""
    table, unique = {}, True
    for s in (1, -1) if polarity else (1,):
        for g in range(G):
            mask = sum(1 << i for i in range(L) if s * (-1 if (i + g) % G == 0 else 1) < 0)
            unique &= mask not in table
            table.setdefault(mask, (s, g))
    return table, unique


class outer_group_ref(outer_ref):
    """outer_ref with qpsk_outer_reset_group's group; group = 0 is outer_ref"""

    def __init__(self, nstreams, n, branches=1, sync=0x47, lock=2, drop=3, flags=POLARITY, group=0):
        super().__init__(nstreams, n, branches, sync, lock, drop, flags)
        assert group == 0 or (3 <= group <= 16 and group <= lock <= 16)
        self.G = group
        if group:
            table, unique = legal_masks(group, lock, bool(flags & POLARITY))
            assert unique
            self.lut_s, self.lut_g = np.zeros(1 << lock, np.int64), np.zeros(1 << lock, np.int64)
            for mask, (s, g) in table.items():
                self.lut_s[mask], self.lut_g[mask] = s, g

    def _m2(self, v):
        """m(u) of group mode: both signs, whatever POLARITY says"""
        return (v == self.sync).astype(np.int64) - (v == (self.sync ^ 0xFF))

    def _hunt(self, st):
        if not self.G:
            return super()._hunt(st)
        step = 8 * self.n
        last = len(st.B) - (step * (self.L - 1) + 8)
        while st.h <= last:
            a, b = st.h, min(last + 1, st.h + self.HUNT_BLOCK)
            ok, mask = np.ones(b - a, bool), np.zeros(b - a, np.int64)
            for i in range(self.L):
                m = self._m2(st.V[a + step * i:b + step * i])
                ok &= m != 0
                mask |= (m < 0).astype(np.int64) << i
            ok &= self.lut_s[mask] != 0                      # L sync bytes whose signs fit no (s, g) are not a lock
            if ok.any():
                k = int(np.argmax(ok))
                st.locked, st.u0, st.s, st.g, st.c, st.run = True, a + k, int(self.lut_s[mask[k]]), int(self.lut_g[mask[k]]), 0, 0
                return True
            st.h = b
        return False

    def push(self, bits):
        if not self.G:
            return super().push(bits)
        bits = np.asarray(bits, np.uint8)
        assert bits.ndim == 2 and bits.shape[0] == self.S and 1 <= bits.shape[1] <= 1 << 20 and bits.max() <= 1
        n, I, G, step = self.n, self.I, self.G, 8 * self.n
        q = np.arange(n)
        gather = 8 * q - step * (I - 1 - q % I)
        expect = lambda k: self.sync ^ (0xFF if k == 0 else 0)
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
                miss = (int(st.V[at]) ^ inv) != expect((st.g + st.c) % G)
                st.run = st.run + 1 if miss else 0
                if self.drop > 0 and st.run == self.drop:
                    st.locked, st.h, st.g = False, at + 1, None
                    out["info"][i, 3] += 1
                    continue
                if st.c >= I - 1:
                    z = (st.V[at + gather] ^ inv).astype(np.uint8)
                    kz = (st.g + st.c - (I - 1)) % G
                    words.append(z)
                    pos.append(at + self.advanced)
                    flags.append((1 if z[0] != expect(kz) else 0) | (2 if st.s < 0 else 0) | kz << 4)
                st.c += 1
            out["count"][i] = len(words)
            out["words"].append(np.array(words, np.uint8).reshape(len(words), n))
            out["pos"].append(np.array(pos, np.int64))
            out["flags"].append(np.array(flags, np.uint8))
            out["info"][i, 0], out["info"][i, 1] = int(st.locked), st.s if st.locked else 0
        return out


def group_words(rng, nwords, n, G, phase, sync=0x47, plain_body=False):
    """source words: word w has the group index (w + phase) mod G and the first byte that goes with it; plain_body: no other byte equals
    the sync byte or its complement"""
    x = rng.integers(0, 256, (nwords, n), dtype=np.uint8)
    if plain_body:
        x[(x == sync) | (x == sync ^ 0xFF)] = 0
    x[:, 0] = np.where((np.arange(nwords) + phase) % G == 0, sync ^ 0xFF, sync)
    return x


DECOY_GAP = 13      # bits between a decoy and the stream behind it: the two are not word-aligned, so no candidate straddles them legally


def group_stream(rng, n, I, G, L, nwords, lead=0, phase=0, kind="clean", invert=False, msb_first=False, sync=0x47, plain_body=False):
    """one stream: `lead` random bits, for kind "decoy" L raw words whose first bytes are all the sync byte or its complement in a sign
    pattern no (s, g) gives, and DECOY_GAP bits, then nwords interleaved group words; "slip" deletes one bit in the middle of those.  The
    decoy has two complements next to each other, inside one group, and sync bytes behind them; at G = 3 that is the legal pattern of an
    inverted stream (two of three bytes inverted), so there the decoy is L sync bytes with no complement at all, the other pattern no
    (s, g) gives.  -> (bits, the source words, the bit the first interleaved word begins at)"""
    x = group_words(rng, nwords, n, G, phase, sync, plain_body)
    y, _ = outer_interleave_ref(x[None], I)
    body = bytes_to_bits(y.reshape(-1), msb_first)
    parts = [rng.integers(0, 2, lead, dtype=np.uint8)]
    for k in kind.split("+"):
        if k == "decoy":
            d = rng.integers(0, 256, (L, n), dtype=np.uint8)
            d[(d == sync) | (d == sync ^ 0xFF)] = 0
            d[:, 0] = sync
            if G > 3:
                d[:2, 0] = sync ^ 0xFF
            parts += [bytes_to_bits(d.reshape(-1), msb_first), rng.integers(0, 2, DECOY_GAP, dtype=np.uint8)]
        elif k == "slip":
            body = np.delete(body, len(body) // 2)
        else:
            assert k == "clean"
    start = sum(len(p) for p in parts)
    b = np.concatenate(parts + [body])
    return (b ^ 1 if invert else b), x, start


# ------------------------------------------------------------------- what the GPU tests push
# As in test_outer_cpu.py: every input test_dvb_gpu.py feeds qpsk_outer_push under group sync is built here, so that the scalar port of the
# kernel (outer_port.py, test_outer_port_cpu.py) runs over literally the same bits.
STREAMS = (("clean", False, 5, 1), ("clean", True, 18, -1), ("decoy", False, 0, 2), ("slip", True, 43, 0), ("decoy+slip", False, 62, 3))
GPU_GROUPS = ((6, 3, 3, 3), (20, 1, 8, 9), (204, 12, 8, 8), (255, 5, 16, 16))      # n, I, G, L
GPU_FLAGS = (POLARITY, POLARITY | MSB_FIRST, 0, MSB_FIRST)
GPU_DROP = 2


def reference_of(s):
    """the restatement of the header for an input set: outer_ref, or outer_group_ref where the set has a group"""
    return outer_group_ref(**s["reset"])


def reference_outputs(s):
    """what the reference returns for every push of an input set"""
    ref, wants = reference_of(s), []
    for step in s["steps"]:
        if step[0] == "advance":
            ref.advance(step[1])
        else:
            wants.append(ref.push(step[1]))
    return wants


def group_streams(rng, n, I, G, L, msb_first):
    """five streams (not a multiple of a workgroup's four waves): kind, inverted or not, lead-in and group phase all differ; random bodies,
    false sync bytes and all.  -> bits (5, N)"""
    nwords = 3 * L + 2 * I + 3 * G
    made = [group_stream(rng, n, I, G, L, nwords, lead, phase % G, kind, inv, msb_first)[0] for kind, inv, lead, phase in STREAMS]
    N = min(len(b) for b in made)
    return np.stack([b[:N] for b in made])


def random_cuts(rng, N, step):
    """pushes of 1 bit seven times over (so that every bit phase total & 7 begins a push), then 7, 8191 and random lengths"""
    sizes = [1] * 7 + [7, 8191] + [int(v) for v in rng.integers(1, 4 * step, 64)]
    spans = cut(N, tuple(sizes))
    assert {a & 7 for a, _ in spans} == set(range(8)) or N < 8
    return spans


def group_sync_inputs(n, I, G, L, flags):
    rng = np.random.default_rng(n * 1000 + I * 100 + G * 10 + L + flags)
    bits = group_streams(rng, n, I, G, L, bool(flags & MSB_FIRST))
    return bits, random_cuts(rng, bits.shape[1], 8 * n)


# b. a look-ahead longer than two groups (p0 has bits from 2 G on), the longest look-ahead with the shortest group, and I = 32 under group sync
LONG_LOCKS = ((6, 3, 3, 7), (6, 2, 3, 16), (8, 4, 5, 16), (96, 32, 16, 16))      # n, I, G, L
LONG_FLAGS = (POLARITY, 0)


def long_lock_set(n, I, G, L, flags):
    bits, spans = group_sync_inputs(n, I, G, L, flags)

    def check(wants):
        groups = np.concatenate([f >> 4 for w in wants for f in w["flags"]])
        assert set(groups.tolist()) == set(range(G)), sorted(set(groups.tolist()))
        emitted = sum(w["count"].astype(np.int64) for w in wants)
        assert (emitted > 0).all() if flags & POLARITY else (emitted[0] > 0 and emitted[1] == 0 and emitted[3] == 0)
    return input_set("long look-ahead %s flags %d" % ((n, I, G, L), flags), n, I, L, GPU_DROP, bits, spans, flags=flags, group=G, check=check)


# d. the late decoy: L sync-like bytes whose first complement comes a whole group late -- complements at G, 2 G, ..., none at 0.  Every
# legal mask has its first set bit below G, so the pattern is no (s, g)'s; a hunt that compared it with p0 shifted by G would take it
LATE_DECOYS = ((6, 3, 3, 7), (6, 1, 3, 4), (20, 1, 8, 9), (6, 2, 8, 16))       # n, I, G, L
LATE_STREAMS = ((False, 0, 1), (True, 3, 0), (False, 13, 2), (True, 6, 1))      # inverted, lead-in of zero bits, group phase


def late_decoy_stream(rng, n, I, G, L, invert, lead, phase, sync=0x47):
    """-> (bits, the bit the stream behind the decoy begins at)"""
    d = rng.integers(0, 256, (L, n), dtype=np.uint8)
    d[(d == sync) | (d == sync ^ 0xFF)] = 0
    d[:, 0] = sync
    d[G::G, 0] = sync ^ 0xFF
    behind, _, start = group_stream(rng, n, I, G, L, L + I + G + 3, 0, phase, "clean", False, False, sync, plain_body=True)
    assert start == 0
    front = np.concatenate([np.zeros(lead, np.uint8), bytes_to_bits(d.reshape(-1)), rng.integers(0, 2, DECOY_GAP, dtype=np.uint8)])
    b = np.concatenate([front, behind])
    return (b ^ 1 if invert else b), len(front)


def late_decoy_set(n, I, G, L):
    rng = np.random.default_rng(n * 1000 + I * 100 + G * 10 + L + 7)
    made = [late_decoy_stream(rng, n, I, G, L, inv, lead, phase) for inv, lead, phase in LATE_STREAMS]
    N = min(len(b) for b, _ in made)
    bits = np.stack([b[:N] for b, _ in made])

    def check(wants):
        for i, (_, start) in enumerate(made):
            pos = np.concatenate([w["pos"][i] for w in wants])
            info = sum(w["info"][i, 2:].astype(np.int64) for w in wants)
            # one lock, never lost, on the first word behind the decoy: nothing was declared while the decoy passed
            assert tuple(info) == (1, 0) and len(pos) > 0 and pos[0] == start + 8 * n * (I - 1), (i, info, pos[:2], start)
            assert wants[-1]["info"][i, 1] == (-1 if LATE_STREAMS[i][0] else 1)
    return input_set("late decoy %s" % ((n, I, G, L),), n, I, L, GPU_DROP, bits, [(0, N // 3 + 5), (N // 3 + 5, N)], group=G, check=check)


def dvb_gpu_sets(new=True):
    """every link test_dvb_gpu.py pushes through the device under group sync (new=False: without the cases b and d above).  Its test of
    the old reset pushes test_outer_cpu's partition inputs, which outer_gpu_sets() holds"""
    sets = []
    if new:
        sets += [late_decoy_set(*case) for case in LATE_DECOYS]
        sets += [long_lock_set(*case, flags) for case in LONG_LOCKS for flags in LONG_FLAGS]
    for n, I, G, L in GPU_GROUPS:
        for flags in GPU_FLAGS:
            bits, spans = group_sync_inputs(n, I, G, L, flags)
            sets.append(input_set("group sync %s flags %d" % ((n, I, G, L), flags), n, I, L, GPU_DROP, bits, spans, flags=flags, group=G))
    p = DVB
    pushes = [unpack_bits(c["bits"], c["nbits"]) for c in dvb_link_result()["vcalls"] if c["nbits"]]
    sets.append(input_set("the DVB link", p["n"], p["I"], p["L"], p["drop"], steps=[("push", b, None) for b in pushes], flags=p["flags"], group=p["G"]))
    return sets


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_dvb_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in DVB_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    for word in ("GROUP SYNC", "DVB TRANSPORT", "QPSK_DISPERSAL_MSB_FIRST = 1", "03 F6 08 34 30", "a fused RS-decode + dispersal"):
        assert word in header, word
    assert callable(getattr(qpsk_amd.Modem, "dispersal", None)) and callable(qpsk_amd.dispersal_sequence)
    assert list(inspect.signature(qpsk_amd.Modem.outer_reset).parameters)[-2:] == ["msb_first", "group"]
    assert inspect.signature(qpsk_amd.Modem.outer_reset).parameters["group"].default == 0
    sig = inspect.signature(qpsk_amd.Modem.dispersal).parameters
    assert list(sig) == ["self", "rows", "group", "flags", "first", "msb_first", "pitch"]
    assert [sig[k].default for k in ("group", "flags", "first", "msb_first", "pitch")] == [8, None, 0, False, 0]
    sig = inspect.signature(qpsk_amd.dispersal_sequence).parameters
    assert [(k, v.default) for k, v in sig.items()] == [("len", 188), ("group", 8), ("msb_first", False)]
    makefile = open(os.path.join(ROOT, "qpsk_amd", "csrc", "Makefile")).read()
    assert "dispersal.o" in makefile and "api_dispersal.o" in makefile
    buf, out = (C.c_uint8 * 512)(), (C.c_uint8 * 512)()
    assert qpsk_lib.qpsk_outer_reset_group(None, 1, 204, 12, 0x47, 8, 3, POLARITY | MSB_FIRST, 8) == QPSK_ERR_ARG
    assert b"qpsk_outer_reset_group: null context" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_dispersal_batch(None, buf, 0, 2, 188, 8, 0, None, 0, out, 0) == QPSK_ERR_ARG
    assert b"qpsk_dispersal_batch: null context" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_dispersal_sequence(2, 1, 0, out) == 1      # host arithmetic: no context to refuse


def test_every_argument_error_of_the_new_calls_is_decided_before_a_device_is_touched(qpsk_lib):
    L = qpsk_lib

    def refused(rc, text):
        assert rc == QPSK_ERR_ARG and text in L.qpsk_last_error(), (rc, text, L.qpsk_last_error())
    good = dict(nstreams=1, n=6, branches=3, sync=0x47, lock=8, drop=3, flags=POLARITY | MSB_FIRST, group=8)
    names = ("nstreams", "n", "branches", "sync", "lock", "drop", "flags", "group")
    reset = lambda **k: L.qpsk_outer_reset_group(None, *[{**good, **k}[a] for a in names])
    refused(reset(), b"null context")
    for k, text in ((dict(group=1), b"group = 1 (0, or 3..16)"), (dict(group=2), b"group = 2 (0, or 3..16)"), (dict(group=17, lock=16), b"group = 17"),
                    (dict(group=-1), b"group = -1"), (dict(lock=7), b"lock = 7 below group = 8"), (dict(lock=2, group=3), b"lock = 2 below group = 3"),
                    (dict(group=16, lock=15), b"lock = 15 below group = 16"), (dict(lock=17, group=16), b"lock = 17 outside"),
                    (dict(nstreams=0), b"nstreams = 0"), (dict(n=1, branches=1), b"n = 1 outside"), (dict(branches=4), b"branches = 4"),
                    (dict(sync=256), b"sync = 256"), (dict(drop=17), b"drop = 17"), (dict(flags=4), b"unknown flags 0x4")):
        refused(reset(**k), text)
        assert b"qpsk_outer_reset_group" in L.qpsk_last_error()
    for G, lock in ((0, 1), (0, 16), (3, 3), (3, 16), (8, 8), (16, 16)):      # the corners pass; group 0 is the old reset with every lock
        refused(reset(group=G, lock=lock), b"null context")
    refused(L.qpsk_outer_reset(None, 1, 6, 3, 0x47, 2, 3, 4), b"qpsk_outer_reset: unknown flags 0x4")      # the old reset knows no new flag

    buf, out, fl = (C.c_uint8 * 4096)(), (C.c_uint8 * 4096)(), (C.c_uint8 * 64)()
    at = lambda b, off=0: C.c_void_p(C.addressof(b) + off)
    good = dict(i=at(buf), ip=0, nrows=4, len=188, group=8, flags=0, f=None, first=0, o=at(out), op=0)
    names = ("i", "ip", "nrows", "len", "group", "flags", "f", "first", "o", "op")
    disp = lambda **k: L.qpsk_dispersal_batch(None, *[{**good, **k}[a] for a in names])
    refused(disp(), b"null context")
    for k, text in ((dict(i=None), b"null d_in or d_out"), (dict(o=None), b"null d_in or d_out"), (dict(len=1), b"len = 1 outside 2..255"),
                    (dict(len=256), b"len = 256 outside"), (dict(group=0), b"group = 0 outside 1..16"), (dict(group=17), b"group = 17 outside"),
                    (dict(flags=2), b"unknown flags 0x2"), (dict(nrows=0), b"nrows = 0"), (dict(ip=187), b"in_pitch = 187"),
                    (dict(op=187), b"out_pitch = 187"), (dict(ip=-1), b"in_pitch = -1"), (dict(first=8), b"first = 8 outside 0..group - 1"),
                    (dict(first=-1), b"first = -1 outside"), (dict(f=at(fl), first=1), b"first = 1 with d_flags"),
                    (dict(o=at(buf, 1)), b"d_out overlaps d_in"), (dict(o=at(buf, 751)), b"d_out overlaps d_in"),
                    (dict(o=at(buf), op=204), b"d_out overlaps d_in"),      # the same first byte, another pitch: not in place
                    (dict(f=at(buf, 700)), b"d_flags overlaps d_in"), (dict(f=at(out, 751)), b"d_flags overlaps d_out"),
                    (dict(i=at(buf, 100), ip=204, f=at(buf, 96 + 3 * 204 + 188)), b"d_flags overlaps d_in")):
        refused(disp(**k), text)
        assert b"qpsk_dispersal_batch" in L.qpsk_last_error()
    for k in (dict(o=at(buf)), dict(o=at(buf), ip=204, op=204), dict(o=at(buf, 752)), dict(f=at(buf, 752)), dict(f=at(fl)), dict(first=7),
              dict(len=2, group=1), dict(len=255, group=16, nrows=1), dict(ip=204, op=207), dict(flags=DISPERSAL_MSB_FIRST)):
        refused(disp(**k), b"null context")                   # in place, abutting buffers and the corners of the ranges
    # the boundary of every overlap test, a byte on either side: 3 rows of 188 at pitch 204 end at byte 2 * 204 + 188 = 596, padding apart
    pad = dict(nrows=3, ip=204, op=204)
    for k, text in ((dict(pad, o=at(buf, 595)), b"d_out overlaps d_in"), (dict(pad, i=at(buf, 595), o=at(buf)), b"d_out overlaps d_in"),
                    (dict(pad, f=at(buf, 595)), b"d_flags overlaps d_in"), (dict(pad, i=at(buf, 2), f=at(buf)), b"d_flags overlaps d_in"),
                    (dict(pad, f=at(out, 595)), b"d_flags overlaps d_out"), (dict(pad, o=at(out, 2), f=at(out)), b"d_flags overlaps d_out"),
                    (dict(i=at(buf, 751), o=at(buf)), b"d_out overlaps d_in"), (dict(o=at(buf), ip=204), b"d_out overlaps d_in")):
        refused(disp(**k), text)                              # one shared byte, the last of one range on the first of the other
    for k in (dict(pad, o=at(buf, 596)), dict(pad, i=at(buf, 596), o=at(buf)), dict(pad, f=at(buf, 596)), dict(pad, i=at(buf, 3), f=at(buf)),
              dict(pad, f=at(out, 596)), dict(pad, o=at(out, 3), f=at(out)), dict(i=at(buf, 752), o=at(buf)), dict(pad, o=at(buf))):
        refused(disp(**k), b"null context")                   # touching: the padding behind the last row is not the buffer; in place at pitch 204
    for (n, G, flags), text in (((1, 8, 0), b"len = 1 outside"), ((256, 8, 0), b"len = 256"), ((188, 0, 0), b"group = 0"), ((188, 17, 0), b"group = 17"),
                                ((188, 8, 2), b"unknown flags 0x2")):
        refused(L.qpsk_dispersal_sequence(n, G, flags, out), text)
        assert b"qpsk_dispersal_sequence" in L.qpsk_last_error()
    refused(L.qpsk_dispersal_sequence(188, 8, 0, None), b"null out")


# ------------------------------------------------------------------- 2. the dispersal sequence
def test_the_sequence_is_the_standard_s_and_the_oracle_s_keystream_repacked(qpsk_lib, oracle):
    import qpsk_amd
    seq = qpsk_amd.dispersal_sequence(188, 8, msb_first=True)
    assert isinstance(seq, bytes) and len(seq) == 1503 and seq[:8] == STANDARD
    assert qpsk_amd.dispersal_sequence() == qpsk_amd.dispersal_sequence(188, 8, False) and len(qpsk_amd.dispersal_sequence()) == 1503
    # the oracle's scramble() on zero symbols from SEED: dibit d = K[2 d] | K[2 d + 1] << 1
    d = oracle.scramble_stream(np.zeros(4 * (16 * 255 - 1), np.uint8))
    K = np.stack([d & 1, d >> 1], axis=1).reshape(-1)
    for n, G in ((188, 8), (2, 1), (255, 16), (7, 3)):
        for msb in (False, True):
            want = np.packbits(K[:8 * (G * n - 1)].reshape(-1, 8), axis=1, bitorder="big" if msb else "little")[:, 0]
            got = np.frombuffer(qpsk_amd.dispersal_sequence(n, G, msb), np.uint8)
            assert np.array_equal(got, want), (n, G, msb)
            assert np.array_equal(dispersal_sequence_ref(n, G, msb), want), (n, G, msb)      # and the restatement of the standard's drawing
    with pytest.raises(qpsk_amd.QpskError):
        qpsk_amd.dispersal_sequence(1, 8)


def test_dispersal_ref_is_an_involution_that_inverts_one_sync_byte_in_a_group_and_leaves_the_others():
    rng = np.random.default_rng(188)
    for n, G, msb in ((188, 8, True), (2, 1, False), (255, 16, False), (5, 3, True)):
        x = rng.integers(0, 256, (3 * G + 2, n), dtype=np.uint8)
        idx = (np.arange(len(x)) + 2) % G
        y = dispersal_ref(x, G, idx, msb)
        assert np.array_equal(dispersal_ref(y, G, idx, msb), x)
        assert np.array_equal(y[:, 0], x[:, 0] ^ np.where(idx == 0, 0xFF, 0))
        pr = dispersal_sequence_ref(n, G, msb)
        k = int(idx[1])
        assert np.array_equal(y[1, 1:] ^ x[1, 1:], pr[k * n:k * n + n - 1])
        idx[0] = G                                            # an index outside the group: the row is copied
        assert np.array_equal(dispersal_ref(x, G, idx, msb)[0], x[0])


# ------------------------------------------------------------------- 3. group sync on the restatement
def test_a_look_ahead_over_one_group_determines_polarity_and_phase_and_a_shorter_one_or_a_group_of_two_does_not():
    for G in range(3, 17):
        for L in range(G, 17):
            assert legal_masks(G, L)[1], (G, L)
        for L in range(1, G - 1):
            assert not legal_masks(G, L)[1], (G, L)
        # L = G - 1 still tells the (s, g) apart, but one of them by a window that holds no complement at all -- what a stream without
        # groups looks like; the header asks for a whole group
        assert 0 in legal_masks(G, G - 1)[0] and 0 not in legal_masks(G, G)[0]
    for L in range(2, 17):
        assert not legal_masks(2, L)[1], L


@pytest.mark.parametrize("n,I,L,drop,kind", CASES)
def test_group_zero_is_outer_ref_on_its_own_cases(n, I, L, drop, kind):
    rng = np.random.default_rng(n * 1000 + I * 100 + L * 10 + drop)
    streams = [damaged_stream(rng, n, I, 60, int(rng.integers(0, 71)), kind)[0] for _ in range(4)]
    N = min(len(b) for b in streams)
    bits = np.stack([b[:N] for b in streams])
    for flags in (POLARITY, 0):
        spans = cut(N, split_sizes(n))
        want = run_outer(outer_ref(4, n, I, 0x47, L, drop, flags), bits, spans)
        got = run_outer(outer_group_ref(4, n, I, 0x47, L, drop, flags, group=0), bits, spans)
        for a, b in zip(want[0], got[0]):
            assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["info"], b["info"])
        for k in (1, 2, 3):
            for i in range(4):
                assert np.array_equal(want[k][i], got[k][i])
        assert all((f < 4).all() for f in got[3])             # bits 4..7 stay zero


GROUP_CASES = [(6, 3, 3, 3, 2), (4, 2, 4, 5, 1), (20, 1, 8, 9, 3), (12, 4, 16, 16, 2)]      # n, I, G, L, drop


def group_case(n, I, G, L, flags=POLARITY, seed=0):
    """four streams of one case: clean, inverted, decoy in front, a slip in the middle -- each with its own lead-in and group phase"""
    rng = np.random.default_rng(n * 1000 + I * 100 + G * 10 + L + seed)
    nwords = 3 * L + 2 * I + 3 * G
    msb = bool(flags & MSB_FIRST)
    made = [group_stream(rng, n, I, G, L, nwords, 5, 1, "clean", False, msb, plain_body=True),
            group_stream(rng, n, I, G, L, nwords, 18, G - 1, "clean", True, msb, plain_body=True),
            group_stream(rng, n, I, G, L, nwords, 0, 2, "decoy", False, msb, plain_body=True),
            group_stream(rng, n, I, G, L, nwords, 43, 0, "slip", True, msb, plain_body=True)]
    N = min(len(b) for b, _, _ in made)
    return np.stack([b[:N] for b, _, _ in made]), made


@pytest.mark.parametrize("n,I,G,L,drop", GROUP_CASES)
@pytest.mark.parametrize("flags", [POLARITY, POLARITY | MSB_FIRST])
def test_group_sync_locks_where_it_must_whatever_the_cuts_and_the_word_bound_holds(n, I, G, L, drop, flags):
    bits, made = group_case(n, I, G, L, flags)
    S, N = bits.shape
    step = 8 * n
    one_calls, one_w, one_p, one_f = run_outer(outer_group_ref(S, n, I, 0x47, L, drop, flags, G), bits, [(0, N)])
    for sizes in ((1,), split_sizes(n), (1000,)):
        spans = cut(N, sizes)
        calls, w, p, f = run_outer(outer_group_ref(S, n, I, 0x47, L, drop, flags, G), bits, spans)
        for (a, b), c in zip(spans, calls):
            assert (c["count"] <= word_bound(L, n, b - a)).all(), (a, b, c["count"])
        for i in range(S):
            assert np.array_equal(w[i], one_w[i]) and np.array_equal(p[i], one_p[i]) and np.array_equal(f[i], one_f[i])
    info = one_calls[0]["info"]
    for i, (b, x, start) in enumerate(made):
        phase = (1, G - 1, 2, 0)[i]
        # the first lock falls on the first interleaved word -- behind a decoy too --, with the stream's sign and that word's group index
        assert one_p[i][0] == start + step * (I - 1), (i, one_p[i][:2], start)
        assert bool(one_f[i][0] & 2) == (i in (1, 3))
        w0 = (one_p[i] - start) // step - (I - 1)             # the source word an emitted word is
        if i != 3:
            assert np.array_equal(one_w[i], x[w0]) and not (one_f[i] & 1).any()
            assert np.array_equal(one_f[i] >> 4, (w0 + phase) % G)
            assert np.array_equal(one_w[i][:, 0], np.where((w0 + phase) % G == 0, 0xB8, 0x47))      # bytes as received: 0xB8 stays 0xB8
            assert tuple(info[i]) == (1, -1 if i == 1 else 1, 1, 0)
    # the decoy's L first bytes do all match: only their signs tell it from a lock
    ref = outer_group_ref(1, n, I, 0x47, L, drop, flags, G)
    ref.push(bits[2:3])
    m = ref._m2(ref.streams[0].V[step * np.arange(L)])
    assert (m != 0).all() and ref.lut_s[int(((m < 0) << np.arange(L)).sum())] == 0
    # the slip: the lock is lost and found again one bit earlier, with the group index of the word it falls on
    assert info[3, 2] == 2 and info[3, 3] == 1
    grid = made[3][2] - 1                                     # where the words begin behind the deleted bit
    late = (one_p[3] > grid + len(bits[3]) // 2) & ((one_p[3] - grid) % step == 0)      # the words of the second lock
    w1 = (one_p[3][late] - grid) // step - (I - 1)
    assert late.sum() >= 3
    assert np.array_equal(one_f[3][late] >> 4, w1 % G) and np.array_equal(one_w[3][late], made[3][1][w1])


def test_without_polarity_an_inverted_stream_never_locks():
    n, I, G, L, drop = 6, 3, 3, 3, 2
    bits, _ = group_case(n, I, G, L)
    for flags, want in ((0, (1, 0, 1, 0)), (POLARITY, (1, 1, 1, 1))):
        calls, w, p, f = run_outer(outer_group_ref(4, n, I, 0x47, L, drop, flags, G), bits, [(0, bits.shape[1])])
        assert tuple(int(len(x) > 0) for x in w) == want
        if not flags:
            assert not calls[0]["info"][1].any() and not calls[0]["info"][3].any()


# ------------------------------------------------------------------- 4. the link at DVB-S's own parameters, on the restatements alone
# 3 streams of 40 transport packets (0x47 + 187 random bytes) -> dispersal (every stream starts its group somewhere else) -> RS (204, 188) ->
# interleaver I = 12 -> bytes sent high bit first -> rate 3/4 at +-64.  Stream 1 gets a half turn; stream 2 a run of RUN inverted dibits,
# the burst of DESIGN.md 4.4.14 -- at rate 3/4 a run of 400 dibits is 600 data bits, 75 bytes in a row, 7 to a word behind 12 branches, which
# is inside the radius of 8: measured on these restatements, RUN = 400 decodes clean at I = 12 (test below), so it is not shortened.
DVB = dict(n=204, k=188, I=12, G=8, L=8, drop=3, S=3, npackets=40, first=(0, 3, 5), run=400, at=20000, depth=128, window=256, seed=300421,
           pattern=NAMED["3/4"], flags=POLARITY | MSB_FIRST, cuts=(0, 8192, 12290, 30000))
_DVB = {}


def dvb_link_result():
    """computed once, shared with test_dvb_gpu.py: every stage's output"""
    if _DVB:
        return _DVB
    p = DVB
    S, n, k, G = p["S"], p["n"], p["k"], p["G"]
    rng = np.random.default_rng(p["seed"])
    packets = rng.integers(0, 256, (S, p["npackets"], k), dtype=np.uint8)
    packets[:, :, 0] = 0x47
    index = (np.array(p["first"])[:, None] + np.arange(p["npackets"])) % G
    randomised = np.stack([dispersal_ref(packets[i], G, index[i], True) for i in range(S)])
    sent = rs_encode_ref(randomised.reshape(-1, k), n - k).reshape(S, -1, n)
    y, _ = outer_interleave_ref(sent, p["I"])
    tx_bits = bytes_to_bits(y.reshape(S, -1), True)
    nbits = tx_bits.shape[1]
    dibits, _ = conv_encode_stream_ref(pack_bits(tx_bits), nbits, p["pattern"])
    soft = dibits_to_soft(dibits).astype(np.int16)
    soft[1] *= -1                                             # the half turn
    soft[2, p["at"]:p["at"] + p["run"]] *= -1                 # the burst
    soft = soft.astype(np.int8)
    dec = viterbi_stream_ref(S, p["depth"], p["window"], p["pattern"])
    cuts = list(p["cuts"]) + [dibits.shape[1]]
    vcalls = [dec.push(soft[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    vcalls.append(dec.flush())
    ref = outer_group_ref(S, n, p["I"], 0x47, p["L"], p["drop"], p["flags"], G)
    ocalls = [ref.push(unpack_bits(c["bits"], c["nbits"])) for c in vcalls if c["nbits"]]
    words = [np.concatenate([c["words"][i] for c in ocalls]) for i in range(S)]
    flags = [np.concatenate([c["flags"][i] for c in ocalls]) for i in range(S)]
    pos = [np.concatenate([c["pos"][i] for c in ocalls]) for i in range(S)]
    decoded = [rs_decode_ref(w, n - k) for w in words]
    out = [dispersal_ref(d[:, :k], G, f >> 4, True) for (d, _), f in zip(decoded, flags)]
    _DVB.update(packets=packets, index=index, randomised=randomised, sent=sent, interleaved=y, tx_bits=tx_bits, dibits=dibits, soft=soft,
                cuts=cuts, vcalls=vcalls, ocalls=ocalls, words=words, flags=flags, pos=pos, decoded=[d for d, _ in decoded],
                info=[i for _, i in decoded], out=out)
    return _DVB


def test_the_dvb_link_returns_the_transport_packets_with_0x47_in_front():
    r, p = dvb_link_result(), DVB
    step = 8 * p["n"]
    for i in range(p["S"]):
        assert (r["info"][i][:, 0] >= 0).all(), ("stream", i, "a word failed its decode")      # clean at I = 12, the burst of 400 included
        # which packets came out: the lock falls on a word boundary of the sent stream, at or behind word 0
        assert len(r["pos"][i]) and (r["pos"][i][0] % step == 0) and (np.diff(r["pos"][i]) == step).all()
        w0 = int(r["pos"][i][0]) // step - (p["I"] - 1)
        count = len(r["out"][i])
        assert count >= p["npackets"] - (p["I"] - 1) - 2 and w0 + count == p["npackets"] - (p["I"] - 1)
        assert np.array_equal(r["out"][i], r["packets"][i, w0:w0 + count]) and (r["out"][i][:, 0] == 0x47).all()
        assert np.array_equal(r["flags"][i] >> 4, r["index"][i, w0:w0 + count]) and not (r["flags"][i] & 1).any()
        assert (r["flags"][i] & 2).all() == (i == 1) and (r["flags"][i] & 2).any() == (i == 1)      # s = -1 on the turned stream only
        assert sum(c["info"][i, 3] for c in r["ocalls"]) == 0 and sum(c["info"][i, 2] for c in r["ocalls"]) == 1
    assert (r["info"][2][:, 0] > 0).sum() >= p["I"]           # the burst did land: behind 12 branches it reaches at least 12 words
    assert r["info"][2][:, 0].max() <= 8
