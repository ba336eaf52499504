"""qpsk_outer_* on the GPU: every output of every call bit for bit against test_outer_cpu.outer_ref / outer_interleave_ref (OUTER LINK of
include/qpsk_hip.h restated in numpy).  Poison (0x55) sits behind every output and between the words where word_pitch > n, and behind every
input row's bits; the bits of a row's last byte beyond nbits are set, so that a kernel that reads them shows.  Every stream of every case has
its own random content and its own lead-in, so that u0 & 7 takes all eight values; at n = 4 random data is full of false sync bytes, which
is the point.  The shapes are the smallest that reach each branch.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_dvb_cpu import reference_of
from test_outer_cpu import (EDGES, GPU_FLAGS, GPU_GEOMETRIES, GPU_LOCKS, GPU_PARTITIONS, GPU_SLIPS, LIMITS, LINK, MSB_FIRST, POLARITY,
                            big16_inputs, big20_inputs, cut, edge_sets, geometry_inputs, layout_inputs, limit_set, link_result, no_slots_set,
                            noise_set, outer_interleave_ref, outer_ref, partition_inputs, polarity_inputs, positions_inputs, refusal_inputs,
                            replaced_link_inputs, slip_inputs, split_sizes, word_bound)
from test_viterbi_cpu import pack_bits
from test_viterbi_gpu import modem, ptr

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
GUARD = 64
ALL = ("words", "pos", "flags", "info")


def device_bits(bits, pitch=0):
    """bits (S, nbits) of 0 / 1 -> (a device tensor of rows `pitch` bytes apart, pitch): poison behind each row, ones behind its last bit"""
    import torch
    S, nbits = bits.shape
    nb = (nbits + 7) // 8
    pitch = pitch or nb
    rows = np.full((S, pitch), 0x55, np.uint8)
    rows[:, :nb] = pack_bits(np.concatenate([bits, np.ones((S, 8 * nb - nbits), np.uint8)], axis=1))
    return torch.from_numpy(rows).cuda(), pitch


def push(m, S, n, bits, want=ALL, max_words=None, word_pitch=0, bits_pitch=0, nbits=None):
    """a raw qpsk_outer_push with guarded outputs.  bits: numpy (S, nbits) of 0 / 1, or a device tensor of packed rows (then nbits is given)"""
    import torch
    if hasattr(bits, "data_ptr"):
        d_bits, bp = bits, bits.shape[1]
    else:
        nbits = bits.shape[1]
        d_bits, bp = device_bits(bits, bits_pitch)
    mw = m.outer_max_words(nbits) if max_words is None else max_words
    wp = word_pitch or n
    count = torch.full((S + GUARD,), 0x55555555, dtype=torch.int32, device="cuda")
    words = torch.full((S * mw * wp + GUARD,), 0x55, dtype=torch.uint8, device="cuda") if "words" in want else None
    pos = torch.full((S * mw + GUARD,), 0x5555555555555555, dtype=torch.int64, device="cuda") if "pos" in want else None
    flags = torch.full((S * mw + GUARD,), 0x55, dtype=torch.uint8, device="cuda") if "flags" in want else None
    info = torch.full((S * 4 + GUARD,), 0x55555555, dtype=torch.int32, device="cuda") if "info" in want else None
    m._check(m.L.qpsk_outer_push(m.h, ptr(d_bits), bp if (bits_pitch or hasattr(bits, "data_ptr")) else 0, nbits, mw, ptr(count), ptr(words),
                                 word_pitch, ptr(pos), ptr(flags), ptr(info)))
    assert m.last_kernel() == "outer_push_kernel"
    torch.cuda.synchronize()
    h = count.cpu().numpy()
    assert (h[S:] == 0x55555555).all(), "guard behind d_count overwritten"
    out = dict(count=h[:S].copy(), max_words=mw, d_words=words, word_pitch=wp)
    kept = np.minimum(out["count"], mw)
    written = np.arange(mw)[None, :] < kept[:, None]          # (S, mw): the entries the call may write
    if words is not None:
        h = words.cpu().numpy()
        w = h[:S * mw * wp].reshape(S, mw, wp)
        mask = np.zeros((S, mw, wp), bool)
        mask[:, :, :n] = written[:, :, None]
        assert (h[S * mw * wp:] == 0x55).all() and (w[~mask] == 0x55).all(), "bytes outside the emitted words were written"
        out["words"] = [w[i, :kept[i], :n] for i in range(S)]
    for key, buf, poison in (("pos", pos, 0x5555555555555555), ("flags", flags, 0x55)):
        if buf is not None:
            h = buf.cpu().numpy()
            v = h[:S * mw].reshape(S, mw)
            assert (h[S * mw:] == poison).all() and (v[~written] == poison).all(), "entries of d_%s outside the emitted words were written" % key
            out[key] = [v[i, :kept[i]] for i in range(S)]
    if info is not None:
        h = info.cpu().numpy()
        assert (h[S * 4:] == 0x55555555).all(), "guard behind d_info overwritten"
        out["info"] = h[:S * 4].reshape(S, 4)
    return out


def same(got, want, what=""):
    """a device call against the restatement's: the true count, and the first min(count, max_words) entries of every output it has"""
    assert np.array_equal(got["count"], want["count"]), (what, "count", got["count"], want["count"])
    for i in range(len(want["count"])):
        k = min(int(want["count"][i]), got["max_words"])
        for key in ("words", "pos", "flags"):
            if key in got:
                assert np.array_equal(got[key][i], want[key][i][:k]), (what, key, "stream", i, got[key][i], want[key][i][:k])
    if "info" in got:
        assert np.array_equal(got["info"], want["info"]), (what, "info", got["info"], want["info"])


def run_both(m, ref, n, bits, spans, what="", **kw):
    """push bits (S, N) in the given spans through the device and the restatement, every call compared -> the device's calls"""
    calls = []
    for a, b in spans:
        got = push(m, bits.shape[0], n, bits[:, a:b], **kw)
        same(got, ref.push(bits[:, a:b]), (what, a, b))
        calls.append(got)
    return calls


def run_set(m, s, **kw):
    """one input set of test_outer_cpu / test_dvb_cpu -- the sets the scalar port of the kernel is held to in test_outer_port_cpu.py --
    through the device and the restatement, every call compared; what the set asserts on the reference alone is asserted here too
    -> the device's calls"""
    r = s["reset"]
    m.outer_reset(r["nstreams"], r["n"], r["branches"], r["sync"], r["lock"], r["drop"], polarity=bool(r["flags"] & POLARITY),
                  msb_first=bool(r["flags"] & MSB_FIRST), group=r["group"])
    ref, calls, wants = reference_of(s), [], []
    for step in s["steps"]:
        if step[0] == "advance":
            m.outer_advance(step[1])
            ref.advance(step[1])
            continue
        got = push(m, r["nstreams"], r["n"], step[1], max_words=step[2], **kw)
        wants.append(ref.push(step[1]))
        same(got, wants[-1], (s["what"], "push", len(calls)))
        calls.append(got)
    if s["check"]:
        s["check"](wants)
    return calls


# ------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("n,I", GPU_GEOMETRIES)
@pytest.mark.parametrize("L,drop", GPU_LOCKS)
def test_every_geometry_locks_at_every_bit_phase_and_emits_the_reference_s_words(n, I, L, drop):
    bits, spans = geometry_inputs(n, I, L, drop)
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop)
    assert m.last_kernel() == "outer_init_kernel"
    assert m.outer_max_words(N) == word_bound(L, n, N)
    calls = run_both(m, outer_ref(S, n, I, 0x47, L, drop), n, bits, spans)
    assert sum(int(c["count"].sum()) for c in calls) >= S
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. polarity and bit order
@pytest.mark.parametrize("flags", GPU_FLAGS)
def test_inverted_streams_lock_with_s_minus_one_only_with_polarity_and_msb_first_reverses_the_bytes(flags):
    n, I, L, drop = 6, 3, 2, 2
    bits, x, spans = polarity_inputs(flags)                   # every other stream inverted
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop, polarity=bool(flags & POLARITY), msb_first=bool(flags & MSB_FIRST))
    ref = outer_ref(S, n, I, 0x47, L, drop, flags)
    calls = run_both(m, ref, n, bits, spans)
    last = calls[-1]
    assert (last["info"][0::2, 1] == 1).all()
    if flags & POLARITY:
        assert (last["info"][1::2, 1] == -1).all() and all((f & 2).all() for f in last["flags"][1::2])
        for i in range(S):                                    # bytes right, inverted or not: the last words are the source's
            assert any(np.array_equal(last["words"][i][-3:], x[i][k:k + 3]) for k in range(len(x[i]) - 2))
    else:
        assert (last["info"][1::2, 0] == 0).all() and all(len(w) == 0 for w in last["words"][1::2])
    m.close()


# ------------------------------------------------------------------------------------------ 3. slips
@pytest.mark.parametrize("across", [False, True])
@pytest.mark.parametrize("n,I", GPU_SLIPS)
def test_a_deleted_bit_an_inserted_bit_and_an_inversion_drop_the_lock_and_relock(n, I, across):
    bits, spans = slip_inputs(n, I, across)      # the slips near N / 2, the inversion at 2 N / 3: inside one push, or a push boundary on each
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, n, I, 0x47, 2, 2)
    ref = outer_ref(S, n, I, 0x47, 2, 2)
    calls = run_both(m, ref, n, bits, spans)
    info = sum(c["info"][:, 2:].astype(np.int64) for c in calls)
    assert (info[:, 0] >= 2).all() and (info[:, 1] >= 1).all()      # every stream lost its lock and found another
    assert any((f & 2).any() for f in calls[-1]["flags"])     # and locked with the other s behind the inversion
    m.close()


# ------------------------------------------------------------------------------------------ 4. partition independence
@pytest.mark.parametrize("n,I,L,drop", GPU_PARTITIONS)
def test_the_same_bits_in_one_push_and_in_the_repeating_split(n, I, L, drop):
    bits = partition_inputs(n, I)
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop)
    parts = run_both(m, outer_ref(S, n, I, 0x47, L, drop), n, bits, cut(N, split_sizes(n)))
    m.outer_reset(S, n, I, 0x47, L, drop)                     # over an armed link: as new
    one = run_both(m, outer_ref(S, n, I, 0x47, L, drop), n, bits, [(0, N)])[0]
    for i in range(S):
        for key in ("words", "pos", "flags"):
            assert np.array_equal(np.concatenate([c[key][i] for c in parts]), one[key][i]), (key, i)
    assert np.array_equal(sum(c["count"] for c in parts), one["count"]) and one["count"].min() > 0
    m.close()


# ------------------------------------------------------------------------------------------ 5. large pushes
def test_a_push_of_65536_bits_into_three_slots_counts_every_word_and_the_state_goes_on():
    n, I, L, drop = 4, 2, 2, 2
    bits = big16_inputs()
    S = bits.shape[0]
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop)
    ref = outer_ref(S, n, I, 0x47, L, drop)
    big = push(m, S, n, bits[:, :1 << 16], max_words=3)
    want = ref.push(bits[:, :1 << 16])
    same(big, want, "2^16 bits")
    assert (big["count"] > 1500).all() and all(len(w) == 3 for w in big["words"])
    nxt = push(m, S, n, bits[:, 1 << 16:])
    same(nxt, ref.push(bits[:, 1 << 16:]), "the push behind it")
    assert (nxt["count"] > 0).all()
    m.close()


def test_one_push_of_2_to_the_20_bits_at_204_12():
    n, I = 204, 12
    bits = big20_inputs()
    m = modem()
    m.outer_reset(2, n, I)
    got = push(m, 2, n, bits)
    same(got, outer_ref(2, n, I).push(bits), "2^20 bits")
    assert got["count"][0] == ((1 << 20) - 5) // 1632 - (I - 1) and got["max_words"] == 2 + 643
    m.close()


# ------------------------------------------------------------------------------------------ 6. layout
def test_pitched_rows_pitched_words_and_each_optional_output_null_in_turn():
    n, I, L, drop = 6, 3, 2, 2
    bits, spans = layout_inputs()
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop)
    ref = outer_ref(S, n, I, 0x47, L, drop)
    wants = [ALL, ("pos", "flags", "info"), ("words", "flags", "info"), ("words", "pos", "info"), ("words", "pos", "flags"), ()]
    for k, (a, b) in enumerate(spans):
        got = push(m, S, n, bits[:, a:b], want=wants[k % len(wants)], word_pitch=(0, 11, n)[k % 3], bits_pitch=(b - a + 7) // 8 + (0, 3, 17)[k % 3])
        same(got, ref.push(bits[:, a:b]), ("layout", k))
    m.close()


# ------------------------------------------------------------------------------------------ 7. positions
@pytest.mark.parametrize("delta", [1 << 31, 1 << 40])
def test_positions_past_32_bits_are_exact(delta):
    n, I, L, drop = 6, 3, 2, 2
    bits = positions_inputs()
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop)
    ref = outer_ref(S, n, I, 0x47, L, drop)
    first = run_both(m, ref, n, bits, [(0, N // 4)])[0]
    assert (first["info"][:, 0] == 1).all()                   # locked
    assert m.L.qpsk_test_outer_advance(m.h, 12) == QPSK_ERR_ARG and m.L.qpsk_test_outer_advance(m.h, -8) == QPSK_ERR_ARG
    m.outer_advance(delta)
    ref.advance(delta)
    calls = run_both(m, ref, n, bits, [(N // 4, N // 2 + 9), (N // 2 + 9, N)])
    assert all(p.min() > delta for c in calls for p in c["pos"] if len(p))
    assert sum(int(c["info"][:, 3].sum()) for c in calls) >= S      # the slips came behind the advance
    m.close()


# ------------------------------------------------------------------------------------------ 8. state and refusals
def test_refused_calls_launch_nothing_and_leave_the_state_untouched():
    import torch
    n, I, L, drop = 6, 3, 2, 2
    bits = refusal_inputs()
    S, N = bits.shape
    m = modem()
    d_bits, bp = device_bits(bits[:, :400])
    cnt = torch.zeros(S + 2, dtype=torch.int32, device="cuda")
    buf = torch.zeros(S * 64 * 8 + 64, dtype=torch.uint8, device="cuda")
    raw = lambda **k: m.L.qpsk_outer_push(m.h, k.get("bits", ptr(d_bits)), k.get("bp", 0), k.get("nbits", 400), k.get("mw", 4), k.get("count", ptr(cnt)),
                                          k.get("words"), k.get("wp", 0), k.get("pos"), k.get("flags"), k.get("info"))
    # before a reset
    assert raw() == QPSK_ERR_STATE
    assert m.L.qpsk_outer_max_words(m.h, 64) == QPSK_ERR_STATE and m.L.qpsk_test_outer_advance(m.h, 8) == QPSK_ERR_STATE
    # every QPSK_ERR_ARG of the reset; none of them arms a link
    for bad in ((0, n, I, 0x47, L, drop, 0), (S, 1, 1, 0x47, L, drop, 0), (S, 256, 1, 0x47, L, drop, 0), (S, n, 0, 0x47, L, drop, 0),
                (S, n, 4, 0x47, L, drop, 0), (S, 66, 33, 0x47, L, drop, 0), (S, n, I, -1, L, drop, 0), (S, n, I, 256, L, drop, 0),
                (S, n, I, 0x47, 0, drop, 0), (S, n, I, 0x47, 17, drop, 0), (S, n, I, 0x47, L, -1, 0), (S, n, I, 0x47, L, 17, 0),
                (S, n, I, 0x47, L, drop, 4)):
        assert m.L.qpsk_outer_reset(m.h, *bad) == QPSK_ERR_ARG, bad
    assert raw() == QPSK_ERR_STATE
    m.outer_reset(S, n, I, 0x47, L, drop)
    ref = outer_ref(S, n, I, 0x47, L, drop)
    run_both(m, ref, n, bits, [(0, 400)])
    # a refused reset leaves the armed link as it was
    assert m.L.qpsk_outer_reset(m.h, S, n, 4, 0x47, L, drop, POLARITY) == QPSK_ERR_ARG
    for nbits in (0, -1, (1 << 20) + 1):
        assert m.L.qpsk_outer_max_words(m.h, nbits) == QPSK_ERR_ARG
    assert m.outer_max_words(1 << 20) == L + -(-(1 << 20) // (8 * n))
    # refused pushes
    for k in (dict(nbits=0), dict(nbits=(1 << 20) + 1), dict(bp=49), dict(mw=-1), dict(words=ptr(buf), wp=n - 1), dict(bits=None), dict(count=None),
              dict(info=C.c_void_p(buf.data_ptr() + 2)), dict(pos=C.c_void_p(buf.data_ptr() + 4)), dict(count=C.c_void_p(cnt.data_ptr() + 1)),
              dict(words=ptr(d_bits)), dict(words=ptr(buf), flags=C.c_void_p(buf.data_ptr() + 8)), dict(info=ptr(cnt)),
              dict(pos=ptr(buf), words=C.c_void_p(buf.data_ptr() + 64))):
        assert raw(**k) == QPSK_ERR_ARG, k
        assert b"qpsk_outer_push" in m.L.qpsk_last_error()
    run_both(m, ref, n, bits, [(400, 901), (901, N)], "behind the refused calls")
    # the interleaver's refusals
    w = torch.zeros(2 * 5 * 6 + 64, dtype=torch.uint8, device="cuda")
    o = torch.zeros(2 * 5 * 6 + 64, dtype=torch.uint8, device="cuda")
    h = torch.zeros(2 * 2 * 6 + 64, dtype=torch.uint8, device="cuda")
    il = lambda *a: m.L.qpsk_outer_interleave_batch(m.h, *a)
    assert il(ptr(w), 2, 5, 6, 3, None, None, ptr(o)) == 0
    for a in ((None, 2, 5, 6, 3, None, None, ptr(o)), (ptr(w), 2, 5, 6, 3, None, None, None), (ptr(w), 0, 5, 6, 3, None, None, ptr(o)),
              (ptr(w), 2, 0, 6, 3, None, None, ptr(o)), (ptr(w), 2, 5, 1, 1, None, None, ptr(o)), (ptr(w), 2, 5, 256, 1, None, None, ptr(o)),
              (ptr(w), 2, 5, 6, 0, None, None, ptr(o)), (ptr(w), 2, 5, 6, 4, None, None, ptr(o)), (ptr(w), 2, 5, 66, 33, None, None, ptr(o)),
              (ptr(w), 2, 5, 6, 3, None, None, ptr(w)), (ptr(w), 2, 5, 6, 3, None, None, C.c_void_p(w.data_ptr() + 59)),
              (ptr(w), 2, 5, 6, 3, ptr(h), ptr(h), ptr(o)), (ptr(w), 2, 5, 6, 3, ptr(h), C.c_void_p(h.data_ptr() + 23), ptr(o)),
              (ptr(w), 2, 5, 6, 3, None, C.c_void_p(w.data_ptr() + 40), ptr(o)), (ptr(w), 2, 5, 6, 3, ptr(o), None, ptr(o)),
              (ptr(w), 2, 5, 6, 3, None, C.c_void_p(o.data_ptr() + 59), ptr(o))):
        assert il(*a) == QPSK_ERR_ARG, a
        assert b"qpsk_outer_interleave_batch" in m.L.qpsk_last_error()
    m.sync()
    m.close()


def test_push_buffers_that_touch_are_accepted_and_the_least_shared_bytes_are_refused():
    """2 streams, n = 4, 64 bits a push, four slots, all six buffers inside one allocation.  Every pair of them, one of the two moved so
    that it ends where the other begins and begins where the other ends (accepted, and the push is the restatement's), then one step of
    its alignment further in (refused: "<the later argument> overlaps <the earlier>"); the link goes on behind the refusals"""
    import torch
    from test_outer_cpu import LEADS, streams_of
    S, n, nbits, mw = 2, 4, 64, 4
    bits = streams_of(np.random.default_rng(64), n, 2, 70, ("clean", "delete"), leads=LEADS[:2])[0]
    assert bits.shape[0] == S and bits.shape[1] >= 31 * nbits
    m = modem()
    m.outer_reset(S, n, 2, 0x47, 2, 2)
    ref = outer_ref(S, n, 2, 0x47, 2, 2)
    assert m.outer_max_words(nbits) == mw
    names = ("d_bits", "d_count", "d_words", "d_pos", "d_flags", "d_info")
    size = dict(d_bits=S * 8, d_count=S * 4, d_words=S * mw * n, d_pos=S * mw * 8, d_flags=S * mw, d_info=S * 16)
    align = dict(d_bits=1, d_count=4, d_words=1, d_pos=8, d_flags=1, d_info=4)
    home = {name: 256 * (i + 1) for i, name in enumerate(names)}
    arena = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    pushes = 0

    def push_at(where):
        nonlocal pushes
        chunk = bits[:, pushes * nbits:(pushes + 1) * nbits]
        host = np.full(2048, 0x55, np.uint8)
        host[where["d_bits"]:where["d_bits"] + S * 8] = pack_bits(chunk).reshape(-1)
        arena.copy_(torch.from_numpy(host))
        p = {k: C.c_void_p(arena.data_ptr() + v) for k, v in where.items()}
        rc = m.L.qpsk_outer_push(m.h, p["d_bits"], 0, nbits, mw, p["d_count"], p["d_words"], 0, p["d_pos"], p["d_flags"], p["d_info"])
        torch.cuda.synchronize()
        if rc:
            return rc
        pushes += 1
        host = arena.cpu().numpy()
        cut = lambda name, dtype, shape: host[where[name]:where[name] + size[name]].view(dtype).reshape(shape)      # noqa: E731
        count = cut("d_count", np.int32, (S,))
        kept = np.minimum(count, mw)
        got = dict(count=count, max_words=mw, info=cut("d_info", np.int32, (S, 4)), words=[cut("d_words", np.uint8, (S, mw, n))[i, :kept[i]] for i in range(S)],
                   pos=[cut("d_pos", np.int64, (S, mw))[i, :kept[i]] for i in range(S)], flags=[cut("d_flags", np.uint8, (S, mw))[i, :kept[i]] for i in range(S)])
        same(got, ref.push(chunk), where)
        return 0

    assert push_at(home) == 0
    for j, later in enumerate(names):
        for earlier in names[:j]:
            mover, fixed = (later, earlier) if align[later] <= align[earlier] else (earlier, later)
            lo, hi, step = home[fixed] - size[mover], home[fixed] + size[fixed], align[mover]
            for off, accepted in ((lo, True), (hi, True), (lo + step, False), (hi - step, False)):
                rc = push_at({**home, mover: off})
                if accepted:
                    assert rc == 0, (later, earlier, off, m.L.qpsk_last_error())
                else:
                    assert rc == QPSK_ERR_ARG and ("qpsk_outer_push: %s overlaps %s" % (later, earlier)).encode() in m.L.qpsk_last_error(), (later, earlier, off)
    assert pushes == 31
    m.sync()
    m.close()


def test_a_reset_over_an_armed_link_replaces_it():
    bits, other = replaced_link_inputs()
    S, N = bits.shape
    m = modem()
    m.outer_reset(S, 4, 2, 0x47, 2, 2)
    run_both(m, outer_ref(S, 4, 2, 0x47, 2, 2), 4, bits, [(0, N // 2)])
    m.outer_reset(3, 6, 3, 0xB8, 1, 0, polarity=False)
    calls = run_both(m, outer_ref(3, 6, 3, 0xB8, 1, 0, 0), 6, other, [(0, other.shape[1])])
    assert (calls[0]["pos"][0] < N // 2).any()                # positions count from the new reset
    m.close()


# ------------------------------------------------------------------------------------------ 8a. limits, edges and chunks
# The inputs are input sets of test_outer_cpu.py; test_outer_port_cpu.py shows on the scalar port of the kernel what each is there to catch.
@pytest.mark.parametrize("n,I,L,drop,split", LIMITS)
def test_the_limits_of_the_geometry_32_branches_a_lock_of_16_and_a_drop_of_16(n, I, L, drop, split):
    m = modem()
    run_set(m, limit_set(n, I, L, drop, split))
    m.sync()
    m.close()


@pytest.mark.parametrize("n,I,L", EDGES)
def test_a_push_that_ends_on_the_last_bit_of_a_look_ahead_or_of_a_word_and_one_that_ends_a_bit_sooner(n, I, L):
    """the lock is declared by the push that brings the last bit of the candidate's look-ahead, a word is emitted by the push that brings
    its last bit: lead-ins of 0 .. 9 bits, cuts from two bits before to two bits behind (the sets assert that on the reference)"""
    m = modem()
    sets = edge_sets(n, I, L)
    assert len(sets) == 14 + 11
    for s in sets:
        run_set(m, s)
    m.sync()
    m.close()


@pytest.mark.parametrize("phase", [0, 3])
def test_a_hunt_whose_look_ahead_spans_four_chunks_finds_nothing_in_noise_and_then_the_stream(phase):
    m = modem()
    calls = run_set(m, noise_set(phase))
    assert not calls[-2]["count"].any() and not calls[-2]["info"].any() and (calls[-1]["info"][:, 0] == 1).all()
    m.close()


def test_a_push_with_no_slots_writes_the_true_count_and_nothing_else_and_the_link_goes_on():
    """max_words = 0 with all four outputs given: push() finds its poison in every byte of d_words, d_pos and d_flags"""
    m = modem()
    calls = run_set(m, no_slots_set())
    assert calls[1]["max_words"] == 0 and (calls[1]["count"] > 0).all() and all(len(w) == 0 for w in calls[1]["words"])
    assert set(calls[1]) >= {"words", "pos", "flags", "info"}
    m.close()


# ------------------------------------------------------------------------------------------ 9. the interleaver
@pytest.mark.parametrize("n,I", [(4, 1), (4, 2), (4, 4), (6, 3), (255, 1), (204, 12)])
@pytest.mark.parametrize("R", [1, 5, 70])
def test_the_interleaver_with_a_history_carried_across_calls(n, I, R):
    rng = np.random.default_rng(n + I + R)
    nw = 2 * I + 3
    x = rng.integers(0, 256, (R, nw, n), dtype=np.uint8)
    want, want_hist = outer_interleave_ref(x, I)
    m = modem()
    hist, parts = None, []
    for a, b in ((0, 1), (1, I + 2), (I + 2, nw)):           # a call shorter than the history among them
        y, hist = m.outer_interleave(x[:, a:b], I, hist)
        assert m.last_kernel() == "outer_interleave_kernel"
        parts.append(y.cpu().numpy())
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    assert np.array_equal(hist.cpu().numpy(), want_hist)
    one, h1 = m.outer_interleave(x, I)
    assert np.array_equal(one.cpu().numpy(), want) and np.array_equal(h1.cpu().numpy(), want_hist)
    m.close()


def test_the_interleaver_writes_nothing_behind_its_outputs_and_takes_a_null_history_out():
    import torch
    rng = np.random.default_rng(99)
    R, nw, n, I = 5, 7, 6, 3
    x = rng.integers(0, 256, (R, nw, n), dtype=np.uint8)
    hin = rng.integers(0, 256, (R, I - 1, n), dtype=np.uint8)
    want, want_hist = outer_interleave_ref(x, I, hin)
    m = modem()
    d_x, d_h = torch.from_numpy(x).cuda(), torch.from_numpy(hin).cuda()
    out = torch.full((R * nw * n + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    hout = torch.full((R * (I - 1) * n + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    for d_hout in (ptr(hout), None):
        m._check(m.L.qpsk_outer_interleave_batch(m.h, ptr(d_x), R, nw, n, I, ptr(d_h), d_hout, ptr(out)))
        torch.cuda.synchronize()
        o, h = out.cpu().numpy(), hout.cpu().numpy()
        assert np.array_equal(o[:R * nw * n].reshape(R, nw, n), want) and (o[R * nw * n:] == 0x55).all()
        assert np.array_equal(h[:R * (I - 1) * n].reshape(R, I - 1, n), want_hist) and (h[R * (I - 1) * n:] == 0x55).all()
    m.close()


# ------------------------------------------------------------------------------------------ 10. the composition on the device
@pytest.mark.parametrize("I", [1, 12])
def test_the_link_of_the_restatements_with_the_library_s_calls(I):
    """test_outer_cpu's link: rs_encode_batch -> outer_interleave_batch -> conv_encode_stream_batch -> the damage -> viterbi_stream_push in
    several pushes -> outer_push straight on its d_bits -> rs_decode_batch with in_pitch = word_pitch; every stage equal to the CPU link's"""
    import torch
    r, p = link_result()[I], LINK
    n, nroots, wp = p["n"], p["n"] - p["k"], 64
    m = modem()
    sent = m.rs_encode(np.ascontiguousarray(r["sent"][:, :p["k"]]), nroots)
    assert np.array_equal(sent.cpu().numpy(), r["sent"])
    y, _ = m.outer_interleave(sent.contiguous().reshape(1, -1, n), I)
    assert np.array_equal(y.cpu().numpy()[0], r["interleaved"])
    nbits = 8 * y.numel()
    dibits, _ = m.conv_encode_stream(y.reshape(1, -1), nbits)      # a byte's bit 0 first: the byte row is the packed bit row
    assert np.array_equal(dibits.cpu().numpy(), r["dibits"])
    soft = torch.from_numpy(r["soft"]).cuda()
    m.viterbi_stream_reset(1, p["depth"], p["window"])
    m.outer_reset(1, n, I, p["sync"], p["lock"], p["drop"])
    vouts = [m.viterbi_stream(soft[:, a:b].contiguous()) for a, b in zip(r["cuts"][:-1], r["cuts"][1:])] + [m.viterbi_stream_flush()]
    ocalls = iter(r["ocalls"])
    decoded, infos = [], []
    for v, want_v in zip(vouts, r["vcalls"]):
        assert v["nbits"] == want_v["nbits"] and np.array_equal(v["bits"].cpu().numpy(), want_v["bits"])
        assert np.array_equal(v["info"].cpu().numpy(), want_v["info"])
        if not v["nbits"]:
            continue
        got = push(m, 1, n, v["bits"].contiguous(), nbits=v["nbits"], word_pitch=wp)
        same(got, next(ocalls), "outer_push on the decoder's d_bits")
        k = int(got["count"][0])
        if k:      # the rows of d_words as they lie: qpsk_rs_decode_batch's d_in with in_pitch = word_pitch
            rows = got["d_words"][:got["max_words"] * wp].reshape(got["max_words"], wp)
            out, info = m.rs_decode(rows, nroots, pitch=wp, n=n)
            decoded.append(out.cpu().numpy()[:k])
            infos.append(info.cpu().numpy()[:k])
    assert np.array_equal(np.concatenate(decoded), r["decoded"]) and np.array_equal(np.concatenate(infos), r["info"])
    m.sync()
    m.close()
