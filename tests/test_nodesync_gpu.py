"""qpsk_nodesync_* on the GPU: every output byte and every d_info word of every call against test_nodesync_cpu.nodesync_ref (NODE SYNC of
include/qpsk_hip.h restated in numpy).  Poison (0x55) sits in front of, between and behind the rows of both soft buffers, whose first rows
begin 2 bytes behind a 16-byte boundary at odd pitches, so every row meets the vector path at another alignment.  The closed loops are the CPU
file's, run with the library's calls, the decoder's d_info handed to the next tick on the device.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_nodesync_cpu import LOOP, LOOPS, THRESHOLD, clean_words, lock_calls, loop_link, loop_result, nodesync_ref
from test_outer_gpu import push as outer_push, same as outer_same
from test_viterbi_gpu import modem, ptr
from test_viterbi_stream_cpu import random_soft

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
GUARD = 64
POISON = 0x55555555


def soft_rows(rows, pitch, S, ntx):
    """a device byte buffer of S rows `pitch` dibits apart, the first 2 bytes behind a 16-byte boundary, poison everywhere but in `rows`
    (numpy (S, ntx, 2) int8 or None) -> (the buffer, the view that begins at the first row)"""
    import torch
    h = np.full(2 + 2 * S * pitch + GUARD, 0x55, np.uint8)
    if rows is not None:
        v = h[2:2 + 2 * S * pitch].reshape(S, pitch, 2)
        v[:, :ntx] = rows.view(np.uint8)
    d = torch.from_numpy(h).cuda()
    assert d.data_ptr() % 16 == 0
    return d, d[2:]


def ns_push(m, soft, vinfo=None, in_pitch=0, out_pitch=0, want_info=True):
    """a raw qpsk_nodesync_push with guarded buffers.  soft: numpy (S, ntx, 2) int8; vinfo: numpy (S, 4), a device tensor or None"""
    import torch
    S, ntx = soft.shape[:2]
    ip, op = in_pitch or ntx, out_pitch or ntx
    _, d_in = soft_rows(soft, ip, S, ntx)
    d_out_all, d_out = soft_rows(None, op, S, ntx)
    d_v = None if vinfo is None else vinfo if hasattr(vinfo, "data_ptr") else torch.from_numpy(np.ascontiguousarray(vinfo, np.int32)).cuda()
    info = torch.full((S * 8 + GUARD,), POISON, dtype=torch.int32, device="cuda") if want_info else None
    m._check(m.L.qpsk_nodesync_push(m.h, ptr(d_in), in_pitch, ntx, ptr(d_v), ptr(d_out), out_pitch, ptr(info)))
    assert m.last_kernel() == "nodesync_push_kernel"
    torch.cuda.synchronize()
    h = d_out_all.cpu().numpy()
    rows = h[2:2 + 2 * S * op].reshape(S, op, 2)
    assert (h[:2] == 0x55).all() and (h[2 + 2 * S * op:] == 0x55).all() and (rows[:, ntx:] == 0x55).all(), "bytes outside the rows were written"
    out = dict(soft=rows[:, :ntx].copy().view(np.int8))
    if info is not None:
        h = info.cpu().numpy()
        assert (h[S * 8:] == POISON).all(), "guard behind d_info overwritten"
        out["info"] = h[:S * 8].reshape(S, 8)
    return out


def same(got, want, what=""):
    if "info" in got:
        assert np.array_equal(got["info"], want["info"]), (what, "info", got["info"], want["info"])
    bad = np.argwhere(got["soft"] != want["soft"])
    assert bad.size == 0, (what, "soft differs at (link, dibit, component)", bad[:8], got["soft"][tuple(bad[0])], want["soft"][tuple(bad[0])])


def cand_tensor(c):
    import torch
    return torch.from_numpy(np.asarray(c, np.int32)).cuda()


# ------------------------------------------------------------------------------------------ 6. the transform alone
CANDS = [0 + 4 * 0, 1 + 4 * 1, 2 + 4 * 7, 3 + 4 * 8, 1 + 4 * 31]      # (r, h) = (0, 0), (1, 1), (2, 7), (3, 8), (1, 31)


def test_the_transform_bit_for_bit_at_every_alignment_and_across_the_cuts():
    rng = np.random.default_rng(6)
    S, total = 5, 31 + 33 + 516 + 2052
    soft = random_soft(rng, S, total)
    assert (soft == -128).any() and (soft == 0).any()
    m = modem()
    whole = []
    for sizes in ((31, 33, 516, 2052), (516, 33, 2052, 31)):
        m.nodesync_reset(S, nrot=4, nshift=32)
        assert m.last_kernel() == "nodesync_init_kernel"
        m.nodesync_set(cand_tensor(CANDS))
        assert m.last_kernel() == "nodesync_init_kernel"
        ref = nodesync_ref(S, nrot=4, nshift=32)
        ref.set(CANDS)
        at, parts = 0, []
        for ntx in sizes:
            got = ns_push(m, soft[:, at:at + ntx], in_pitch=2055, out_pitch=2053)
            same(got, ref.push(soft[:, at:at + ntx]), (sizes, ntx))
            parts.append(got["soft"])
            at += ntx
        whole.append(np.concatenate(parts, axis=1))
        assert got["info"][:, :2].tolist() == [[0, 0], [1, 1], [2, 7], [3, 8], [1, 31]]
    assert np.array_equal(whole[0], whole[1])                     # property 2 on the device
    assert not whole[0][4, :31].any() and not (whole[0] == -128).any()      # the erasure fill of the first push
    # the pitches 0 = ntx, and no d_info
    m.nodesync_reset(3, nrot=1, nshift=1)
    got = ns_push(m, soft[:3, :700], want_info=False)
    assert np.array_equal(got["soft"], np.where(soft[:3, :700] == -128, -127, soft[:3, :700]))      # property 1
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 7. the tick alone
def test_the_tick_word_for_word_on_every_branch():
    rng = np.random.default_rng(7)
    x = random_soft(rng, 3, 4)
    m = modem()
    # link 0: the hand cases of the CPU file (settle, good, bad while locked below and at drop, the wrap, bad while hunting, n = 0);
    # links 1 and 2: random counts around the threshold 1 / 10, so that every branch is taken many times
    hand = [(5, 0), (30, 30), (30, 30), (4, 60), (6, 40), (11, 100), (0, 100), (11, 100), (11, 100), (0, 50), (50, 100)]
    calls = 48
    seq = np.zeros((calls, 3, 4), np.int32)
    seq[:, :, 2:] = rng.integers(-5, 5, (calls, 3, 2))            # words 2 and 3 are not the tick's
    seq[:len(hand), 0, :2] = hand
    n = rng.choice([0, 20, 60, 100, 130], (calls, 3))
    seq[len(hand):, 0, 1] = n[len(hand):, 0]
    seq[:, 1:, 1] = n[:, 1:]
    e = (n * rng.choice([0.02, 0.09, 0.11, 0.3], (calls, 3))).astype(np.int32)
    seq[len(hand):, 0, 0] = e[len(hand):, 0]
    seq[:, 1:, 0] = e[:, 1:]
    kw = dict(nrot=2, nshift=2, span=100, settle=50, threshold=(1, 10), drop=2)
    m.nodesync_reset(3, **kw)
    m.nodesync_set(cand_tensor([3, 0, 6]))
    ref = nodesync_ref(3, **kw)
    ref.set([3, 0, 6])
    same(ns_push(m, x), ref.push(x), "no tick")
    seen = set()
    for k in range(calls):
        got, want = ns_push(m, x, seq[k]), ref.push(x, seq[k])
        same(got, want, ("call", k))
        seen.update((int(v), int(l)) for v, l in zip(want["info"][:, 4], want["info"][:, 2]))
    assert seen >= {(0, 0), (0, 1), (1, 1), (2, 0), (2, 1), (3, 0)}          # every verdict, hunting and locked
    assert max(s["switches"] for s in ref.st) > 4                          # the wrap C - 1 -> 0 among them
    # an int64 product that overflows int32: span 2^24 with the threshold 65535 / 65535
    kw = dict(nrot=1, nshift=1, span=1 << 24, settle=0, threshold=(65535, 65535), drop=1)
    m.nodesync_reset(1, **kw)
    ref = nodesync_ref(1, **kw)
    for k, (e, n) in enumerate([(1 << 23, 1 << 23), (1 << 23, 1 << 23), ((1 << 24) + 1, 1 << 24), ((1 << 24) - 1, 1 << 24)]):
        v = np.array([[e, n, 0, 0]], np.int32)
        got, want = ns_push(m, x[:1], v), ref.push(x[:1], v)
        same(got, want, ("big", k))
    assert want["info"][0].tolist() == [0, 0, 1, 1, 1, 0, 0, 0]
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 8. / 9. the closed loop with the library's calls
def run_loop(m, name):
    """qpsk_nodesync_push -> qpsk_viterbi_stream_push over the CPU file's blocks, the decoder's d_info handed on as a device pointer; nothing
    is copied to the host before the last call is enqueued"""
    p, q, res = LOOP, LOOPS[name], loop_result(name)
    m.nodesync_reset(1, q["nrot"], res["nshift"], p["span"], p["settle"], THRESHOLD[name], p["drop"])
    m.viterbi_stream_reset(1, p["depth"], p["window"], name)
    ncalls, vcalls, v = [], [], None
    for blk in res["blocks"]:
        n = m.nodesync(blk, vinfo=v)
        assert m.last_kernel() == "nodesync_push_kernel"
        v = m.viterbi_stream(n)
        ncalls.append(n)
        vcalls.append(v)
    m.sync()
    return res, ncalls, vcalls


@pytest.mark.parametrize("name", ["3/4", "1/2"])
def test_the_closed_loop_of_the_restatements_with_the_library_s_calls(name):
    m = modem()
    res, ncalls, vcalls = run_loop(m, name)
    for k, (n, v, wn, wv) in enumerate(zip(ncalls, vcalls, res["ncalls"], res["vcalls"])):
        same(dict(soft=n["soft"].cpu().numpy(), info=n["info"].cpu().numpy()), wn, (name, "call", k))
        assert v["nbits"] == wv["nbits"] and np.array_equal(v["bits"].cpu().numpy(), wv["bits"]), (name, "call", k)
        assert np.array_equal(v["info"].cpu().numpy(), wv["info"]), (name, "call", k)
    assert len(lock_calls(res["info"])) == (2 if LOOPS[name]["slip"] else 1)      # the slip and the relock are among the calls
    m.close()


def test_the_link_behind_the_loop_decodes_every_word_after_the_lock():
    """the 3/4 loop's bits on into qpsk_outer_push with QPSK_OUTER_POLARITY and qpsk_rs_decode_batch on RS (60, 44) words with the sync byte as
    byte 0: the outer link reports s = -1 for the half-turn twin, and every word whose bits were decoded under a lock decodes clean"""
    p, wp = LOOP, 64
    n, nroots = p["n"], p["n"] - p["k"]
    want = loop_link()
    m = modem()
    res, ncalls, vcalls = run_loop(m, "3/4")
    m.outer_reset(1, n, 1, p["sync"], 2, 3)
    words, pos, flags, decoded, infos = [], [], [], [], []
    for v, wo in zip(vcalls, want["ocalls"]):
        if not v["nbits"]:
            assert wo is None
            continue
        got = outer_push(m, 1, n, v["bits"].contiguous(), nbits=v["nbits"], word_pitch=wp)
        outer_same(got, wo, "outer_push on the decoder's d_bits")
        k = int(got["count"][0])
        if k:
            rows = got["d_words"][:got["max_words"] * wp].reshape(got["max_words"], wp)
            out, info = m.rs_decode(rows, nroots, pitch=wp, n=n)
            decoded.append(out.cpu().numpy()[:k])
            infos.append(info.cpu().numpy()[:k])
            pos.append(got["pos"][0])
            flags.append(got["flags"][0])
        last = got
    decoded, infos, pos, flags = np.concatenate(decoded), np.concatenate(infos), np.concatenate(pos), np.concatenate(flags)
    assert np.array_equal(decoded, want["decoded"]) and np.array_equal(infos, want["rsinfo"]) and np.array_equal(pos, want["pos"])
    assert last["info"][0, :2].tolist() == [1, -1]                # locked, the stream inverted
    ok = clean_words(res, pos)
    assert ok.sum() >= 40 and (flags[ok] & 2).all() and (infos[ok, 0] >= 0).all()
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 10. the kernel's name, the refusals, a reset over an armed node sync
def test_refusals_launch_nothing_and_leave_the_state_as_it_was():
    import torch
    rng = np.random.default_rng(10)
    S = 2
    soft = random_soft(rng, S, 64)
    m = modem()
    L = m.L
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    at = lambda off: C.c_void_p(buf.data_ptr() + off)
    word = torch.zeros(64, dtype=torch.int32, device="cuda")

    def refused(rc, code, text):
        assert rc == code and text in L.qpsk_last_error(), (rc, L.qpsk_last_error())
    # before a reset
    refused(L.qpsk_nodesync_push(m.h, at(0), 0, 8, None, at(1024), 0, None), QPSK_ERR_STATE, b"no qpsk_nodesync_reset yet")
    refused(L.qpsk_nodesync_set(m.h, None), QPSK_ERR_STATE, b"no qpsk_nodesync_reset yet")
    kw = dict(nrot=2, nshift=8, span=64, settle=0, threshold=(1, 4), drop=1)
    m.nodesync_reset(S, **kw)
    m.nodesync_set(cand_tensor([5, 14]))
    ref = nodesync_ref(S, **kw)
    ref.set([5, 14])
    same(ns_push(m, soft[:, :20]), ref.push(soft[:, :20]), "before the refusals")
    before = m.last_kernel()
    push = lambda i=at(0), ip=0, ntx=8, v=None, o=at(1024), op=0, info=None: L.qpsk_nodesync_push(m.h, i, ip, ntx, v, o, op, info)
    for k, text in ((dict(i=None), b"null context, input or d_soft_out"), (dict(o=None), b"null context, input or d_soft_out"),
                    (dict(ntx=0), b"ntx = 0 outside"), (dict(ntx=6), b"ntx = 6 outside max(1, nshift - 1 = 7)"), (dict(ntx=-1), b"ntx = -1"),
                    (dict(ntx=(1 << 20) + 1), b"ntx = 1048577 outside"), (dict(ip=7), b"in_pitch = 7"), (dict(op=7), b"out_pitch = 7"),
                    (dict(ip=-1), b"in_pitch = -1"), (dict(i=at(1)), b"not 2-byte aligned"), (dict(o=at(1025)), b"not 2-byte aligned"),
                    (dict(v=C.c_void_p(word.data_ptr() + 2)), b"d_vinfo or d_info is not 4-byte aligned"),
                    (dict(info=C.c_void_p(word.data_ptr() + 1)), b"d_vinfo or d_info is not 4-byte aligned"),
                    (dict(o=at(0)), b"d_soft_out overlaps d_soft_in"), (dict(o=at(30)), b"d_soft_out overlaps d_soft_in"),
                    (dict(i=at(1024 + 30)), b"d_soft_out overlaps d_soft_in"), (dict(ip=100, o=at(200)), b"d_soft_out overlaps d_soft_in")):
        refused(push(**k), QPSK_ERR_ARG, text)
    refused(L.qpsk_nodesync_set(m.h, C.c_void_p(word.data_ptr() + 2)), QPSK_ERR_ARG, b"d_cand is not 4-byte aligned")
    assert push(o=at(32)) == 0                                    # abutting, not overlapping: S rows of 8 dibits are 32 bytes
    ref.push(np.zeros((S, 8, 2), np.int8))
    assert m.last_kernel() == "nodesync_push_kernel" == before
    # a refused reset leaves the armed node sync as it was: candidates, counters and history
    refused(L.qpsk_nodesync_reset(m.h, S, 3, 8, 64, 0, 1, 4, 1), QPSK_ERR_ARG, b"nrot = 3")
    refused(L.qpsk_nodesync_reset(m.h, 0, 2, 8, 64, 0, 1, 4, 1), QPSK_ERR_ARG, b"nlinks = 0")
    v = np.array([[40, 64, 0, 0], [1, 64, 0, 0]], np.int32)
    got, want = ns_push(m, soft[:, 20:], v), ref.push(soft[:, 20:], v)
    same(got, want, "behind the refusals")
    assert want["info"][:, :5].tolist() == [[0, 3, 0, 1, 2], [0, 7, 1, 0, 1]]      # link 0 moved on, link 1 locked
    # a reset over an armed node sync: candidate 0, no history, whatever the old geometry was
    m.nodesync_reset(3, nrot=1, nshift=3)
    assert m.last_kernel() == "nodesync_init_kernel"
    ref = nodesync_ref(3, nrot=1, nshift=3)
    s3 = random_soft(rng, 3, 40)
    same(ns_push(m, s3), ref.push(s3), "behind the reset")
    m.nodesync_set(None)
    ref.set(None)
    m.nodesync_set(cand_tensor([2, -1, 7]))
    ref.set([2, -1, 7])
    got = ns_push(m, s3)
    same(got, ref.push(s3), "behind the set")
    assert got["info"][:, 1].tolist() == [2, 0, 1]                # -1 = 2^32 - 1 = 0 mod 3, 7 = 1 mod 3
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 11. the boundary of the overlap test
def test_buffers_that_touch_are_accepted_and_a_shared_dibit_is_refused():
    """2 links of 64 dibits inside one allocation.  The rows of a buffer span 2 ((S - 1) pitch + ntx) bytes: 256 when tight, 272 at pitch 72,
    and the 16 bytes of padding behind the last row are not the buffer.  Both pointers are 2-byte aligned, so the least two ranges can share
    is one dibit.  An accepted call's output is the reference's; a refused one leaves the links where they were."""
    import torch
    rng = np.random.default_rng(11)
    S, ntx, pitch = 2, 64, 72
    soft = random_soft(rng, S, ntx)
    m = modem()
    L = m.L
    kw = dict(nrot=4, nshift=8)
    m.nodesync_reset(S, **kw)
    m.nodesync_set(cand_tensor([5, 14]))
    ref = nodesync_ref(S, **kw)
    ref.set([5, 14])
    arena = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    at = lambda off: C.c_void_p(arena.data_ptr() + off)
    cases = (      # the input at, its pitch, the output at, its pitch, accepted
        (512, 0, 768, 0, True), (512, 0, 256, 0, True), (512, 0, 766, 0, False), (512, 0, 258, 0, False),
        (512, pitch, 784, 0, True), (512, pitch, 782, 0, False), (512, 0, 240, pitch, True), (512, 0, 242, pitch, False))
    for k, (i0, ip, o0, op, accepted) in enumerate(cases):
        rows = np.zeros((S, ip or ntx, 2), np.int8)
        rows[:, :ntx] = soft
        arena[i0:i0 + rows.size] = torch.from_numpy(rows.view(np.uint8).reshape(-1)).cuda()
        info = torch.full((S * 8,), POISON, dtype=torch.int32, device="cuda") if k else None      # the first call: no d_info, and never a d_vinfo
        rc = L.qpsk_nodesync_push(m.h, at(i0), ip, ntx, None, at(o0), op, ptr(info))
        if not accepted:
            assert rc == QPSK_ERR_ARG and b"d_soft_out overlaps d_soft_in" in L.qpsk_last_error(), (k, rc, L.qpsk_last_error())
            continue
        assert rc == 0, (k, L.qpsk_last_error())
        torch.cuda.synchronize()
        h = arena.cpu().numpy()
        got = dict(soft=np.stack([h[o0 + 2 * s * (op or ntx):][:2 * ntx] for s in range(S)]).reshape(S, ntx, 2).view(np.int8))
        if info is not None:
            got["info"] = info.cpu().numpy().reshape(S, 8)
        same(got, ref.push(soft), cases[k])
    m.sync()
    m.close()
