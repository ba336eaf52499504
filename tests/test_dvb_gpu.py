"""DVB-S transport framing on the GPU: qpsk_outer_reset_group's pushes and qpsk_dispersal_batch, every output of every call bit for bit against
test_dvb_cpu.outer_group_ref / dispersal_ref (GROUP SYNC and DVB TRANSPORT of include/qpsk_hip.h restated in numpy).  The pushes go through
test_outer_gpu.push, so poison sits behind every output and behind every input row's bits; the dispersal's rows lie in poisoned buffers with
guard bytes in front of, between and behind them.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_dvb_cpu import (DVB, GPU_DROP, GPU_FLAGS, GPU_GROUPS, LATE_DECOYS, LONG_FLAGS, LONG_LOCKS, dispersal_ref, dvb_link_result,
                          group_sync_inputs, late_decoy_set, long_lock_set, outer_group_ref)
from test_outer_cpu import MSB_FIRST, POLARITY, bytes_to_bits, cut, outer_ref, partition_inputs, split_sizes
from test_outer_gpu import run_both, run_set
from test_viterbi_cpu import pack_bits
from test_viterbi_gpu import modem, ptr

pytestmark = pytest.mark.gpu

GUARD = 64


# ------------------------------------------------------------------------------------------ 1. group sync
@pytest.mark.parametrize("n,I,G,L", GPU_GROUPS)
@pytest.mark.parametrize("flags", GPU_FLAGS)
def test_group_sync_at_every_geometry_bit_order_polarity_and_bit_phase(n, I, G, L, flags):
    bits, spans = group_sync_inputs(n, I, G, L, flags)        # five streams; every bit phase begins a push
    S, N = bits.shape
    drop = GPU_DROP
    m = modem()
    m.outer_reset(S, n, I, 0x47, L, drop, polarity=bool(flags & POLARITY), msb_first=bool(flags & MSB_FIRST), group=G)
    assert m.last_kernel() == "outer_init_kernel"
    calls = run_both(m, outer_group_ref(S, n, I, 0x47, L, drop, flags, G), n, bits, spans)
    emitted = sum(c["count"].astype(np.int64) for c in calls)
    info = sum(c["info"][:, 2:].astype(np.int64) for c in calls)
    if flags & POLARITY:
        assert (emitted > 0).all() and (info[3:, 1] >= 1).all() and (info[3:, 0] >= 2).all()      # the slips cost a lock, and it came back
        groups = np.concatenate([f >> 4 for c in calls for f in c["flags"]])
        assert set(groups.tolist()) == set(range(G))
        assert all((f & 2).all() for c in calls for f in (c["flags"][1], c["flags"][3])) and any((c["flags"][1] & 2).any() for c in calls)
    else:
        assert emitted[1] == 0 and emitted[3] == 0 and emitted[0] > 0      # the inverted streams never lock
    m.sync()
    m.close()


# The inputs of the next two are input sets of test_dvb_cpu.py; test_outer_port_cpu.py shows on the scalar port of the kernel what each is
# there to catch (p0's bits from 2 G on, I = 32 under group sync; a legal-mask test that forgets fx < G or fy < G).
@pytest.mark.parametrize("n,I,G,L", LONG_LOCKS)
@pytest.mark.parametrize("flags", LONG_FLAGS)
def test_group_sync_with_a_look_ahead_longer_than_two_groups_and_with_32_branches(n, I, G, L, flags):
    m = modem()
    run_set(m, long_lock_set(n, I, G, L, flags))             # every group index appears in the flags: asserted on the reference
    m.sync()
    m.close()


@pytest.mark.parametrize("n,I,G,L", LATE_DECOYS)
def test_a_decoy_whose_first_complement_comes_a_whole_group_late_is_not_a_lock(n, I, G, L):
    """L sync-like bytes with complements at G, 2 G, ... and none at 0, upright and inverted: no lock while they pass, one lock on the first
    word of the stream behind them (asserted on the reference)"""
    m = modem()
    calls = run_set(m, late_decoy_set(n, I, G, L))
    assert np.array_equal(sum(c["info"][:, 2:] for c in calls), [[1, 0]] * 4) and all(c["info"][:, 0].all() for c in calls[-1:])
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. the old reset
@pytest.mark.parametrize("n,I,L,drop", [(6, 3, 3, 1), (204, 12, 2, 3)])
def test_the_old_reset_is_unchanged(n, I, L, drop):
    """test_outer_gpu's partition cases through qpsk_outer_reset, and through qpsk_outer_reset_group with group 0: outer_ref's outputs, bits
    4..7 of the flags zero"""
    bits = partition_inputs(n, I)
    S, N = bits.shape
    m = modem()
    for group_zero in (False, True):
        if group_zero:
            m._check(m.L.qpsk_outer_reset_group(m.h, S, n, I, 0x47, L, drop, POLARITY, 0))
        else:
            m.outer_reset(S, n, I, 0x47, L, drop)
        calls = run_both(m, outer_ref(S, n, I, 0x47, L, drop), n, bits, cut(N, split_sizes(n)))
        assert sum(int(c["count"].sum()) for c in calls) > S and all((f < 4).all() for c in calls for f in c["flags"])
    assert m.L.qpsk_outer_reset(m.h, S, n, I, 0x47, L, drop, 4) == -2 and b"unknown flags 0x4" in m.L.qpsk_last_error()
    m.close()


# ------------------------------------------------------------------------------------------ 3. dispersal
def run_dispersal(m, x, group, index=None, first=0, msb=False, ip=0, op=0, inplace=False, offset=0, rng=None):
    """the raw call on rows that lie in poisoned buffers, GUARD + offset bytes in: every byte of the output buffer against what it must
    hold -- the rows' results, and poison (or, in place, the input's bytes) everywhere else"""
    import torch
    R, n = x.shape
    ipitch, opitch = ip or n, op or n
    if inplace:
        assert ipitch == opitch
    src = np.full(2 * GUARD + offset + R * ipitch, 0x55, np.uint8)
    rows = np.lib.stride_tricks.as_strided(src[GUARD + offset:], (R, n), (ipitch, 1))
    rows[:] = x
    want = src.copy() if inplace else np.full(2 * GUARD + offset + R * opitch, 0x55, np.uint8)
    idx = (first + np.arange(R)) % group if index is None else np.asarray(index)
    np.lib.stride_tricks.as_strided(want[GUARD + offset:], (R, n), (opitch, 1))[:] = dispersal_ref(x, group, idx, msb)
    d_in = torch.from_numpy(src).cuda()
    d_out = d_in if inplace else torch.full((len(want),), 0x55, dtype=torch.uint8, device="cuda")
    d_fl = None
    if index is not None:      # the low four bits are qpsk_outer_push's own and must not matter
        fl = np.full(R + 2 * GUARD, 0x55, np.uint8)
        fl[GUARD:GUARD + R] = (idx << 4) | rng.integers(0, 16, R)
        d_fl = torch.from_numpy(fl).cuda()
    at = lambda t, off: C.c_void_p(t.data_ptr() + off)
    m._check(m.L.qpsk_dispersal_batch(m.h, at(d_in, GUARD + offset), ip, R, n, group, 1 if msb else 0, at(d_fl, GUARD) if d_fl is not None else None,
                                      first, at(d_out, GUARD + offset), op))
    assert m.last_kernel() == "dispersal_kernel"
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want), ("first difference at byte", int(np.argmax(got != want)) - GUARD - offset)
    if not inplace:
        assert np.array_equal(d_in.cpu().numpy(), src), "the input was written"
    if d_fl is not None:
        assert np.array_equal(d_fl.cpu().numpy(), fl)


SHAPES = [  # len, group, in_pitch, out_pitch, rows, offset of the first row from an aligned address
    (188, 8, 0, 0, 37, 0), (188, 8, 204, 204, 37, 0), (188, 8, 207, 207, 37, 0), (188, 8, 204, 188, 19, 0), (188, 8, 204, 204, 19, 1),
    (2, 1, 0, 0, 301, 0), (2, 16, 4, 4, 33, 0), (255, 16, 0, 0, 35, 0), (255, 16, 256, 256, 35, 0), (255, 1, 256, 260, 3, 0), (7, 3, 8, 8, 50, 0),
    (188, 8, 204, 204, 1, 0), (188, 8, 204, 204, 4099, 0), (188, 8, 0, 0, 4099, 3)]


@pytest.mark.parametrize("n,G,ip,op,R,offset", SHAPES)
def test_dispersal_rows_pitches_groups_in_place_and_indices_outside_the_group(n, G, ip, op, R, offset):
    rng = np.random.default_rng(n * 100 + G + R + ip)
    x = rng.integers(0, 256, (R, n), dtype=np.uint8)
    m = modem()
    for msb in (False, True):
        run_dispersal(m, x, G, first=int(rng.integers(0, G)), msb=msb, ip=ip, op=op, offset=offset)
        index = rng.integers(0, 16, R)                        # whatever a byte's high half can hold: >= group in some rows
        index[0] = 15 if G < 16 else 0
        run_dispersal(m, x, G, index=index, msb=msb, ip=ip, op=op, offset=offset, rng=rng)
        if (ip or n) == (op or n):
            run_dispersal(m, x, G, first=int(rng.integers(0, G)), msb=msb, ip=ip, op=op, inplace=True, offset=offset)
            run_dispersal(m, x, G, index=index, msb=msb, ip=ip, op=op, inplace=True, offset=offset, rng=rng)
    m.sync()
    m.close()


def test_dispersal_through_the_modem_is_an_involution_takes_strided_rows_and_refuses_on_a_context():
    import torch
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, (21, 204), dtype=np.uint8)
    m = modem()
    d = torch.from_numpy(x).cuda()
    y = m.dispersal(d[:, :188], group=8, first=3, msb_first=True)              # rows 204 bytes apart, as qpsk_rs_decode_batch leaves them
    assert np.array_equal(y.cpu().numpy(), dispersal_ref(x[:, :188], 8, (3 + np.arange(21)) % 8, True))
    back = m.dispersal(y, group=8, first=3, msb_first=True, pitch=207)
    assert back.stride(0) == 207 and np.array_equal(back.cpu().numpy(), x[:, :188])
    flags = ((np.arange(21) % 11) << 4).astype(np.uint8)
    z = m.dispersal(x[:, :188], group=8, flags=flags)
    assert np.array_equal(z.cpu().numpy(), dispersal_ref(x[:, :188], 8, np.arange(21) % 11, False))
    # the refusals once more on a context: nothing is launched
    for bad in ((ptr(d), 187, 21, 188, 8, 0, None, 0, ptr(y), 0), (ptr(d), 0, 21, 188, 17, 0, None, 0, ptr(y), 0),
                (ptr(d), 0, 21, 188, 8, 0, ptr(y), 1, ptr(back), 0), (ptr(d), 204, 21, 188, 8, 0, None, 0, C.c_void_p(d.data_ptr() + 1), 204),
                (ptr(d), 204, 21, 188, 8, 0, None, 0, ptr(d), 188)):
        assert m.L.qpsk_dispersal_batch(m.h, *bad) == -2, bad
        assert b"qpsk_dispersal_batch" in m.L.qpsk_last_error()
    m.sync()
    m.close()


def test_dispersal_buffers_that_touch_are_accepted_and_descramble_as_ever():
    """3 rows of 188 at pitch 204 inside one allocation: a buffer is 2 * 204 + 188 = 596 bytes, the 16 bytes of padding behind its last row
    are not part of it.  d_out and the 3 bytes of d_flags in front of and behind the input and each other, touching: accepted, and every
    row is the reference's.  One byte further in the call is refused (test_dvb_cpu.py has the rows; two of them once more on a context)"""
    import torch
    rng = np.random.default_rng(204)
    R, n, P, G = 3, 188, 204, 8
    x = rng.integers(0, 256, (R, n), dtype=np.uint8)
    idx = np.array([7, 0, 3])
    m = modem()
    arena = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    at = lambda off: None if off is None else C.c_void_p(arena.data_ptr() + off)      # noqa: E731

    def run(i=1000, o=2000, f=None):
        host = np.full(4096, 0x55, np.uint8)
        for r in range(R):
            host[i + r * P:i + r * P + n] = x[r]
        if f is not None:
            host[f:f + R] = (idx << 4) | 5
        arena.copy_(torch.from_numpy(host))
        rc = m.L.qpsk_dispersal_batch(m.h, at(i), P, R, n, G, 0, at(f), 0, at(o), P)
        torch.cuda.synchronize()
        if rc == 0:
            got = arena.cpu().numpy()
            want = dispersal_ref(x, G, np.arange(R) % G if f is None else idx, False)
            assert np.array_equal(np.stack([got[o + r * P:o + r * P + n] for r in range(R)]), want), (i, o, f)
        return rc
    for kw in (dict(o=1596), dict(o=404), dict(f=1596), dict(f=997), dict(f=2596), dict(f=1997), dict(o=1000), dict(o=1000, f=1596)):
        assert run(**kw) == 0, (kw, m.L.qpsk_last_error())
    for kw, text in ((dict(o=1595), b"d_out overlaps d_in"), (dict(o=405), b"d_out overlaps d_in"), (dict(f=1595), b"d_flags overlaps d_in"),
                     (dict(f=998), b"d_flags overlaps d_in"), (dict(f=2595), b"d_flags overlaps d_out"), (dict(f=1998), b"d_flags overlaps d_out")):
        assert run(**kw) == -2 and b"qpsk_dispersal_batch: " + text in m.L.qpsk_last_error(), (kw, m.L.qpsk_last_error())
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 4. the link at DVB-S's own parameters
def test_the_dvb_link_with_the_library_s_calls():
    """test_dvb_cpu's link: dispersal -> rs_encode (204, 188) -> outer_interleave (12) -> conv_encode_stream at rate 3/4 -> the half turn and
    the burst -> viterbi_stream (128, 256) -> outer with group 8, lock 8 -> rs_decode -> dispersal with the outer link's flags; every stage
    equal to its restatement, every packet that comes out equal to the packet that went in"""
    import torch
    r, p = dvb_link_result(), DVB
    S, n, k, G, I = p["S"], p["n"], p["k"], p["G"], p["I"]
    m = modem()
    randomised = torch.stack([m.dispersal(r["packets"][i], group=G, first=p["first"][i], msb_first=True) for i in range(S)])
    assert np.array_equal(randomised.cpu().numpy(), r["randomised"])
    sent = m.rs_encode(randomised.reshape(-1, k), n - k)
    assert np.array_equal(sent.cpu().numpy().reshape(S, -1, n), r["sent"])
    y, _ = m.outer_interleave(sent.contiguous().reshape(S, -1, n), I)
    assert np.array_equal(y.cpu().numpy(), r["interleaved"])
    # bytes go out high bit first; the encoder takes a row's first bit in bit 0 of its first byte
    tx = pack_bits(bytes_to_bits(y.cpu().numpy().reshape(S, -1), True))
    dibits, _ = m.conv_encode_stream(tx, 8 * tx.shape[1], puncture="3/4")
    assert np.array_equal(dibits.cpu().numpy(), r["dibits"])
    soft = torch.from_numpy(r["soft"]).cuda()
    m.viterbi_stream_reset(S, p["depth"], p["window"], puncture="3/4")
    m.outer_reset(S, n, I, 0x47, p["L"], p["drop"], polarity=True, msb_first=True, group=G)
    vouts = [m.viterbi_stream(soft[:, a:b].contiguous()) for a, b in zip(r["cuts"][:-1], r["cuts"][1:])] + [m.viterbi_stream_flush()]
    ocalls = iter(r["ocalls"])
    done = [0] * S
    for v, want_v in zip(vouts, r["vcalls"]):
        assert v["nbits"] == want_v["nbits"] and np.array_equal(v["bits"].cpu().numpy(), want_v["bits"])
        assert np.array_equal(v["info"].cpu().numpy(), want_v["info"])
        if not v["nbits"]:
            continue
        o, want = m.outer(v), next(ocalls)
        assert m.last_kernel() == "outer_push_kernel"
        count = o["count"].cpu().numpy()
        assert np.array_equal(count, want["count"]) and np.array_equal(o["info"].cpu().numpy(), want["info"])
        mw = o["words"].shape[1]
        assert count.max() <= mw
        decoded, info = m.rs_decode(o["words"].reshape(S * mw, n), n - k)      # every slot, written or not
        out = m.dispersal(decoded[:, :k], group=G, flags=o["flags"], msb_first=True)
        assert m.last_kernel() == "dispersal_kernel"
        h = {key: t.cpu().numpy() for key, t in (("words", o["words"]), ("pos", o["pos"]), ("flags", o["flags"]))}
        h["decoded"], h["info"], h["out"] = decoded.cpu().numpy().reshape(S, mw, n), info.cpu().numpy().reshape(S, mw, 4), out.cpu().numpy().reshape(S, mw, k)
        for i in range(S):
            c, a = int(count[i]), done[i]
            for key in ("words", "pos", "flags"):
                assert np.array_equal(h[key][i, :c], want[key][i]), (key, i)
            assert np.array_equal(h["decoded"][i, :c], r["decoded"][i][a:a + c]) and np.array_equal(h["info"][i, :c], r["info"][i][a:a + c])
            assert np.array_equal(h["out"][i, :c], r["out"][i][a:a + c])
            w0 = int(r["pos"][i][0]) // (8 * n) - (I - 1)
            assert np.array_equal(h["out"][i, :c], r["packets"][i, w0 + a:w0 + a + c]) and (h["out"][i, :c, 0] == 0x47).all()
            assert (((h["flags"][i, :c] & 2) != 0) == (i == 1)).all()      # s = -1 on the turned stream
            done[i] += c
    assert done == [len(x) for x in r["out"]] and min(done) >= p["npackets"] - (I - 1) - 2
    m.sync()
    m.close()
