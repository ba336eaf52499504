"""qpsk_frame_batch on the GPU against frame_ref (test_frame_cpu.py), which restates FRAMER of include/qpsk_hip.h: bit for bit with guard
bytes round every buffer, against the composition of the existing calls, through the three deframers on the device, and through the whole
chain payload -> PCM -> receive streams -> packets against the CPU oracle.  Everything is an equality; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_cpu import cut
from test_frame_cpu import (HALF, LINK, LINK_CODINGS, body_len, frame_ref, ks_prefix, link_deframe, link_receive, link_shape, starts)
from test_punct_cpu import BAD_PATTERNS, NAMED, PERIOD32, punct_nsent

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG = -2
UNCODED, CODED = 0, 1
GUARD = 0xEE


@pytest.fixture(scope="module")
def m():
    import qpsk_amd
    from oracle.pyoracle import TIMING_FIXED
    k = LINK
    md = qpsk_amd.Modem(fs=k["fs"], rs=k["rs"], frame_size=k["L"], timing_mode=TIMING_FIXED, fixed_index=126 % int(k["fs"] / k["rs"]))
    yield md
    md.close()


def code_args(coded, pattern):
    return (CODED if coded else UNCODED,) + tuple(HALF if pattern is None else pattern)


def frame_guarded(m, payloads, sync, coded, pattern, per_row, lead, gap, row_len, pitch=0, front=64, want_crc=True):
    """qpsk_frame_batch through the raw ABI on buffers with guard bytes in front of and behind d_out and d_crc, and payload rows `pitch`
    bytes apart in a buffer of guard bytes.  Asserts that nothing but the outputs was written -> (dibits (nrows, row_len), crc or None)"""
    import torch
    payloads = np.asarray(payloads, np.uint8)
    npk, nbytes = payloads.shape
    nrows = npk // per_row
    step = pitch or nbytes
    src = np.full(front + (npk - 1) * step + nbytes + 64, GUARD, np.uint8)
    for k in range(npk):
        src[front + k * step:front + k * step + nbytes] = payloads[k]
    d_src = torch.from_numpy(src).cuda()
    d_out = torch.full((front + nrows * row_len + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_crc = torch.full((8 + npk + 8,), 0x5EEE, dtype=torch.int16, device="cuda")
    sw = np.ascontiguousarray(np.asarray(sync, np.uint8))
    rc = m.L.qpsk_frame_batch(m.h, C.c_void_p(d_src.data_ptr() + front), pitch, nrows, per_row, nbytes, sw.ctypes.data_as(C.c_void_p), len(sw),
                              *code_args(coded, pattern), lead, gap, row_len, C.c_void_p(d_out.data_ptr() + front),
                              C.c_void_p(d_crc.data_ptr() + 16) if want_crc else None)
    assert rc == 0, m.L.qpsk_last_error()
    m.sync()
    assert m.last_kernel() == ("frame_kernel<coded>" if coded else "frame_kernel<uncoded>")
    out, crc = d_out.cpu().numpy(), d_crc.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), src), "the payload buffer was written"
    assert (out[:front] == GUARD).all() and (out[front + nrows * row_len:] == GUARD).all(), "d_out's guard bytes were written"
    assert (crc[:8] == 0x5EEE).all() and (crc[8 + (npk if want_crc else 0):] == 0x5EEE).all(), "d_crc's guard words were written"
    return out[front:front + nrows * row_len].reshape(nrows, row_len), crc[8:8 + npk].view(np.uint16) if want_crc else None


def exact_fit(nsync, nbytes, coded, pattern, per_row, lead, gap):
    return starts(nsync, nbytes, coded, pattern, per_row, lead, gap)[-1] + nsync + body_len(nbytes, coded, HALF if pattern is None else pattern)


def check_case(m, seed, nsync, nbytes, coded, pattern, nrows, per_row, lead, gap, extra, pitch=0, front=64):
    rng = np.random.default_rng(seed)
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    payloads = rng.integers(0, 256, (nrows * per_row, nbytes), dtype=np.uint8)
    row_len = exact_fit(nsync, nbytes, coded, pattern, per_row, lead, gap) + extra
    want, want_crc = frame_ref(payloads, sync, coded, pattern, per_row, lead, gap, row_len)
    got, got_crc = frame_guarded(m, payloads, sync, coded, pattern, per_row, lead, gap, row_len, pitch, front)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d dibits differ, first at (row, column) %s: %d for %d" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(got_crc, want_crc)


# ------------------------------------------------------------------- 1. bit for bit against frame_ref
@pytest.mark.parametrize("coding", ["uncoded", "1/2", "7/8"])
@pytest.mark.parametrize("nbytes", [1, 63, 64, 65, 1024])
def test_payload_sizes_round_the_crc_chunk_steps_and_the_largest(m, nbytes, coding):
    """nbytes 1: fewer bytes than lanes; 63, 64, 65: the CRC chunk per lane steps from 1 to 2; 1024: the largest packet (the LDS slice and
    the factor table's end).  Five packets: the second workgroup is partly filled"""
    coded, pattern = coding != "uncoded", NAMED.get(coding)
    check_case(m, nbytes, 16, nbytes, coded, pattern, nrows=5, per_row=1, lead=nbytes % 4, gap=0, extra=0)
    check_case(m, nbytes + 1, 16, nbytes, coded, pattern, nrows=1, per_row=5, lead=1, gap=3, extra=9, pitch=nbytes + 3)


@pytest.mark.parametrize("coded", [False, True])
@pytest.mark.parametrize("nsync", [1, 128])
def test_shortest_and_longest_sync_word(m, nsync, coded):
    check_case(m, nsync, nsync, 5, coded, None, nrows=2, per_row=3, lead=2, gap=0, extra=9)
    check_case(m, nsync + 1, nsync, 16, coded, None, nrows=5, per_row=1, lead=0, gap=0, extra=0, pitch=19)


def test_odd_nsent_sends_a_zero_pad_bit(m):
    """nbytes 5 at rate 2/3: 62 steps, nsent = 93, the last dibit of a body carries one coded bit and the pad"""
    assert punct_nsent(62, NAMED["2/3"]) == 93 and body_len(5, True, NAMED["2/3"]) == 47
    for gap in (0, 5):
        check_case(m, 93 + gap, 24, 5, True, NAMED["2/3"], nrows=2, per_row=3, lead=1, gap=gap, extra=0)


@pytest.mark.parametrize("coded", [False, True])
@pytest.mark.parametrize("front", [64, 61])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_alignment_of_a_packet_s_start_and_end(m, lead, front, coded):
    """the byte-wise head and tail round the dword stores: start columns 0..3 mod 4 (P = 44 or 78 and gap 1 move the later packets of a row
    on), d_out itself 4-byte aligned and not (front 61), rows of the exact fit and of the exact fit + 9, payload rows nbytes + 3 bytes apart"""
    for extra in (0, 9):
        for per_row, gap in ((1, 0), (3, 0), (3, 1)):
            check_case(m, 16 * lead + extra + per_row + gap, 16, 5, coded, None, nrows=3, per_row=per_row, lead=lead, gap=gap, extra=extra,
                       pitch=8, front=front)


@pytest.mark.parametrize("name", sorted(NAMED) + ["period32"])
def test_every_named_rate_and_a_period_32_pattern(m, name):
    pattern = PERIOD32 if name == "period32" else NAMED[name]
    check_case(m, len(name) + pattern[0], 32, 16, True, pattern, nrows=2, per_row=3, lead=5, gap=7, extra=9, pitch=19)
    check_case(m, len(name) + pattern[0] + 1, 32, 5, True, pattern, nrows=5, per_row=1, lead=0, gap=0, extra=0)


def test_modem_frame_takes_both_payload_shapes_and_may_leave_the_crc_out(m):
    rng = np.random.default_rng(5)
    sync = rng.integers(0, 4, 20, dtype=np.uint8)
    payloads = rng.integers(0, 256, (2, 3, 7), dtype=np.uint8)
    want, want_crc = frame_ref(payloads.reshape(6, 7), sync, True, NAMED["3/4"], 3, 4, 2, None)
    for p in (payloads, payloads.reshape(6, 7)):
        o = m.frame(p, sync, puncture="3/4", per_row=3, lead=4, gap=2)
        assert np.array_equal(o["dibits"].cpu().numpy(), want) and np.array_equal(o["crc"].cpu().numpy().view(np.uint16), want_crc)
    got, none = frame_guarded(m, payloads.reshape(6, 7), sync, True, NAMED["3/4"], 3, 4, 2, want.shape[1], want_crc=False)
    assert np.array_equal(got, want) and none is None
    o = m.frame(payloads, sync, coded=False, per_row=3, row_len=200)
    assert np.array_equal(o["dibits"].cpu().numpy(), frame_ref(payloads.reshape(6, 7), sync, False, None, 3, 0, 0, 200)[0])


# ------------------------------------------------------------------- 2. the composition of the existing calls, GPU against GPU
@pytest.mark.parametrize("coded", [True, False])
def test_frame_equals_the_composition_of_the_existing_calls(m, coded):
    """crc16 -> append big-endian -> conv_encode with the tail (uncoded: qpsk_pack_symbols' packing in reverse) -> scramble -> the sync word
    in front: the five launches and the glue the framer replaces"""
    import torch
    rng = np.random.default_rng(21)
    nbytes, sync = 37, rng.integers(0, 4, 24, dtype=np.uint8)
    payloads = torch.from_numpy(rng.integers(0, 256, (9, nbytes), dtype=np.uint8)).cuda()
    crc = torch.from_numpy(m.crc16(payloads).astype(np.int32)).cuda()
    pkt = torch.cat([payloads, (crc >> 8).to(torch.uint8)[:, None], (crc & 255).to(torch.uint8)[:, None]], dim=1)
    if coded:
        body = m.conv_encode(pkt, 8 * (nbytes + 2), tail=True)
    else:
        shifts = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device="cuda")
        body = ((pkt.to(torch.int32)[:, :, None] >> shifts) & 3).to(torch.uint8).reshape(9, -1)
    rows = torch.cat([torch.from_numpy(sync).cuda()[None, :].expand(9, -1), m.scramble(body)], dim=1)
    o = m.frame(payloads, sync, coded=coded)
    m.sync()
    assert torch.equal(o["dibits"], rows) and torch.equal(o["crc"].to(torch.int32) & 0xFFFF, crc)


# ------------------------------------------------------------------- 3. round trips on the device
STREAMS, PER_ROW = 3, 3


def costas_of(torch, dibits, amp=0.7):
    """dibits on the diagonals, on the device (test_deframe_coded_cpu.dibits_to_costas with q = 0 and no noise)"""
    d = dibits.to(torch.int32)
    return torch.stack([amp * (1.0 - 2.0 * (d & 1).to(torch.float32)), amp * (1.0 - 2.0 * (d >> 1).to(torch.float32))], dim=-1).contiguous()


def pushes_of(total):
    sizes = cut(np.arange(total), [1, 7, 64])
    return [len(s) for s in sizes]


@pytest.mark.parametrize("nbytes", [5, 16])
@pytest.mark.parametrize("coding", ["uncoded", "1/2", "3/4"])
def test_frame_through_the_deframers_on_the_device(m, coding, nbytes):
    """3 streams x 3 packets, rows cut into pushes of 1, 7 and 64 symbols and the rest: every count, position, payload and crc_ok as planted"""
    import torch
    coded, pattern = coding != "uncoded", NAMED["3/4"] if coding == "3/4" else None
    rng = np.random.default_rng(300 + nbytes)
    nsync, lead, gap = 24, 5, 7
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    payloads = rng.integers(0, 256, (STREAMS, PER_ROW, nbytes), dtype=np.uint8)
    at = starts(nsync, nbytes, coded, pattern, PER_ROW, lead, gap)
    row_len = exact_fit(nsync, nbytes, coded, pattern, PER_ROW, lead, gap) + 9
    o = m.frame(payloads, sync, coded=coded, puncture=pattern, per_row=PER_ROW, lead=lead, gap=gap, row_len=row_len)
    rows = o["dibits"]
    if coded:
        m.deframer_reset_coded(STREAMS, sync, nbytes, nsync, max_packets=4, puncture=pattern)
        z = costas_of(torch, rows)
        gain = torch.full((STREAMS,), 90.0, dtype=torch.float32, device="cuda")
    else:
        m.deframer_reset(STREAMS, sync, nbytes, nsync, max_packets=4)
    got = [[] for _ in range(STREAMS)]
    a = 0
    for n in pushes_of(row_len):
        r = m.deframe_coded(z[:, a:a + n].contiguous(), gain) if coded else m.deframe(data=rows[:, a:a + n].contiguous())
        a += n
        h = {k: r[k].cpu().numpy() for k in ("count", "pos", "rot", "bytes", "crc_ok")}
        for s in range(STREAMS):
            got[s] += [(int(h["pos"][s, j]), int(h["rot"][s, j]), h["bytes"][s, j].tobytes(), bool(h["crc_ok"][s, j])) for j in range(h["count"][s])]
    m.sync()
    crc = o["crc"].cpu().numpy().view(np.uint16).reshape(STREAMS, PER_ROW)
    for s in range(STREAMS):
        want = [(at[j], 0, payloads[s, j].tobytes() + bytes([int(crc[s, j]) >> 8, int(crc[s, j]) & 255]), True) for j in range(PER_ROW)]
        assert got[s] == want, s


# ------------------------------------------------------------------- 4. the whole chain on the device
@pytest.mark.parametrize("coding", sorted(LINK_CODINGS))
def test_payload_to_pcm_to_packets_on_the_device_equals_the_oracle(m, oracle, coding):
    """test_frame_cpu's noise-free link with 2 streams, every stage on the device: frame -> tx_symbols (PCM) -> streams_rx_pcm block by
    block -> the deframer of the coding.  The PCM, every block's costas_frame[] and the packet records equal the CPU oracle's for the same
    rows bit for bit, and every packet comes back crc_ok with its payload at column + 159"""
    k = LINK
    S = 2
    shape = link_shape(coding, nstreams=S)
    coded, pattern = shape["coded"], shape["pattern"]
    o = m.frame(shape["payloads"], shape["sync"], coded=coded, puncture=pattern, per_row=k["per_row"], lead=k["lead"], gap=k["gap"],
                row_len=shape["row_len"])
    rows = o["dibits"].cpu().numpy()
    assert np.array_equal(rows, frame_ref(shape["payloads"], shape["sync"], coded, pattern, k["per_row"], k["lead"], k["gap"], shape["row_len"])[0])
    m.tx_reset(S, k["tx_hz"])
    pcm = m.tx_symbols(o["dibits"])["pcm"]
    m.streams_reset(S, k["mixer_hz"])
    if coded:
        m.deframer_reset_coded(S, shape["sync"], k["nbytes"], k["min_score"], max_packets=4, puncture=pattern)
    else:
        m.deframer_reset(S, shape["sync"], k["nbytes"], k["min_score"], max_packets=4)
    L, nblocks = k["L"], shape["row_len"] // shape["nsym"]
    blocks, got = [], [[] for _ in range(S)]
    for b in range(nblocks):
        rx = m.streams_rx_pcm(pcm[:, b * L:(b + 1) * L].contiguous(), want_costas=True)
        r = m.deframe_coded(rx) if coded else m.deframe(costas=rx)
        blocks.append(rx["costas"].cpu().numpy())
        h = {key: r[key].cpu().numpy() for key in ("count", "pos", "rot", "score", "bytes", "crc_ok")}
        for s in range(S):
            got[s] += [(int(h["pos"][s, j]), int(h["rot"][s, j]), int(h["score"][s, j]), h["bytes"][s, j].tobytes(), bool(h["crc_ok"][s, j]))
                       for j in range(h["count"][s])]
    m.sync()
    pcm = pcm.cpu().numpy()
    for s in range(S):
        want_pcm, want_blocks = link_receive(oracle, rows[s])
        assert np.array_equal(pcm[s], want_pcm), s
        for b in range(nblocks):
            assert np.array_equal(blocks[b][s].view(np.uint32), want_blocks[b].view(np.uint32)), (s, b)
        want = [(p["pos"], p["rot"], p["score"], p["bytes"].tobytes(), p["crc_ok"]) for p in link_deframe(shape, want_blocks)]
        assert got[s] == want, s
        assert [g[0] for g in got[s]] == [c + 159 for c in shape["at"]]
        for g, payload in zip(got[s], shape["payloads"][s * k["per_row"]:(s + 1) * k["per_row"]]):
            assert g[4] and g[3][:k["nbytes"]] == payload.tobytes()


# ------------------------------------------------------------------- 5. the error contract
def test_bad_arguments_are_refused_and_leave_the_output_alone(m):
    import torch
    rng = np.random.default_rng(9)
    sync = np.ascontiguousarray(rng.integers(0, 4, 128, dtype=np.uint8))
    src = torch.from_numpy(rng.integers(0, 256, 70000, dtype=np.uint8)).cuda()
    out = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    crc = torch.full((64,), 0x5EEE, dtype=torch.int16, device="cuda")
    p, q, w, sw = src.data_ptr(), out.data_ptr(), crc.data_ptr(), sync.ctypes.data
    good = dict(payload=p, pitch=0, nrows=2, per_row=3, nbytes=5, sync=sw, nsync=16, coding=CODED, pattern=HALF, lead=3, gap=2, row_len=300,
                out=q, crc=w)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda v: C.c_void_p(v) if v else None      # noqa: E731
        return m.L.qpsk_frame_batch(m.h, ptr(a["payload"]), a["pitch"], a["nrows"], a["per_row"], a["nbytes"], ptr(a["sync"]), a["nsync"], a["coding"],
                                    *a["pattern"], a["lead"], a["gap"], a["row_len"], ptr(a["out"]), ptr(a["crc"]))

    P = 16 + 62
    assert 3 + 3 * P + 2 * 2 == 241
    bad = [dict(nsync=0), dict(nsync=129), dict(nbytes=0), dict(nbytes=1025), dict(nrows=0), dict(nrows=-1), dict(per_row=0), dict(per_row=65),
           dict(nrows=40000000, per_row=64), dict(lead=-1), dict(gap=-1), dict(row_len=240), dict(row_len=0), dict(row_len=(1 << 21) + 1),
           dict(lead=63), dict(gap=32), dict(pitch=4), dict(pitch=-8), dict(coding=2), dict(coding=-1),
           dict(payload=0), dict(sync=0), dict(out=0),
           dict(payload=q + 100), dict(payload=q - 20), dict(crc=q + 8), dict(crc=p + 2), dict(crc=w + 1)]
    bad += [dict(pattern=b) for b in BAD_PATTERNS]
    for kw in bad:
        assert call(**kw) == QPSK_ERR_ARG, kw
        assert b"qpsk_frame_batch" in m.L.qpsk_last_error(), kw
    m.sync()
    assert (out.cpu().numpy() == GUARD).all() and (crc.cpu().numpy() == 0x5EEE).all()
    # the same arguments are fine as they stand, at the exact fit too, and a bad pattern does not matter to an uncoded body
    assert call() == 0 and call(row_len=241) == 0 and m.last_kernel() == "frame_kernel<coded>"
    for b in BAD_PATTERNS:
        assert call(coding=UNCODED, pattern=b) == 0, b
    assert m.last_kernel() == "frame_kernel<uncoded>"
    m.sync()
    payloads = src.cpu().numpy()[:30].reshape(6, 5)
    assert np.array_equal(out.cpu().numpy()[:600].reshape(2, 300), frame_ref(payloads, sync[:16], False, None, 3, 3, 2, 300)[0])
    assert (out.cpu().numpy()[600:] == GUARD).all()
    # all three buffers inside `out`: 6 payloads of 5 bytes at pitch 8 span 5 * 8 + 5 = 45 bytes (the padding behind the last one is not the
    # buffer), d_out 600, d_crc 12.  Touching on either side is accepted and frames as ever; one byte shared (d_crc is 2-byte aligned: two) is not
    want, want_crc = frame_ref(payloads, sync[:16], False, None, 3, 3, 2, 300)
    crc_text = b"d_crc is not 2-byte aligned, or overlaps d_payload or d_out"
    for kw, text in ((dict(out=q + 1045), None), (dict(out=q + 400), None), (dict(out=q + 1044), b"d_out overlaps d_payload"),
                     (dict(out=q + 401), b"d_out overlaps d_payload"), (dict(crc=q + 988), None), (dict(crc=q + 990), crc_text),
                     (dict(payload=q + 1001, crc=q + 1046), None), (dict(payload=q + 1001, crc=q + 1044), crc_text), (dict(crc=q + 1988), None),
                     (dict(crc=q + 1990), crc_text), (dict(crc=q + 2600), None), (dict(crc=q + 2598), crc_text), (dict(crc=0), None)):
        a = dict(dict(payload=q + 1000, pitch=8, out=q + 2000, crc=q + 3000, coding=UNCODED), **kw)
        host = np.full(4096, GUARD, np.uint8)
        at = a["payload"] - q
        for i in range(6):
            host[at + 8 * i:at + 8 * i + 5] = payloads[i]
        out.copy_(torch.from_numpy(host))
        rc = call(**a)
        if text:
            assert rc == QPSK_ERR_ARG and b"qpsk_frame_batch: " + text in m.L.qpsk_last_error(), (kw, rc, m.L.qpsk_last_error())
            continue
        assert rc == 0, (kw, m.L.qpsk_last_error())
        m.sync()
        host = out.cpu().numpy()
        assert np.array_equal(host[a["out"] - q:a["out"] - q + 600].reshape(2, 300), want), kw
        assert not a["crc"] or np.array_equal(host[a["crc"] - q:a["crc"] - q + 12].view(np.uint16), want_crc), kw
        assert all(np.array_equal(host[at + 8 * i:at + 8 * i + 5], payloads[i]) for i in range(6)), kw


def test_a_framer_call_disturbs_neither_a_deframer_nor_the_receive_streams_nor_the_scrambler(m):
    """two contexts run the same pushes and stream blocks; one of them frames packets (growing its keystream table on the way) in between"""
    import qpsk_amd
    import torch
    from oracle.pyoracle import TIMING_FIXED
    k = LINK
    rng = np.random.default_rng(77)
    b = qpsk_amd.Modem(fs=k["fs"], rs=k["rs"], frame_size=k["L"], timing_mode=TIMING_FIXED, fixed_index=2)
    sync = rng.integers(0, 4, 16, dtype=np.uint8)
    payloads = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    rows = m.frame(payloads, sync, per_row=2, lead=9, gap=30, row_len=400)["dibits"]
    z = costas_of(torch, rows)
    pcm = torch.from_numpy((5000 * rng.standard_normal((3, 2, k["L"]))).astype(np.int16)).cuda()
    sym = torch.from_numpy(rng.integers(0, 4, (3, 50), dtype=np.uint8)).cuda()
    outs = []
    for md, framing in ((m, True), (b, False)):
        md.streams_reset(2, k["mixer_hz"])
        md.deframer_reset_coded(2, sync, 8, 16, max_packets=4)
        got = [md.scramble(sym)]
        for i, (lo, hi) in enumerate(((0, 90), (90, 250), (250, 400))):
            got.append(md.deframe_coded(z[:, lo:hi].contiguous()))
            got.append(md.streams_rx_pcm(pcm[i], want_costas=True))
            if framing:
                md.frame(payloads, sync, coded=bool(i & 1), per_row=1, row_len=9000 + 3000 * i)
        got.append(md.scramble(sym))
        md.sync()
        outs.append(got)
    assert len(outs[0]) == len(outs[1]) == 8
    for ga, gb in zip(*outs):
        if not isinstance(ga, dict):
            assert torch.equal(ga, gb)
            continue
        for key in ga:
            if key != "_keep" and ga[key] is not None:
                assert np.array_equal(ga[key].cpu().numpy().view(np.uint8), gb[key].cpu().numpy().view(np.uint8)), key
    assert sum(int(g["count"].sum()) for g in outs[0] if isinstance(g, dict) and "count" in g) == 4
    assert np.array_equal(outs[0][0].cpu().numpy(), sym.cpu().numpy() ^ ks_prefix(50))
    b.close()
