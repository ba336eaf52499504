"""qpsk_viterbi_ilv_batch / qpsk_conv_encode_ilv_batch / qpsk_frame_batch_ilv / qpsk_deframer_reset_coded_ilv and interleave= of the Modem
calls on the GPU, bit for bit against the numpy restatements of test_ilv_cpu.py (INTERLEAVING of include/qpsk_hip.h): both routes of
the decoder, the chunks, the 32-bit edge of the modular product, the two identities the header states, the encoder, the framer, the
stream deframer, a burst on the device, and the error contract.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_cpu import dibits_to_costas
from test_deframe_coded_gpu import hunt_set_on_the_device, push_all, rec, rows_of
from test_deframe_cpu import hunt_coded_sets
from test_frame_cpu import HALF, body_len, frame_ref, starts
from test_ilv_cpu import (deframe_coded_ilv_ref, frame_ilv_ref, gather_ref, ilv_stream, ilv_stride, interleave_ref, strides_for,
                          viterbi_ilv_ref)
from test_punct_cpu import ALL_FLAGS, DELETED_STEP, NAMED, PERIOD32, coded_punct_steps, depuncture_ref, punct_nsent, punct_ntx, puncture_ref
from test_punct_gpu import run as run_punct
from test_viterbi_cpu import OPEN_END, conv_encode_ref, viterbi_ref
from test_viterbi_gpu import GUARD, assert_equal, modem, ptr, random_soft

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG, QPSK_ERR_STATE = -2, -5
LDS_ROUTE, SCRATCH_ROUTE = "viterbi_ilv_lds_kernel", "viterbi_ilv_kernel"
PATTERNS = {"1/2": NAMED["1/2"], "3/4": NAMED["3/4"], "7/8": NAMED["7/8"], "deleted": DELETED_STEP, "period32": PERIOD32}
FRAME_GUARD = 0xEE


def run(m, soft, nsteps, pattern, stride, flip=None, flags=0, pitch=0, route=None):
    """the raw call with guarded outputs; soft: numpy (R, ntx or pitch, 2) int8 as on air"""
    import torch
    q = torch.from_numpy(np.ascontiguousarray(soft, np.int8)).cuda()
    R, nb = q.shape[0], (nsteps + 7) // 8
    f = None if flip is None else torch.from_numpy(np.ascontiguousarray(flip, np.uint8)).cuda()
    bits = torch.full((R * nb + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    info = torch.full((R * 4 + GUARD,), 0x55555555, dtype=torch.int32, device="cuda")
    m.tune(viterbi_lds=route)
    m._check(m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), pitch, R, nsteps, *pattern, stride, ptr(f), flags, ptr(bits), ptr(info)))
    kernel = m.last_kernel()
    torch.cuda.synchronize()
    hb, hi = bits.cpu().numpy(), info.cpu().numpy()
    assert np.all(hb[R * nb:] == 0x55) and np.all(hi[R * 4:] == 0x55555555), "a guard behind an output was overwritten"
    return {"kernel": kernel, "bits": hb[:R * nb].reshape(R, nb), "info": hi[:R * 4].reshape(R, 4)}


def on_air(R, nsteps, pattern, seed):
    """random soft rows as on air, (R, ntx, 2), with a -128 and a 0 in every row (wherever they land: every on-air number but the pad's
    is read)"""
    soft = random_soft(R, punct_ntx(nsteps, pattern), seed)
    flat = soft.reshape(R, -1)
    flat[:, 0] = -128
    flat[:, flat.shape[1] // 2] = 0
    return soft


def ref_row(soft, nsteps, pattern, stride, flip):
    """what the decoder sees: the zero-filled rate-1/2 row of viterbi_ilv_ref, so that many cases share one viterbi_ref call"""
    ntx = punct_ntx(nsteps, pattern)
    rows, key = gather_ref(np.maximum(soft, -127), ntx, stride, flip)
    return depuncture_ref(rows, nsteps, pattern, key)


# ------------------------------------------------------------------------------------------ 1. random rows, every shape, both routes
@pytest.mark.parametrize("n", [1, 6, 63, 64, 65, 150, 262])
def test_random_rows_bit_for_bit_on_both_routes(n):
    """every pattern, stride, flip and flag value on 3 rows, and 70 pitched rows with poisoned bytes between them; the references of one
    length are computed in one viterbi_ref call per flag value (its rows are independent).  ref_row is checked against viterbi_ilv_ref,
    the definition, on the first case"""
    m = modem()
    cases, rows = [], []
    for name, pattern in sorted(PATTERNS.items()):
        ntx = punct_ntx(n, pattern)
        assert ntx >= 1
        soft = on_air(3, n, pattern, 10 * n + len(name))
        key = np.random.default_rng(n).integers(0, 4, ntx).astype(np.uint8)
        for s in strides_for(2 * ntx):
            for flip in (None, key):
                cases.append((name, pattern, s, soft, flip, 0))
                rows.append(ref_row(soft, n, pattern, s, flip))
    pattern = PATTERNS["3/4"]
    ntx = punct_ntx(n, pattern)
    big, s = on_air(70, n, pattern, n), strides_for(2 * ntx)[-1]
    key = np.random.default_rng(n + 1).integers(0, 4, ntx).astype(np.uint8)
    cases.append(("70 rows", pattern, s, big, key, ntx + 3))
    rows.append(ref_row(big, n, pattern, s, key))
    first = viterbi_ilv_ref(cases[1][3], n, cases[1][1], cases[1][2], flip=cases[1][4], flags=OPEN_END)
    for flags in ALL_FLAGS:
        ref = viterbi_ref(np.concatenate(rows), flags=flags)
        if flags == OPEN_END:
            assert np.array_equal(ref["bits"][3:6], first["bits"]) and np.array_equal(ref["info"][3:6], first["info"])
        at = 0
        for name, pattern, s, soft, flip, pitch in cases:
            R = soft.shape[0]
            want = {k: ref[k][at:at + R] for k in ("bits", "info")}
            at += R
            buf = soft
            if pitch:
                buf = np.full((R, pitch, 2), -0x80 if flags & 1 else 0x7F, np.int8)      # poison between the rows
                buf[:, :soft.shape[1]] = soft
            for route, kernel in ((0, SCRATCH_ROUTE), (1, LDS_ROUTE)):
                got = run(m, buf, n, pattern, s, flip=flip, flags=flags, pitch=pitch, route=route)
                assert got["kernel"] == kernel, (route, got["kernel"])
                assert_equal(got, want, (name, s, flags, flip is None, route))
    m.sync()
    m.close()


def test_the_pad_position_is_never_read():
    m = modem()
    n, pattern = 4, DELETED_STEP                                          # nsent = 5, n = 6, s = 5: the pad rides on on-air number 1
    soft = on_air(3, n, pattern, 4)
    outs = []
    for fill in (0x7F, -0x80, 0):
        buf = soft.copy()
        buf[:, 0, 1] = fill
        outs.append(run(m, buf, n, pattern, 5, flags=OPEN_END, route=1))
        assert_equal(outs[-1], viterbi_ilv_ref(soft, n, pattern, 5, flags=OPEN_END), fill)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. the scratch route and the chunks
def test_a_row_past_the_lds_limit_takes_the_scratch_route_and_chunks_of_one_row_make_three_launches():
    m = modem()
    n, pattern = 8193, NAMED["3/4"]
    ntx = punct_ntx(n, pattern)
    s = ilv_stride(2 * ntx, 2 * ntx // 16)
    soft = on_air(2, n, pattern, 82)
    key = np.random.default_rng(83).integers(0, 4, ntx).astype(np.uint8)
    want = viterbi_ilv_ref(soft, n, pattern, s, flip=key)
    for route in (None, 1):
        got = run(m, soft, n, pattern, s, flip=key, route=route)
        assert got["kernel"] == SCRATCH_ROUTE and m.viterbi_launches() == 1, (got["kernel"], m.viterbi_launches())
        assert_equal(got, want, route)
    n, pattern = 150, NAMED["7/8"]
    ntx = punct_ntx(n, pattern)
    s = ilv_stride(2 * ntx, 2 * ntx // 16)
    soft = on_air(3, n, pattern, 15)
    want = viterbi_ilv_ref(soft, n, pattern, s)
    m.tune(viterbi_chunk_rows=1)
    got = run(m, soft, n, pattern, s, route=0)
    assert got["kernel"] == SCRATCH_ROUTE and m.viterbi_launches() == 3, (got["kernel"], m.viterbi_launches())
    assert_equal(got, want, "chunks")
    got = run(m, soft, n, pattern, s, route=1)
    assert got["kernel"] == LDS_ROUTE and m.viterbi_launches() == 1                 # the key is the scratch route's alone
    assert_equal(got, want, "lds")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. the 32-bit edge, and the two identities
@pytest.mark.parametrize("which", ["n - 1", "half"])
def test_the_longest_row_where_the_product_passes_32_bits_equals_the_punctured_call_on_the_gathered_row(which):
    """nsteps = 131072 at rate 1/2: n = 2^18 bits on air, k s up to 2^36.  Identity (1), GPU against GPU, so that no numpy decoder runs
    131072 steps"""
    m = modem()
    n = 131072
    nbits = 2 * n
    s = nbits - 1 if which == "n - 1" else ilv_stride(nbits, 2 ** 17)
    assert s == (nbits - 1 if which == "n - 1" else 2 ** 17 + 1)
    soft = on_air(2, n, HALF, 18)
    key = np.random.default_rng(19).integers(0, 4, n).astype(np.uint8)
    rows, fkey = gather_ref(soft, n, s, key)
    a = run(m, soft, n, HALF, s, flip=key, flags=OPEN_END)
    b = run_punct(m, rows, n, HALF, flip=fkey, flags=OPEN_END)
    assert a["kernel"] == SCRATCH_ROUTE and b["kernel"] == "viterbi_punct_kernel"
    assert_equal(a, b, which)
    assert a["info"][:, 3].min() > 1000                                    # random rows: the error count saw the whole row
    m.sync()
    m.close()


@pytest.mark.parametrize("n", [65, 262])
def test_identity_1_on_the_host_gathered_row_and_identity_2_stride_one(n):
    import torch
    m = modem()
    for name, pattern in sorted(PATTERNS.items()):
        ntx = punct_ntx(n, pattern)
        soft = on_air(3, n, pattern, n + 7 * len(name))
        key = np.random.default_rng(n).integers(0, 4, ntx).astype(np.uint8)
        for flip in (None, key):
            for flags in (0, OPEN_END):
                for route in (0, 1):
                    for s in strides_for(2 * ntx)[1:]:
                        rows, fkey = gather_ref(soft, ntx, s, flip)
                        a = run(m, soft, n, pattern, s, flip=flip, flags=flags, route=route)
                        b = run_punct(m, rows, n, pattern, flip=fkey, flags=flags, route=route)
                        assert "ilv" in a["kernel"] and "punct" in b["kernel"]
                        assert_equal(a, b, (name, s, flip is None, flags, route))
                    a = run(m, soft, n, pattern, 1, flip=flip, flags=flags, route=route)
                    b = run_punct(m, soft, n, pattern, flip=flip, flags=flags, route=route)
                    assert "ilv" in a["kernel"] and "punct" in b["kernel"]
                    assert_equal(a, b, (name, "stride 1", flip is None, flags, route))
        # the encoder at stride 1 is the punctured twin's
        packed = np.random.default_rng(n).integers(0, 256, (4, (n + 7) // 8), dtype=np.uint8)
        pt = torch.from_numpy(packed).cuda()
        ntx = punct_ntx(n + 6, pattern)
        a, b = (torch.full((4 * ntx,), 0x55, dtype=torch.uint8, device="cuda") for _ in range(2))
        m._check(m.L.qpsk_conv_encode_ilv_batch(m.h, ptr(pt), 4, n, 1, *pattern, 1, ptr(a)))
        assert m.last_kernel() == "conv_encode_ilv_kernel"
        m._check(m.L.qpsk_conv_encode_punct_batch(m.h, ptr(pt), 4, n, 1, *pattern, ptr(b)))
        m.sync()
        assert torch.equal(a, b), name
    m.close()


# ------------------------------------------------------------------------------------------ 4. the encoder
@pytest.mark.parametrize("nbits", [1, 8, 150, 8222])
def test_encoder_equals_the_restatement(nbits):
    import torch
    m = modem()
    R = 3
    packed = np.random.default_rng(nbits).integers(0, 256, (R, (nbits + 7) // 8), dtype=np.uint8)      # garbage in the last byte's padding
    pt = torch.from_numpy(packed).cuda()
    odd = 0
    coded = {tail: conv_encode_ref(packed, nbits, tail=tail) for tail in (True, False)}      # the reference's step loop runs once per tail
    for name, pattern in sorted(PATTERNS.items()):
        for tail in (True, False):
            nsteps = nbits + (6 if tail else 0)
            ntx, nsent = punct_ntx(nsteps, pattern), punct_nsent(nsteps, pattern)
            plain = puncture_ref(coded[tail], pattern)
            for s in strides_for(2 * ntx):
                want = interleave_ref(plain, nsent, s)                    # conv_encode_ilv_ref, its parts shared
                out = torch.full((R * ntx + GUARD,), 0x55, dtype=torch.uint8, device="cuda")
                m._check(m.L.qpsk_conv_encode_ilv_batch(m.h, ptr(pt), R, nbits, 1 if tail else 0, *pattern, s, ptr(out)))
                assert m.last_kernel() == "conv_encode_ilv_kernel"
                m.sync()
                assert np.array_equal(out[:R * ntx].cpu().numpy().reshape(R, ntx), want) and torch.all(out[R * ntx:] == 0x55), (name, tail, s)
                if s > 1:
                    got = m.conv_encode(packed, nbits, tail=tail, puncture=pattern, interleave=s)
                    m.sync()
                    assert np.array_equal(got.cpu().numpy(), want), (name, tail, s)
                odd += nsent & 1
    assert odd or nbits == 1, nbits
    assert m.conv_encode(packed, nbits, interleave=None).shape[1] == nbits + 6 and m.last_kernel() == "conv_encode_kernel"
    m.close()


def test_device_loopback_through_the_python_front_end():
    """conv_encode(interleave) -> scramble -> soft values at +-64 -> viterbi(interleave, flip = keystream) returns the bits"""
    import torch
    m = modem()
    R, nbits = 4, 256
    bits = np.random.default_rng(5).integers(0, 2, (R, nbits), dtype=np.uint8)
    packed = np.packbits(bits, axis=1, bitorder="little")
    for name in (None, "3/4"):
        ntx = m.punct_ntx(nbits + 6, name or "1/2")
        s = ilv_stride(2 * ntx, 2 * ntx // 16)
        tx = m.scramble(m.conv_encode(packed, nbits, puncture=name, interleave=s))
        key = m.scramble(torch.zeros((1, ntx), dtype=torch.uint8))[0]
        d = tx.to(torch.int16)
        soft = torch.stack([64 - 128 * (d & 1), 64 - 64 * (d & 2)], dim=-1).to(torch.int8)
        got = m.viterbi(soft, flip=key, nsteps=nbits + 6, puncture=name, interleave=s)
        assert "viterbi_ilv" in m.last_kernel()
        m.sync()
        out = np.unpackbits(got["bits"].cpu().numpy(), axis=1, bitorder="little")
        assert np.array_equal(out[:, :nbits], bits) and not got["info"].cpu().numpy()[:, 3].any(), name
    m.close()


# ------------------------------------------------------------------------------------------ 5. the framer
def frame_ilv_guarded(m, payloads, sync, pattern, stride, per_row, lead, gap, row_len, front, coded=True):
    """qpsk_frame_batch_ilv through the raw ABI with guard bytes in front of and behind d_out, which starts `front` bytes into its buffer"""
    import torch
    payloads = np.ascontiguousarray(payloads, np.uint8)
    npk, nbytes = payloads.shape
    nrows = npk // per_row
    d_src = torch.from_numpy(payloads).cuda()
    d_out = torch.full((front + nrows * row_len + 64,), FRAME_GUARD, dtype=torch.uint8, device="cuda")
    d_crc = torch.zeros((npk,), dtype=torch.int16, device="cuda")
    sw = np.ascontiguousarray(np.asarray(sync, np.uint8))
    rc = m.L.qpsk_frame_batch_ilv(m.h, ptr(d_src), 0, nrows, per_row, nbytes, sw.ctypes.data_as(C.c_void_p), len(sw), 1 if coded else 0, *pattern,
                                  stride, lead, gap, row_len, C.c_void_p(d_out.data_ptr() + front), ptr(d_crc))
    assert rc == 0, m.L.qpsk_last_error()
    kernel = m.last_kernel()
    m.sync()
    out = d_out.cpu().numpy()
    assert (out[:front] == FRAME_GUARD).all() and (out[front + nrows * row_len:] == FRAME_GUARD).all(), "d_out's guard bytes were written"
    return out[front:front + nrows * row_len].reshape(nrows, row_len), d_crc.cpu().numpy().view(np.uint16), kernel


@pytest.mark.parametrize("name", ["1/2", "3/4", "deleted"])
@pytest.mark.parametrize("nbytes", [1, 30, 1024])
def test_framer_equals_the_restatement_and_stride_one_equals_qpsk_frame_batch(nbytes, name):
    import torch
    m = modem()
    pattern = PATTERNS[name]
    rng = np.random.default_rng(nbytes + len(name))
    nsync, per_row, lead, gap, front = 17, 3, 5, 7, 61                    # odd lead and gap, d_out at an odd address
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    payloads = rng.integers(0, 256, (2 * per_row, nbytes), dtype=np.uint8)
    B = body_len(nbytes, True, pattern)
    row_len = starts(nsync, nbytes, True, pattern, per_row, lead, gap)[-1] + nsync + B + 9
    plain = frame_ref(payloads, sync, True, pattern, per_row, lead, gap, row_len)
    for s in strides_for(2 * B):
        want, want_crc = frame_ilv_ref(payloads, sync, True, pattern, per_row, lead, gap, row_len, s, plain=plain)
        got, crc, kernel = frame_ilv_guarded(m, payloads, sync, pattern, s, per_row, lead, gap, row_len, front)
        assert kernel == ("frame_kernel<coded,ilv>" if s > 1 else "frame_kernel<coded>"), (s, kernel)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "stride %d: %d dibits differ, first at (row, column) %s" % (s, len(bad), bad[0])
        assert np.array_equal(crc, want_crc)
        if s > 1:
            o = m.frame(payloads, sync, puncture=pattern, per_row=per_row, lead=lead, gap=gap, row_len=row_len, interleave=s)
            m.sync()
            assert np.array_equal(o["dibits"].cpu().numpy(), want)
        else:
            o = m.frame(payloads, sync, puncture=pattern, per_row=per_row, lead=lead, gap=gap, row_len=row_len)
            assert m.last_kernel() == "frame_kernel<coded>"
            m.sync()
            assert np.array_equal(o["dibits"].cpu().numpy(), got)             # byte for byte qpsk_frame_batch
    # the uncoded format: stride 1 is qpsk_frame_batch, any other is refused
    row_len = lead + nsync + 4 * (nbytes + 2)
    got, _, kernel = frame_ilv_guarded(m, payloads[:2], sync, (1, 1, 1), 1, 1, lead, 0, row_len, front, coded=False)
    assert kernel == "frame_kernel<uncoded>"
    assert np.array_equal(got, m.frame(payloads[:2], sync, coded=False, lead=lead)["dibits"].cpu().numpy())
    buf = torch.zeros((2 * row_len,), dtype=torch.uint8, device="cuda")
    sw = np.ascontiguousarray(sync)
    assert m.L.qpsk_frame_batch_ilv(m.h, ptr(torch.from_numpy(payloads).cuda()), 0, 2, 1, nbytes, sw.ctypes.data_as(C.c_void_p), nsync, 0, 1, 1, 1, 3,
                                    lead, 0, row_len, ptr(buf), None) == QPSK_ERR_ARG
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 6. the stream deframer
DF = dict(S=2, nbytes=5, nsync=20, min_score=18, npackets=3)


def df_streams(pattern, stride, seed):
    """2 streams of 3 packets each with noise as in test_punct_cpu.punct_stream, brought to one length with random dibits -> (S, total, 2)"""
    rng = np.random.default_rng(seed)
    sync = rng.integers(0, 4, DF["nsync"], dtype=np.uint8)
    zs = [ilv_stream(rng, sync, DF["nbytes"], pattern, stride, DF["npackets"], noise=0.12, bad=(1,) if k else ())[0] for k in range(DF["S"])]
    total = max(len(z) for z in zs) + 5
    zs = [np.concatenate([z, dibits_to_costas(rng.integers(0, 4, total - len(z), dtype=np.uint8), amp=0.8, noise=0.12, rng=rng)]) for z in zs]
    return sync, np.stack(zs).astype(np.float32)


def cuts_of(sizes, total):
    """pushes of the given sizes, cut off at the stream's end, then the rest"""
    out = []
    for size in sizes:
        if sum(out) < total:
            out.append(min(size, total - sum(out)))
    return out + ([total - sum(out)] if sum(out) < total else [])


def df_want(rows, gains, sync, pattern, stride):
    out = []
    for k in range(DF["S"]):
        ref = deframe_coded_ilv_ref([r[k] for r in rows], None if gains is None else [g[k] for g in gains], sync, DF["min_score"], DF["nbytes"],
                                    pattern, stride)
        out.append([rec(j, p) for j, push in enumerate(ref) for p in push])
    return out


def reset_ilv(m, sync, pattern, stride, S=DF["S"], nbytes=DF["nbytes"], max_packets=4):
    sw = np.ascontiguousarray(sync)
    rc = m.L.qpsk_deframer_reset_coded_ilv(m.h, S, sw.ctypes.data_as(C.c_void_p), len(sw), DF["min_score"], nbytes, max_packets, 0, 64.0,
                                           *pattern, stride)
    if rc == 0:
        m.df_shape = (S, nbytes, max_packets)
    return rc


@pytest.mark.parametrize("name", ["1/2", "3/4", "deleted"])
def test_deframer_bit_for_bit_for_several_cuts_and_stride_one_equals_the_punctured_reset(name):
    m = modem()
    pattern = PATTERNS[name]
    n = 2 * punct_ntx(coded_punct_steps(DF["nbytes"]), pattern)
    s = ilv_stride(n, n // 16)
    sync, z = df_streams(pattern, s, len(name))
    total, P = z.shape[1], DF["nsync"] + n // 2
    for cuts, with_gain in (([total], True), ([P // 2, P, 7, 1], True), ([33] * total, False), ([3 * P // 2], True)):
        rows = rows_of(z, cuts_of(cuts, total))
        gains = np.full((len(rows), DF["S"]), 70.0, np.float32) if with_gain else None
        assert reset_ilv(m, sync, pattern, s) == 0
        got = push_all(m, rows, gains)
        assert "deframe_coded_decode_ilv_kernel" in m.last_kernel(), m.last_kernel()
        want = df_want(rows, gains, sync, pattern, s)
        for k in range(DF["S"]):
            assert got[k] == want[k], (cuts[:3], k, got[k][:1], want[k][:1])
        assert [len(g) for g in got] == [DF["npackets"]] * DF["S"] and [r[5] for r in got[0]] == [True] * 3 and [r[5] for r in got[1]] == [True, False, True]
    # the Python front end, both routes
    for route, word in ((0, "<global>"), (1, "<lds>")):
        m.tune(viterbi_lds=route)
        m.deframer_reset_coded(DF["S"], sync, DF["nbytes"], DF["min_score"], max_packets=4, puncture=pattern, interleave=s)
        assert push_all(m, rows, gains) == got and m.last_kernel().endswith("deframe_coded_decode_ilv_kernel" + word), m.last_kernel()
    # stride 1 is the punctured reset
    assert reset_ilv(m, sync, pattern, 1) == 0
    a = push_all(m, rows, gains)
    ka = m.last_kernel()
    m.deframer_reset_coded(DF["S"], sync, DF["nbytes"], DF["min_score"], max_packets=4, puncture=pattern)
    b = push_all(m, rows, gains)
    assert "ilv" in ka and "punct" in m.last_kernel() and a == b and sum(len(x) for x in a) == 6
    m.close()


def test_packets_back_to_back_at_the_per_push_bound_through_a_stride():
    """test_deframe_coded_gpu's back-to-back sets behind the pattern 3/4 and a stride: max_packets = k + 1, k and 64"""
    sets = hunt_coded_sets("ilv")
    assert len(sets) == 3 and all(s["stride"] > 1 for s in sets)
    for s in sets:
        hunt_set_on_the_device(s)


def test_a_refused_reset_leaves_the_deframer_working_and_the_uncoded_push_is_refused():
    import torch
    m = modem()
    pattern = PATTERNS["3/4"]
    n = 2 * punct_ntx(coded_punct_steps(DF["nbytes"]), pattern)
    s = ilv_stride(n, n // 16)
    sync, z = df_streams(pattern, s, 9)
    total = z.shape[1]
    rows = rows_of(z, cuts_of([total // 3, total // 3], total))
    gains = np.full((len(rows), DF["S"]), 70.0, np.float32)
    want = df_want(rows, gains, sync, pattern, s)
    assert reset_ilv(m, sync, pattern, s) == 0
    got = push_all(m, rows[:1], gains[:1])
    for bad in (0, -1, 2, n, n + 1, bad_odd(n)):
        assert reset_ilv(m, sync, pattern, bad) == QPSK_ERR_ARG, bad
        assert b"qpsk_deframer_reset_coded_ilv" in m.L.qpsk_last_error()
    more = push_all(m, rows[1:], gains[1:])
    got = [g + [(r[0] + 1,) + r[1:] for r in h] for g, h in zip(got, more)]
    assert got == want and sum(len(g) for g in got) == 6
    cnt = torch.zeros((DF["S"],), dtype=torch.int32, device="cuda")
    zz = torch.zeros((DF["S"], 50, 2), dtype=torch.float32, device="cuda")
    assert m.L.qpsk_deframer_push(m.h, ptr(zz), None, 50, ptr(cnt), None, None, None, None, None) == QPSK_ERR_STATE
    m.sync()
    m.close()


def bad_odd(n):
    """an odd stride below n that shares a factor with n"""
    return next(v for v in range(3, n, 2) if np.gcd(v, n) != 1)


# ------------------------------------------------------------------------------------------ 7. a burst, end to end on the device
def test_a_burst_of_16_dibits_passes_every_crc_through_the_interleaver_and_fails_without_it():
    """Modem.frame(interleave=s) -> dibits on the diagonals -> 16 consecutive body dibits inverted -> deframe_coded.  30-byte packets at
    rate 1/2, n = 524, s = 33, no other noise.  Asserted: with the interleaver every CRC passes; without it, on the same burst positions,
    at least 3 of the 4 packets fail"""
    m = modem()
    rng = np.random.default_rng(16)
    nbytes, nsync, npk, gap = 30, 24, 4, 9
    sync = rng.integers(0, 4, nsync, dtype=np.uint8)
    payloads = rng.integers(0, 256, (npk, nbytes), dtype=np.uint8)
    B = body_len(nbytes, True, HALF)
    s = ilv_stride(2 * B, 2 * B // 16)
    assert (2 * B, s) == (524, 33)
    at = rng.integers(0, B - 16 + 1, npk)
    failed = {}
    for stride in (s, None):
        o = m.frame(payloads, sync, per_row=npk, lead=3, gap=gap, interleave=stride)
        assert m.last_kernel() == ("frame_kernel<coded,ilv>" if stride else "frame_kernel<coded>")
        z = dibits_to_costas(o["dibits"].cpu().numpy()[0], amp=0.7)
        for j, a0 in enumerate(starts(nsync, nbytes, True, HALF, npk, 3, gap)):
            a = a0 + nsync + int(at[j])
            z[a:a + 16] = -z[a:a + 16]
        m.deframer_reset_coded(1, sync, nbytes, nsync - 2, max_packets=8, interleave=stride)
        got = m.deframe_coded(z[None], gain=np.array([64.0 / 0.7], np.float32))
        m.sync()
        assert int(got["count"][0]) == npk
        ok = got["crc_ok"].cpu().numpy()[0, :npk].astype(bool)
        if stride:
            assert np.array_equal(got["bytes"].cpu().numpy()[0, :npk, :nbytes], payloads)
        failed[stride] = int((~ok).sum())
    print("CRC failures of %d packets: %d through the interleaver, %d without" % (npk, failed[s], failed[None]))
    assert failed[s] == 0 and failed[None] >= 3, failed
    m.close()


# ------------------------------------------------------------------------------------------ 8. the error contract
def test_every_bad_stride_class_is_refused_launches_nothing_and_leaves_the_context_usable():
    import torch
    m = modem()
    R, n = 3, 262
    pattern = HALF
    ntx = punct_ntx(n, pattern)
    nbits = 2 * ntx
    assert nbits == 524
    soft = on_air(R, n, pattern, 1)
    want = viterbi_ilv_ref(soft, n, pattern, 33)
    assert_equal(run(m, soft, n, pattern, 33), want)
    last = m.last_kernel()
    q = torch.from_numpy(soft).cuda()
    bits = torch.full((R * 33,), 0x55, dtype=torch.uint8, device="cuda")
    info = torch.full((R, 4), 0x55555555, dtype=torch.int32, device="cuda")
    enc_in = torch.zeros((R, 32), dtype=torch.uint8, device="cuda")
    enc_out = torch.full((R * ntx,), 0x55, dtype=torch.uint8, device="cuda")
    pay = torch.zeros((2, 30), dtype=torch.uint8, device="cuda")
    row = torch.full((2 * 300,), 0x55, dtype=torch.uint8, device="cuda")
    sw = (C.c_uint8 * 16)(*([1, 2, 3, 0] * 4))
    for bad in (0, -1, -33, 2, 262, nbits, nbits + 1, 2 ** 31 - 1, bad_odd(nbits)):      # 0, negative, even, >= n, odd but not coprime (131)
        assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), 0, R, n, *pattern, bad, None, 0, ptr(bits), ptr(info)) == QPSK_ERR_ARG, bad
        assert b"qpsk_viterbi_ilv_batch" in m.L.qpsk_last_error() and m.viterbi_launches() == 0
        assert m.L.qpsk_conv_encode_ilv_batch(m.h, ptr(enc_in), R, 256, 1, *pattern, bad, ptr(enc_out)) == QPSK_ERR_ARG, bad
        assert m.L.qpsk_frame_batch_ilv(m.h, ptr(pay), 0, 2, 1, 30, sw, 16, 1, *pattern, bad, 0, 0, 300, ptr(row), None) == QPSK_ERR_ARG, bad
        assert m.L.qpsk_deframer_reset_coded_ilv(m.h, 1, sw, 16, 14, 30, 4, 0, 64.0, *pattern, bad) == QPSK_ERR_ARG, bad
        assert m.last_kernel() == last
    assert bad_odd(nbits) == 131
    # n = 2 takes stride 1 alone; nothing sent at all is refused
    one = on_air(R, 1, HALF, 2)
    assert_equal(run(m, one, 1, HALF, 1), viterbi_ilv_ref(one, 1, HALF, 1))
    last = m.last_kernel()
    for bad in (0, 2, 3):
        assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), 0, R, 1, *HALF, bad, None, 0, ptr(bits), ptr(info)) == QPSK_ERR_ARG, bad
    assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), 0, R, 1, 2, 2, 2, 1, None, 0, ptr(bits), ptr(info)) == QPSK_ERR_ARG      # ntx = 0
    assert m.L.qpsk_conv_encode_ilv_batch(m.h, ptr(enc_in), R, 1, 0, 2, 2, 2, 1, ptr(enc_out)) == QPSK_ERR_ARG
    # the twins' other argument checks hold here too
    assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), ntx - 1, R, n, *pattern, 33, None, 0, ptr(bits), ptr(info)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), 0, R, n, 3, 8, 1, 33, None, 0, ptr(bits), ptr(info)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), 0, R, n, *pattern, 33, None, 4, ptr(bits), ptr(info)) == QPSK_ERR_ARG
    assert m.L.qpsk_viterbi_ilv_batch(m.h, ptr(q), 0, R, n, *pattern, 33, None, 0, None, None) == QPSK_ERR_ARG
    assert m.last_kernel() == last
    m.sync()
    assert torch.all(bits == 0x55) and torch.all(info == 0x55555555) and torch.all(enc_out == 0x55) and torch.all(row == 0x55)
    with pytest.raises(Exception):
        m.viterbi(soft, nsteps=n, interleave=2)
    assert_equal(run(m, soft, n, pattern, 33), want)                       # the context still works
    m.sync()
    m.close()
