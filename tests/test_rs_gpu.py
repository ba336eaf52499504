"""qpsk_rs_encode_batch / qpsk_rs_decode_batch and Modem.rs_encode / rs_decode on the GPU, bit for bit against the numpy restatements of
test_rs_cpu.py (REED-SOLOMON of include/qpsk_hip.h): every code and error pattern in one call per code, so that neighbouring waves leave by
different exits; the call shapes (row counts, pitches with poison between the rows, in place, either output alone, guards); the encoder;
the erasure identity; the error contract; and the link of the CPU test on the device, the deframer's bytes decoded where they lie.  There
is no tolerance anywhere.  Section 7 decodes the rare paths and the seams of the kernel's lane chunks, the rows of rs_rows.py."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_cpu import dibits_to_costas
from rs_rows import directed_codes, directed_rows, edge_codes, edge_rows
from test_punct_cpu import NAMED
from test_rs_cpu import LINK, RS_CODES, case, encoder_rows, link_result, rs_decode_ref, rs_encode_ref
from test_viterbi_gpu import GUARD, modem, ptr

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG = -2
POISON, OUT_FILL, INFO_FILL = 0xA5, 0x55, 0x55555555


# ------------------------------------------------------------------------------------------ the rows of one code, and their references
def tile(a, R):
    return np.ascontiguousarray(np.resize(a, (R,) + a.shape[1:]))


def decode(m, words, nroots, flags=None, in_pitch=0, out_pitch=0, inplace=False, want=("out", "info")):
    """the raw call: pitched buffers filled with POISON between the rows, GUARD elements behind every output -> dict(out, info, kernel); an
    output that was not asked for is passed as NULL"""
    import torch
    R, n = words.shape
    ip, op = in_pitch or n, (in_pitch or n) if inplace else (out_pitch or n)
    src = np.full((R, ip), POISON, np.uint8)
    src[:, :n] = words
    d_in = torch.from_numpy(np.concatenate([src.reshape(-1), np.full(GUARD, POISON, np.uint8)])).cuda()
    d_er = None if flags is None else torch.from_numpy(np.array(flags, np.uint8)).cuda()
    d_out = d_in if inplace else torch.full((R * op + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    d_info = torch.full((R * 4 + GUARD,), INFO_FILL, dtype=torch.int32, device="cuda")
    m._check(m.L.qpsk_rs_decode_batch(m.h, ptr(d_in), in_pitch, R, n, nroots, ptr(d_er), ptr(d_out) if "out" in want else None,
                                      in_pitch if inplace else out_pitch, ptr(d_info) if "info" in want else None))
    kernel = m.last_kernel()
    torch.cuda.synchronize()
    ho, hi, hin = d_out.cpu().numpy(), d_info.cpu().numpy(), d_in.cpu().numpy()
    fill = POISON if inplace else OUT_FILL
    assert np.all(ho[R * op:] == fill) and np.all(hi[R * 4:] == INFO_FILL), "a guard behind an output was overwritten"
    rows = ho[:R * op].reshape(R, op)
    assert np.all(rows[:, n:] == fill), "bytes between the output's rows were written"
    if "out" not in want:
        assert np.all(ho == fill) or inplace
    if "info" not in want:
        assert np.all(hi == INFO_FILL)
    if not inplace or "out" not in want:
        assert np.array_equal(hin[:R * ip].reshape(R, ip), src), "the input was written"
    return dict(out=rows[:, :n], info=hi[:R * 4].reshape(R, 4), kernel=kernel)


def assert_rows(got, want, names, what):
    out, info = want
    for i in range(len(out)):
        name = names[i % len(names)]
        assert np.array_equal(got["info"][i], info[i]), (what, i, name, got["info"][i], info[i])
        assert np.array_equal(got["out"][i], out[i]), (what, i, name)


def case_checked(n, k):
    """case(n, k), after the references themselves have said what the patterns were built for: rows within the radius come back as sent,
    the others fail or come back as another codeword"""
    c = case(n, k)
    nroots, t = n - k, (n - k) // 2
    names, (out, info) = c["names"], c["erased"]
    for name in ("clean", "t errors", "f = nroots, e = 0", "2 e + f = nroots", "erased bytes that are right", "error at j = 0",
                 "error at j = n - 1", "error in the parity")[:3 if nroots == 1 else None]:
        i = names.index(name)
        if name.startswith("error") and t == 0:
            continue
        assert info[i, 0] >= 0 and np.array_equal(out[i], c["sent"][i]), (name, info[i])
    assert info[names.index("f = nroots + 1"), 0] == -1 and info[names.index("f = nroots + 1"), 1] == nroots + 1
    i = names.index("erased bytes that are right")
    assert 0 <= info[i, 0] < info[i, 1] == nroots
    assert tuple(info[names.index("clean with erasures")]) == (0, max(t, 1), 0, 1)
    i = names.index("t + 1 errors")
    assert info[i, 0] == -1 or not np.array_equal(out[i], c["sent"][i])          # beyond the radius: failed, or another codeword
    return c


# ------------------------------------------------------------------------------------------ 1. every code, every pattern, one call
@pytest.mark.parametrize("n,k", RS_CODES)
def test_every_pattern_of_a_code_in_one_call_bit_for_bit(n, k):
    c = case_checked(n, k)
    nroots, names = n - k, c["names"]
    m = modem()
    got = decode(m, c["words"], nroots, c["flags"])
    assert got["kernel"] == "rs_decode_kernel"
    assert_rows(got, c["erased"], names, "erasures")
    assert_rows(decode(m, c["words"], nroots, None), c["plain"], names, "d_erase NULL")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. the call shapes
@pytest.mark.parametrize("n,k", [(60, 44), (21, 16), (255, 191)])
@pytest.mark.parametrize("R", [1, 5, 70])
def test_row_counts_pitches_in_place_and_either_output_alone(n, k, R):
    c = case(n, k)
    words, flags = tile(c["words"], R), tile(c["flags"], R)
    want = (tile(c["erased"][0], R), tile(c["erased"][1], R))
    m = modem()
    for what, kw in (("tight", {}), ("pitched input", dict(in_pitch=n + 2)), ("pitched output", dict(out_pitch=n + 7)),
                     ("both pitched", dict(in_pitch=n + 1, out_pitch=n + 3)), ("in place", dict(inplace=True)),
                     ("in place, pitched", dict(inplace=True, in_pitch=n + 2))):
        assert_rows(decode(m, words, n - k, flags, **kw), want, c["names"], what)
    got = decode(m, words, n - k, flags, in_pitch=n + 2, want=("info",))
    assert np.array_equal(got["info"], want[1])
    got = decode(m, words, n - k, flags, out_pitch=n + 5, want=("out",))
    assert np.array_equal(got["out"], want[0])
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. the encoder
def encode(m, data, nroots, data_pitch=0, out_pitch=0):
    import torch
    R, k = data.shape
    n, ip, op = k + nroots, data_pitch or k, out_pitch or k + nroots
    src = np.full((R, ip), POISON, np.uint8)
    src[:, :k] = data
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((R * op + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    m._check(m.L.qpsk_rs_encode_batch(m.h, ptr(d_in), data_pitch, R, k, nroots, ptr(d_out), out_pitch))
    assert m.last_kernel() == "rs_encode_kernel"
    torch.cuda.synchronize()
    ho = d_out.cpu().numpy()
    assert np.all(ho[R * op:] == OUT_FILL), "the guard behind the output was overwritten"
    rows = ho[:R * op].reshape(R, op)
    assert np.all(rows[:, n:] == OUT_FILL), "bytes between the output's rows were written"
    assert np.array_equal(d_in.cpu().numpy(), src)
    return rows[:, :n]


@pytest.mark.parametrize("n,k", RS_CODES)
def test_encoder_equals_the_restatement_for_every_row_count_and_pitch(n, k):
    m = modem()
    for R, data in encoder_rows(n, k):
        want = rs_encode_ref(data, n - k)
        for dp, op in ((0, 0), (k + 3, 0), (0, n + 2), (k + 1, n + 5)):
            assert np.array_equal(encode(m, data, n - k, dp, op), want), (R, dp, op)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 4. encode, erase, decode
def encode_erase_decode(m, n, k):
    """the encoder's rows with random erasures of up to nroots places each come back, with the counts the damage says"""
    import torch
    nroots, R = n - k, 33
    rng = np.random.default_rng(n + 7 * k)
    data = torch.from_numpy(rng.integers(0, 256, (R, k), dtype=np.uint8)).cuda()
    rows = m.rs_encode(data, nroots)
    assert tuple(rows.shape) == (R, n)
    sent = rows.cpu().numpy()
    flags, hit = np.zeros((R, n), np.uint8), sent.copy()
    for r in range(R):
        f = nroots if r == 0 else int(rng.integers(0, nroots + 1))
        at = rng.choice(n, f, replace=False)
        flags[r, at] = 1
        hit[r, at] = rng.integers(0, 256, f, dtype=np.uint8)                   # some erased bytes stay right by chance
    out, info = m.rs_decode(hit, nroots, erasures=flags)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(out, sent)
    assert np.array_equal(info[:, 0], (hit != sent).sum(axis=1)) and np.array_equal(info[:, 1], flags.sum(axis=1)) and not info[:, 2].any()


@pytest.mark.parametrize("n,k", RS_CODES)
def test_the_encoder_s_rows_come_back_from_random_erasures_of_up_to_nroots_positions(n, k):
    m = modem()
    encode_erase_decode(m, n, k)
    m.sync()
    m.close()


def test_python_front_end_pitch_n_and_inplace():
    import torch
    c = case(60, 44)
    m = modem()
    words, flags, (want_out, want_info) = c["words"].copy(), c["flags"].copy(), c["erased"]
    out, info = m.rs_decode(words, 16, erasures=flags)
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(info.cpu().numpy(), want_info)
    wide = np.full((len(words), 62), POISON, np.uint8)
    wide[:, :60] = words
    dev = torch.from_numpy(wide).cuda()
    out, info = m.rs_decode(dev, 16, erasures=flags, pitch=62, n=60)
    assert tuple(out.shape) == (len(words), 60) and np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(dev.cpu().numpy(), wide)
    out, info = m.rs_decode(dev, 16, erasures=flags, pitch=62, n=60, inplace=True)
    assert out.data_ptr() == dev.data_ptr() and np.array_equal(info.cpu().numpy(), want_info)
    back = dev.cpu().numpy()
    assert np.array_equal(back[:, :60], want_out) and np.all(back[:, 60:] == POISON)
    enc = m.rs_encode(c["sent"][:, :44], 16, pitch=62)
    assert tuple(enc.shape) == (len(words), 60) and enc.stride(0) == 62
    good = c["erased"][1][:, 0] >= 0
    assert np.array_equal(enc.cpu().numpy()[good], want_out[good])              # every decoded row is a codeword: re-encoding its data gives it
    with pytest.raises(ValueError):
        m.rs_decode(words, 16, inplace=True)                                    # a numpy array cannot be decoded in place
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 5. the error contract
def test_every_bad_argument_is_refused_with_nothing_written_and_the_context_stays_usable():
    import torch
    import qpsk_amd
    c = case(21, 16)
    m = modem()
    n, nroots, R = 21, 5, 8
    words = tile(c["words"], R)
    d_in = torch.from_numpy(words.copy()).cuda()
    d_er = torch.zeros((R, n), dtype=torch.uint8, device="cuda")
    d_out = torch.full((R * 64,), OUT_FILL, dtype=torch.uint8, device="cuda")
    d_info = torch.full((R * 4 + 8,), INFO_FILL, dtype=torch.int32, device="cuda")
    before = m.last_kernel()
    L, h = m.L, m.h
    at = lambda t, off: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    dec = [
        ("null context", lambda: L.qpsk_rs_decode_batch(None, ptr(d_in), 0, R, n, nroots, None, ptr(d_out), 0, ptr(d_info))),
        ("null input", lambda: L.qpsk_rs_decode_batch(h, None, 0, R, n, nroots, None, ptr(d_out), 0, ptr(d_info))),
        ("both outputs null", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, nroots, None, None, 0, None)),
        ("nrows 0", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, 0, n, nroots, None, ptr(d_out), 0, ptr(d_info))),
        ("nrows negative", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, -1, n, nroots, None, ptr(d_out), 0, ptr(d_info))),
        ("nroots 0", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, 0, None, ptr(d_out), 0, ptr(d_info))),
        ("nroots 65", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, 1, 130, 65, None, ptr(d_out), 0, ptr(d_info))),
        ("k = 0", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, 5, 5, None, ptr(d_out), 0, ptr(d_info))),
        ("n = 256", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, 1, 256, 32, None, ptr(d_out), 0, ptr(d_info))),
        ("in_pitch below n", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), n - 1, R, n, nroots, None, ptr(d_out), 0, ptr(d_info))),
        ("in_pitch negative", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), -n, R, n, nroots, None, ptr(d_out), 0, ptr(d_info))),
        ("out_pitch below n", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, nroots, None, ptr(d_out), n - 1, ptr(d_info))),
        ("a pitch that leaves 64 bits", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, nroots, None, ptr(d_out), 1 << 62, ptr(d_info))),
        ("in place with another pitch", lambda: L.qpsk_rs_decode_batch(h, ptr(d_out), 0, R, n, nroots, None, ptr(d_out), n + 1, ptr(d_info))),
        ("output one byte into the input", lambda: L.qpsk_rs_decode_batch(h, ptr(d_out), 0, R, n, nroots, None, at(d_out, 1), 0, ptr(d_info))),
        ("output overlaps the input's tail", lambda: L.qpsk_rs_decode_batch(h, ptr(d_out), 0, R, n, nroots, None, at(d_out, R * n - 1), 0, ptr(d_info))),
        ("info misaligned", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, nroots, None, ptr(d_out), 0, at(d_info, 2))),
        ("info inside the output", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, nroots, None, ptr(d_out), 0, at(d_out, 16))),
        ("info inside the input", lambda: L.qpsk_rs_decode_batch(h, ptr(d_out), 0, R, n, nroots, None, None, 0, at(d_out, 16))),
        ("erasures inside the output", lambda: L.qpsk_rs_decode_batch(h, ptr(d_in), 0, R, n, nroots, at(d_out, 8), ptr(d_out), 0, ptr(d_info))),
    ]
    enc = [
        ("null context", lambda: L.qpsk_rs_encode_batch(None, ptr(d_in), 0, R, 16, 5, ptr(d_out), 0)),
        ("null data", lambda: L.qpsk_rs_encode_batch(h, None, 0, R, 16, 5, ptr(d_out), 0)),
        ("null output", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, R, 16, 5, None, 0)),
        ("nrows 0", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, 0, 16, 5, ptr(d_out), 0)),
        ("k 0", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, R, 0, 5, ptr(d_out), 0)),
        ("nroots 0", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, R, 16, 0, ptr(d_out), 0)),
        ("nroots 65", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, 1, 16, 65, ptr(d_out), 0)),
        ("k + nroots = 256", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, 1, 192, 64, ptr(d_out), 0)),
        ("data_pitch below k", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 15, R, 16, 5, ptr(d_out), 0)),
        ("out_pitch below n", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, R, 16, 5, ptr(d_out), 20)),
        ("out_pitch negative", lambda: L.qpsk_rs_encode_batch(h, ptr(d_in), 0, R, 16, 5, ptr(d_out), -21)),
        ("output over the data", lambda: L.qpsk_rs_encode_batch(h, ptr(d_out), 21, R, 16, 5, ptr(d_out), 21)),
    ]
    for who, calls in (("qpsk_rs_decode_batch", dec), ("qpsk_rs_encode_batch", enc)):
        for what, call in calls:
            assert call() == QPSK_ERR_ARG, (who, what)
            assert who.encode() in L.qpsk_last_error(), (who, what)
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == OUT_FILL) and np.all(d_info.cpu().numpy() == INFO_FILL) and np.array_equal(d_in.cpu().numpy(), words)
    assert m.last_kernel() == before                                            # nothing was launched
    with pytest.raises(qpsk_amd.QpskError):
        m.rs_encode(np.zeros((2, 200), np.uint8), 64)
    m.sync()                                                                    # no call raised the context's status word
    got = decode(m, c["words"], nroots, c["flags"])
    assert_rows(got, c["erased"], c["names"], "after the refusals")
    assert (c["erased"][1][:, 0] == -1).any()                                   # ... and failed rows do not raise it either
    m.sync()
    m.close()


def test_buffers_that_touch_are_accepted_and_one_shared_byte_is_refused():
    """3 rows of (15, 11) inside one allocation, tight (45 bytes) or at pitch 20 (2 * 20 + 15 = 55 bytes: the padding behind the last row is
    not the buffer).  Every pair of ranges the two calls compare, with the later one beginning at the byte behind the earlier one's last
    (accepted, and the call's results are the reference's) and on that last byte (refused, with the present text)"""
    import torch
    rng = np.random.default_rng(15)
    R, n, nroots, pitch = 3, 15, 4, 20
    k = n - nroots
    sent = rs_encode_ref(rng.integers(0, 256, (R, k), dtype=np.uint8), nroots)
    words, flags = sent.copy(), np.zeros((R, n), np.uint8)
    words[1, 2] ^= 0x40
    words[1, 9] ^= 0x01
    words[2, 0] ^= 0xFF
    words[2, 7] ^= 0x10
    flags[2, 0] = flags[2, 7] = 1
    wants = {True: rs_decode_ref(words, nroots, flags), False: rs_decode_ref(words, nroots, None)}
    assert all(np.array_equal(w[0], sent) for w in wants.values()) and wants[True][1][1:, 0].all()
    m = modem()
    L, h = m.L, m.h
    arena = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    at = lambda off: None if off is None else C.c_void_p(arena.data_ptr() + off)      # noqa: E731

    def put(off, rows, p):
        for r in range(R):
            arena[off + r * p:off + r * p + rows.shape[1]] = torch.from_numpy(rows[r].copy()).cuda()

    def get(off, w, p):
        host = arena.cpu().numpy()
        return np.stack([host[off + r * p:off + r * p + w] for r in range(R)])

    def dec(i=400, ip=0, e=None, o=800, op=0, f=900):
        arena.zero_()
        put(i, words, ip or n)
        if e is not None:
            put(e, flags, n)
        rc = L.qpsk_rs_decode_batch(h, at(i), ip, R, n, nroots, at(e), at(o), op, at(f))
        torch.cuda.synchronize()
        return rc

    accepted = (dict(o=445, f=352), dict(i=403, o=358, f=448), dict(ip=20, o=455), dict(ip=20, o=345, op=20), dict(o=500, e=545), dict(o=500, e=455),
                dict(e=603, f=648), dict(e=600, f=552), dict(o=603, f=648), dict(o=600, f=552), dict(o=400), dict(ip=20, o=400, op=20),
                dict(o=None), dict(f=None), dict(e=200, f=None))
    for kw in accepted:
        assert dec(**kw) == 0, (kw, L.qpsk_last_error())
        want_out, want_info = wants[kw.get("e") is not None]
        if kw.get("o", 800) is not None:
            assert np.array_equal(get(kw.get("o", 800), n, kw.get("op", 0) or n), want_out), kw
        if kw.get("f", 900) is not None:
            assert np.array_equal(get(kw.get("f", 900), 16, 16).view(np.int32), want_info), kw
    io, oe, info = b"d_out overlaps d_in", b"d_out overlaps d_erase", b"d_info is not 4-byte aligned, or overlaps d_in, d_out or d_erase"
    refused = ((dict(o=444), io), (dict(i=403, o=359), io), (dict(ip=20, o=454), io), (dict(ip=20, o=346, op=20), io), (dict(o=400, op=20), io),
               (dict(o=500, e=544), oe), (dict(o=500, e=456), oe), (dict(e=604, f=648), info), (dict(e=599, f=552), info),
               (dict(o=604, f=648), info), (dict(o=599, f=552), info), (dict(i=404, f=448), info), (dict(i=399, f=352), info))
    for kw, text in refused:
        assert dec(**kw) == QPSK_ERR_ARG and b"qpsk_rs_decode_batch: " + text in L.qpsk_last_error(), (kw, L.qpsk_last_error())

    def enc(i=400, ip=0, o=800, op=0):
        arena.zero_()
        put(i, sent[:, :k], ip or k)
        rc = L.qpsk_rs_encode_batch(h, at(i), ip, R, k, nroots, at(o), op)
        torch.cuda.synchronize()
        return rc
    for kw in (dict(o=433), dict(i=445, o=400), dict(ip=20, o=451), dict(i=455, o=400, op=20)):      # the data are 33 bytes, or 2 * 20 + 11 = 51
        assert enc(**kw) == 0, (kw, L.qpsk_last_error())
        assert np.array_equal(get(kw["o"], n, kw.get("op", 0) or n), sent), kw
    for kw in (dict(o=432), dict(i=444, o=400), dict(ip=20, o=450), dict(i=454, o=400, op=20)):
        assert enc(**kw) == QPSK_ERR_ARG and b"qpsk_rs_encode_batch: d_out overlaps d_data" in L.qpsk_last_error(), (kw, L.qpsk_last_error())
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 6. the link of the CPU test, on the device
def test_the_cpu_link_on_the_device_with_the_deframer_s_bytes_decoded_where_they_lie():
    """Modem.rs_encode -> Modem.frame -> the CPU test's inverted run -> Modem.deframe_coded, then qpsk_rs_decode_batch straight on the
    deframer's bytes (64 streams x 1 packet x 62 bytes) through in_pitch = nbytes + 2: crc_ok and the decoded data equal the CPU link
    test's packet for packet"""
    import torch
    lk, r = LINK, link_result()
    P, n, k = lk["packets"], lk["n"], lk["k"]
    m = modem()
    words = m.rs_encode(r["data"], n - k)
    assert np.array_equal(words.cpu().numpy(), r["words"])
    o = m.frame(words.contiguous(), r["sync"], coded=True, puncture=lk["rate"], per_row=1, lead=lk["lead"], gap=lk["gap"])
    rows = o["dibits"].cpu().numpy()
    assert np.array_equal(rows, r["rows"])
    hit = rows.copy()
    b0 = lk["lead"] + lk["nsync"] + lk["at"]
    hit[:, b0:b0 + lk["run"]] ^= 3
    assert np.array_equal(hit, r["hit"])
    z = np.stack([dibits_to_costas(row, amp=lk["amp"]) for row in hit])
    m.deframer_reset_coded(P, r["sync"], n, lk["min_score"], max_packets=1, puncture=NAMED[lk["rate"]])
    gain = torch.full((P,), float(np.float32(64.0 / lk["amp"])), dtype=torch.float32, device="cuda")
    d = m.deframe_coded(torch.from_numpy(z).cuda(), gain)
    assert np.all(d["count"].cpu().numpy() == 1)
    assert np.array_equal(d["crc_ok"].cpu().numpy()[:, 0] != 0, r["crc_ok"]) and not r["crc_ok"].any()
    before = d["bytes"].cpu().numpy()
    assert np.array_equal(before[:, 0], r["bytes"])
    out = torch.full((P * n + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    info = torch.full((P * 4 + GUARD,), INFO_FILL, dtype=torch.int32, device="cuda")
    m._check(m.L.qpsk_rs_decode_batch(m.h, ptr(d["bytes"]), n + 2, P, n, n - k, None, ptr(out), 0, ptr(info)))
    m.sync()
    want_out, want_info = rs_decode_ref(r["bytes"][:, :n], n - k)
    ho, hi = out.cpu().numpy(), info.cpu().numpy()
    assert np.all(ho[P * n:] == OUT_FILL) and np.all(hi[P * 4:] == INFO_FILL)
    assert np.array_equal(ho[:P * n].reshape(P, n), want_out) and np.array_equal(hi[:P * 4].reshape(P, 4), want_info)
    assert np.array_equal(ho[:P * n].reshape(P, n)[:, :k], r["data"])
    assert np.array_equal(d["bytes"].cpu().numpy(), before)                     # the deframer's output was only read
    # and in place, the CRC bytes between the codewords untouched
    m._check(m.L.qpsk_rs_decode_batch(m.h, ptr(d["bytes"]), n + 2, P, n, n - k, None, ptr(d["bytes"]), n + 2, None))
    m.sync()
    after = d["bytes"].cpu().numpy()[:, 0]
    assert np.array_equal(after[:, :n], want_out) and np.array_equal(after[:, n:], before[:, 0, n:])
    m.close()


# ------------------------------------------------------------------------------------------ 7. the rare paths and the chunk seams
@pytest.mark.parametrize("n,k", directed_codes())
def test_the_directed_rows_of_a_code_in_one_call_bit_for_bit(n, k):
    """rows picked with the scalar port's trace for what a random draw does not reach (rs_rows.directed_rows): zero discrepancies inside
    Berlekamp-Massey, lengths that jump, repeated roots, roots among the missing bytes, words that fail the last check alone,
    miscorrections; decoded and failing rows in turn, so that the waves of a workgroup leave by different exits"""
    c = directed_rows(n, k)
    ok = c["erased"][1][:, 0] >= 0
    assert sum(bool(a) != bool(b) for a, b in zip(ok[:-1], ok[1:])) >= 8
    m = modem()
    got = decode(m, c["words"], n - k, c["flags"])
    assert got["kernel"] == "rs_decode_kernel"
    assert_rows(got, c["erased"], c["names"], "erasures")
    assert_rows(decode(m, c["words"], n - k, None), c["plain"], c["names"], "d_erase NULL")
    m.sync()
    m.close()


PITCHED_EDGE = (129, 121)
assert PITCHED_EDGE in edge_codes()


@pytest.mark.parametrize("n,k", edge_codes())
def test_the_edge_codes_decode_and_encode_bit_for_bit(n, k):
    """n on both sides of the 64-lane chunks' seams, errors and erasures on the seams (rs_rows.edge_rows), nroots 33 and 63"""
    c = edge_rows(n, k)
    m = modem()
    assert_rows(decode(m, c["words"], n - k, c["flags"]), c["erased"], c["names"], "erasures")
    assert_rows(decode(m, c["words"], n - k, None), c["plain"], c["names"], "d_erase NULL")
    if (n, k) == PITCHED_EDGE:
        for what, kw in (("pitched input", dict(in_pitch=n + 2)), ("in place", dict(inplace=True)), ("in place, pitched", dict(inplace=True, in_pitch=n + 3))):
            assert_rows(decode(m, c["words"], n - k, c["flags"], **kw), c["erased"], c["names"], what)
    (R, data), = encoder_rows(n, k, (5,))
    want = rs_encode_ref(data, n - k)
    for dp, op in ((0, 0), (k + 3, 0), (0, n + 2), (k + 1, n + 5)):
        assert np.array_equal(encode(m, data, n - k, dp, op), want), (dp, op)
    m.sync()
    m.close()


@pytest.mark.parametrize("n,k", edge_codes())
def test_the_edge_codes_rows_come_back_from_random_erasures(n, k):
    m = modem()
    encode_erase_decode(m, n, k)
    m.sync()
    m.close()
