"""qpsk_rs_cross_encode_batch / _decode_batch / _place_batch and Modem.rs_cross_encode / rs_cross_decode / rs_cross_place on the GPU, bit for
bit against the numpy restatements of test_cross_cpu.py (PACKET ERASURE CODE of include/qpsk_hip.h): every code with groups damaged in
every way in one call, so that neighbouring workgroups leave by different exits; the coded widths around the 64-column tile; pitches with
poison between the packets; missing packets filled with poison; in place, either output alone, d_colfail; the encoder; encode, drop,
decode; place; the error contract; and the link of the CPU test on the device with library calls only.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from test_deframe_coded_cpu import dibits_to_costas
from test_frame_cpu import ks_prefix
from test_cross_cpu import LINK, cross_decode_ref, cross_encode_ref, cross_place_ref, link_result, place_case
from test_viterbi_gpu import GUARD, modem, ptr

pytestmark = pytest.mark.gpu

QPSK_ERR_ARG = -2
POISON, OUT_FILL, INFO_FILL = 0xA5, 0x55, 0x55555555
CODES = ((3, 1), (6, 2), (12, 8), (65, 1), (255, 191), (255, 254))
SHAPES = ((1, 0), (63, 1), (64, 0), (65, 1), (257, 1), (1, 39))      # (coded width len - skip, skip); the last is skip = len - 1


# ------------------------------------------------------------------------------------------ the groups of one code, and their reference
def damage(n, k, G, ln, skip, seed, fill=None, first=0):
    """G encoded groups, group i damaged by pattern (first + i) % 9 -> (groups, have, sent).  A missing packet is overwritten, header and
    all, with `fill` (None: random bytes, some of them right by chance).  Which packets are missing depends on the code and the pattern
    only, so that the shapes of one code share the reference's eliminations"""
    nroots = n - k
    rng = np.random.default_rng(seed)
    sent = cross_encode_ref(rng.integers(0, 256, (G, n, ln), dtype=np.uint8), nroots, skip)
    groups, have = sent.copy(), np.ones((G, n), np.uint8)
    col = skip + (ln - skip) // 2
    for i in range(G):
        kind = (first + i) % 9
        pick = np.random.default_rng(1000 * n + k + 17 * kind)
        f = (0, 1, nroots, nroots + 1, nroots, min(nroots, k), max(nroots - 1, 0), nroots, nroots)[kind]
        f = min(f, n)
        if kind == 4:
            miss = np.arange(n - f, n)                               # only among the parity
        elif kind == 5:
            miss = pick.choice(k, f, replace=False)                  # only among the data
        elif kind == 8:
            miss = np.arange(f)                                      # the first packets: at n = 255 their locators meet the register's
        else:
            miss = pick.choice(n, f, replace=False)
        have[i, miss] = 0
        groups[i, miss] = rng.integers(0, 256, (f, ln), dtype=np.uint8) if fill is None else fill
        if kind in (6, 7) and f < n:                                 # a wrong byte in a present packet, in one column
            groups[i, np.nonzero(have[i])[0][i % (n - f)], col] ^= 0x5A
    return groups, have, sent


_CASES = {}


def case(n, k, G, ln, skip, first=0):
    """a damaged call with its reference, computed once and shared; nobody changes them"""
    key = (n, k, G, ln, skip, first)
    if key not in _CASES:
        groups, have, sent = damage(n, k, G, ln, skip, seed=1000003 * n + 1009 * k + 101 * G + 7 * ln + skip + first, first=first)
        ref = cross_decode_ref(groups, have, n - k, skip)
        for a in (groups, have, sent) + ref:
            a.setflags(write=False)
        _CASES[key] = dict(groups=groups, have=have, sent=sent, ref=ref)
    return _CASES[key]


def decode(m, groups, have, nroots, skip, pitch=0, out_pitch=0, inplace=False, want=("out", "info", "colfail")):
    """the raw call: pitched buffers with POISON between the packets, GUARD elements behind every output -> dict(out, info, colfail,
    kernel); an output that was not asked for is passed as NULL"""
    import torch
    G, n, ln = groups.shape
    ip, op = pitch or ln, (pitch or ln) if inplace else (out_pitch or ln)
    src = np.full((G, n, ip), POISON, np.uint8)
    src[:, :, :ln] = groups
    d_in = torch.from_numpy(np.concatenate([src.reshape(-1), np.full(GUARD, POISON, np.uint8)])).cuda()
    d_have = torch.from_numpy(np.array(have, np.uint8)).cuda()
    d_out = d_in if inplace else torch.full((G * n * op + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    d_info = torch.full((G * 4 + GUARD,), INFO_FILL, dtype=torch.int32, device="cuda")
    d_cf = torch.full((G * (ln - skip) + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    m._check(m.L.qpsk_rs_cross_decode_batch(m.h, ptr(d_in), pitch, G, n, nroots, ln, skip, ptr(d_have), ptr(d_out) if "out" in want else None,
                                            pitch if inplace else out_pitch, ptr(d_info) if "info" in want else None,
                                            ptr(d_cf) if "colfail" in want else None))
    kernel = m.last_kernel()
    torch.cuda.synchronize()
    ho, hi, hc, hin = d_out.cpu().numpy(), d_info.cpu().numpy(), d_cf.cpu().numpy(), d_in.cpu().numpy()
    fill = POISON if inplace else OUT_FILL
    assert np.all(ho[G * n * op:] == fill) and np.all(hi[G * 4:] == INFO_FILL) and np.all(hc[G * (ln - skip):] == OUT_FILL), "a guard was overwritten"
    pk = ho[:G * n * op].reshape(G, n, op)
    assert np.all(pk[:, :, ln:] == fill), "bytes between the output's packets were written"
    if "out" not in want:
        assert inplace or np.all(ho == fill)
    if "info" not in want:
        assert np.all(hi == INFO_FILL)
    if "colfail" not in want:
        assert np.all(hc == OUT_FILL)
    if not inplace or "out" not in want:
        assert np.array_equal(hin[:G * n * ip].reshape(G, n, ip), src), "the input was written"
    assert np.array_equal(d_have.cpu().numpy(), have)
    return dict(out=pk[:, :, :ln], info=hi[:G * 4].reshape(G, 4), colfail=hc[:G * (ln - skip)].reshape(G, ln - skip), kernel=kernel)


def assert_groups(got, ref, what, want=("out", "info", "colfail")):
    for key, r in zip(("out", "info", "colfail"), ref):
        if key in want:
            for i in range(len(r)):
                assert np.array_equal(got[key][i], r[i]), (what, key, i, got["info"][i] if "info" in want else None, ref[1][i])


# ------------------------------------------------------------------------------------------ 1. every code, every damage, every width
@pytest.mark.parametrize("width,skip", SHAPES)
@pytest.mark.parametrize("n,k", CODES)
def test_every_damage_of_a_code_in_one_call_bit_for_bit(n, k, width, skip):
    c = case(n, k, 9, width + skip, skip)
    nroots, (out, info, colfail) = n - k, c["ref"]
    # the reference itself says what the patterns were built for
    assert tuple(info[0]) == (0, 0, 0, 1) and info[3, 0] == width and info[3, 1] == min(nroots + 1, n) > nroots
    for i in (1, 2, 4, 5, 8):
        assert info[i, 0] == 0 and np.array_equal(out[i, :, skip:], c["sent"][i, :, skip:]), (i, info[i])
    assert info[6, 0] == 1 and colfail[6].sum() == 1 and colfail[6, width // 2] == 1           # the wrong byte's column alone fails
    assert info[7, 0] == 0 and not np.array_equal(out[7], c["sent"][7])                        # at f = nroots it is invisible
    m = modem()
    got = decode(m, c["groups"], c["have"], nroots, skip)
    assert got["kernel"] == "rs_cross_decode_kernel"
    assert_groups(got, c["ref"], "tight")
    assert_groups(decode(m, c["groups"], c["have"], nroots, skip, inplace=True, pitch=width + skip + 3), c["ref"], "in place, pitched")
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 2. the call shapes
@pytest.mark.parametrize("n,k", [(12, 8), (65, 1)])
@pytest.mark.parametrize("G", [1, 5, 70])
def test_group_counts_pitches_in_place_and_either_output_alone(n, k, G):
    ln, skip = 70, 1
    c = case(n, k, G, ln, skip, first=2)
    m = modem()
    for what, kw in (("tight", {}), ("pitched input", dict(pitch=ln + 2)), ("pitched output", dict(out_pitch=ln + 7)),
                     ("both pitched", dict(pitch=ln + 1, out_pitch=ln + 3)), ("in place", dict(inplace=True)),
                     ("in place, pitched", dict(inplace=True, pitch=ln + 2))):
        assert_groups(decode(m, c["groups"], c["have"], n - k, skip, **kw), c["ref"], what)
    for want in (("info",), ("out",), ("out", "info"), ("info", "colfail")):
        assert_groups(decode(m, c["groups"], c["have"], n - k, skip, pitch=ln + 2, out_pitch=ln + 5, want=want), c["ref"], want, want)
    assert_groups(decode(m, c["groups"], c["have"], n - k, skip, inplace=True, want=("out",)), c["ref"], "in place, out alone", ("out",))
    m.sync()
    m.close()


@pytest.mark.parametrize("n,k", [(12, 8), (255, 191)])
def test_missing_packets_are_not_read_for_the_result_whatever_fills_them(n, k):
    """the same groups with the missing packets filled with 0xA5, with 0x00 and with random bytes: each equals its reference, and wherever
    no column failed the three outputs are the same bytes"""
    ln, skip, G = 67, 1, 9
    m = modem()
    outs = []
    for fill in (0xA5, 0x00, None):
        groups, have, sent = damage(n, k, G, ln, skip, seed=31 * n + k, fill=fill)
        ref = cross_decode_ref(groups, have, n - k, skip)
        got = decode(m, groups, have, n - k, skip)
        assert_groups(got, ref, fill)
        outs.append((got, have, sent))
    (a, have, sent), (b, _, _), (r, _, _) = outs
    whole = a["info"][:, 0] == 0
    assert whole.sum() >= 6 and np.array_equal(a["info"][:, :2], b["info"][:, :2]) and np.array_equal(a["colfail"], b["colfail"])
    for i in np.nonzero(whole)[0]:
        assert np.array_equal(a["out"][i, :, skip:], b["out"][i, :, skip:]) and np.array_equal(a["out"][i, :, skip:], r["out"][i, :, skip:]), i
        if i % 9 != 7:                                               # (pattern 7 carries a wrong present byte, which stays)
            assert np.array_equal(a["out"][i][have[i] != 0], sent[i][have[i] != 0])
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 3. the encoder
def encode(m, groups, nroots, skip, pitch=0):
    import torch
    G, n, ln = groups.shape
    ip = pitch or ln
    src = np.full((G, n, ip), POISON, np.uint8)
    src[:, :, :ln] = groups
    d = torch.from_numpy(np.concatenate([src.reshape(-1), np.full(GUARD, POISON, np.uint8)])).cuda()
    m._check(m.L.qpsk_rs_cross_encode_batch(m.h, ptr(d), pitch, G, n - nroots, nroots, ln, skip))
    assert m.last_kernel() == "rs_cross_encode_kernel"
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    assert np.all(h[G * n * ip:] == POISON), "the guard behind the groups was overwritten"
    pk = h[:G * n * ip].reshape(G, n, ip)
    assert np.all(pk[:, :, ln:] == POISON), "bytes between the packets were written"
    return pk[:, :, :ln]


@pytest.mark.parametrize("n,k", CODES)
def test_encoder_equals_the_restatement_for_every_width_group_count_and_pitch(n, k):
    m = modem()
    rng = np.random.default_rng(n * 300 + k)
    for (width, skip), G in zip(SHAPES, (5, 1, 70, 5, 5, 5)):
        ln = width + skip
        groups = rng.integers(0, 256, (G, n, ln), dtype=np.uint8)      # the parity packets start as garbage: it is overwritten, their headers stay
        groups[0, :k] = 0xFF
        groups[G // 2, :k] = 0
        want = cross_encode_ref(groups, n - k, skip)
        assert np.array_equal(want[:, :, :skip], groups[:, :, :skip]) and np.array_equal(want[:, :k], groups[:, :k])
        for pitch in (0, ln + 3):
            assert np.array_equal(encode(m, groups, n - k, skip, pitch), want), (width, skip, G, pitch)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 4. encode, drop, decode: the Python front end
@pytest.mark.parametrize("n,k", CODES)
def test_the_encoder_s_groups_come_back_from_random_losses_of_up_to_nroots_packets(n, k):
    import torch
    m = modem()
    nroots, G, ln, skip = n - k, 33, 45, 2
    rng = np.random.default_rng(n + 7 * k)
    dev = torch.from_numpy(rng.integers(0, 256, (G, n, ln), dtype=np.uint8)).cuda()
    enc = m.rs_cross_encode(dev, nroots, skip=skip)
    assert enc.data_ptr() == dev.data_ptr() and tuple(enc.shape) == (G, n, ln)
    sent = enc.cpu().numpy()
    have, hit = np.ones((G, n), np.uint8), sent.copy()
    for g in range(G):
        f = nroots if g == 0 else int(rng.integers(0, nroots + 1))
        at = rng.choice(n, f, replace=False)
        have[g, at] = 0
        hit[g, at, skip:] = rng.integers(0, 256, (f, ln - skip), dtype=np.uint8)
    out, info = m.rs_cross_decode(hit, have, nroots, skip=skip)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(out, sent)
    want = np.stack([np.zeros(G), (have == 0).sum(axis=1), (hit != sent).sum(axis=(1, 2)), np.ones(G)], axis=1)
    assert np.array_equal(info, want)
    d_hit = torch.from_numpy(hit).cuda()
    same, info2 = m.rs_cross_decode(d_hit, have, nroots, skip=skip, inplace=True)
    assert same.data_ptr() == d_hit.data_ptr() and np.array_equal(d_hit.cpu().numpy(), sent) and np.array_equal(info2.cpu().numpy(), want)
    with pytest.raises(ValueError):
        m.rs_cross_decode(hit, have, nroots, skip=skip, inplace=True)             # a numpy array cannot be decoded in place
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 5. place
def test_place_equals_the_restatement_with_pitches_poison_and_accumulation():
    import torch
    c = place_case()
    S, M, row = c["bytes"].shape
    n, ngroups, ln = c["n"], c["ngroups"], c["len"]
    m = modem()
    for pitch, with_base in ((0, True), (ln + 4, True), (0, False)):
        gp = pitch or ln
        g0 = np.full((S, ngroups, n, gp), POISON, np.uint8)
        h0 = np.zeros((S, ngroups * n), np.uint8)
        h0[2, 4] = 1
        d_g = torch.from_numpy(np.concatenate([g0.reshape(-1), np.full(GUARD, POISON, np.uint8)])).cuda()
        d_h = torch.from_numpy(np.concatenate([h0.reshape(-1), np.full(GUARD, POISON, np.uint8)])).cuda()
        d_b, d_c, d_ok = (torch.from_numpy(c[key]).cuda() for key in ("bytes", "count", "crc_ok"))
        d_base = torch.from_numpy(c["base"]).cuda() if with_base else None
        m._check(m.L.qpsk_rs_cross_place_batch(m.h, ptr(d_b), row, ptr(d_c), ptr(d_ok), S, M, ln, n, ngroups, ptr(d_base), ptr(d_g), pitch, ptr(d_h)))
        assert m.last_kernel() == "rs_cross_place_kernel"
        torch.cuda.synchronize()
        want_g, want_h = cross_place_ref(c["bytes"], c["count"], c["crc_ok"], n, ngroups, c["base"] if with_base else None, g0[..., :ln], h0)
        hg, hh = d_g.cpu().numpy(), d_h.cpu().numpy()
        assert np.all(hg[g0.size:] == POISON) and np.all(hh[h0.size:] == POISON), "a guard was overwritten"
        pk = hg[:g0.size].reshape(S, ngroups, n, gp)
        assert np.all(pk[..., ln:] == POISON), "bytes between the packets were written"
        assert np.array_equal(pk[..., :ln], want_g) and np.array_equal(hh[:h0.size].reshape(S, -1), want_h), (pitch, with_base)
        assert np.array_equal(d_b.cpu().numpy(), c["bytes"]) and np.array_equal(d_c.cpu().numpy(), c["count"])
    # the front end: fresh buffers take the whole row; given ones are accumulated into, over two pushes
    groups, have = m.rs_cross_place(c["bytes"], c["count"], c["crc_ok"], n, ngroups, base=c["base"])
    want_g, want_h = cross_place_ref(c["bytes"], c["count"], c["crc_ok"], n, ngroups, c["base"])
    assert tuple(groups.shape) == (S, ngroups, n, row) and np.array_equal(groups.cpu().numpy(), want_g) and np.array_equal(have.cpu().numpy(), want_h)
    acc_g = torch.zeros((S, ngroups, n, ln), dtype=torch.uint8, device="cuda")
    acc_h = torch.zeros((S, ngroups * n), dtype=torch.uint8, device="cuda")
    second = c["bytes"][:, ::-1].copy()
    second[:, :, 0] = (second[:, :, 0].astype(np.int64) + 3) & 255
    for b in (c["bytes"], second):
        g2, h2 = m.rs_cross_place(b, c["count"], c["crc_ok"], n, ngroups, base=c["base"], groups=acc_g, have=acc_h)
        assert g2.data_ptr() == acc_g.data_ptr() and h2.data_ptr() == acc_h.data_ptr()
    w_g, w_h = cross_place_ref(c["bytes"], c["count"], c["crc_ok"], n, ngroups, c["base"], length=ln)
    w_g, w_h = cross_place_ref(second, c["count"], c["crc_ok"], n, ngroups, c["base"], w_g, w_h)
    assert np.array_equal(acc_g.cpu().numpy(), w_g) and np.array_equal(acc_h.cpu().numpy(), w_h)
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 6. the error contract
def test_every_bad_argument_is_refused_with_nothing_written_and_the_context_stays_usable():
    import torch
    c = case(12, 8, 5, 70, 1, first=2)
    m = modem()
    G, n, nroots, ln, skip = 5, 12, 4, 70, 1
    d_in = torch.from_numpy(c["groups"].copy()).cuda()
    d_have = torch.from_numpy(c["have"].copy()).cuda()
    d_out = torch.full((G * n * ln + 256,), OUT_FILL, dtype=torch.uint8, device="cuda")
    d_info = torch.full((G * 4 + 8,), INFO_FILL, dtype=torch.int32, device="cuda")
    d_cf = torch.full((G * ln,), OUT_FILL, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((8,), 2, dtype=torch.int32, device="cuda")
    d_ok = torch.ones((64,), dtype=torch.uint8, device="cuda")
    before = m.last_kernel()
    L, h = m.L, m.h
    at = lambda t, off: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    dec = lambda **kw: L.qpsk_rs_cross_decode_batch(*[kw.get(key, dflt) for key, dflt in (      # noqa: E731
        ("ctx", h), ("grp", ptr(d_in)), ("pitch", 0), ("G", G), ("n", n), ("nroots", nroots), ("len", ln), ("skip", skip), ("have", ptr(d_have)),
        ("out", ptr(d_out)), ("op", 0), ("info", ptr(d_info)), ("cf", ptr(d_cf)))])
    enc = lambda **kw: L.qpsk_rs_cross_encode_batch(*[kw.get(key, dflt) for key, dflt in (      # noqa: E731
        ("ctx", h), ("grp", ptr(d_out)), ("pitch", 0), ("G", G), ("k", 8), ("nroots", nroots), ("len", ln), ("skip", skip))])
    plc = lambda **kw: L.qpsk_rs_cross_place_batch(*[kw.get(key, dflt) for key, dflt in (       # noqa: E731
        ("ctx", h), ("bytes", ptr(d_in)), ("bp", 0), ("cnt", ptr(d_cnt)), ("ok", ptr(d_ok)), ("S", 2), ("M", 4), ("len", ln), ("n", n), ("ng", 2),
        ("base", None), ("grp", ptr(d_out)), ("pitch", 0), ("have", ptr(d_cf)))])
    calls = {
        "qpsk_rs_cross_decode_batch": [
            ("null context", lambda: dec(ctx=None)), ("null groups", lambda: dec(grp=None)), ("null have", lambda: dec(have=None)),
            ("both outputs null", lambda: dec(out=None, info=None)), ("ngroups 0", lambda: dec(G=0)), ("ngroups negative", lambda: dec(G=-1)),
            ("nroots 0", lambda: dec(nroots=0)), ("nroots 65", lambda: dec(n=130, nroots=65)), ("k = 0", lambda: dec(n=4)),
            ("n = 256", lambda: dec(n=256, nroots=32)), ("len 0", lambda: dec(len=0, skip=0)), ("skip = len", lambda: dec(skip=ln)),
            ("skip negative", lambda: dec(skip=-1)), ("pitch below len", lambda: dec(pitch=ln - 1)), ("pitch negative", lambda: dec(pitch=-ln)),
            ("out_pitch below len", lambda: dec(op=ln - 1)), ("a pitch that leaves 64 bits", lambda: dec(op=1 << 62)),
            ("in place with another pitch", lambda: dec(grp=ptr(d_out), op=ln + 1)),
            ("output one byte into the input", lambda: dec(grp=ptr(d_out), out=at(d_out, 1))),
            ("output overlaps the input's tail", lambda: dec(grp=ptr(d_out), out=at(d_out, G * n * ln - 1))),
            ("info misaligned", lambda: dec(info=at(d_info, 2))), ("info inside the output", lambda: dec(info=at(d_out, 16))),
            ("info inside the input", lambda: dec(grp=ptr(d_out), out=None, info=at(d_out, 16))),
            ("have inside the output", lambda: dec(have=at(d_out, 8))), ("colfail inside the output", lambda: dec(cf=at(d_out, 8))),
            ("colfail over have", lambda: dec(cf=ptr(d_have))), ("colfail inside info", lambda: dec(cf=at(d_info, 4))),
        ],
        "qpsk_rs_cross_encode_batch": [
            ("null context", lambda: enc(ctx=None)), ("null groups", lambda: enc(grp=None)), ("ngroups 0", lambda: enc(G=0)),
            ("k 0", lambda: enc(k=0)), ("nroots 0", lambda: enc(nroots=0)), ("nroots 65", lambda: enc(k=16, nroots=65)),
            ("k + nroots = 256", lambda: enc(k=192, nroots=64)), ("len 0", lambda: enc(len=0, skip=0)), ("skip = len", lambda: enc(skip=ln)),
            ("skip negative", lambda: enc(skip=-1)), ("pitch below len", lambda: enc(pitch=ln - 1)), ("pitch negative", lambda: enc(pitch=-ln)),
        ],
        "qpsk_rs_cross_place_batch": [
            ("null context", lambda: plc(ctx=None)), ("null bytes", lambda: plc(bytes=None)), ("null count", lambda: plc(cnt=None)),
            ("null crc_ok", lambda: plc(ok=None)), ("null groups", lambda: plc(grp=None)), ("null have", lambda: plc(have=None)),
            ("nstreams 0", lambda: plc(S=0)), ("max_packets 0", lambda: plc(M=0)), ("len 0", lambda: plc(len=0)), ("n 0", lambda: plc(n=0)),
            ("n 256", lambda: plc(n=256, ng=1)), ("ngroups 0", lambda: plc(ng=0)), ("a window of 257", lambda: plc(n=1, ng=257)),
            ("a window of 264", lambda: plc(n=12, ng=22)), ("byte_pitch below len", lambda: plc(bp=ln - 1)),
            ("pitch below len", lambda: plc(pitch=ln - 1)), ("count misaligned", lambda: plc(cnt=at(d_cnt, 2))),
            ("base misaligned", lambda: plc(base=at(d_cnt, 18))), ("groups over the bytes", lambda: plc(grp=ptr(d_in))),
            ("have inside the groups", lambda: plc(have=at(d_out, 5))), ("have over crc_ok", lambda: plc(have=ptr(d_ok))),
            ("groups over the count", lambda: plc(grp=ptr(d_cnt))),
        ],
    }
    for who, bad in calls.items():
        for what, call in bad:
            assert call() == QPSK_ERR_ARG, (who, what)
            assert who.encode() in L.qpsk_last_error(), (who, what)
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == OUT_FILL) and np.all(d_info.cpu().numpy() == INFO_FILL) and np.all(d_cf.cpu().numpy() == OUT_FILL)
    assert np.array_equal(d_in.cpu().numpy(), c["groups"]) and np.array_equal(d_have.cpu().numpy(), c["have"]) and np.all(d_cnt.cpu().numpy() == 2)
    assert m.last_kernel() == before                                            # nothing was launched
    with pytest.raises(ValueError):
        m.rs_cross_decode(c["groups"].copy(), c["have"][:, :5], nroots)
    m.sync()                                                                    # no call raised the context's status word
    got = decode(m, c["groups"], c["have"], nroots, skip)
    assert_groups(got, c["ref"], "after the refusals")
    assert c["ref"][1][:, 0].any()                                              # ... and failed columns do not raise it either
    m.sync()
    m.close()


def test_decode_buffers_that_touch_are_accepted_and_one_shared_byte_is_refused():
    """2 groups of (6, 4), len 70, skip 2 (two column tiles, one partial) inside one allocation: 12 packets span 840 bytes tight and
    11 * 80 + 70 = 950 at pitch 80 -- the padding behind the last packet is not the buffer.  d_have is 12 bytes, d_info 32, d_colfail 136.
    Every pair the call compares, with the later range on the byte behind the earlier one's last (accepted, every output the reference's) and
    on that last byte (refused, with the present text); d_info is 4-byte aligned, so it is its neighbour that moves"""
    import torch
    G, n, nroots, ln, skip = 2, 6, 2, 70, 2
    c = case(n, n - nroots, G, ln, skip, first=1)
    m = modem()
    L, h = m.L, m.h
    arena = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    at = lambda off: None if off is None else C.c_void_p(arena.data_ptr() + off)      # noqa: E731

    def dec(i=1000, ip=0, o=2000, op=0, hv=3000, f=3100, cf=3200):
        host = np.zeros(4096, np.uint8)
        p = ip or ln
        for r in range(G * n):
            host[i + r * p:i + r * p + ln] = c["groups"].reshape(G * n, ln)[r]
        host[hv:hv + G * n] = c["have"].reshape(-1)
        arena.copy_(torch.from_numpy(host))
        rc = L.qpsk_rs_cross_decode_batch(h, at(i), ip, G, n, nroots, ln, skip, at(hv), at(o), op, at(f), at(cf))
        torch.cuda.synchronize()
        return rc

    accepted = (dict(o=1840), dict(o=160), dict(ip=80, o=1950), dict(op=80, o=50), dict(hv=988), dict(hv=1840), dict(hv=1988), dict(hv=2840),
                dict(f=968), dict(f=1840), dict(f=1968), dict(f=2840), dict(cf=864), dict(cf=1840), dict(cf=1864), dict(cf=2840),
                dict(hv=3088), dict(hv=3132), dict(hv=3188), dict(hv=3336), dict(f=3168), dict(f=3336), dict(o=1000), dict(ip=80, op=80, o=1000),
                dict(o=None), dict(f=None), dict(cf=None), dict(f=None, cf=None))
    for kw in accepted:
        assert dec(**kw) == 0, (kw, L.qpsk_last_error())
        host = arena.cpu().numpy()
        o, op, f, cf = kw.get("o", 2000), kw.get("op", 0) or ln, kw.get("f", 3100), kw.get("cf", 3200)
        if o is not None:
            assert np.array_equal(np.stack([host[o + r * op:o + r * op + ln] for r in range(G * n)]).reshape(G, n, ln), c["ref"][0]), kw
        if f is not None:
            assert np.array_equal(host[f:f + 16 * G].view(np.int32).reshape(G, 4), c["ref"][1]), kw
        if cf is not None:
            assert np.array_equal(host[cf:cf + G * (ln - skip)].reshape(G, ln - skip), c["ref"][2]), kw
    io, side = b"d_out overlaps d_group (allowed", b" overlaps d_group or d_out"
    refused = ((dict(o=1839), io), (dict(o=161), io), (dict(ip=80, o=1949), io), (dict(op=80, o=51), io), (dict(o=1000, op=80), io),
               (dict(hv=989), b"d_have" + side), (dict(hv=1839), b"d_have" + side), (dict(hv=1989), b"d_have" + side), (dict(hv=2839), b"d_have" + side),
               (dict(i=999, f=968), b"d_info" + side), (dict(i=1001, f=1840), b"d_info" + side), (dict(o=1999, f=1968), b"d_info" + side),
               (dict(o=2001, f=2840), b"d_info" + side), (dict(cf=865), b"d_colfail" + side), (dict(cf=1839), b"d_colfail" + side),
               (dict(cf=1865), b"d_colfail" + side), (dict(cf=2839), b"d_colfail" + side), (dict(hv=3089), b"d_info overlaps d_have"),
               (dict(hv=3131), b"d_info overlaps d_have"), (dict(hv=3189), b"d_colfail overlaps d_have"), (dict(hv=3335), b"d_colfail overlaps d_have"),
               (dict(cf=3131), b"d_colfail overlaps d_info"), (dict(cf=2965, hv=3500), b"d_colfail overlaps d_info"))
    for kw, text in refused:
        assert dec(**kw) == QPSK_ERR_ARG and b"qpsk_rs_cross_decode_batch: " + text in L.qpsk_last_error(), (kw, L.qpsk_last_error())
    m.sync()
    m.close()


def test_place_buffers_that_touch_are_accepted_and_one_shared_byte_is_refused():
    """2 streams of 3 slots of 6 bytes at byte_pitch 8 (5 * 8 + 6 = 46 bytes) into windows of 2 groups of 3 at pitch 8 (11 * 8 + 6 = 94
    bytes), all inside one allocation: each output in front of and behind each input and the other output, touching (accepted, groups and
    d_have the reference's) and one byte further in (refused, with the present text).  d_base is given only where it is the input in question"""
    import torch
    rng = np.random.default_rng(8)
    S, M, ln, n, ng, P = 2, 3, 6, 3, 2, 8
    byts = rng.integers(0, 256, (S, M, P), dtype=np.uint8)
    byts[0, :, 0], byts[1, :, 0] = (0, 4, 5), (11, 12, 19)
    byts[:, :, ln:] = 0      # the padding: an output may begin in the last row's, and the call never clears
    count, crc_ok, base = np.array([3, 3], np.int32), np.array([[1, 1, 1], [1, 0, 1]], np.uint8), np.array([0, 10 + 256], np.int32)
    wants = {False: cross_place_ref(byts, count, crc_ok, n, ng, None, length=ln), True: cross_place_ref(byts, count, crc_ok, n, ng, base, length=ln)}
    assert wants[False][1].tolist() == [[1, 0, 0, 0, 1, 1], [0] * 6] and wants[True][1].tolist() == [[1, 0, 0, 0, 1, 1], [0, 1, 0, 0, 0, 0]]
    m = modem()
    L, h = m.L, m.h
    arena = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    at = lambda off: None if off is None else C.c_void_p(arena.data_ptr() + off)      # noqa: E731
    ins = dict(d_bytes=(1000, 46), d_count=(1200, 8), d_crc_ok=(1500, 6), d_base=(1800, 8))
    outs = dict(d_group=(2400, 94), d_have=(2600, 12))

    def place(grp=2400, hv=2600, with_base=False):
        host = np.zeros(4096, np.uint8)
        host[1000:1048] = byts.reshape(-1)
        host[1200:1208], host[1500:1506], host[1800:1808] = count.view(np.uint8), crc_ok.reshape(-1), base.view(np.uint8)
        arena.copy_(torch.from_numpy(host))
        rc = L.qpsk_rs_cross_place_batch(h, at(1000), P, at(1200), at(1500), S, M, ln, n, ng, at(1800) if with_base else None, at(grp), P, at(hv))
        torch.cuda.synchronize()
        if rc == 0:
            host = arena.cpu().numpy()
            groups = np.stack([host[grp + r * P:grp + r * P + ln] for r in range(S * ng * n)]).reshape(S, ng, n, ln)
            assert np.array_equal(groups, wants[with_base][0]) and np.array_equal(host[hv:hv + S * ng * n].reshape(S, ng * n), wants[with_base][1])
        return rc

    assert place() == 0 and place(with_base=True) == 0, L.qpsk_last_error()
    pairs = [(o, i, i == "d_base") for o in outs for i in ins] + [("d_have", "d_group", False)]
    for o, i, with_base in pairs:
        (start, size), mine = {**ins, **outs}[i], outs[o][1]
        for off, accepted in ((start - mine, True), (start + size, True), (start - mine + 1, False), (start + size - 1, False)):
            rc = place(with_base=with_base, **{"grp" if o == "d_group" else "hv": off})
            if accepted:
                assert rc == 0, (o, i, off, L.qpsk_last_error())
            else:
                assert rc == QPSK_ERR_ARG and ("qpsk_rs_cross_place_batch: %s overlaps %s" % (o, i)).encode() in L.qpsk_last_error(), (o, i, off, L.qpsk_last_error())
    m.sync()
    m.close()


# ------------------------------------------------------------------------------------------ 7. the link of the CPU test, on the device
def test_the_cpu_link_on_the_device_with_library_calls_only():
    """Modem.rs_cross_encode -> Modem.frame -> the CPU test's lost rows and inverted runs -> costas_frame[] rows -> Modem.deframe_coded ->
    Modem.rs_cross_place -> Modem.rs_cross_decode: every stage equals the CPU link test's, and the groups with at most nroots packets
    missing come back complete"""
    import torch
    lk, r = LINK, link_result()
    n, k, nb, G, skip = lk["n"], lk["k"], lk["nbytes"], lk["ngroups"], lk["skip"]
    m = modem()
    groups = r["sent"].copy()
    groups[:, k:, skip:] = 0x77                                                   # the parity is the encoder's to fill
    enc = m.rs_cross_encode(torch.from_numpy(groups).cuda(), n - k, skip=skip)
    assert np.array_equal(enc.cpu().numpy(), r["sent"])
    o = m.frame(enc.reshape(G * n, nb), r["sync"], coded=True, per_row=1, lead=lk["lead"], gap=0)
    rows = o["dibits"].cpu().numpy()
    assert np.array_equal(rows, r["rows"])
    hit = rows.copy()
    b0 = lk["lead"] + lk["nsync"] + lk["at"]
    for g, places in lk["lost"].items():
        for p in places:
            hit[g * n + p] = ks_prefix(rows.shape[1])                             # the whole row is idle fill
    for g, places in lk["broken"].items():
        for p in places:
            hit[g * n + p, b0:b0 + lk["run"]] ^= 3
    assert np.array_equal(hit, r["hit"])
    z = dibits_to_costas(hit.reshape(-1), amp=lk["amp"])
    M = G * n
    m.deframer_reset_coded(1, r["sync"], nb, lk["min_score"], max_packets=M)
    gain = torch.full((1,), float(np.float32(64.0 / lk["amp"])), dtype=torch.float32, device="cuda")
    d = m.deframe_coded(torch.from_numpy(z[None]).cuda(), gain)
    cnt = int(d["count"].cpu().numpy()[0])
    assert cnt == r["bytes"].shape[1]
    assert np.array_equal(d["bytes"].cpu().numpy()[0, :cnt], r["bytes"][0]) and np.array_equal(d["crc_ok"].cpu().numpy()[0, :cnt], r["crc_ok"][0])
    base = torch.full((1,), lk["base"], dtype=torch.int32, device="cuda")
    acc = torch.zeros((1, G, n, nb), dtype=torch.uint8, device="cuda")
    placed, have = m.rs_cross_place(d["bytes"], d["count"], d["crc_ok"], n, G, base=base, groups=acc)
    assert np.array_equal(placed.cpu().numpy(), r["groups"]) and np.array_equal(have.cpu().numpy(), r["have"])
    out, info = m.rs_cross_decode(placed[0], have.reshape(G, n), n - k, skip=skip)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(out, r["out"]) and np.array_equal(info, r["info"])
    for g in (0, 2):
        assert np.array_equal(out[g, :k, skip:], r["sent"][g, :k, skip:])         # every data byte
    assert tuple(info[1]) == (nb - skip, 5, 0, 0) and np.array_equal(out[1], r["groups"][0, 1])
    m.sync()
    m.close()
