"""The packet erasure code (PACKET ERASURE CODE in include/qpsk_hip.h: qpsk_rs_cross_encode_batch, qpsk_rs_cross_decode_batch,
qpsk_rs_cross_place_batch): what can be checked without a GPU.

The restatements below are the header's definition in numpy, in integers.  cross_decode_ref is NOT the kernel's algorithm (a shift
register, then one matrix per group built from the locator of the missing places): here the k first present places of a column determine
a codeword through the generator matrix, by elimination, and the column is accepted iff that codeword equals the column in EVERY present
place.  It is not a call of test_rs_cpu's rs_decode_ref either; section 2 pins it to that decoder by the header's relation (equal where
rs_decode_ref reports e = 0, failed where it reports e > 0 or fails) and to the codebook decoder of four small codes.  The GPU tests
(test_cross_gpu.py) compare the kernels with these functions bit for bit.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_deframe_coded_cpu import deframe_coded_ref, dibits_to_costas, flat
from test_frame_cpu import HALF, body_len, frame_ref, ks_prefix
from test_rs_cpu import BOOK_CODES, codebook_decode, gf_inv, gf_mul, rs_decode_ref, rs_encode_ref, rs_syndromes
from test_rx_ext_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS_SYMBOLS = ("qpsk_rs_cross_encode_batch", "qpsk_rs_cross_decode_batch", "qpsk_rs_cross_place_batch")
CROSS_KERNELS = ("rs_cross_encode_kernel", "rs_cross_decode_kernel", "rs_cross_place_kernel")
QPSK_ERR_ARG = -2


# ------------------------------------------------------------------- the numpy restatement
def cross_encode_ref(groups, nroots, skip=0):
    """groups (G, n, len) uint8 -> a copy whose parity packets' bytes [skip, len) make every column a codeword of (n, n - nroots)"""
    g = np.array(groups, np.uint8)
    G, n, ln = g.shape
    k = n - nroots
    assert k >= 1 and 0 <= skip < ln
    for i in range(G):
        g[i, :, skip:] = rs_encode_ref(g[i, :k, skip:].T, nroots).T
    return g


_GEN, _INV = {}, {}


def generator_matrix(n, k):
    """(k, n): row m is the codeword of the m-th unit data word, so c = sum_m d[m] row m"""
    if (n, k) not in _GEN:
        _GEN[(n, k)] = rs_encode_ref(np.eye(k, dtype=np.uint8), n - k).astype(np.int64)
    return _GEN[(n, k)]


def gf_matmul(A, B):
    """(r, m) x (m, c) over the field"""
    A, B = np.asarray(A, np.int64), np.asarray(B, np.int64)
    out = np.zeros((A.shape[0], B.shape[1]), np.int64)
    for m in range(A.shape[1]):
        out ^= gf_mul(A[:, m:m + 1], B[m:m + 1, :])
    return out


def gf_inverse(A):
    """Gauss-Jordan elimination on [A | I]; A (m, m) must be non-singular"""
    m = len(A)
    M = np.concatenate([np.asarray(A, np.int64), np.eye(m, dtype=np.int64)], axis=1)
    for c in range(m):
        p = c + int(np.nonzero(M[c:, c])[0][0])
        M[[c, p]] = M[[p, c]]
        M[c] = gf_mul(M[c], gf_inv(M[c, c]))
        factor = M[:, c].copy()
        factor[c] = 0
        M ^= gf_mul(factor[:, None], M[c][None, :])
    return M[:, m:]


def cross_decode_ref(groups, have, nroots, skip=0):
    """DECODER of the header.  groups (G, n, len) uint8, have (G, n) (zero = missing) -> (out (G, n, len) uint8, info (G, 4) int32,
    colfail (G, len - skip) uint8)"""
    g = np.asarray(groups, np.uint8)
    G, n, ln = g.shape
    k = n - nroots
    assert 1 <= nroots <= 64 and k >= 1 and n <= 255 and 0 <= skip < ln
    hv = np.asarray(have).reshape(G, n) != 0
    gen = generator_matrix(n, k)
    out, info, colfail = g.copy(), np.zeros((G, 4), np.int32), np.zeros((G, ln - skip), np.uint8)
    for i in range(G):
        present = np.nonzero(hv[i])[0]
        f = n - len(present)
        if f > nroots:
            colfail[i] = 1
            info[i] = (ln - skip, f, 0, 0)
            continue
        cols = g[i, :, skip:].astype(np.int64)                    # (n, columns)
        first = present[:k]
        key = (n, k, first.tobytes())
        if key not in _INV:
            _INV[key] = gf_inverse(gen[:, first].T)               # the data from the k first present places
        cand = gf_matmul(gen.T, gf_matmul(_INV[key], cols[first]))     # the one codeword through them, per column
        ok = (cand[present] == cols[present]).all(axis=0)         # ... must meet EVERY present place
        new = np.where(ok[None, :], cand, cols)
        out[i, :, skip:] = new
        colfail[i] = ~ok
        info[i] = (int((~ok).sum()), f, int((new != cols).sum()), int(ok.all()))
    return out, info, colfail


def cross_place_ref(byts, count, crc_ok, n, ngroups, base=None, groups=None, have=None, length=None):
    """PLACE of the header.  byts (S, M, row), count (S,), crc_ok (S, M); groups (S, ngroups, n, len) and have (S, ngroups n) are updated
    copies of the ones given, or start as zeros with len = length (None = row)"""
    byts, count, crc_ok = np.asarray(byts, np.uint8), np.asarray(count), np.asarray(crc_ok)
    S, M, row = byts.shape
    ln = (row if length is None else length) if groups is None else np.asarray(groups).shape[3]
    assert 1 <= ln <= row and ngroups * n <= 256
    groups = np.zeros((S, ngroups, n, ln), np.uint8) if groups is None else np.array(groups, np.uint8)
    have = np.zeros((S, ngroups * n), np.uint8) if have is None else np.array(have, np.uint8)
    for s in range(S):
        b = 0 if base is None else int(base[s]) & 255
        for i in range(min(max(int(count[s]), 0), M)):
            d = (int(byts[s, i, 0]) - b) & 255
            if not crc_ok[s, i] or d >= ngroups * n:
                continue
            groups[s, d // n, d % n] = byts[s, i, :ln]
            have[s, d] = 1
    return groups, have


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_cross_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in CROSS_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "PACKET ERASURE CODE" in header and all(k in header for k in CROSS_KERNELS)
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(qpsk_amd.Modem.rs_cross_encode) == ["self", "groups", "nroots", "skip"]
    assert sig(qpsk_amd.Modem.rs_cross_decode) == ["self", "groups", "have", "nroots", "skip", "inplace"]
    assert sig(qpsk_amd.Modem.rs_cross_place) == ["self", "bytes", "count", "crc_ok", "n", "ngroups", "base", "groups", "have"]
    d = inspect.signature(qpsk_amd.Modem.rs_cross_decode).parameters
    assert d["skip"].default == 0 and d["inplace"].default is False
    buf, have, info, cnt = (C.c_uint8 * 256)(), (C.c_uint8 * 8)(), (C.c_int32 * 4)(), (C.c_int32 * 1)()
    assert qpsk_lib.qpsk_rs_cross_encode_batch(None, buf, 0, 1, 2, 2, 8, 1) == QPSK_ERR_ARG
    assert b"qpsk_rs_cross_encode_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_rs_cross_decode_batch(None, buf, 0, 1, 4, 2, 8, 1, have, buf, 0, info, None) == QPSK_ERR_ARG
    assert b"qpsk_rs_cross_decode_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_rs_cross_place_batch(None, buf, 0, cnt, have, 1, 1, 8, 4, 1, None, buf, 0, have) == QPSK_ERR_ARG
    assert b"qpsk_rs_cross_place_batch" in qpsk_lib.qpsk_last_error()


# ------------------------------------------------------------------- 2. the restatement, its relation to rs_decode_ref, the codebook
def damaged_groups(n, k, ln, skip, seed):
    """groups of one code damaged in every way the header's DECODER distinguishes -> (groups (G, n, ln), have (G, n), sent, names).  The
    missing packets are filled with bytes that are NOT the sent ones unless the name says so"""
    nroots = n - k
    rng = np.random.default_rng(seed)
    rows = []

    def add(name, f, wrong=0, missing_right=False, zero=False, where=None):
        data = np.zeros((1, n, ln), np.uint8) if zero else rng.integers(0, 256, (1, n, ln), dtype=np.uint8)
        sent = cross_encode_ref(data, nroots, skip)[0]
        order = rng.permutation(n) if where is None else np.concatenate([where, np.setdiff1d(rng.permutation(n), where, assume_unique=True)])
        miss = order[:min(f, n)]
        hv = np.ones(n, np.uint8)
        hv[miss] = 0
        grp = sent.copy()
        if not missing_right:
            grp[miss] ^= rng.integers(1, 256, (len(miss), ln), dtype=np.uint8)      # every byte of a missing packet is wrong, header too
        for c in range(wrong):                                      # one wrong byte in a present packet, in coded column skip + c
            grp[order[min(f, n):][c % max(n - f, 1)], skip + c % (ln - skip)] ^= int(rng.integers(1, 256))
        rows.append((name, grp, hv, sent))

    add("clean", 0)
    for f in range(1, nroots + 2):
        add("f = %d" % f, f)
    add("clean, a wrong present byte", 0, wrong=1)
    if nroots > 1:
        add("f = 1 < nroots, a wrong present byte", 1, wrong=1)
        add("f = nroots - 1, wrong present bytes in two columns", nroots - 1, wrong=2)
    add("f = nroots, a wrong present byte", nroots, wrong=1)
    add("f = nroots, the missing bytes happen to be right", nroots, missing_right=True)
    add("f = nroots + 1, the missing bytes happen to be right", nroots + 1, missing_right=True)
    add("all zero, clean", 0, zero=True)
    add("all zero, f = nroots", nroots, zero=True, missing_right=True)
    add("only parity missing", min(nroots, n - k), where=np.arange(k, n))
    add("only data missing", min(nroots, k), where=np.arange(k))
    return (np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), [r[0] for r in rows])


def assert_relation(groups, have, nroots, skip, got, decoder):
    """the header's relation, column by column: decoder(word, flags) -> (out word, info) is REED-SOLOMON's DECODER"""
    out, info, colfail = got
    G, n, ln = groups.shape
    for i in range(G):
        flags = (have[i] == 0).astype(np.uint8)
        fails = changed = 0
        for j in range(skip, ln):
            w, (c0, f, e, _) = decoder(groups[i, :, j], flags)
            if c0 >= 0 and e == 0:
                assert np.array_equal(out[i, :, j], w) and colfail[i, j - skip] == 0, (i, j)
                changed += c0
            else:
                assert np.array_equal(out[i, :, j], groups[i, :, j]) and colfail[i, j - skip] == 1, (i, j)
                fails += 1
        assert tuple(info[i]) == (fails, int(flags.sum()), changed, int(fails == 0)), (i, info[i])
        assert np.array_equal(out[i, :, :skip], groups[i, :, :skip])


@pytest.mark.parametrize("n,k", BOOK_CODES)
def test_cross_decode_ref_equals_the_codebook_decoder_restricted_to_e_zero(n, k):
    groups, have, sent, names = damaged_groups(n, k, ln=5, skip=1, seed=900 + 10 * n + k)
    got = cross_decode_ref(groups, have, n - k, skip=1)
    assert_relation(groups, have, n - k, 1, got, lambda w, fl: codebook_decode(w, fl, n, k))
    out, info, colfail = got
    nroots = n - k
    for name, i in ((nm, names.index(nm)) for nm in names):
        f = int((have[i] == 0).sum())
        if "wrong present" in name:
            nwrong = 2 if "two columns" in name else 1
            if f < nroots:      # detected: exactly those columns fail, the others come back
                assert info[i, 0] == nwrong and colfail[i, :nwrong].all() and not colfail[i, nwrong:].any(), (name, info[i])
                assert np.array_equal(out[i][:, 1 + nwrong:], sent[i][:, 1 + nwrong:])
            else:               # invisible: a codeword comes back, and it is not the one that was sent
                assert info[i, 0] == 0 and not np.array_equal(out[i][:, 1], sent[i][:, 1]), (name, info[i])
                assert not rs_syndromes(out[i][:, 1:].T, nroots).any()
        elif f <= nroots:
            assert info[i, 0] == 0 and info[i, 3] == 1 and np.array_equal(out[i][:, 1:], sent[i][:, 1:]), (name, info[i])
            if "happen to be right" in name or "zero" in name:
                assert info[i, 2] == 0
            elif f:
                assert info[i, 2] > 0
        else:
            assert tuple(info[i]) == (4, f, 0, 0) and np.array_equal(out[i], groups[i]), (name, info[i])


@pytest.mark.parametrize("n,k", [(6, 2), (12, 8), (20, 16), (65, 1), (40, 30)])
def test_cross_decode_ref_equals_rs_decode_ref_column_by_column_by_the_relation(n, k):
    groups, have, _, _ = damaged_groups(n, k, ln=4, skip=1, seed=7 * n + k)
    got = cross_decode_ref(groups, have, n - k, skip=1)

    def decoder(w, fl):
        o, info = rs_decode_ref(w[None, :], n - k, fl[None, :])
        return o[0], tuple(int(x) for x in info[0])

    assert_relation(groups, have, n - k, 1, got, decoder)


# ------------------------------------------------------------------- 3. the encoder
@pytest.mark.parametrize("n,k", [(3, 1), (6, 2), (12, 8), (65, 1), (255, 191), (255, 254)])
@pytest.mark.parametrize("skip", [0, 1, 6])
def test_every_column_of_an_encoded_group_is_a_codeword_and_nothing_else_changes(n, k, skip):
    rng = np.random.default_rng(n + 3 * k + skip)
    groups = rng.integers(0, 256, (3, n, 7), dtype=np.uint8)
    enc = cross_encode_ref(groups, n - k, skip)
    assert np.array_equal(enc[:, :k], groups[:, :k]) and np.array_equal(enc[:, :, :skip], groups[:, :, :skip])
    for i in range(3):
        assert not rs_syndromes(enc[i, :, skip:].T, n - k).any()
    assert np.array_equal(cross_encode_ref(enc, n - k, skip), enc)
    out, info, colfail = cross_decode_ref(enc, np.ones((3, n), np.uint8), n - k, skip)
    assert np.array_equal(out, enc) and not colfail.any() and np.array_equal(info, np.tile([0, 0, 0, 1], (3, 1)))


# ------------------------------------------------------------------- 4. place
def place_case():
    """two streams, n = 5, ngroups = 3, window 15 from base (250, 3): a wrap across 255 -> 0, numbers beyond the window, crc_ok = 0, a
    duplicated number, a count above max_packets, a negative count's twin (count 0)"""
    rng = np.random.default_rng(77)
    S, M, row, ln = 3, 10, 9, 7
    byts = rng.integers(0, 256, (S, M, row), dtype=np.uint8)
    crc_ok = np.ones((S, M), np.uint8)
    byts[0, :, 0] = [250, 255, 0, 4, 9, 250, 8, 249, 100, 251]      # d = 0 5 6 10 15(out) 0(duplicate) 14 255(out) 106(out) 1
    crc_ok[0, 3] = 0                                                 # d = 10 is dropped
    byts[1, :, 0] = [3, 17, 18, 2, 4, 4, 4, 10, 11, 12]             # d = 0 14 15(out) 255(out) 1 1 1 ...; count 7 stops before 10
    crc_ok[1, 5] = 0                                                 # the middle one of the three: the last still wins
    count = np.array([13, 7, 0], np.int32)                           # 13 > max_packets is taken as 10
    base = np.array([250, 3 + 256 * 5, 0], np.int32)                 # only the low 8 bits count
    return dict(bytes=byts, count=count, crc_ok=crc_ok, base=base, n=5, ngroups=3, len=ln)


def test_place_ref_wrap_window_crc_duplicates_count_and_untouched_slots():
    c = place_case()
    g0 = np.full((3, 3, 5, c["len"]), 0xEE, np.uint8)
    h0 = np.zeros((3, 15), np.uint8)
    h0[2, 4] = 1                                                     # the call never clears
    groups, have = cross_place_ref(c["bytes"], c["count"], c["crc_ok"], 5, 3, c["base"], g0, h0)
    want0 = {0: 5, 5: 1, 6: 2, 14: 6, 1: 9}                          # d -> index; d = 0 came twice, index 5 wins
    want1 = {0: 0, 14: 1, 1: 6}
    for s, want in ((0, want0), (1, want1), (2, {})):
        for d in range(15):
            if d in want:
                assert have[s, d] == 1 and np.array_equal(groups[s, d // 5, d % 5], c["bytes"][s, want[d], :c["len"]]), (s, d)
            else:
                assert have[s, d] == h0[s, d] and np.all(groups[s, d // 5, d % 5] == 0xEE), (s, d)
    assert have[2, 4] == 1
    fresh, fh = cross_place_ref(c["bytes"], c["count"], c["crc_ok"], 5, 3, c["base"], length=c["len"])
    assert fresh.shape == (3, 3, 5, c["len"]) and np.array_equal(fh[:2], have[:2]) and not fh[2].any()
    none, _ = cross_place_ref(c["bytes"], c["count"], c["crc_ok"], 5, 3, None, length=c["len"])
    assert np.array_equal(none[1, 0, 3], c["bytes"][1, 0, :c["len"]])      # base NULL = 0: q = 3 is d = 3


# ------------------------------------------------------------------- 5. the link on the restatements
LINK = dict(n=12, k=8, nbytes=30, skip=1, ngroups=3, base=250, nsync=32, min_score=28, lead=24, run=40, at=60, amp=0.8, seed=1208,
            lost={0: (2, 9), 1: (0, 5, 11)}, broken={0: (4, 7), 1: (3, 8)})


def link_packets():
    """three groups of (12, 8) x 30-byte packets on one stream, byte 0 the sequence number (250, 251, .. across 255 -> 0), one packet per
    on-air row at rate 1/2.  Group 0 loses 2 packets (the whole row, sync word included, is idle fill) and has 2 broken (LINK["run"]
    consecutive body dibits from body dibit LINK["at"] on inverted); group 1 loses 3 and has 2 broken; group 2 is untouched"""
    lk = LINK
    n, k, nb, G = lk["n"], lk["k"], lk["nbytes"], lk["ngroups"]
    rng = np.random.default_rng(lk["seed"])
    groups = rng.integers(0, 256, (G, n, nb), dtype=np.uint8)
    groups[:, :, 0] = ((lk["base"] + np.arange(G * n)) & 255).reshape(G, n)
    sent = cross_encode_ref(groups, n - k, lk["skip"])
    sync = rng.integers(0, 4, lk["nsync"], dtype=np.uint8)
    rows, _ = frame_ref(sent.reshape(G * n, nb), sync, True, HALF, 1, lk["lead"], 0, None)
    hit = rows.copy()
    b0 = lk["lead"] + lk["nsync"] + lk["at"]
    assert lk["at"] + lk["run"] <= body_len(nb, True, HALF)
    damaged = np.zeros(G * n, bool)
    for g, places in lk["lost"].items():
        for p in places:
            hit[g * n + p] = ks_prefix(rows.shape[1])
            damaged[g * n + p] = True
    for g, places in lk["broken"].items():
        for p in places:
            hit[g * n + p, b0:b0 + lk["run"]] ^= 3
            damaged[g * n + p] = True
    return dict(sent=sent, sync=sync, rows=rows, hit=hit, damaged=damaged)


_LINK_RESULT = {}


def link_result():
    """the CPU verdicts, computed once: the deframer's packets of the one stream, then place and decode"""
    if not _LINK_RESULT:
        lk, p = LINK, link_packets()
        z = dibits_to_costas(p["hit"].reshape(-1), amp=lk["amp"])
        got = flat(deframe_coded_ref([z], [np.float32(64.0 / lk["amp"])], p["sync"], lk["min_score"], lk["nbytes"]))
        M = len(got)
        byts = np.stack([q["bytes"] for q in got])[None]
        crc_ok = np.array([q["crc_ok"] for q in got], np.uint8)[None]
        pos = np.array([q["pos"] for q in got])
        groups, have = cross_place_ref(byts, [M], crc_ok, lk["n"], lk["ngroups"], [lk["base"]], length=lk["nbytes"])
        out, info, colfail = cross_decode_ref(groups[0], have.reshape(lk["ngroups"], lk["n"]), lk["n"] - lk["k"], lk["skip"])
        _LINK_RESULT.update(p, z=z, bytes=byts, crc_ok=crc_ok, pos=pos, groups=groups, have=have, out=out, info=info, colfail=colfail)
    return _LINK_RESULT


def test_lost_and_broken_packets_come_back_through_the_group_and_one_loss_too_many_fails_the_whole_group(qpsk_lib):
    """The chain test_cross_gpu.py runs on the device with the three library calls (so they have to be there), here on the restatements.
    Asserted first, on the restatements alone: the deframer delivers exactly the undamaged packets with crc_ok = 1 (a broken packet is
    found and fails its CRC; a lost one is not found, and the idle fill raises no false sync word).  Then: groups 0 (4 = nroots missing)
    and 2 come back complete, every data byte; group 1 (5 missing) fails in every column with its bytes untouched and
    d_info = {len - skip, 5, 0, 0}"""
    assert all(hasattr(qpsk_lib, name) for name in CROSS_SYMBOLS)
    lk, r = LINK, link_result()
    n, k, nb = lk["n"], lk["k"], lk["nbytes"]
    row_len = r["rows"].shape[1]
    lost = np.array(sorted(g * n + p for g, ps in lk["lost"].items() for p in ps))
    found = np.setdiff1d(np.arange(lk["ngroups"] * n), lost)
    assert np.array_equal(r["pos"], found * row_len + lk["lead"])                 # every row that was sent is found, where it lies, and nothing else
    assert np.array_equal(r["crc_ok"][0] != 0, ~r["damaged"][found])
    good = found[~r["damaged"][found]]
    assert np.array_equal(r["bytes"][0][r["crc_ok"][0] != 0][:, :nb], r["sent"].reshape(-1, nb)[good])
    assert np.array_equal(r["have"][0], (~r["damaged"]).astype(np.uint8))
    out, info = r["out"], r["info"]
    for g in (0, 2):
        assert np.array_equal(out[g, :, 1:], r["sent"][g, :, 1:]) and np.array_equal(out[g, :k, 1:], r["sent"][g, :k, 1:])
        assert np.array_equal(out[g, r["have"][0].reshape(-1, n)[g] != 0], r["sent"][g, r["have"][0].reshape(-1, n)[g] != 0])
    assert tuple(info[0])[:2] == (0, 4) and info[0, 3] == 1 and info[0, 2] > 0
    assert tuple(info[2]) == (0, 0, 0, 1)
    assert tuple(info[1]) == (nb - lk["skip"], 5, 0, 0)
    assert r["colfail"][1].all() and np.array_equal(out[1], r["groups"][0, 1]) and not r["colfail"][[0, 2]].any()
