"""The Reed-Solomon outer code of the coded packet path (REED-SOLOMON in include/qpsk_hip.h: qpsk_rs_generator, qpsk_rs_encode_batch,
qpsk_rs_decode_batch): what can be checked without a GPU.

The restatements below are the header's definition in numpy, in integers.  rs_decode_ref is NOT the kernel's algorithm: the kernel runs
Berlekamp-Massey from the erasure locator and Forney's formula; here the locator comes from Euclid's algorithm on the erasure-modified
syndromes, the error values from a linear system solved by elimination, and the verdict is the definition's, applied literally to the
candidate (a codeword, 2 e + f <= nroots).  What pins the verdict independently of any decoding algorithm is the codebook decoder of
section 2: all 256^k codewords of four small codes, enumerated.  The GPU tests (test_rs_gpu.py) compare the kernels with rs_encode_ref /
rs_decode_ref bit for bit.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_deframe_coded_cpu import dibits_to_costas
from test_frame_cpu import body_len, frame_ref, starts
from test_punct_cpu import NAMED, deframe_coded_punct_ref
from test_rx_ext_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_SYMBOLS = ("qpsk_rs_generator", "qpsk_rs_encode_batch", "qpsk_rs_decode_batch")
QPSK_ERR_ARG = -2
RS_MAX_ROOTS = 64


# ------------------------------------------------------------------- the field: GF(256) modulo 0x11D, alpha = 2
def _tables():
    exp, log = np.zeros(512, np.int64), np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    exp[255:510] = exp[:255]
    return exp, log


EXP, LOG = _tables()


def gf_mul(a, b):
    """elementwise product of two integer arrays (or scalars) of field elements"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, EXP[LOG[a] + LOG[b]])


def gf_inv(a):
    assert np.all(np.asarray(a) != 0)
    return EXP[(255 - LOG[np.asarray(a, np.int64)]) % 255]


def gf_pow_alpha(e):
    """alpha^e for any integer array e"""
    return EXP[np.asarray(e, np.int64) % 255]


def poly_mul(a, b):
    """polynomials as int64 arrays, LOWEST coefficient first"""
    out = np.zeros(len(a) + len(b) - 1, np.int64)
    for i, c in enumerate(a):
        out[i:i + len(b)] ^= gf_mul(c, b)
    return out


def poly_eval(p, x):
    """p (lowest first) at every element of the array x, by Horner"""
    x = np.asarray(x, np.int64)
    v = np.zeros_like(x)
    for c in p[::-1]:
        v = gf_mul(v, x) ^ int(c)
    return v


def poly_deg(p):
    nz = np.nonzero(p)[0]
    return int(nz[-1]) if len(nz) else -1


# ------------------------------------------------------------------- the numpy restatement
def rs_generator_ref(nroots):
    """g(x) = prod_{i < nroots} (x - alpha^i), the nroots + 1 coefficients HIGHEST first (g[0] = 1)"""
    g = np.array([1], np.int64)
    for i in range(nroots):
        g = poly_mul(g, np.array([EXP[i], 1], np.int64))
    return g[::-1].astype(np.uint8)


def rs_encode_ref(data, nroots):
    """data (R, k) uint8 -> (R, k + nroots): the data, then (d(x) x^nroots) mod g(x), by the division's shift register on every row at once"""
    d = np.atleast_2d(np.asarray(data, np.uint8)).astype(np.int64)
    R, k = d.shape
    assert k >= 1 and 1 <= nroots <= RS_MAX_ROOTS and k + nroots <= 255
    g = rs_generator_ref(nroots).astype(np.int64)[1:]
    par = np.zeros((R, nroots), np.int64)
    for j in range(k):
        fb = d[:, j] ^ par[:, 0]
        par = np.concatenate([par[:, 1:], np.zeros((R, 1), np.int64)], axis=1) ^ gf_mul(fb[:, None], g[None, :])
    return np.concatenate([d, par], axis=1).astype(np.uint8)


def rs_syndromes(rows, nroots):
    """rows (R, n) -> (R, nroots): S_i = c(alpha^i) with c(x) = sum_j row[j] x^(n - 1 - j)"""
    r = np.atleast_2d(np.asarray(rows, np.uint8)).astype(np.int64)
    a = EXP[np.arange(nroots)][None, :]
    S = np.zeros((r.shape[0], nroots), np.int64)
    for j in range(r.shape[1]):
        S = gf_mul(S, a) ^ r[:, j:j + 1]
    return S


def _solve(A, b):
    """A x = b over the field by elimination; A (m, m) non-singular, or None"""
    m = len(b)
    M = np.concatenate([np.asarray(A, np.int64), np.asarray(b, np.int64)[:, None]], axis=1)
    for c in range(m):
        p = next((r for r in range(c, m) if M[r, c]), None)
        if p is None:
            return None
        M[[c, p]] = M[[p, c]]
        M[c] = gf_mul(M[c], gf_inv(M[c, c]))
        for r in range(m):
            if r != c and M[r, c]:
                M[r] ^= gf_mul(M[r, c], M[c])
    return M[:, m]


def _candidate(r, flags, nroots, S):
    """the one word the algebra proposes for a row with non-zero syndromes and f <= nroots, or None.  Euclid on (x^nroots, S Gamma mod
    x^nroots) down to a remainder of degree < (nroots + f) / 2 gives the error locator sigma; the positions are the stored positions where
    Gamma sigma vanishes; the values solve sum_p v_p X_p^i = S_i"""
    n = len(r)
    X = gf_pow_alpha(n - 1 - np.arange(n))                       # position j's locator alpha^(n - 1 - j)
    gamma = np.array([1], np.int64)
    for j in np.nonzero(flags)[0]:
        gamma = poly_mul(gamma, np.array([1, X[j]], np.int64))
    f = len(gamma) - 1
    T = poly_mul(S, gamma)[:nroots]
    r0, r1 = np.zeros(nroots + 1, np.int64), T.copy()
    r0[nroots] = 1
    t0, t1 = np.array([0], np.int64), np.array([1], np.int64)
    while 2 * poly_deg(r1) >= nroots + f:
        d1 = poly_deg(r1)
        q = np.zeros(max(poly_deg(r0) - d1 + 1, 1), np.int64)
        rem = r0.copy()
        while poly_deg(rem) >= d1:
            s = poly_deg(rem) - d1
            c = int(gf_mul(rem[poly_deg(rem)], gf_inv(r1[d1])))
            q[s] = c
            rem[s:s + d1 + 1] ^= gf_mul(c, r1[:d1 + 1])
        qt = poly_mul(q, t1)
        t2 = np.zeros(max(len(qt), len(t0)), np.int64)
        t2[:len(qt)] ^= qt
        t2[:len(t0)] ^= t0
        r0, r1, t0, t1 = r1, rem, t1, t2
    if poly_deg(t1) < 0 or t1[0] == 0:
        return None
    lam = poly_mul(gamma, t1[:poly_deg(t1) + 1])
    at = np.nonzero(poly_eval(lam, gf_inv(X)) == 0)[0]
    if len(at) != poly_deg(lam) or len(at) > nroots or len(at) == 0:
        return None
    A = gf_pow_alpha(np.outer(np.arange(len(at)), LOG[X[at]]))   # A[i][p] = X_p^i
    v = _solve(A, S[:len(at)])
    if v is None:
        return None
    c = r.astype(np.int64)
    c[at] ^= v
    return c.astype(np.uint8)


def rs_decode_ref(words, nroots, erasures=None):
    """DECODER of the header.  words (R, n) uint8, erasures (R, n) (non-zero = erased) or None -> (out (R, n) uint8, info (R, 4) int32)"""
    w = np.atleast_2d(np.asarray(words, np.uint8))
    R, n = w.shape
    assert 1 <= nroots <= RS_MAX_ROOTS and nroots < n <= 255
    er = np.zeros((R, n), bool) if erasures is None else np.atleast_2d(np.asarray(erasures)) != 0
    S = rs_syndromes(w, nroots)
    out, info = w.copy(), np.zeros((R, 4), np.int32)
    for i in range(R):
        f, clean = int(er[i].sum()), not S[i].any()
        info[i] = (-1, f, -1, int(clean))
        if f > nroots:
            continue
        c = w[i] if clean else _candidate(w[i], er[i], nroots, S[i])
        if c is None or rs_syndromes(c, nroots).any():
            continue
        e = int(((c != w[i]) & ~er[i]).sum())
        if 2 * e + f > nroots:
            continue
        out[i] = c
        info[i, 0], info[i, 2] = int((c != w[i]).sum()), e
    return out, info


# ------------------------------------------------------------------- 1. ABI (fails without the feature)
def test_rs_entry_points_are_declared_bound_exported_and_refuse_without_a_context(qpsk_lib):
    import qpsk_amd
    from qpsk_amd.lib import API_SYMBOLS
    for name in RS_SYMBOLS:
        assert name in declared("qpsk_hip.h"), name
        assert name in API_SYMBOLS, name
        assert hasattr(qpsk_lib, name), name
    header = open(os.path.join(ROOT, "include", "qpsk_hip.h")).read()
    assert "REED-SOLOMON" in header
    assert callable(getattr(qpsk_amd, "rs_generator", None))
    assert list(inspect.signature(qpsk_amd.Modem.rs_encode).parameters) == ["self", "data", "nroots", "pitch"]
    assert list(inspect.signature(qpsk_amd.Modem.rs_decode).parameters) == ["self", "words", "nroots", "erasures", "pitch", "n", "inplace"]
    buf, info = (C.c_uint8 * 64)(), (C.c_int32 * 4)()
    assert qpsk_lib.qpsk_rs_encode_batch(None, buf, 0, 1, 4, 2, buf, 0) == QPSK_ERR_ARG
    assert b"qpsk_rs_encode_batch" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_rs_decode_batch(None, buf, 0, 1, 6, 2, None, buf, 0, info) == QPSK_ERR_ARG
    assert b"qpsk_rs_decode_batch" in qpsk_lib.qpsk_last_error()


# ------------------------------------------------------------------- 2. the codebook pins the restatement, failure verdict included
BOOK_CODES = ((3, 1), (6, 2), (5, 2), (8, 2))
_BOOKS = {}


def codebook(n, k):
    """all 256^k codewords, (256^k, n)"""
    if (n, k) not in _BOOKS:
        data = np.stack(np.meshgrid(*[np.arange(256, dtype=np.uint8)] * k, indexing="ij"), axis=-1).reshape(-1, k)
        _BOOKS[(n, k)] = rs_encode_ref(data, n - k)
    return _BOOKS[(n, k)]


def codebook_decode(word, flags, n, k):
    """the definition, literally: over every codeword c, e = the unflagged places where it differs from the word; the output is the c with
    2 e + f <= nroots if f <= nroots and one exists (there is never a second), else the word and -1"""
    nroots, book = n - k, codebook(n, k)
    flags = np.asarray(flags) != 0
    f, clean = int(flags.sum()), int(not rs_syndromes(word, nroots).any())
    if f <= nroots:
        e = ((book != word[None, :]) & ~flags[None, :]).sum(axis=1)
        hit = np.nonzero(2 * e + f <= nroots)[0]
        assert len(hit) <= 1                                      # the minimum distance is nroots + 1
        if len(hit):
            c = book[hit[0]]
            return c, (int((c != word).sum()), f, int(e[hit[0]]), clean)
    return word, (-1, f, -1, clean)


def book_cases(rng, n, k, with_erasures):
    """(word, flags) pairs: random words; codewords with e errors and f erasures at exactly the radius (2 e + f = nroots, and = nroots - 1
    where the parity allows no equality), one step beyond it (nroots + 1), far beyond it, f > nroots; erased bytes both changed and left
    right"""
    nroots, book = n - k, codebook(n, k)
    cases = []
    for _ in range(12):
        flags = np.zeros(n, bool)
        if with_erasures:
            flags[rng.choice(n, rng.integers(0, nroots + 2), replace=False)] = True
        cases.append((rng.integers(0, 256, n, dtype=np.uint8), flags))
    fs = range(0, nroots + 2) if with_erasures else (0,)
    for f in fs:
        at_radius = max((nroots - f) // 2, 0)
        for e in sorted({0, at_radius, min(at_radius + 1, n - f), n - f}):
            for keep_right in (False, True):
                c = book[rng.integers(0, len(book))].copy()
                at = rng.permutation(n)
                flags = np.zeros(n, bool)
                flags[at[:f]] = True
                w = c.copy()
                w[at[f:f + e]] ^= rng.integers(1, 256, e, dtype=np.uint8)
                hit = at[:f] if not keep_right else at[:f // 2]
                w[hit] ^= rng.integers(1, 256, len(hit), dtype=np.uint8)
                cases.append((w, flags))
    return cases


@pytest.mark.parametrize("with_erasures", [False, True])
@pytest.mark.parametrize("n,k", BOOK_CODES)
def test_rs_decode_ref_equals_the_codebook_decoder(n, k, with_erasures):
    rng = np.random.default_rng(100 * n + k + with_erasures)
    cases = book_cases(rng, n, k, with_erasures)
    words, flags = np.stack([w for w, _ in cases]), np.stack([f for _, f in cases])
    out, info = rs_decode_ref(words, n - k, flags if with_erasures else None)
    verdicts = set()
    for i, (w, fl) in enumerate(cases):
        c, want = codebook_decode(w, fl, n, k)
        assert np.array_equal(out[i], c) and tuple(info[i]) == want, (n, k, i, w, fl, out[i], info[i], c, want)
        verdicts.add((want[0] < 0, want[0] >= 0 and 2 * want[2] + want[1] >= n - k - 1))
    assert (True, False) in verdicts and (False, True) in verdicts      # failures, and decodes where one more error would pass the radius, both occurred


def test_a_word_beyond_the_radius_within_another_codeword_s_radius_decodes_to_that_codeword():
    """the consequence the header states, on (8, 2): a codeword with 4 errors of which 3 are the bytes of ANOTHER codeword is that other
    codeword with at most 3 errors"""
    book = codebook(8, 2)
    a, b = book[1], book[77]
    diff = np.nonzero(a != b)[0]
    assert len(diff) >= 7                                         # minimum distance nroots + 1 = 7
    w = a.copy()
    w[diff[:4]] = b[diff[:4]]                                     # 4 errors from a; b lies len(diff) - 4 <= 4 away ...
    w[diff[4]] = b[diff[4]]                                       # ... 5 from a, <= 3 from b
    out, info = rs_decode_ref(w, 6)
    assert np.array_equal(out[0], b) and info[0, 2] == len(diff) - 5 and info[0, 2] <= 3


# ------------------------------------------------------------------- 3. algebra
def test_qpsk_rs_generator_equals_the_numpy_product_and_refuses_out_of_range(qpsk_lib):
    import qpsk_amd
    for nroots in range(1, RS_MAX_ROOTS + 1):
        buf = (C.c_uint8 * (nroots + 2))(*([0xEE] * (nroots + 2)))
        assert qpsk_lib.qpsk_rs_generator(nroots, buf) == 0, nroots
        want = rs_generator_ref(nroots)
        assert want[0] == 1 and list(buf)[:nroots + 1] == want.tolist() and buf[nroots + 1] == 0xEE, nroots
        assert not poly_eval(want[::-1].astype(np.int64), EXP[np.arange(nroots)]).any()       # the roots are alpha^0 .. alpha^(nroots - 1)
        assert np.array_equal(qpsk_amd.rs_generator(nroots), want)
    assert rs_generator_ref(1).tolist() == [1, 1] and rs_generator_ref(2).tolist() == [1, 3, 2]       # (x - 1)(x - 2) = x^2 + 3 x + 2
    buf = (C.c_uint8 * 80)()
    for bad in (0, -1, 65, 255):
        assert qpsk_lib.qpsk_rs_generator(bad, buf) == QPSK_ERR_ARG, bad
        assert b"qpsk_rs_generator" in qpsk_lib.qpsk_last_error()
    assert qpsk_lib.qpsk_rs_generator(4, None) == QPSK_ERR_ARG
    with pytest.raises(qpsk_amd.QpskError):
        qpsk_amd.rs_generator(65)


RS_CODES = ((3, 1), (6, 2), (7, 5), (15, 11), (34, 32), (60, 44), (204, 188), (255, 223), (255, 254), (65, 1), (255, 191), (21, 16))


def patterns(n, k):
    """-> (words (R, n), flags (R, n), sent (R, n), names): codewords damaged in every way the issue lists, in an order that puts rows
    with different exits next to each other"""
    nroots, t = n - k, (n - k) // 2
    rng = np.random.default_rng(1000 * n + k)
    rows = []

    def add(name, errors=0, erased=0, erased_right=0, at=None, word=None):
        """a fresh codeword with `erased` flagged positions, of which `erased_right` keep their byte, and `errors` unflagged wrong bytes
        (at the places `at` when given)"""
        sent = rs_encode_ref(rng.integers(0, 256, (1, k), dtype=np.uint8), nroots)[0]
        w, fl = sent.copy(), np.zeros(n, np.uint8)
        if word is not None:
            sent = w = np.asarray(word, np.uint8)
        erased, errors = min(erased, n), min(errors, n - min(erased, n))
        order = rng.permutation(n) if at is None else np.concatenate([at, np.setdiff1d(rng.permutation(n), at, assume_unique=True)])
        err_at, era_at = order[:errors], order[errors:errors + erased]
        fl[era_at] = 1
        hit = np.concatenate([err_at, era_at[erased_right:]]).astype(np.int64)
        w = w.copy()
        w[hit] ^= rng.integers(1, 256, len(hit), dtype=np.uint8)
        rows.append((name, w, fl, sent))

    add("clean")
    add("1 error", errors=1)
    add("t errors", errors=t)
    add("t + 1 errors", errors=t + 1)
    add("clean, again")
    add("error at j = 0", errors=1, at=np.array([0]))
    add("f = nroots + 1", erased=nroots + 1)
    add("error at j = n - 1", errors=1, at=np.array([n - 1]))
    add("all zero", word=np.zeros(n, np.uint8))
    add("error in the parity", errors=1, at=np.array([k + (nroots - 1) // 2]))
    add("garbage", word=rng.integers(0, 256, n, dtype=np.uint8))
    add("errors at both ends and in the parity", errors=min(3, max(t, 1)), at=np.array([0, n - 1, n - 2][:min(3, max(t, 1))]))
    add("all 0xFF", word=np.full(n, 0xFF, np.uint8))
    add("f = nroots, e = 0", erased=nroots)
    e = max(1, t // 2)
    add("2 e + f = nroots", errors=e, erased=max(nroots - 2 * e, 0))
    add("2 e + f = nroots + 1", errors=e, erased=max(nroots + 1 - 2 * e, 0))
    add("erased bytes that are right", erased=nroots, erased_right=(nroots + 1) // 2)
    add("clean with erasures", erased=max(t, 1), erased_right=max(t, 1))
    add("garbage with erasures", erased=t, word=rng.integers(0, 256, n, dtype=np.uint8))
    add("t errors, again", errors=t)
    return (np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), [r[0] for r in rows])


_CASES = {}


def case(n, k):
    """the rows of a code with both references, computed once and shared by every test; nobody changes them"""
    if (n, k) not in _CASES:
        words, flags, sent, names = patterns(n, k)
        out_e, info_e = rs_decode_ref(words, n - k, flags)
        out_0, info_0 = rs_decode_ref(words, n - k, None)
        for a in (words, flags, sent, out_e, info_e, out_0, info_0):
            a.setflags(write=False)
        _CASES[(n, k)] = dict(words=words, flags=flags, sent=sent, names=names, erased=(out_e, info_e), plain=(out_0, info_0))
    return _CASES[(n, k)]


def encoder_rows(n, k, counts=(1, 5, 70)):
    """the data blocks the encoder's GPU test sends, per row count"""
    rng = np.random.default_rng(n * 300 + k)
    sets = []
    for R in counts:
        data = rng.integers(0, 256, (R, k), dtype=np.uint8)
        data[0] = 0xFF
        data[R // 2] = 0
        sets.append((R, data))
    return sets


@pytest.mark.parametrize("n,k", RS_CODES)
def test_every_encoded_row_is_systematic_and_has_zero_syndromes(n, k):
    rng = np.random.default_rng(n * 256 + k)
    data = rng.integers(0, 256, (6, k), dtype=np.uint8)
    data[0], data[1] = 0, 0xFF
    rows = rs_encode_ref(data, n - k)
    assert rows.shape == (6, n) and np.array_equal(rows[:, :k], data) and not rows[0].any()
    assert not rs_syndromes(rows, n - k).any()
    # the parity is the remainder: c(x) is a multiple of g(x), checked by dividing it out the long way on one row
    g = rs_generator_ref(n - k).astype(np.int64)
    rem = rows[2].astype(np.int64)
    for j in range(k):
        rem[j:j + n - k + 1] ^= gf_mul(rem[j], g)
    assert not rem.any()


@pytest.mark.parametrize("n,k", RS_CODES)
def test_errors_and_erasures_up_to_the_radius_come_back_and_one_more_does_not_come_back_as_sent(n, k):
    nroots = n - k
    rng = np.random.default_rng(n + k)
    sent = rs_encode_ref(rng.integers(0, 256, (1, k), dtype=np.uint8), nroots)[0]
    for f in sorted({0, 1, nroots // 2, nroots - 1, nroots}):
        e = (nroots - f) // 2
        for extra in (0, 1):
            at = rng.permutation(n)
            if f + e + extra > n:
                continue
            w, flags = sent.copy(), np.zeros(n, np.uint8)
            flags[at[:f]] = 1
            w[at[:f + e + extra]] ^= rng.integers(1, 256, f + e + extra, dtype=np.uint8)
            out, info = rs_decode_ref(w, nroots, flags)
            if extra == 0:
                assert np.array_equal(out[0], sent) and tuple(info[0]) == (f + e, f, e, int(f + e == 0)), (f, e, info[0])
            else:
                assert not np.array_equal(out[0], sent) and (info[0, 0] == -1 or info[0, 2] <= e), (f, e, info[0])
                assert info[0, 0] != -1 or np.array_equal(out[0], w)


# ------------------------------------------------------------------- 4. the link: what the outer code is for
LINK = dict(packets=64, n=60, k=44, rate="7/8", nsync=32, min_score=28, lead=40, gap=0, run=36, at=100, amp=0.8, seed=6044)


def link_packets():
    """64 packets whose payload is a (60, 44) codeword, framed at rate 7/8 without interleaver, one row each; in every row the LINK["run"]
    consecutive body dibits from body dibit LINK["at"] on are inverted (both bits: the symbol's negative) -> dict(data (64, 44), words
    (64, 60), sync, rows (64, row_len) dibits on air, hit the same with the run inverted)"""
    lk = LINK
    rng = np.random.default_rng(lk["seed"])
    data = rng.integers(0, 256, (lk["packets"], lk["k"]), dtype=np.uint8)
    words = rs_encode_ref(data, lk["n"] - lk["k"])
    sync = rng.integers(0, 4, lk["nsync"], dtype=np.uint8)
    rows, _ = frame_ref(words, sync, True, NAMED[lk["rate"]], 1, lk["lead"], lk["gap"], None)
    hit = rows.copy()
    b0 = starts(lk["nsync"], lk["n"], True, NAMED[lk["rate"]], 1, lk["lead"], lk["gap"])[0] + lk["nsync"] + lk["at"]
    assert lk["at"] + lk["run"] <= body_len(lk["n"], True, NAMED[lk["rate"]])
    hit[:, b0:b0 + lk["run"]] ^= 3
    return dict(data=data, words=words, sync=sync, rows=rows, hit=hit)


_LINK_RESULT = {}


def link_result():
    """the CPU verdicts, computed once: per packet the deframer's bytes (62) and crc_ok from the numpy restatements"""
    if not _LINK_RESULT:
        lk, p = LINK, link_packets()
        byts, ok = [], []
        for row in p["hit"]:
            z = dibits_to_costas(row, amp=lk["amp"])
            got = deframe_coded_punct_ref([z], [np.float32(64.0 / lk["amp"])], p["sync"], lk["min_score"], lk["n"], NAMED[lk["rate"]])[0]
            assert len(got) == 1 and got[0]["pos"] == lk["lead"]
            byts.append(got[0]["bytes"])
            ok.append(got[0]["crc_ok"])
        _LINK_RESULT.update(p, bytes=np.stack(byts), crc_ok=np.array(ok, bool))
    return _LINK_RESULT


def test_a_burst_that_fails_every_crc_is_repaired_by_the_outer_code():
    """LINK["run"] = 36 was found on the CPU: this test's own computation (link_result, then rs_decode_ref) with the run varied over 8, 12, ..
    48, 56, 64 inverted dibits from body dibit 100 on, this seed.  Every one of those runs fails the CRC in 64 of 64 packets -- at rate 7/8
    the inner code has no strength to spare for a run of inverted symbols.  Runs up to 36 leave 8 or fewer wrong bytes in every packet
    (8, 12, .. 32 dibits: 2..5, 3, 4, 5, 6, 7, 8 wrong bytes; 36: 8 in every packet, exactly the radius) and all 64 data blocks come back;
    40 dibits leave 9 wrong bytes per packet and nothing comes back.  36 is the longest run with 64 of 64 on both sides.  Asserted:
    (1) without the outer code the CRC fails in all 64 packets; (2) every packet has at most 8 = nroots / 2 wrong bytes and rs_decode_ref
    returns all 64 data blocks"""
    lk, r = LINK, link_result()
    wrong = (r["bytes"][:, :lk["n"]] != r["words"]).sum(axis=1)
    out, info = rs_decode_ref(r["bytes"][:, :lk["n"]], lk["n"] - lk["k"])
    back = int((out[:, :lk["k"]] == r["data"]).all(axis=1).sum())
    print("run %d at %d: crc fails in %d of %d, wrong bytes per packet %d..%d, data blocks back %d" %
          (lk["run"], lk["at"], int((~r["crc_ok"]).sum()), lk["packets"], wrong.min(), wrong.max(), back))
    assert not r["crc_ok"].any()
    assert wrong.max() <= 8 and wrong.min() >= 1
    assert back == lk["packets"] and np.array_equal(info[:, 0], wrong) and np.array_equal(info[:, 2], wrong) and not info[:, 3].any()
    clean = deframe_coded_punct_ref([dibits_to_costas(r["rows"][0], amp=lk["amp"])], [np.float32(64.0 / lk["amp"])], r["sync"], lk["min_score"],
                                    lk["n"], NAMED[lk["rate"]])[0]
    assert clean[0]["crc_ok"] and np.array_equal(clean[0]["bytes"][:lk["n"]], r["words"][0])      # the run, nothing else, breaks the packet
