"""The Reed-Solomon decoder's rare paths as inputs, built once on the CPU and decoded by both sides: test_rs_port_cpu.py runs the scalar port
(rs_port.py) over them, test_rs_gpu.py the device.

directed_rows(n, k)   rows chosen for the events a single random draw reaches by chance or not at all: a zero discrepancy in the middle of
                      Berlekamp-Massey, a length that jumps by more than one, a repeated root, a root among the shortened code's missing
                      bytes, a candidate that passes every check but the last.  They were FOUND by a seeded random search with the port's
                      trace (small codes) and by construction ((60, 44) and (255, 223): error values solved for so that chosen
                      discrepancies vanish); what is committed is the result, golden/rs_directed.json: per row the seed of its codeword, the damage as
                      (place, xor) pairs and the flagged places.  The builder decodes every row with rs_decode_ref and the port, tags it
                      (tags_of) and asserts WANTED: every event in at least 2 rows.  A Berlekamp-Massey event counts only in a row that
                      rs_decode_ref decodes, an exit only in a row it rejects just as the port does.
edge_codes()          n on both sides of the seams of the kernel's four 64-lane chunks, all four n mod 4, nroots 33 and 63, with damage placed
                      on the seams, next to the 20 patterns of test_rs_cpu.patterns.
"""
import json
import os

import numpy as np

from rs_port import rs_port
from test_rs_cpu import patterns, rs_decode_ref, rs_encode_ref


def codeword(n, k, seed):
    return rs_encode_ref(np.random.default_rng([n, k, seed]).integers(0, 256, (1, k), dtype=np.uint8), n - k)[0]


def make_row(n, k, seed, damage, erased):
    """-> (word, flags, sent): codeword `seed` of the code with word[j] ^= v for (j, v) in damage and the places `erased` flagged"""
    sent = codeword(n, k, seed)
    w, fl = sent.copy(), np.zeros(n, np.uint8)
    for j, v in damage:
        w[j] ^= v
    fl[list(erased)] = 1
    return w, fl, sent


def tags_of(trace, ref_info, ref_out, sent, flagged):
    """what a row is good for, from the port's trace of it and rs_decode_ref's verdict"""
    how = "with flags" if flagged else "without flags"
    tags = set()
    if ref_info[0] >= 0:
        if trace["exit"] == "decoded":
            tags |= {"decoded: " + ev for ev in trace["events"]}
            tags |= {"decoded, %s: %s" % (how, ev) for ev in trace["events"]}
        if not np.array_equal(ref_out, sent):
            tags.add("miscorrection")
    elif trace["exit"] not in ("decoded", "clean"):
        ex = trace["exit"]
        if ex == "roots != deg":
            ex += " with a root in the shortened region" if "a root in the shortened region" in trace["events"] else ""
        tags.add("exit: " + ex)                          # the first check, in the kernel's order, that stopped the row
        tags.add("exit, %s: %s" % (how, ex))
        tags |= {"failed: " + ev for ev in trace["events"]}
    return tags


# every entry: at least 2 rows over all codes; (tag, codes): on at least that many codes
WANTED = (
    ("decoded, without flags: interior zero discrepancy", 1), ("decoded, with flags: interior zero discrepancy", 1),
    ("decoded, without flags: zero discrepancy at r = f + 1", 1), ("decoded, with flags: zero discrepancy at r = f + 1", 1),
    ("decoded: length jump of 2", 1), ("decoded: length jump of 3 or more", 1), ("decoded: length change right after a zero", 1),
    ("decoded: a root whose value is 0", 1),
    ("exit: nz == 0", 1), ("exit: bad", 1), ("exit: roots != deg with a root in the shortened region", 1), ("exit: 2 e + f", 1),
    ("exit, with flags: second syndromes", 3), ("exit, without flags: second syndromes", 3),
    ("failed: dd == 0 at a root", 1), ("failed: deg != len", 1),
    ("miscorrection", 3),
)
BM_CODES = ((60, 44), (255, 223))                            # must hold the Berlekamp-Massey events too, not the small codes alone
BM_TAGS = ("decoded: interior zero discrepancy", "decoded: zero discrepancy at r = f + 1", "decoded: length jump of 2",
           "decoded: length jump of 3 or more")

def _load():
    """golden/rs_directed.json: "n,k" -> [[seed, [[j, v], ..], [erased j, ..]], ..], the rows the search and the construction gave"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rs_directed.json")) as fh:
        return {tuple(int(x) for x in key.split(",")): [(e[0], tuple(map(tuple, e[1])), tuple(e[2])) for e in rows] for key, rows in json.load(fh).items()}


DIRECTED = _load()

_BUILT = {}


def _build():
    if _BUILT:
        return _BUILT
    have = {}
    for (n, k), entries in DIRECTED.items():
        nroots = n - k
        rows = [make_row(n, k, *e) for e in entries]
        words, flags, sent = (np.stack([r[i] for r in rows]) for i in range(3))
        # a clean row with too many flags: the only input on which the order of the first two exits shows
        extra = sent[:2].copy(), np.zeros((2, n), np.uint8)
        extra[1][0, :nroots + 1] = 1
        extra[1][1, -(nroots + 1):] = 1
        words, flags, sent = np.concatenate([words, extra[0]]), np.concatenate([flags, extra[1]]), np.concatenate([sent, sent[:2]])
        plain = rs_decode_ref(words, nroots, None)
        erased = rs_decode_ref(words, nroots, flags)
        assert tuple(erased[1][-1]) == (-1, nroots + 1, -1, 1)
        # neighbouring waves take different exits: decoded and failing rows in turn, as far as both last
        good, bad = [list(np.nonzero(erased[1][:, 0] >= 0)[0]), list(np.nonzero(erased[1][:, 0] < 0)[0])]
        order = [x for pair in zip(good, bad) for x in pair] + good[len(bad):] + bad[len(good):]
        words, flags, sent = words[order], flags[order], sent[order]
        plain, erased = (plain[0][order], plain[1][order]), (erased[0][order], erased[1][order])
        tags = []
        for fl, want in ((flags, erased), (None, plain)):
            port = rs_port()
            got = port.decode(words, nroots, fl)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, k, "the port and rs_decode_ref disagree")
            for i, tr in enumerate(port.traces):
                flagged = fl is not None and bool(fl[i].any())
                t = tags_of(tr, want[1][i], want[0][i], sent[i], flagged)
                tags.append(t)
                if fl is None and not flags[i].any():
                    continue                             # the same decode as in the first pass: counted once
                for tag in t:
                    have.setdefault(tag, []).append((n, k))
        for a in (words, flags, sent) + plain + erased:
            a.setflags(write=False)
        names = ["directed %d" % i for i in order]
        _BUILT[(n, k)] = dict(words=words, flags=flags, sent=sent, names=names, erased=erased, plain=plain, tags=tags)
    for tag, codes in WANTED:
        at = have.get(tag, [])
        assert len(at) >= 2 and len(set(at)) >= codes, (tag, at)
    for code in BM_CODES:
        for tag in BM_TAGS:
            assert have.get(tag, []).count(code) >= 1, (tag, code)
    _BUILT["have"] = {tag: len(at) for tag, at in have.items()}
    return _BUILT


def directed_codes():
    return tuple(DIRECTED)


def directed_have():
    """tag -> the number of directed rows that carry it, each row counted once"""
    return _build()["have"]


def directed_rows(n, k):
    """-> dict(words, flags, sent, names, erased=(out, info), plain=(out, info), tags): the rows of one code, both references; read-only"""
    return _build()[(n, k)]


# ------------------------------------------------------------------------------------------ the seams of the lane chunks
SEAMS = (0, 62, 63, 64, 65, 127, 128, 191, 192)
EDGE_CODES = tuple((n, n - 8) for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255)) + ((130, 97), (130, 67))
_EDGE = {}


def edge_codes():
    """n on both sides of every multiple of 64 and at the top, nroots = 8; nroots = 33 and 63 (an odd `top` at a large degree) at n = 130"""
    assert {n % 4 for n, _ in EDGE_CODES} == {0, 1, 2, 3}
    return EDGE_CODES


def seam_rows(n, k):
    """-> (words, flags, sent, names): errors and erasures on the places SEAMS and n - 1, alone, in pairs across a seam and all at once; an
    erasure-only row with f = nroots over every chunk; rows beyond the radius in between, so that neighbouring waves leave differently"""
    nroots, t = n - k, (n - k) // 2
    rng = np.random.default_rng([n, k, 64])
    seams = sorted({j for j in SEAMS + (n - 1,) if j < n})
    rows = []

    def add(name, errors=(), erased=(), right=()):
        """errors: unflagged wrong bytes; erased: flagged places, wrong except those in `right`"""
        sent = rs_encode_ref(rng.integers(0, 256, (1, k), dtype=np.uint8), nroots)[0]
        w, fl = sent.copy(), np.zeros(n, np.uint8)
        hit = np.array(sorted(set(errors) | (set(erased) - set(right))), np.int64)
        w[hit] ^= rng.integers(1, 256, len(hit), dtype=np.uint8)
        fl[list(erased)] = 1
        rows.append((name, w, fl, sent))

    others = [j for j in range(n) if j not in seams]
    for j in seams:
        add("error at %d" % j, errors=[j])
        add("erasure at %d" % j, erased=[j])
    add("t + 1 errors from the seams on", errors=(seams + others)[:t + 1])
    for a, b in ((62, 63), (63, 64), (64, 65), (127, 128), (191, 192), (0, n - 1)):
        if b < n:
            add("errors at %d and %d" % (a, b), errors=[a, b])
            add("error at %d, erasure at %d" % (a, b), errors=[a], erased=[b])
            add("erasure at %d, error at %d" % (a, b), erased=[a], errors=[b])
            add("erasures at %d and %d, the second right" % (a, b), erased=[a, b], right=[b])
    add("t errors from the seams on", errors=(seams + others)[:t])
    add("f = nroots from the seams on", erased=(seams + others)[:nroots])
    add("f = nroots + 1 from the seams on", erased=(seams + others)[:nroots + 1])
    add("e and f at the radius from the seams on", errors=(seams + others)[:t // 2], erased=(seams + others)[t // 2:t // 2 + nroots - 2 * (t // 2)])
    add("one error more than that", errors=(seams + others)[:t // 2] + others[-1:], erased=(seams + others)[t // 2:t // 2 + nroots - 2 * (t // 2)])
    spread = sorted({int(x) for x in np.round(np.linspace(0, n - 1, nroots))})
    assert len(spread) == nroots and {j // 64 for j in spread} == set(range((n + 63) // 64))
    add("f = nroots over every chunk, nothing else", erased=spread)
    add("the same, half of them right", erased=spread, right=spread[::2])
    return (np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), [r[0] for r in rows])


def edge_rows(n, k):
    """the seam rows and the 20 patterns of an edge code with both references, computed once; read-only"""
    if (n, k) not in _EDGE:
        a, b = seam_rows(n, k), patterns(n, k)
        words, flags, sent = (np.concatenate([a[i], b[i]]) for i in range(3))
        erased, plain = rs_decode_ref(words, n - k, flags), rs_decode_ref(words, n - k, None)
        for x in (words, flags, sent) + erased + plain:
            x.setflags(write=False)
        names = a[3] + b[3]
        # the rows do what they are there for, on the reference alone
        for name in ("t errors from the seams on", "f = nroots from the seams on", "e and f at the radius from the seams on",
                     "f = nroots over every chunk, nothing else", "the same, half of them right") + tuple(x for x in names if x.startswith(("error at", "erasure")) or " and " in x):
            i = names.index(name)
            assert erased[1][i, 0] >= 0 and np.array_equal(erased[0][i], sent[i]), (n, k, name, erased[1][i])
        for name in ("t + 1 errors from the seams on", "one error more than that"):
            i = names.index(name)
            assert erased[1][i, 0] == -1 or not np.array_equal(erased[0][i], sent[i]), (n, k, name)
        assert erased[1][names.index("f = nroots + 1 from the seams on"), 0] == -1
        _EDGE[(n, k)] = dict(words=words, flags=flags, sent=sent, names=names, erased=erased, plain=plain)
    return _EDGE[(n, k)]
