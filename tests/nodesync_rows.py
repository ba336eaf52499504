"""The node sync's input space as sets of calls, built once on the CPU and run by both sides: test_nodesync_port_cpu.py runs the scalar port
(nodesync_port.py) over them, test_nodesync_sweep_gpu.py the device.  A set is a dict(name, streams, steps):

  steps     ("reset", nlinks, kw) | ("set", cand or None) | ("push", soft (S, ntx, 2) int8, vinfo (S, 4) or None, in_pitch, out_pitch, want_info)
  streams   the input's first row this many bytes behind a 16-byte boundary, one run of all steps per entry.  The output's first row is always
            2 bytes behind one, as in test_nodesync_gpu.soft_rows; both buffers are poison (0x55) outside their rows, GUARD bytes behind.

sweep(nshift)   candidate x head x input alignment in full: one link per (candidate, output alignment), two streams.
every_pair()    all 65536 int8 pairs through turn_packed on the device's own path, twice with other neighbours, at h = 0 and h = 1.
walk()          a candidate switch by the tick at every push, through every delay and the wrap, with a qpsk_nodesync_set in the middle.
limit()         NODESYNC_MAX_NTX dibits in one push on the deepest candidate, then a push that reads nothing but history.
products()      threshold products of which one side passes 2^31 and the other does not.
old_transform(), old_tick()   the inputs of test_nodesync_gpu.py's transform and tick tests, rebuilt by its code at its seeds and pitches:
                what the suite ran before these sets.

Each builder runs the port and asserts from its trace that the set holds what it was built for, so a set that does not fails here, on the
CPU, when it is built.  run_ref and run_port keep their results with the set: the reference of a set is computed once."""
import numpy as np

from nodesync_port import Image, nodesync_port
from test_nodesync_cpu import minus128, nodesync_ref, turn_ref
from test_viterbi_stream_cpu import random_soft

GUARD = 64
IN_ADDR, OUT_ADDR = 0x7F2A40000000, 0x7F2A80000000          # 16-byte aligned, as a device allocation is
STRIDE = 96
_SETS = {}


def image(rows, pitch, S, ntx, off):
    """the host image of test_nodesync_gpu.soft_rows with the first row `off` bytes in: poison everywhere but in `rows`"""
    h = np.full(off + 2 * S * pitch + GUARD, 0x55, np.uint8)
    if rows is not None:
        h[off:off + 2 * S * pitch].reshape(S, pitch, 2)[:, :ntx] = rows.view(np.uint8)
    return h


def state_image(ref, raw):
    """the state a device leaves behind where nodesync_ref stands: per link 8 int32 { c, locked, run, err, cnt, settle_left, switches, 0 },
    at byte 32 the last nshift - 1 input dibits, raw, and zeros up to the stride"""
    S, H = ref.S, ref.nshift - 1
    w = np.zeros((S, STRIDE // 4), np.int32)
    for l, s in enumerate(ref.st):
        w[l, :7] = (s["c"], s["locked"], s["run"], s["err"], s["cnt"], s["settle_left"], s["switches"])
    b = w.view(np.uint8).reshape(S, STRIDE).copy()
    b[:, 32:32 + 2 * H] = raw.view(np.uint8).reshape(S, 2 * H)
    return b.reshape(-1)


def run_ref(s):
    """nodesync_ref over the steps, once per set -> per push dict(soft, info or None, state)"""
    if "_ref" not in s:
        calls, ref, raw = [], None, None
        for step in s["steps"]:
            if step[0] == "reset":
                ref = nodesync_ref(step[1], **step[2])
                raw = np.zeros((step[1], ref.nshift - 1, 2), np.int8)
            elif step[0] == "set":
                ref.set(step[1])
            else:
                _, soft, vinfo, ip, op, want_info = step
                o = ref.push(soft, vinfo)
                raw = np.concatenate([raw, soft], axis=1)[:, soft.shape[1] + raw.shape[1] - (ref.nshift - 1):]
                calls.append(dict(soft=o["soft"], info=o["info"] if want_info else None, state=state_image(ref, raw)))
        s["_ref"] = calls
    return s["_ref"]


def run_port(s, stream=0, fault=None, seed=None):
    """the port over the steps -> (per push dict(soft, info or None, state), the port); the unfaulted run from zeros is kept with the set"""
    key = ("_port", stream)
    if fault is None and seed is None and key in s:
        return s[key]
    port, calls, off = nodesync_port(fault, seed), [], s["streams"][stream]
    for step in s["steps"]:
        if step[0] == "reset":
            port.reset(step[1], **step[2])
        elif step[0] == "set":
            port.set(step[1])
        else:
            _, soft, vinfo, ip, op, want_info = step
            S, ntx = soft.shape[:2]
            src, dst = Image(image(soft, ip or ntx, S, ntx, off), IN_ADDR), Image(image(None, op or ntx, S, ntx, 2), OUT_ADDR)
            info = port.push(src, IN_ADDR + off, ip, ntx, vinfo, dst, OUT_ADDR + 2, op, want_info)
            rows = dst.b[2:2 + 2 * S * (op or ntx)].reshape(S, op or ntx, 2)
            calls.append(dict(soft=rows[:, :ntx].copy().view(np.int8), info=info, state=port.state.copy()))
    if fault is None and seed is None:
        s[key] = (calls, port)
    return calls, port


def _traces(s):
    return [(stream, k, tr) for stream in range(len(s["streams"])) for k, tr in enumerate(run_port(s, stream)[1].traces)]


# ------------------------------------------------------------------------------------------ the product of candidate, head and alignment
SWEEP_NTX = {2: [27] + list(range(1, 27)) + [1100], 32: list(range(31, 59)) + [1100]}
# The lengths of the issue that asked for the sweep: 1..27 at nshift = 2 and 31..58, then 1100, at nshift = 32.  27 goes first at nshift = 2:
# only a link's first push can meet an erasure, and a push of 1 dibit has no chunk to meet it in.  The push of 1100 (a lane takes more than
# one chunk) is run at nshift = 2 as well.  What a geometry rules out is not asserted of it: at nshift = 32 a push is at least 31 dibits, so
# none is shorter than its head and none has fewer than 3 chunks.
IMPOSSIBLE = {2: (), 32: ("ntx below its head", "nchunk 0", "nchunk 1")}


def sweep(nshift):
    """nrot = 4: C = 4 nshift candidates x 8 output alignments, one link each, plus one so that the last workgroup holds a single wave.  An
    odd output pitch walks the eight heads from link to link; the input pitch is even, so every row of a stream stands the same 0 or 2
    bytes off a dword, and the two streams (first row 2 and 4 bytes behind a 16-byte boundary) give both."""
    name = "sweep(%d)" % nshift
    if name in _SETS:
        return _SETS[name]
    C = 4 * nshift
    S = 8 * C + 1
    rng = np.random.default_rng([nshift, 12])
    cand = (np.arange(S) // 8) % C
    cand = np.where(np.arange(S) % 2, cand - C * (1 + np.arange(S) % 5), cand + C * (np.arange(S) % 3)).astype(np.int32)      # congruent, signed and large
    sizes = SWEEP_NTX[nshift]
    soft = random_soft(rng, S, sum(sizes))
    steps, at = [("reset", S, dict(nrot=4, nshift=nshift)), ("set", cand)], 0
    for ntx in sizes:
        steps.append(("push", soft[:, at:at + ntx], None, (ntx | 1) + 3, (ntx | 1) + 2, True))
        at += ntx
    s = _SETS[name] = dict(name=name, streams=(2, 4), steps=steps, C=C, cand=cand)
    # ---- what it was built for, from the port's trace
    have = set()
    product = np.zeros((C, 8, 2), bool)                     # candidate x head x the funnel shift, over the body chunks of the vector route
    for stream, k, tr in _traces(s):
        ntx = sizes[k]
        have |= {"head %d" % v for v in np.unique(tr["head"][tr["head"] <= ntx])} | {"tail %d" % v for v in np.unique(tr["tail"])}
        have |= {"nchunk %d" % v for v in np.unique(tr["nchunk"]) if v < 2}
        for flag, what in (("first_dword_at_row_start", "k0 == 1 two bytes off a dword"), ("last_dword_at_row_end", "k0 + 10 == ntx on a dword"),
                           ("chunk_hist", "a gathered chunk: k0 < 1 into the history"), ("chunk_erasure", "a gathered chunk: k0 < 1 into an erasure"),
                           ("chunk_end", "a gathered chunk: k0 + 10 > ntx")):
            if tr[flag].any():
                have.add(what)
        if (tr["nchunk"] > 64).any():
            have.add("nchunk above 64")
        if (ntx < ((16 - ((OUT_ADDR + 2 + 2 * np.arange(S) * ((ntx | 1) + 2)) & 15)) & 15) >> 1).any():
            have.add("ntx below its head")
        if ntx == nshift - 1:
            have.add("ntx == nshift - 1")
        for bit in (0, 1):
            m = (tr["shifts"] >> bit & 1) != 0
            have |= {"shift %d at head %d" % (16 * bit, v) for v in np.unique(tr["head"][m])}
            product[np.arange(S)[m] // 8 % C, tr["head"][m], bit] = True
    want = (["head %d" % v for v in range(8)] + ["tail %d" % v for v in range(8)] + ["nchunk 0", "nchunk 1", "nchunk above 64"] +
            ["shift %d at head %d" % (sh, v) for sh in (0, 16) for v in range(8)] +
            ["k0 == 1 two bytes off a dword", "k0 + 10 == ntx on a dword", "a gathered chunk: k0 < 1 into the history",
             "a gathered chunk: k0 < 1 into an erasure", "a gathered chunk: k0 + 10 > ntx", "ntx below its head", "ntx == nshift - 1"])
    missing = [w for w in want if w not in have and w not in IMPOSSIBLE[nshift]]
    assert not missing, (name, missing)
    assert not [w for w in IMPOSSIBLE[nshift] if w in have], name
    assert product.all(), (name, "candidate x head x shift not met on the vector route", np.argwhere(~product)[:4])
    s["have"] = sorted(have)
    return s


# ------------------------------------------------------------------------------------------ every int8 pair
def every_pair():
    """dibit a * 256 + b of the first push is the pair (a, b) - 128 of int8: all 65536.  The second push holds the same pairs in the order
    i -> 40503 i + 1 mod 65536 (an odd factor: a permutation; the 1 moves every pair to a place of the other parity), so each pair stands
    in the other half of a dword, beside other neighbours.
    nrot = 4, nshift = 2: link c runs candidate c, r = c mod 4 at h = 0 (links 0..3) and h = 1 (links 4..7); every link gets the same row."""
    if "every_pair()" in _SETS:
        return _SETS["every_pair()"]
    v = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    x = np.stack([np.repeat(v, 256), np.tile(v, 256)], axis=-1)
    order = (40503 * np.arange(65536) + 1) % 65536
    assert len(np.unique(order)) == 65536 and (order % 2 != np.arange(65536) % 2).all()
    rows = [np.repeat(x[None], 8, axis=0), np.repeat(x[order][None], 8, axis=0)]
    steps = [("reset", 8, dict(nrot=4, nshift=2)), ("set", np.arange(8, dtype=np.int32))] + [("push", r, None, 65538, 65537, True) for r in rows]
    s = _SETS["every_pair()"] = dict(name="every_pair()", streams=(2,), steps=steps, order=order)
    # the expected output is the turn of the pairs after the -128 rule, a dibit late at h = 1
    whole, got = np.concatenate([rows[0][0], rows[1][0]]), np.concatenate([c["soft"] for c in run_ref(s)], axis=1)
    for c in range(8):
        t = turn_ref(minus128(whole), c % 4)
        assert np.array_equal(got[c], t if c < 4 else np.concatenate([np.zeros((1, 2), np.int8), t[:-1]])), c
    assert not (got == -128).any()
    for _, _, tr in _traces(s):
        assert (tr["nvec"] > 8000).all() and (tr["shifts"] > 0).all()
    return s


# ------------------------------------------------------------------------------------------ a switch at every push
WALK = dict(pushes=130, set_after=64, jump=37, kw=dict(nrot=4, nshift=32, span=1, settle=0, threshold=(0, 1), drop=1))


def walk_sizes():
    return [31 + p % 16 for p in range(WALK["pushes"])]


def walk():
    """one link per starting candidate of nrot = 4, nshift = 32.  span = 1 and the threshold 0 / 1 make every tick of (e, n) = (1, 1) a bad
    span, drop = 1 and settle = 0 make every bad span a switch: push p runs link l on candidate l + p + 1 (mod 128), each switch reading the
    carried history at a new delay, the lengths cycling through 31..46.  After 64 pushes a qpsk_nodesync_set moves every link 37 candidates
    on (the values congruent mod 128, half of them negative), history and switches kept."""
    if "walk()" in _SETS:
        return _SETS["walk()"]
    p, S = WALK, 128
    rng = np.random.default_rng(13)
    sizes = walk_sizes()
    soft = random_soft(rng, S, sum(sizes))
    steps, at = [("reset", S, p["kw"]), ("set", np.arange(S, dtype=np.int32))], 0
    for k, ntx in enumerate(sizes):
        if k == p["set_after"]:
            c = np.arange(S) + k + p["jump"]
            steps.append(("set", np.where(np.arange(S) % 2, c - 256, c).astype(np.int32)))
        vinfo = np.concatenate([np.ones((S, 2), np.int32), rng.integers(-5, 5, (S, 2)).astype(np.int32)], axis=1)
        steps.append(("push", soft[:, at:at + ntx], vinfo, 50, 49, True))
        at += ntx
    s = _SETS["walk()"] = dict(name="walk()", streams=(2,), steps=steps, soft=soft)
    want = run_ref(s)
    for k, c in enumerate(want):
        cand = (np.arange(S) + k + 1 + (p["jump"] if k >= p["set_after"] else 0)) % 128
        assert np.array_equal(c["info"][:, 0] + 4 * c["info"][:, 1], cand) and (c["info"][:, 3] == k + 1).all() and (c["info"][:, 4] == 2).all()
    traces = run_port(s)[1].traces
    wraps = [sum(tr["branch"][l] == "bad, switch over the wrap" for tr in traces) for l in range(S)]
    assert wraps.count(0) == p["jump"] and max(wraps) == 2      # all but the 37 links that the set takes over the wrap; some twice
    assert all(set(tr["branch"]) <= {"bad, switch", "bad, switch over the wrap"} for tr in traces)
    return s


def walk_recut():
    """the walk's dibits, ticks and set through nodesync_ref with OTHER CUTS: the lengths of every pair of pushes (2 i, 2 i + 1) swapped, so
    that the cut inside the pair falls elsewhere and every other cut, the set among them, stays.  Push p of either run stands on the same
    candidate.  -> (soft (S, total, 2) of all pushes in a row, per dibit the push it was part of, the same for the walk's own cuts)"""
    s = walk()
    if "_recut" not in s:
        sizes = walk_sizes()
        other = [sizes[k ^ 1] for k in range(len(sizes))]
        ref, at, outs, k = None, 0, [], 0
        for step in s["steps"]:
            if step[0] == "reset":
                ref = nodesync_ref(step[1], **step[2])
            elif step[0] == "set":
                ref.set(step[1])
            else:
                outs.append(ref.push(s["soft"][:, at:at + other[k]], step[2])["soft"])
                at += other[k]
                k += 1
        s["_recut"] = (np.concatenate(outs, axis=1), np.repeat(np.arange(len(other)), other), np.repeat(np.arange(len(sizes)), sizes))
    return s["_recut"]


# ------------------------------------------------------------------------------------------ the longest push
def limit():
    """one link on candidate (3, 31) of nrot = 4, nshift = 32: NODESYNC_MAX_NTX = 2^20 dibits in one push, then 31, every one of which
    comes out of the history, then 40 more (the GPU test puts a refused push in front of them)"""
    if "limit()" in _SETS:
        return _SETS["limit()"]
    rng = np.random.default_rng(14)
    soft = random_soft(rng, 1, (1 << 20) + 31 + 40)
    steps = [("reset", 1, dict(nrot=4, nshift=32)), ("set", np.array([127], np.int32)), ("push", soft[:, :1 << 20], None, 0, 0, True),
             ("push", soft[:, 1 << 20:(1 << 20) + 31], None, 0, 0, True), ("push", soft[:, (1 << 20) + 31:], None, 0, 0, True)]
    s = _SETS["limit()"] = dict(name="limit()", streams=(2,), steps=steps, soft=soft)
    tr = run_port(s)[1].traces
    assert tr[0]["nchunk"][0] == ((1 << 20) - 7) >> 3 and tr[1]["hist"][0] and not tr[1]["erasure"][0]
    assert tr[1]["nvec"][0] == 0 and tr[1]["row_reads"][0] == 0      # the last transform read no row
    return s


# ------------------------------------------------------------------------------------------ products that need 64 bits
def products():
    """one link, span = 2^24.  The tick test's products beyond 32 bits (threshold 65535 / 65535) differ by less than 2^31 from each other,
    so both wrap alike and an int32 compare gives the same verdicts.  Here one side wraps and the other does not: 40000 errors in 2^24 against
    1 / 65535 (40000 x 65535 is above 2^31: bad, int32 says good), then 200 in 2^24 against 65535 / 1 (65535 x 2^24 wraps below zero: good,
    int32 says bad).  A wrong verdict shows in d_info's locked, switches and verdict words."""
    if "products()" in _SETS:
        return _SETS["products()"]
    x = random_soft(np.random.default_rng(15), 1, 4)
    steps = []
    for threshold, e in (((1, 65535), 40000), ((65535, 1), 200)):
        steps.append(("reset", 1, dict(nrot=1, nshift=1, span=1 << 24, settle=0, threshold=threshold, drop=1)))
        steps.append(("push", x, np.array([[e, 1 << 24, 0, 0]], np.int32), 0, 0, True))
    s = _SETS["products()"] = dict(name="products()", streams=(2,), steps=steps)
    assert [c["info"][0, 2:5].tolist() for c in run_ref(s)] == [[0, 1, 2], [1, 0, 1]]
    assert 40000 * 65535 > 1 << 31 and 65535 << 24 > 1 << 31
    return s


# ------------------------------------------------------------------------------------------ what the suite ran before
CANDS = [0 + 4 * 0, 1 + 4 * 1, 2 + 4 * 7, 3 + 4 * 8, 1 + 4 * 31]


def old_transform():
    """test_nodesync_gpu.test_the_transform_bit_for_bit_at_every_alignment_and_across_the_cuts: its seed, links, cuts and pitches"""
    if "old transform" in _SETS:
        return _SETS["old transform"]
    rng = np.random.default_rng(6)
    S, total = 5, 31 + 33 + 516 + 2052
    soft = random_soft(rng, S, total)
    steps = []
    for sizes in ((31, 33, 516, 2052), (516, 33, 2052, 31)):
        steps += [("reset", S, dict(nrot=4, nshift=32)), ("set", np.array(CANDS, np.int32))]
        at = 0
        for ntx in sizes:
            steps.append(("push", soft[:, at:at + ntx], None, 2055, 2053, True))
            at += ntx
    steps += [("reset", 3, dict(nrot=1, nshift=1)), ("push", soft[:3, :700], None, 0, 0, False)]
    _SETS["old transform"] = dict(name="old transform", streams=(2,), steps=steps)
    return _SETS["old transform"]


def old_tick():
    """test_nodesync_gpu.test_the_tick_word_for_word_on_every_branch: its seed and its sequence of (e, n)"""
    if "old tick" in _SETS:
        return _SETS["old tick"]
    rng = np.random.default_rng(7)
    x = random_soft(rng, 3, 4)
    hand = [(5, 0), (30, 30), (30, 30), (4, 60), (6, 40), (11, 100), (0, 100), (11, 100), (11, 100), (0, 50), (50, 100)]
    calls = 48
    seq = np.zeros((calls, 3, 4), np.int32)
    seq[:, :, 2:] = rng.integers(-5, 5, (calls, 3, 2))
    seq[:len(hand), 0, :2] = hand
    n = rng.choice([0, 20, 60, 100, 130], (calls, 3))
    seq[len(hand):, 0, 1] = n[len(hand):, 0]
    seq[:, 1:, 1] = n[:, 1:]
    e = (n * rng.choice([0.02, 0.09, 0.11, 0.3], (calls, 3))).astype(np.int32)
    seq[len(hand):, 0, 0] = e[len(hand):, 0]
    seq[:, 1:, 0] = e[:, 1:]
    steps = [("reset", 3, dict(nrot=2, nshift=2, span=100, settle=50, threshold=(1, 10), drop=2)), ("set", np.array([3, 0, 6], np.int32)),
             ("push", x, None, 0, 0, True)] + [("push", x, seq[k], 0, 0, True) for k in range(calls)]
    steps.append(("reset", 1, dict(nrot=1, nshift=1, span=1 << 24, settle=0, threshold=(65535, 65535), drop=1)))
    for e_, n_ in [(1 << 23, 1 << 23), (1 << 23, 1 << 23), ((1 << 24) + 1, 1 << 24), ((1 << 24) - 1, 1 << 24)]:
        steps.append(("push", x[:1], np.array([[e_, n_, 0, 0]], np.int32), 0, 0, True))
    _SETS["old tick"] = dict(name="old tick", streams=(2,), steps=steps)
    return _SETS["old tick"]


BUILDERS = {"old tick": old_tick, "old transform": old_transform, "products()": products, "walk()": walk, "sweep(2)": lambda: sweep(2),
            "sweep(32)": lambda: sweep(32), "every_pair()": every_pair, "limit()": limit}
OLD = ("old tick", "old transform")
NEW = ("products()", "walk()", "sweep(2)", "sweep(32)", "every_pair()", "limit()")


def get(name):
    """a set by its name, built at the first call"""
    return BUILDERS[name]()
