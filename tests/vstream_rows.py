"""The streaming Viterbi decoder's input space as sets of calls, built once on the CPU and run by both sides: test_vstream_port_cpu.py runs the
scalar port (vstream_port.py) over them, test_viterbi_stream_sweep_gpu.py the device.  A set is a dict(name, steps, have):

  steps     ("reset", S, depth, window, pattern) | ("advance", delta) | ("flush", flags, want) |
            ("push", soft (S, ntx, 2) int8, dict(pitch, off, slack, want, fill)): the rows `pitch` dibits apart (0: ntx), the first row `off`
            bytes behind a 4-byte boundary, the bits rows `slack` bytes further apart than the call needs, want = which of "bits" and "info"
            the call asks for, fill = the byte the soft image holds outside its rows
  have      what the port's traces show on the set and what it was built for: asserted when the set is built, on the CPU

OLD are the inputs of test_viterbi_stream_gpu.py's decoder tests (its sections 1 to 8), rebuilt by its own code (pieces, SPLIT) at its seeds,
splits, pitches and advances: what the suite ran before.  NEW are the smallest shapes that reach what OLD does not; every stream has its own
content.  run_ref and run_port keep their results with the set: the reference of a set is computed once."""
import numpy as np

from test_punct_cpu import NAMED, PERIOD32, popc
from test_viterbi_stream_cpu import TERMINATED, random_soft, viterbi_step, viterbi_stream_ref
from test_viterbi_stream_gpu import FLUSH_PITCH, GUARD, pieces
from vstream_port import LANE, NEG, VS_LAST, VS_PEND, VS_RING, Image, vstream_port

SOFT_ADDR, BITS_ADDR, INFO_ADDR = 0x7F2A40000000, 0x7F2A80000000, 0x7F2AC0000000
BOTH = ("bits", "info")
_SETS = {}
U64 = np.uint64
_W64 = U64(1) << np.arange(64, dtype=U64)


def P(soft, pitch=0, off=0, slack=0, want=BOTH, fill=0x55):
    return ("push", np.ascontiguousarray(soft, np.int8), dict(pitch=pitch, off=off, slack=slack, want=want, fill=fill))


def F(flags=0, want=BOTH):
    return ("flush", flags, want)


def soft_image(soft, pitch, off, fill):
    """the bytes of a push's input: the first row `off` bytes in, `fill` everywhere outside the rows, GUARD bytes behind"""
    S, ntx = soft.shape[:2]
    pitch = pitch or ntx
    h = np.full(off + 2 * S * pitch + GUARD, fill, np.uint8)
    h[off:off + 2 * S * pitch].reshape(S, pitch, 2)[:, :ntx] = soft.view(np.uint8)
    return h


# ------------------------------------------------------------------------------------------ the state a device leaves where the reference stands
class expected_state:
    """the bytes of the state that are alive behind a call, from viterbi_stream_ref's books: pm as it stood at the last whole block (the
    definition's own viterbi_step over its own soft pairs where the push ended off the grid; compared after its maximum is taken off), the
    pending pairs of the steps behind the last whole block, the last emitted word, and the ring's blocks by slot: block j since the
    reset lies in slot j mod nring (an advance moves no block)"""

    def __init__(self, S, depth, window):
        self.S, self.nring = S, (depth + window) // 64
        self.stride = VS_RING + self.nring * 544
        self.img = np.zeros((S, self.stride), np.uint8)
        self.alive = np.zeros(self.stride, bool)
        self.fresh()

    def fresh(self):
        self.alive[:] = False
        self.alive[:VS_PEND] = self.alive[VS_LAST:VS_LAST + 8] = True
        self.img[:, :VS_PEND] = np.where(LANE == 0, 0, NEG).astype(np.int32).view(np.uint8)
        self.img[:, VS_LAST:VS_LAST + 8] = 0
        self.nb = 0
        self.pm = np.where(LANE == 0, 0, NEG).astype(np.int64)[None, :].repeat(self.S, axis=0)

    def behind_push(self, ref):
        S = self.S
        pc = ref.t % 64
        if pc == 0:
            self.pm = ref.pm.copy()
        else:
            for t in range(64 * self.nb, ref.t - pc):
                if t % 64 == 0:
                    self.pm = self.pm - self.pm.max(axis=1, keepdims=True)
                self.pm, _ = viterbi_step(self.pm, ref.soft[t][:, 0:1], ref.soft[t][:, 1:2])
        self.img[:, :VS_PEND] = np.ascontiguousarray(self.pm.astype(np.int32)).view(np.uint8)
        self.alive[VS_PEND:VS_LAST] = False
        if pc:
            self.img[:, VS_PEND:VS_PEND + 2 * pc] = np.stack(ref.soft[-pc:], axis=1).astype(np.int8).view(np.uint8).reshape(S, 2 * pc)
            self.alive[VS_PEND:VS_PEND + 2 * pc] = True
        n = ref.out.shape[1]
        if n >= 64:
            self.img[:, VS_LAST:VS_LAST + 8] = (ref.out[:, n - 64:].astype(U64) * _W64).sum(axis=1, dtype=U64)[:, None].view(np.uint8)
        nb = ref.t // 64
        for j in range(max(self.nb, nb - self.nring), nb):
            slot = j % self.nring
            dec = np.stack(ref.dec[64 * j:64 * j + 64])                                           # (64 steps, S)
            bit = (dec[:, :, None] >> LANE.astype(U64)[None, None, :]) & U64(1)                     # (step, S, state)
            words = (bit * _W64[:, None, None]).sum(axis=0, dtype=U64)                              # lane = state, bit = step
            a = VS_RING + 512 * slot
            self.img[:, a:a + 512] = np.ascontiguousarray(words).view(np.uint8)
            soft = np.stack(ref.soft[64 * j:64 * j + 64], axis=1)                                   # (S, 64, 2)
            bal = [((c.astype(U64)) * _W64).sum(axis=1, dtype=U64) for c in (soft[:, :, 0] < 0, soft[:, :, 0] != 0, soft[:, :, 1] < 0, soft[:, :, 1] != 0)]
            b = VS_RING + 512 * self.nring + 32 * slot
            self.img[:, b:b + 32] = np.ascontiguousarray(np.stack(bal, axis=1)).view(np.uint8)
            self.alive[a:a + 512] = self.alive[b:b + 32] = True
        self.nb = nb

    def snapshot(self):
        return dict(state=self.img[:, self.alive].copy(), alive=self.alive.copy())


def state_differs(got, want):
    """where a state image differs from the expected one on the bytes that are alive, pm after its own maximum is taken off; None if nowhere"""
    if got.shape[1] != want["alive"].size:
        return "the stride differs"
    g, w = got[:, want["alive"]].copy(), want["state"].copy()
    for x in (g, w):
        pm = x[:, :VS_PEND].view(np.int32)
        pm -= pm.max(axis=1, keepdims=True)
    if np.array_equal(g, w):
        return None
    s, k = np.argwhere(g != w)[0]
    return "stream %d, state byte %d" % (s, np.flatnonzero(want["alive"])[k])


# ------------------------------------------------------------------------------------------ running a set
def run_ref(s, state=True):
    """viterbi_stream_ref over the steps, once per set -> per push or flush dict(bits, nbits, info, state, alive); state = False leaves the
    expected state out (the device run has no use for it)"""
    if not state and "_ref" not in s:
        calls, ref = [], None
        for step in s["steps"]:
            if step[0] == "reset":
                ref = viterbi_stream_ref(step[1], step[2], step[3], step[4])
            elif step[0] in ("push", "flush"):
                calls.append(ref.push(step[1]) if step[0] == "push" else ref.flush(step[1]))
        return calls
    if "_ref" not in s:
        calls, ref, exp = [], None, None
        for step in s["steps"]:
            if step[0] == "reset":
                ref = viterbi_stream_ref(step[1], step[2], step[3], step[4])
                exp = expected_state(step[1], step[2], step[3])
            elif step[0] == "push":
                o = ref.push(step[1])
                exp.behind_push(ref)
                calls.append(dict(o, **exp.snapshot()))
            elif step[0] == "flush":
                o = ref.flush(step[1])
                exp.fresh()
                calls.append(dict(o, **exp.snapshot()))
        s["_ref"] = calls
    return s["_ref"]


def run_port(s, fault=None, seed=None):
    """the port over the steps -> (per push or flush dict(bits or None, nbits, info or None, state), the port); the unfaulted run from
    zeros is kept with the set"""
    if fault is None and seed is None and "_port" in s:
        return s["_port"]
    port, calls = vstream_port(fault, seed), []
    for step in s["steps"]:
        if step[0] == "reset":
            port.reset(*step[1:])
        elif step[0] == "advance":
            port.advance(step[1])
        else:
            S = port.S
            if step[0] == "push":
                soft, o = step[1], step[2]
                ntx, want = soft.shape[1], o["want"]
                bits_pitch = port.emits(ntx) // 8 + o["slack"]
            else:
                want, bits_pitch = step[2], FLUSH_PITCH
            bits = Image(np.full(S * bits_pitch + GUARD, 0x55, np.uint8), BITS_ADDR)
            info = Image(np.full(S * 16 + 4 * GUARD, 0x55, np.uint8), INFO_ADDR)
            b = (bits, BITS_ADDR, bits_pitch) if "bits" in want else None
            i = (info, INFO_ADDR) if "info" in want else None
            if step[0] == "push":
                src = Image(soft_image(soft, o["pitch"], o["off"], o["fill"]), SOFT_ADDR)
                nbits = port.push(src, SOFT_ADDR + o["off"], o["pitch"], ntx, b, i)
            else:
                nbits = port.flush(step[1], b, i)
            nb = (nbits + 7) // 8
            calls.append(dict(bits=bits.b[:S * bits_pitch].reshape(S, bits_pitch)[:, :nb].copy() if b else None, nbits=nbits,
                              info=info.b[:S * 16].view(np.int32).reshape(S, 4).copy() if i else None, state=port.state.copy()))
    if fault is None and seed is None:
        s["_port"] = (calls, port)
    return calls, port


def calls_of(s):
    """the steps that are calls with outputs, in order"""
    return [step for step in s["steps"] if step[0] in ("push", "flush")]


def _close(name, steps, want):
    """keep a set and assert from the port's traces that it holds what it was built for"""
    s = _SETS[name] = dict(name=name, steps=steps)
    calls, port = run_port(s)
    have = set()
    for tr in port.traces:
        if tr["kind"] == "flush":
            h = tr["have"]
            have.add("a flush of nothing" if tr["total"] == 0 else "a flush with pc %s 0" % (">" if tr["pc"] else "=="))
            if tr["pc"] == 0 and h > 0:
                have.add("a flush on the block grid with bits waiting")
                have.add("a flush on the grid with have = %d" % h)
                if tr["total"] % port.W == 0:
                    have.add("a flush at a decision point")
            if 0 < tr["total"] < 6:
                have.add("a flush of fewer than six steps")
            if tr["flags"]:
                have.add("TERMINATED")
        else:
            if tr["pc_after"] and tr["blocks"] == 0:
                have.add("a push that completes no block")
            if tr["pc"] and tr["blocks"]:
                have.add("a block of pending pairs and new ones")
            if tr["n"] == 131072:
                have.add("a push of 131072 steps")
        for d in tr["decisions"]:
            if d["nemit"] and max(d["step_ties"]) > 0:
                have.add("step ties on a walked path")
            if max(d["tied"]) == 64:
                have.add("a 64-way tie of the best state")
            if any(1 < v < 64 for v in d["tied"]):
                have.add("a tie of the best state between some states")
            if d["nemit"] == 0 and tr["kind"] == "push":
                have.add("a decision that emits nothing")
            if tr["kind"] == "push" and d["nemit"] and d["ntrace"] < port.nring:
                have.add("a decision while the trace is still growing")
            if d["ntrace"] == 128 and d["nskip"] == 127:
                have.add("a walk of 128 blocks with dblk = 127")
    missing = [w for w in want if w not in have]
    assert not missing, (name, "does not hold", missing, sorted(have))
    s["have"] = sorted(have)
    return s


def _set(name, build):
    return _SETS[name] if name in _SETS else build(name)


# ------------------------------------------------------------------------------------------ OLD: what test_viterbi_stream_gpu.py pushes
def cut(soft, sizes, **kw):
    out, at = [], 0
    for n in sizes:
        out.append(P(soft[:, at:at + n], **kw))
        at += n
    assert at == soft.shape[1]
    return out


def old_splits(name):
    S, N = 5, 1000
    soft = random_soft(np.random.default_rng(1), S, N)
    return _close(name, [("reset", S, 64, 64, (1, 1, 1))] + cut(soft, pieces(N)) + [F(), P(soft), F()], ["a block of pending pairs and new ones"])


def old_rings(name):
    steps = []
    for depth, window in ((192, 128), (64, 192)):
        S, N = 3, 1500
        soft = random_soft(np.random.default_rng(depth), S, N)
        steps += [("reset", S, depth, window, (1, 1, 1))] + cut(soft, pieces(N, (300, 1, 450, 77))) + [F(TERMINATED)]
    return _close(name, steps, ["TERMINATED"])


def old_limit(name):
    S, N = 2, 9000
    soft = random_soft(np.random.default_rng(4096), S, N)
    return _close(name, [("reset", S, 4096, 4096, (1, 1, 1))] + cut(soft, [4000, 4200, 800]) + [F()], [])


def old_punctured(name):
    steps = []
    for key in ("2/3", "3/4", "5/6", "7/8"):
        pattern = NAMED[key]
        K = popc(pattern[1]) + popc(pattern[2])
        unit = K // 2 if K % 2 == 0 else K
        sizes = [unit * k for k in (1, 2, 9, 65)] * 2
        soft = random_soft(np.random.default_rng(K), 3, sum(sizes))
        steps += [("reset", 3, 64, 64, pattern)] + cut(soft, sizes) + [F()]
    return _close(name, steps, ["a push that completes no block"])


def old_row_decoder(name):
    steps = []
    for flags in (0, TERMINATED):
        for key, N in (("1/2", 700), ("3/4", 702)):
            pattern = NAMED[key]
            ntx = N * (popc(pattern[1]) + popc(pattern[2])) // pattern[0] // 2
            soft = random_soft(np.random.default_rng(N + flags), 4, ntx)
            steps += [("reset", 4, 512, 512, pattern)] + cut(soft, [240, ntx - 240]) + [F(flags)]
    return _close(name, steps, ["a decision that emits nothing"])


def old_pitches(name):
    S, N, Pt = 3, 520, 531
    soft = random_soft(np.random.default_rng(5), S, N)
    steps = [("reset", S, 64, 128, (1, 1, 1)), P(soft[:, :N // 2], pitch=Pt, slack=5, fill=0x7F), P(soft[:, N // 2:], want=("bits",)), F(want=("info",))]
    return _close(name, steps, [])


def old_resets(name):
    soft = random_soft(np.random.default_rng(6), 4, 600)
    steps = [("reset", 4, 64, 64, (1, 1, 1))] + cut(soft, [333, 267]) + [("reset", 4, 64, 64, (1, 1, 1))] + cut(soft[:, ::-1], [100, 500])
    steps += [("reset", 2, 128, 64, NAMED["3/4"])] + cut(soft[:2], [200, 400]) + [F()] + cut(soft[2:], [90, 510]) + [F(TERMINATED), F()]
    return _close(name, steps, ["a flush of nothing"])


def old_isolation(name):
    soft = random_soft(np.random.default_rng(7), 3, 900)
    return _close(name, [("reset", 3, 128, 64, (1, 1, 1))] + cut(soft, [450, 450]) + [F()], [])


def old_positions(name):
    S, depth, window = 3, 192, 128
    soft = random_soft(np.random.default_rng(8), S, 1400)
    steps = [("reset", S, depth, window, (1, 1, 1))] + cut(soft[:, :421], [300, 121]) + [("advance", 1 << 40)] + cut(soft[:, 421:], [3, 400, 576])
    steps += [("advance", (1 << 62) // window * window), F()]
    return _close(name, steps, [])


# ------------------------------------------------------------------------------------------ NEW
def flush_on_the_grid(name):
    """D = 64, W = 128: a flush at 64 steps (before any decision, have = 1), at 192 (between decisions, have = 2), at 256 (exactly at a
    decision point, have = D / 64 = 1) and at 448 (later, have = 2), each behind pushes off the block grid and followed by a short push and
    a flush that find the state of a reset"""
    S = 4
    rng = np.random.default_rng(21)
    steps = [("reset", S, 64, 128, (1, 1, 1))]
    for total, flags in ((64, 0), (64, TERMINATED), (192, 0), (192, TERMINATED), (256, 0), (448, 0)):
        steps += cut(random_soft(rng, S, total), pieces(total)) + [F(flags)] + cut(random_soft(rng, S, 70), [70]) + [F()]
    return _close(name, steps, ["a flush on the block grid with bits waiting", "a flush on the grid with have = 1", "a flush on the grid with have = 2",
                                "a flush at a decision point", "TERMINATED"])


def short_streams(name):
    S = 3
    rng = np.random.default_rng(22)
    steps = [("reset", S, 64, 64, (1, 1, 1))]
    for total in (1, 2, 5, 6, 7, 63):
        for flags in (0, TERMINATED):
            steps += cut(random_soft(rng, S, total), pieces(total, (2, 1, 60))) + [F(flags)]
    return _close(name, steps, ["a flush of fewer than six steps", "TERMINATED", "a push that completes no block"])


TIES = dict(N=64 * 5 + 17, run=6, at=(128, 256))


def ties(name):
    """stream 0: erasures only; 1: -128 only; 2 and 3: values in {-1, 0, 1}; 4: random content with six erasure steps that end exactly at
    the decision points 128 and 256 (all 64 metrics equal: the tie rule picks the state); 5: the same run ending one step earlier"""
    N, S = TIES["N"], 6
    rng = np.random.default_rng(23)
    soft = random_soft(rng, S, N)
    soft[0] = 0
    soft[1] = -128
    soft[2:4] = rng.integers(-1, 2, (2, N, 2))
    for T in TIES["at"]:
        soft[4, T - TIES["run"]:T] = 0
        soft[5, T - TIES["run"] - 1:T - 1] = 0
        soft[5, T - 1] = (77, -31)
    s = _close(name, [("reset", S, 64, 64, (1, 1, 1))] + cut(soft, pieces(N)) + [F()],
               ["a 64-way tie of the best state", "step ties on a walked path", "a tie of the best state between some states"])
    tied = np.array([d["tied"] for tr in run_port(s)[1].traces if tr["kind"] == "push" for d in tr["decisions"]])      # (decision, stream)
    assert tied.shape == (5, S) and (tied[:, 0] == 64).all() and (tied[[1, 3], 4] == 64).all() and (tied[[1, 3], 5] == 32).all(), tied
    return s


def rings(name):
    """(128, 64): decisions while the trace is still growing, dblk > wblk; (64, 4096); (8128, 64): the ring of 128 blocks with dblk = 127,
    pushed just past 8192 + 3 x 64 steps so that it wraps once it is full.  All on the repeating split off the block grid"""
    steps = []
    for k, (depth, window, N) in enumerate(((128, 64, 64 * 7 + 30), (64, 4096, 8300), (8128, 64, 8192 + 3 * 64 + 10))):
        soft = random_soft(np.random.default_rng([24, k]), 2, N)
        steps += [("reset", 2, depth, window, (1, 1, 1))] + cut(soft, pieces(N)) + [F(TERMINATED if k == 1 else 0)]
    return _close(name, steps, ["a decision while the trace is still growing", "a walk of 128 blocks with dblk = 127", "a decision that emits nothing"])


def one_period_pushes(name):
    steps = []
    for k, pattern in enumerate([NAMED[key] for key in sorted(NAMED)] + [PERIOD32]):
        K = popc(pattern[1]) + popc(pattern[2])
        unit = K // 2 if K % 2 == 0 else K
        soft = random_soft(np.random.default_rng([25, k]), 3, 30 * unit)
        steps += [("reset", 3, 64, 64, pattern)] + cut(soft, [unit] * 30) + [F()]
    return _close(name, steps, ["a push that completes no block", "a block of pending pairs and new ones"])


def many_streams(name):
    S = 300
    soft = random_soft(np.random.default_rng(26), S, 200)
    steps = [("reset", S, 64, 64, (1, 1, 1))]
    steps += [P(soft[:, a:b], pitch=b - a + 1, slack=3) for a, b in ((0, 70), (70, 135), (135, 200))] + [F()]
    return _close(name, steps, [])


def alignment(name):
    """the soft image 2 bytes off a 4-byte boundary and rows an odd number of dibits apart, for PairLoader and PunctLoader"""
    steps = []
    for k, (pattern, sizes) in enumerate((((1, 1, 1), (33, 100, 167)), (NAMED["7/8"], (4, 100, 196)))):
        soft = random_soft(np.random.default_rng([27, k]), 3, sum(sizes))
        steps += [("reset", 3, 64, 64, pattern)] + cut(soft, sizes, pitch=201, off=2, slack=1) + [F()]
    return _close(name, steps, [])


LONGEST_S = 1
LONGEST = {"longest_push 1/2": ((1, 1, 1), 131072), "longest_push 7/8": (NAMED["7/8"], 74896)}


def longest_push(name):
    """one push of VITERBI_MAX_STEPS = 131072 steps at rate 1/2, or one of 131068 steps (74896 dibits) at 7/8, D = W = 64, a set each.  One
    stream: viterbi_stream_ref alone takes three to four seconds per stream and case"""
    pattern, ntx = LONGEST[name]
    soft = random_soft(np.random.default_rng([28, ntx]), LONGEST_S, ntx)
    return _close(name, [("reset", LONGEST_S, 64, 64, pattern), P(soft), F()], ["a push of 131072 steps"] if ntx == 131072 else ["a flush with pc > 0"])


BUILDERS = {"old splits": old_splits, "old rings": old_rings, "old limit": old_limit, "old punctured": old_punctured,
            "old row decoder": old_row_decoder, "old pitches": old_pitches, "old resets": old_resets, "old isolation": old_isolation,
            "old positions": old_positions,
            "flush_on_the_grid": flush_on_the_grid, "short_streams": short_streams, "ties": ties, "rings": rings,
            "one_period_pushes": one_period_pushes, "many_streams": many_streams, "alignment": alignment, "longest_push 1/2": longest_push, "longest_push 7/8": longest_push}
OLD = ("old splits", "old rings", "old limit", "old punctured", "old row decoder", "old pitches", "old resets", "old isolation", "old positions")
NEW = ("short_streams", "flush_on_the_grid", "ties", "one_period_pushes", "alignment", "many_streams", "rings", "longest_push 1/2", "longest_push 7/8")


def get(name):
    """a set by its name, built at the first call"""
    return _set(name, BUILDERS[name])
