"""deframe_hunt() of qpsk_amd/csrc/deframe_hunt.h restated in Python -- the TEMPLATE, not the header's definition: one stream at a time, its
DeframeHeader fields and its tail bytes as the state, X = [tail][row] loaded 64 positions at a time into two bit planes, the funnel64 windows
and the diff0 / diff1 algebra scored by three popcounts, the chunked walk over the candidate ballots with hx, the restart behind a packet,
the pending packet, the count < cap gate, the tail's write and the header's write-back.  What 64 lanes do at once is an array over the
lanes (uint64 words, as the device's); every wave-uniform variable keeps the kernel's name.  The policy is the caller's, as in the kernel:
the port calls ring(i), complete(slot, pos, rot, score, have, row0) and collect(have, row0, cnt, rot) exactly where the kernel does.
BytePackets and SoftPackets below are deframe.hip's and deframe_coded.hip's policies as far as the hunt can tell them apart: which values
end up in the packet, from the pending buffer and from the row.

test_hunt_port_cpu.py holds the port equal to the numpy restatements of the header (deframe_ref, deframe_coded_ref and its punctured and
interleaved forms) on every input the GPU tests push, so that the port stands for the template, and then uses it for what cannot be done on
a device:

  bounds   every push records the highest tail byte read and written, plane word asked for, row symbol handed to the policy, pending
           index written and slot completed; bounds() says which of them left what the kernel owns.  On the device none of these faults.
  faults   fault= switches on exactly ONE of FAULTS, a single wrong token each.  The GPU tests' inputs are adequate when every fault
           changes an output on them.  Nothing faulty exists outside this file: no kernel is ever built with one."""
import numpy as np

HUNT_CHUNK = 4
TAIL_BYTES = 128                                  # DEFRAME_PEND_OFFSET - DEFRAME_TAIL_OFFSET
ROOM = 256                                        # behind a pending buffer, so that an overrun is recorded instead of raised

FAULTS = (
    "tie_ge",           # c > best becomes >=: the LAST rotation with the largest count
    "gt_hx",            # gx + lane >= hx becomes >
    "skip_step",        # gx + 63 < hx becomes <=
    "restart",          # s = hx >> 6 becomes (hx + 63) >> 6
    "P_edge",           # gx + lane < P becomes < P - 1: the last position that completes in the push is dropped
    "pend_eq",          # nsym >= N - have becomes >
    "h_carry",          # h is not written back
    "hx_ge",            # hx > X becomes >=
    "m0_short",         # m0 one bit short
    "m1_short",         # m1 one bit short
    "load_guard",       # s + k - 2 < steps becomes s + k - 1 < steps
    "T2_short",         # T2 one short
    "row0_off",         # row0 = px + n - T + 1
    "got_off",          # got = nsym - row0 - 1
    "have_stuck",       # a collecting push does not advance have
    "cap_le",           # count < cap becomes <=
    "count_written",    # count advances only for written packets
)

_LANE = np.arange(64, dtype=np.uint64)
_LANE_I = np.arange(64, dtype=np.int64)
_FULL = (1 << 64) - 1


class HuntArgs:
    """what DeframeHuntArgs gives the hunt: nsync, min_score, the sync word's planes (api_packets.cpp: bit i % 64 of word i / 64 = bit 0 /
    bit 1 of ring(sync[i])), and nsym, set by every push"""

    def __init__(self, sync, min_score):
        sync = [int(v) for v in sync]
        self.nsync, self.min_score, self.nsym = len(sync), int(min_score), 0
        self.sync_lo, self.sync_hi = [0, 0], [0, 0]
        for i, v in enumerate(sync):
            r = v ^ (v >> 1)
            if r & 1:
                self.sync_lo[i >> 6] |= 1 << (i & 63)
            if r & 2:
                self.sync_hi[i >> 6] |= 1 << (i & 63)


class HuntState:
    """one stream's DeframeHeader and tail bytes, as the reset's memset leaves them"""

    def __init__(self):
        self.len = self.h = self.ppos = 0
        self.pending = self.have = self.prot = self.pscore = 0
        self.tail = [0] * TAIL_BYTES


def _funnel64(lo, hi):
    """funnel64 for lanes 0..63 at once: lane 0 takes lo as it is"""
    lo, hi = np.uint64(lo), np.uint64(hi)
    return np.where(_LANE == 0, lo, (lo >> _LANE) | (hi << ((np.uint64(64) - _LANE) & np.uint64(63))))


def _popc(x):
    return np.bitwise_count(x).astype(np.int64)


def deframe_hunt(a, N, cap, st, p, fault=None, seen=None):
    """one push of one stream -> count.  seen: a dict that takes this push's maxima (tail_read, tail_written, word, row, pend, slot; absent
    where nothing was touched) and iterations, steps, packets (the walk's: a pending packet completed in front of it costs it nothing)"""
    assert fault is None or fault in FAULTS, fault
    see = {} if seen is None else seen

    def note(key, v):
        if v > see.get(key, -1):
            see[key] = v

    def ring(i):
        note("row", i)
        return p.ring(i)

    def complete(slot, pos, rot, score, have, row0):
        note("slot", slot)
        if N - have > 0:
            note("row", row0 + N - have - 1)
        p.complete(slot, pos, rot, score, have, row0)

    def collect(have, row0, cnt, rot):
        if cnt > 0:
            note("row", row0 + cnt - 1)
            note("pend", have + cnt - 1)
        p.collect(have, row0, cnt, rot)

    n, nsym = a.nsync, a.nsym
    tail = st.tail
    len_, h, pending, have = st.len, st.h, st.pending, st.have
    T = min(len_, n - 1)
    count = 0

    # 1. the packet collecting since an earlier push
    if pending:
        ppos, prot, pscore = st.ppos, st.prot, st.pscore
        if (nsym > N - have) if fault == "pend_eq" else (nsym >= N - have):
            if count < cap:
                complete(count, ppos, prot, pscore, have, 0)
            count += 1
            pending = 0
        else:
            collect(have, 0, nsym, prot)
            if fault != "have_stuck":
                have += nsym

    # 2. the hunt over the positions whose word completes in this push
    base0 = len_ - T
    X = T + nsym
    P = X - n + 1
    iterations = steps = found = 0
    if not pending and P > 0 and h < base0 + P:
        hx = h - base0 if h > base0 else 0
        s0 = hx >> 6
        steps = (P + 63) >> 6

        def xload(w):
            """lanes 0..63 of xload(w) and the two ballots: the plane words (bit 0, bit 1) of positions 64 w .. 64 w + 63"""
            note("word", w)
            lo = hi = 0
            for lane in range(64):
                j = 64 * w + lane
                if j >= X:
                    break                                               # (the lanes behind it return 0 too)
                if j < T:
                    note("tail_read", j)
                    v = tail[j]
                else:
                    v = ring(j - T)
                lo |= (v & 1) << lane
                hi |= ((v >> 1) & 1) << lane
            return lo, hi

        m0 = _FULL if n >= 64 else (1 << n) - 1
        m1 = (_FULL if n == 128 else (1 << (n - 64)) - 1) if n > 64 else 0
        if fault == "m0_short":
            m0 >>= 1
        if fault == "m1_short":
            m1 >>= 1
        m0, m1 = np.uint64(m0), np.uint64(m1)
        sl0, sl1, sh0, sh1 = (np.uint64(v) for v in (a.sync_lo[0], a.sync_lo[1], a.sync_hi[0], a.sync_hi[1]))
        moved = False
        s = s0
        while s < steps:
            iterations += 1
            if iterations > steps + found + 8:
                break                                                   # (a fault that does not end: the caller sees the iterations)
            lo, hi = [0] * (HUNT_CHUNK + 2), [0] * (HUNT_CHUNK + 2)
            for k in range(HUNT_CHUNK + 2):
                if k < 2 or s + k - (1 if fault == "load_guard" else 2) < steps:
                    lo[k], hi[k] = xload(s + k)
            px, pk = -1, 0
            for k in range(HUNT_CHUNK):
                gx = 64 * (s + k)
                if px >= 0 or s + k >= steps or (gx + 63 <= hx if fault == "skip_step" else gx + 63 < hx):
                    continue
                x0, x1 = _funnel64(lo[k], lo[k + 1]), _funnel64(hi[k], hi[k + 1])
                d0 = x0 ^ sl0
                d1 = x1 ^ sh0 ^ (~x0 & sl0)
                c1, c2, c3 = _popc(~d1 & d0 & m0), _popc(d1 & ~d0 & m0), _popc(d1 & d0 & m0)
                if n > 64:
                    y0, y1 = _funnel64(lo[k + 1], lo[k + 2]), _funnel64(hi[k + 1], hi[k + 2])
                    d0 = y0 ^ sl1
                    d1 = y1 ^ sh1 ^ (~y0 & sl1)
                    c1, c2, c3 = c1 + _popc(~d1 & d0 & m1), c2 + _popc(d1 & ~d0 & m1), c3 + _popc(d1 & d0 & m1)
                best = n - c1 - c2 - c3                                # the first rotation with the largest count
                r = np.zeros(64, np.int64)
                for q, c in ((1, c1), (2, c2), (3, c3)):
                    up = c >= best if fault == "tie_ge" else c > best
                    best = np.where(up, c, best)
                    r = np.where(up, q, r)
                at = gx + _LANE_I
                mask = (at < (P - 1 if fault == "P_edge" else P)) & (at > hx if fault == "gt_hx" else at >= hx) & (best >= a.min_score)
                if mask.any():
                    first = int(np.argmax(mask))                        # ctz of the ballot
                    pk = int(best[first]) * 4 + int(r[first])
                    px = gx + first
            if px < 0:
                s += HUNT_CHUNK
                continue
            found += 1
            hx = px + n + N
            moved = True
            row0 = px + n - T + (1 if fault == "row0_off" else 0)
            if (hx >= X) if fault == "hx_ge" else (hx > X):              # collects into the next pushes
                got = nsym - row0 - (1 if fault == "got_off" else 0)
                collect(0, row0, got, pk & 3)
                pending = 1
                have = got
                st.ppos, st.prot, st.pscore = base0 + px, pk & 3, pk >> 2
                break
            written = (count <= cap) if fault == "cap_le" else (count < cap)
            if written:
                complete(count, base0 + px, pk & 3, pk >> 2, 0, row0)
            if written or fault != "count_written":
                count += 1
            s = (hx + 63) >> 6 if fault == "restart" else hx >> 6
        if moved and fault != "h_carry":
            h = base0 + hx

    # 3. the carried tail: the last min(len + nsym, nsync - 1) values of D, read before any lane writes
    len2 = len_ + nsym
    T2 = X if X < n - 1 else n - 1
    if fault == "T2_short" and T2 > 0:
        T2 -= 1
    tv = []
    for i in range(T2):
        j = X - T2 + i
        if j < T:
            note("tail_read", j)
            tv.append(tail[j])
        else:
            tv.append(ring(j - T))
    for i in range(T2):
        note("tail_written", i)
        tail[i] = tv[i]
    st.len, st.h, st.pending, st.have = len2, h, pending, have
    see["iterations"], see["steps"], see["packets"] = iterations, steps, found
    return count


def bounds(see, a, N, cap):
    """None where a push stayed inside what the kernel owns and its walk ended in time, or what it left"""
    n = a.nsync
    for key, limit, what in (("tail_read", n - 1, "tail byte read"), ("tail_written", n - 1, "tail byte written"),
                             ("word", see["steps"] + 2, "plane word"), ("row", a.nsym, "row symbol"), ("pend", N, "pending index"),
                             ("slot", cap, "slot")):
        if see.get(key, -1) >= limit:
            return "%s %d, the limit is %d" % (what, see[key], limit)
    if see["iterations"] > see["steps"] + see["packets"]:
        return "%d iterations for %d steps and %d packets" % (see["iterations"], see["steps"], see["packets"])
    return None


class BytePackets:
    """deframe.hip's policy for one push: row = the ring values of the push's row, pend = the stream's pending buffer (N + ROOM values).
    out takes (slot, pos, rot, score, the packet's N ring values: the first `have` from the pending buffer, the others from the row)"""

    def __init__(self, row, N, pend):
        self.row, self.N, self.pend, self.out = row, N, pend, []

    def ring(self, i):
        return int(self.row[i]) if 0 <= i < len(self.row) else 0        # (a faulty index: what lies there is not the stream's)

    def complete(self, slot, pos, rot, score, have, row0):
        self.out.append((slot, pos, rot, score, [self.pend[i] if i < have else self.ring(row0 + i - have) for i in range(self.N)]))

    def collect(self, have, row0, cnt, rot):
        for i in range(cnt):
            if 0 <= have + i < len(self.pend):
                self.pend[have + i] = self.ring(row0 + i)


class SoftPackets:
    """deframe_coded.hip's policy for one push, as far as the hunt sees it: a body is put together from pieces (row0, cnt, rot) of the rows
    of the pushes that brought them.  soften(row0, cnt, rot) -> cnt entries, the caller's restatement of quantise_body on THIS push's row
    and gain (entries behind the row: None).  out takes (slot, pos, rot, score, the body's N entries)"""

    def __init__(self, row, N, pend, soften):
        self.row, self.N, self.pend, self.soften, self.out = row, N, pend, soften, []

    def ring(self, i):
        return int(self.row[i]) if 0 <= i < len(self.row) else 0

    def complete(self, slot, pos, rot, score, have, row0):
        self.out.append((slot, pos, rot, score, list(self.pend[:have]) + list(self.soften(row0, self.N - have, rot))))

    def collect(self, have, row0, cnt, rot):
        for i, v in enumerate(self.soften(row0, cnt, rot)):
            if 0 <= have + i < len(self.pend):
                self.pend[have + i] = v
