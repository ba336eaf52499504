"""nodesync_push_kernel and nodesync_init_kernel of qpsk_amd/csrc/nodesync.hip, with the host's part of qpsk_nodesync_* (api_nodesync.cpp: the
pitches in force, `have`), restated in numpy -- the KERNELS, not the header: the tick on int32 header words, the carried history copied into
the LDS before the transform and stored back behind it, the output row cut into head, body and tail by the OUTPUT's address, each body chunk
on the vector route (five aligned dwords and a funnel shift) or the gather (row, history slot, erasure) by the kernel's own condition, and
turn_packed on uint32 with the kernel's masks and adds.  The definition stays test_nodesync_cpu.nodesync_ref.

The port works on BYTE IMAGES AT SIMULATED ADDRESSES: an Image is a flat uint8 array whose byte i stands at address addr + i; d_soft_in and
d_soft_out are addresses inside one, pitches are in dibits.  So the alignment of either buffer is a parameter, and what the device cannot show
is on record:

  reads     every read of an input image as (links, addresses, bytes each); each has to lie in its link's row [in + 2 link pitch, + 2 ntx).
            A read in front of or behind a row fetches a neighbour's bytes or poison, the funnel shift throws them away and every output
            stays right: only the record shows it.  hist_reads holds the LDS slots read, each one of the link's H = nshift - 1.
  writes    per push how often every byte of the output image was written: once inside a link's row, never outside.  A byte written
            twice with the same value fails nothing on a device.
  stores16  the address of every 16-byte store; each has to be a multiple of 16.
  headers   per push whether the header was stored; it is only with a d_vinfo.
  traces    per push a dict of arrays over the links (trace(push, link) gives one link's as a dict): head, tail, nchunk, the chunks per
            route (nvec, ngather), the funnel shifts used (bit 0: by 0, bit 1: by 16), whether a vector chunk had k0 == 1 / k0 + 10 == ntx
            (k0_1, k0_10) and under which shift (first_dword_at_row_start: k0 == 1 two bytes off a dword, so the first dword read begins
            with the row; last_dword_at_row_end: k0 + 10 == ntx on a dword), whether a gathered chunk reached the history or an erasure or
            lay at the row's end (chunk_hist, chunk_erasure, chunk_end), whether any gather did (hist, erasure), how many reads of the
            row the transform made (row_reads), and the tick's verdict and branch.
  broken    what left a bound, by kind (KINDS), the first of each kind as text.

The loop over a link's chunks, the 64 lanes and the 16 lanes of head and tail are arrays here; the tick is scalar per link.  A launch finds
the LDS (and a reset its fresh state) holding anything: with seed= both start as random bytes.

fault= switches on exactly ONE of FAULTS, a single wrong token each, or one of EQUIVALENT, which no input can show."""
import numpy as np

NS_HDR, STRIDE, MAX_SHIFT, MAX_NTX = 32, 96, 32, 1 << 20

FAULTS = (
    # the transform and the history
    "the vector route at k0 >= 0",                           # reads the 2 bytes in front of a row that is 2 bytes off a dword
    "the vector route at k0 + 9 <= ntx",                     # reads the dword behind a row that ends on a dword
    "the shift fixed at 0",
    "the shift fixed at 16",
    "the head taken from the input's address",               # body stores that are not 16-byte aligned
    "the tail's bound <= ntx",                               # out[ntx] written
    "the history slot H + k + 1",
    "the erasure test -k < have",
    "the history stored from ntx - H + k - 1",
    "the history stored before the transform reads it",
    "no -128 rule",
    "the -128 rule applied after the turn",
    "the negation's add without its 0x7f7f7f7f mask",
    "the swap applied for even r",
    "the mask of r = 3 equal to that of r = 1",
    # the tick and the set
    "bad on >=",
    "the span test on cnt > span",
    "run > drop",
    "the wrap at c + 1 == C + 1",
    "settle_left not clamped at 0",
    "the products in int32",
    "locked kept on a switch",
    "err and cnt kept after a span",
    "a tick at n == 0",
    "the header stored without a d_vinfo",                   # the same words again: only the record of header stores shows it
    "qpsk_nodesync_set clearing switches",
    "cand reduced as a signed value",
)
# Not in the list, because no input can show them; the port still takes each as fault=, and test_nodesync_port_cpu.py checks on every set
# that no output, d_info word or state changes:
EQUIVALENT = {
    "the erasure test have == 0": "the host's have only ever takes 0 and nshift - 1, because a push is at least nshift - 1 long: -k <= have "
                                  "with 1 <= -k <= nshift - 1 asks no more than whether have is 0",
    "head and tail on each other's lanes": "which lanes gather the head and the tail (0..7 and 8..15) is no output's business: lane i of "
                                           "either group takes dibit i of its part, whichever group goes first",
    "the wrap as (c + 1) % C": "0 <= c < C always (the set reduces cand, the reset gives 0), so c + 1 == C ? 0 : c + 1 is the remainder",
}
KINDS = ("reads", "history", "outside", "twice", "unwritten", "stores16", "header")
DEVICE_SEES = ("soft", "info", "outside", "unwritten")      # of all evidence, what a GPU test can see: outputs, d_info, the poison and guards

M7, M8, ONES = np.uint32(0x7f7f7f7f), np.uint32(0x80808080), np.uint32(0x01010101)
LO, HI, ALL = np.uint32(0x00ff00ff), np.uint32(0xff00ff00), np.uint32(0xffffffff)


def w32(x):
    """a Python integer as the int32 the device holds"""
    return (int(x) + (1 << 31)) % (1 << 32) - (1 << 31)


def turn_packed(x, r, fault=None):
    """the kernel's turn_packed on uint32 arrays: four int8 (a0, b0, a1, b1) = two dibits, the -128 rule, then turn_r (r an int or an array)"""
    x = np.atleast_1d(np.asarray(x, np.uint32))
    r = np.broadcast_to(np.asarray(r, np.int64), x.shape)

    def rule(x):
        t = x ^ M8
        return x | ((~(((t & M7) + M7) | t | M7)) >> np.uint32(7))      # bytes that are 0x80 become 0x81
    if fault not in ("no -128 rule", "the -128 rule applied after the turn"):
        x = rule(x)
    odd = (r & 1) != 0
    if fault == "the swap applied for even r":
        odd = ~odd
    x = np.where(odd, ((x >> np.uint32(8)) & LO) | ((x << np.uint32(8)) & HI), x)
    nx = ~x
    neg = ((nx if fault == "the negation's add without its 0x7f7f7f7f mask" else nx & M7) + ONES) ^ (nx & M8)
    m3 = HI if fault == "the mask of r = 3 equal to that of r = 1" else LO
    m = np.where(r == 0, np.uint32(0), np.where(r == 1, HI, np.where(r == 2, ALL, m3))).astype(np.uint32)
    x = (x & ~m) | (neg & m)
    if fault == "the -128 rule applied after the turn":
        x = rule(x)
    return x


class Image:
    """bytes at simulated addresses: b[i] stands at addr + i"""

    def __init__(self, b, addr):
        self.b, self.addr = np.ascontiguousarray(b, np.uint8), int(addr)
        assert self.b.ndim == 1


class nodesync_port:
    """reset() / set() / push() as qpsk_nodesync_reset / _set / _push.  push(src, d_soft_in, in_pitch, ntx, vinfo, dst, d_soft_out, out_pitch)
    writes into the Image dst and returns d_info (S, 8) int32 or None; .state is the device state as bytes."""

    def __init__(self, fault=None, seed=None):
        assert fault is None or fault in FAULTS or fault in EQUIVALENT, fault
        self.fault = fault
        self.rng = None if seed is None else np.random.default_rng(seed)
        self.state = None
        self.reads, self.hist_reads, self.writes, self.stores16, self.headers, self.traces = [], [], [], [], [], []
        self.broken = {}

    def _junk(self, n):
        return np.zeros(n, np.uint8) if self.rng is None else self.rng.integers(0, 256, n).astype(np.uint8)

    def _break(self, kind, text):
        self.broken.setdefault(kind, "push %d: %s" % (len(self.traces), text))

    def trace(self, push, link):
        return {k: (v[link].item() if isinstance(v, np.ndarray) else v[link]) for k, v in self.traces[push].items()}

    # ------------------------------------------------------------------ the host: api_nodesync.cpp
    def reset(self, nlinks, nrot=2, nshift=1, span=4096, settle=1024, threshold=(1, 32), drop=2):
        self.S, self.nrot, self.nshift, self.span, self.settle, self.drop = nlinks, nrot, nshift, span, settle, drop
        self.num, self.den = threshold
        self.have = 0
        self.state = self._junk(nlinks * STRIDE)             # a fresh allocation holds anything
        self._init(None, False)

    def set(self, cand=None):
        self._init(None if cand is None else np.asarray(cand, np.int32), True)

    def _init(self, cand, keep):
        """nodesync_init_kernel"""
        w = self.state.view(np.int32).reshape(self.S, STRIDE // 4)
        C = self.nrot * self.nshift
        if not keep:
            w[:] = 0
            return
        if cand is None:
            w[:, 0] = 0
        elif self.fault == "cand reduced as a signed value":
            w[:, 0] = np.fmod(cand.astype(np.int64), C)      # C's %: the sign of the dividend
        else:
            w[:, 0] = cand.astype(np.int64) % (1 << 32) % C  # (unsigned)cand % C
        w[:, 1:5] = 0
        w[:, 5] = self.settle
        if self.fault == "qpsk_nodesync_set clearing switches":
            w[:, 6] = 0

    # ------------------------------------------------------------------ memory, on record
    def _read(self, src, link, addr, n, row, ntx):
        """n bytes at each address of the input image -> (len, n) uint8; a read outside its link's row is recorded and, outside the image, 0xAA"""
        self.reads.append((link, addr, n))
        lo = row[link]
        out = (addr < lo) | (addr + n > lo + 2 * ntx)
        if out.any():
            i = int(np.flatnonzero(out)[0])
            self._break("reads", "link %d reads %d bytes at row %+d, the row has %d" % (link[i], n, addr[i] - lo[i], 2 * ntx))
        idx = (addr - src.addr)[:, None] + np.arange(n)
        ok = (idx >= 0) & (idx < src.b.size)
        return np.where(ok, src.b[np.clip(idx, 0, src.b.size - 1)], np.uint8(0xAA))

    def _store(self, dst, count, addr, vals):
        """vals (len, n) uint8 to the output image at each address, every byte counted"""
        n = vals.shape[1]
        idx = (addr - dst.addr)[:, None] + np.arange(n)
        ok = (idx >= 0) & (idx < dst.b.size)
        if not ok.all():
            self._break("outside", "a store outside the output image")
        np.add.at(count, idx[ok], 1)
        dst.b[idx[ok]] = vals[ok]

    # ------------------------------------------------------------------ nodesync_push_kernel
    def push(self, src, d_soft_in, in_pitch, ntx, vinfo, dst, d_soft_out, out_pitch, want_info=True):
        f, S, nrot = self.fault, self.S, self.nrot
        H, C = self.nshift - 1, self.nrot * self.nshift
        assert self.state is not None and 1 <= ntx <= MAX_NTX and ntx >= H, "refused: ntx"
        ip, op = in_pitch or ntx, out_pitch or ntx
        assert ip >= ntx and op >= ntx and d_soft_in % 2 == 0 and d_soft_out % 2 == 0, "refused: pitch or alignment"
        have = self.have
        hdr = self.state.view(np.int32).reshape(S, STRIDE // 4)
        shist = self.state.reshape(S, STRIDE)[:, NS_HDR:NS_HDR + 2 * MAX_SHIFT]
        link = np.arange(S, dtype=np.int64)
        tr = dict(verdict=np.zeros(S, np.int64), branch=["no d_vinfo"] * S)

        # ---- 1. the tick: int32 words, int64 products
        if vinfo is not None:
            vinfo = np.asarray(vinfo, np.int32)
            for l in range(S):
                c, locked, run, err, cnt, settle_left, switches = (int(v) for v in hdr[l, :7])
                e, n = int(vinfo[l, 0]), int(vinfo[l, 1])
                verdict, branch = 0, "n <= 0"
                if n > 0 or (f == "a tick at n == 0" and n == 0):
                    if settle_left > 0:
                        settle_left = settle_left - n if f == "settle_left not clamped at 0" else max(0, settle_left - n)
                        verdict, branch = 3, "settle"
                    else:
                        err, cnt, branch = w32(err + e), w32(cnt + n), "counting"
                        if cnt > self.span if f == "the span test on cnt > span" else cnt >= self.span:
                            lhs, rhs = err * self.den, self.num * cnt
                            if f == "the products in int32":
                                lhs, rhs = w32(lhs), w32(rhs)
                            bad = lhs >= rhs if f == "bad on >=" else lhs > rhs
                            if f != "err and cnt kept after a span":
                                err = cnt = 0
                            if not bad:
                                run, locked, verdict, branch = 0, 1, 1, "good"
                            else:
                                verdict, branch = 2, "bad, held"
                                run += 1
                                if not locked or (run > self.drop if f == "run > drop" else run >= self.drop):
                                    if f == "the wrap as (c + 1) % C":
                                        c = (c + 1) % C
                                    else:
                                        c = 0 if c + 1 == (C + 1 if f == "the wrap at c + 1 == C + 1" else C) else c + 1
                                    if f != "locked kept on a switch":
                                        locked = 0
                                    run, settle_left, switches = 0, self.settle, w32(switches + 1)
                                    branch = "bad, switch over the wrap" if c == 0 else "bad, switch"
                hdr[l, :7] = (c, locked, run, err, cnt, settle_left, switches)
                tr["verdict"][l], tr["branch"][l] = verdict, branch
        stored = vinfo is not None or f == "the header stored without a d_vinfo"
        if stored and vinfo is None:
            hdr[:, :7] = hdr[:, :7].copy()                   # the words it read, again
            self._break("header", "the header stored without a d_vinfo")
        self.headers.append(stored)
        c = hdr[:, 0].astype(np.int64)
        r = np.fmod(c, nrot)                                 # C's % and /: what a c outside 0..C - 1 would give
        h = (c - r) // nrot
        info = None
        if want_info:
            info = np.stack([r, h, hdr[:, 1], hdr[:, 6], tr["verdict"], hdr[:, 2], hdr[:, 3], hdr[:, 4]], axis=1).astype(np.int32)

        in_row, out_row = d_soft_in + 2 * link * ip, d_soft_out + 2 * link * op

        def history_out():                                   # 4. the row's last H dibits, raw
            if H:
                k = np.arange(H) - (1 if f == "the history stored from ntx - H + k - 1" else 0)
                a = (in_row[:, None] + 2 * (ntx - H + k)[None, :]).reshape(-1)
                shist[:, :2 * H] = self._read(src, np.repeat(link, H), a, 2, in_row, ntx).reshape(S, 2 * H)
        if f == "the history stored before the transform reads it":
            history_out()

        # ---- 2. the carried history into the LDS: a slice of MAX_SHIFT slots per wave, whatever the last workgroup left in it
        lds = self._junk(2 * MAX_SHIFT * (S + 2)).view(np.uint16)       # a slice of room either side: a slot outside its slice is recorded
        lh = MAX_SHIFT * (link + 1)
        if H:
            lds[lh[:, None] + np.arange(H)] = np.ascontiguousarray(shist[:, :2 * H]).view(np.uint16)

        # ---- 3. the transform
        flags = dict(hist=np.zeros(S, bool), erasure=np.zeros(S, bool), row_reads=np.zeros(S, np.int64))

        def source(L, k):
            """Source::operator() on arrays: raw dibit k of link L as uint32"""
            L, k = np.broadcast_arrays(L, k)
            shape = k.shape
            L, k = L.reshape(-1), k.reshape(-1)
            out = np.zeros(k.size, np.uint32)
            row = k >= 0
            if row.any():
                np.add.at(flags["row_reads"], L[row], 1)
                b = self._read(src, L[row], in_row[L[row]] + 2 * k[row], 2, in_row, ntx).astype(np.uint32)
                out[row] = b[:, 0] | (b[:, 1] << np.uint32(8))
            if f == "the erasure test -k < have":
                held = ~row & (-k < have)
            elif f == "the erasure test have == 0":
                held = ~row & (have != 0)
            else:
                held = ~row & (-k <= have)
            if held.any():
                slot = H + k[held] + (1 if f == "the history slot H + k + 1" else 0)
                self.hist_reads.append((L[held], slot))
                if ((slot < 0) | (slot >= H)).any():
                    self._break("history", "slot %d of %d read" % (slot[(slot < 0) | (slot >= H)][0], H))
                out[held] = lds[np.clip(lh[L[held]] + slot, 0, lds.size - 1)]
                flags["hist"][L[held]] = True
            flags["erasure"][L[~row & ~held]] = True
            return out.reshape(shape), held.reshape(shape), (~row & ~held).reshape(shape)

        count = np.zeros(dst.b.size, np.int32)
        at = in_row if f == "the head taken from the input's address" else out_row
        head = np.minimum(ntx, ((16 - (at & 15)) & 15) >> 1)
        nchunk = (ntx - head) >> 3
        tail0 = head + 8 * nchunk
        # head: lanes 0..6; tail: lanes 8..14
        lane = np.arange(16)[None, :]
        first = lane >= 8 if f == "head and tail on each other's lanes" else lane < 8
        t = tail0[:, None] + (lane & 7)
        in_tail = t <= ntx if f == "the tail's bound <= ntx" else t < ntx
        j = np.where(first, np.where((lane & 7) < head[:, None], lane & 7, -1), np.where(in_tail, t, -1))
        L, lanes = np.nonzero(j >= 0)
        J = j[L, lanes]
        raw, _, _ = source(L, J - h[L])
        v = turn_packed(raw, r[L], f)
        self._store(dst, count, out_row[L] + 2 * J, np.stack([v & np.uint32(0xff), (v >> np.uint32(8)) & np.uint32(0xff)], 1).astype(np.uint8))

        # body: chunk q of a link goes to lane q % 64
        Lc = np.repeat(link, nchunk)
        q = np.arange(Lc.size) - np.repeat(np.cumsum(nchunk) - nchunk, nchunk)
        j0 = head[Lc] + 8 * q
        k0 = j0 - h[Lc]
        vec = (k0 >= (0 if f == "the vector route at k0 >= 0" else 1)) & (k0 + (9 if f == "the vector route at k0 + 9 <= ntx" else 10) <= ntx)
        o = np.zeros((Lc.size, 4), np.uint32)
        p = in_row[Lc[vec]] + 2 * k0[vec]
        sh = (p & 2) * 8
        if f == "the shift fixed at 0":
            sh[:] = 0
        elif f == "the shift fixed at 16":
            sh[:] = 16
        if vec.any():
            np.add.at(flags["row_reads"], Lc[vec], 5)
            w = self._read(src, Lc[vec], p & ~3, 20, in_row, ntx).reshape(-1, 5, 4).astype(np.uint64)
            w = w[:, :, 0] | (w[:, :, 1] << np.uint64(8)) | (w[:, :, 2] << np.uint64(16)) | (w[:, :, 3] << np.uint64(24))
            o[vec] = (((w[:, :4] | (w[:, 1:] << np.uint64(32))) >> sh.astype(np.uint64)[:, None]) & np.uint64(0xffffffff)).astype(np.uint32)
        g = ~vec
        reached_hist, reached_erasure = np.zeros(Lc.size, bool), np.zeros(Lc.size, bool)
        if g.any():
            d, was_hist, was_erasure = source(Lc[g][:, None], k0[g][:, None] + np.arange(8)[None, :])
            o[g] = d[:, 0::2] | (d[:, 1::2] << np.uint32(16))
            reached_hist[g], reached_erasure[g] = was_hist.any(1), was_erasure.any(1)
        v = turn_packed(o, r[Lc][:, None], f)
        a16 = out_row[Lc] + 2 * j0
        self.stores16.append(a16)
        if (a16 & 15).any():
            self._break("stores16", "a 16-byte store at ...%x" % (a16[(a16 & 15) != 0][0] & 0xff))
        self._store(dst, count, a16, np.ascontiguousarray(v).view(np.uint8).reshape(-1, 16))

        # ---- 4. the history behind this push
        if f != "the history stored before the transform reads it":
            history_out()

        # every byte of every row exactly once, none elsewhere
        self.writes.append(count)
        rows = (out_row - dst.addr)[:, None] + np.arange(2 * ntx)[None, :]
        if rows.min() >= 0 and rows.max() < count.size:
            inside = count[rows]
            if (inside > 1).any():
                self._break("twice", "link %d: a byte written %d times" % (np.argwhere(inside > 1)[0][0], inside.max()))
            if (inside == 0).any():
                self._break("unwritten", "link %d: dibit %d not written" % tuple(np.argwhere(inside == 0)[0] // (1, 2)))
            if count.sum() != inside.sum():
                self._break("outside", "%d bytes written outside the rows" % (count.sum() - inside.sum()))
        else:
            self._break("outside", "the rows leave the output image")

        def per_link(mask, of=Lc):
            return np.bincount(of[mask], minlength=S) > 0
        k1, k10 = vec & (k0 == 1), vec & (k0 + 10 == ntx)
        shv = np.zeros(Lc.size, np.int64)
        shv[vec] = sh
        tr.update(head=head, tail=ntx - tail0, nchunk=nchunk, nvec=np.bincount(Lc[vec], minlength=S), ngather=np.bincount(Lc[g], minlength=S),
                  shifts=per_link(vec & (shv == 0)) * 1 + per_link(vec & (shv == 16)) * 2, k0_1=per_link(k1), k0_10=per_link(k10),
                  first_dword_at_row_start=per_link(k1 & (shv == 16)), last_dword_at_row_end=per_link(k10 & (shv == 0)),
                  chunk_hist=per_link(g & (k0 < 1) & reached_hist), chunk_erasure=per_link(g & (k0 < 1) & reached_erasure),
                  chunk_end=per_link(g & (k0 + 10 > ntx)), hist=flags["hist"], erasure=flags["erasure"], row_reads=flags["row_reads"])
        self.traces.append(tr)
        self.have = min(self.have + ntx, H)
        return info
