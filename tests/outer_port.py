"""outer_push of qpsk_amd/csrc/outer.hip restated in scalar Python -- the KERNEL, not the header: one stream at a time, its 8-int header and
its ring as the state, a window in an LDS slice of outer_slice_bytes, the push appended at the bit phase total & 7 in pieces of OUTER_CHUNK
bytes, the HUNT / LOCKED machine over the window, the move-down and the write-back.  What 64 lanes do at once is a loop over the lanes (the
append and the move-down, which are plain copies, are array operations); every wave-uniform variable keeps the kernel's name.

test_outer_port_cpu.py holds the port equal to the numpy restatements of the header (test_outer_cpu.outer_ref, test_dvb_cpu.outer_group_ref)
on every input the GPU tests push, so that the port stands for the kernel, and then uses it for what cannot be done on a device:

  capacity  the port records the highest byte of the window and of the ring it touches.  On the device a window that leaves its slice
            corrupts the neighbouring wave's stream without a sound, and a ring that leaves its state_stride the next stream's header.
  faults    fault= switches on exactly ONE of FAULTS, a single wrong token each, of the kind a later change to the hunt or the window
            would make.  The GPU tests' inputs are adequate when every fault changes an output on them.  Nothing faulty exists outside
            this file: no kernel is ever built with one.

A fresh launch finds its LDS holding whatever the last workgroup left there: the port fills the window with random bytes before every push,
so an output that depended on a byte behind the window would differ from the reference."""
import numpy as np

OUTER_CHUNK, OUTER_HDR = 1024, 32
POLARITY, MSB_FIRST = 1, 2

FAULTS = (
    "hunt counts one candidate too few",            # nv = avail - span - p
    "hunt counts one candidate too many",           # nv = avail - span - p + 2
    "fx < G dropped from the legal-mask test",
    "fy < G dropped from the legal-mask test",
    "p0 loses its bits from 2 G on",
    "the gather's back[k] wrong for I > 16",
    "lmask one bit short",
    "ring sized by I alone",
    "a word needs one bit more",                    # p + wordbits >= avail
    "kz ignores I",
    "run > drop",
    "move-down keeps I - 2 words",
    "drop resumes at p",
    "ring sized by L alone",
    "ring one word short",
)
# "gk kept after a drop" is not listed: the relock overwrites gk before anything reads it, so no output can show it
RING_FAULTS = ("ring sized by I alone", "ring sized by L alone", "ring one word short")

_BREV = np.array([int("{:08b}".format(v)[::-1], 2) for v in range(256)], np.uint8).tolist()


def outer_ring_bytes(n, branches, lock):
    return (max(branches, lock) * n + 8 + 15) & ~15


def outer_slice_bytes(n, branches, lock):
    return outer_ring_bytes(n, branches, lock) + OUTER_CHUNK + 16


def kept_bound(n, branches, lock):
    """the header comment of outer.hip: what stays behind a push is at most max(I, L) n + 2 bytes"""
    return max(branches, lock) * n + 2


def _cmod(a, b):
    """C's a % b for b > 0: the sign of a"""
    return a % b if a >= 0 else -((-a) % b)


def _ffs(x):
    """__ffs: the place of the lowest set bit counted from 1, 0 for 0"""
    return (x & -x).bit_length()


class _State:
    """one stream's state_stride bytes: the header { locked, p, s, c, run, kbits, gk, 0 } and the ring"""

    def __init__(self, ring_bytes):
        self.hdr = [0] * 8
        self.ring = np.zeros(ring_bytes, np.uint8)


class outer_port:
    """S streams pushed together, as outer_ref / outer_group_ref: push(bits (S, nbits) of 0 / 1, max_words) -> dict(count, words, pos, flags,
    info), the per-word outputs cut to max_words as the device's.  After any push: hi_window / hi_ring = the highest byte index touched in
    a slice / a ring so far, kept = the most bytes a push left in a ring, and slice_bytes / ring_bytes what the (possibly faulty) sizing
    gives them."""

    def __init__(self, nstreams, n, branches=1, sync=0x47, lock=2, drop=3, flags=POLARITY, group=0, fault=None, seed=0):
        assert fault is None or fault in FAULTS, fault
        assert nstreams >= 1 and 2 <= n <= 255 and 1 <= branches <= 32 and n % branches == 0 and 0 <= sync <= 255
        assert 1 <= lock <= 16 and 0 <= drop <= 16 and not flags & ~(POLARITY | MSB_FIRST) and (group == 0 or 3 <= group <= min(lock, 16))
        self.S, self.n, self.I, self.sync, self.L, self.drop, self.flags, self.G, self.fault = nstreams, n, branches, sync, lock, drop, flags, group, fault
        if fault == "ring sized by I alone":
            self.ring_bytes = outer_ring_bytes(n, branches, 1)
        elif fault == "ring sized by L alone":
            self.ring_bytes = outer_ring_bytes(n, 1, lock)
        elif fault == "ring one word short":
            self.ring_bytes = outer_ring_bytes(n, max(branches, lock) - 1, 1)
        else:
            self.ring_bytes = outer_ring_bytes(n, branches, lock)
        self.slice_bytes = self.ring_bytes + OUTER_CHUNK + 16
        self.states = [_State(self.ring_bytes) for _ in range(nstreams)]      # outer_init_kernel: the header zeroed
        self.total = 0
        self.hi_window = self.hi_ring = -1
        self.kept = 0
        self.rng = np.random.default_rng(seed)
        # room behind the slice, so that an overrun is recorded instead of raised
        self.room = outer_slice_bytes(n, branches, lock) + 2 * OUTER_CHUNK

    def max_words(self, nbits):
        return self.L + -(-nbits // (8 * self.n))

    def advance(self, delta):
        assert delta >= 0 and delta % 8 == 0
        self.total += delta

    def push(self, bits, max_words=None):
        bits = np.asarray(bits, np.uint8)
        assert bits.ndim == 2 and bits.shape[0] == self.S and bits.shape[1] >= 1
        nbits = bits.shape[1]
        mw = self.max_words(nbits) if max_words is None else max_words
        # the caller's packed rows: bit j of a row in bit j & 7 of byte j >> 3, ones behind the last bit (the kernel must mask them)
        rows = np.packbits(np.concatenate([bits, np.ones((self.S, -nbits % 8), np.uint8)], axis=1), axis=1, bitorder="little")
        out = dict(count=np.zeros(self.S, np.int32), words=[], pos=[], flags=[], info=np.zeros((self.S, 4), np.int32))
        for i, st in enumerate(self.states):
            count, words, pos, flags, info = self._stream(st, rows[i], nbits, mw)
            out["count"][i] = count
            out["words"].append(np.array(words, np.uint8).reshape(len(words), self.n))
            out["pos"].append(np.array(pos, np.int64))
            out["flags"].append(np.array(flags, np.uint8))
            out["info"][i] = info
        self.total += nbits
        return out

    # ------------------------------------------------------------------ outer_push<MSB, GROUP> for one stream
    def _stream(self, st, row, nbits, max_words):
        fault = self.fault
        n, I, L = self.n, self.I, self.L
        wordbits = 8 * n
        span = wordbits * (L - 1) + 8
        sync, comp = self.sync, self.sync ^ 255
        polarity = bool(self.flags & POLARITY)
        msb = bool(self.flags & MSB_FIRST)
        GROUP = self.G != 0
        G = self.G if GROUP else 1
        both = GROUP or polarity
        lmask = (1 << (L - 1 if fault == "lmask one bit short" else L)) - 1
        p0 = 0
        if GROUP:
            for i in range(0, min(L, 2 * G) if fault == "p0 loses its bits from 2 G on" else L, G):
                p0 |= 1 << i
        locked, p, s, c, run, avail, gk = st.hdr[:7]
        if not GROUP:
            gk = 0
        wbuf = bytearray(self.rng.integers(0, 256, self.room, dtype=np.uint8).tobytes())      # the LDS as a launch finds it
        w = wbuf
        wv = np.frombuffer(wbuf, np.uint8)                    # the same bytes, for the copies
        hi = -1                                               # the highest window byte touched

        def vbyte(u):
            b = u >> 3
            v = (((w[b + 1] << 8) | w[b]) >> (u & 7)) & 255
            return _BREV[v] if msb else v

        def match(u):
            v = vbyte(u)
            return 1 if v == sync else -1 if both and v == comp else 0

        # the ring into the window, whole dwords
        nd = (avail + 31) >> 5
        if nd:
            self.hi_ring = max(self.hi_ring, 4 * nd - 1)
            have = min(4 * nd, self.ring_bytes)
            wv[:have] = st.ring[:have]
            wv[have:4 * nd] = 0                               # (a faulty sizing: what lies behind the ring is not the stream's)
            hi = max(hi, 4 * nd - 1)
        pos0 = self.total - avail
        ph = self.total & 7
        nin = (nbits + 7) >> 3
        lastmask = (1 << (nbits & 7)) - 1 if nbits & 7 else 255
        count = nlock = nlost = 0
        words, pos, flags = [], [], []
        if fault == "the gather's back[k] wrong for I > 16":
            back = [I - 1 - (q % I) % 16 for q in range(n)]
        else:
            back = [I - 1 - q % I for q in range(n)]

        for g0 in range(0, nin, OUTER_CHUNK):
            # ---- append input bytes [g0, g1) at bit `avail`
            g1 = min(g0 + OUTER_CHUNK, nin)
            kb, nout = avail >> 3, g1 - g0 + (1 if ph else 0)
            carry = w[kb] & ((1 << ph) - 1)
            cur = np.zeros(nout, np.uint16)
            cur[:g1 - g0] = row[g0:g1]
            if g1 == nin:
                cur[nin - 1 - g0] &= lastmask
            low = np.empty(nout, np.uint16)
            low[0] = carry
            low[1:] = cur[:-1] >> (8 - ph)
            wv[kb:kb + nout] = ((cur << ph) | low) & 255
            hi = max(hi, kb + nout - 1)
            avail += nbits - 8 * g0 if g1 == nin else 8 * (g1 - g0)
            # ---- the state machine, as far as the window allows
            while True:
                if not locked:
                    nv = avail - span - p + 1
                    if fault == "hunt counts one candidate too few":
                        nv -= 1
                    elif fault == "hunt counts one candidate too many":
                        nv += 1
                    nv = min(nv, 64)
                    if nv <= 0:
                        break
                    first = -1
                    for lane in range(nv):
                        u = p + lane
                        b = (u >> 3) + 1
                        if b > hi:
                            hi = b
                        m = match(u)
                        if not m:
                            continue
                        hit, x = True, 1 if m < 0 else 0
                        b = ((u + (L - 1) * wordbits) >> 3) + 1      # the last byte the look-ahead reads, unless it stops sooner
                        for i in range(1, L):
                            mi = match(u + i * wordbits)
                            if GROUP:
                                hit = mi != 0
                                x |= (1 if mi < 0 else 0) << i
                            else:
                                hit = mi == m
                            if not hit:
                                b = ((u + i * wordbits) >> 3) + 1
                                break
                        if b > hi:
                            hi = b
                        sg = 0
                        if GROUP and hit:
                            y = ~x & lmask
                            fx, fy = _ffs(x) - 1, _ffs(y) - 1
                            if x and (fx < G or fault == "fx < G dropped from the legal-mask test") and x == ((p0 << fx) & lmask):
                                sg = _cmod(G - fx, G)
                            elif polarity and y and (fy < G or fault == "fy < G dropped from the legal-mask test") and y == ((p0 << fy) & lmask):
                                sg = 16 | _cmod(G - fy, G)
                            else:
                                hit = False
                        if hit and first < 0:
                            first, first_sg, first_m = lane, sg, m
                    if first >= 0:
                        if GROUP:
                            s = -1 if first_sg & 16 else 1
                            gk = first_sg & 15
                        else:
                            s = 1 if first_m > 0 else -1
                        p += first
                        locked = 1
                        c = run = 0
                        nlock += 1
                    else:
                        p += nv
                        if nv < 64:
                            break
                else:
                    if p + wordbits > avail or (fault == "a word needs one bit more" and p + wordbits >= avail):
                        break
                    inv = 255 if s < 0 else 0
                    hi = max(hi, (p >> 3) + 1)
                    miss = (vbyte(p) ^ inv) != (comp if GROUP and gk == 0 else sync)
                    run = run + 1 if miss else 0
                    if self.drop > 0 and (run > self.drop if fault == "run > drop" else run == self.drop):
                        locked = 0
                        if fault != "drop resumes at p":
                            p += 1
                        nlost += 1
                        if GROUP:
                            gk = 0
                        continue
                    if c >= I - 1:
                        if count < max_words:
                            first = p - wordbits * (I - 1)
                            words.append([vbyte(p - wordbits * back[q] + 8 * q) ^ inv for q in range(n)])
                            hi = max(hi, ((p + 8 * (n - 1)) >> 3) + 1)
                            pos.append(pos0 + p)
                            if GROUP:
                                kz = gk if fault == "kz ignores I" else _cmod(gk - (I - 1) % G + G, G)
                                ez = comp if kz == 0 else sync
                                flags.append(((1 if (vbyte(first) ^ inv) != ez else 0) | (2 if s < 0 else 0) | kz << 4) & 255)
                            else:
                                flags.append((1 if (vbyte(first) ^ inv) != sync else 0) | (2 if s < 0 else 0))
                        count += 1
                    c = min(c + 1, I - 1)
                    if GROUP:
                        gk = 0 if gk + 1 == G else gk + 1
                    p += wordbits
            # ---- move the window down to the first byte still needed
            keep = max(c - 1, 0) if fault == "move-down keeps I - 2 words" else c
            off = (p - wordbits * keep if locked else p) >> 3
            if off > 0:
                nb = ((avail + 7) >> 3) - off
                if nb > 0:
                    wv[:nb] = wv[off:off + nb].copy()
                p -= 8 * off
                avail -= 8 * off
                pos0 += 8 * off
        # ---- what is left goes back into the ring
        nb = (avail + 7) >> 3
        nd = (nb + 3) >> 2
        wv[nb:4 * nd] = 0
        if nd:
            hi = max(hi, 4 * nd - 1)
            self.hi_ring = max(self.hi_ring, 4 * nd - 1)
            have = min(4 * nd, self.ring_bytes)
            st.ring[:have] = wv[:have]                        # (a faulty sizing: the rest lands in the next stream's state and is lost to this one)
        self.kept = max(self.kept, nb)
        self.hi_window = max(self.hi_window, hi)
        st.hdr[:6] = [locked, p, s, c, run, avail]
        if GROUP:
            st.hdr[6] = gk
        return count, words, pos, flags, (locked, s if locked else 0, nlock, nlost)


def agree(got, want, max_words=None):
    """a port's call against a reference's, as test_outer_gpu.same compares a device's: the true count, the first min(count, max_words)
    entries of words, pos and flags, and info -> None, or what differs first"""
    if not np.array_equal(got["count"], want["count"]):
        return "count"
    for i in range(len(want["count"])):
        k = int(want["count"][i]) if max_words is None else min(int(want["count"][i]), max_words)
        for key in ("words", "pos", "flags"):
            if not np.array_equal(got[key][i], want[key][i][:k]):
                return "%s of stream %d" % (key, i)
    return None if np.array_equal(got["info"], want["info"]) else "info"


def capacity(port):
    """None where the port stayed inside what the kernel gives it, or what it left"""
    if port.hi_window >= port.slice_bytes:
        return "window byte %d touched in a slice of %d" % (port.hi_window, port.slice_bytes)
    if port.hi_ring >= port.ring_bytes:
        return "ring byte %d touched in a ring of %d" % (port.hi_ring, port.ring_bytes)
    if port.kept > kept_bound(port.n, port.I, port.L):
        return "%d bytes kept, the bound is %d" % (port.kept, kept_bound(port.n, port.I, port.L))
    return None
