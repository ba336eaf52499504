"""viterbi_stream_kernel, viterbi_stream_punct_kernel, viterbi_stream_flush_kernel and viterbi_stream_init_kernel of
qpsk_amd/csrc/viterbi_stream.hip, with the host's part of qpsk_viterbi_stream_* (api_vstream.cpp: total, advanced, what a call emits, the five
numbers of a launch, vstream_args_fit's refusals) and the loaders of viterbi_row.h as a push uses them, restated in numpy -- the KERNELS, not
the header: the chain on int32 with chain_make's signs and sources, the normalisation once per block, the ring of decision and ballot words
at the kernel's byte offsets, the pending pairs, decide<false> and decide<true> a block at a time, ballot_errors with its lo / hi / x, the
load a block ahead.  The definition stays test_viterbi_stream_cpu.viterbi_stream_ref.

The port works on BYTE IMAGES AT SIMULATED ADDRESSES (nodesync_port.Image): d_soft, d_bits and d_info are addresses inside one, so base
offsets and pitches are parameters, and the state is one byte image of state_stride bytes per stream with the kernel's layout (pm[64] int32
at 0, the pending pairs at 256, `last` at 384, nring blocks of 64 decision words at 512, nring x 4 ballot words behind them).  All streams
run the same launch, so the streams are an array axis; the 64 lanes are another; the chain's steps and the blocks are loops, the trace-back
is a scalar walk per stream.  What a device cannot show is on record:

  soft_reads    every read of the input image as (streams, addresses, bytes each); each has to lie in its stream's row
                [soft + 2 s pitch, + 2 ntx).  The load a block ahead runs past the push by design and must be masked.
  state_writes  per state byte the lane that last wrote it (-1: nothing since the reset), state_reads per byte a bit mask of the lanes that
                read it.  A read has to be of a byte written since the reset (pm and `last` by the init kernel, everything else by a push or
                a flush of this stream life: a flush leaves the stream as after a reset, so it ends the life of the pairs and the ring too)
                and by the lane that wrote it; nothing outside state_stride is touched; a ring slot stays below nring; a push writes the
                pending pairs of lanes below rem and no other.
  writes        per call how often each byte of the bits image and of the d_info image was written: exactly once inside
                [0, ceil(nbits / 8)) of a stream's bits row and inside its four info words, never elsewhere.
  traces        per call a dict: kind, pc before and behind it, the launch's numbers, the blocks run, whether the flush ran a partial
                block, and per decision ntrace, nskip, nemit, per stream how many states tied for the best metric (`tied`) and how many
                steps of the walked path were ties of m0 and m1 (`step_ties`).
  broken        what left a bound, by kind (KINDS), the first of each kind as text.

With seed= the whole state image starts as random bytes before the init kernel runs, and the bytes whose life a flush ends are random
again behind it.  fault= switches on exactly ONE of FAULTS, a single wrong token each, or one of EQUIVALENT, which no input can show."""
import numpy as np

from nodesync_port import Image, w32      # Image: the byte images of this port's callers are nodesync_port's

VS_PEND, VS_LAST, VS_RING = 256, 384, 512
NEG = -(1 << 30)
MAX_STEPS, MAX_SPAN, TERMINATED = 131072, 8192, 1

FAULTS = (
    # chain and loaders
    "a tie takes p1",
    "best_state ties to the highest state",
    "the pending s0 read without the int8 sign",
    "the pending s1 read without the int8 sign",
    "the pending pairs stored before the -128 rule",
    "pending read at t <= 0",
    "pending written for lane <= rem",                       # a dead pair: only the record of the pairs a push writes shows it
    "the load ahead not masked at a.n",                      # reads behind the row; what it fetches never reaches a step
    "the pattern's phase taken from the stream's position",
    "no -128 rule in PunctLoader::value",
    "no -128 rule in load_soft",
    "sg0 from the generator of sg1",
    "from1 without its | 128",
    # ring
    "the slot's wrap at slot + 1 > nring",
    "have not clamped at nring",
    "the ballots stored by lanes 1..4",                      # the same words at the same places, read back by other lanes
    "neg1 and nz1 swapped",
    "the ballot base at nring * 544",
    # decide
    "nskip = dblk - 1",
    "nskip = dblk + 1",
    "the count taken for i >= nskip",
    "later_bal taken before the count",
    "the oldest block counted against 0",
    "last = later",
    "last not stored behind a push",
    "the byte store for lane < (n >> 3)",
    "ob without e.outblk",
    "e.outblk not advanced",
    "the walk's wrap to nring",
    "ballot_errors with the masks swapped",
    # flush
    "n_newest = a.pc without the 64 of pc == 0",
    "pending read for lane <= a.pc",
    "TERMINATED ignored",
    "info[2] taken before the TERMINATED override",
    "pm not reset",
    "last not cleared",
    "no partial block stored into the ring",
    # host
    "slot without - advanced",
    "the flush's slot = blocks % nring",
    "the flush's have without the + 63",
    "wphase = total / 64 % nring",
    "pc = total % 32",
)
# Not in the list, because no input can show them; the port still takes each as fault=, and test_vstream_port_cpu.py checks on every set
# that no bit, info word or state changes:
EQUIVALENT = {
    "no normalisation": "every output and info word depends on metric differences only: the decisions compare two metrics, best_state takes "
                        "the place of the largest, spread is a difference, and the state is compared after its own maximum is taken off.  "
                        "A metric grows by at most 254 a step, so int32 holds for fewer than 2^31 / 254 = 8.4 million steps since a reset, "
                        "which no set reaches (the longest has 131072); that bound is asserted by the port",
    "vstream_emitted without the total < window case": "for total < window, total / window * window is 0 and max(0, 0 - depth) is the 0 "
                                                       "the case returns: the case is a shortcut, not a rule",
    "the slot's wrap as (slot + 1) % nring": "0 <= slot < nring always (vstream_args_fit), so the select is the remainder",
    "the normalisation by min(pm)": "as above: the differences stay, and the metrics stay within max - min <= 2^30 + 254 x 64 of 0",
    "the push's have from total - advanced": "an advance needs total >= depth + window before it and moves total and advanced alike, so "
                                             "total - advanced >= depth + window behind it and both quotients are clamped to nring",
}
KINDS = ("refused", "soft_reads", "state outside", "state unwritten", "state lane", "slot", "pend", "outside", "twice", "unwritten")
DEVICE_SEES = ("bits", "nbits", "info", "refused", "outside", "unwritten")      # outputs, d_info, the return code, the poison and guards

LANE = np.arange(64)
U64 = np.uint64
_W64 = U64(1) << np.arange(64, dtype=U64)
_PAR = np.array([bin(v).count("1") & 1 for v in range(128)], np.int64)


def popc(v):
    return bin(int(v)).count("1")


def _pack(b):
    """(..., 64) bool, lane l's vote -> (...) uint64: __ballot"""
    return (b.astype(U64) * _W64).sum(axis=-1, dtype=U64)


class Refused(Exception):
    """the host's refusal of a call (QPSK_ERR_ARG / QPSK_ERR_STATE): nothing was launched"""


class vstream_port:
    """reset() / emits() / push() / flush() / advance() as qpsk_viterbi_stream_reset / _emits / _push / _flush and
    qpsk_test_viterbi_stream_advance.  push and flush write into Images and return nbits; .state is (S, state_stride) uint8."""

    def __init__(self, fault=None, seed=None):
        assert fault is None or fault in FAULTS or fault in EQUIVALENT, fault
        self.fault = fault
        self.rng = None if seed is None else np.random.default_rng(seed)
        self.state = None
        self.soft_reads, self.writes, self.traces = [], [], []
        self.broken = {}

    def _junk(self, shape):
        return np.zeros(shape, np.uint8) if self.rng is None else self.rng.integers(0, 256, shape).astype(np.uint8)

    def _break(self, kind, text):
        assert kind in KINDS
        self.broken.setdefault(kind, "call %d: %s" % (len(self.traces), text))

    # ------------------------------------------------------------------ the host: api_vstream.cpp
    def reset(self, S, depth, window, pattern=(1, 1, 1)):
        period, keep0, keep1 = pattern
        K = popc(keep0) + popc(keep1)
        if not (1 <= period <= 32 and K >= 1 and keep0 >> period == 0 and keep1 >> period == 0):
            raise Refused("pattern")
        if S < 1 or depth < 64 or window < 64 or depth % 64 or window % 64 or depth + window > MAX_SPAN:
            raise Refused("nstreams, depth or window")
        self.S, self.D, self.W = S, depth, window
        self.period, self.keep0, self.keep1, self.K = period, keep0, keep1, K
        self.punctured = tuple(pattern) != (1, 1, 1)
        self.nring, self.dblk, self.wblk = (depth + window) // 64, depth // 64, window // 64
        self.stride = VS_RING + self.nring * (512 + 32)      # vstream_state_stride
        self.state = self._junk((S, self.stride))            # a fresh allocation holds anything
        self.state_writes = np.full(self.stride, -1, np.int16)
        self.state_reads = np.zeros(self.stride, U64)
        self.ties = {}                                       # beside the ring, not of it: per slot the ties of m0 and m1, as decision words
        self.total = self.advanced = 0
        low = [(1 << r) - 1 for r in range(period)]
        self._b0 = np.array([(keep0 >> r) & 1 for r in range(period)], np.int64)
        self._b1 = np.array([(keep1 >> r) & 1 for r in range(period)], np.int64)
        self._pre = np.array([popc(keep0 & m) + popc(keep1 & m) for m in low], np.int64)
        self._touched = np.zeros(self.stride, np.int32)
        self._init_kernel()

    def _emitted(self, total):
        if self.fault == "vstream_emitted without the total < window case":
            return max(0, total // self.W * self.W - self.D)
        return 0 if total < self.W else max(0, total // self.W * self.W - self.D)

    def _steps(self, ntx):
        if ntx < 1 or (2 * ntx) % self.K:
            return 0
        n = 2 * ntx // self.K * self.period
        return n if 1 <= n <= MAX_STEPS else 0

    def emits(self, ntx):
        n = self._steps(ntx)
        if self.state is None or not n:
            raise Refused("emits")
        return self._emitted(self.total + n) - self._emitted(self.total)

    def push_numbers(self):
        """pc, slot, have, wphase of a push now, as qpsk_viterbi_stream_push computes them"""
        f, total, adv, nring = self.fault, self.total, self.advanced, self.nring
        return dict(pc=total % (32 if f == "pc = total % 32" else 64),
                    slot=(total if f == "slot without - advanced" else total - adv) // 64 % nring,
                    have=min((total - adv if f == "the push's have from total - advanced" else total) // 64, nring),
                    wphase=total // 64 % (nring if f == "wphase = total / 64 % nring" else self.wblk))

    def flush_numbers(self):
        """pc, slot, have and nbits of a flush now, as qpsk_viterbi_stream_flush computes them"""
        f, total, adv, nring = self.fault, self.total, self.advanced, self.nring
        first = self._emitted(total)
        blocks = ((total if f == "slot without - advanced" else total - adv) + 63) // 64
        if f == "the flush's slot = blocks % nring":
            slot = blocks % nring if blocks else 0
        else:
            slot = (blocks - 1) % nring if blocks else 0
        have = (total if f == "the flush's have without the + 63" else total + 63) // 64 - first // 64
        return dict(pc=total % (32 if f == "pc = total % 32" else 64), slot=slot, have=have, nbits=total - first)

    def _args_fit(self, a, outputs):
        return (self.nring >= 2 and self.nring <= MAX_SPAN // 64 and self.dblk >= 1 and self.wblk >= 1 and self.dblk + self.wblk == self.nring and
                0 <= a["slot"] < self.nring and 0 <= a["have"] <= self.nring and 0 <= a["pc"] < 64 and outputs)

    def _outputs(self, nbits, bits, info):
        """vstream_outputs -> the bits pitch in force"""
        if bits is None and info is None:
            raise Refused("every output is NULL")
        if info is not None and info[1] % 4:
            raise Refused("d_info is not 4-byte aligned")
        need = (nbits + 7) // 8
        if bits is None:
            return 0
        pitch = bits[2] or need
        if pitch < need:
            raise Refused("bits_pitch")
        return pitch

    def advance(self, delta):
        if self.state is None or delta < 0 or delta > 1 << 62 or delta % self.W or self.total < self.D + self.W:
            raise Refused("advance")
        self.total += delta
        self.advanced += delta

    # ------------------------------------------------------------------ memory, on record
    def _sld(self, off, size, lanes):
        """lane lanes[i] loads `size` bytes at state offset off[i] of every stream -> (S, len) uint64"""
        off, lanes = np.asarray(off, np.int64), np.asarray(lanes, np.int64)
        idx = off[:, None] + np.arange(size)
        ok = (idx >= 0) & (idx < self.stride)
        if not ok.all():
            self._break("state outside", "lane %d reads at %d of %d" % (lanes[~ok.all(1)][0], off[~ok.all(1)][0], self.stride))
        ci = np.clip(idx, 0, self.stride - 1)
        wr = self.state_writes[ci]
        who = lanes[:, None]
        if (ok & (wr == -1)).any():
            i = np.argwhere(ok & (wr == -1))[0]
            self._break("state unwritten", "lane %d reads byte %d, not written since the reset" % (lanes[i[0]], ci[i[0], i[1]]))
        if (ok & (wr >= 0) & (wr != who)).any():
            i = np.argwhere(ok & (wr >= 0) & (wr != who))[0]
            self._break("state lane", "lane %d reads byte %d, written by lane %d" % (lanes[i[0]], ci[i[0], i[1]], wr[i[0], i[1]]))
        np.bitwise_or.at(self.state_reads, ci[ok], (U64(1) << np.broadcast_to(who, idx.shape)[ok].astype(U64)))
        b = np.where(ok[None], self.state[:, ci], np.uint8(0xAA)).astype(U64)
        return sum(b[:, :, k] << U64(8 * k) for k in range(size))

    def _sst(self, off, size, lanes, vals):
        """lane lanes[i] stores vals[:, i] as `size` bytes at state offset off[i] of every stream"""
        off, lanes = np.asarray(off, np.int64), np.asarray(lanes, np.int64)
        vals = np.asarray(vals).astype(U64)
        idx = off[:, None] + np.arange(size)
        ok = (idx >= 0) & (idx < self.stride)
        if not ok.all():
            self._break("state outside", "lane %d writes at %d of %d" % (lanes[~ok.all(1)][0], off[~ok.all(1)][0], self.stride))
        b = np.stack([(vals >> U64(8 * k)) & U64(255) for k in range(size)], axis=-1).astype(np.uint8)
        self.state[:, idx[ok]] = b[:, ok]
        self.state_writes[idx[ok]] = np.broadcast_to(lanes[:, None], idx.shape)[ok]
        np.add.at(self._touched, idx[ok], 1)

    def _dec_off(self, slot):
        if not 0 <= slot < self.nring:
            self._break("slot", "ring slot %d of %d" % (slot, self.nring))
        return VS_RING + (slot << 9) + 8 * LANE

    def _bal_off(self, slot):
        base = VS_RING + self.nring * (544 if self.fault == "the ballot base at nring * 544" else 512)
        return base + (slot << 5) + 8 * LANE[:4]

    def _read(self, src, d_soft, pitch, ntx, streams, at, n):
        """n bytes at byte `at` of each stream's row -> (len, n) uint8; a read outside the row is recorded and, outside the image, 0xAA"""
        addr = d_soft + 2 * streams * pitch + at
        self.soft_reads.append((streams, addr, n))
        out = (at < 0) | (at + n > 2 * ntx)
        if out.any():
            i = int(np.flatnonzero(out)[0])
            self._break("soft_reads", "stream %d reads %d bytes at row %+d, the row has %d" % (streams[i], n, at[i], 2 * ntx))
        idx = (addr - src.addr)[:, None] + np.arange(n)
        ok = (idx >= 0) & (idx < src.b.size)
        return np.where(ok, src.b[np.clip(idx, 0, src.b.size - 1)], np.uint8(0xAA))

    def _ostore(self, out, count, addr, vals):
        """one byte each to an output image (out = (Image, ...)), every byte counted"""
        idx = addr - out[0].addr
        ok = (idx >= 0) & (idx < out[0].b.size)
        if not ok.all():
            self._break("outside", "a store outside the output image")
        np.add.at(count, idx[ok], 1)
        out[0].b[idx[ok]] = vals[ok]

    def _check_writes(self, what, out, count, row_addr, nbytes):
        rows = (row_addr - out[0].addr)[:, None] + np.arange(nbytes)[None, :]
        if rows.size and (rows.min() < 0 or rows.max() >= count.size):
            self._break("outside", "%s: the rows leave the image" % what)
            return
        inside = count[rows]
        if (inside > 1).any():
            self._break("twice", "%s: stream %d byte %d written %d times" % ((what,) + tuple(np.argwhere(inside > 1)[0]) + (inside.max(),)))
        if (inside == 0).any():
            self._break("unwritten", "%s: stream %d byte %d not written" % ((what,) + tuple(np.argwhere(inside == 0)[0])))
        if count.sum() != inside.sum():
            self._break("outside", "%s: %d bytes written outside the rows" % (what, count.sum() - inside.sum()))

    # ------------------------------------------------------------------ the chain
    def _chain(self):
        """chain_make: sg0, sg1 and the lanes from0 / from1 stand for (byte addresses / 4)"""
        g0 = 0x5B if self.fault == "sg0 from the generator of sg1" else 0x79
        sg0 = np.array([-1 if popc(l & g0) & 1 else 1 for l in range(64)], np.int32)
        sg1 = np.array([-1 if popc(l & 0x5B) & 1 else 1 for l in range(64)], np.int32)
        from0 = (LANE >> 1) << 2
        from1 = from0 if self.fault == "from1 without its | 128" else from0 | 128
        return sg0, sg1, from0 >> 2, from1 >> 2

    def _forward(self, s0v, s1v, n, pm):
        """forward_block (n = 64) / forward_partial: -> (the lanes' decision words (S, 64) uint64, the ties as such words, pm)"""
        sg0, sg1, p0, p1 = self._chain()
        b = sg0[None, None, :] * s0v[:, :n, None] + sg1[None, None, :] * s1v[:, :n, None]      # __mul24 is exact below 2^23
        keep = self.fault == "a tie takes p1"
        dec = np.zeros((n, self.S, 64), bool)
        tie = np.zeros((n, self.S, 64), bool)
        for t in range(n):
            m0 = pm[:, p0] + b[:, t]
            m1 = pm[:, p1] - b[:, t]
            tie[t] = m1 == m0
            dec[t] = m1 >= m0 if keep else m1 > m0
            pm = np.maximum(m0, m1)
        wt = _W64[:n, None, None]
        assert np.abs(pm.astype(np.int64)).max() < (1 << 31) - 255, "int32 is about to wrap"
        return (dec.astype(U64) * wt).sum(axis=0, dtype=U64), (tie.astype(U64) * wt).sum(axis=0, dtype=U64), pm

    def _normalise(self, pm):
        if self.fault == "no normalisation":
            return pm
        return pm - (pm.min(axis=1, keepdims=True) if self.fault == "the normalisation by min(pm)" else pm.max(axis=1, keepdims=True))

    def _ring_store(self, slot, w, tiew, s0v, s1v):
        self._sst(self._dec_off(slot), 8, LANE, w)
        self.ties[slot] = tiew
        neg0, nz0, neg1, nz1 = _pack(s0v < 0), _pack(s0v != 0), _pack(s1v < 0), _pack(s1v != 0)
        words = np.stack([neg0, nz0, nz1, neg1] if self.fault == "neg1 and nz1 swapped" else [neg0, nz0, neg1, nz1], axis=1)
        self._sst(self._bal_off(slot), 8, LANE[:4] + (1 if self.fault == "the ballots stored by lanes 1..4" else 0), words)

    def _best_state(self, pm):
        mx = pm.max(axis=1, keepdims=True)
        spread = (mx[:, 0].astype(np.int64) - pm.min(axis=1)).astype(np.int32)
        at = pm == mx
        st = 63 - np.argmax(at[:, ::-1], axis=1) if self.fault == "best_state ties to the highest state" else np.argmax(at, axis=1)
        return st.astype(np.int64), spread, at.sum(axis=1)

    def _ballot_errors(self, b, cur, prev, e):
        """b (S, 4) uint64 out of lanes 0..3; cur / prev (S,) uint64"""
        cur, prev = np.asarray(cur, U64)[:, None], np.asarray(prev, U64)[:, None]
        lo, hi = (cur << U64(6)) | (prev >> U64(58)), cur >> U64(58)
        lane = LANE.astype(U64)[None, :]
        x = (((lo >> lane) | ((hi << U64(1)) << (U64(63) - lane))) & U64(127)).astype(np.int64)
        ma, mb = (0x6D, 0x4F) if self.fault == "ballot_errors with the masks swapped" else (0x4F, 0x6D)
        c0, c1 = _pack(_PAR[x & ma] != 0), _pack(_PAR[x & mb] != 0)
        neg0, nz0, neg1, nz1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        for s in range(self.S):
            e["errs"][s] = w32(e["errs"][s] + popc(nz0[s] & (neg0[s] ^ c0[s])) + popc(nz1[s] & (neg1[s] ^ c1[s])))
            e["nz"][s] = w32(e["nz"][s] + popc(nz0[s]) + popc(nz1[s]))

    def _decide(self, partial, st, spread, tied, slot, ntrace, nskip, n_newest, last, e, tr):
        """decide<PARTIAL>: -> last"""
        f, S = self.fault, self.S
        e["st"], e["spread"] = st.copy(), spread
        nemit = max(ntrace - nskip, 0)
        rec = dict(ntrace=ntrace, nskip=nskip, nemit=nemit, tied=tied.tolist(), step_ties=[0] * S)
        tr["decisions"].append(rec)
        if nemit == 0:
            return last
        st = st.tolist()
        later, newest = np.zeros(S, U64), np.zeros(S, U64)
        later_bal = np.zeros((S, 4), U64)
        for i in range(ntrace):
            w = self._sld(self._dec_off(slot), 8, LANE).tolist()
            b = self._sld(self._bal_off(slot), 8, LANE[:4])
            tw = self.ties[slot].tolist() if slot in self.ties else None
            n = n_newest if partial and i == 0 else 64
            word = np.zeros(S, U64)
            for s in range(S):
                ws, x, acc, nt = w[s], st[s], 0, 0
                ts = tw[s] if tw is not None else None
                for t in range(n - 1, -1, -1):
                    d = (ws[x] >> t) & 1
                    if ts is not None:
                        nt += (ts[x] >> t) & 1
                    acc |= (x & 1) << t
                    x = (x >> 1) | (d << 5)
                st[s], word[s] = x, acc
                rec["step_ties"][s] += nt
            if i >= nskip:
                ob = (0 if f == "ob without e.outblk" else e["outblk"]) + (ntrace - 1 - i)
                if e["bits"] is not None:
                    nl = (n >> 3) if f == "the byte store for lane < (n >> 3)" else (n + 7) >> 3
                    lanes = LANE[:nl]
                    addr = e["bits"][1] + np.arange(S)[:, None] * e["pitch"] + (ob << 3) + lanes[None, :]
                    vals = ((word[:, None] >> (lanes.astype(U64) << U64(3))[None, :]) & U64(255)).astype(np.uint8)
                    self._ostore(e["bits"], e["count"], addr.reshape(-1), vals.reshape(-1))
                if f == "later_bal taken before the count":
                    later_bal = b
                if i >= nskip if f == "the count taken for i >= nskip" else i > nskip:
                    self._ballot_errors(later_bal, later, word, e)
                else:
                    newest = word
                later = word
                later_bal = b
            if f == "the walk's wrap to nring":
                slot = self.nring if slot == 0 else slot - 1
            else:
                slot = self.nring - 1 if slot == 0 else slot - 1
        self._ballot_errors(later_bal, later, np.zeros(S, U64) if f == "the oldest block counted against 0" else last, e)
        if f != "e.outblk not advanced":
            e["outblk"] += nemit
        return later if f == "last = later" else newest

    def _emit(self, bits, pitch, info):
        S = self.S
        return dict(bits=bits, pitch=pitch, info=info, outblk=0, errs=[0] * S, nz=[0] * S, st=np.full(S, -1, np.int64), spread=np.zeros(S, np.int32),
                    count=None if bits is None else np.zeros(bits[0].b.size, np.int32), icount=None if info is None else np.zeros(info[0].b.size, np.int32))

    def _emit_info(self, e, st_word=None):
        if e["info"] is None:
            return
        S = self.S
        words = np.stack([np.array(e["errs"], np.int64), np.array(e["nz"], np.int64), e["st"] if st_word is None else st_word,
                          e["spread"].astype(np.int64)], axis=1).astype(np.int32)
        addr = e["info"][1] + 16 * np.arange(S)[:, None] + np.arange(16)[None, :]
        self._ostore(e["info"], e["icount"], addr.reshape(-1), np.ascontiguousarray(words).view(np.uint8).reshape(-1))

    def _finish(self, e, nbits, tr):
        S = self.S
        if e["bits"] is not None:
            self._check_writes("bits", e["bits"], e["count"], e["bits"][1] + np.arange(S) * e["pitch"], (nbits + 7) // 8)
        if e["info"] is not None:
            self._check_writes("info", e["info"], e["icount"], e["info"][1] + 16 * np.arange(S), 16)
        self.writes.append((e["count"], e["icount"]))
        self.traces.append(tr)

    def _load_state(self):
        pm = self._sld(4 * LANE, 4, LANE).astype(np.uint32).view(np.int32)
        last = self._sld([VS_LAST], 8, [0])[:, 0]
        return pm, last

    def _pend(self, lanes, s0, s1):
        """the pending pairs of `lanes` into s0 / s1 (S, 64) int32"""
        f = self.fault
        w = self._sld(VS_PEND + 2 * lanes, 2, lanes).astype(np.int64)
        a, b = w & 255, w >> 8
        s0[:, lanes] = a if f == "the pending s0 read without the int8 sign" else (a ^ 128) - 128
        s1[:, lanes] = b if f == "the pending s1 read without the int8 sign" else (b ^ 128) - 128

    # ------------------------------------------------------------------ viterbi_stream_init_kernel
    def _init_kernel(self):
        self._sst(4 * LANE, 4, LANE, np.broadcast_to(np.where(LANE == 0, 0, NEG).astype(np.int64) & 0xFFFFFFFF, (self.S, 64)))
        self._sst([VS_LAST], 8, [0], np.zeros((self.S, 1), U64))

    # ------------------------------------------------------------------ viterbi_stream_kernel / viterbi_stream_punct_kernel
    def _load_push(self, src, d_soft, pitch, ntx, n, pc, nblk):
        """the load lambda for blocks 0..nblk at once (it depends on nothing the chain computes): -> s0, s1 after the -128 rule and raw,
        each (S, nblk + 1, 64) int32.  Lanes of block 0 below pc are left 0 for the pending pairs"""
        f, S = self.fault, self.S
        t = (np.arange(nblk + 1)[:, None] << 6) - pc + LANE[None, :]
        mask = (t > 0 if f == "pending read at t <= 0" else t >= 0) & ((t < n) | (f == "the load ahead not masked at a.n"))
        raw = np.zeros((2, S, nblk + 1, 64), np.int32)
        bi, li = np.nonzero(mask)
        tt = t[bi, li]
        streams = np.repeat(np.arange(S), tt.size)
        if not self.punctured:
            b = self._read(src, d_soft, pitch, ntx, streams, np.tile(2 * tt, S), 2).view(np.int8).astype(np.int32).reshape(S, tt.size, 2)
            raw[0][:, bi, li], raw[1][:, bi, li] = b[:, :, 0], b[:, :, 1]
            rule = f != "no -128 rule in load_soft"
        else:
            u = tt + pc if f == "the pattern's phase taken from the stream's position" else tt
            q, r = u // self.period, u % self.period
            k0 = q * self.K + self._pre[r]
            b0, b1 = self._b0[r] != 0, self._b1[r] != 0
            for j, (sent, at) in enumerate(((b0, k0), (b1, k0 + b0))):
                if sent.any():
                    v = self._read(src, d_soft, pitch, ntx, np.repeat(np.arange(S), sent.sum()), np.tile(at[sent], S), 1)
                    raw[j][:, bi[sent], li[sent]] = v.view(np.int8).astype(np.int32).reshape(S, -1)
            rule = f != "no -128 rule in PunctLoader::value"
        s = np.maximum(raw, -127) if rule else raw
        return s[0], s[1], raw[0], raw[1]

    def push(self, src, d_soft, row_pitch, ntx, bits=None, info=None):
        """bits = (Image, d_bits, bits_pitch) or None, info = (Image, d_info) or None -> nbits"""
        f, S = self.fault, self.S
        if self.state is None:
            raise Refused("no reset yet")
        n = self._steps(ntx)
        if not n:
            raise Refused("ntx")
        pitch = row_pitch or ntx
        if pitch < ntx or d_soft % 2:
            raise Refused("row_pitch or alignment")
        nbits = self.emits(ntx)
        bits_pitch = self._outputs(nbits, bits, info)
        a = self.push_numbers()
        tr = dict(kind="push", n=n, pc=a["pc"], decisions=[], partial=False, **{k: a[k] for k in ("slot", "have", "wphase")})
        e = self._emit(bits, bits_pitch, info)
        if not self._args_fit(a, True) or not 0 <= a["wphase"] < self.wblk:
            self._break("refused", "the launch refuses pc %(pc)d slot %(slot)d have %(have)d wphase %(wphase)d" % a)
            tr.update(blocks=0, pc_after=a["pc"])
            self._finish(e, nbits, tr)
            return nbits
        self._touched[:] = 0
        pc = a["pc"]
        nblk = (pc + n) >> 6
        s0, s1, r0, r1 = self._load_push(src, d_soft, pitch, ntx, n, pc, nblk)
        lanes = LANE[:pc + 1] if f == "pending read at t <= 0" else LANE[:pc]
        if lanes.size:
            self._pend(lanes, s0[:, 0], s1[:, 0])
            r0[:, 0, lanes], r1[:, 0, lanes] = s0[:, 0, lanes], s1[:, 0, lanes]
        pm, last = self._load_state()
        slot, have, wphase = a["slot"], a["have"], a["wphase"]
        for blk in range(nblk):
            pm = self._normalise(pm)
            w, tiew, pm = self._forward(s0[:, blk], s1[:, blk], 64, pm)
            self._ring_store(slot, w, tiew, s0[:, blk], s1[:, blk])
            have = have + 1 if f == "have not clamped at nring" else min(have + 1, self.nring)
            wphase += 1
            if wphase == self.wblk:
                wphase = 0
                st, spread, tied = self._best_state(pm)
                nskip = self.dblk + (-1 if f == "nskip = dblk - 1" else 1 if f == "nskip = dblk + 1" else 0)
                last = self._decide(False, st, spread, tied, slot, have, nskip, 64, last, e, tr)
            if f == "the slot's wrap as (slot + 1) % nring":
                slot = (slot + 1) % self.nring
            else:
                slot = 0 if slot + 1 == (self.nring + 1 if f == "the slot's wrap at slot + 1 > nring" else self.nring) else slot + 1
        rem = (pc + n) & 63
        lanes = LANE[:rem + 1] if f == "pending written for lane <= rem" else LANE[:rem]
        lanes = lanes[lanes < 64]
        if lanes.size:
            n0, n1 = (r0, r1) if f == "the pending pairs stored before the -128 rule" else (s0, s1)
            self._sst(VS_PEND + 2 * lanes, 2, lanes, (n0[:, nblk, lanes].astype(np.int64) & 255) | ((n1[:, nblk, lanes].astype(np.int64) & 255) << 8))
        want = np.zeros(self.stride, bool)
        want[VS_PEND:VS_PEND + 2 * rem] = True
        if not np.array_equal(self._touched[VS_PEND:VS_LAST] > 0, want[VS_PEND:VS_LAST]):
            self._break("pend", "a push that leaves %d steps wrote the pairs %s" % (rem, np.flatnonzero(self._touched[VS_PEND:VS_LAST:2]).tolist()[-3:]))
        self._sst(4 * LANE, 4, LANE, pm.astype(np.int64) & 0xFFFFFFFF)
        if f != "last not stored behind a push":
            self._sst([VS_LAST], 8, [0], last[:, None])
        self._emit_info(e)
        self.total += n
        tr.update(blocks=nblk, pc_after=rem)
        self._finish(e, nbits, tr)
        return nbits

    # ------------------------------------------------------------------ viterbi_stream_flush_kernel
    def flush(self, flags=0, bits=None, info=None):
        f, S = self.fault, self.S
        if self.state is None:
            raise Refused("no reset yet")
        if flags & ~TERMINATED:
            raise Refused("unknown flags")
        a = self.flush_numbers()
        nbits = a["nbits"]
        bits_pitch = self._outputs(nbits, bits, info)
        tr = dict(kind="flush", pc=a["pc"], slot=a["slot"], have=a["have"], decisions=[], partial=a["pc"] > 0, blocks=int(a["pc"] > 0), pc_after=0,
                  flags=flags, total=self.total)
        e = self._emit(bits, bits_pitch, info)
        if not self._args_fit(a, True):
            self._break("refused", "the launch refuses pc %(pc)d slot %(slot)d have %(have)d" % a)
            self._finish(e, nbits, tr)
            return nbits
        pc = a["pc"]
        pm, last = self._load_state()
        if pc > 0:
            s0v, s1v = np.zeros((S, 64), np.int32), np.zeros((S, 64), np.int32)
            self._pend(LANE[:pc + 1] if f == "pending read for lane <= a.pc" else LANE[:pc], s0v, s1v)
            pm = self._normalise(pm)
            w, tiew, pm = self._forward(s0v, s1v, pc, pm)
            if f != "no partial block stored into the ring":
                self._ring_store(a["slot"], w, tiew, s0v, s1v)
        st, spread, tied = self._best_state(pm)
        best = st
        if flags & TERMINATED and f != "TERMINATED ignored":
            st = np.zeros(S, np.int64)
        n_newest = pc if pc > 0 or f == "n_newest = a.pc without the 64 of pc == 0" else 64
        last = self._decide(True, st, spread, tied, a["slot"], a["have"], 0, n_newest, last, e, tr)
        if f == "pm not reset":
            self._sst(4 * LANE, 4, LANE, pm.astype(np.int64) & 0xFFFFFFFF)
        else:
            self._sst(4 * LANE, 4, LANE, np.broadcast_to(np.where(LANE == 0, 0, NEG).astype(np.int64) & 0xFFFFFFFF, (S, 64)))
        self._sst([VS_LAST], 8, [0], last[:, None] if f == "last not cleared" else np.zeros((S, 1), U64))
        self._emit_info(e, best if f == "info[2] taken before the TERMINATED override" else None)
        self.total = self.advanced = 0
        # the stream is as after a reset: the life of the pending pairs and of the ring ends here
        self.state_writes[VS_PEND:VS_LAST] = -1
        self.state_writes[VS_RING:] = -1
        self.ties = {}
        if self.rng is not None:
            self.state[:, VS_PEND:VS_LAST] = self._junk((S, VS_LAST - VS_PEND))
            self.state[:, VS_RING:] = self._junk((S, self.stride - VS_RING))
        self._finish(e, nbits, tr)
        return nbits
