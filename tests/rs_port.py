"""rs_decode_kernel and rs_encode_kernel of qpsk_amd/csrc/rs.hip restated in scalar Python -- the KERNELS, not the header: one wave per row,
64 explicit lanes (every per-lane variable is an array of 64, every wave-uniform one a plain int with the kernel's name), the workgroup's
LDS as ONE array of bytes laid out as RsLds (exp[512], log[256], then RS_WAVES slices of row[256] syn[64] lam[68] om[64]), the row staged
right-aligned behind `pad` zeros, the four interleaved Horner runs, the erasure locator in ballot order, Berlekamp-Massey with lane l holding
Lambda_(l + 1) and (x B)_(l + 1), Chien and Forney per 64-lane chunk, the three-part early test, the second syndromes and leave().

test_rs_port_cpu.py holds the port equal to the numpy restatements of the header (test_rs_cpu.rs_decode_ref / rs_encode_ref) on every row the
GPU tests decode, so that the port stands for the kernel, and then uses it for what cannot be done on a device:

  trace     per row the exit taken, the checks of the early test that fired, and the rare events of the algorithm (EVENTS).  rs_rows.py
            picks its directed rows by them.
  indices   the highest index used in exp[], row[], syn[], lam[] and om[] (BOUNDS).  The LDS is one array here as there, so an index past
            its table reads what lies behind it -- the log table, a neighbouring wave's slice -- and fails nothing; only the record shows it.
  faults    fault= switches on exactly ONE of FAULTS (decoder) or ENCODE_FAULTS, a single wrong token each.  The GPU tests' inputs are
            adequate when every fault changes an output or leaves a bound on them.  Nothing faulty exists outside this file.
  removals  remove= takes out ONE of the early exits REMOVALS.  rs.hip's header says nothing rests on them: no output may change, ever.

A launch finds its LDS holding whatever the last workgroup left there: the port fills it with random bytes (seed=) before every workgroup."""
import numpy as np

RS_WAVES, RS_MAX_ROOTS = 4, 64
EXP_AT, LOG_AT, SLICES_AT = 0, 512, 768                      # struct RsLds { GfTables gf; RsSlice w[RS_WAVES]; }
FIELD_AT = dict(row=0, syn=256, lam=320, om=388)             # struct RsSlice
SLICE_BYTES = 452
BOUNDS = dict(exp=511, row=255, syn=63, lam=67, om=63)
_ROOM = 2048                                                 # behind the LDS, so that an overrun is recorded instead of raised

FAULTS = (
    # Berlekamp-Massey
    "a zero discrepancy keeps xb",                           # d == 0: continue without xb = shifted
    "len forgets f",                                         # len = r - len
    "the length test forgets f",                             # 2 len <= r - 1
    "lane 0 of the erasure product takes 0 for prev",
    "lane 0 of up takes 0",                                  # B loses its constant term
    # verdict and counts
    "no second syndromes",
    "S2 not zeroed on lanes >= nroots",
    "e counts flagged places",
    "changed counts roots",
    "info's e holds changed",
    "a failed row leaves with the corrected bytes",
    # staging and syndromes
    "the row left-aligned",                                  # zeros behind
    "the pad zeros are not written",
    "the scale factors of h0 and h1 swapped",
    "a scale factor's % 255 dropped",                        # 3 s: the index leaves exp[]
    "S not zeroed on lanes >= nroots",
    # erasures
    "an erasure's position without 64 c",
    "erasure locator alpha^(n - j)",
    # Forney
    "Forney's factor X_j dropped",
    "top takes the even term",
    "ly2's % 255 dropped",                                   # the index leaves exp[]
    # Chien and exits
    "Chien counts lanes with j >= n",
    "f >= nroots fails",
    "the clean exit taken before the f > nroots test",
)
ENCODE_FAULTS = (
    "feedback taken from lane 1",
    "lane 63 keeps its own value",                           # shfl_down without the lane == 63 substitute
)
# Not in the lists, because no input can show them; the port still takes each as fault=, and test_rs_port_cpu.py checks on every row it
# has that nothing changes:
EQUIVALENT = {
    "chunk skip 64 c > n": "at n = 64 c the chunk has no valid lane, so no root, rm == 0 and the next skip takes it; cb[c] = rb[c] is never stored",
    "Omega loses its Lambda_deg term": "otop <= deg - 1 and Omega_i for i < deg sums k <= i only: the term is never read",
    "lane < nroots dropped from gn": "the launcher zero-fills RsEncodeArgs, so gnz[lane] is 0 on every lane >= nroots",
    "gnz ignored": "no generator with nroots <= 64 has a zero coefficient, so gnz is 1 on every lane < nroots (checked for all 64)",
}
REMOVALS = ("nz == 0", "bad", "roots != deg")
EVENTS = ("interior zero discrepancy", "zero discrepancy at r = f + 1", "length jump of 2", "length jump of 3 or more",
          "length change right after a zero", "dd == 0 at a root", "a root in the shortened region", "a root whose value is 0", "deg != len")
EXITS = ("f > nroots", "clean", "nz == 0", "bad", "roots != deg", "2 e + f", "second syndromes", "decoded")

LANE = np.arange(64, dtype=np.int64)


def gf_tables():
    """gf_make(): exp[i] = alpha^i for i < 510 (the period twice), the last two 0; log[0] = 0 is never used as a logarithm"""
    exp, log = np.zeros(512, np.int64), np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i] = exp[i + 255] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    return exp, log


_EXP, _LOG = gf_tables()


def generator(nroots):
    """rs_generator(): g(x) = prod (x - alpha^i), highest coefficient first"""
    low = [1] + [0] * nroots
    for i in range(nroots):
        for j in range(i + 1, 0, -1):
            m = int(_EXP[_LOG[low[j]] + i]) if low[j] else 0
            low[j] = low[j - 1] ^ m
        low[0] = int(_EXP[_LOG[low[0]] + i]) if low[0] else 0
    return low[::-1]


def shfl_up(v):
    """__shfl_up(v, 1, 64): lane 0 keeps its own value"""
    return np.concatenate([v[:1], v[:-1]])


def shfl_down(v):
    """__shfl_down(v, 1, 64): lane 63 keeps its own value"""
    return np.concatenate([v[1:], v[-1:]])


class rs_port:
    """decode(words (R, n), nroots, flags (R, n) or None) -> (out (R, n) uint8, info (R, 4) int32), the traces of the call in .traces;
    encode(data (R, k), nroots) -> (R, k + nroots).  .hi = the highest index used per table so far, over_bounds() what left its table."""

    def __init__(self, fault=None, remove=None, seed=0):
        assert fault is None or fault in FAULTS or fault in ENCODE_FAULTS or fault in EQUIVALENT, fault
        assert remove is None or remove in REMOVALS, remove
        self.fault, self.remove = fault, remove
        self.rng = np.random.default_rng(seed)
        self.hi = dict.fromkeys(BOUNDS, -1)
        self.traces = []
        self.mem = None

    def over_bounds(self):
        """None, or the first table an index left"""
        for name, bound in BOUNDS.items():
            if self.hi[name] > bound:
                return "%s[%d] used, the last entry is %d" % (name, self.hi[name], bound)
        return None

    # ------------------------------------------------------------------ the LDS of one workgroup
    def _launch(self):
        """a workgroup's LDS as it finds it, then load_tables()"""
        self.mem = self.rng.integers(0, 256, SLICES_AT + RS_WAVES * SLICE_BYTES + _ROOM).astype(np.int64)
        self.mem[EXP_AT:EXP_AT + 512] = _EXP
        self.mem[LOG_AT:LOG_AT + 256] = _LOG

    def _note(self, name, idx):
        top = idx if isinstance(idx, int) else int(idx.max())                   # (no index is ever negative: each is guarded where it is made)
        if top > self.hi[name]:
            self.hi[name] = top

    def _exp(self, idx):
        self._note("exp", idx)
        return self.mem[EXP_AT + idx]

    def _log(self, a):
        return self.mem[LOG_AT + a]

    def _gmul(self, a, b):
        v = self._exp(self._log(a) + self._log(b))
        return np.where((a != 0) & (b != 0), v, 0)

    def _gmul_log(self, a, l):
        v = self._exp(self._log(a) + l)
        return np.where(a != 0, v, 0)

    def _rd(self, base, name, idx):
        self._note(name, idx)
        return self.mem[base + FIELD_AT[name] + idx]

    def _wr(self, base, name, idx, v):
        self._note(name, idx)
        self.mem[base + FIELD_AT[name] + idx] = np.asarray(v, np.int64) & 255

    def _syndrome(self, base, q):
        """syndrome(): lane i = LANE; the four chains are the rows of h"""
        fault, i = self.fault, LANE
        h = np.zeros((4, 64), np.int64)
        starts = np.array([0, q, 2 * q, 3 * q], np.int64)
        for t in range(q):
            h = self._gmul_log(h, i[None, :]) ^ self._rd(base, "row", starts + t)[:, None]
        s = (i * q) % 255
        s3, s2 = (3 * s) % 255, (2 * s) % 255
        if fault == "a scale factor's % 255 dropped":
            s3 = 3 * s
        if fault == "the scale factors of h0 and h1 swapped":
            s3, s2 = s2, s3
        return self._gmul_log(h[0], s3) ^ self._gmul_log(h[1], s2) ^ self._gmul_log(h[2], s) ^ h[3]

    # ------------------------------------------------------------------ rs_decode_kernel
    def decode(self, words, nroots, flags=None):
        w = np.atleast_2d(np.asarray(words, np.uint8))
        R, n = w.shape
        assert 1 <= nroots <= RS_MAX_ROOTS and nroots < n <= 255            # launch_rs_decode
        er = None if flags is None else np.atleast_2d(np.asarray(flags))
        out, info = np.zeros((R, n), np.uint8), np.zeros((R, 4), np.int32)
        self.traces = []
        for urow in range(R):
            wave = urow % RS_WAVES
            if wave == 0:
                self._launch()
            o, i4, trace = self._decode_wave(SLICES_AT + wave * SLICE_BYTES, w[urow].astype(np.int64), None if er is None else er[urow], n, nroots)
            out[urow], info[urow] = o, i4
            self.traces.append(trace)
        return out, info

    def _decode_wave(self, base, src, er, n, nroots):
        fault, remove, lane = self.fault, self.remove, LANE
        q = (n + 3) >> 2
        pad = 4 * q - n
        rb, fl = np.zeros((4, 64), np.int64), np.zeros((4, 64), bool)
        left = fault == "the row left-aligned"
        for c in range(4):
            j = lane + 64 * c
            m = j < n
            rb[c, m] = src[j[m]]
            if er is not None:
                fl[c, m] = er[j[m]] != 0
            if m.any():
                self._wr(base, "row", (0 if left else pad) + j[m], rb[c, m])
        if pad and fault != "the pad zeros are not written":
            self._wr(base, "row", (n if left else 0) + lane[:pad], 0)
        f = int(fl.sum())
        trace = dict(exit=None, fired=(), events=set(), f=f, zeros=[], nonzero=[], changes=[], len=None, deg=None, roots=None)

        S = self._syndrome(base, q)
        if fault != "S not zeroed on lanes >= nroots":
            S = np.where(lane >= nroots, 0, S)
        clean = 0 if S.any() else 1
        out, info = np.zeros(n, np.uint8), np.zeros(4, np.int32)

        def leave(how, byts, changed, e):
            for c in range(4):
                j = lane + 64 * c
                m = j < n
                out[j[m]] = byts[c, m]
            info[:] = (changed, f, changed if fault == "info's e holds changed" else e, clean)
            trace["exit"] = how
            return out, info, trace

        too_many = f >= nroots if fault == "f >= nroots fails" else f > nroots
        if fault == "the clean exit taken before the f > nroots test":
            if clean:
                return leave("clean", rb, 0, 0)
            if too_many:
                return leave("f > nroots", rb, -1, -1)
        else:
            if too_many:
                return leave("f > nroots", rb, -1, -1)
            if clean:
                return leave("clean", rb, 0, 0)
        self._wr(base, "syn", lane, S)

        # Lambda = the erasure locator; lane l holds Lambda_(l + 1)
        lam = np.zeros(64, np.int64)
        for c in range(4):
            for b in np.nonzero(fl[c])[0]:                                      # the ballot's bits from the lowest: __ffsll, m &= m - 1
                j = int(b) if fault == "an erasure's position without 64 c" else 64 * c + int(b)
                prev = shfl_up(lam)
                prev[0] = 0 if fault == "lane 0 of the erasure product takes 0 for prev" else 1
                lam = lam ^ self._gmul_log(prev, n - j if fault == "erasure locator alpha^(n - j)" else n - 1 - j)
        # Berlekamp-Massey; xb = x B, lane l holds (x B)_(l + 1)
        xb = shfl_up(lam)
        xb[0] = 1
        ln = f
        for r in range(f + 1, nroots + 1):
            at = r - 2 - lane
            term = np.where(at >= 0, self._gmul(lam, self._rd(base, "syn", np.where(at >= 0, at, 0))), 0)
            d = int(np.bitwise_xor.reduce(term)) ^ int(self._rd(base, "syn", r - 1))
            shifted = shfl_up(xb)
            shifted[0] = 0
            if d == 0:
                if fault != "a zero discrepancy keeps xb":
                    xb = shifted
                trace["zeros"].append(r)
                continue
            trace["nonzero"].append(r)
            nxt = lam ^ self._gmul(np.int64(d), xb)
            if 2 * ln <= (r - 1 if fault == "the length test forgets f" else r + f - 1):
                new = r - ln if fault == "len forgets f" else r + f - ln
                trace["changes"].append((r, ln, new))
                ln = new
                dinv = self._exp(255 - self._log(d))
                up = shfl_up(lam)
                up[0] = 0 if fault == "lane 0 of up takes 0" else 1
                xb = self._gmul(up, dinv)
            else:
                xb = shifted
            lam = nxt
        trace["len"] = ln
        self._events_of_bm(trace, f)
        nz = np.nonzero(lam)[0]
        if len(nz) == 0 and remove != "nz == 0":
            return leave("nz == 0", rb, -1, -1)
        deg = int(nz[-1]) + 1 if len(nz) else 0                                 # 64 - clz(0) = 0
        trace["deg"] = deg
        if deg != ln:
            trace["events"].add("deg != len")
        self._wr(base, "lam", lane + 1, lam)
        self._wr(base, "lam", 0, 1)

        # Omega_i = sum_k S_(i - k) Lambda_k
        om = np.zeros(64, np.int64)
        for k in range(0, min(deg - 1 if fault == "Omega loses its Lambda_deg term" else deg, 63) + 1):
            at = lane - k
            t = self._gmul(self._rd(base, "syn", np.where(at >= 0, at, 0)), self._rd(base, "lam", k))
            om = om ^ np.where(at >= 0, t, 0)
        self._wr(base, "om", lane, np.where(lane < nroots, om, 0))

        cb = rb.copy()
        roots = changed = e = 0
        bad = False
        top = deg if (deg & 1) else deg - 1
        if fault == "top takes the even term":
            top = deg - 1 if (deg & 1) else deg
        for c in range(4):
            if 64 * c > n if fault == "chunk skip 64 c > n" else 64 * c >= n:
                continue
            j = lane + 64 * c
            valid = j < n
            lx = np.where(valid, n - 1 - j, 0)
            ly = (255 - lx) % 255
            v = np.zeros(64, np.int64)
            for i in range(deg, -1, -1):
                v = self._gmul_log(v, ly) ^ self._rd(base, "lam", i)
            root = (v == 0) if fault == "Chien counts lanes with j >= n" else valid & (v == 0)
            roots += int(root.sum())
            if not root.any():
                continue
            o, dd = np.zeros(64, np.int64), np.zeros(64, np.int64)
            otop = min(deg - 1, nroots - 1)
            for i in range(otop, -1, -1):
                o = self._gmul_log(o, ly) ^ self._rd(base, "om", i)
            ly2 = 2 * ly if fault == "ly2's % 255 dropped" else (2 * ly) % 255
            for i in range(top, 0, -2):
                dd = self._gmul_log(dd, ly2) ^ self._rd(base, "lam", i)
            num = o if fault == "Forney's factor X_j dropped" else self._gmul_log(o, lx)
            quot = self._exp(self._log(num) + 255 - self._log(dd))
            val = np.where(root & (num != 0) & (dd != 0), quot, 0)
            if (root & (dd == 0)).any():
                bad = True
                trace["events"].add("dd == 0 at a root")
            if (root & (val == 0)).any():
                trace["events"].add("a root whose value is 0")
            cb[c] = rb[c] ^ val
            changed += int(root.sum()) if fault == "changed counts roots" else int((val != 0).sum())
            e += int((val != 0).sum()) if fault == "e counts flagged places" else int(((val != 0) & ~fl[c]).sum())
        trace["roots"] = roots
        if self._shortened_root(lam, n):
            trace["events"].add("a root in the shortened region")
        fired = tuple(name for name, on in (("bad", bad), ("roots != deg", roots != deg), ("2 e + f", 2 * e + f > nroots)) if on)
        trace["fired"] = fired
        failed = rb if fault != "a failed row leaves with the corrected bytes" else cb
        acting = tuple(name for name in fired if name != remove)
        if acting:
            return leave(acting[0], failed, -1, -1)

        # the verdict: the corrected word's own syndromes
        for c in range(4):
            j = lane + 64 * c
            m = j < n
            if m.any():
                self._wr(base, "row", (0 if left else pad) + j[m], cb[c, m])
        if fault != "no second syndromes":
            S2 = self._syndrome(base, q)
            if fault != "S2 not zeroed on lanes >= nroots":
                S2 = np.where(lane >= nroots, 0, S2)
            if S2.any():
                return leave("second syndromes", failed, -1, -1)
        return leave("decoded", cb, changed, e)

    @staticmethod
    def _events_of_bm(trace, f):
        zeros, changes = trace["zeros"], trace["changes"]
        last_nonzero = max(trace["nonzero"], default=0)                        # a zero followed by a non-zero one: the shift of xb is used
        if any(z < last_nonzero for z in zeros):
            trace["events"].add("interior zero discrepancy")
        if f + 1 in zeros and last_nonzero > f + 1:
            trace["events"].add("zero discrepancy at r = f + 1")
        for r, old, new in changes:
            if new - old == 2:
                trace["events"].add("length jump of 2")
            if new - old >= 3:
                trace["events"].add("length jump of 3 or more")
            if r - 1 in zeros:
                trace["events"].add("length change right after a zero")

    @staticmethod
    def _shortened_root(lam, n):
        """the trace only, nothing of the kernel: does Lambda vanish at an X^-1 of the missing leading bytes, X = alpha^n .. alpha^254"""
        coef = [1] + [int(x) for x in lam]
        for lx in range(n, 255):
            ly, v = (255 - lx) % 255, 0
            for cf in reversed(coef):
                v = (int(_EXP[_LOG[v] + ly]) if v else 0) ^ cf
            if v == 0:
                return True
        return False

    # ------------------------------------------------------------------ rs_encode_kernel
    def encode(self, data, nroots):
        d = np.atleast_2d(np.asarray(data, np.uint8)).astype(np.int64)
        R, k = d.shape
        assert k >= 1 and 1 <= nroots <= RS_MAX_ROOTS and k + nroots <= 255    # launch_rs_encode
        fault, lane = self.fault, LANE
        gen = generator(nroots)
        glog, gnz = np.zeros(64, np.int64), np.zeros(64, np.int64)              # RsEncodeArgs a{}: zeros behind nroots
        for l in range(nroots):
            glog[l], gnz[l] = _LOG[gen[l + 1]], gen[l + 1] != 0
        out = np.zeros((R, k + nroots), np.uint8)
        for urow in range(R):
            wave = urow % RS_WAVES
            if wave == 0:
                self._launch()
            base = SLICES_AT + wave * SLICE_BYTES
            self._wr(base, "row", np.arange(k), d[urow])
            out[urow, :k] = d[urow]
            gl = glog[lane]
            gn = gnz[lane] != 0
            if fault != "lane < nroots dropped from gn":
                gn = gn & (lane < nroots)
            if fault == "gnz ignored":
                gn = lane < nroots
            par = np.zeros(64, np.int64)
            for j in range(k):
                fb = int(self._rd(base, "row", j)) ^ int(par[1 if fault == "feedback taken from lane 1" else 0])
                nxt = shfl_down(par)
                if fault != "lane 63 keeps its own value":
                    nxt[63] = 0
                t = self._exp(self._log(fb) + gl)
                par = nxt ^ (np.where(gn, t, 0) if fb else 0)
            out[urow, k:] = par[:nroots]
        return out
