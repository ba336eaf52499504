"""Time the packet erasure code (qpsk_rs_cross_encode_batch, qpsk_rs_cross_decode_batch, qpsk_rs_cross_place_batch) at 4096 groups of
(20, 16) x 32-byte packets, skip 1, next to what a caller paid before it existed.  One process, events as bench.py times its steps, rounds
interleaved, medians.

  encode            the 4 parity packets of 4096 groups, in place
  decode f = 0      every group complete: the check alone, out of place (so every byte is copied)
  decode f = 4      4 packets missing per group at random places, filled with garbage, out of place
  place             4096 streams x 20 packets of one push sorted into one group each, numbers shuffled
  rows f = 4        THE YARDSTICK of decode f = 4: qpsk_rs_decode_batch on the same 4096 x 31 columns laid out as rows beforehand, the same
                    4 places flagged in each -- a wave per codeword.  The two transposes a caller needs around it are NOT in the time
  rows encode       THE YARDSTICK of encode: qpsk_rs_encode_batch on the 4096 x 31 data columns laid out as rows beforehand
  copy              THE YARDSTICK of decode f = 0 and of place: a device-to-device copy of the group buffer

Every decode leg is checked to return the groups that were sent before anything is timed.  No time is a condition here: the record is
each leg's ratio to its yardstick.  Prints one JSON line and writes the record to --out (profiles/cross.txt).
Usage: python tools/bench_cross.py [--groups 4096] [--steps 50] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m = qpsk_amd.Modem()
    G, n, k, ln, skip, f = args.groups, 20, 16, 32, 1, 4
    nroots, width = n - k, ln - skip
    rng = np.random.default_rng(2016)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731

    plain = rng.integers(0, 256, (G, n, ln)).astype(np.uint8)
    plain[:, :, 0] = np.arange(n, dtype=np.uint8)[None, :]             # byte 0: the sequence number, base 0
    work = torch.from_numpy(plain).to(dev)
    sent = m.rs_cross_encode(work.clone(), nroots, skip=skip)
    h_sent = sent.cpu().numpy()

    have = np.ones((G, n), np.uint8)
    hit = h_sent.copy()
    for g in range(G):
        at = rng.choice(n, f, replace=False)
        have[g, at] = 0
        hit[g, at, skip:] = rng.integers(0, 256, (f, width)).astype(np.uint8)
    d_hit, d_have = torch.from_numpy(hit).to(dev), torch.from_numpy(have).to(dev)
    d_full = torch.ones((G, n), dtype=torch.uint8, device=dev)
    out = torch.zeros((G, n, ln), dtype=torch.uint8, device=dev)
    info = torch.zeros((G, 4), dtype=torch.int32, device=dev)

    # the yardstick's rows: column j of group g is row g * width + j, the missing places flagged
    rows = torch.from_numpy(np.ascontiguousarray(hit[:, :, skip:].transpose(0, 2, 1)).reshape(G * width, n)).to(dev)
    flags = torch.from_numpy(np.ascontiguousarray(np.repeat((have == 0).astype(np.uint8), width, axis=0))).to(dev)
    want_rows = torch.from_numpy(np.ascontiguousarray(h_sent[:, :, skip:].transpose(0, 2, 1)).reshape(G * width, n)).to(dev)
    rows_out = torch.zeros((G * width, n), dtype=torch.uint8, device=dev)
    rows_info = torch.zeros((G * width, 4), dtype=torch.int32, device=dev)
    rows_data = want_rows[:, :k].contiguous()
    rows_enc = torch.zeros((G * width, n), dtype=torch.uint8, device=dev)

    # place: one push of n packets per stream, in shuffled order, every CRC good
    order = np.stack([rng.permutation(n) for _ in range(G)])
    pushed = np.take_along_axis(h_sent, order[:, :, None], axis=1)
    d_bytes = torch.from_numpy(np.ascontiguousarray(pushed)).to(dev)
    d_count = torch.full((G,), n, dtype=torch.int32, device=dev)
    d_ok = torch.ones((G, n), dtype=torch.uint8, device=dev)
    placed = torch.zeros((G, 1, n, ln), dtype=torch.uint8, device=dev)
    placed_have = torch.zeros((G, n), dtype=torch.uint8, device=dev)

    def encode():
        m._check(m.L.qpsk_rs_cross_encode_batch(m.h, P(work), 0, G, k, nroots, ln, skip))

    def decode_leg(groups, hv):
        def leg():
            m._check(m.L.qpsk_rs_cross_decode_batch(m.h, P(groups), 0, G, n, nroots, ln, skip, P(hv), P(out), 0, P(info), None))
        return leg

    def place():
        m._check(m.L.qpsk_rs_cross_place_batch(m.h, P(d_bytes), 0, P(d_count), P(d_ok), G, n, ln, n, 1, None, P(placed), 0, P(placed_have)))

    def rows_leg():
        m._check(m.L.qpsk_rs_decode_batch(m.h, P(rows), 0, G * width, n, nroots, P(flags), P(rows_out), 0, P(rows_info)))

    def rows_encode():
        m._check(m.L.qpsk_rs_encode_batch(m.h, P(rows_data), 0, G * width, k, nroots, P(rows_enc), 0))

    def copy():
        out.copy_(d_hit)

    legs = {"encode": encode, "decode f = 0": decode_leg(sent, d_full), "decode f = 4": decode_leg(d_hit, d_have), "place": place,
            "rows f = 4": rows_leg, "rows encode": rows_encode, "copy": copy}
    yardstick = {"encode": "rows encode", "decode f = 0": "copy", "decode f = 4": "rows f = 4", "place": "copy"}
    kernels = {}
    for name, want in (("decode f = 0", (0, 0, 0, 1)), ("decode f = 4", None)):
        out.zero_()
        legs[name]()
        kernels[name] = m.last_kernel()
        m.sync()
        assert torch.equal(out, sent), name
        got = info.cpu().numpy()
        assert np.all(got[:, [0, 1, 3]] == (np.array([0, f, 1]) if want is None else np.array(want)[[0, 1, 3]])[None, :]), name
    encode()
    kernels["encode"] = m.last_kernel()
    place()
    kernels["place"] = m.last_kernel()
    rows_leg()
    kernels["rows f = 4"] = m.last_kernel()
    rows_encode()
    kernels["rows encode"] = m.last_kernel()
    kernels["copy"] = "device-to-device copy"
    m.sync()
    assert torch.equal(rows_enc, want_rows)
    assert torch.equal(work, sent) and torch.equal(placed[:, 0], sent) and bool(placed_have.all()) and torch.equal(rows_out, want_rows)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        m.sync()
        return e0.elapsed_time(e1) / args.steps

    res = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            res[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in res.items()}
    spread = {name: float(max(v) - min(v)) for name, v in res.items()}
    ratio = {name: med[name] / med[y] for name, y in yardstick.items()}
    rec = {"groups": G, "n": n, "k": k, "len": ln, "skip": skip, "missing": f, "steps": args.steps, "rounds": args.rounds, "ms_per_call": med,
           "spread_ms": spread, "over_yardstick": ratio, "yardstick": yardstick, "kernels": kernels, "all": res}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("The packet erasure code beside its yardsticks -- measurement record (tools/bench_cross.py; DESIGN.md 4.4.17)\n"
                 "MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call, +- = max - min of a leg's rounds.\n"
                 "%d groups of (%d, %d) x %d-byte packets, skip %d; rows f = %d: qpsk_rs_decode_batch on the same %d codewords as rows, the\n"
                 "same %d places flagged (the caller's two transposes not timed); copy: the %d-byte group buffer, device to device\n\n"
                 % (args.rounds, args.steps, G, n, k, ln, skip, f, G * width, f, G * n * ln))
        for name in legs:
            fh.write("  %-13s %8.4f (+-%.4f)   %-28s [%s]\n" % (name, med[name], spread[name],
                                                               "/ %s = %.4f" % (yardstick[name], ratio[name]) if name in ratio else "a yardstick",
                                                               kernels[name]))
        fh.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
