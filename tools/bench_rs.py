"""Time the Reed-Solomon outer code (qpsk_rs_encode_batch, qpsk_rs_decode_batch) at the DVB shape, 4096 rows of (204, 188), next to the
inner decoder it sits behind: qpsk_viterbi_batch on the 4096 x (8 * 204 + 6)-step rows that would carry those bytes at rate 1/2.  One
process, events as bench.py times its steps, rounds interleaved, medians.

  decode clean      every row a codeword: the syndromes and the fast exit
  decode 8 errors   8 wrong bytes at random places in every row (the radius): locator, Chien search, Forney, the second syndrome pass
  decode 16 erased  16 flagged bytes per row, all of them wrong (f = nroots, e = 0)
  encode            the parity of 4096 data rows
  viterbi           the scale: the soft rows of the same bytes, noise-free

Every decode leg is checked to return the rows that were sent before anything is timed.  No time is a condition here: the record is the
ratio of each leg to the Viterbi call.  Prints one JSON line and writes the record to --out (profiles/rs.txt).
Usage: python tools/bench_rs.py [--rows 4096] [--steps 50] [--rounds 5]
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
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rs.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m = qpsk_amd.Modem()
    R, n, k = args.rows, 204, 188
    nroots = n - k
    rng = np.random.default_rng(204)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731

    data = torch.from_numpy(rng.integers(0, 256, (R, k)).astype(np.uint8)).to(dev)
    sent = m.rs_encode(data, nroots).contiguous()
    h_sent = sent.cpu().numpy()

    def damaged(count):
        """(rows with `count` wrong bytes each at random places, the flags of those places)"""
        w, fl = h_sent.copy(), np.zeros((R, n), np.uint8)
        for r in range(R):
            at = rng.choice(n, count, replace=False)
            w[r, at] ^= rng.integers(1, 256, count).astype(np.uint8)
            fl[r, at] = 1
        return torch.from_numpy(w).to(dev), torch.from_numpy(fl).to(dev)

    errors, _ = damaged(nroots // 2)
    erased, flags = damaged(nroots)
    out = torch.zeros((R, n), dtype=torch.uint8, device=dev)
    info = torch.zeros((R, 4), dtype=torch.int32, device=dev)
    parity = torch.zeros((R, n), dtype=torch.uint8, device=dev)

    # the scale: the same bytes through the inner code at rate 1/2, tail included, noise-free soft values
    nsteps = 8 * n + 6
    dibits = m.conv_encode(sent, 8 * n, tail=True)
    d = dibits.to(torch.int32)
    soft = torch.stack([64 - 128 * (d & 1), 64 - 128 * (d >> 1)], dim=-1).to(torch.int8).contiguous()
    bits = torch.zeros((R, (nsteps + 7) // 8), dtype=torch.uint8, device=dev)
    vinfo = torch.zeros((R, 4), dtype=torch.int32, device=dev)

    def decode_leg(words, fl):
        def leg():
            m._check(m.L.qpsk_rs_decode_batch(m.h, P(words), 0, R, n, nroots, P(fl), P(out), 0, P(info)))
        return leg

    def encode():
        m._check(m.L.qpsk_rs_encode_batch(m.h, P(data), 0, R, k, nroots, P(parity), 0))

    def viterbi():
        m._check(m.L.qpsk_viterbi_batch(m.h, P(soft), 0, R, nsteps, None, 0, P(bits), P(vinfo)))

    legs = {"decode clean": decode_leg(sent, None), "decode 8 errors": decode_leg(errors, None), "decode 16 erased": decode_leg(erased, flags),
            "encode": encode, "viterbi": viterbi}
    kernels = {}
    for name, want in (("decode clean", (0, 0, 0, 1)), ("decode 8 errors", (nroots // 2, 0, nroots // 2, 0)), ("decode 16 erased", (nroots, nroots, 0, 0))):
        legs[name]()
        kernels[name] = m.last_kernel()
        m.sync()
        assert torch.equal(out, sent), name
        assert np.all(info.cpu().numpy() == np.array(want, np.int32)[None, :]), name
    encode()
    kernels["encode"] = m.last_kernel()
    viterbi()
    kernels["viterbi"] = m.last_kernel()
    m.sync()
    assert torch.equal(parity, sent) and torch.equal(bits[:, :n], sent)

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
    ratio = {name: med[name] / med["viterbi"] for name in legs if name != "viterbi"}
    rec = {"rows": R, "n": n, "k": k, "viterbi_steps": nsteps, "steps": args.steps, "rounds": args.rounds, "ms_per_call": med, "spread_ms": spread,
           "over_viterbi": ratio, "kernels": kernels, "all": res}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("The Reed-Solomon outer code beside the inner decoder -- measurement record (tools/bench_rs.py; DESIGN.md 4.4.11)\n"
                 "MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call, +- = max - min of a leg's rounds.\n"
                 "%d rows of (%d, %d); viterbi = qpsk_viterbi_batch on %d rows x %d steps, the same bytes at rate 1/2, noise-free\n\n"
                 % (args.rounds, args.steps, R, n, k, R, nsteps))
        for name in legs:
            fh.write("  %-17s %8.4f (+-%.4f)   %s   [%s]\n" % (name, med[name], spread[name],
                                                             "/ viterbi = %.4f" % ratio[name] if name in ratio else "the scale        ", kernels[name]))
        fh.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
