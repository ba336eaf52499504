"""Time qpsk_frame_batch next to the composition of existing calls that produces the same bytes, in one process, with events as bench.py
times its steps; rounds interleaved, medians.  Shapes: 4096 rows x 1 packet of 64 bytes and 4096 rows x 4 packets (32-dibit word, lead 0,
gap 0, the exact fit, so that the composition needs no idle fill); codings: uncoded, rate 1/2, rate 3/4.

  frame     qpsk_frame_batch: one launch
  compose   qpsk_crc16_batch -> the CRC appended big-endian (torch) -> qpsk_conv_encode_batch / qpsk_conv_encode_punct_batch (uncoded:
            qpsk_pack_symbols' packing in reverse, in torch) -> qpsk_scramble_batch -> the sync word and the body copied into the rows
            (torch), all into buffers allocated beforehand, on the context's stream

Both legs are checked to give the same bytes before anything is timed.  The one condition: the framer's median is not above the
composition's median by more than the composition's own spread (max - min of its round medians).  Prints one JSON line and writes the
record to --out (profiles/frame.txt).
Usage: python tools/bench_frame.py [--rows 4096] [--steps 50] [--rounds 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    from qpsk_amd.lib import PUNCTURE
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m = qpsk_amd.Modem()
    R, nbytes, nsync = args.rows, 64, 32
    nb, nbits = nbytes + 2, 8 * (nbytes + 2)
    rng = np.random.default_rng(4)
    word = np.ascontiguousarray(rng.integers(0, 4, nsync).astype(np.uint8))
    d_word = torch.from_numpy(word).to(dev)
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731

    def legs_of(per_row, coding):
        """-> (frame, compose, out_frame, out_compose, kernel name) for one shape and coding"""
        npk = R * per_row
        coded = coding != "uncoded"
        pat = PUNCTURE[coding] if coded else (1, 1, 1)
        plen = qpsk_amd.frame_len(nsync, nbytes, coded=coded, puncture=pat if coded else None)
        B = plen - nsync
        payload = torch.from_numpy(rng.integers(0, 256, (npk, nbytes)).astype(np.uint8)).to(dev)
        out_f = torch.zeros((R, per_row * plen), dtype=torch.uint8, device=dev)
        out_c = torch.zeros((R, per_row * plen), dtype=torch.uint8, device=dev)
        crc_f = torch.zeros(npk, dtype=torch.int16, device=dev)
        crc_c = torch.zeros(npk, dtype=torch.int16, device=dev)
        pkt = torch.zeros((npk, nb), dtype=torch.uint8, device=dev)
        body = torch.zeros((npk, B), dtype=torch.uint8, device=dev)
        rows = out_c.view(npk, plen)

        def frame():
            m._check(m.L.qpsk_frame_batch(m.h, P(payload), 0, R, per_row, nbytes, word.ctypes.data_as(C.c_void_p), nsync, 1 if coded else 0, *pat,
                                          0, 0, per_row * plen, P(out_f), P(crc_f)))

        def compose():
            m._check(m.L.qpsk_crc16_batch(m.h, P(payload), npk, nbytes, P(crc_c)))
            c = crc_c.to(torch.int32)
            pkt[:, :nbytes].copy_(payload)
            pkt[:, nbytes].copy_((c >> 8) & 255)
            pkt[:, nbytes + 1].copy_(c & 255)
            if not coded:
                body.copy_(((pkt.to(torch.int32)[:, :, None] >> shifts) & 3).reshape(npk, B))
            elif coding == "1/2":
                m._check(m.L.qpsk_conv_encode_batch(m.h, P(pkt), npk, nbits, 1, P(body)))
            else:
                m._check(m.L.qpsk_conv_encode_punct_batch(m.h, P(pkt), npk, nbits, 1, *pat, P(body)))
            m._check(m.L.qpsk_scramble_batch(m.h, P(body), npk, B))
            rows[:, :nsync].copy_(d_word)
            rows[:, nsync:].copy_(body)

        frame()
        kernel = m.last_kernel()
        compose()
        m.sync()
        assert torch.equal(out_f, out_c) and torch.equal(crc_f, crc_c), (per_row, coding)
        return frame, compose, kernel

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

    cases = [(per_row, coding) for per_row in (1, 4) for coding in ("uncoded", "1/2", "3/4")]
    legs = {case: legs_of(*case) for case in cases}
    res = {case: {"frame": [], "compose": []} for case in cases}
    for _ in range(args.rounds):
        for case in cases:
            res[case]["frame"].append(timed(legs[case][0]))
            res[case]["compose"].append(timed(legs[case][1]))
    table, ok = [], True
    for case in cases:
        f, c = res[case]["frame"], res[case]["compose"]
        mf, mc, spread = float(np.median(f)), float(np.median(c)), float(max(c) - min(c))
        within = mf <= mc + spread
        ok = ok and within
        table.append({"per_row": case[0], "coding": case[1], "kernel": legs[case][2], "frame_ms": mf, "compose_ms": mc, "compose_spread_ms": spread,
                      "compose_over_frame": mc / mf, "frame_not_above_compose_plus_spread": within, "frame_rounds": f, "compose_rounds": c})
    rec = {"rows": R, "nbytes": nbytes, "nsync": nsync, "steps": args.steps, "rounds": args.rounds, "condition_holds": ok, "cases": table}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("qpsk_frame_batch against the composition of existing calls, %d rows of 1 and of 4 packets of %d bytes, %d-dibit word, exact fit\n"
                 "(tools/bench_frame.py: MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call; spread = max - min\n"
                 "of the composition's rounds)\n\n" % (R, nbytes, nsync, args.rounds, args.steps))
        fh.write("  per_row coding    frame    compose   spread   compose / frame\n")
        for t in table:
            fh.write("  %7d %-7s %8.4f %9.4f %8.4f %10.1f\n" % (t["per_row"], t["coding"], t["frame_ms"], t["compose_ms"], t["compose_spread_ms"],
                                                              t["compose_over_frame"]))
        fh.write("\nThe framer's median is %s the composition's median + spread in every case.\n\n" % ("not above" if ok else "ABOVE (in some case)"))
        fh.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
