"""Time the batched rational resampler (qpsk_resample_push) on five shapes, each next to a device-to-device copy that moves the leg's input
plus output bytes (a pass reads and writes each sample once: 8 B per input sample, 8 B per output sample) and to the qpsk_streams_rx_cplx
call on the block the leg feeds.  One process, events as bench.py times its steps, rounds interleaved, medians.

  5/4 P8           4096 streams x 2048 outputs, L / D = 5 / 4, P = 8:   resample_push_kernel<8, staged>
  4/5 P16          the same at 4 / 5, P = 16:                           resample_push_kernel<16, staged>
  160/147 P16      the same at 160 / 147, P = 16 (44.1 -> 48 kHz):      resample_push_kernel<16, staged>, 10 KiB of taps in LDS
  4/5 P16 long     64 streams x 131072 outputs at 4 / 5, P = 16:        the same kernel on few long rows
  1/8 P16          4096 streams x 2048 outputs at 1 / 8, P = 16:        resample_push_kernel<16, staged>, a window of 2057 samples per tile
  copy <leg>       THE YARDSTICK of the leg: a device-to-device copy of (bytes in + bytes out) / 2, which reads and writes as many bytes
                   together as the leg does
  streams 4096     qpsk_streams_rx_cplx on 4096 streams x 2048 samples, the rows the legs of 4096 streams write
  streams 64       qpsk_streams_rx_cplx on 64 streams x 131072 samples, the rows of the long leg

A timed call is what a caller does per block: qpsk_resample_need, then the push with that many inputs (the need moves from push to push
where nout D is no multiple of L; the bytes counted are those of the mean need, nout D / L, rounded down).  The input is Gaussian noise at unit variance and a
Kaiser prototype (resample_prototype); neither changes what the kernels do.  Before anything is timed the first push of each shape is
compared with the numpy restatement of tests/test_resample_cpu.py on its first streams.  No time is a condition here: the record is each
leg's ratio to its copy and its share of the stream call it feeds.  NOT measured: other shapes, the direct path, hardware counters, the
launch floor at short pushes.  Prints one JSON line and writes the record to --out (profiles/resample.txt).
Usage: python tools/bench_resample.py [--steps 20] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# leg: (streams, outputs per push, L, D, P, the stream call it feeds)
SHAPES = {"5/4 P8": (4096, 2048, 5, 4, 8, "4096"), "4/5 P16": (4096, 2048, 4, 5, 16, "4096"), "160/147 P16": (4096, 2048, 160, 147, 16, "4096"),
          "4/5 P16 long": (64, 131072, 4, 5, 16, "64"), "1/8 P16": (4096, 2048, 1, 8, 16, "4096")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    from test_resample_cpu import bits, resample_ref
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    P_ = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    most = max(S * (nout * D // L + 2) for S, nout, L, D, _, _ in SHAPES.values())
    gen = torch.Generator(device=dev)
    gen.manual_seed(2020)
    x = torch.randn((most, 2), generator=gen, dtype=torch.float32, device=dev)      # every leg reads its rows from the front, tight
    legs, kernels, modems, needs, nbytes = {}, {}, {}, {}, {}
    rx = {"4096": qpsk_amd.Modem(frame_size=2048), "64": qpsk_amd.Modem(frame_size=131072)}
    out = {"4096": torch.zeros((4096, 2048, 2), dtype=torch.float32, device=dev), "64": torch.zeros((64, 131072, 2), dtype=torch.float32, device=dev)}
    for tag, (S, nout, L, D, P, feeds) in SHAPES.items():
        m = qpsk_amd.Modem(frame_size=2048)
        h = qpsk_amd.resample_prototype(L, D, P)
        m.resample_reset(S, L, D, P, h)
        K = m.resample_need(nout)
        dst = out[feeds]
        m._check(m.L.qpsk_resample_push(m.h, P_(x), 0, K, nout, P_(dst), 0))
        kernels[tag] = m.last_kernel()
        m.sync()
        first = x[:2 * K].cpu().numpy().reshape(2, K, 2)
        want, _ = resample_ref(first, None, h, L, D, P, nout)
        assert np.array_equal(bits(dst[:2].cpu().numpy()), bits(want)), tag
        modems[tag], needs[tag] = m, []

        def push(m=m, nout=nout, dst=dst, seen=needs[tag]):
            K = m.L.qpsk_resample_need(m.h, nout)
            seen.append(K)
            m._check(m.L.qpsk_resample_push(m.h, P_(x), 0, K, nout, P_(dst), 0))

        legs[tag] = push
    for feeds, m in rx.items():
        m.streams_reset(out[feeds].shape[0])
        o = m._stream_out(False)

        def streams(m=m, rows=out[feeds], o=o):
            m._check(m.L.qpsk_streams_rx_cplx(m.h, P_(rows), P_(o["sym"]), P_(o["freq"]), P_(o["phase"]), None, P_(o["index"])))

        streams()
        kernels["streams " + feeds] = m.last_kernel()
        m.sync()
        legs["streams " + feeds], modems["streams " + feeds] = streams, m
    spare = torch.empty((most, 2), dtype=torch.float32, device=dev)
    for tag, (S, nout, L, D, P, _) in SHAPES.items():
        nbytes[tag] = 8 * S * (nout * D // L + nout)                # bytes in + bytes out at the mean need
        half = nbytes[tag] // 16                                    # complex samples of (in + out) / 2 bytes
        legs["copy " + tag] = lambda half=half: spare[:half].copy_(x[:half])
        kernels["copy " + tag] = "device-to-device copy of %d bytes" % (8 * half)

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
        for m in modems.values():
            m.sync()
        return e0.elapsed_time(e1) / args.steps

    res = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            res[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in res.items()}
    spread = {name: float(max(v) - min(v)) for name, v in res.items()}
    ratio = {"%s / copy" % t: med[t] / med["copy " + t] for t in SHAPES}
    ratio.update({"%s / streams %s" % (t, s[5]): med[t] / med["streams " + s[5]] for t, s in SHAPES.items()})
    gbs = {t: nbytes[t] / med[t] / 1e6 for t in SHAPES}
    gbs.update({"copy " + t: nbytes[t] / med["copy " + t] / 1e6 for t in SHAPES})
    # lane operations per output by the definition: P multiplies and P - 1 adds on each of the two parts
    gops = {t: s[0] * s[1] * (4 * s[4] - 2) / med[t] / 1e6 for t, s in SHAPES.items()}
    rec = {"shapes": SHAPES, "bytes": nbytes, "steps": args.steps, "rounds": args.rounds, "ms_per_call": med, "spread_ms": spread, "ratios": ratio,
           "gb_per_s": gbs, "gflop_per_s": gops, "needs": {t: sorted(set(v)) for t, v in needs.items()}, "kernels": kernels, "all": res}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("The batched rational resampler beside its yardsticks -- measurement record (tools/bench_resample.py; DESIGN.md 4.4.20)\n"
                 "MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call, +- = max - min of a leg's rounds.\n"
                 "A leg: streams x outputs per push at L / D with P taps per branch; a call = qpsk_resample_need + qpsk_resample_push.\n"
                 "copy <leg>: (bytes in + bytes out) / 2 of the leg, device to device; streams: qpsk_streams_rx_cplx on the rows the legs wrote.\n"
                 "GB/s = (bytes in + bytes out) / time; GFLOP/s = outputs x (4 P - 2) / time, the definition's unfused multiplies and adds.\n"
                 "Not measured: other shapes, the direct path, hardware counters, the launch floor at short pushes.\n\n" % (args.rounds, args.steps))
        for name in legs:
            shape = "%d x %d, %d/%d, P = %d" % SHAPES[name][:5] if name in SHAPES else ""
            fh.write("  %-18s %9.4f (+-%.4f)   %-10s %-13s %-28s [%s]\n" % (name, med[name], spread[name], "%.0f GB/s" % gbs[name] if name in gbs else "",
                                                                       "%.0f GFLOP/s" % gops[name] if name in gops else "", shape, kernels[name]))
        fh.write("\n")
        for name, v in ratio.items():
            fh.write("  %-32s %.4f\n" % (name, v))
        fh.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
