"""Time the polyphase channeliser (qpsk_channel_push) on the 4096-stream block and on the same bytes at M = 64, next to a device-to-device
copy of its input (the algorithmic traffic is 8 B in and 8 B out per sample) and to the qpsk_streams_rx_cplx call on the block the push
produces.  One process, events as bench.py times its steps, rounds interleaved, medians.

  push 4096        M = 4096, P = 8, T = 2048: 64 MiB in, 64 MiB out, channel_push_kernel<8, 1024>, tile 4
  push 64          M = 64, P = 16, T = 131072: the same bytes, channel_push_kernel<16, 256>, tile 128
  push 4096 x1     push 4096 with one channel selected: the branch sums and the transform of every channel, the store of one row --
                   what push 4096 costs beyond it is its transposed store (32-byte segments, 16 KiB apart)
  copy             THE YARDSTICK of both pushes: a device-to-device copy of the 64 MiB input
  streams 4096     qpsk_streams_rx_cplx on 4096 streams x 2048 samples, the rows push 4096 wrote (a context with frame_size 2048)
  streams 64       qpsk_streams_rx_cplx on 64 streams x 131072 samples, the rows push 64 wrote (a context with frame_size 131072)

The input is Gaussian noise at unit variance and a Kaiser prototype (channel_prototype); neither changes what the kernels do.  Before
anything is timed a push of each shape is compared with the numpy restatement of tests/test_channel_cpu.py on its first output times.  No
time is a condition here: the record is each push's ratio to the copy and its share of the stream call it feeds.  NOT measured: other
shapes, hardware counters, the launch floor at small M and short pushes.  Prints one JSON line and writes the record to --out
(profiles/channel.txt).
Usage: python tools/bench_channel.py [--steps 20] [--rounds 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    from test_channel_cpu import bits, channel_ref, twiddles
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    P_ = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    shapes = {"4096": (4096, 8, 2048), "64": (64, 16, 131072)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(2018)
    x = torch.randn((4096 * 2048, 2), generator=gen, dtype=torch.float32, device=dev)
    dst = torch.empty_like(x)
    legs, kernels, modems, rows = {}, {}, {}, {}
    for tag, (M, P, T) in shapes.items():
        m = qpsk_amd.Modem(frame_size=T)
        h = qpsk_amd.channel_prototype(M, P)
        m.channel_reset(M, P, h)
        out = torch.zeros((M, T, 2), dtype=torch.float32, device=dev)
        m._check(m.L.qpsk_channel_push(m.h, P_(x), T, P_(out), 0))
        kernels["push " + tag] = m.last_kernel()
        m.sync()
        check = 4 * P
        want, _ = channel_ref(x[:check * M].cpu().numpy(), None, h, M, P, twiddles(M))
        assert np.array_equal(bits(out[:, :check].cpu().numpy()), bits(want)), tag
        m.streams_reset(M)
        modems[tag], rows[tag] = m, out

        def push(m=m, T=T, out=out):
            m._check(m.L.qpsk_channel_push(m.h, P_(x), T, P_(out), 0))

        o = m._stream_out(False)

        def streams(m=m, out=out, o=o):
            m._check(m.L.qpsk_streams_rx_cplx(m.h, P_(out), P_(o["sym"]), P_(o["freq"]), P_(o["phase"]), None, P_(o["index"])))

        legs["push " + tag], legs["streams " + tag] = push, streams
        streams()
        kernels["streams " + tag] = m.last_kernel()
        m.sync()
    one = qpsk_amd.Modem(frame_size=2048)
    one.channel_reset(4096, 8, qpsk_amd.channel_prototype(4096, 8), chan=[1234])
    row = torch.zeros((1, 2048, 2), dtype=torch.float32, device=dev)
    modems["x1"] = one

    def push_one():
        one._check(one.L.qpsk_channel_push(one.h, P_(x), 2048, P_(row), 0))

    push_one()
    one.sync()
    assert torch.equal(row[0], rows["4096"][1234])
    legs["push 4096 x1"], kernels["push 4096 x1"] = push_one, one.last_kernel()
    legs["copy"] = lambda: dst.copy_(x)
    kernels["copy"] = "device-to-device copy"

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
    nbytes = x.numel() * 4
    ratio = {"push %s / copy" % t: med["push " + t] / med["copy"] for t in shapes}
    ratio.update({"push %s / streams %s" % (t, t): med["push " + t] / med["streams " + t] for t in shapes})
    ratio["push 4096 x1 / push 4096"] = med["push 4096 x1"] / med["push 4096"]
    gbs = {name: 2 * nbytes / med[name] / 1e6 for name in ("push 4096", "push 64", "copy")}      # read + written
    rec = {"shapes": shapes, "bytes_in": nbytes, "steps": args.steps, "rounds": args.rounds, "ms_per_call": med, "spread_ms": spread,
           "ratios": ratio, "gb_per_s": gbs, "kernels": kernels, "all": res}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("The polyphase channeliser beside its yardsticks -- measurement record (tools/bench_channel.py; DESIGN.md 4.4.18)\n"
                 "MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call, +- = max - min of a leg's rounds.\n"
                 "push 4096: M = 4096, P = 8, T = 2048; push 64: M = 64, P = 16, T = 131072 -- %d bytes in, as many out; copy: that input,\n"
                 "device to device; streams: qpsk_streams_rx_cplx on the rows the push wrote.  GB/s = (bytes in + bytes out) / time.\n"
                 "Not measured: other shapes, hardware counters, the launch floor at small M and short pushes.\n\n"
                 % (args.rounds, args.steps, nbytes))
        for name in legs:
            fh.write("  %-13s %9.4f (+-%.4f)   %-22s [%s]\n" % (name, med[name], spread[name], "%.0f GB/s" % gbs[name] if name in gbs else "",
                                                             kernels[name]))
        fh.write("\n")
        for name, v in ratio.items():
            fh.write("  %-28s %.4f\n" % (name, v))
        fh.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
