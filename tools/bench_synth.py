"""Time the polyphase synthesis bank (qpsk_synth_push) at the channeliser's headline shapes, next to the analysis push of the same shape
(qpsk_channel_push) and to a device-to-device copy of the 64 MiB both read and write.  One process, events as bench.py times its steps,
rounds interleaved, medians: the method of tools/bench_channel.py.

  synth 4096       M = 4096, P = 8, T = 2048, all channels: 64 MiB in, 64 MiB out, synth_transform_kernel<1024> (tile 4) into the scratch
                   of transformed vectors (64 MiB written, read (16 + 7) / 16 times), synth_filter_kernel<8>, polyphase_history_kernel
  synth 64         M = 64, P = 16, T = 131072: the same bytes, synth_transform_kernel<256> (tile 128), synth_filter_kernel<16>
  synth 4096 x1    synth 4096 with ONE channel selected: 16 KiB in; the transform of 4095 zeros and one value, the whole filter
  push 4096 / 64   THE YARDSTICK of each shape: qpsk_channel_push on the same M, P, T
  copy             a device-to-device copy of the 64 MiB

The input is Gaussian noise at unit variance and a Kaiser prototype with the interpolation gain (channel_prototype(M, P, gain=M)); neither
changes what the kernels do.  Before anything is timed a push of each shape is compared with the numpy restatement of
tests/test_synth_cpu.py on its first output times.  No time is a condition here: the record is each leg's ratio to the analysis push and
to the copy.  NOT measured: other shapes, hardware counters, a kernel trace (the split between the three launches), the cost of a push
that grows the scratch, the launch floor at small M and short pushes.  Prints one JSON line and writes the record to --out
(profiles/synth.txt).
Usage: python tools/bench_synth.py [--steps 20] [--rounds 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    from test_channel_cpu import bits, twiddles
    from test_synth_cpu import synth_ref
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    P_ = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    shapes = {"4096": (4096, 8, 2048), "64": (64, 16, 131072)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(2019)
    x = torch.randn((4096 * 2048, 2), generator=gen, dtype=torch.float32, device=dev)      # the rows of every shape, and the analysis push's input
    dst = torch.empty_like(x)
    legs, kernels, modems, outs = {}, {}, {}, {}
    for tag, (M, P, T) in shapes.items():
        m = qpsk_amd.Modem(frame_size=T)
        g = qpsk_amd.channel_prototype(M, P, gain=M)
        m.synth_reset(M, P, g)
        m.channel_reset(M, P, qpsk_amd.channel_prototype(M, P))
        wide = torch.zeros((T * M, 2), dtype=torch.float32, device=dev)
        rows = torch.zeros((M, T, 2), dtype=torch.float32, device=dev)
        m._check(m.L.qpsk_synth_push(m.h, P_(x), 0, T, P_(wide)))
        kernels["synth " + tag] = m.last_kernel()
        m.sync()
        check = 4 * P
        c = x.view(M, T, 2)[:, :check].cpu().numpy()
        want, _ = synth_ref(c, None, None, g, M, P, twiddles(M))
        assert np.array_equal(bits(wide[:check * M].cpu().numpy()), bits(want)), tag
        modems[tag], outs[tag] = m, wide

        def synth(m=m, T=T, wide=wide):
            m._check(m.L.qpsk_synth_push(m.h, P_(x), 0, T, P_(wide)))

        def push(m=m, T=T, rows=rows):
            m._check(m.L.qpsk_channel_push(m.h, P_(x), T, P_(rows), 0))

        legs["synth " + tag], legs["push " + tag] = synth, push
        push()
        kernels["push " + tag] = m.last_kernel()
        m.sync()
    M, P, T = shapes["4096"]
    one = qpsk_amd.Modem(frame_size=T)
    g = qpsk_amd.channel_prototype(M, P, gain=M)
    one.synth_reset(M, P, g, chan=[1234])
    wide1 = torch.zeros((T * M, 2), dtype=torch.float32, device=dev)
    modems["x1"] = one

    def synth_one():
        one._check(one.L.qpsk_synth_push(one.h, P_(x), 0, T, P_(wide1)))

    synth_one()
    one.sync()
    want, _ = synth_ref(x[:4 * P].cpu().numpy()[None], [1234], None, g, M, P, twiddles(M))
    assert np.array_equal(bits(wide1[:4 * P * M].cpu().numpy()), bits(want))
    legs["synth 4096 x1"], kernels["synth 4096 x1"] = synth_one, one.last_kernel()
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
    ratio = {"synth %s / push %s" % (t, t): med["synth " + t] / med["push " + t] for t in shapes}
    ratio.update({"synth %s / copy" % t: med["synth " + t] / med["copy"] for t in shapes})
    ratio.update({"push %s / copy" % t: med["push " + t] / med["copy"] for t in shapes})
    ratio["synth 4096 x1 / synth 4096"] = med["synth 4096 x1"] / med["synth 4096"]
    ratio["synth 4096 x1 / push 4096"] = med["synth 4096 x1"] / med["push 4096"]
    gbs = {name: 2 * nbytes / med[name] / 1e6 for name in legs if not name.endswith("x1")}      # read + written by the caller's buffers
    rec = {"shapes": shapes, "bytes_in": nbytes, "steps": args.steps, "rounds": args.rounds, "ms_per_call": med, "spread_ms": spread,
           "ratios": ratio, "gb_per_s": gbs, "kernels": kernels, "all": res}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("The polyphase synthesis bank beside its yardsticks -- measurement record (tools/bench_synth.py; DESIGN.md 4.4.19)\n"
                 "MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call, +- = max - min of a leg's rounds.\n"
                 "synth / push 4096: M = 4096, P = 8, T = 2048; synth / push 64: M = 64, P = 16, T = 131072 -- %d bytes in, as many out;\n"
                 "synth 4096 x1: one channel selected; copy: those bytes, device to device.  GB/s = (bytes in + bytes out) / time, the\n"
                 "scratch of transformed vectors between the bank's launches not counted.\n"
                 "Not measured: other shapes, hardware counters, a kernel trace, a push that grows the scratch, the launch floor.\n\n"
                 % (args.rounds, args.steps, nbytes))
        for name in legs:
            fh.write("  %-14s %9.4f (+-%.4f)   %-22s [%s]\n" % (name, med[name], spread[name], "%.0f GB/s" % gbs[name] if name in gbs else "",
                                                              kernels[name]))
        fh.write("\n")
        for name, v in ratio.items():
            fh.write("  %-28s %.4f\n" % (name, v))
        fh.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
