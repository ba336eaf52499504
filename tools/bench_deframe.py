"""Time qpsk_deframer_push at 4096 streams x 2048 symbols next to one qpsk_streams_rx_pcm block of the same shape (fs 19200, rs 2400,
16384-sample blocks: 2048 symbols per stream), in one process, with events as bench.py times its steps; rounds interleaved.

  block    qpsk_streams_rx_pcm, costas_frame[] requested (what the deframer's costas input reads)
  data     qpsk_deframer_push on data rows (4096 x 2048 uint8)
  costas   qpsk_deframer_push on that block's d_costas (4096 x 2048 x 8 bytes: the data rule on load)

The rows are random dibits with a 64-dibit word (min_score 56), so pushes find no packet: the cost of the hunt itself.  Prints one JSON
line.  Usage: python tools/bench_deframe.py [--streams 4096] [--steps 50] [--rounds 5]
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
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import qpsk_amd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    S, fs, rs, L = args.streams, 19200.0, 2400.0, 16384
    m = qpsk_amd.Modem(fs=fs, rs=rs, frame_size=L)
    N = m.nsym
    m.streams_reset(S, 1500.0)
    g = torch.Generator(device=dev).manual_seed(1)
    pcm = (torch.randn((S, L), device=dev, generator=g) * 6000).to(torch.int16)
    sym = torch.empty((S, N), dtype=torch.uint8, device=dev)
    costas = torch.empty((S, N, 2), dtype=torch.float32, device=dev)
    freq = torch.empty(S, dtype=torch.float32, device=dev)
    phase = torch.empty(S, dtype=torch.float32, device=dev)
    index = torch.empty(S, dtype=torch.int32, device=dev)
    data = torch.randint(0, 4, (S, N), dtype=torch.uint8, device=dev, generator=g)
    nsync, nbytes, M = 64, 64, 8
    m.deframer_reset(S, np.random.default_rng(3).integers(0, 4, nsync), nbytes, 56, max_packets=M)
    count = torch.empty(S, dtype=torch.int32, device=dev)
    out = torch.empty((S, M, nbytes + 2), dtype=torch.uint8, device=dev)
    pos = torch.empty((S, M), dtype=torch.int64, device=dev)
    rot = torch.empty((S, M), dtype=torch.int32, device=dev)
    score = torch.empty((S, M), dtype=torch.int32, device=dev)
    ok = torch.empty((S, M), dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def block():
        rc = m.L.qpsk_streams_rx_pcm(m.h, P(pcm), P(sym), P(freq), P(phase), P(costas), P(index))
        if rc:
            m._check(rc)

    block()
    m.sync()

    def push(z, d):
        def fn():
            rc = m.L.qpsk_deframer_push(m.h, z, d, N, P(count), P(out), P(pos), P(rot), P(score), P(ok))
            if rc:
                m._check(rc)
        return fn

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        m.sync()
        return e0.elapsed_time(e1) / steps

    legs = (("block", block), ("data", push(None, P(data))), ("costas", push(P(costas), None)))
    res = {k: [] for k, _ in legs}
    for _ in range(args.rounds):
        for k, fn in legs:
            res[k].append(timed(fn, args.steps))
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({"streams": S, "nsym": N, "nsync": nsync, "nbytes": nbytes, "ms_per_call": med, "all": res,
                      "data_over_block": med["data"] / med["block"], "costas_over_block": med["costas"] / med["block"],
                      "costas_GBps": S * N * 8 / (med["costas"] * 1e-3) / 1e9}))


if __name__ == "__main__":
    main()
