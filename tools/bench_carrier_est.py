"""Time qpsk_carrier_est_batch at config 2's shape (4096 frames x 16384 samples, FS 19200, RS 2400) against one qpsk_rx_batch, in
one process, with events as bench.py times its steps; rounds interleaved so that clock and power drift fall on every leg alike.

  est_<n>      qpsk_carrier_est_batch over samples 128 .. 128 + n - 1 of every frame (seed output only)
  rx           qpsk_rx_batch on a TIMING_FIXED context (fixed_index = bench.py's FIXED_INDEX)
  est_ext      qpsk_carrier_est_batch (n = 1024) then qpsk_rx_batch_ext with its seeds and the fixed offsets

Prints one JSON line.  Usage: python tools/bench_carrier_est.py [--steps 200] [--rounds 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (512, 1024, 2048, 8192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import qpsk_amd
    import bench
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    F, L = args.frames, bench.L
    x = bench.tx_frames_gpu(torch, dev, qpsk_amd, F, seed=1)
    m = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=bench.FIXED_INDEX)
    sym = torch.empty((F, m.nsym), dtype=torch.uint8, device=dev)
    freq = torch.empty(F, dtype=torch.float32, device=dev)
    phase = torch.empty(F, dtype=torch.float32, device=dev)
    seed = torch.empty((F, 2), dtype=torch.float32, device=dev)
    idx = torch.full((F,), bench.FIXED_INDEX, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def est(n):
        def go():
            rc = m.L.qpsk_carrier_est_batch(m.h, P(x), 0, F, 128, n, P(seed), None, None, None)
            if rc:
                m._check(rc)
        return go

    def rx():
        m.rx_batch_raw(x, F, sym, freq, phase)

    def est_ext():
        est(1024)()
        rc = m.L.qpsk_rx_batch_ext(m.h, P(x), 0, F, P(idx), P(seed), P(sym), P(freq), P(phase), None, None, None)
        if rc:
            m._check(rc)

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

    legs = [("est_%d" % n, est(n)) for n in NS] + [("rx", rx), ("est_ext", est_ext)]
    res = {k: [] for k, _ in legs}
    kern = {}
    for _ in range(args.rounds):
        for k, fn in legs:
            res[k].append(timed(fn))
            kern[k] = m.last_kernel()
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({"frames": F, "frame_size": L, "start": 128, "ms_per_call": med, "all": res, "kernels": kern,
                      "est_1024_over_rx": med["est_1024"] / med["rx"]}))


if __name__ == "__main__":
    main()
