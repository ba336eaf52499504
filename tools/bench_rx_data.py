"""Time the data route at config 2's shape (4096 frames x 16384 samples, offset 6), in one process, with events as bench.py times its
steps; rounds of the legs interleaved so that clock and power drift fall on all alike.

  rx_batch     qpsk_rx_batch on a TIMING_FIXED context (bench.py's step)
  data         qpsk_rx_batch_data, data only (d_sym NULL), the same offsets: rx_lean_kernel with the data rule in its flush
  costas_route the route to the same bytes without it: qpsk_rx_batch_ext with a costas_frame[] dump, the quadrant taken in torch
  sync         qpsk_sync_batch over the data (nsync 64, lag window 256, nout 1024)

Prints one JSON line.  Usage: python tools/bench_rx_data.py [--steps 200] [--rounds 5]
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
    F, L, IX = args.frames, bench.L, 6
    x = bench.tx_frames_gpu(torch, dev, qpsk_amd, F, seed=1)
    m = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=IX)
    N = m.nsym
    sym = torch.empty((F, N), dtype=torch.uint8, device=dev)
    data = torch.empty((F, N), dtype=torch.uint8, device=dev)
    costas = torch.empty((F, N, 2), dtype=torch.float32, device=dev)
    freq = torch.empty(F, dtype=torch.float32, device=dev)
    phase = torch.empty(F, dtype=torch.float32, device=dev)
    idx = torch.full((F,), IX, dtype=torch.int32, device=dev)
    nsync, window, nout = 64, 256, 1024
    sw = (C.c_uint8 * nsync)(*np.random.default_rng(3).integers(0, 4, nsync).tolist())
    out = torch.empty((F, nout), dtype=torch.uint8, device=dev)
    lag = torch.empty(F, dtype=torch.int32, device=dev)
    rot = torch.empty(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def rx_batch():
        m.rx_batch_raw(x, F, sym, freq, phase)

    def data_only():
        rc = m.L.qpsk_rx_batch_data(m.h, P(x), 0, F, P(idx), None, P(data), None, P(freq), P(phase), None, None)
        if rc:
            m._check(rc)

    def costas_route():
        rc = m.L.qpsk_rx_batch_ext(m.h, P(x), 0, F, P(idx), None, P(sym), P(freq), P(phase), P(costas), None, None)
        if rc:
            m._check(rc)
        torch.add((costas[..., 1] < 0).to(torch.uint8) * 2, (costas[..., 0] < 0).to(torch.uint8), out=data)

    def sync():
        rc = m.L.qpsk_sync_batch(m.h, P(data), F, N, sw, nsync, 0, window - 1, nout, P(out), P(lag), P(rot), None)
        if rc:
            m._check(rc)

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

    legs = (("rx_batch", rx_batch), ("data", data_only), ("costas_route", costas_route), ("sync", sync))
    res = {k: [] for k, _ in legs}
    kern = {}
    for _ in range(args.rounds):
        for k, fn in legs:
            res[k].append(timed(fn, args.steps))
            kern[k] = m.last_kernel()
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({"frames": F, "frame_size": L, "index": IX, "ms_per_step": med, "all": res, "kernels": kern,
                      "data_over_rx_batch": med["data"] / med["rx_batch"], "costas_route_over_data": med["costas_route"] / med["data"],
                      "sync": {"nsync": nsync, "window": window, "nout": nout}}))


if __name__ == "__main__":
    main()
