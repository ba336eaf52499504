"""Time qpsk_rx_batch_ext against qpsk_rx_batch at config 2's shape (4096 frames x 16384 samples), in one process, with events as
bench.py times its steps; rounds of the two interleaved so that clock and power drift fall on both alike.

  ext          qpsk_rx_batch_ext on a TIMING_FIXED context, per-frame offsets (the FFT estimate's) and per-frame seeds
  fixed        qpsk_rx_batch on the same context (fixed_index = bench.py's FIXED_INDEX)
  config3      qpsk_rx_batch on a TIMING_FFT context: the estimate inside every call (bench.py's config3 key)
  est_once     qpsk_timing_fft_batch once, then N ext calls reusing its offsets: per-call cost over the N calls

Prints one JSON line.  Usage: python tools/bench_rx_ext.py [--steps 200] [--rounds 5] [--reuse 16]
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
    ap.add_argument("--reuse", type=int, default=16, help="ext calls per FFT estimate in the est_once leg")
    args = ap.parse_args()
    import torch
    import qpsk_amd
    import bench
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    F, L = args.frames, bench.L
    x = bench.tx_frames_gpu(torch, dev, qpsk_amd, F, seed=1)
    mf = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=bench.FIXED_INDEX)
    m3 = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FFT)
    sym = torch.empty((F, mf.nsym), dtype=torch.uint8, device=dev)
    freq = torch.empty(F, dtype=torch.float32, device=dev)
    phase = torch.empty(F, dtype=torch.float32, device=dev)
    idx = mf.timing_fft(x)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    seed = torch.empty((F, 2), dtype=torch.float32, device=dev)
    seed[:, 0] = (torch.rand(F, generator=g, device=dev) * 2 - 1) * np.pi
    seed[:, 1] = (torch.rand(F, generator=g, device=dev) * 2 - 1) * 0.01
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def ext():
        rc = mf.L.qpsk_rx_batch_ext(mf.h, P(x), 0, F, P(idx), P(seed), P(sym), P(freq), P(phase), None, None, None)
        if rc:
            mf._check(rc)

    def fixed():
        mf.rx_batch_raw(x, F, sym, freq, phase)

    def config3():
        m3.rx_batch_raw(x, F, sym, freq, phase)

    def est_once():
        mf._check(mf.L.qpsk_timing_fft_batch(mf.h, P(x), F, P(idx), None, None))
        for _ in range(args.reuse):
            ext()

    def timed(fn, steps, per_call=1):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        mf.sync()
        m3.sync()
        return e0.elapsed_time(e1) / (steps * per_call)

    res = {k: [] for k in ("ext", "fixed", "config3", "est_once")}
    kern = {}
    for _ in range(args.rounds):
        res["fixed"].append(timed(fixed, args.steps)); kern["fixed"] = mf.last_kernel()
        res["ext"].append(timed(ext, args.steps)); kern["ext"] = mf.last_kernel()
        res["config3"].append(timed(config3, args.steps)); kern["config3"] = m3.last_kernel()
        res["est_once"].append(timed(est_once, max(1, args.steps // args.reuse), args.reuse))
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({"frames": F, "frame_size": L, "ms_per_step": med, "all": res, "kernels": kern,
                      "ext_over_fixed": med["ext"] / med["fixed"], "est_once_over_config3": med["est_once"] / med["config3"],
                      "reuse": args.reuse}))


if __name__ == "__main__":
    main()
