"""Time qpsk_soft_batch on the costas_frame[] of config 2's batch (rows of 2048 symbols) next to the receive call that produces it, in
one process, with events as bench.py times its steps; rounds of the legs interleaved so that clock and power drift fall on all alike.

  rx        qpsk_rx_batch_ext with d_costas requested (the yardstick: what a caller who wants soft decisions runs anyway)
  soft      qpsk_soft_batch, soft output (skip 256, the whole row) and quality together: soft_onepass_kernel, each row read once
  quality   qpsk_soft_batch, quality only: soft_sums_kernel
  apply     qpsk_soft_batch, soft output only from the caller's d_gain_in: soft_apply_kernel, nothing summed

at 4096 and 8192 rows.  Bytes are the algorithm's: 8 per symbol read, 2 per symbol written (soft), 16 per row (quality); the share is
against the 8 TB/s HBM figure the project uses.  Prints one JSON line.  Usage: python tools/bench_soft.py [--steps 200] [--rounds 5]

  --counter-pass K   no timing: each soft leg K times at --rows rows, then exit -- the child of a rocprofv3 --pmc FETCH_SIZE (or
                     WRITE_SIZE) run of its own, to read each kernel's memory traffic per launch
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096, help="rows of the counter pass")
    ap.add_argument("--counter-pass", type=int, default=0)
    args = ap.parse_args()
    import torch
    import qpsk_amd
    import bench
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L, SKIP = bench.L, 256
    m = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=bench.FIXED_INDEX)
    N = m.nsym
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def legs_for(F):
        x = bench.tx_frames_gpu(torch, dev, qpsk_amd, F, seed=1)
        sym = torch.empty((F, N), dtype=torch.uint8, device=dev)
        freq = torch.empty(F, dtype=torch.float32, device=dev)
        phase = torch.empty(F, dtype=torch.float32, device=dev)
        costas = torch.empty((F, N, 2), dtype=torch.float32, device=dev)
        soft = torch.empty((F, N, 2), dtype=torch.int8, device=dev)
        quality = torch.empty((F, 4), dtype=torch.float32, device=dev)
        gain = torch.full((F,), 45.0, dtype=torch.float32, device=dev)
        keep = (x, sym, freq, phase, costas, soft, quality, gain)

        def call(fn, *a):
            def run():
                rc = fn(m.h, *a)
                if rc:
                    m._check(rc)
            return run

        rx = call(m.L.qpsk_rx_batch_ext, P(x), 0, F, None, None, P(sym), P(freq), P(phase), P(costas), None, None)
        both = call(m.L.qpsk_soft_batch, P(costas), 0, F, N, SKIP, 0, 64.0, None, None, None, 0, N, P(soft), P(quality), None)
        qual = call(m.L.qpsk_soft_batch, P(costas), 0, F, N, SKIP, 0, 64.0, None, None, None, 0, 0, None, P(quality), None)
        apply_ = call(m.L.qpsk_soft_batch, P(costas), 0, F, N, SKIP, 0, 64.0, P(gain), None, None, 0, N, P(soft), None, None)
        rx()
        m.sync()
        nbytes = {"soft": F * N * 10 + F * 16, "quality": F * N * 8 + F * 16, "apply": F * N * 10 + F * 4}
        return {"rx": rx, "soft": both, "quality": qual, "apply": apply_}, nbytes, keep

    if args.counter_pass:
        legs, _, keep = legs_for(args.rows)
        for k in ("soft", "quality", "apply"):
            for _ in range(args.counter_pass):
                legs[k]()
            m.sync()
        return

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

    out = {"nsym": N, "skip": SKIP, "lib_sha256": hashlib.sha256(open(qpsk_amd.lib_path(), "rb").read()).hexdigest()[:16], "rows": {}}
    for F in (4096, 8192):
        legs, nbytes, keep = legs_for(F)
        res, kern = {k: [] for k in legs}, {}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                res[k].append(timed(fn, args.steps))
                kern[k] = m.last_kernel()
        med = {k: float(np.median(v)) for k, v in res.items()}
        out["rows"][F] = {"ms_per_call": med, "all": res, "kernels": kern,
                          "TBps": {k: nbytes[k] / (med[k] * 1e-3) / 1e12 for k in nbytes},
                          "share_of_8TBps": {k: nbytes[k] / (med[k] * 1e-3) / HBM_BYTES_PER_S for k in nbytes},
                          "soft_over_rx": med["soft"] / med["rx"], "quality_over_rx": med["quality"] / med["rx"]}
        del legs, keep
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
