"""Time the interleaved calls (INTERLEAVING in include/qpsk_hip.h) next to the calls they extend, in one process, with events as bench.py
times its steps; rounds of the legs interleaved so that clock and power drift fall on all alike, medians.  Rates 1/2 and 3/4, each at
the recommended stride qpsk_ilv_stride(n, n / 16).

  decode   4096 rows x 2054 steps of random int8 soft values (the decoder's time does not depend on the data), d_flip given, bits and info:
             punct      qpsk_viterbi_punct_batch -- of --parent-lib where one is given (the parent commit's build of the library), else
                        this library's, whose punctured kernels are the parent's instruction for instruction
             punct_b    the same leg a second time: its distance from punct is the leg's own run-to-run spread
             ilv        qpsk_viterbi_ilv_batch at the stride
             ilv_s1     qpsk_viterbi_ilv_batch at stride 1: the interleaved kernel, its modular product and its byte loads, on loads that
                        lie where the punctured kernel's do.  ilv_s1 - punct is what the product costs, ilv - ilv_s1 what the scatter costs
           each on the library's own route and, in a second pair of contexts, with QPSK_VITERBI_LDS = 1
  frame    4096 rows of 1 and of 4 packets of 64 bytes, 32-dibit word, exact fit: qpsk_frame_batch (frame), qpsk_frame_batch_ilv (frame_ilv)
  push     qpsk_deframer_push_coded on 4096 streams x 2048 symbols, one 64-byte packet per stream and push (64-dibit word), d_gain given:
           after qpsk_deframer_reset_coded_punct on plain rows (push) and after qpsk_deframer_reset_coded_ilv on interleaved rows (push_ilv)

Prints one JSON line and writes the record to --out (profiles/ilv.txt).
Usage: python tools/bench_ilv.py [--rows 4096] [--steps 30] [--rounds 5] [--parent-lib PATH]
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
RATES = ("1/2", "3/4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=2054)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libqpsk_hip.so: its qpsk_viterbi_punct_batch is the decode's yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ilv.txt"))
    args = ap.parse_args()
    import torch
    import qpsk_amd
    from qpsk_amd.lib import PUNCTURE
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    R, N = args.rows, args.nsteps
    rng = np.random.default_rng(R + N)
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()[:16]      # noqa: E731

    def timed(fn, sync):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        sync()
        return e0.elapsed_time(e1) / args.steps

    def call(fn, h, *a):
        def run():
            rc = fn(h, *a)
            if rc:
                raise RuntimeError("call failed: %d" % rc)
        return run

    legs, syncs, kernels = {}, {}, {}
    keep = []

    # ---- decode
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.qpsk_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        parent.qpsk_viterbi_punct_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        parent.qpsk_ctx_sync.argtypes = [C.c_void_p]
        parent.qpsk_ctx_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        parent.qpsk_ctx_last_kernel.argtypes = [C.c_void_p]
        parent.qpsk_ctx_last_kernel.restype = C.c_char_p
    strides = {}
    for route, lds in (("own", None), ("lds", 1)):
        m = qpsk_amd.Modem()
        m.tune(viterbi_lds=lds)
        keep.append(m)
        ph = None
        if parent is not None:
            ph = C.c_void_p()
            assert parent.qpsk_ctx_create(C.byref(ph), 0, C.byref(m.params), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
            assert parent.qpsk_ctx_set_tuning(ph, b"QPSK_VITERBI_LDS", -1 if lds is None else lds) == 0
        for rate in RATES:
            pat = PUNCTURE[rate]
            ntx = m.punct_ntx(N, pat)
            s = strides[rate] = qpsk_amd.ilv_stride(2 * ntx, 2 * ntx // 16)
            soft = torch.from_numpy(rng.integers(-127, 128, (R, ntx, 2)).astype(np.int8)).to(dev)
            key = torch.from_numpy(rng.integers(0, 4, ntx).astype(np.uint8)).to(dev)
            bits = torch.empty((R, (N + 7) // 8), dtype=torch.uint8, device=dev)
            info = torch.empty((R, 4), dtype=torch.int32, device=dev)
            keep.append((soft, key, bits, info))
            tail = (P(key), 0, P(bits), P(info))
            base = "decode %s %s " % (route, rate)
            for name in ("punct", "punct_b"):
                if parent is not None:
                    legs[base + name] = call(parent.qpsk_viterbi_punct_batch, ph, P(soft), 0, R, N, *pat, *tail)
                    syncs[base + name] = lambda ph=ph: parent.qpsk_ctx_sync(ph)
                    kernels[base + name] = lambda ph=ph: parent.qpsk_ctx_last_kernel(ph).decode()
                else:
                    legs[base + name] = call(m.L.qpsk_viterbi_punct_batch, m.h, P(soft), 0, R, N, *pat, *tail)
            legs[base + "ilv"] = call(m.L.qpsk_viterbi_ilv_batch, m.h, P(soft), 0, R, N, *pat, s, *tail)
            legs[base + "ilv_s1"] = call(m.L.qpsk_viterbi_ilv_batch, m.h, P(soft), 0, R, N, *pat, 1, *tail)
            for name in ("punct", "punct_b", "ilv", "ilv_s1"):
                syncs.setdefault(base + name, m.sync)
                kernels.setdefault(base + name, m.last_kernel)

    # ---- frame
    mf = qpsk_amd.Modem()
    keep.append(mf)
    nbytes, nsync = 64, 32
    word = np.ascontiguousarray(rng.integers(0, 4, nsync).astype(np.uint8))
    for per_row in (1, 4):
        for rate in RATES:
            pat = PUNCTURE[rate]
            plen = qpsk_amd.frame_len(nsync, nbytes, coded=True, puncture=pat)
            s = qpsk_amd.ilv_stride(2 * (plen - nsync), 2 * (plen - nsync) // 16)
            payload = torch.from_numpy(rng.integers(0, 256, (R * per_row, nbytes)).astype(np.uint8)).to(dev)
            out = torch.zeros((R, per_row * plen), dtype=torch.uint8, device=dev)
            crc = torch.zeros(R * per_row, dtype=torch.int16, device=dev)
            keep.append((payload, out, crc))
            base = "frame %d %s " % (per_row, rate)
            head = (P(payload), 0, R, per_row, nbytes, word.ctypes.data_as(C.c_void_p), nsync, 1) + tuple(pat)
            legs[base + "frame"] = call(mf.L.qpsk_frame_batch, mf.h, *head, 0, 0, per_row * plen, P(out), P(crc))
            legs[base + "frame_ilv"] = call(mf.L.qpsk_frame_batch_ilv, mf.h, *head, s, 0, 0, per_row * plen, P(out), P(crc))
            for name in ("frame", "frame_ilv"):
                syncs[base + name] = mf.sync
                kernels[base + name] = mf.last_kernel

    # ---- push: one packet inside every row, the same row pushed again and again (every push completes one packet per stream)
    nsym, wsync, amp = 2048, 64, 0.7
    word64 = np.ascontiguousarray(rng.integers(0, 4, wsync).astype(np.uint8))
    payload = torch.from_numpy(rng.integers(0, 256, (R, nbytes)).astype(np.uint8)).to(dev)
    gain = torch.full((R,), 64.0 / amp, dtype=torch.float32, device=dev)
    for rate in RATES:
        pat = PUNCTURE[rate]
        B = qpsk_amd.frame_len(wsync, nbytes, coded=True, puncture=pat) - wsync
        s = qpsk_amd.ilv_stride(2 * B, 2 * B // 16)
        for name, stride in (("push", None), ("push_ilv", s)):
            m = qpsk_amd.Modem()
            keep.append(m)
            d = m.frame(payload, word64, puncture=pat, lead=100, row_len=nsym, interleave=stride)["dibits"].to(torch.int32)
            z = torch.stack([amp * (1 - 2 * (d & 1)), amp * (1 - 2 * (d >> 1))], dim=-1).to(torch.float32).contiguous()
            m.deframer_reset_coded(R, word64, nbytes, wsync - 8, max_packets=4, puncture=pat, interleave=stride)
            o = m.deframe_coded(z, gain)
            m.sync()
            assert bool((o["count"] == 1).all()) and bool(o["crc_ok"][:, 0].all()), name
            assert torch.equal(o["bytes"][:, 0, :nbytes], payload), name
            keep.append((z, o))
            base = "push %s " % rate
            legs[base + name] = call(m.L.qpsk_deframer_push_coded, m.h, P(z), nsym, P(gain), P(o["count"]), P(o["bytes"]), P(o["pos"]), P(o["rot"]),
                                     P(o["score"]), P(o["crc_ok"]), P(o["info"]))
            syncs[base + name] = m.sync
            kernels[base + name] = m.last_kernel

    res = {k: [] for k in legs}
    names = {}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            res[k].append(timed(fn, syncs[k]))
            names[k] = kernels[k]()
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = {k: float(max(v) - min(v)) for k, v in res.items()}
    rec = {"rows": R, "nsteps": N, "steps": args.steps, "rounds": args.rounds, "strides": strides, "lib_sha256": sha(qpsk_amd.lib_path()),
           "parent_lib_sha256": sha(args.parent_lib) if args.parent_lib else None, "ms_per_call": med, "spread_ms": spread, "kernels": names,
           "all": res, "ratios": {}}
    lines = []
    for route in ("own", "lds"):
        for rate in RATES:
            b = "decode %s %s " % (route, rate)
            own = abs(med[b + "punct_b"] - med[b + "punct"]) + max(spread[b + "punct"], spread[b + "punct_b"])
            r = {"ilv_over_punct": med[b + "ilv"] / med[b + "punct"], "ilv_s1_over_punct": med[b + "ilv_s1"] / med[b + "punct"],
                 "punct_b_over_punct": med[b + "punct_b"] / med[b + "punct"], "punct_own_spread_ms": own,
                 "ilv_minus_punct_ms": med[b + "ilv"] - med[b + "punct"], "product_ms": med[b + "ilv_s1"] - med[b + "punct"],
                 "scatter_ms": med[b + "ilv"] - med[b + "ilv_s1"]}
            rec["ratios"][b.strip()] = r
            lines.append("  decode %-3s rate %s stride %4d   punct %.4f (+-%.4f)  punct again %.4f   ilv %.4f (+-%.4f)   ilv at stride 1 %.4f   "
                         "ilv / punct = %.4f   [%s | %s]" % (route, rate, strides[rate], med[b + "punct"], spread[b + "punct"], med[b + "punct_b"],
                                                             med[b + "ilv"], spread[b + "ilv"], med[b + "ilv_s1"], r["ilv_over_punct"],
                                                             names[b + "punct"], names[b + "ilv"]))
    for per_row in (1, 4):
        for rate in RATES:
            b = "frame %d %s " % (per_row, rate)
            rec["ratios"][b.strip()] = {"frame_ilv_over_frame": med[b + "frame_ilv"] / med[b + "frame"]}
            lines.append("  frame per_row %d rate %s   frame %.4f (+-%.4f)   frame_ilv %.4f (+-%.4f)   frame_ilv / frame = %.4f   [%s]"
                         % (per_row, rate, med[b + "frame"], spread[b + "frame"], med[b + "frame_ilv"], spread[b + "frame_ilv"],
                            med[b + "frame_ilv"] / med[b + "frame"], names[b + "frame_ilv"]))
    for rate in RATES:
        b = "push %s " % rate
        rec["ratios"][b.strip()] = {"push_ilv_over_push": med[b + "push_ilv"] / med[b + "push"]}
        lines.append("  push rate %s   push %.4f (+-%.4f)   push_ilv %.4f (+-%.4f)   push_ilv / push = %.4f   [%s]"
                     % (rate, med[b + "push"], spread[b + "push"], med[b + "push_ilv"], spread[b + "push_ilv"],
                        med[b + "push_ilv"] / med[b + "push"], names[b + "push_ilv"]))
    line = json.dumps(rec)
    print(line)
    with open(args.out, "w") as fh:
        fh.write("The interleaved calls beside the calls they extend -- measurement record (tools/bench_ilv.py; DESIGN.md 4.4.10)\n"
                 "MI355X, one process, events, %d interleaved rounds of %d calls, medians in ms per call, +- = max - min of a leg's rounds.\n"
                 "decode: %d rows x %d steps; punct = qpsk_viterbi_punct_batch of %s; frame: %d rows of 1 / 4 packets of 64 bytes;\n"
                 "push: %d streams x 2048 symbols, one 64-byte packet per stream and push\n\n"
                 % (args.rounds, args.steps, R, N, "the parent commit's library (--parent-lib)" if args.parent_lib else "this library", R, R))
        fh.write("\n".join(lines) + "\n\n" + line + "\n")
    for m in keep:
        if hasattr(m, "close"):
            m.close()


if __name__ == "__main__":
    main()
