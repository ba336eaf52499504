"""Time qpsk_viterbi_batch beside the chain that feeds it -- qpsk_rx_batch_ext with d_costas and qpsk_soft_batch of the same shape -- in one
process, with events as bench.py times its steps; rounds of the legs interleaved so that clock and power drift fall on all alike.

  rx        qpsk_rx_batch_ext with d_costas requested (frame_size = 8 x the row's symbols)
  soft      qpsk_soft_batch, soft output over the whole row and quality together
  viterbi   qpsk_viterbi_batch on that soft output (d_flip = the scrambler's keystream, bits and info), the library's own route
  vit_lds / vit_scratch   the same with QPSK_VITERBI_LDS = 1 / 0, where the row fits the LDS route (the route is part of the record)
  forward   (with --profile-lib) the measurement build's flag that stops after the forward pass; and one call per shape with the cycle
            flag: the shader cycles of the forward pass and of the trace-back per wave, median over rows, divided by the steps

  viterbi_punct / vit_punct_lds / vit_punct_scratch   (with --puncture RATE) qpsk_viterbi_punct_batch on the SAME number of trellis steps: the
            first ntx symbols of the same soft rows (row_pitch = the row's symbols) are taken as what was transmitted, so the punctured and
            the rate-1/2 call do the same steps and differ in the loader alone; same process, same interleaved rounds.  The record, with
            the ratios punctured / rate 1/2 per route, also goes to --out (default profiles/viterbi_punct.txt)

Shapes: 4096 x 2054 and 8192 x 2054 steps off rows of 2054 symbols of a 2054-symbol frame's costas_frame[]; 384 x 131072 off config 5's
row.  The soft values are the receive chain's own (random payload symbols: the decoder's time does not depend on whether the row is a
codeword, every step does the same work).  Prints one JSON line.
Usage: python tools/bench_viterbi.py [--steps 50] [--rounds 5] [--profile-lib qpsk_amd/libqpsk_hip_vprof.so] [--shapes 4096x2054,...]
                                     [--puncture 3/4 [--out profiles/viterbi_punct.txt]]
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
FORWARD_ONLY, CYCLES = 0x100, 0x200      # kernels.h, VITERBI_PROFILE_*: the measurement build only


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="4096x2054,8192x2054,384x131072")
    ap.add_argument("--profile-lib", default=None, help="the measurement build (make -C qpsk_amd/csrc viterbi_profile)")
    ap.add_argument("--puncture", default=None, metavar="RATE", help="also time qpsk_viterbi_punct_batch at this rate (a key of qpsk_amd.PUNCTURE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi_punct.txt"), help="with --puncture: where the record is written")
    args = ap.parse_args()
    import torch
    import qpsk_amd
    import bench
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    prof = None
    if args.profile_lib:
        prof = C.CDLL(os.path.abspath(args.profile_lib))
        prof.qpsk_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        prof.qpsk_viterbi_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        prof.qpsk_ctx_sync.argtypes = [C.c_void_p]
        prof.qpsk_ctx_destroy.argtypes = [C.c_void_p]
        prof.qpsk_ctx_destroy.restype = None
        prof.qpsk_ctx_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        prof.qpsk_ctx_last_kernel.argtypes = [C.c_void_p]
        prof.qpsk_ctx_last_kernel.restype = C.c_char_p

    def timed(fn, steps, sync):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        sync()
        return e0.elapsed_time(e1) / steps

    out = {"lib_sha256": hashlib.sha256(open(qpsk_amd.lib_path(), "rb").read()).hexdigest()[:16], "shapes": {}}
    for shape in args.shapes.split(","):
        R, N = (int(v) for v in shape.split("x"))
        L = 8 * N
        m = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=bench.FIXED_INDEX)
        assert m.nsym == N
        rng = np.random.default_rng(R + N)
        x = torch.from_numpy(rng.standard_normal((min(R, 64), L, 2)).astype(np.float32)).to(dev)
        x = x.repeat((R + x.shape[0] - 1) // x.shape[0], 1, 1)[:R].contiguous()
        x *= 1.0 + 0.01 * torch.arange(R, device=dev, dtype=torch.float32)[:, None, None] / R      # rows differ
        sym = torch.empty((R, N), dtype=torch.uint8, device=dev)
        freq = torch.empty(R, dtype=torch.float32, device=dev)
        phase = torch.empty(R, dtype=torch.float32, device=dev)
        costas = torch.empty((R, N, 2), dtype=torch.float32, device=dev)
        soft = torch.empty((R, N, 2), dtype=torch.int8, device=dev)
        quality = torch.empty((R, 4), dtype=torch.float32, device=dev)
        key = m.scramble(torch.zeros((1, N), dtype=torch.uint8, device=dev))[0].contiguous()
        bits = torch.empty((R, (N + 7) // 8), dtype=torch.uint8, device=dev)
        info = torch.empty((R, 4), dtype=torch.int32, device=dev)

        def call(fn, h, *a):
            def run():
                rc = fn(h, *a)
                if rc:
                    raise RuntimeError("call failed: %d" % rc)
            return run

        vit_args = (P(soft), 0, R, N, P(key), 0, P(bits), P(info))
        legs = {"rx": call(m.L.qpsk_rx_batch_ext, m.h, P(x), 0, R, None, None, P(sym), P(freq), P(phase), P(costas), None, None),
                "soft": call(m.L.qpsk_soft_batch, m.h, P(costas), 0, R, N, 0, 0, 64.0, None, None, None, 0, N, P(soft), P(quality), None),
                "viterbi": call(m.L.qpsk_viterbi_batch, m.h, *vit_args)}
        syncs = {k: m.sync for k in legs}
        routes, namers = {}, {"viterbi": m.last_kernel}
        extra = []
        if 8 * ((N + 63) // 64 * 64) <= 65536:
            for name, v in (("vit_lds", 1), ("vit_scratch", 0)):
                mm = qpsk_amd.Modem(fs=bench.FS, rs=bench.RS, frame_size=L, timing_mode=qpsk_amd.TIMING_FIXED, fixed_index=bench.FIXED_INDEX)
                mm.tune(viterbi_lds=v)
                extra.append(mm)
                legs[name] = call(mm.L.qpsk_viterbi_batch, mm.h, *vit_args)
                syncs[name] = mm.sync
                namers[name] = mm.last_kernel
        ph = None
        if prof is not None:
            ph = C.c_void_p()
            assert prof.qpsk_ctx_create(C.byref(ph), 0, C.byref(m.params), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
            legs["forward"] = call(prof.qpsk_viterbi_batch, ph, P(soft), 0, R, N, P(key), FORWARD_ONLY, P(bits), P(info))
            legs["viterbi_profile_build"] = call(prof.qpsk_viterbi_batch, ph, *vit_args)
            syncs["forward"] = syncs["viterbi_profile_build"] = lambda: prof.qpsk_ctx_sync(ph)
            namers["viterbi_profile_build"] = lambda: prof.qpsk_ctx_last_kernel(ph).decode()
        if args.puncture:
            pat = qpsk_amd.PUNCTURE[args.puncture]
            ntx = m.punct_ntx(N, pat)
            punct_args = (P(soft), N, R, N) + tuple(pat) + (P(key), 0, P(bits), P(info))
            for name, mm in [("viterbi_punct", m)] + [(n.replace("vit_", "vit_punct_"), e) for n, e in zip(("vit_lds", "vit_scratch"), extra)]:
                legs[name] = call(mm.L.qpsk_viterbi_punct_batch, mm.h, *punct_args)
                syncs[name] = mm.sync
                namers[name] = mm.last_kernel
        legs["rx"]()
        legs["soft"]()
        m.sync()
        steps = max(3, args.steps // 8) if N > 8192 else args.steps
        res = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                res[k].append(timed(fn, steps, syncs[k]))
                if k in namers:
                    routes[k] = namers[k]()
        med = {k: float(np.median(v)) for k, v in res.items()}
        rec = {"ms_per_call": med, "min_ms": {k: float(np.min(v)) for k, v in res.items()}, "all": res, "routes": routes,
               "viterbi_over_rx": med["viterbi"] / med["rx"], "viterbi_over_rx_plus_soft": med["viterbi"] / (med["rx"] + med["soft"]),
               "decoded_Mbit_per_s": R * N / (med["viterbi"] * 1e-3) / 1e6}
        if args.puncture:
            pairs = [("viterbi_punct", "viterbi"), ("vit_punct_lds", "vit_lds"), ("vit_punct_scratch", "vit_scratch")]
            rec["puncture"] = {"rate": args.puncture, "pattern": list(pat), "nsteps": N, "ntx": ntx,
                               "punct_over_half": {a: med[a] / med[b] for a, b in pairs if a in med}}
        if prof is not None:
            rec["traceback_ms_by_difference"] = med["viterbi_profile_build"] - med["forward"]
            assert prof.qpsk_viterbi_batch(ph, P(soft), 0, R, N, P(key), CYCLES, P(bits), P(info)) == 0
            prof.qpsk_ctx_sync(ph)
            cyc = info.cpu().numpy()
            rec["cycles_per_step_per_wave"] = {"forward": float(np.median(cyc[:, 1])) / N, "traceback": float(np.median(cyc[:, 2])) / N,
                                               "note": "shader cycles of one wave among the waves resident beside it, median over rows"}
            prof.qpsk_ctx_destroy(ph)
        out["shapes"][shape] = rec
        for mm in extra:
            mm.close()
        m.close()
        del legs, x, costas, soft, bits, info, sym
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.puncture:
        with open(args.out, "w") as f:
            f.write("qpsk_viterbi_punct_batch beside qpsk_viterbi_batch -- measurement record (tools/bench_viterbi.py --puncture %s; DESIGN.md 4.4.8)\n"
                    "ms per call, medians of %d interleaved rounds of %d calls; the punctured call runs the same trellis steps on the first ntx\n"
                    "symbols of the same soft rows\n\n" % (args.puncture, args.rounds, args.steps))
            for shape, rec in out["shapes"].items():
                med, pu = rec["ms_per_call"], rec["puncture"]
                f.write("%s steps, rate %s (ntx %d)\n" % (shape, pu["rate"], pu["ntx"]))
                for a, ratio in pu["punct_over_half"].items():
                    b = {"viterbi_punct": "viterbi", "vit_punct_lds": "vit_lds", "vit_punct_scratch": "vit_scratch"}[a]
                    f.write("  %-18s %9.4f ms (%s)   %-12s %9.4f ms (%s)   punctured / rate 1/2 = %.4f\n"
                            % (a, med[a], rec["routes"].get(a, "?"), b, med[b], rec["routes"].get(b, "?"), ratio))
            f.write("\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
