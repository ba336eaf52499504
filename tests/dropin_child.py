"""Child process of tests/test_dropin_gpu.py: the drop-in (include/qpsk_dropin.h) is a process-wide singleton whose failure mode is
abort(), so every run of it gets a process of its own.

    python dropin_child.py IN.npz OUT.npz

IN.npz holds `steps`, a JSON list, and the arrays the steps name; OUT.npz gets what each step observed, under "<step number>.<name>".
  {"op": "configure", "fs":, "rs":, "frame_size":, "center":}   qpsk_dropin_configure() with the other parameters at their defaults
  {"op": "configure_default"}                                   qpsk_dropin_configure() with qpsk_params_default(), centre 1500 Hz
  {"op": "init", "fs":, "rs":}                                  rrc_make(fs, rs, .35f); create_control_loop(TAU / 100, -1, 1), as main() does
  {"op": "blocks", "pcm": key, "frame_size":, "schedule": bool} rx_frame() block after block; with schedule, loopsched.SCHEDULE[k - 1]
                                                                in front of block k.  -> sym, costas, index, hz, state (the 8 getters)
  {"op": "staging", "calls": [[name, n], ...], "mem": key, "x<i>": ...}   rrc_fir / fft / fftn / ifft / ifftn in that order on one
                                                                carried delay line -> y<i>, m<i> (rrc_fir), in<i> (the input afterwards)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from loopsched import BW, SCHEDULE, apply_lib, declare, getters_of      # noqa: E402
from qpsk_amd.lib import Params, lib_path                               # noqa: E402


def main(fin, fout):
    z = np.load(fin)
    steps = json.loads(str(z["steps"]))
    L = C.CDLL(lib_path())
    declare(L)
    L.qpsk_params_default.argtypes = [C.POINTER(Params)]
    L.qpsk_dropin_configure.argtypes = [C.POINTER(Params), C.c_double]
    L.rrc_make.argtypes = [C.c_float] * 3
    L.rrc_make.restype = None
    L.rx_frame.argtypes = [C.c_void_p]
    L.rx_frame.restype = None
    L.rrc_fir.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.rrc_fir.restype = None
    for n in ("fft", "ifft"):
        getattr(L, n).argtypes = [C.c_void_p, C.c_void_p]
        getattr(L, n).restype = None
    for n in ("fftn", "ifftn"):
        getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        getattr(L, n).restype = None
    L.qpsk_dropin_costas_frame.restype = C.POINTER(C.c_float)
    L.qpsk_dropin_symbols.restype = C.POINTER(C.c_uint8)
    L.qpsk_dropin_offset_freq.restype = C.c_float
    L.qpsk_dropin_shutdown.restype = None
    out = {}
    for i, st in enumerate(steps):
        op = st["op"]
        if op in ("configure", "configure_default"):
            p = Params()
            L.qpsk_params_default(C.byref(p))
            center = 1500.0
            if op == "configure":
                p.fs, p.rs, p.frame_size, center = st["fs"], st["rs"], st["frame_size"], st["center"]
            rc = L.qpsk_dropin_configure(C.byref(p), center)
            assert rc == 0, "qpsk_dropin_configure: %d" % rc
        elif op == "init":
            L.rrc_make(st["fs"], st["rs"], 0.35)
            L.create_control_loop(BW, -1.0, 1.0)
        elif op == "blocks":
            pcm, fs = z[st["pcm"]], st["frame_size"]
            obs = dict(sym=[], costas=[], index=[], hz=[], state=[], edited=[])
            for k in range(pcm.size // fs):
                if st["schedule"] and k:
                    apply_lib(L, SCHEDULE[k - 1])
                obs["edited"].append(getters_of(L))
                blk = np.ascontiguousarray(pcm[k * fs:(k + 1) * fs])
                L.rx_frame(blk.ctypes.data_as(C.c_void_p))
                nsym = st["nsym"]
                obs["sym"].append(np.ctypeslib.as_array(L.qpsk_dropin_symbols(), shape=(nsym,)).copy())
                obs["costas"].append(np.ctypeslib.as_array(L.qpsk_dropin_costas_frame(), shape=(nsym, 2)).copy())
                obs["index"].append(L.qpsk_dropin_timing_index())
                obs["hz"].append(np.float32(L.qpsk_dropin_offset_freq()))
                obs["state"].append(getters_of(L))
            for name, v in obs.items():
                out["%d.%s" % (i, name)] = np.array(v)
        elif op == "staging":
            mem = z[st["mem"]].copy()
            for j, (name, n) in enumerate(st["calls"]):
                x = z["%s%d" % (st["x"], j)].copy()
                if name == "rrc_fir":
                    L.rrc_fir(mem.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), n)
                    out["%d.y%d" % (i, j)] = x
                    out["%d.m%d" % (i, j)] = mem.copy()
                else:
                    y = np.full(x.shape, np.nan + 1j * np.nan, np.complex128)
                    args = [x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)] + ([n] if name in ("fftn", "ifftn") else [])
                    getattr(L, name)(*args)
                    out["%d.y%d" % (i, j)] = y
                    out["%d.in%d" % (i, j)] = x
        else:
            raise ValueError(op)
    L.qpsk_dropin_shutdown()
    np.savez(fout, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
