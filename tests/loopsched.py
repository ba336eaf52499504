"""The loop's control surface used between blocks: one schedule of costas_loop.h calls, and the same calls applied to the three
things that answer to them -- the reference (oracle/_ref, or its record), the oracle's Costas struct, the drop-in's singletons.

Shared by tests/test_oracle_vs_ref.py (which pins the oracle's side of it to the reference), tests/test_dropin_cpu.py,
tests/test_dropin_gpu.py and its child process tests/dropin_child.py.  numpy + ctypes only.
"""
import ctypes as C

import numpy as np

from oracle.pyoracle import TAU

f32 = np.float32
BW = f32(TAU / 100.0)
STATE = ("phase", "freq", "max_freq", "min_freq", "damping", "loop_bw", "alpha", "beta")      # ref_costas_state's order
GETTERS = ("get_phase", "get_frequency", "get_max_freq", "get_min_freq", "get_damping_factor", "get_loop_bandwidth", "get_alpha",
           "get_beta")                                                                      # the same order
SETTERS = ("set_loop_bandwidth", "set_damping_factor", "set_alpha", "set_beta", "set_frequency", "set_phase", "set_max_freq",
           "set_min_freq")
NOARG = ("update_gains", "phase_wrap", "frequency_limit")
DAMPING = f32(np.sqrt(f32(2.0))) / f32(2.0)      # sqrtf(2.0f) / 2.0f (costas_loop.c:39)

# One entry per block boundary: the calls a host program makes between two rx_frame() calls.
SCHEDULE = [
    [],
    [],                                                     # gains unchanged twice: qpsk_ctx_set_loop's early return
    [("set_phase", 20.0)],
    [("set_frequency", 99.0)],                              # clamps to max_freq
    [("set_max_freq", 0.01), ("set_min_freq", -0.005)],     # asymmetric; a 50 Hz offset is 0.13 rad/symbol: the clamp acts at every step
    [],                                                     # the limits persist
    [("set_min_freq", -1.0), ("set_max_freq", 1.0), ("set_loop_bandwidth", f32(TAU / 50.0))],
    [("set_damping_factor", 1.0)],
    [("set_alpha", 0.2), ("set_beta", 0.0)],
    [("set_alpha", 0.0), ("set_beta", 0.0)],                # both zero: the loop coasts on freq
    [],                                                     # still both zero
    [("create_control_loop", f32(TAU / 100.0), -1.0, 1.0)],
    [("advance_loop", 0.3), ("phase_wrap",), ("frequency_limit",)],
    [("set_phase", -0.0), ("set_frequency", -0.0)],
]
NBLOCKS = len(SCHEDULE) + 1      # one untouched block in front

# The scalar calls test_costas_scalar_api_matches_reference leaves out (dead range checks included), run after a
# create_control_loop(bw, lo, hi): limits moved and a frequency beyond either, phases at +-float32(2 pi) (the wrap's comparison is
# strict and against the DOUBLE 2 pi), signed zeros, far phases, update_gains() on its own after set_alpha().
# No infinite phase and none near 2^27 rad: the reference's phase_wrap() would not return.
TWO_PI_F = float(f32(TAU))
SETTER_LIST = [
    ("set_alpha", 7.0), ("set_beta", -3.0), ("set_loop_bandwidth", -0.1), ("set_damping_factor", -1.0),
    ("set_frequency", 99.0), ("set_frequency", -99.0), ("set_phase", 20.0), ("set_phase", -20.0),
    ("set_max_freq", 0.25), ("set_frequency", 0.3), ("set_frequency", 0.25), ("set_min_freq", -0.125), ("set_frequency", -0.2),
    ("set_frequency", -0.125), ("set_max_freq", -0.5), ("set_frequency", 0.0), ("set_min_freq", 0.5), ("set_frequency", 0.0),
    ("set_max_freq", 1.0), ("set_min_freq", -1.0), ("frequency_limit",),
    ("set_phase", TWO_PI_F), ("set_phase", -TWO_PI_F), ("set_phase", 0.0), ("set_phase", -0.0), ("set_phase", 1e6), ("set_phase", -1e6),
    ("set_frequency", -0.0), ("set_frequency", 0.0),
    ("set_loop_bandwidth", 0.05), ("set_alpha", 0.5), ("update_gains",), ("set_damping_factor", 0.5), ("set_beta", 0.125),
    ("update_gains",), ("advance_loop", 2.5), ("phase_wrap",), ("frequency_limit",),
]
TRIPLES = [(BW, -1.0, 1.0), (f32(TAU / 200), -0.2, 0.3), (f32(0.5), -5.0, 5.0)]      # of test_costas_scalar_api_matches_reference


def declare(lib):
    """argument and result types of the costas_loop.h names on a ctypes library (the drop-in, or oracle/_ref)"""
    for n in SETTERS + ("advance_loop",):
        getattr(lib, n).argtypes = [C.c_float]
        getattr(lib, n).restype = None
    for n in NOARG:
        getattr(lib, n).argtypes = []
        getattr(lib, n).restype = None
    lib.create_control_loop.argtypes = [C.c_float] * 3
    lib.create_control_loop.restype = None
    for n in GETTERS:
        getattr(lib, n).argtypes = []
        getattr(lib, n).restype = C.c_float


def apply_lib(lib, ops):
    """the calls by their own names: the reference's library (or its record's proxy), the drop-in"""
    for op in ops:
        getattr(lib, op[0])(*[float(a) for a in op[1:]])


def apply_oracle(orc, c, ops):
    """the same calls on the oracle's Costas struct c through its qo_ functions; set_max_freq / set_min_freq, which have none, are
    assignments, and create_control_loop() is the reference's sequence of setters on the EXISTING struct (costas_loop.c:31-42:
    set_frequency(0) there is clamped by the limits of before) -- qo_costas_create() would start from a fresh process's zeros"""
    L, p = orc.lib, C.byref(c)
    for op in ops:
        name, args = op[0], [float(a) for a in op[1:]]
        if name == "set_max_freq":
            c.max_freq = args[0]
        elif name == "set_min_freq":
            c.min_freq = args[0]
        elif name == "create_control_loop":
            L.qo_set_phase(p, 0.0)
            L.qo_set_frequency(p, 0.0)
            c.max_freq = args[2]
            c.min_freq = args[1]
            L.qo_set_damping_factor(p, float(DAMPING))
            L.qo_set_loop_bandwidth(p, args[0])
        else:
            getattr(L, "qo_" + name)(p, *args)


def state_of(c):
    """the oracle's Costas struct in ref_costas_state's order"""
    return np.array([getattr(c, n) for n in STATE], f32)


def getters_of(lib):
    """the eight getters of a declare()d library in the same order"""
    return np.array([getattr(lib, n)() for n in GETTERS], f32)


def detector_grid():
    """(n, 2) float32 (re, im) pairs for phase_detector() and the slicer: signed zeros, denormals, +-1, +-FLT_MAX, NaN, the four
    diagonals |re| == |im| at several magnitudes (there the slicer's difference re k - im k is an exact zero) and 3000 random pairs"""
    fmax, den = np.finfo(f32).max, f32(1e-42)
    edge = [0.0, -0.0, den, -den, 1.0, -1.0, fmax, -fmax, float("nan")]
    pts = [(a, b) for a in edge for b in edge]
    for mag in (den, f32(1e-20), f32(0.3), f32(0.70710677), 1.0, f32(3.0), f32(1e20), fmax):
        pts += [(mag, mag), (mag, -mag), (-mag, mag), (-mag, -mag)]
    rng = np.random.default_rng(12)
    rnd = rng.standard_normal((3000, 2)) * np.exp(rng.uniform(-30.0, 30.0, (3000, 1)))
    return np.concatenate([np.array(pts, f32), rnd.astype(f32)])


def oracle_detector(orc, grid):
    """-> (qo_phase_detector as float32 (n,), the oracle's slicer as uint8 (n,): (bits[1] << 1) | bits[0])"""
    e = np.array([orc.lib.qo_phase_detector(float(re), float(im)) for re, im in grid], f32)
    s = np.array([orc.lib.qo_demod(float(re), float(im)) for re, im in grid], np.uint8)
    return e, s


def same_with_nans(a, b):
    """bit-equal where neither is a NaN; NaN where the other is (a NaN's sign and payload depend on operand order)"""
    a, b = np.asarray(a, f32).ravel(), np.asarray(b, f32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def stimulus(orc, fs, rs, frame_size, center_hz, nblocks=NBLOCKS, seed=31):
    """nblocks blocks of PCM from the oracle's transmitter at centre + 50 Hz, with mild noise -> int16 (nblocks * frame_size,)"""
    nsym = nblocks * (frame_size // int(fs / rs))
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=2 * nsym).astype(np.int32)
    tx = orc.tx(fs, rs, f32(.35), center_hz + 50.0)
    pcm = np.concatenate([tx.symbols(bits[2 * k:2 * min(k + 256, nsym)]) for k in range(0, nsym, 256)]).astype(np.float64)
    pcm += 0.03 * np.sqrt(np.mean(pcm ** 2)) * rng.standard_normal(pcm.size)
    return np.clip(np.rint(pcm), -32768, 32767).astype(np.int16)


def oracle_schedule(orc, fs, rs, frame_size, center_hz, pcm, mixer=None):
    """The schedule on an oracle modem (shipped loop: TAU / 100, -1, 1): the first block untouched, then SCHEDULE[i] applied in front of
    block i + 1.  -> per block dict(sym, costas, index, hz, state (8,), gains (alpha + beta in force), reach max(|re| + |im|),
    limit max(|min_freq|, |max_freq|) in force)"""
    m = orc.modem(fs, rs, frame_size, loop_bw=BW)
    if mixer is None:
        m.set_mixer_hz(center_hz)
    else:
        m.set_mixer(mixer)
    out = []
    for k in range(pcm.size // frame_size):
        if k:
            apply_oracle(orc, m.s.loop, SCHEDULE[k - 1])
        force = dict(gains=float(m.s.loop.alpha) + float(m.s.loop.beta), limit=max(abs(float(m.s.loop.min_freq)), abs(float(m.s.loop.max_freq))))
        m.rx_pcm(pcm[k * frame_size:(k + 1) * frame_size])
        z = m.costas_frame.astype(np.float64)
        out.append(dict(sym=m.symbols, costas=m.costas_frame, index=m.index, hz=m.offset_hz, state=state_of(m.s.loop),
                        reach=float(np.max(np.abs(z[:, 0]) + np.abs(z[:, 1]))), decimated=m.decimated, **force))
    return out
