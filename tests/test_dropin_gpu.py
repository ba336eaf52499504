"""The drop-in layer (include/qpsk_dropin.h, qpsk_amd/csrc/dropin.c) on the GPU, bit for bit against the oracle:
  * rx_frame() with the loop's control surface used between blocks (loopsched.SCHEDULE) -- per block qpsk_ctx_set_loop (gains cached,
    uploaded when they change, alpha == beta == 0 special), the limits as kernel arguments, the state in and out through
    qpsk_streams_rx_pcm_host -- at the shipped configuration and, through qpsk_dropin_configure(), at CYCLES = 8;
  * qpsk_dropin_configure() there and back, with the golden recordings replayed on either side;
  * rrc_fir() / fft() / fftn() / ifft() / ifftn() at sizes that make grow() reallocate the staging they share.
The oracle's side of the schedule is pinned to the reference by tests/test_oracle_vs_ref.py.  The drop-in is a process-wide singleton
that aborts on failure: every run is a child process (tests/dropin_child.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden
from loopsched import NBLOCKS, SCHEDULE, oracle_schedule, stimulus
from oracle.pyoracle import TAU
from rxerrors import LIM
from sigutil import bits_equal

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_child.py")
CENTER = 1500.0
CONFIGS = {"shipped": (9600.0, 2400.0, 512), "c1small": (19200.0, 2400.0, 1024)}


def run_child(tmp_path, steps, arrays):
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, steps=np.array(json.dumps(steps)), **arrays)
    r = subprocess.run([sys.executable, CHILD, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "child exit %d\n%s\n%s" % (r.returncode, r.stdout, r.stderr)
    return np.load(fout)


def assert_clean(want):
    """the clean condition of tests/rxerrors.py for every block, with the gains and limits in force for it: no step of a correct
    library can reach the bounded wrap's limit, so no block can be flagged and the test provokes nothing (a condition on the fixture)"""
    for k, w in enumerate(want):
        assert w["gains"] * w["reach"] + TAU + w["limit"] < 0.9 * LIM, (k, w["gains"], w["reach"], w["limit"])


def assert_golden(o, i, g):
    """the golden recording's own blocks, as test_dropin_reference_signatures_golden asserts them"""
    n = g["sym"].shape[0]
    assert o["%d.sym" % i].shape[0] == n
    for k in range(n):
        assert bits_equal(o["%d.sym" % i][k], g["sym"][k]) and bits_equal(o["%d.costas" % i][k], g["costas"][k]), k
        assert o["%d.state" % i][k][0] == g["phase"][k] and o["%d.state" % i][k][1] == g["freq"][k], k
        assert o["%d.hz" % i][k] == g["hz"][k] and o["%d.index" % i][k] == g["index"][k], k


@pytest.mark.parametrize("name", ["shipped", "c1small"])
def test_rx_frame_with_the_control_surface_between_blocks(oracle, tmp_path, name):
    fs, rs, L = CONFIGS[name]
    nsym = L // int(fs / rs)
    pcm = stimulus(oracle, fs, rs, L, CENTER)
    assert pcm.size == NBLOCKS * L and NBLOCKS >= 14
    want = oracle_schedule(oracle, fs, rs, L, CENTER, pcm)
    assert_clean(want)
    blocks = dict(op="blocks", pcm="pcm", frame_size=L, nsym=nsym, schedule=True)
    if name == "shipped":       # the shipped values apply without qpsk_dropin_configure()
        steps, arrays, at = [dict(op="init", fs=fs, rs=rs), blocks], dict(pcm=pcm), 1
    else:                       # configured; the golden recording first, the schedule on a fresh configuration, then back to the defaults
        gc, gs = golden("stream_pcm_c1small.npz"), golden("stream_pcm_shipped.npz")
        assert (float(gc["fs"]), float(gc["rs"]), int(gc["frame_size"])) == (fs, rs, L)
        conf = dict(op="configure", fs=fs, rs=rs, frame_size=L, center=CENTER)
        steps = [conf, dict(op="init", fs=fs, rs=rs), dict(op="blocks", pcm="gc", frame_size=L, nsym=nsym, schedule=False),
                 conf, dict(op="init", fs=fs, rs=rs), blocks,
                 dict(op="configure_default"), dict(op="init", fs=9600.0, rs=2400.0),
                 dict(op="blocks", pcm="gs", frame_size=512, nsym=128, schedule=False)]
        arrays, at = dict(pcm=pcm, gc=gc["pcm"], gs=gs["pcm"]), 5
    o = run_child(tmp_path, steps, arrays)
    if name == "c1small":
        assert_golden(o, 2, gc)
    for k, w in enumerate(want):
        assert bits_equal(o["%d.sym" % at][k], w["sym"]) and bits_equal(o["%d.costas" % at][k], w["costas"]), k
        assert o["%d.index" % at][k] == w["index"], k
        assert o["%d.hz" % at][k].tobytes() == w["hz"].tobytes(), k
        assert bits_equal(o["%d.state" % at][k], w["state"]), (k, o["%d.state" % at][k], w["state"])
        # a block leaves gains, limits, damping and bandwidth exactly as the setters left them
        assert bits_equal(o["%d.state" % at][k][2:], o["%d.edited" % at][k][2:]), k
    assert len(SCHEDULE) == len(want) - 1
    if name == "c1small":       # a reconfiguration leaves nothing behind
        assert_golden(o, 8, gs)


# rrc_fir / fft* in an order that makes grow() reallocate between users of the same two staging buffers (bytes: 8 per FIR sample, 16 per
# transform point), on one carried delay line; the last two rrc_fir calls have nothing to do and must touch neither array
STAGING = [("rrc_fir", 1), ("rrc_fir", 126), ("rrc_fir", 127), ("rrc_fir", 128), ("fftn", 512), ("rrc_fir", 513), ("rrc_fir", 4097),
           ("fftn", 16384), ("rrc_fir", 3), ("ifftn", 8192), ("fftn", 1), ("fftn", 2), ("rrc_fir", 70000), ("rrc_fir", 2), ("ifft", 512),
           ("fft", 512), ("rrc_fir", 0), ("rrc_fir", -5)]


def test_rrc_fir_and_fft_share_their_staging(oracle, tmp_path):
    rng = np.random.default_rng(77)
    arrays = dict(mem=rng.standard_normal((127, 2)).astype(np.float32))
    for j, (name, n) in enumerate(STAGING):
        if name == "rrc_fir":
            arrays["x%d" % j] = rng.standard_normal((max(n, 4), 2)).astype(np.float32)
        else:
            arrays["x%d" % j] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    o = run_child(tmp_path, [dict(op="init", fs=9600.0, rs=2400.0), dict(op="staging", calls=STAGING, mem="mem", x="x")], arrays)
    taps = oracle.rrc_make(np.float32(9600.0), np.float32(2400.0), np.float32(.35))
    mem = arrays["mem"].copy()
    for j, (name, n) in enumerate(STAGING):
        x = arrays["x%d" % j]
        if name == "rrc_fir":
            y = x.copy()
            if n > 0:
                oracle.rrc_fir(taps, mem, y[:n])
            assert bits_equal(o["1.y%d" % j], y), (j, name, n)
            assert bits_equal(o["1.m%d" % j], mem), (j, name, n)
        else:
            want = oracle.ifftn(x) if name in ("ifft", "ifftn") else oracle.fftn(x)
            assert bits_equal(o["1.y%d" % j], want), (j, name, n)
            assert bits_equal(o["1.in%d" % j], x), (j, name, n)
