"""The drop-in's scalar loop API (include/qpsk_dropin.h, qpsk_amd/csrc/dropin.c) without a GPU: create_control_loop ... get_min_freq,
phase_detector() and qpsk_demod() are host arithmetic on the drop-in's one loop record, as the reference's are on its file statics.
Bit for bit against the oracle's Costas struct and qo_ functions, which tests/test_oracle_vs_ref.py pins to the reference on the same
sequences (loopsched.py).  None of these calls may need a device: where there is none, a call that tried to create a context would
abort the process."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from loopsched import (GETTERS, SETTER_LIST, TRIPLES, apply_lib, apply_oracle, declare, detector_grid, getters_of, oracle_detector,
                       same_with_nans, state_of)
from oracle.pyoracle import Costas
from sigutil import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dropin(qpsk_lib):
    import qpsk_amd
    lib = C.CDLL(qpsk_amd.lib_path())          # host symbols only: no GPU call
    declare(lib)
    return lib


def test_getters_return_what_the_setters_stored(dropin):
    """each getter reads its own field: eight distinct values in, the same eight out"""
    vals = dict(set_phase=0.5, set_frequency=0.03125, set_max_freq=3.0, set_min_freq=-2.0, set_damping_factor=0.75,
                set_loop_bandwidth=0.0625)
    dropin.set_max_freq(3.0)
    dropin.set_min_freq(-2.0)
    for n in ("set_phase", "set_frequency", "set_damping_factor", "set_loop_bandwidth"):
        getattr(dropin, n)(vals[n])
    dropin.set_alpha(0.375)         # after set_loop_bandwidth(), which recomputes both gains
    dropin.set_beta(-0.4375)
    want = np.array([0.5, 0.03125, 3.0, -2.0, 0.75, 0.0625, 0.375, -0.4375], np.float32)
    assert bits_equal(getters_of(dropin), want), dict(zip(GETTERS, getters_of(dropin)))


def test_step_sequences_and_setters_match_the_oracle(oracle, dropin):
    """create_control_loop() at three (bandwidth, limits) settings, 200 random errors each through advance_loop() -> phase_wrap() ->
    frequency_limit(), then the setter list, dead range checks included: all eight getters against the oracle's struct after every call"""
    rng = np.random.default_rng(8)
    c = Costas()
    # whatever an earlier test left: both start from the same record (twice: the first call's set_frequency(0) is clamped by old limits)
    apply_oracle(oracle, c, [("create_control_loop", 0.0, 0.0, 0.0)] * 2)
    apply_lib(dropin, [("create_control_loop", 0.0, 0.0, 0.0)] * 2)
    assert bits_equal(getters_of(dropin), state_of(c))
    for bw, lo, hi in TRIPLES:
        for op in [("create_control_loop", bw, lo, hi)]:
            apply_lib(dropin, [op])
            apply_oracle(oracle, c, [op])
            assert bits_equal(getters_of(dropin), state_of(c)), op
        for i in range(200):
            e = np.float32(rng.standard_normal() * 3)
            for op in (("advance_loop", e), ("phase_wrap",), ("frequency_limit",)):
                apply_lib(dropin, [op])
                apply_oracle(oracle, c, [op])
                assert bits_equal(getters_of(dropin), state_of(c)), (i, op)
        for op in SETTER_LIST:
            apply_lib(dropin, [op])
            apply_oracle(oracle, c, [op])
            assert bits_equal(getters_of(dropin), state_of(c)), op


HOST = r"""
#include <stdio.h>
#include <stdlib.h>
#include "qpsk_dropin.h"
/* float pairs in, per pair: phase_detector() as a float, then bits[0], bits[1] of qpsk_demod() as two floats */
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 3;
    float p[2];
    while (fread(p, sizeof p, 1, fi) == 1) {
        int bits[2] = {-1, -1};
        const complex float z = CMPLXF(p[0], p[1]);
        float out[3];
        out[0] = phase_detector(z);
        qpsk_demod(z, bits);
        out[1] = (float)bits[0];
        out[2] = (float)bits[1];
        if (fwrite(out, sizeof out, 1, fo) != 1) return 4;
    }
    fclose(fi);
    return fclose(fo) ? 5 : 0;
}
"""


def test_phase_detector_and_demod_by_value(oracle, qpsk_lib, tmp_path):
    """the two functions that take a complex float BY VALUE, called from C11 as a program written against the reference calls them"""
    import qpsk_amd
    src, exe = tmp_path / "host.c", str(tmp_path / "host")
    src.write_text(HOST)
    libdir = os.path.dirname(qpsk_amd.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                           "-lqpsk_hip", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    grid = detector_grid()
    fin, fout = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    grid.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fout, np.float32).reshape(-1, 3)
    assert got.shape[0] == grid.shape[0]
    e, s = oracle_detector(oracle, grid)
    assert same_with_nans(got[:, 0], e)
    assert set(np.unique(got[:, 1:])) <= {0.0, 1.0}
    sym = (got[:, 2].astype(np.uint8) << 1) | got[:, 1].astype(np.uint8)
    assert bits_equal(sym, s)
    # the grid does hold what it is for: exact zeros of the slicer's difference, NaN results, both signs of every decision
    assert np.isnan(e).any() and len(np.unique(s)) == 4 and (np.abs(grid[:, 0]) == np.abs(grid[:, 1])).sum() >= 32
