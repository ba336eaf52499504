"""What the outer link's GPU tests cannot show on a device, shown on the scalar port of outer_push_kernel (outer_port.py) -- no GPU needed.

The port is run over every input set test_outer_gpu.py and test_dvb_gpu.py push (test_outer_cpu.outer_gpu_sets, test_dvb_cpu.dvb_gpu_sets:
the GPU tests build their inputs with the same functions):

 1. it equals the restatement of the header on every output of every push, so it stands for the kernel;
 2. its window never leaves the LDS slice and what it writes back never leaves the ring, within the bound outer.hip's header gives --
    on the device an overrun corrupts the neighbouring stream without failing anything;
 3. every seeded fault of outer_port.FAULTS changes an output (or, for the ring's sizing, leaves the ring) on at least one set: the
    inputs are adequate.  A change to the kernel's hunt or window is repeated in the port and has to keep this file green.
"""
import numpy as np
import pytest

from outer_port import FAULTS, RING_FAULTS, agree, capacity, kept_bound, outer_port, outer_ring_bytes, outer_slice_bytes
from test_dvb_cpu import dvb_gpu_sets, reference_outputs
from test_outer_cpu import outer_gpu_sets

_SETS = {}


def input_sets(new=True):
    """the sets and the reference's outputs for each, computed once"""
    if new not in _SETS:
        sets = outer_gpu_sets(new) + dvb_gpu_sets(new)
        _SETS[new] = [(s, reference_outputs(s)) for s in sets] if new else [(s, w) for s, w in input_sets(True) if s["what"] in {t["what"] for t in sets}]
    return _SETS[new]


def run_port(s, wants, fault=None):
    """the port over one set -> (None or the first output that differs from the reference, the port)"""
    port = outer_port(fault=fault, **s["reset"])
    k = 0
    for step in s["steps"]:
        if step[0] == "advance":
            port.advance(step[1])
            continue
        got = port.push(step[1], step[2])
        differs = agree(got, wants[k], step[2])
        if differs:
            return "push %d: %s" % (k, differs), port
        k += 1
    return None, port


def killed_by(fault, sets):
    """the first set on which a fault shows, and how; None where it survives them all"""
    for s, wants in sets:
        differs, port = run_port(s, wants, fault)
        if differs or (fault in RING_FAULTS and capacity(port)):
            return s["what"], differs or capacity(port)
    return None


def test_the_sets_hold_what_the_cases_are_there_for():
    """what each new case asserts on the reference alone (the GPU tests assert the same on the same outputs)"""
    sets = input_sets()
    assert len({s["what"] for s, _ in sets}) == len(sets)
    checked = 0
    for s, wants in sets:
        if s["check"]:
            s["check"](wants)
            checked += 1
    assert checked >= 50
    geometries = {(s["reset"]["n"], s["reset"]["branches"], s["reset"]["lock"]) for s, _ in sets}
    assert {(224, 32, 2), (255, 1, 16), (64, 32, 2), (6, 3, 16)} <= geometries
    assert any(s["reset"]["branches"] == 32 and s["reset"]["group"] for s, _ in sets)


def test_the_port_equals_the_reference_and_stays_inside_its_slice_and_its_ring():
    seen_window = seen_kept = 0.0
    for s, wants in input_sets():
        differs, port = run_port(s, wants)
        assert differs is None, (s["what"], differs)
        r = s["reset"]
        assert (port.slice_bytes, port.ring_bytes) == (outer_slice_bytes(r["n"], r["branches"], r["lock"]), outer_ring_bytes(r["n"], r["branches"], r["lock"]))
        assert capacity(port) is None, (s["what"], capacity(port))
        seen_window = max(seen_window, (port.hi_window + 1) / port.slice_bytes)
        seen_kept = max(seen_kept, port.kept / kept_bound(r["n"], r["branches"], r["lock"]))
    # the sets do press on both: a hunt's longest look-ahead fills the ring to within a byte or two of the bound, and a chunk on top of it the slice
    assert seen_kept > 0.999 and seen_window > 0.99, (seen_kept, seen_window)


def test_no_byte_behind_the_window_reaches_an_output():
    """the LDS of a launch holds what the last one left: the port fills its window with other random bytes and returns the same"""
    for s, wants in input_sets():
        if s["what"].startswith(("limits", "late decoy", "hunt edge", "word edge", "noise")):
            port = outer_port(seed=1, **s["reset"])
            got = [port.push(step[1], step[2]) for step in s["steps"] if step[0] == "push"]
            assert all(agree(g, w, step[2]) is None for g, w, step in zip(got, wants, s["steps"])), s["what"]


@pytest.mark.parametrize("fault", FAULTS)
def test_every_seeded_fault_shows_on_the_inputs_the_gpu_tests_push(fault):
    found = killed_by(fault, input_sets())
    print(fault, "->", found)
    assert found is not None, "%r changes no output of any input set: the GPU tests would pass a kernel with it" % fault


SURVIVED_BEFORE = ("fx < G dropped from the legal-mask test", "fy < G dropped from the legal-mask test", "p0 loses its bits from 2 G on")


@pytest.mark.parametrize("fault", SURVIVED_BEFORE)
def test_the_faults_the_new_cases_are_for_survive_without_them(fault):
    """why the limits, the long look-aheads and the late decoy are there: on the other sets these three change nothing.  (The fourth the
    look-ahead edge is for, the hunt that counts one candidate too few, shows on them by chance alone: in the info of one push of one
    link, the repeating split at (6, 3, 3, 1), where a push happens to end on the last bit of a look-ahead.  The edge sets put a push there
    at every lead-in.)"""
    assert killed_by(fault, input_sets(new=False)) is None
