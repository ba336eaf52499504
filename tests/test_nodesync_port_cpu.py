"""What the node sync's GPU tests cannot show on a device, shown on the scalar port of nodesync_push_kernel and nodesync_init_kernel
(nodesync_port.py) -- no GPU needed.

The port is run over every set of nodesync_rows (the sweeps of candidate x head x alignment, every int8 pair, the walk through every
candidate, the longest push -- test_nodesync_sweep_gpu.py runs the device over the same sets) and over the inputs of test_nodesync_gpu.py's
transform and tick tests, rebuilt by its code at its seeds, base offsets and pitches:

 1. it equals nodesync_ref in every output byte, every d_info word and the state behind every push, so it stands for the kernels.  limit()
    is run in full: the port takes a row's chunks as one array, so 2^20 dibits cost it a fraction of a second;
 2. every read stays in its link's row or history, every output byte of a row is written exactly once and none outside it, every 16-byte
    store is aligned, the header is stored only with a d_vinfo -- on the device a read beside a row, a byte written twice or an unaligned
    store fails nothing -- and the results from a state and an LDS of random bytes are those from zeros;
 3. turn_packed equals turn_ref(minus128(.)) for all 2^16 values of either half of the word beside six neighbours in the other, all four
    r, and neither half depends on the other;
 4. every fault of nodesync_port.FAULTS changes an output, a d_info word or a state, or breaks a bound of 2., on at least one set: the
    inputs are adequate.  A change to the kernels is repeated in the port and has to keep this file green;
 5. the faults that survive the inputs the suite had before (SURVIVED_BEFORE, bounds included) are held to survive them, and each is
    caught by the new sets.  PORT_ONLY are the faults that no device output shows on any set -- only the port's records of reads, stores
    and the state do.  That is what the port is for;
 6. no change of nodesync_port.EQUIVALENT alters any output, d_info word or state on any set.
"""
import numpy as np
import pytest

from nodesync_port import DEVICE_SEES, EQUIVALENT, FAULTS, turn_packed
from nodesync_rows import NEW, OLD, get, run_port, run_ref
from test_nodesync_cpu import minus128, turn_ref


def evidence(got, want, port):
    """{kind: the first of it}: soft / info / state where a call differs from the reference, and what the port's bounds caught"""
    found = {}
    for k, (g, w) in enumerate(zip(got, want)):
        for key in ("soft", "info", "state"):
            if key not in found and w[key] is not None and not np.array_equal(g[key], w[key]):
                at = np.argwhere(g[key] != w[key])[0].tolist()
                found[key] = "push %d: %s differs at %s" % (k, key, at)
    found.update(port.broken)
    return found


def caught(fault, names, device_only=False):
    """the first set and stream on which a fault shows, and how; None where it survives them all.  device_only: where a GPU test would see it"""
    for name in names:
        s = get(name)
        for stream in range(len(s["streams"])):
            got, port = run_port(s, stream, fault=fault)
            ev = evidence(got, run_ref(s), port)
            if device_only:
                ev = {k: v for k, v in ev.items() if k in DEVICE_SEES}
            if ev:
                return s["name"], "stream %d" % stream, ev
    return None


# ------------------------------------------------------------------------------------------ 1., 2. the port stands for the kernels
@pytest.mark.parametrize("name", OLD + NEW)
def test_the_port_equals_the_reference_and_leaves_no_bound(name):
    s = get(name)
    want = run_ref(s)
    for stream in range(len(s["streams"])):
        got, port = run_port(s, stream)
        assert len(got) == len(want) == len(port.traces)
        assert evidence(got, want, port) == {}, (s["name"], stream)
        assert all((a & 15 == 0).all() for a in port.stores16) and sum(a.size for a in port.stores16) == sum(int(tr["nchunk"].sum()) for tr in port.traces)
        assert port.headers == [step[2] is not None for step in s["steps"] if step[0] == "push"]
        assert all((c == (c > 0)).all() for c in port.writes)
        # a state and an LDS that start as random bytes: the same outputs, d_info and states
        other, port = run_port(s, stream, seed=[stream, 2])
        assert evidence(other, want, port) == {}, (s["name"], stream, "from random bytes")
    if "have" in s:
        print(s["name"], "holds:", ", ".join(s["have"]))


# ------------------------------------------------------------------------------------------ 3. turn_packed, every byte beside every kind of neighbour
@pytest.mark.parametrize("r", range(4))
def test_turn_packed_on_every_value_of_either_half_beside_six_neighbours(r):
    half = np.arange(65536, dtype=np.uint32)
    pairs = np.stack([half & 0xff, half >> 8], axis=-1).astype(np.uint8).view(np.int8)      # (a, b) of the dibit as the device reads it
    want = np.ascontiguousarray(turn_ref(minus128(pairs), r)).view(np.uint8).astype(np.uint32)
    want = want[:, 0] | (want[:, 1] << 8)
    lows, highs = [], []
    for other in (0x0000, 0x8080, 0x7f7f, 0xffff, 0x0180, 0x80ff):
        lo, hi = turn_packed(half | np.uint32(other << 16), r), turn_packed((half << 16) | np.uint32(other), r)
        assert np.array_equal(lo & 0xffff, want) and np.array_equal(hi >> 16, want), (r, hex(other))      # no carry came in from the neighbour
        lows.append(hi & 0xffff)
        highs.append(lo >> 16)
    # ... and none went out: the neighbour's half is the same whatever the half under test holds
    for v in lows + highs:
        assert (v == v[0]).all(), r


# ------------------------------------------------------------------------------------------ 4., 5. the seeded faults
@pytest.mark.parametrize("fault", FAULTS)
def test_every_seeded_fault_shows_on_the_sets_the_gpu_tests_run(fault):
    found = caught(fault, OLD + NEW)
    print(fault, "->", found)
    assert found is not None, "%r changes nothing on any set" % fault


# As found by running the port over OLD, the inputs of test_nodesync_gpu.py's transform and tick tests: nothing differs from the reference and
# no bound of the port breaks.  (No chunk with k0 == 0 belongs to a row 2 bytes off a dword there; its products beyond 32 bits wrap alike on
# both sides; its only set comes before the first switch; its candidates are not negative.)
SURVIVED_BEFORE = ("the vector route at k0 >= 0", "the products in int32", "qpsk_nodesync_set clearing switches", "cand reduced as a signed value")
# As found by running the port over every set: no output byte, d_info word or guard shows these on any of them, on a device every test
# passes.  Only the port's records do: the reads beside a row, the alignment of a 16-byte store, a settle_left below zero in the state (which
# the next tick treats as the 0 it should be), a header stored again with the words just read.  This is what the port is for.
PORT_ONLY = ("the vector route at k0 >= 0", "the vector route at k0 + 9 <= ntx", "the head taken from the input's address",
             "settle_left not clamped at 0", "the header stored without a d_vinfo")


@pytest.mark.parametrize("fault", FAULTS)
def test_survived_before_and_port_only_are_as_the_port_finds_them(fault):
    before, seen = caught(fault, OLD), caught(fault, OLD + NEW, device_only=True)
    print(fault, "| before:", before, "| on a device:", seen)
    assert (before is None) == (fault in SURVIVED_BEFORE), before
    assert (seen is None) == (fault in PORT_ONLY), seen
    if fault in SURVIVED_BEFORE:
        assert caught(fault, NEW) is not None                               # what the new sets are for


def test_the_two_lists_are_not_empty_by_construction():
    """the two bound faults of the vector route's condition cannot change an output: they are PORT_ONLY wherever they are caught"""
    assert {"the vector route at k0 >= 0", "the vector route at k0 + 9 <= ntx"} <= set(PORT_ONLY)
    assert set(SURVIVED_BEFORE) <= set(FAULTS) and set(PORT_ONLY) <= set(FAULTS)


# ------------------------------------------------------------------------------------------ 6. what may change nothing
@pytest.mark.parametrize("change", sorted(EQUIVALENT))
def test_the_changes_left_out_of_the_fault_list_change_nothing(change):
    assert caught(change, OLD + NEW) is None, EQUIVALENT[change]
