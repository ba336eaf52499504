"""What the streaming Viterbi decoder's GPU tests cannot show on a device, shown on the scalar port of viterbi_stream_kernel,
viterbi_stream_punct_kernel, viterbi_stream_flush_kernel and viterbi_stream_init_kernel with the host's bookkeeping (vstream_port.py) -- no
GPU needed.

The port is run over every set of vstream_rows: OLD, the inputs of test_viterbi_stream_gpu.py's decoder tests rebuilt by its code at its
seeds, splits, pitches and advances, and NEW (flushes on the block grid, streams of a few steps, ties, the rings' corners, one-period
pushes, 300 streams, odd alignments, the longest push), which test_viterbi_stream_sweep_gpu.py runs on the device:

 1. it equals viterbi_stream_ref in every bit, nbits and all four info words of every call and in the state behind it (what of the state is
    alive: pm at the last whole block, the pending pairs, the last emitted word, the ring by slot), and leaves no bound: every read of the
    soft image inside its stream's row, every state byte read written since the reset and by the lane that reads it, no ring slot at or
    above nring, no pending pair written at or beyond rem, every byte of a call's bits and info written exactly once and none elsewhere;
 2. the same from a state of random bytes, and the traces hold what each set was built for (its `have`, asserted when the set is built);
 3. every fault of vstream_port.FAULTS changes a bit, an info word or the state behind a call, or breaks a bound, on at least one set;
 4. the faults that survive the inputs the suite had before (SURVIVED_BEFORE) are held to survive them, and each is caught by NEW.
    PORT_ONLY are the faults that nothing a device shows (bits, nbits, info, the return code, guards and poison) gives away on any set;
    UNSEEN_ON_A_DEVICE_BEFORE those that nothing a device shows gave away on OLD and something does on NEW.  All three are pinned both ways;
 5. no change of vstream_port.EQUIVALENT alters anything on any set;
 6. the host's numbers of a launch (pc, slot, have, wphase, nbits) equal a count of blocks, one step at a time, for every total in
    0..4 (D + W), with and without an advance that is no multiple of the ring.

Run time on the machine this was written on: 104 s, against 32 s of test_nodesync_port_cpu.py measured there the same day.  The two longest
pushes (131072 and 131068 steps, one stream each) take about 58 s of it: 23 s in parts 1 and 2 (the reference once, the port twice), the
rest in the eight runs of parts 4 and 5 that no smaller set ends early (three PORT_ONLY faults, five equivalent changes).  Without them
the file takes about 45 s.
"""
import functools

import numpy as np
import pytest

from vstream_port import DEVICE_SEES, EQUIVALENT, FAULTS, Refused, vstream_port
from vstream_rows import NEW, OLD, get, run_port, run_ref, state_differs


def evidence(got, want, port):
    """{kind: the first of it}: nbits / bits / info / state where a call differs from the reference, and what the port's bounds caught"""
    found = {}
    for k, (g, w) in enumerate(zip(got, want)):
        if "nbits" not in found and g["nbits"] != w["nbits"]:
            found["nbits"] = "call %d: nbits %d, not %d" % (k, g["nbits"], w["nbits"])
        for key in ("bits", "info"):
            if key not in found and g[key] is not None and not np.array_equal(g[key], w[key]):
                found[key] = "call %d: %s differs" % (k, key) + (" at %s" % np.argwhere(g[key] != w[key])[0].tolist() if g[key].shape == w[key].shape else "")
        if "state" not in found:
            d = state_differs(g["state"], w)
            if d:
                found["state"] = "call %d: %s" % (k, d)
    found.update(port.broken)
    return found


@functools.lru_cache(maxsize=None)
def shows(fault, name):
    """the evidence of one fault on one set, as a tuple of (kind, text)"""
    s = get(name)
    try:
        got, port = run_port(s, fault=fault)
    except Refused as e:
        return (("refused", "the host refuses a call: %s" % e),)
    return tuple(sorted(evidence(got, run_ref(s), port).items()))


def caught(fault, names, device_only=False):
    """the first set on which a fault shows, and how; None where it survives them all.  device_only: where a GPU test would see it"""
    for name in names:
        ev = {k: v for k, v in shows(fault, name) if not device_only or k in DEVICE_SEES}
        if ev:
            return name, ev
    return None


# ------------------------------------------------------------------------------------------ 1., 2. the port stands for the kernels
@pytest.mark.parametrize("name", OLD + NEW)
def test_the_port_equals_the_reference_and_leaves_no_bound(name):
    s = get(name)
    want = run_ref(s)
    got, port = run_port(s)
    assert len(got) == len(want) == len(port.traces) == len(port.writes)
    assert evidence(got, want, port) == {}, name
    for (count, icount), g in zip(port.writes, got):
        assert (count is None) == (g["bits"] is None) and (icount is None) == (g["info"] is None)
        assert all(c is None or (c.sum() == g["state"].shape[0] * ((g["nbits"] + 7) // 8 if c is count else 16) and c.max(initial=0) <= 1) for c in (count, icount))
    # a state that starts as random bytes, and is random again where a flush ends its life: the same bits, info and live state
    other, port = run_port(s, seed=[len(name), 2])
    assert evidence(other, want, port) == {}, (name, "from random bytes")
    print(name, "holds:", ", ".join(s["have"]))


# ------------------------------------------------------------------------------------------ 3., 4. the seeded faults
@pytest.mark.parametrize("fault", FAULTS)
def test_every_seeded_fault_shows_on_the_sets_the_gpu_tests_run(fault):
    found = caught(fault, OLD + NEW)
    print(fault, "->", found)
    assert found is not None, "%r changes nothing on any set" % fault


# As found by running the port over OLD, the inputs of test_viterbi_stream_gpu.py's decoder tests: nothing differs from the reference and no
# bound of the port breaks.  (No flush of OLD stands on the block grid with bits waiting, so decide<true> never walks a whole newest block.)
# The other fault expected here from reading, "best_state ties to the highest state", does NOT survive OLD: full-range random content ties
# the best metric between a few states at some decision point of most sets (their `have` says so: "a tie of the best state between some
# states"; with some hundred decisions of 64 metrics a few thousand apart that is no rare event), info[2] of that call shows the other state
# in six of the nine sets of OLD, 'old splits' first, and in four of them a bit changes too.  What OLD lacks is the 64-way tie, where the
# rule decides alone; 'ties' has it.
SURVIVED_BEFORE = ("n_newest = a.pc without the 64 of pc == 0",)
# As found by running the port over OLD: the port's records show these there (a state byte that differs, a read of a byte not written), but
# no bit, info word, return code or guard does, so test_viterbi_stream_gpu.py passes with them on a device; the device sees each on NEW.
#   no -128 rule in PunctLoader::value     a -128 moves the metrics by one and reaches info[3] (spread) first in the one-period pushes
#   last not cleared                       behind a flush's partial block `last` has no bit above the block's steps, and only bits 58..63
#                                          reach the next stream's first count: it takes a flush on the block grid to leave them set
#   n_newest = a.pc ...                    as above
UNSEEN_ON_A_DEVICE_BEFORE = ("no -128 rule in PunctLoader::value", "n_newest = a.pc without the 64 of pc == 0", "last not cleared")
# As found by running the port over every set: no bit, info word, return code or guard shows these on any of them, on a device every test
# passes.  Only the port's records do: a pending pair written at rem (dead: the next push reads the pairs below its pc, and writes this one
# first if it ends later), reads of the soft image behind the row (what they fetch goes to lanes whose pairs no step and no pending store
# takes), ballot words read back by a lane that did not write them (the same words at the same places).  This is what the port is for.
PORT_ONLY = ("pending written for lane <= rem", "the load ahead not masked at a.n", "the ballots stored by lanes 1..4")


@pytest.mark.parametrize("fault", FAULTS)
def test_survived_before_and_port_only_are_as_the_port_finds_them(fault):
    before, seen = caught(fault, OLD), caught(fault, OLD + NEW, device_only=True)
    seen_before = caught(fault, OLD, device_only=True)
    print(fault, "| before:", before, "| on a device before:", seen_before, "| on a device:", seen)
    assert (before is None) == (fault in SURVIVED_BEFORE), before
    assert (seen is None) == (fault in PORT_ONLY), seen
    assert (seen_before is None and seen is not None) == (fault in UNSEEN_ON_A_DEVICE_BEFORE), (seen_before, seen)
    if fault in SURVIVED_BEFORE:
        assert caught(fault, NEW) is not None                               # what the new sets are for
    if fault in UNSEEN_ON_A_DEVICE_BEFORE:
        assert caught(fault, NEW, device_only=True) is not None


def test_the_predictions_of_the_port_s_first_reading():
    """expected to survive OLD: the flush's 64 of pc == 0 (it does) and the tie rule of best_state (it does not: info[2] shows it, and
    bits in some sets); expected to be PORT_ONLY: the pending pair at rem and the unmasked load ahead (both are)"""
    assert "n_newest = a.pc without the 64 of pc == 0" in SURVIVED_BEFORE
    tie = {n: dict(shows("best_state ties to the highest state", n)) for n in OLD}
    assert "info" in tie["old splits"] and sum("info" in ev for ev in tie.values()) == 6 and sum("bits" in ev for ev in tie.values()) == 4, tie
    assert not any("a 64-way tie of the best state" in get(n)["have"] for n in OLD) and "a 64-way tie of the best state" in get("ties")["have"]
    assert {"pending written for lane <= rem", "the load ahead not masked at a.n"} <= set(PORT_ONLY)


def test_the_two_lists_hold_faults_only():
    assert set(SURVIVED_BEFORE + UNSEEN_ON_A_DEVICE_BEFORE + PORT_ONLY) <= set(FAULTS) and not set(EQUIVALENT) & set(FAULTS)


# ------------------------------------------------------------------------------------------ 5. what may change nothing
@pytest.mark.parametrize("change", sorted(EQUIVALENT))
def test_the_changes_left_out_of_the_fault_list_change_nothing(change):
    assert caught(change, OLD + NEW) is None, EQUIVALENT[change]


# ------------------------------------------------------------------------------------------ 6. the host's numbers against a count of blocks
def count_blocks(depth, window, upto, advance_at=None, delta=0):
    """one step at a time, with no division of a position: per total the numbers a push and a flush at that total must get.  An advance
    (at total advance_at, by delta) moves the position and nothing that is counted"""
    nring, rows = (depth + window) // 64, {}
    stored = inring = since = inblock = waiting = 0          # whole blocks: stored since the reset, held by the ring, since the last decision
    total, next_slot = 0, 0                                  # point, waiting to be emitted; steps of the block in the making; the ring's hand
    for _ in range(upto + 1):
        if total == advance_at:
            total += delta
        rows[total] = dict(push=dict(pc=inblock, slot=next_slot, have=inring, wphase=since),
                           flush=dict(pc=inblock, slot=next_slot if inblock else (next_slot - 1) % nring if stored else 0,
                                      have=waiting + (inblock > 0), nbits=64 * waiting + inblock))
        total, inblock = total + 1, inblock + 1
        if inblock == 64:
            inblock, stored, inring, since, waiting = 0, stored + 1, min(inring + 1, nring), since + 1, waiting + 1
            next_slot = 0 if next_slot + 1 == nring else next_slot + 1
            if since == window // 64:
                since, waiting = 0, min(waiting, depth // 64)      # a decision point: all but the newest D steps leave
    return rows


@pytest.mark.parametrize("depth,window", [(64, 64), (192, 128), (64, 192)])
@pytest.mark.parametrize("advanced", [False, True])
def test_the_hosts_numbers_equal_a_count_of_blocks(depth, window, advanced):
    nring = (depth + window) // 64
    delta = window * 12345677 if advanced else 0
    assert not advanced or delta // 64 % nring != 0
    at = depth + window + 70 if advanced else None
    port = vstream_port()
    port.reset(1, depth, window)
    for total, want in count_blocks(depth, window, 4 * (depth + window), at, delta).items():
        port.total, port.advanced = total, delta if advanced and total > at else 0
        assert port.push_numbers() == want["push"], (total, port.push_numbers(), want["push"])
        assert port.flush_numbers() == want["flush"], (total, port.flush_numbers(), want["flush"])
