"""What the deframers' GPU tests cannot show on a device, shown on the scalar port of deframe_hunt() (hunt_port.py) -- no GPU needed.

The port is run over every input set the deframers' GPU tests push for the hunt (test_deframe_cpu.hunt_sets / hunt_coded_sets / old_sets: the
GPU tests build their inputs with the same functions, so no input reaches a device that has not passed this file):

 1. it equals the restatements of the header -- deframe_ref, deframe_coded_ref and its punctured and interleaved forms -- on every field
    of every packet and on the push that completes it, so it stands for the template;
 2. every push stays inside what the kernel owns (tail index < nsync - 1, plane word <= steps + 1, row symbol < nsym, pending index < N,
    slot < cap) and every walk ends within steps + packets iterations;
 3. every seeded fault of hunt_port.FAULTS changes an output on at least one set: the inputs are adequate.  A change to the template is
    repeated in the port and has to keep this file green;
 4. which faults a subset of the inputs of test_deframe_gpu's tests 1, 1b and 2 lets through on its own is asserted, as a record of why
    the sets are there.  Equality, bounds and this list all run the first twelve of the 300 streams of test 1 and of the 64 of test 2
    (OLD_STREAMS; a full pass costs minutes).  Run once over all their streams, tie_ge, cap_le and count_written pass the whole of
    tests 1, 1b and 2, and skip_step does not.
"""
import numpy as np
import pytest

from hunt_port import FAULTS, ROOM, BytePackets, HuntArgs, HuntState, SoftPackets, bounds, deframe_hunt
from test_deframe_cpu import (HUNT_S, coded_reference, crc16, hunt_coded_sets, hunt_sets, keystream, old_sets, overflow_set, set_of_test_1,
                              want_of, written)
from test_rx_data_cpu import RING, data_rule, dibits_to_bytes
from test_soft_cpu import quantise

OLD_STREAMS = slice(0, 12)      # of the 300 streams of test 1 and the 64 of test 2: the first twelve
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def uncoded_sets():
    return cached("uncoded", hunt_sets)


def coded_sets():
    return cached("coded", lambda: [s for kind in ("plain", "punct", "ilv") for s in hunt_coded_sets(kind)])


def old():
    return cached("old", lambda: old_sets(OLD_STREAMS))


def uncoded_wants(s):
    """per cutting, per stream: (count per push, the records the pushes write)"""
    return cached(("want", s["what"]), lambda: [[written(want_of(s["D"][k], cuts, s["sync"], s["min_score"], s["nbytes"]), len(cuts), s["max_packets"])
                                                 for k in range(s["D"].shape[0])] for cuts in s["cuttings"]])


def coded_wants(s):
    return cached(("want", s["what"]), lambda: [coded_reference(s, cuts) for cuts in s["cuttings"]])


def run_uncoded(s, cuts, k, fault=None):
    """the port with deframe.hip's policy over stream k of a set under one cutting -> (count per push, records as want_of's, None or
    the first bound a push left)"""
    a, st = HuntArgs(s["sync"], s["min_score"]), HuntState()
    nbytes = s["nbytes"]
    N = 4 * (nbytes + 2)
    ks = keystream(N)
    row_all = RING[s["D"][k] & 3]
    pend = [0] * (N + ROOM)
    counts, recs, left, at = [], [], None, 0
    for j, c in enumerate(cuts):
        a.nsym = c
        p, see = BytePackets(row_all[at:at + c], N, pend), {}
        count = deframe_hunt(a, N, s["max_packets"], st, p, fault, see)
        left = left or bounds(see, a, N, s["max_packets"])
        counts.append(count)
        for slot, pos, rot, score, v in p.out:
            b = dibits_to_bytes(RING[(np.array(v, np.int64) - rot) & 3] ^ ks)
            recs.append((j, pos, rot, score, b.tobytes(), bool(crc16(b[:nbytes]) == (int(b[nbytes]) << 8 | int(b[nbytes + 1])))))
        at += c
    return counts, recs, left


def run_coded(s, cuts, k, fault=None):
    """the port with deframe_coded.hip's policy -> (count per push, records (push, pos, rot, score, soft bytes), the first bound left).
    cap is api_packets.cpp's per_stream"""
    a, st = HuntArgs(s["sync"], s["min_score"]), HuntState()
    N, g = s["nbody"], s["gain"][k]
    z = s["z"][k]
    row_all = RING[data_rule(z)]
    pend = [None] * (N + ROOM)
    counts, recs, left, at = [], [], None, 0
    for j, c in enumerate(cuts):
        a.nsym = c
        row = z[at:at + c]

        def soften(row0, cnt, rot, row=row):
            x = row[max(row0, 0):max(row0 + cnt, 0)]
            u, v = ((x[:, 0], x[:, 1]), (x[:, 1], -x[:, 0]), (-x[:, 0], -x[:, 1]), (-x[:, 1], x[:, 0]))[rot]
            q = np.stack([quantise(u, g), quantise(v, g)], axis=1)
            return [(int(e[0]), int(e[1])) for e in q] + [None] * (cnt - len(q))

        cap = min(s["max_packets"], c // (s["nsync"] + N) + 1)
        p, see = SoftPackets(row_all[at:at + c], N, pend, soften), {}
        count = deframe_hunt(a, N, cap, st, p, fault, see)
        left = left or bounds(see, a, N, cap)
        counts.append(count)
        recs += [(j, pos, rot, score, tuple(body)) for slot, pos, rot, score, body in p.out]
        at += c
    return counts, recs, left


def coded_records(ref, max_packets):
    """one stream's reference under one cutting -> (count per push, the records the pushes write, in run_coded's form)"""
    return [len(push) for push in ref], [(j, p["pos"], p["rot"], p["score"], tuple((int(e[0]), int(e[1])) for e in p["soft"]))
                                         for j, push in enumerate(ref) for p in push[:max_packets]]


def differs(s, fault=None, check_bounds=False):
    """None where the port equals the reference on a whole set, or where it first does not"""
    coded = "z" in s
    wants = coded_wants(s) if coded else uncoded_wants(s)
    for c, cuts in enumerate(s["cuttings"]):
        for k in range(s["z" if coded else "D"].shape[0]):
            counts, recs, left = (run_coded if coded else run_uncoded)(s, cuts, k, fault)
            want = coded_records(wants[c][k], s["max_packets"]) if coded else wants[c][k]
            if counts != want[0]:
                return "cutting %d, stream %d: count" % (c, k)
            if recs != want[1]:
                return "cutting %d, stream %d: records" % (c, k)
            if check_bounds and left:
                return "cutting %d, stream %d: %s" % (c, k, left)
    return None


def killed_by(fault, sets):
    for s in sets:
        d = differs(s, fault)
        if d:
            return s["what"], d
    return None


def test_the_sets_hold_what_the_cases_are_there_for():
    """what each set asserts on the reference alone, before anything is compared with it"""
    for s in uncoded_sets():
        s["check"](s)
    for s in coded_sets():
        s["check"](s, coded_wants(s))
    names = [s["what"] for s in uncoded_sets() + coded_sets()]
    assert len(set(names)) == len(names)
    assert all(s["D"].shape[0] == HUNT_S for s in uncoded_sets()) and all(s["z"].shape[0] == HUNT_S for s in coded_sets())
    # the cap is the nsym term of per_stream in one set, max_packets in the next, and both at equality with what the push completes
    for s in coded_sets():
        if "back to back" in s["what"]:
            big = max(s["cuttings"][0])
            per = min(s["max_packets"], big // (s["nsync"] + s["nbody"]) + 1)
            assert per == min(s["max_packets"], 4) and max(len(r[k][1]) for r in coded_wants(s) for k in range(HUNT_S)) == 4


@pytest.mark.parametrize("which", ["new", "coded", "old"])
def test_the_port_equals_the_references_stays_in_bounds_and_ends(which):
    for s in {"new": uncoded_sets, "coded": coded_sets, "old": old}[which]():
        assert differs(s, None, check_bounds=True) is None, s["what"]


@pytest.mark.parametrize("fault", FAULTS)
def test_every_seeded_fault_shows_on_the_new_sets(fault):
    found = killed_by(fault, uncoded_sets() + coded_sets())
    print(fault, "->", found)
    assert found is not None, "%r changes no output of any new set: the GPU tests would pass a kernel with it" % fault


def test_each_tie_set_and_each_cap_set_does_what_it_is_there_for():
    """killed_by stops at the first set that shows a fault, which is dense noise for most.  The sets made for one fault must show it
    themselves: every tie set the rotation rule, every set whose max_packets is below what one push completes the count < cap gate"""
    sets = uncoded_sets() + coded_sets()
    ties = [s for s in sets if s["what"].startswith("ties")]
    caps = [s for s in sets if s["what"].endswith("max_packets 3")]
    assert len(ties) == 8 and len(caps) == 4
    for s in ties:
        assert differs(s, "tie_ge"), s["what"]
    for s in caps:
        assert differs(s, "cap_le") and differs(s, "count_written"), s["what"]


SURVIVED_BEFORE = ("tie_ge", "skip_step", "cap_le", "count_written")      # by OLD_STREAMS of tests 1 and 2 and all of 1b
SKIP_STEP_SHOWS = (32, 16, 116)                                            # test 1 at (nsync, nbytes): a stream beyond OLD_STREAMS


def test_the_faults_that_survive_the_old_inputs():
    """the inputs of tests 1, 1b and 2 of test_deframe_gpu.py alone, tests 1 and 2 cut to OLD_STREAMS (all six streams of 1b): the faults
    that subset lets through.  The list is NOT what the whole of test 1 lets through:

      tie_ge                  survives every old input outright: at those thresholds two rotations never reach the same count.
      skip_step               survives the subset only.  Among test 1's 300 streams some do show it -- by volume, an hx that happens to be
                              the last position of a step -- and one of them is asserted here; the noise sets show it in every stream.
      cap_le, count_written   no push of tests 1, 1b and 2 completes more than max_packets, in any stream; the input of test 3 (the
                              overflow test: ten packets, max_packets = 3) shows both."""
    alive = tuple(f for f in FAULTS if killed_by(f, old()) is None)
    print("survive the old sets:", alive)
    assert alive == SURVIVED_BEFORE
    nsync, nbytes, stream = SKIP_STEP_SHOWS
    one = set_of_test_1(nsync, nbytes, [stream])
    one["what"] += ", stream %d" % stream
    assert differs(one) is None and differs(one, "skip_step") and differs(one, "tie_ge") is None
    test3 = [overflow_set()]
    assert differs(test3[0]) is None
    assert [f for f in alive if killed_by(f, test3) is None] == ["tie_ge", "skip_step"]
