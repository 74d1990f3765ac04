"""ftk_amd/csrc/ingest_steps.hpp WITHOUT a GPU: which steps bring a caller's array into a resident FP64 array -- adopted, copied, staged,
which kernel writes it first, whether the adjust kernel follows in place, which debug counter moves, whether the caller waits -- for
every case there is, against the rules written out here a second time; and what must hold of any plan whatever the rules say."""
import pytest

import ingest_cases as IC


def expected(f32, planar, smooth, adjust, on_device, on_this_device):
    """the rules, as the push entry points have behaved since planar snapshots and aux fields came in"""
    if planar:
        reads_here = on_device == 1 and on_this_device          # planes given as "any device" (2) are always staged ...
    else:
        reads_here = on_device != 0 and on_this_device          # ... an interleaved array of 2 on this device is read where it lies
    adopt = (not f32) and (not planar) and on_device == 1 and (not smooth) and (not adjust)
    waits = on_device != 0 and not adopt
    if adopt:
        return IC.Plan(reads_here, True, False, "none", "none", "none", False, frozenset())
    if not (f32 or smooth or planar):
        if not adjust:
            return IC.Plan(reads_here, False, waits, "none", "dst", "none", False, frozenset())
        if reads_here:
            return IC.Plan(reads_here, False, waits, "none", "none", "adjust", False, frozenset(["out_of_place"]))
        return IC.Plan(reads_here, False, waits, "none", "dst", "none", True, frozenset(["in_place"]))
    stage = "none" if reads_here else "f32_stage" if f32 else "pooled"
    copy = "none" if reads_here else "stage"
    counters = set()
    if planar:
        first = "concat"; counters.add("planar")
    elif smooth:
        first = "conv"
        if f32:
            counters.add("f32_direct")
    elif adjust:
        first = "adjust"; counters.add("from_float")
    else:
        first = "widen"; counters.add("f32_widened")
    then_adjust = adjust and first != "adjust"
    if then_adjust:
        counters.add("in_place")
    return IC.Plan(reads_here, False, waits, stage, copy, first, then_adjust, frozenset(counters))


def legal_cases():
    """all 96 inputs but the 24 every caller refuses before the plan is asked (planes and spatial smoothing)"""
    cases = [c for c in IC.all_inputs() if not (c[1] and c[2])]
    assert len(IC.all_inputs()) == 96 and len(cases) == 72 and len(set(cases)) == 72
    return cases


def test_every_case_follows_the_rules():
    seen = 0
    for case in legal_cases():
        got, exp = IC.plan(*case), expected(*case)
        for field in IC.Plan._fields:
            assert getattr(got, field) == getattr(exp, field), (case, field, got, exp)
        seen += 1
    assert seen == 72


def test_what_holds_of_every_plan():
    for case in legal_cases():
        f32, planar, smooth, adjust, on_device, on_this_device = case
        p = IC.plan(*case)
        if p.adopt:                                             # nothing is queued, nobody waits
            assert (p.stage, p.copy, p.first, p.then_adjust, p.counters, p.caller_waits) == ("none", "none", "none", False, frozenset(), False), case
            assert not f32 and on_device == 1, case
            continue
        # dst has exactly one first writer: the copy, or the first kernel
        assert (p.copy == "dst") != (p.first != "none"), (case, p)
        # never both a stage and a copy into dst; a stage is what the copy fills
        assert (p.stage != "none") == (p.copy == "stage"), (case, p)
        # the first kernel reads the caller's pointers exactly where nothing was copied -- and only where they are this device's memory
        kernel_reads_source = p.first != "none" and p.copy == "none"
        assert not kernel_reads_source or p.reads_here, (case, p)
        # a float source is never copied into dst as it is, and is staged in the float block only
        assert not (f32 and p.copy == "dst") and (p.stage == "f32_stage") == (f32 and p.copy == "stage"), (case, p)
        # adjust is applied exactly once iff it is asked for
        assert int(p.first == "adjust") + int(p.then_adjust) == int(adjust), (case, p)
        adjust_counted = len(p.counters & {"from_float", "in_place", "out_of_place"})
        assert adjust_counted == int(adjust), (case, p)
        assert ("in_place" in p.counters) == p.then_adjust, (case, p)
        assert p.caller_waits == (on_device != 0), (case, p)
        if on_device == 0:                                      # whatever on_this_device says
            assert not p.reads_here, (case, p)


def test_host_memory_is_never_read_in_place_and_unasked_pointers_do_not_matter():
    for case in legal_cases():
        f32, planar, smooth, adjust, on_device, on_this_device = case
        if on_device == 0:
            assert not IC.plan(*case).reads_here and not IC.asks_where(*case[:5]), case
        if not IC.asks_where(*case[:5]):                        # the executor does not examine the pointer there: the plan must not depend on it
            a, b = IC.plan(*case[:5], False), IC.plan(*case[:5], True)
            assert a._replace(reads_here=False) == b._replace(reads_here=False), case
            assert (a.first == "none" or a.copy != "none") and (a.adopt or a.copy != "none"), case


def test_a_caller_that_must_own_never_adopts():
    """the temporal ring: the case that would be adopted is a plain copy into the slot, and the caller waits for it"""
    for case in legal_cases():
        p, q = IC.plan(*case), IC.plan(*case, must_own=True)
        assert not q.adopt
        if not p.adopt:
            assert p == q, case
        else:
            assert (q.stage, q.copy, q.first, q.then_adjust, q.counters, q.caller_waits) == ("none", "dst", "none", False, frozenset(), True), case


@pytest.mark.parametrize("on_device,here", [(1, True), (2, True), (2, False)])
def test_the_planar_quirk_is_kept(on_device, here):
    """planes handed over as device memory of any device (2) are staged even where they lie on this device; an interleaved array is not"""
    planes, array = IC.plan(True, True, False, False, on_device, here), IC.plan(True, False, False, False, on_device, here)
    assert array.reads_here == here and planes.reads_here == (here and on_device == 1)
    assert (planes.stage == "none") == planes.reads_here and (array.stage == "none") == array.reads_here
