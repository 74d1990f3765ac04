"""ftk_amd/csrc/batch_plan.hpp WITHOUT a GPU: every decision of the host-driven batch (ftkx_sweep_enqueue / ftkx_sweep_collect /
ftkx_sweep_cull) -- which way a request goes, which tile kernel form it may take, which masks a batch builds in which sub-batch, its
tile launches, where the descriptors lie, the sort's key bits, what follows from a batch's counters -- against the rules written out
here a second time, and against what must hold of any plan whatever the rules say."""
import itertools
import math
import random
from fractions import Fraction


import batch_cases as BC
from batch_cases import Facts, Request

INT64_MAX = (1 << 63) - 1


# ---- the rules, a second time ----------------------------------------------------------------------------------------------------------
def overflow_free(nd, maxabs, factor):
    M = math.floor(Fraction(maxabs) * factor) + 1
    return 24 * M ** 3 < INT64_MAX if nd == 3 else 6 * M * M < INT64_MAX


def valid(nd, f, factor, two_level, u_rows):
    if not f.has_M or (two_level and not f.has_U) or f.mask_factor == 0 or f.mask_factor > factor:
        return False
    if two_level and f.u_rows != u_rows:
        return False
    if f.mask_big and f.mask_factor == factor:
        return True
    return f.max_known and overflow_free(nd, f.maxabs, factor)


def built(nd, f, factor, two_level, u_rows):
    """the facts of a slice after a mask job under `factor`"""
    rule_on = not (f.max_known and overflow_free(nd, f.maxabs, factor))
    return f._replace(has_M=True, has_U=f.has_U or two_level, mask_factor=factor, mask_big=rule_on, u_rows=u_rows), rule_on


def form(nd, robust, bound, fan):
    if nd == 3 and not robust:
        f = 0
    elif bound < 0:
        f = 1
    elif bound < (2 ** 19 - 1 if nd == 3 else 2 ** 25 - 1):
        f = 2
    elif bound < 2 ** 31 - 1:
        f = 1
    else:
        f = 0
    return min(f, 2 if fan == 9 else fan)


def test_overflow_free_and_the_big_threshold():
    safe = {2: 1239850262, 3: 727041}                          # the largest M with 6 M^2 / 24 M^3 < 2^63
    for nd, M in safe.items():
        assert overflow_free(nd, float(M - 1), 1) and not overflow_free(nd, float(M), 1)
        for maxabs, factor in ((float(M - 1), 1), (float(M), 1), (0.0, 1 << 53), (1.0, 1 << 20), (1.0, 1 << 19), (3.5, 1 << 30), ((M - 1) / 4096.0, 4096), (M / 4096.0, 4096), (1e300, 2)):
            assert BC.overflow_free(nd, maxabs, factor) == overflow_free(nd, maxabs, factor), (nd, maxabs, factor)
        for factor in (1, 256, 1 << 40):
            assert BC.big_threshold(nd, factor) == M / factor
    for f in (0, 1, 2, 3, 6, 1 << 20, (1 << 20) + 1, 1 << 53, 1 << 54, (1 << 64) - 1):
        assert BC.pow2_factor(f) == (f != 0 and f & (f - 1) == 0 and f <= 1 << 53), f


# ---- slices as a batch may find them ---------------------------------------------------------------------------------------------------
LOW, HIGH = 16384, 65536                                       # the two factors of the series below
SMALL, HUGE = 0.75, 1e9                                        # max |v|: no vertex big under either factor (2D and 3D) / under both


def masks(factor, big=False, known=None, u_rows=1, sparse=False):
    return Facts(True, True, sparse, factor, big, u_rows, known is not None or sparse, known if known is not None else 0.0)


STARTS = [BC.NO_MASKS, BC.NO_MASKS._replace(max_known=True, maxabs=SMALL), BC.NO_MASKS._replace(max_known=True, maxabs=HUGE),
          Facts(True, False, False, LOW, False, 1, True, SMALL),                            # masks without summaries
          masks(4096, known=SMALL), masks(4096), masks(LOW, known=SMALL), masks(LOW, big=True), masks(LOW, big=True, known=HUGE),
          masks(HIGH, known=SMALL), masks(HIGH, big=True), masks(1 << 20, known=SMALL), masks(LOW, known=SMALL, u_rows=4),
          masks(LOW, sparse=True, known=SMALL), masks(HIGH, sparse=True, known=SMALL), masks(LOW, sparse=True, known=HUGE)]


def test_masks_valid_and_job_big_follow_the_rules():
    for nd, f, factor, two_level, u_rows in itertools.product((2, 3), STARTS, (4096, LOW, HIGH, 1 << 20), (False, True), (1, 4)):
        assert BC.masks_valid(nd, f, factor, two_level, u_rows) == valid(nd, f, factor, two_level, u_rows), (nd, f, factor, two_level, u_rows)
        big, on = BC.job_big(nd, f, factor)
        assert on == built(nd, f, factor, two_level, u_rows)[1]
        assert big == (BC.big_threshold(nd, factor) if on else math.inf)
    assert valid(2, masks(LOW, known=SMALL), HIGH, True, 1) and not valid(2, masks(LOW, big=True), HIGH, True, 1) and not valid(2, masks(HIGH, known=SMALL), LOW, True, 1)


# ---- modes -----------------------------------------------------------------------------------------------------------------------------
def test_modes_full_product():
    factors = [1, 2, 4, 16384, 1 << 53, 1 << 54, 3, 5, 16383, 16385, (1 << 53) + 2, (1 << 64) - 1]
    seen = set()
    for exact_only, factor, nd, robust, dense in itertools.product((False, True), factors, (2, 3), (False, True), (0, 1, 16)):
        fast = (not exact_only) and factor & (factor - 1) == 0 and factor <= 1 << 53 and (nd == 2 or robust)
        exp = "tile" if not fast else "tile_cull" if dense > 0 else "fast"
        got = BC.request_mode(exact_only, factor, nd, robust, dense)
        assert got == exp, (exact_only, factor, nd, robust, dense)
        # a masked halo slice: refused unless the cull is usable and masks are what the request goes by
        assert BC.sparse_slice_refuses(got) == ((not fast) or dense > 0)
        seen.add(got)
    assert seen == {"tile", "fast", "tile_cull"}


# ---- forms -----------------------------------------------------------------------------------------------------------------------------
BOUNDS = [-1, 2 ** 19 - 1, 2 ** 19, 2 ** 25 - 1, 2 ** 25, 2 ** 31 - 1, 2 ** 31]


def test_forms_at_every_threshold():
    for nd, robust, bound, fan in itertools.product((2, 3), (False, True), BOUNDS + [0, 2 ** 19 - 2, 2 ** 25 - 2, 2 ** 31 - 2, 1e300], (0, 1, 2, 9)):
        assert BC.tile_form(nd, robust, bound, fan) == form(nd, robust, bound, fan), (nd, robust, bound, fan)
    # the table, spelt out where it matters: unknown magnitudes take the integer form with the fp64 fan off; small ones the fp64 fan;
    # what may leave int32 the general form; the knob only ever lowers the form, and 9 stands for 2
    assert [BC.tile_form(2, True, b, 2) for b in BOUNDS] == [1, 2, 2, 1, 1, 0, 0]
    assert [BC.tile_form(3, True, b, 9) for b in BOUNDS] == [1, 1, 1, 1, 1, 0, 0] and BC.tile_form(3, True, 2 ** 19 - 2, 9) == 2
    assert all(BC.tile_form(3, False, b, fan) == 0 for b in BOUNDS for fan in (0, 1, 2, 9))
    assert all(BC.tile_form(2, True, b, 0) == 0 and BC.tile_form(2, True, b, 1) <= 1 for b in BOUNDS)


# ---- sub-batches -----------------------------------------------------------------------------------------------------------------------
def series(factors, nslices=None):
    """what a tracker sweeps: the interval [t, t + 1] for every t but the last slice's, which is swept on its own"""
    n = len(factors)
    nslices = nslices or n
    return [Request("fast", t, t + 1 if t + 1 < nslices else -1, f) for t, f in enumerate(factors)]


def check_plan(nd, two_level, u_rows, requests, slices, plan):
    """what holds of every plan that was not refused; returns the replayed facts"""
    what = (nd, two_level, u_rows, requests, slices, plan)
    fast = [i for i, r in enumerate(requests) if r.mode == "fast"]
    assert [s for sb in plan.subs for s in sb.steps] == fast, what       # every fast request once, in order
    assert plan.tile_steps == [i for i, r in enumerate(requests) if r.mode != "fast"], what
    assert len(plan.subs) >= 1 and all(sb.steps for sb in plan.subs[1:]), what
    facts = list(slices)
    for sb in plan.subs:
        at_start = list(facts)
        assert len({j.slice for j in sb.jobs}) == len(sb.jobs), what     # no slice is built twice in one sub-batch
        for j in sb.jobs:
            assert not slices[j.slice].sparse, what                      # a masked halo slice is never rebuilt
            # in the sub-batch of the first step that needs it: a step of this sub-batch reads the slice under the job's factor, the
            # masks it found did not serve, and (below) every step of the sub-batches before had what it needed without the job
            needs = [s for s in sb.steps if j.slice in (requests[s].s0, requests[s].s1) and requests[s].factor == j.factor]
            assert needs and not valid(nd, at_start[j.slice], j.factor, two_level, u_rows), what
            facts[j.slice], rule_on = built(nd, facts[j.slice], j.factor, two_level, u_rows)
            assert j.rule_on == rule_on and j.big == (BC.big_threshold(nd, j.factor) if rule_on else math.inf), what
        # the sub-batch's masks are all built before its one cull: every step must find its slices served at its factor
        for s in sb.steps:
            r = requests[s]
            for sl in (r.s0, r.s1):
                assert sl < 0 or valid(nd, facts[sl], r.factor, two_level, u_rows), what
    assert plan.facts == facts, what                                     # the facts returned are the replay's
    return facts




def test_sub_batches_enumerated():
    """series of 1-2 requests over 2-3 slices in full, of 3-4 requests over 4-5 slices sampled (seeded), requests out of time order and
    ordinal-only ones included"""
    rng = random.Random(20260)
    cases = []
    for n in (1, 2):
        for fs in itertools.product((LOW, HIGH), repeat=n):
            for starts in itertools.product(STARTS, repeat=n + 1):
                cases.append((series(fs, n + 1), list(starts)))
    for n in (3, 4):
        for _ in range(2500):
            reqs = series([rng.choice((LOW, HIGH, HIGH)) for _ in range(n)], n + 1 if rng.random() < 0.7 else n)
            if rng.random() < 0.25:
                rng.shuffle(reqs)
            if rng.random() < 0.25:
                reqs = [r._replace(s1=-1) if rng.random() < 0.3 else r for r in reqs]
            cases.append((reqs, [rng.choice(STARTS) for _ in range(n + 1)]))
    refused = ok = multi = 0
    for k, (reqs, starts) in enumerate(cases):
        nd, two_level, u_rows = (2, True, 1) if k % 3 else (3, k % 2 == 0, 1 + 3 * (k % 2))
        plan = BC.plan_batch(nd, True, two_level, u_rows, reqs, starts)
        # the first request a sparse slice cannot serve, replaying the rules over the requests before it
        facts, first_refused = list(starts), -1
        for i, r in enumerate(reqs):
            need = [s for s in (r.s0, r.s1) if s >= 0 and not valid(nd, facts[s], r.factor, two_level, u_rows)]
            if any(facts[s].sparse for s in need):
                first_refused = i
                break
            for s in need:
                facts[s] = built(nd, facts[s], r.factor, two_level, u_rows)[0]
        if first_refused >= 0:
            assert (plan.status, plan.refused) == ("sparse_cannot_serve", first_refused), (reqs, starts, plan)
            assert all(not starts[j.slice].sparse for sb in plan.subs for j in sb.jobs)
            refused += 1
            continue
        assert plan.status == "ok" and plan.refused == -1, (reqs, starts, plan)
        assert check_plan(nd, two_level, u_rows, reqs, starts, plan) == facts
        ok += 1
        multi += len(plan.subs) > 1
        if len({r.factor for r in reqs}) == 1:
            assert len(plan.subs) == 1, (reqs, starts, plan)             # a constant-factor series is one sub-batch
    assert refused > 100 and ok > 1000 and multi > 100, (refused, ok, multi)


def test_the_series_whose_factor_changes_once():
    """[16384, 65536, 65536] over three slices whose maxima are not known: slice 1 is built under 16384 for the first step and again,
    in a second sub-batch, under 65536 -- exactly two sub-batches; with the maxima known (and small) one, and slice 1 built once"""
    reqs = series([LOW, HIGH, HIGH])
    for nd in (2, 3):
        plan = BC.plan_batch(nd, True, True, 1, reqs, [BC.NO_MASKS] * 3)
        assert plan.status == "ok" and len(plan.subs) == 2
        assert [(j.slice, j.factor, j.rule_on) for j in plan.subs[0].jobs] == [(0, LOW, True), (1, LOW, True)] and plan.subs[0].steps == [0]
        assert [(j.slice, j.factor, j.rule_on) for j in plan.subs[1].jobs] == [(1, HIGH, True), (2, HIGH, True)] and plan.subs[1].steps == [1, 2]
        check_plan(nd, True, 1, reqs, [BC.NO_MASKS] * 3, plan)
        known = [BC.NO_MASKS._replace(max_known=True, maxabs=SMALL)] * 3
        plan = BC.plan_batch(nd, True, True, 1, reqs, known)
        assert len(plan.subs) == 1 and [(j.slice, j.factor, j.rule_on) for j in plan.subs[0].jobs] == [(0, LOW, False), (1, LOW, False), (2, HIGH, False)]
        check_plan(nd, True, 1, reqs, known, plan)


def test_a_sparse_slice_serves_or_refuses_and_is_never_rebuilt():
    halo_ok, halo_big = masks(256, sparse=True, known=SMALL), masks(256, sparse=True, known=HUGE)
    reqs = series([LOW, LOW], 3)
    plan = BC.plan_batch(3, True, True, 1, reqs, [BC.NO_MASKS, BC.NO_MASKS, halo_ok])
    assert plan.status == "ok" and sorted(j.slice for sb in plan.subs for j in sb.jobs) == [0, 1] and plan.facts[2] == halo_ok
    plan = BC.plan_batch(3, True, True, 1, reqs, [BC.NO_MASKS, BC.NO_MASKS, halo_big])
    assert (plan.status, plan.refused) == ("sparse_cannot_serve", 1)
    plan = BC.plan_batch(3, True, True, 1, series([128, 128], 3), [BC.NO_MASKS, BC.NO_MASKS, halo_ok])      # a factor below the masks'
    assert (plan.status, plan.refused) == ("sparse_cannot_serve", 1)
    plan = BC.plan_batch(3, True, True, 4, reqs, [BC.NO_MASKS, BC.NO_MASKS, halo_ok])                       # summaries of another geometry
    assert (plan.status, plan.refused) == ("sparse_cannot_serve", 1)


# ---- tile runs -------------------------------------------------------------------------------------------------------------------------
def test_tile_runs():
    rng = random.Random(7)
    known = [Facts(False, False, False, 0, False, 1, True, m) for m in (0.5, 30.0, 4000.0, 3e6)] + [BC.NO_MASKS]
    for case in range(600):
        nd, robust, fan, walk = rng.choice((2, 3)), rng.random() < 0.8, rng.choice((0, 1, 2, 9)), rng.random() < 0.7
        nsl = rng.randint(2, 5)
        slices = [rng.choice(known) for _ in range(nsl)]
        reqs = []
        for _ in range(rng.randint(1, 7)):
            t = rng.randrange(nsl)
            reqs.append(Request(rng.choice(("tile", "tile", "tile_cull", "fast")), t, t + 1 if t + 1 < nsl and rng.random() < 0.8 else -1, rng.choice((3, 1000, LOW, 1 << 24))))
        plan = BC.plan_batch(nd, robust, True, 1, reqs, slices, tile_walk=walk, tile_fan=fan)
        assert plan.status == "ok"
        tiles = [i for i, r in enumerate(reqs) if r.mode != "fast"]
        assert plan.tile_steps == tiles

        def own_form(i):
            r = reqs[i]
            sl = [slices[s] for s in (r.s0, r.s1) if s >= 0]
            bound = max(s.maxabs for s in sl) * float(r.factor) if all(s.max_known for s in sl) else -1.0
            return form(nd, robust, bound, fan)
        # runs: consecutive tile requests (fast requests in between do not part them) with the same cull setting, maximal; one per request without the walk
        exp = []
        for k, i in enumerate(tiles):
            cull = int(reqs[i].mode == "tile_cull")
            if walk and exp and exp[-1][2] == cull:
                exp[-1][1] += 1
                exp[-1][4] = min(exp[-1][4], own_form(i))
            else:
                exp.append([k, 1, cull, fan, own_form(i)])
        assert [list(r) for r in plan.runs] == exp, (reqs, slices, walk, fan, plan.runs, exp)
        if not walk:
            assert len(plan.runs) == len(tiles)
        for a, b in zip(plan.runs, plan.runs[1:]):
            assert a.first + a.nsteps == b.first and (not walk or a.cull != b.cull)
        assert sum(r.nsteps for r in plan.runs) == len(tiles)


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
def check_layout(plan):
    L = BC.host()
    blocks = [(sb.job_off, len(sb.jobs) * L.sizeof_mask_job) for sb in plan.subs] + [(plan.fields_off, plan.nfields * L.sizeof_fields)]
    end = 0
    for off, size in blocks:                                   # multiples of 256, in order, none reaching into the next
        assert off % 256 == 0 and off >= end
        end = off + size
    assert plan.bytes == sum((size + 255) // 256 * 256 for _, size in blocks) and plan.bytes % 256 == 0 and plan.bytes >= end
    base = 0
    for sb in plan.subs:                                       # the steps of sub-batch i at step_base[i], back to back; the tile fields behind them
        assert sb.step_base == base
        base += len(sb.steps)
    assert plan.tile_base == base and plan.nfields == base + len(plan.tile_steps)


def test_layout():
    rng = random.Random(3)
    for case in range(400):
        nsl = rng.randint(2, 6)
        slices = [rng.choice(STARTS[:13]) for _ in range(nsl)]
        reqs = []
        for _ in range(rng.randint(1, 9)):
            t = rng.randrange(nsl)
            reqs.append(Request(rng.choice(("fast", "fast", "tile", "tile_cull")), t, t + 1 if t + 1 < nsl else -1, rng.choice((LOW, HIGH, 1 << 20))))
        plan = BC.plan_batch(2, True, True, 1, reqs, slices)
        assert plan.status == "ok"
        check_layout(plan)
    empty = BC.plan_batch(2, True, True, 1, [], [])
    assert empty.status == "ok" and empty.bytes == 0 and empty.nfields == 0 and len(empty.subs) == 1
    # sizes that cross a 256-byte boundary: 1 .. 12 jobs in one sub-batch
    L = BC.host()
    for n in range(1, 13):
        plan = BC.plan_batch(2, True, True, 1, [Request("fast", t, -1, LOW) for t in range(n)], [BC.NO_MASKS] * n)
        assert len(plan.subs) == 1 and len(plan.subs[0].jobs) == n and plan.fields_off == (n * L.sizeof_mask_job + 255) // 256 * 256
        check_layout(plan)


def test_the_request_count_limit():
    """a pass descriptor has 64 - 46 = 18 bits for the request's index: 2^18 fields are one too many, 2^18 - 1 are not"""
    L = BC.host()
    assert L.step_bits == 18
    for n, status in (((1 << 18) - 1, "ok"), (1 << 18, "too_many")):
        for mode in ("tile", "fast"):
            plan = BC.plan_batch(2, True, True, 1, [Request(mode, 0, 1, LOW)] * n, [masks(LOW, known=SMALL)] * 2)
            assert plan.status == status and plan.nfields == n, (n, mode, plan.status)
            if status == "ok":
                check_layout(plan)


# ---- key bits --------------------------------------------------------------------------------------------------------------------------
def test_key_bits():
    L = BC.host()
    exact64 = next(m for m in range(8) if m not in (L.tag_reference, L.tag_work_index))

    def exp(nd, sizes, steps):
        bound = (12 if nd == 2 else 60) * math.prod(sizes[:nd]) * steps
        return max(1, min(64, bound.bit_length()))             # the smallest b with 2^b > bound
    for nd in (2, 3):
        per = 12 if nd == 2 else 60
        for p in (10, 20, 31, 32, 40, 62):                     # bounds on either side of 2^p
            for delta in (-1, 0, 1):
                n0 = ((1 << p) + per - 1) // per + delta
                dom = [max(n0, 1), 1, 1]
                for t_max in (-1, 0, 5):                       # (t_max + 2) = 1: the bound is per x n0, straddling 2^p
                    assert BC.key_bits(exact64, nd, [7, 7, 7], dom, t_max) == exp(nd, dom, t_max + 2), (nd, p, delta, t_max)
                    assert BC.key_bits(L.tag_work_index, nd, dom, [9, 9, 9], t_max) == exp(nd, dom, 1), (nd, p, delta, t_max)      # t_max ignored
                    assert BC.key_bits(L.tag_reference, nd, dom, dom, t_max) == 64
        assert BC.key_bits(exact64, nd, [1, 1, 1], [1 << 30, 1 << 30, 1 << 30], 1 << 20) == 64
    assert BC.key_bits(exact64, 2, [1, 1, 1], [128, 96, 1], 2) == exp(2, [128, 96], 4) == 20


# ---- the verdict -----------------------------------------------------------------------------------------------------------------------
def expected_verdict(n, cap, any_fast, fast_cells, attempt):
    over = [x > c for x, c in zip(n, cap)]
    if not any(over):
        return "done", tuple(cap)
    if attempt == 4:
        return "give_up", None
    hits, listed, refined, fragile = n
    truncated = over[1] or over[2]
    if any_fast and truncated and (listed > fast_cells // 8 or refined * 8 > fast_cells // 8):
        return "replay_dense", (2 * hits + 1024 if over[0] else cap[0], cap[1], cap[2], cap[3])
    room = lambda x: x + x // 8 + 1024
    return "grow", (max(cap[0], room(hits), 2 * hits + 1024 if truncated else 0), room(listed) if over[1] else cap[1], room(refined) if over[2] else cap[2],
                    room(fragile) if over[3] else cap[3])


def test_overflow_verdict():
    cap = (65536, 1 << 20, 1 << 20, 4096)
    seen = set()
    for over in itertools.product((False, True), repeat=4):
        for excess in (1, 100000):
            n = tuple(c + excess if o else c - (c // 3) * (excess == 1) for c, o in zip(cap, over))
            # the dense test on both sides of fast_cells / 8, by the survivor list and by the refine list
            for fast_cells in (0, 8 * n[1] - 8, 8 * n[1], 8 * n[1] + 8, 64 * n[2] - 8, 64 * n[2], 64 * n[2] + 8, 1 << 40):
                for any_fast in (False, True):
                    for attempt in range(5):
                        what, want = BC.overflow_verdict(n, cap, any_fast, fast_cells, attempt)
                        ewhat, ewant = expected_verdict(n, cap, any_fast, fast_cells, attempt)
                        assert what == ewhat, (n, cap, any_fast, fast_cells, attempt, what, ewhat)
                        if ewant is not None:
                            assert want == ewant, (n, what, want, ewant)
                        assert (what == "give_up") == (any(over) and attempt == 4)
                        assert (what == "done") == (not any(over))
                        if what in ("grow", "replay_dense"):
                            assert all(w >= c for w, c in zip(want, cap))
                            if what == "grow":                 # everything that overflowed fits the next time, as far as the counts say
                                assert all(w >= x for w, x in zip(want, n))
                            else:
                                assert any_fast and (over[1] or over[2]) and want[1:] == cap[1:]
                        seen.add((what, over))
    assert {w for w, _ in seen} == {"done", "replay_dense", "grow", "give_up"}
    # the numbers themselves
    assert BC.overflow_verdict((76000, 5, 5, 0), cap, True, 1 << 20, 0) == ("grow", (76000 + 9500 + 1024, 1 << 20, 1 << 20, 4096))
    assert BC.overflow_verdict((70000, (1 << 20) + 8, 5, 0), cap, True, 1 << 40, 0) == ("grow", (2 * 70000 + 1024, (1 << 20) + 8 + (1 << 17) + 1 + 1024, 1 << 20, 4096))
    assert BC.overflow_verdict((1000, 5, 5, 5000), cap, True, 1 << 20, 3) == ("grow", (65536, 1 << 20, 1 << 20, 5000 + 625 + 1024))
    assert BC.overflow_verdict((70000, (1 << 20) + 8, 5, 0), cap, True, 1 << 22, 0) == ("replay_dense", (2 * 70000 + 1024, 1 << 20, 1 << 20, 4096))
    assert BC.overflow_verdict((1000, 5, (1 << 20) + 8, 0), cap, True, 1 << 26, 0)[0] == "replay_dense"        # refined x 8 > cells / 8
    assert BC.overflow_verdict((1000, 5, (1 << 20) + 8, 0), cap, True, 1 << 27, 0)[0] == "grow"
    assert BC.overflow_verdict((1000, 5, (1 << 20) + 8, 0), cap, False, 0, 0)[0] == "grow"                     # nothing fast: nothing to replay another way


def test_cull_verdict_keeps_its_own_numbers():
    """ftkx_sweep_cull: only the lists count, the survivor list doubles, the fourth overflow is the last"""
    lc, rc = 1 << 20, 1 << 20
    for over_l, over_r in itertools.product((False, True), repeat=2):
        listed, refined = lc + 7 if over_l else lc, rc + 9 if over_r else 17
        for attempt in range(4):
            what, want = BC.cull_verdict(listed, refined, lc, rc, attempt)
            if not (over_l or over_r):
                assert (what, want) == ("done", (lc, rc))
            elif attempt == 3:
                assert what == "give_up"
            else:
                assert (what, want) == ("grow", (2 * listed + 1024 if over_l else lc, refined + refined // 8 + 1024 if over_r else rc))
