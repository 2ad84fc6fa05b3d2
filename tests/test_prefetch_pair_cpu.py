"""The prefetch two updates ahead (``prefetch_plan`` in core/update_group.py, ``macjd_prefetch_batches`` in
include/macjd_nets.h) without a GPU: the plan's coverage, lead and staging-set hazards, the schedule of every form of a
captured group (``group_schedule``), its switch, and the new entry points' header / exports."""
import ctypes
import re
import os

import pytest

import __graft_entry__ as entry
from _harness import REPO

from macjd_amd import _native, options
from macjd_amd.core.qmix import prefetch_plan
from macjd_amd.core.update_group import GroupStep, group_schedule
from test_prefetch_launch_cpu import _draw


def _reads(u, n_sets):
    return u % n_sets


@pytest.mark.parametrize("K,ahead", [(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (20, 2), (20, 1)])
def test_plan_covers_every_update_once_in_time_and_without_a_staging_hazard(K, ahead):
    launches, n_sets = prefetch_plan(K, ahead)
    assert n_sets == 2 * ahead
    covered = [u for l in launches for u in l.updates]
    assert covered == list(range(1, K))                          # every update 1 .. K-1 exactly once, in order
    issued = [l.issue_at for l in launches]
    assert len(set(issued)) == len(issued) and issued == sorted(issued)   # at most one launch per issuing update
    for l in launches:
        assert 1 <= len(l.updates) <= ahead and len(l.updates) == len(l.offsets) == len(l.sets)
        assert list(l.updates) == list(range(l.updates[0], l.updates[0] + len(l.updates)))   # consecutive updates
        for u, off, s in zip(l.updates, l.offsets, l.sets):
            assert off == u - 1 and s == _reads(u, n_sets)       # update u's batch: the draw of offset u - 1, into its set
        a = l.updates[0]
        assert 0 <= l.issue_at <= a - 1                          # issued before its first consumer starts
        if ahead == 2 and a >= 3:
            assert l.issue_at <= a - 2                           # ... two updates before it in steady state
        # in flight from its issuing update to its last consumer: no other update of that span reads a set it writes
        for v in range(l.issue_at, l.updates[-1] + 1):
            if v not in l.updates:
                assert _reads(v, n_sets) not in l.sets, (l, v)
        # ... and a consumer reads only its own set of the launch's
        for u in l.updates:
            assert [s for s in l.sets if s == _reads(u, n_sets)] == [_reads(u, n_sets)]
        assert len(set(l.sets)) == len(l.sets)
    # a launch on the side stream runs behind the one before it: consumers are served in order
    firsts = [l.updates[0] for l in launches]
    assert firsts == sorted(firsts)
    if ahead == 2:
        assert [len(l.updates) for l in launches] == [2] * ((K - 1) // 2) + [1] * ((K - 1) % 2 if K > 1 else 0)


def test_ahead_one_is_the_plan_of_single_launches():
    launches, n_sets = prefetch_plan(20, 1)
    assert n_sets == 2 and len(launches) == 19
    for a, l in enumerate(launches, start=1):
        assert tuple(l) == (a - 1, (a,), (a - 1,), (a % 2,))
    with pytest.raises(ValueError):
        prefetch_plan(4, 3)


def test_pair_plan_of_a_group_of_twenty():
    launches, _ = prefetch_plan(20, 2)
    assert [(l.issue_at, l.updates) for l in launches[:4]] == [(0, (1, 2)), (1, (3, 4)), (3, (5, 6)), (5, (7, 8))]
    assert launches[-1].updates == (19,) and launches[-1].issue_at == 17 and launches[-1].offsets == (18,)


FORMS = {  # form -> (pipelined, one_launch, ahead of the schedule, ahead of the plan it must issue)
    "unpipelined": (False, False, 1, None), "four launches": (True, False, 1, 1), "four launches, ahead ignored": (True, False, 2, 1),
    "one launch, ahead 1": (True, True, 1, 1), "one launch, ahead 2": (True, True, 2, 2),
}


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 20])
@pytest.mark.parametrize("form", list(FORMS))
def test_group_schedule_serves_every_update_once_and_leaves_the_counter_of_k_draws(K, form):
    """``group_schedule`` walked the way the capture walks it, with the sampler's counter on the host: who prepares each
    update's batch, into which set, which optimiser launches draw at which offset, and what the counter and the drawn
    indices are afterwards — against K draws one behind the other."""
    pipelined, one_launch, ahead, plan_ahead = FORMS[form]
    steps, n_sets = group_schedule(K, pipelined, one_launch, ahead)
    assert len(steps) == K and all(isinstance(s, GroupStep) for s in steps)
    n, N, seed, c0 = 4, 33, 0x1234ABCD5678, 7
    seq = [_draw(n, N, c0 + i, seed) for i in range(K)]        # K sequential draws: the batches of updates 1 .. K-1, then
    counter, in_set, idx, drawn = c0, {}, None, []             # ... the batch the group leaves behind; counter c0 + K
    issued = []
    for u, s in enumerate(steps):
        assert 0 <= s.reads < n_sets
        if u == 0 or not pipelined:
            assert s.prefetched is False                       # prepares its own batch (from the index row as it stands)
        else:
            assert s.prefetched is True
            by = [l for l in issued if u in l.updates]
            assert len(by) == 1 and by[0].issue_at < u         # exactly one earlier update issued it
            assert by[0].sets[by[0].updates.index(u)] == s.reads and in_set.pop(s.reads) == u   # ... into the set it reads
        if s.issues is not None:
            l = s.issues
            assert pipelined and l.issue_at == u
            issued.append(l)
            for v, off, st in zip(l.updates, l.offsets, l.sets):
                assert st not in in_set and st != s.reads      # no set is overwritten before its reader, or under it
                in_set[st] = v
                if one_launch:                                 # reads the counter at its offset
                    drawn.append(_draw(n, N, counter + off, seed))
                else:                                          # the four launches: a draw of offset 0 that advances it
                    drawn.append(_draw(n, N, counter, seed))
                    counter += 1
        if s.draw is not None:                                 # the optimiser launch's draw: counter + offset, then + 1
            idx = _draw(n, N, counter + s.draw, seed)
            drawn.append(idx)
            counter += s.draw + 1
        if pipelined:
            assert (s.draw is not None) == (u == K - 1)        # only the last step draws ...
            if u == K - 1:
                assert s.draw == (K - 1 if one_launch else 0)  # ... at the closing offset of the form
        else:
            assert s.draw == 0 and s.issues is None and s.reads == 0
    assert not in_set                                          # every prefetched batch was consumed
    assert counter == c0 + K and drawn == seq and idx == seq[-1]
    if pipelined:
        assert issued == prefetch_plan(K, plan_ahead)[0] and n_sets == prefetch_plan(K, plan_ahead)[1]
    else:
        assert issued == [] and n_sets == 1


def test_switch_is_declared_and_documented():
    assert options._DEFAULTS["PREFETCH_AHEAD"] == "2"
    assert re.search(r"^\s+MACJD_PREFETCH_AHEAD\s+2 \| 1\s", options.__doc__, flags=re.M)


def test_multi_batch_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("macjd_prefetch_batches", "macjd_prefetch_batches_supported"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, plain) and sym in _native.EXPORTS
    assert re.search(r"#define\s+MACJD_PREFETCH_MAX_BATCHES\s+4\b", plain)
    from macjd_amd import ops
    assert ops.PREFETCH_MAX_BATCHES == 4
    entry.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "macjd_prefetch_batches") and hasattr(lib, "macjd_prefetch_batches_supported")
