"""The search's micro-steps and its register cache (bsf_core.h searchStep / reportAlignment) on the
CPU build of the kernel logic, against the oracle: a text-mode state's child and its split / clip
children in one step, and reports that read a deferred state from the cache and never write it.

Both only change when a lane does a piece of work and which copies of a state exist, so the SAM
text and the per-read counts (FM searches, quick-scan steps, deepest queue, states created) must be
the oracle's, on every tier and across suspend / resume.  The host build also aborts if a deferred
state that is reported is still named by a queue entry (the claim its dropped write-back rests on)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostcore"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
import synth  # noqa: E402
import hostcore  # noqa: E402

from search_step_sets import SETS, genome, reads_of  # noqa: E402


@pytest.fixture(scope="module")
def setup():
    codes, names, lengths = genome()
    oi = O.Index.from_arrays(codes, names, lengths)
    hc = hostcore.HostCore(codes, names, lengths)
    exp = {}
    for name in SETS:
        reads, k = reads_of(codes, lengths, name)
        sam, st = oi.align(reads, O.OrcConfig.default(k=k), with_stats=True)
        cols = np.array([[x.fm_searches, x.quick_steps_cut, x.max_heap, x.states] for x in st])
        exp[name] = (reads, k, sam, cols)
    return hc, exp


# suspend: the first two tiers shrunk to 24 states (as test_hostcore.py::test_suspend_resume_across_tiers
# does), so most searches restart on the second tier and are suspended there between micro-steps
@pytest.mark.parametrize("suspend", [False, True])
@pytest.mark.parametrize("name", ["c2", "c4"])
def test_sam_and_counts_equal_oracle(setup, monkeypatch, name, suspend):
    hc, exp = setup
    reads, k, sam, cols = exp[name]
    if suspend:
        monkeypatch.setenv("HC_T0_ARENA", "24")
        monkeypatch.setenv("HC_T1_ARENA", "24")
    s0 = hostcore.suspends()
    got, st = hc.align(reads, k=k, stats=True)
    if suspend:
        assert hostcore.suspends() - s0 >= 100
    assert got == sam
    # FM searches, quick-scan steps (cut at the (k+1)-th mismatch, as the device scans), deepest queue
    for j in range(3):
        assert np.array_equal(st[:, j], cols[:, j]), (j, np.nonzero(st[:, j] != cols[:, j])[0][:5])
    # states created: the run-ahead over text-mode match runs keeps its intermediate states in
    # registers and never allocates them, so that count is the oracle's only with the run-ahead off
    monkeypatch.setenv("GWA_RUNAHEAD", "0")
    got0, st0 = hc.align(reads, k=k, stats=True)
    assert got0 == sam
    assert np.array_equal(st0, cols), [np.nonzero(st0[:, j] != cols[:, j])[0][:5] for j in range(4)]
