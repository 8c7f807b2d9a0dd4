"""GPU: the reads of tests/test_hostcore_search_steps.py (2 000 C2 reads, 400 C4 reads, an 8 Mbp
genome) through gwa.Batch.  A text-mode state's child and its split / clip children run in one
micro-step, and a report reads a deferred state from the register cache without writing it back
(bsf_core.h searchStep / reportAlignment): the SAM text and the per-read counters stay the
oracle's, with the default tiers and with a 64-state first tier under a small scratch budget, where
most searches overflow, restart on the second tier and are suspended / resumed between micro-steps.
Needs an MI355X (`-m gpu`)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
import synth  # noqa: E402
from search_step_sets import SETS, genome, reads_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    import gwa
    codes, names, lengths = genome()
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths)
    oi = O.Index.from_arrays(codes, names, lengths)
    exp = {}
    for name in SETS:
        reads, k = reads_of(codes, lengths, name)
        sam, st = oi.align(reads, O.OrcConfig.default(k=k), with_stats=True)
        # numFMIndexSearches, FMQuickScan steps (cut at the (k+1)-th mismatch), DP verifications
        cols = np.array([[x.fm_searches, x.quick_steps_cut, x.sw] for x in st])
        exp[name] = (reads, k, sam, cols)
    return gi, oi, exp


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("name", ["c2", "c4"])
def test_sam_and_counters_equal_oracle(setup, monkeypatch, name, small):
    import gwa
    gi, oi, exp = setup
    reads, k, sam, cols = exp[name]
    if small:  # as test_gpu_parity.py::test_concurrent_batches_small_scratch_budget sets them
        monkeypatch.setenv("GWA_SCRATCH_BUDGET_MB", "256")
        monkeypatch.setenv("GWA_TIER_ARENA", "64")
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=k), reads)
    b.run()
    deep = sum(list(b.stats().tier_reads)[1:])
    c = b.read_counters()
    got = b.results()[0]
    b.close()
    # (GWA_TIER_ARENA sets the first tier of the k >= 4 kernels only: the k <= 3 first tier's size is
    # that of its LDS queue, and no C2 read of an i.i.d. genome outgrows it)
    if small and name == "c4":
        assert deep > 0  # the deep tiers ran
    assert got == sam
    for j, col in enumerate((1, 2, 16)):
        assert np.array_equal(c[:, col], cols[:, j]), (col, np.nonzero(c[:, col] != cols[:, j])[0][:5])


def test_sf_same_reads(setup):
    # -m sf shares the lane's arena, queue and verification code with -m bsf
    import gwa
    gi, oi, exp = setup
    reads, k, _, _ = exp["c2"]
    got = gwa.aligner(gi, gwa.AlignmentConfig(k=k, strategy="sf")).align_batch(reads)
    assert got == oi.align(reads, O.OrcConfig.default(k=k, strategy=1))
