"""The midpoint Occ-block layout on the GPU: the device index build (occLocal / occCounts), the
device loadBlock / finishBlock and the k-mer table kernel, on genomes whose BWT ends at every kind
of place in its last block and whose blocks hold N in one half, the other, both or neither.

Genomes: 129, 192, 193 and 1000 bases (text ending just past a block edge, on a half-block edge,
just past it, and mid-block), each as random ACGT, with N as the last character, and with scattered
N plus an N run; one 20 kb genome with three N runs (long enough for a k-mer table).  (An all-A text
is periodic, which the index build refuses, so it stays with the CPU test, tests/test_rank_layout.py.)
Reads: every 30-mer of the genome on both strands, and the same reads with 1 and 2 substitutions.
Each case runs -m bsf -k 2 and -m sf -k 2; the SAM text and, for -m bsf, the per-read counters
(fm_searches, quick-scan steps, DP verifications) must equal the CPU oracle's, as in
tests/test_gpu_parity.py.  Needs an MI355X (`-m gpu`)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

M = 30


def _genome(n, kind):
    rng = np.random.default_rng(1000 * n + len(kind))
    codes = rng.integers(0, 4, n).astype(np.uint8)
    if kind == "endN":
        codes[-1] = 4
    elif kind == "runN":
        codes[rng.integers(0, n, 3)] = 4
        run = int(rng.integers(2, 12 if n < 1000 else 70))
        at = int(rng.integers(0, n - run))
        codes[at:at + run] = 4
    elif kind == "runs3":
        for at, run in ((1500, 200), (9000, 37), (n - 300, 300)):  # the last one ends the text
            codes[at:at + run] = 4
        codes[rng.integers(0, n, 8)] = 4
    return codes


def _reads(codes):
    """every M-mer on both strands, then each with 1 and with 2 substitutions"""
    rng = np.random.default_rng(len(codes))
    n = len(codes) - M + 1
    win = np.lib.stride_tricks.sliding_window_view(codes, M)[:n]
    base = np.concatenate([win, synth.COMP[win[:, ::-1]]])
    out = [base]
    for subs in (1, 2):
        s = base.copy()
        for _ in range(subs):
            j = rng.integers(0, M, len(s))
            r = np.arange(len(s))
            v = s[r, j]
            s[r, j] = np.where(v < 4, (v + rng.integers(1, 4, len(s))) % 4, v)
        out.append(s)
    allr = np.concatenate(out)
    return [("r%d" % i, synth.SYM[allr[i]].tobytes().decode(), None) for i in range(len(allr))]


_CACHE = {}


def _case(n, kind):
    """genome, reads and the oracle's answers, computed once per genome"""
    key = (n, kind)
    if key not in _CACHE:
        codes = _genome(n, kind)
        reads = _reads(codes)
        oi = O.Index.from_arrays(codes, ["g"], [n])
        exp = {}
        sam, st = oi.align(reads, O.OrcConfig.default(k=2.0), with_stats=True, threads=8)
        exp["bsf"] = sam
        exp["stats"] = (np.array([x.fm_searches for x in st]), np.array([x.quick_steps_cut for x in st]),
                        np.array([x.sw for x in st]))
        exp["sf"] = oi.align(reads, O.OrcConfig.default(k=2.0, strategy=1), threads=8)
        _CACHE[key] = (codes, reads, exp)
    return _CACHE[key]


def _check(gi, reads, exp):
    import gwa
    for strat in ("bsf", "sf"):
        b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0, strategy=strat), reads)
        b.run()
        got = b.results()[0]
        c = b.read_counters()
        b.close()
        if got != exp[strat]:
            g, e = got.splitlines(), exp[strat].splitlines()
            bad = [(a, x) for a, x in zip(g, e) if a != x][:3]
            raise AssertionError("-m %s: SAM differs: %d vs %d lines; first diffs: %r" % (strat, len(g), len(e), bad))
        if strat == "bsf":
            fm, qs, sw = exp["stats"]
            assert np.array_equal(c[:, 1], fm), np.nonzero(c[:, 1] != fm)[0][:5]
            assert np.array_equal(c[:, 2], qs), np.nonzero(c[:, 2] != qs)[0][:5]
            assert np.array_equal(c[:, 16], sw), np.nonzero(c[:, 16] != sw)[0][:5]


SMALL = [(n, kind) for n in (129, 192, 193, 1000) for kind in ("acgt", "endN", "runN")]


@pytest.mark.parametrize("n,kind", SMALL + [(20000, "runs3")])
def test_rank_layout_matches_oracle(n, kind):
    import gwa
    codes, reads, exp = _case(n, kind)
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, ["g"], [n])
    try:
        _check(gi, reads, exp)
    finally:
        gi.close()


@pytest.mark.parametrize("n,kind", [(193, "runN"), (1000, "runN"), (20000, "runs3")])
def test_plain_mode_matches_oracle(monkeypatch, n, kind):
    # GWA_OCC_PLAIN=1: the index is built without has-N bits and every rank reads the N quarter, as
    # an index whose symbol counts reach 2^31 is
    import gwa
    codes, reads, exp = _case(n, kind)
    monkeypatch.setenv("GWA_OCC_PLAIN", "1")
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, ["g"], [n])
    monkeypatch.delenv("GWA_OCC_PLAIN")
    try:
        _check(gi, reads, exp)
    finally:
        gi.close()


def test_saved_index_gives_the_same_sam(tmp_path):
    # gwa_index_save -> gwa_index_open: the saved file holds no Occ blocks, the open rebuilds them
    import gwa
    n, kind = 20000, "runs3"
    codes, reads, exp = _case(n, kind)
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, ["g"], [n])
    path = str(tmp_path / "g.gwa.idx")
    gi.save(path)
    gi.close()
    gi2 = gwa.FMIndexOnGenome.load(path)
    try:
        _check(gi2, reads, exp)
    finally:
        gi2.close()
