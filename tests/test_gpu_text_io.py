"""GPU text I/O: the cooperative SAM write pass (batch_io.hip samWriteKernel: short fields per lane,
name / SEQ / QUAL copied by the workgroup in 16-B chunks), the 8-lanes-per-read code-row encode and
the reuse of a batch's length table by gwa_batch_run, byte for byte against the CPU oracle.  Needs
an MI355X (`-m gpu`)."""
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

DEFER_MIN = 16  # sam_core.h kSamDeferMin: fields of more bytes are left to the workgroup
READ_LENS = [1, 15, 16, 17, 31, 33, 100, 128, 129, 250]
NAME_LENS = [1, 7, 16, 17, 40]


@pytest.fixture(scope="module")
def small_pair():
    import gwa
    codes, names, lengths = synth.genome([("chr1", 60000), ("chr2", 40000)], 1)
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths)
    return codes, names, lengths, gi, O.Index.from_arrays(codes, names, lengths)


def _name(i, nl):
    return ("%d_" % i + "nameXYZ" * 6)[:nl] if nl > 1 else "abcdefghijklmnopqrstuvwxyz"[i % 26]


def shape_reads(codes, n, seed, lens=READ_LENS, plain=False):
    """n reads of mixed lengths and name lengths: both strands, every fifth one random (unmappable);
    unless plain, some without a quality, in lower case, with an N, with embedded spaces."""
    rng = np.random.default_rng(seed)
    L = len(codes)
    out = []
    for i in range(n):
        m = int(lens[int(rng.integers(0, len(lens)))])
        if i % 5 == 0:
            s = rng.integers(0, 4, m).astype(np.uint8)
        else:
            a = int(rng.integers(0, L - m))
            s = codes[a:a + m].copy()
            for j in rng.integers(0, m, int(rng.integers(0, 3))):
                if s[j] < 4:
                    s[j] = (s[j] + int(rng.integers(1, 4))) % 4
            if i % 2:
                s = synth.COMP[s[::-1]]
        txt = synth.SYM[s].tobytes().decode()
        qual = "".join(chr(c) for c in rng.integers(33, 74, m))
        if not plain:
            if i % 9 == 2 and m > 2:
                txt = txt[:m // 2] + "N" + txt[m // 2 + 1:]
            if i % 6 == 1:
                txt = txt.lower()
            if i % 8 == 5 and m > 4:
                txt = txt[:2] + " " + txt[2:m - 2] + "  " + txt[m - 2:]
            if i % 4 == 3:
                qual = None
        out.append((_name(i, NAME_LENS[int(rng.integers(0, len(NAME_LENS)))]), txt, qual))
    return out


def oracle_ok(oi, reads, **kw):
    """the reads the oracle aligns (above ~223 bp the reference throws on some reads)"""
    keep = []
    for r in reads:
        try:
            oi.align([r], O.OrcConfig.default(**kw))
            keep.append(r)
        except RuntimeError:
            pass
    return keep


@pytest.fixture(scope="module")
def shapes(small_pair):
    """130 reads of every field shape and their expected SAM (computed once, not modified)"""
    codes, names, lengths, gi, oi = small_pair
    reads = oracle_ok(oi, shape_reads(codes, 150, 3), k=2.0)[:130]
    assert len(reads) == 130
    return reads, oi.align(reads, O.OrcConfig.default(k=2.0))


def _same(got, exp):
    if got != exp:
        g, e = got.splitlines(), exp.splitlines()
        bad = [(a, b) for a, b in zip(g, e) if a != b][:3]
        raise AssertionError("SAM differs: %d vs %d lines; first diffs: %r" % (len(g), len(e), bad))


def _residues(reads, sam):
    """16-B residues of the deferred fields: their offsets in the SAM text (= in the staging buffer,
    whose start is 16-B aligned in the output) and the offsets of names and qualities in their blobs"""
    stage, src = set(), set()
    at = 0
    for line in sam.splitlines():
        f = line.split("\t")
        pos = 0
        for k, x in enumerate(f):
            if k in (0, 9, 10) and len(x) > DEFER_MIN:
                stage.add((at + pos) % 16)
            pos += len(x) + 1
        at += len(line) + 1
    no = qo = 0
    for name, seq, qual in reads:
        if len(name) > DEFER_MIN:
            src.add(no % 16)
        if qual is not None and len(qual) > DEFER_MIN:
            src.add(qo % 16)
        no += len(name)
        qo += len(qual) if qual is not None else 0
    return stage, src


def test_field_shapes_cover_every_residue(small_pair, shapes):
    import gwa
    codes, names, lengths, gi, oi = small_pair
    reads, exp = shapes
    # conditions on the inputs: every read and name length, reads without a quality, in lower case, with
    # N and with spaces, mapped on both strands and unmapped; deferred fields at every residue mod 16
    assert {len(r[1].replace(" ", "")) for r in reads} == set(READ_LENS)
    assert {len(r[0]) for r in reads} == set(NAME_LENS)
    assert any(r[2] is None for r in reads) and any(" " in r[1] for r in reads)
    assert any(r[1].islower() for r in reads) and any("N" in r[1] for r in reads)
    flags = {int(l.split("\t")[1]) & 0x14 for l in exp.splitlines()}
    assert flags >= {0, 0x10, 0x4}
    stage, src = _residues(reads, exp)
    assert stage == set(range(16)) and src == set(range(16)), (sorted(stage), sorted(src))
    _same(gwa.aligner(gi, gwa.AlignmentConfig(k=2.0)).align_batch(reads), exp)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_group_edges(small_pair, shapes, n):
    import gwa
    codes, names, lengths, gi, oi = small_pair
    reads = shapes[0][:n]
    _same(gwa.aligner(gi, gwa.AlignmentConfig(k=2.0)).align_batch(reads), oi.align(reads, O.OrcConfig.default(k=2.0)))


def test_small_stage_staged_next_to_direct(small_pair, shapes, monkeypatch):
    # GWA_SAM_STAGE=1024: the two full workgroups (64 records each, > 1 KiB) write directly, the last
    # one (3 records of 100-129 bp, < 1 KiB) stages its records and serves their deferred fields
    import gwa
    codes, names, lengths, gi, oi = small_pair
    reads = shapes[0][:128] + shape_reads(codes, 3, 8, lens=[100, 128, 129], plain=True)
    part = [oi.align(reads[a:b], O.OrcConfig.default(k=2.0)) for a, b in ((0, 64), (64, 128), (128, 131))]
    assert len(part[2]) + 16 <= 1024 < min(len(part[0]), len(part[1])) and len(part[2].splitlines()) == 3
    monkeypatch.setenv("GWA_SAM_STAGE", "1024")
    _same(gwa.aligner(gi, gwa.AlignmentConfig(k=2.0)).align_batch(reads), "".join(part))


def test_allhits_overflows_the_descriptor_list():
    # -R allhits on the many-equal-hits genome: reads with several lines push more bulk fields than
    # the workgroup's descriptor list holds, the rest are copied by their lanes next to deferred ones
    import gwa
    import genomes
    codes, names, lengths, reads = genomes.many_hits(n_reads=200)
    gi, oi = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths), O.Index.from_arrays(codes, names, lengths)
    exp = oi.align(reads, O.OrcConfig.default(k=5.0, report_type=1))
    per_group = [sum(1 for l in exp.splitlines() if int(l.split("\t")[0][1:]) // 64 == g) for g in range(4)]
    assert max(per_group) * 2 > 192, per_group  # SEQ + QUAL per line against 192 descriptors
    _same(gwa.aligner(gi, gwa.AlignmentConfig(k=5.0, reportType="allhits")).align_batch(reads), exp)
    gi.close()


def test_split_records_partial_ranges(small_pair):
    # chimeric reads at -s 1: split records print partial SEQ / QUAL ranges of both strands
    import gwa
    from test_hostcore import _mk
    codes, names, lengths, gi, oi = small_pair
    rng = np.random.default_rng(17)
    reads = [(n + "_chimeric_read", s, "".join(chr(c) for c in rng.integers(33, 74, len(s))))
             for n, s, q in _mk(codes, 150, 100, 2, True, seed=23)]
    exp = oi.align(reads, O.OrcConfig.default(k=0.1, num_split=1))
    split = [l.split("\t") for l in exp.splitlines() if int(l.split("\t")[1]) & 0x1]
    assert len(split) >= 20 and {int(f[1]) & 0x10 for f in split} == {0, 0x10}
    assert any(DEFER_MIN < len(f[9]) < 100 for f in split) and any(len(f[9]) <= DEFER_MIN for f in split)
    _same(gwa.aligner(gi, gwa.AlignmentConfig(k=0.1, numSplitAlowed=1)).align_batch(reads), exp)


def test_small_paired_batch(small_pair):
    import gwa
    codes, names, lengths, gi, oi = small_pair
    m1, m2 = synth.pairs_codes(codes, lengths, 70, config_id=58)
    s1, s2 = synth.to_strings(m1), synth.to_strings(m2)
    rng = np.random.default_rng(59)
    q = lambda: "".join(chr(c) for c in rng.integers(33, 74, 100))  # noqa: E731
    r1 = [("pair_with_a_long_name_%d/1" % i, s1[i], q()) for i in range(70)]
    r2 = [("p%d/2" % i, "".join(rng.choice(list("ACGT"), 100)) if i % 9 == 0 else s2[i], None if i % 7 == 0 else q())
          for i in range(70)]
    got = gwa.PairedEndAligner(gi, gwa.AlignmentConfig(k=2.0)).align_pairs(r1, r2)
    _same(got, oi.align_pairs(r1, r2, O.OrcConfig.default(k=2.0)))
    assert {int(l.split("\t")[1]) & 0x10 for l in got.splitlines()} == {0, 0x10}


def test_run_three_times_same_sam(small_pair, shapes):
    # gwa_batch_run keeps the batch's length table and rewrites the code rows from the text each run
    import gwa
    codes, names, lengths, gi, oi = small_pair
    reads, exp = shapes
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), reads)
    for _ in range(3):
        b.run()
        _same(b.results()[0], exp)
    b.close()


def test_second_batch_with_other_lengths(small_pair, shapes):
    # two live batches on one index, different read lengths: neither sees the other's length table
    import gwa
    codes, names, lengths, gi, oi = small_pair
    reads, exp = shapes
    other = shape_reads(codes, 97, 41, lens=[36, 50, 77, 101], plain=True)
    a = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), reads)
    a.run()
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), other)
    b.run()
    _same(b.results()[0], oi.align(other, O.OrcConfig.default(k=2.0)))
    a.run()
    _same(a.results()[0], exp)
    a.close()
    b.close()
    c = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), other[:40] + reads[:40])  # (may reuse the freed buffers)
    c.run()
    _same(c.results()[0], oi.align(other[:40] + reads[:40], O.OrcConfig.default(k=2.0)))
    c.close()


def test_fastq_text_path_equals_blob_path(small_pair, tmp_path):
    # the pipeline's batches are created from the FASTQ text itself (fields located on the device) and
    # run once; the same reads as blobs give the same bytes
    import gwa
    codes, names, lengths, gi, oi = small_pair
    reads = oracle_ok(oi, shape_reads(codes, 200, 77, plain=True), k=2.0)
    fq = tmp_path / "reads.fq"
    fq.write_text("".join("@%s\n%s\n+\n%s\n" % r for r in reads))
    pipe = gwa.Pipeline([gi], gwa.AlignmentConfig(k=2.0), batch_reads=64, workers_per_device=2)
    with open(tmp_path / "out.sam", "wb") as f:
        assert pipe.align_file(str(fq), f.fileno()) == len(reads)
    pipe.close()
    got = (tmp_path / "out.sam").read_text()
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), reads)
    b.run()
    blob = b.results()[0]
    b.close()
    _same(got, blob)
    _same(blob, oi.align(reads, O.OrcConfig.default(k=2.0)))
