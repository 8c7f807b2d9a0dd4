"""MD:Z written on the device (include/gwa.h GWA_SAM_TAG_MD, AlignmentConfig.mdTag, gwa_cli align --md).

The reference prints no MD, so every case checks two things: the GPU SAM with the MD fields removed is
the oracle's SAM byte for byte, and every mapped line's MD is what the rule gives for that printed line
(tests/md_ref.py).  The input is small and seeded: a 9.5 kb genome of three contigs, one with a 40-base
N run, and 40 / 64 / 100 / 129 / 300 bp reads with substitutions (N among them), 2-base insertions and
deletions, chimeras of two places and reads at and over the contig ends.  Each single-end case asserts
on the oracle's output that the lines it was written for are there (the sets differ by strategy: -m sf
reports no split chains, so it prints neither an S inside a CIGAR nor split records).  Above about
223 bp the reference throws on some reads (read length), which aborts its run: a case
aligns the 300 bp reads that the oracle aligns under that case's options."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]

import gwa  # noqa: E402
import md_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 11
LENGTHS = [("c1", 4000), ("c2", 3500), ("c3", 2000)]
NRUN = (1000, 1040)  # c2's N run (0-based, in the contig)
SYM = "ACGTN"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def make_genome():
    rng = np.random.Generator(np.random.PCG64(SEED))
    seqs = []
    for name, n in LENGTHS:
        s = "".join(SYM[c] for c in rng.integers(0, 4, n))
        if name == "c2":
            s = s[:NRUN[0]] + "N" * (NRUN[1] - NRUN[0]) + s[NRUN[1]:]
        seqs.append(s)
    return seqs


def make_reads(seqs, n, lens=(40, 64, 100, 129, 300), seed=SEED + 1):
    """n reads (name, bases, quality): plain, with an insertion or a deletion of two bases, chimeras of
    two places (other contig, same contig, the start of a contig), reads cut at and hanging over the
    contig ends (taken from the concatenated text, as the search sees it); then 0-2 substitutions, one
    in four of them an N; half of the reads reverse-complemented."""
    rng = np.random.Generator(np.random.PCG64(seed))
    text = "".join(seqs)
    starts = np.cumsum([0] + [len(s) for s in seqs])
    out = []

    def piece(c, a, m):
        return seqs[c][a:a + m]

    def anywhere(m):
        c = int(rng.integers(0, 3))
        return c, int(rng.integers(0, len(seqs[c]) - m + 1))

    for i in range(n):
        m = int(lens[i % len(lens)])
        kind = int(rng.integers(0, 10))
        if kind <= 2:
            c, a = anywhere(m)
            s = piece(c, a, m)
        elif kind == 3 and m >= 64:  # 2-base insertion
            c, a = anywhere(m)
            p = int(rng.integers(10, m - 12))
            s = piece(c, a, m)
            s = s[:p] + "".join(SYM[x] for x in rng.integers(0, 4, 2)) + s[p:m - 2]
        elif kind == 4 and m >= 64:  # 2-base deletion
            c, a = anywhere(m + 2)
            p = int(rng.integers(10, m - 12))
            s = piece(c, a, m + 2)
            s = s[:p] + s[p + 2:]
        elif kind == 5:  # chimera of two contigs
            h = int(m * (0.3 + 0.4 * rng.random()))
            c1, a1 = anywhere(h)
            c2 = (c1 + 1 + int(rng.integers(0, 2))) % 3
            a2 = int(rng.integers(0, len(seqs[c2]) - (m - h) + 1))
            s = piece(c1, a1, h) + piece(c2, a2, m - h)
        elif kind == 6:  # chimera of two places on one contig
            h = int(m * (0.3 + 0.4 * rng.random()))
            c1, a1 = anywhere(h)
            a2 = int(rng.integers(0, len(seqs[c1]) - (m - h) + 1))
            s = piece(c1, a1, h) + piece(c1, a2, m - h)
        elif kind == 7:  # the second part lies at the very start of a contig: POS - (first part) <= 0
            h = int(m * (0.25 + 0.2 * rng.random()))
            c1, a1 = anywhere(h)
            c2 = (c1 + 1) % 3
            s = piece(c1, a1, h) + piece(c2, int(rng.integers(0, 8)), m - h)
        elif kind == 8:  # over a contig end, from the concatenated text
            b = int(starts[1 + int(rng.integers(0, 2))])
            a = b - int(rng.integers(1, m))
            s = text[a:a + m]
        else:  # cut at a contig's end or start
            c = int(rng.integers(0, 3))
            s = piece(c, len(seqs[c]) - m, m) if rng.random() < 0.5 else piece(c, 0, m)
        s = list(s[:m].ljust(m, "A"))
        for _ in range(int(rng.integers(0, 3))):
            p = int(rng.integers(0, m))
            s[p] = "N" if rng.random() < 0.25 else SYM[(SYM.index(s[p]) + int(rng.integers(1, 4))) % 4] if s[p] != "N" else "A"
        s = "".join(s)
        if rng.random() < 0.5:
            s = revcomp(s)
        out.append(("r%d" % i, s, "".join(chr(33 + (7 * i + j) % 40) for j in range(m))))
    return out


def make_pairs(seqs, n, m=100, seed=SEED + 2):
    """n pairs of m-base mates from fragments of 250-350 bases: plain pairs, pairs whose second mate
    carries six substitutions (beyond k = 2: unmapped by itself, found by mate rescue), pairs whose
    second mate is random (stays unmapped), mates with a 2-base deletion."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m1, m2 = [], []
    for i in range(n):
        c = int(rng.integers(0, 3))
        f = int(rng.integers(250, 351))
        a = int(rng.integers(0, len(seqs[c]) - f - 2))
        frag = seqs[c][a:a + f + 2]
        x, y = frag[:m], revcomp(frag[f - m:f])
        kind = i % 6
        if kind == 1:
            y = list(y)
            for p in (5, 20, 37, 55, 71, 90):
                y[p] = SYM[(SYM.index(y[p]) + 1) % 4] if y[p] != "N" else "A"
            y = "".join(y)
        elif kind == 2:
            y = "".join(SYM[v] for v in rng.integers(0, 4, m))
        elif kind == 3:
            x = frag[:40] + frag[42:m + 2]
        elif kind == 4:
            x = x[:50] + "N" + x[51:]
        if rng.random() < 0.5:
            x, y = y, x
        q = "I" * m
        m1.append(("p%d" % i, x, q))
        m2.append(("p%d" % i, y, q))
    return m1, m2


def cigar_ops(c):
    return re.findall(r"(\d+)([MIDNSHPX=])", c)


def ref_len(c):
    return sum(int(n) for n, op in cigar_ops(c) if op in "MDNX=")


def claims(sam, contigs):
    """what the lines of an oracle SAM exercise: the set of forms present"""
    have = set()
    lines = [l.split("\t") for l in sam.splitlines()]
    for k, f in enumerate(lines):
        flag = int(f[1])
        if flag & 0x4:
            have.add("unmapped")
            continue
        ops = cigar_ops(f[5])
        if any(op == "D" for _, op in ops):
            have.add("D")
        if any(op == "I" for _, op in ops):
            have.add("I")
        if any(op == "S" for _, op in ops[1:-1]):
            have.add("midS")
        if int(f[3]) <= 0:
            have.add("pos<=0")
        if f[2] in contigs and int(f[3]) + ref_len(f[5]) - 1 > len(contigs[f[2]]):
            have.add("past end")
        if flag & 0x10:
            have.add("reverse")
        # a record and its split record: FLAG 0x1 | 0x40 with RNEXT set, then the same read with 0x1 | 0x80
        if flag & 0x41 == 0x41 and f[6] != "*" and k + 1 < len(lines) and lines[k + 1][0] == f[0] \
                and int(lines[k + 1][1]) & 0xC1 == 0x81:
            have.add("split")
        if flag & 0x8:
            have.add("mate unmapped")
    return have


SINGLE = {
    "bsf_k2": (dict(k=2.0), dict(k=2.0), {"D", "I", "midS", "reverse", "split"}),
    "bsf_k5_allhits": (dict(k=5.0, reportType="allhits"), dict(k=5.0, report_type=1), {"D", "I", "midS", "reverse", "split"}),
    "sf_k5": (dict(k=5.0, strategy="sf"), dict(k=5.0, strategy=1), {"D", "I", "reverse"}),
    "k01_s1": (dict(k=0.1, numSplitAlowed=1), dict(k=0.1, num_split=1), {"D", "I", "midS", "reverse", "split"}),
}
N_READS = 600
N_PAIRS = 240


class World:
    def __init__(self):
        import oracle as O
        self.O = O
        self.seqs = make_genome()
        self.names = [n for n, _ in LENGTHS]
        self.contigs = dict(zip(self.names, self.seqs))
        self.fasta = "".join(">%s\n%s\n" % x for x in zip(self.names, self.seqs))
        self.reads = make_reads(self.seqs, N_READS)
        self.m1, self.m2 = make_pairs(self.seqs, N_PAIRS)
        self.oi = O.Index.from_fasta(self.fasta)
        self.fm = gwa.FMIndexOnGenome.buildFromFasta(self.fasta, device=0)
        self._orc, self._gpu, self._reads = {}, {}, {}

    def reads_of(self, case):
        """the case's reads: all short ones, and the 300 bp reads on which the oracle does not throw"""
        if case not in self._reads:
            cfg = self.O.OrcConfig.default(**SINGLE[case][1])
            keep = []
            for r in self.reads:
                if len(r[1]) > 223:
                    try:
                        self.oi.align([r], cfg)
                    except RuntimeError:
                        continue
                keep.append(r)
            self._reads[case] = keep
        return self._reads[case]

    def oracle(self, case):
        if case not in self._orc:
            if case == "pairs":
                self._orc[case] = self.oi.align_pairs(self.m1, self.m2, self.O.OrcConfig.default(k=2.0))
            else:
                self._orc[case] = self.oi.align(self.reads_of(case), self.O.OrcConfig.default(**SINGLE[case][1]), threads=8)
        return self._orc[case]

    def gpu(self, case):
        """the MD-on SAM of a case, computed once and shared"""
        if case not in self._gpu:
            if case == "pairs":
                self._gpu[case] = gwa.PairedEndAligner(self.fm, gwa.AlignmentConfig(k=2.0, mdTag=True)).align_pairs(self.m1, self.m2)
            else:
                cfg = gwa.AlignmentConfig(mdTag=True, **SINGLE[case][0])
                self._gpu[case] = gwa.aligner(self.fm, cfg).align_batch(self.reads_of(case))
        return self._gpu[case]

    def check(self, sam, oracle_sam):
        assert md_ref.strip_md(sam) == oracle_sam
        return md_ref.check_sam(sam, self.contigs)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.fm.close()


@pytest.mark.parametrize("case", list(SINGLE))
def test_single_end_md(world, case):
    exp = world.oracle(case)
    have = claims(exp, world.contigs)
    need = set(SINGLE[case][2])
    assert need <= have, (case, sorted(need - have))
    assert have & {"pos<=0", "past end"}, (case, sorted(have))
    reads = world.reads_of(case)
    assert {len(r[1]) for r in reads} == {40, 64, 100, 129, 300}
    n = world.check(world.gpu(case), exp)
    assert n > len(reads) // 2


def test_paired_end_md(world):
    exp = world.oracle("pairs")
    have = claims(exp, world.contigs)
    assert {"D", "reverse", "unmapped", "mate unmapped"} <= have, sorted(have)
    # pairs whose second mate is found by the rescue only: unmapped as a single-end read at this k
    single = world.oi.align([world.m2[i] for i in range(1, N_PAIRS, 6)] + [world.m1[i] for i in range(1, N_PAIRS, 6)],
                            world.O.OrcConfig.default(k=2.0))
    lone = {l.split("\t")[0] for l in single.splitlines() if int(l.split("\t")[1]) & 0x4}
    rescued = [l for l in exp.splitlines() if l.split("\t")[0] in lone and int(l.split("\t")[1]) & 0x2]
    assert rescued, "no pair needed mate rescue"
    assert world.check(world.gpu("pairs"), exp) > N_PAIRS


@pytest.mark.parametrize("env", [("GWA_SAM_STAGE", "1024"), ("GWA_SAM_DEFER", "0")])
def test_direct_write_and_no_deferral(world, monkeypatch, env):
    # a 1 KiB stage: the 64 reads of most workgroups do not fit and are written directly, lines with
    # long MD values among them; no deferral: every lane copies its own bulk fields
    want = world.gpu("bsf_k5_allhits")
    monkeypatch.setenv(*env)
    cfg = gwa.AlignmentConfig(mdTag=True, **SINGLE["bsf_k5_allhits"][0])
    got = gwa.aligner(world.fm, cfg).align_batch(world.reads_of("bsf_k5_allhits"))
    assert got == want
    world.check(got, world.oracle("bsf_k5_allhits"))


def test_results_range_select_format_and_records(world):
    case = "bsf_k2"
    full = world.gpu(case)
    reads = world.reads_of(case)
    n = len(reads)
    b = gwa.Batch(world.fm, gwa.AlignmentConfig(mdTag=True, **SINGLE[case][0]), reads=reads)
    try:
        b.run()
        sam, off = b.results()
        assert sam == full
        off = [int(x) for x in off]
        for first, count in ((0, 1), (63, 66), (n - 5, 5)):
            part, _ = b.results(first, count)
            assert part == sam[off[first]:off[first + count]]
        idx = [n - 1, 0, 64, 63, 200, 7]
        sel, _ = b.results_select(idx)
        assert sel == "".join(sam[off[i]:off[i + 1]] for i in idx)
        # gwa_batch_format + gwa_batch_sam_copy: the same text in HBM
        import torch
        assert b.format_device() == len(sam)
        assert bytes(b.sam_device().cpu().numpy().tobytes()).decode() == sam
        # gwa_results_records: md_off / md_len index the tag's value, 0 / 0 where the line has none
        text, recs = b.records(world.fm)
        lines = text.splitlines()
        assert len(recs) == len(lines)
        with_md = 0
        for r, line in zip(recs, lines):
            want = md_ref.md_of(line, world.contigs)
            if want is None:
                assert (r.md_off, r.md_len) == (0, 0)
            else:
                assert text[r.md_off:r.md_off + r.md_len] == want
                assert text[r.md_off - 5:r.md_off] == "MD:Z:"
                with_md += 1
        assert 0 < with_md < len(lines)
    finally:
        b.close()


def test_md_off_by_default(world):
    cfg = gwa.AlignmentConfig(**SINGLE["bsf_k2"][0])
    assert not cfg.mdTag and cfg._c().sam_tags == 0
    sam = gwa.aligner(world.fm, cfg).align_batch(world.reads_of("bsf_k2"))
    assert "MD:Z:" not in sam and sam == world.oracle("bsf_k2")
    b = gwa.Batch(world.fm, cfg, reads=world.reads_of("bsf_k2")[:50])
    try:
        b.run()
        _, recs = b.records(world.fm)
        assert recs and all((r.md_off, r.md_len) == (0, 0) for r in recs)
    finally:
        b.close()


def test_pipeline_files_equal_batches(world, tmp_path):
    cfg = gwa.AlignmentConfig(k=2.0, mdTag=True)
    fq = tmp_path / "reads.fq"
    reads = world.reads_of("bsf_k2")
    fq.write_text("".join("@%s\n%s\n+\n%s\n" % r for r in reads))
    f1, f2 = tmp_path / "m_1.fq", tmp_path / "m_2.fq"
    f1.write_text("".join("@%s\n%s\n+\n%s\n" % r for r in world.m1))
    f2.write_text("".join("@%s\n%s\n+\n%s\n" % r for r in world.m2))
    pipe = gwa.Pipeline([world.fm], cfg, batch_reads=97)
    try:
        out = tmp_path / "out.sam"
        with open(out, "wb") as f:
            assert pipe.align_file(str(fq), f.fileno()) == len(reads)
        assert out.read_text() == world.gpu("bsf_k2")
        with open(out, "wb") as f:
            assert pipe.align_pair_files(str(f1), str(f2), f.fileno()) == N_PAIRS
        assert out.read_text() == world.gpu("pairs")
        assert pipe.align_batch(reads) == world.gpu("bsf_k2")
        assert pipe.align_pairs(world.m1, world.m2) == world.gpu("pairs")
    finally:
        pipe.close()


def test_unknown_tag_bit_is_rejected(world):
    c = gwa.AlignmentConfig(k=2.0)._c()
    c.sam_tags = 2
    keep = []
    r = gwa._reads_struct(world.reads[:3], keep)
    L = gwa.lib()
    res, h = gwa._Results(), ctypes.c_void_p()
    msg = "gwa_config_t.sam_tags: unknown bits 0x2"
    assert L.gwa_align_batch(world.fm.h, ctypes.byref(c), ctypes.byref(r), ctypes.byref(res)) != 0
    assert L.gwa_last_error().decode().startswith(msg)
    assert L.gwa_batch_create(world.fm.h, ctypes.byref(c), ctypes.byref(r), ctypes.byref(h)) != 0
    assert L.gwa_last_error().decode().startswith(msg)
    assert L.gwa_batch_create_pairs(world.fm.h, ctypes.byref(c), ctypes.byref(r), ctypes.byref(r), 210, 390, ctypes.byref(h)) != 0
    assert L.gwa_last_error().decode().startswith(msg)
    assert L.gwa_align_pairs(world.fm.h, ctypes.byref(c), ctypes.byref(r), ctypes.byref(r), 210, 390, ctypes.byref(res)) != 0
    assert L.gwa_last_error().decode().startswith(msg)
    arr = (ctypes.c_void_p * 1)(world.fm.h.value if hasattr(world.fm.h, "value") else world.fm.h)
    assert L.gwa_pipeline_open(ctypes.cast(arr, ctypes.c_void_p), 1, ctypes.byref(c), 100, 0, ctypes.byref(h)) != 0
    assert L.gwa_last_error().decode().startswith(msg)
    c.sam_tags = 0x80000001
    assert L.gwa_batch_create(world.fm.h, ctypes.byref(c), ctypes.byref(r), ctypes.byref(h)) != 0
    assert L.gwa_last_error().decode().startswith("gwa_config_t.sam_tags: unknown bits 0x80000000")


def test_cli_md_on_the_fixture_reads(tmp_path):
    """gwa_cli align --md over tests/golden/fixtures/reads_c1.fq.snap (400 reads of the snap_reads genome):
    the header and, tags stripped, the oracle's lines; every MD the rule's; without --md no MD"""
    import io
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gwa_cli
    import oracle as O
    import snap_reads
    import synth
    codes, names, lengths = snap_reads.genome()
    text = synth.fasta_text(codes, names, lengths)
    ref = tmp_path / "ref.fa"
    ref.write_text(text)
    contigs, off = {}, 0
    for nm, n in zip(names, lengths):
        contigs[nm] = "".join(SYM[c] for c in codes[off:off + int(n)])
        off += int(n)
    reads_path = os.path.join(HERE, "golden", "fixtures", "reads_c1.fq.snap")
    reads = list(gwa_cli.reads_of(reads_path))
    oi = O.Index.from_fasta(text)
    exp = oi.sam_header() + oi.align(reads, O.OrcConfig.default(k=2.0))
    outs = {}
    for md in (True, False):
        out = io.StringIO()
        argv = ["align", "-r", str(ref), "-k", "2", "--batch", "64"] + (["--md"] if md else []) + [reads_path]
        assert gwa_cli.align(gwa_cli.build_parser().parse_args(argv), out=out) == len(reads)
        outs[md] = out.getvalue()
    assert outs[False] == exp and md_ref.strip_md(outs[True]) == exp
    body = "".join(l + "\n" for l in outs[True].splitlines() if not l.startswith("@"))
    assert md_ref.check_sam(body, contigs) > 300
