"""`.bam` read files at the CLI, as far as no device is needed (tests/test_cli.py's approach): the suffix is
accepted, the host-side reader gives the reads of the reference, and --shard refuses the file before an index
is built.  The aligned output is compared in tests/test_gpu_bam_in.py."""
import io
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "genome-weaver-align_amd"))

import gwa  # noqa: E402
import gwa_cli  # noqa: E402
import ubam_ref as U  # noqa: E402


def test_kind_accepts_bam():
    assert gwa_cli._kind("reads.bam") == "bam"
    assert gwa_cli._kind("dir.bam/reads.fq") == "fastq"
    with pytest.raises(gwa.GwaError, match="Unsupported file type"):
        gwa_cli._kind("reads.sam")


def test_reads_of_a_bam_file(tmp_path):
    recs = U.random_records(300, seed=12)
    p = tmp_path / "reads.bam"
    p.write_bytes(U.bam_file(recs, "@CO\tx\n", [("chr1", 1000)]))
    assert list(gwa_cli.reads_of(str(p))) == U.reads_of(recs)


def test_shard_refuses_a_bam_file(tmp_path):
    p = tmp_path / "reads.bam"
    p.write_bytes(U.bam_file(U.random_records(10)))
    ns = gwa_cli.build_parser().parse_args(["align", "-r", str(tmp_path / "missing.fa"), "--shard", "0/2", str(p)])
    with pytest.raises(gwa.GwaError, match="a sharded run needs an uncompressed read file"):
        gwa_cli.align(ns, out=io.StringIO())
