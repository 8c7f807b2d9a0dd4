"""What building BAM records on the device costs next to the SAM text (GPU box): one resident index, the C2
reads (100 bp, 0-2 substitutions, constant qualities) in one batch, aligned once; then, alternately and
`--steps` times each, gwa_batch_format (SAM text), gwa_batch_format_bgzf (text + BGZF), gwa_batch_format_bam
(records) and gwa_batch_results_bam (records + BGZF, the blocks copied out).  Prints median (min-max) of
format_ms, bam_ms and of compress_ms for both containers, and the bytes per read of all four outputs.

  python tools/bam_cost.py [--genome hg19|hg19r|<Mbp>] [--reads N] [--steps K] [--md]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "genome-weaver-align_amd")]


def say(*a):
    print("[bam_cost]", *a, flush=True)


def stat(v):
    v = sorted(v)
    return "%.3f (%.3f-%.3f)" % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="200")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import gwa
    import synth
    m, n = 100, args.reads
    t0 = time.time()
    if args.genome in ("hg19", "hg19r"):
        gen = synth.genome_repeats if args.genome == "hg19r" else synth.genome_ngaps
        codes, names, lengths = gen(synth.HG19_CONTIGS, config_id=1)
    else:
        codes, names, lengths = synth.genome([("chr1", int(float(args.genome) * 1e6))], 1)
    seqs = synth.reads_codes(codes, lengths, n, m, 2, config_id=2)
    seq_blob = synth.SYM[seqs].tobytes()
    del seqs
    off = np.arange(0, m * (n + 1), m, dtype=np.uint64)
    nb, no = synth.name_blob(n)
    blobs = (nb, no, seq_blob, off, b"I" * (m * n), off)
    say("genome + %d reads in %.0fs" % (n, time.time() - t0))
    t0 = time.time()
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths)
    del codes
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0, mdTag=args.md), blobs=blobs)
    b.run()
    say("index + batch aligned in %.0fs" % (time.time() - t0))
    sam_ms, bam_ms, sam_z_ms, bam_z_ms = [], [], [], []
    for rep in range(args.steps + 1):
        sam = b.format_device()
        st = b.stats()
        if rep:
            sam_ms.append(st.format_ms)
        sam_z = b.format_bgzf()
        st = b.stats()
        if rep:
            sam_z_ms.append(st.compress_ms)
        bam = b.format_bam()
        st = b.stats()
        if rep:
            bam_ms.append(st.bam_ms)
        bam_z = len(b.results_bam())
        st = b.stats()
        if rep:
            bam_z_ms.append(st.compress_ms)
            bam_ms.append(st.bam_ms)
    say("SAM text:     format_ms %s, %d bytes, %.1f per read" % (stat(sam_ms), sam, sam / n))
    say("BAM records:  bam_ms    %s, %d bytes, %.1f per read (%.3f of SAM)" % (stat(bam_ms), bam, bam / n, bam / sam))
    say("SAM as BGZF:  compress_ms %s, %d bytes, %.1f per read" % (stat(sam_z_ms), sam_z, sam_z / n))
    say("BAM as BGZF:  compress_ms %s, %d bytes, %.1f per read (%.3f of the SAM blocks), %d blocks (%d stored)"
        % (stat(bam_z_ms), bam_z, bam_z / n, bam_z / sam_z, st.bgzf_blocks, st.bgzf_stored))
    b.close()
    gi.close()


if __name__ == "__main__":
    main()
