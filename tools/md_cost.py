"""What the MD:Z tag costs the device SAM writer (GPU box): one resident index, the C2 reads (100 bp,
0-2 substitutions) in two batches that differ only in AlignmentConfig.mdTag, each aligned once; then
gwa_batch_format of the two alternately.  Prints format_ms and the SAM bytes of each, the bytes the
tag adds, and the floor of the extra work at the DESIGN.md §4 gather rates: the MD bytes written, plus
one 8-B text word and one 8-B N word per 32 bases of every mapped line's window, in both passes (the
length pass walks the window too).

  python tools/md_cost.py [--genome hg19|hg19r|<Mbp>] [--reads N] [--steps K]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "genome-weaver-align_amd")]

WORDS_PER_S = 48e9      # random 8-B words
STREAM_B_PER_S = 6.0e12  # a streaming kernel's bytes


def say(*a):
    print("[md_cost]", *a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="hg19")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
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
    bs = {}
    for md in (False, True):
        b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0, mdTag=md), blobs=blobs)
        b.run()
        bs[md] = b
    say("index + two batches aligned in %.0fs" % (time.time() - t0))
    ms = {False: [], True: []}
    size = {}
    for rep in range(args.steps + 1):
        for md in (False, True):
            size[md] = bs[md].format_device()
            if rep > 0:
                ms[md].append(bs[md].stats().format_ms)
    mapped = bs[True].stats().n_mapped
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for md in (False, True):
        say("mdTag=%-5s format_ms median %.3f (min %.3f max %.3f of %d)  SAM bytes %d"
            % (md, med[md], min(ms[md]), max(ms[md]), len(ms[md]), size[md]))
    added = size[True] - size[False]
    words = 2 * ((m + 31) // 32) * mapped  # a text word and an N word per 32 bases
    floor = 2 * (words / WORDS_PER_S) + added / STREAM_B_PER_S
    say("MD adds %d bytes (%.2f per mapped read, %d mapped) and %.3f ms; window words per pass %d; "
        "floor of the extra work %.3f ms (2 x %.3f ms of gathers + %.3f ms of bytes)"
        % (added, added / max(1, mapped), mapped, med[True] - med[False], words, floor * 1e3, words / WORDS_PER_S * 1e3,
           added / STREAM_B_PER_S * 1e3))
    # the tag-on text without its tags is the tag-off text (a sample of reads)
    import re
    strip = re.compile(r"\tMD:Z:[^\t\n]*")
    samp = np.sort(np.random.default_rng(5).choice(n, min(n, 100000), replace=False)).astype(np.uint32)
    a, _ = bs[False].results_select(samp)
    b, _ = bs[True].results_select(samp)
    say("tag-on text of %d sampled reads, tags stripped, equals the tag-off text: %s" % (len(samp), strip.sub("", b) == a))


if __name__ == "__main__":
    main()
