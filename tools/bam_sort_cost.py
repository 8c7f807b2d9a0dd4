"""What the coordinate sort of a batch's BAM records costs on the device next to building them (GPU box): one
resident index, the C2 reads (100 bp, 0-2 substitutions, constant qualities) in one batch, aligned once; then,
alternately and `--steps` times each after one untimed round, gwa_batch_format_bam (records) and
gwa_batch_format_bam_sorted (records + sort).  Prints median (min-max) of bam_ms and of the sort's passes (walk
+ keys, radix sort, permuted sizes + scan, the gather kernel), and, as the gather's yardstick, of a
device-to-device copy of the same number of bytes (torch's Tensor.copy_ between two device tensors, timed with
events in the same process), with gather time / copy time.

  python tools/bam_sort_cost.py [--genome <Mbp>] [--reads N] [--steps K] [--contigs C]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "genome-weaver-align_amd")]


def say(*a):
    print("[bam_sort_cost]", *a, flush=True)


def stat(v):
    v = sorted(v)
    return "%.3f (%.3f-%.3f)" % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="200")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--contigs", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gwa
    import synth
    m, n = 100, args.reads
    t0 = time.time()
    per = int(float(args.genome) * 1e6) // args.contigs
    codes, names, lengths = synth.genome([("chr%d" % (i + 1), per) for i in range(args.contigs)], 1)
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
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), blobs=blobs)
    b.run()
    say("index + batch aligned in %.0fs" % (time.time() - t0))
    bam_ms, walk, sort, perm, gather, copy = [], [], [], [], [], []
    nbytes = nrec = 0
    src = dst = None
    for rep in range(args.steps + 1):
        b.format_bam()
        if rep:
            bam_ms.append(b.stats().bam_ms)
        nbytes, nrec = b.format_bam_sorted()
        t = b.bam_sort_times()
        if rep:
            walk.append(t.walk_ms)
            sort.append(t.sort_ms)
            perm.append(t.permute_ms)
            gather.append(t.gather_ms)
        if src is None:
            dev = torch.device("cuda", gi.device)
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if rep:
            copy.append(e0.elapsed_time(e1))
    g, c = sorted(gather)[len(gather) // 2], sorted(copy)[len(copy) // 2]
    say("BAM records:   bam_ms    %s, %d bytes, %d records" % (stat(bam_ms), nbytes, nrec))
    say("sort, walk + keys:         %s ms" % stat(walk))
    say("sort, radix sort:          %s ms" % stat(sort))
    say("sort, permuted sizes + scan: %s ms" % stat(perm))
    say("sort, gather kernel:       %s ms" % stat(gather))
    say("device-to-device copy (Tensor.copy_) of %d bytes: %s ms (%.0f GB/s read + write)" % (nbytes, stat(copy), 2 * nbytes / c / 1e6))
    say("gather / copy = %.2f" % (g / c))
    b.close()
    gi.close()


if __name__ == "__main__":
    main()
