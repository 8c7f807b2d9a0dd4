"""End-to-end FASTQ file -> output file through the CLI for the three sinks (plain SAM, --bgzf, --bam),
alternating, `--rounds` runs each (GPU box; writes under $TMPDIR): a synthetic genome written as FASTA and
saved as an index by `bwt`, N 100 bp reads in a plain FASTQ, `align --timing --warm-passes 2` (the timed pass
only).  Prints each run's reads/s, the pipeline's stage line and the output size; after the timed part the
--bam file is decoded by tests/bam_ref.py and compared with the plain file (the first `--check` reads).

  python tools/bam_e2e.py [--genome <Mbp>] [--reads N] [--rounds K] [--check N]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="200")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check", type=int, default=100_000)
    a = ap.parse_args()
    import numpy as np
    import synth
    contigs = [("chr%d" % (i + 1), int(float(a.genome) * 1e6 / 4)) for i in range(4)]
    codes, names, lengths = synth.genome(contigs, config_id=1)
    d = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    fa, fq = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq")
    t0 = time.time()
    with open(fa, "wb") as f:
        off = 0
        for nm, L in zip(names, lengths):
            f.write(b">%s\n" % nm.encode())
            rows = (L + 59) // 60  # 60 bases a line
            flat = np.full(rows * 60, ord("A"), dtype=np.uint8)
            flat[:L] = synth.SYM[codes[off:off + L]]
            blk = np.full((rows, 61), ord("\n"), dtype=np.uint8)
            blk[:, :60] = flat.reshape(rows, 60)
            data = blk.tobytes()
            tail = rows * 60 - L  # drop the padding of the last line, keep its newline
            f.write(data[:len(data) - 1 - tail] + b"\n" if tail else data)
            off += L
    m = 100
    sb = synth.SYM[synth.reads_codes(codes, lengths, a.reads, m, 2, config_id=2)]
    with open(fq, "wb") as f:
        for c0 in range(0, a.reads, 1 << 18):
            c1 = min(a.reads, c0 + (1 << 18))
            f.write(b"".join(b"@r%09d\n%s\n+\n%s\n" % (i, sb[i].tobytes(), b"I" * m) for i in range(c0, c1)))
    del sb, codes
    print("[bam_e2e] inputs written in %.1fs (%.2f GB of FASTQ)" % (time.time() - t0, os.path.getsize(fq) / 1e9), flush=True)
    cli = [sys.executable, os.path.join(REPO, "genome-weaver-align_amd", "gwa_cli.py")]
    subprocess.run(cli + ["bwt", fa], check=True, stderr=subprocess.DEVNULL)
    outs = {"plain": os.path.join(d, "out.sam"), "--bgzf": os.path.join(d, "out.sam.gz"), "--bam": os.path.join(d, "out.bam")}
    rates = {k: [] for k in outs}
    for rnd in range(a.rounds):
        for kind, out in outs.items():
            r = subprocess.run(cli + ["align", "-r", fa, "-k", "2", "--timing", "--warm-passes", "2", "-o", out] +
                               ([] if kind == "plain" else [kind]) + [fq], stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(r.stderr)
                sys.exit(r.returncode)
            rate = re.search(r"after it (\d+) reads/s", r.stderr)
            pl = [l for l in r.stderr.splitlines() if l.startswith("[gwa] pipeline")]
            rates[kind].append(int(rate.group(1)))
            print("[bam_e2e] round %d %-6s %5.1f M reads/s, %d bytes; %s" % (rnd, kind, rates[kind][-1] / 1e6, os.path.getsize(out),
                                                                             pl[0][len("[gwa] "):] if pl else ""), flush=True)
    for kind, v in rates.items():
        v = sorted(v)
        print("[bam_e2e] %-6s median %.1f M reads/s (%.1f-%.1f)" % (kind, v[len(v) // 2] / 1e6, v[0] / 1e6, v[-1] / 1e6))
    # after the timed part: the BAM file decodes to the plain file's lines
    import bam_ref
    import zlib
    want, got, at = [], [], 0
    with open(outs["plain"]) as f:
        hdr = []
        for line in f:
            if line.startswith("@"):
                hdr.append(line)
                continue
            want.append(bam_ref.normalise(line.rstrip("\n")))
            if len(want) >= a.check:
                break
    data = open(outs["--bam"], "rb").read()
    assert data.endswith(bam_ref.EOF)
    raw = bytearray()
    while at < len(data) and len(raw) < 400 * (a.check + 1000):
        bsize = int.from_bytes(data[at + 16:at + 18], "little") + 1
        raw += zlib.decompress(data[at + 18:at + bsize - 8], -15)
        at += bsize
    raw = bytes(raw)
    text, contigs2, p = bam_ref.parse_header(raw)
    assert text == "".join(hdr)
    while len(got) < len(want):
        n = int.from_bytes(raw[p:p + 4], "little")
        got.append(bam_ref.render(raw[p:p + 4 + n], contigs2))
        p += 4 + n
    assert got == want, "the BAM file does not decode to the plain SAM"
    print("[bam_e2e] the first %d records of the BAM file decode to the plain file's lines" % len(want))
    for p in list(outs.values()) + [fa, fq, fa + ".gwa.idx"]:
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(d)


if __name__ == "__main__":
    main()
