"""End-to-end FASTQ file -> BAM file through the CLI, input order against coordinate-sorted with an index (GPU
box; writes under $TMPDIR): tools/bam_e2e.py's inputs (a synthetic genome in 4 contigs written as FASTA and saved
as an index by `bwt`, N 100 bp reads in a plain FASTQ), then `align --timing --bam` and `align --timing --bam
--sort --index` alternately, one untimed round and `--rounds` timed ones (no warm passes: --sort refuses them,
so neither kind gets one).  Prints each run's reads/s, the pipeline's stage line, the sorter's line (add, order,
copy, compress, write, index seconds), the output size and the child's peak resident memory; afterwards the
sorted file's first `--check` records are decoded (tests/bam_ref.py, tests/bai_ref.py): SO:coordinate, keys
ascending, and the index's record counts add up to the reads.

  python tools/bam_sort_e2e.py [--genome <Mbp>] [--reads N] [--rounds K] [--check N] [--sort-mem BYTES]
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


def say(*a):
    print("[bam_sort_e2e]", *a, flush=True)


def run(cmd, errpath):
    """(return code, stderr text, peak resident memory of the child in bytes)"""
    with open(errpath, "w") as ef:
        p = subprocess.Popen(cmd, stderr=ef)
        _, status, ru = os.wait4(p.pid, 0)
        p.returncode = os.waitstatus_to_exitcode(status)
    return p.returncode, open(errpath).read(), ru.ru_maxrss * 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="200")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check", type=int, default=100_000)
    ap.add_argument("--sort-mem", type=int, default=4 << 30)
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
    say("inputs written in %.1fs (%.2f GB of FASTQ)" % (time.time() - t0, os.path.getsize(fq) / 1e9))
    cli = [sys.executable, os.path.join(REPO, "genome-weaver-align_amd", "gwa_cli.py")]
    subprocess.run(cli + ["bwt", fa], check=True, stderr=subprocess.DEVNULL)
    spill = os.path.join(d, "spill")
    os.mkdir(spill)
    kinds = {"--bam": (os.path.join(d, "out.bam"), ["--bam"]),
             "--bam --sort --index": (os.path.join(d, "sorted.bam"),
                                      ["--bam", "--sort", "--index", "--sort-mem", str(a.sort_mem), "--tmp-dir", spill])}
    rates = {k: [] for k in kinds}
    rss = {k: [] for k in kinds}
    stages = {}
    for rnd in range(a.rounds + 1):
        for kind, (out, flags) in kinds.items():
            rc, err, peak = run(cli + ["align", "-r", fa, "-k", "2", "--timing", "-o", out] + flags + [fq], os.path.join(d, "err.txt"))
            if rc != 0:
                print(err)
                sys.exit(rc)
            rate = int(re.search(r"after it (\d+) reads/s", err).group(1))
            lines = [l[len("[gwa] "):] for l in err.splitlines() if l.startswith("[gwa] pipeline") or l.startswith("[gwa] sort:")]
            if rnd:
                rates[kind].append(rate)
                rss[kind].append(peak)
                for l in lines:
                    if l.startswith("sort:"):
                        for name, v in re.findall(r"(add|order|copy|compress|write|index) (\d+\.\d+)s", l):
                            stages.setdefault(name, []).append(float(v))
            say("round %d%s %-20s %5.1f M reads/s, %d bytes, peak host memory %.2f GB; %s"
                % (rnd, "" if rnd else " (untimed)", kind, rate / 1e6, os.path.getsize(out), peak / 1e9, "; ".join(lines)))
    for kind in kinds:
        v, r = sorted(rates[kind]), sorted(rss[kind])
        say("%-20s median %.1f M reads/s (%.1f-%.1f), peak host memory %.2f GB (%.2f-%.2f)"
            % (kind, v[len(v) // 2] / 1e6, v[0] / 1e6, v[-1] / 1e6, r[len(r) // 2] / 1e9, r[0] / 1e9, r[-1] / 1e9))
    for name in ("add", "order", "copy", "compress", "write", "index"):
        v = sorted(stages.get(name, [0.0]))
        say("sorter %-8s median %.2fs (%.2f-%.2f)" % (name, v[len(v) // 2], v[0], v[-1]))
    # after the timed part: the sorted file
    import zlib
    import bai_ref
    import bam_ref
    out = kinds["--bam --sort --index"][0]
    data = open(out, "rb").read()
    assert data.endswith(bam_ref.EOF)
    raw, at = bytearray(), 0
    while at < len(data) and len(raw) < 400 * (a.check + 1000):
        bsize = int.from_bytes(data[at + 16:at + 18], "little") + 1
        raw += zlib.decompress(data[at + 18:at + bsize - 8], -15)
        at += bsize
    raw = bytes(raw)
    text, contigs2, p = bam_ref.parse_header(raw)
    assert text.startswith(bai_ref.HD_LINE) and [c[0] for c in contigs2] == names
    keys = []
    while len(keys) < a.check and p + 4 <= len(raw):
        n = int.from_bytes(raw[p:p + 4], "little")
        if p + 4 + n > len(raw):
            break
        keys.append(bai_ref.key(raw[p:p + 4 + n]))
        p += 4 + n
    assert keys == sorted(keys), "the sorted file is not in key order"
    refs, no_coor = bai_ref.parse_bai(open(out + ".bai", "rb").read())
    counted = no_coor + sum(sum(bins[bai_ref.PSEUDO_BIN][1]) for bins, _ in refs if bins)
    assert counted >= a.reads, (counted, a.reads)  # (a split read has two records)
    say("the first %d records of the sorted file are in key order under SO:coordinate; the index counts %d records "
        "(%d without a contig)" % (len(keys), counted, no_coor))
    assert os.listdir(spill) == []
    os.rmdir(spill)
    for p in [v[0] for v in kinds.values()] + [out + ".bai", fa, fq, fa + ".gwa.idx", os.path.join(d, "err.txt")]:
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(d)


if __name__ == "__main__":
    main()
