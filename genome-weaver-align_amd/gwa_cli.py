"""`align` command of genome-weaver on MI355X (A/Align.java:57-110 and the options of
A/AlignmentConfig.java:40-72, A/AlignmentScoreConfig.java:37-77).

  python genome-weaver-align_amd/gwa_cli.py bwt ref.fa            (writes ref.fa.gwa.idx)
  python genome-weaver-align_amd/gwa_cli.py align -r ref.fa [-q SEQ | reads.fq[.gz|.snap] | reads.fa[.gz|.snap]]
         [-k 0.1] [-m bsf|sf|bd|bwa] [-R besthit|allhits|topL] [-L 5] [-g 1] [-e 4] [-s 1] [-M 1] [-N 3]
         [-G 11] [-E 4] [-S 11] [-P 5] [-W 31] [--silent] [--devices 0,1,..] [--batch 1048576] [--md] [--bgzf | --bam]
         [-o FILE]
  python genome-weaver-align_amd/gwa_cli.py align -r ref.fa mates_1.fq[.gz|.snap] mates_2.fq[.gz|.snap]
         [--insert-min 210] [--insert-max 390] [--check-mate-names]       (paired-end, two SAM lines per pair)
  python genome-weaver-align_amd/gwa_cli.py align -r ref.fa --interleaved pairs.fq   (mates alternating in one file)
  python genome-weaver-align_amd/gwa_cli.py align -r ref.fa reads.bam | mates_1.bam mates_2.bam | --interleaved pairs.bam

Writes SAM to stdout: the `@SQ` header (SequenceBoundary.toSAMHeader, A/SequenceBoundary.java:81-87)
then one record per read in input order, as SAMOutput does (A/SAMOutput.java:56-82).  Read files go
through the library's multi-device pipeline (gwa_pipeline_align_file): batches dealt to one index
replica per GPU in --devices, SAM written back in input order.  Like the reference, which loads the
files its `bwt` command wrote next to the FASTA (A/FMIndexOnGenome.java:60-86, A/BWTFiles.java:40-80),
`align -r ref.fa` loads `ref.fa.gwa.idx` when `bwt` made one, and otherwise builds the index on the GPU
from the FASTA.

--bgzf writes the same SAM as BGZF, the blocked gzip of the SAM specification (zcat, samtools and htslib
read it): the `@SQ` header as blocks from the host build of the encoder, every batch's records compressed
on its GPU (gwa_pipeline_set_output; the blocks, not the text, cross PCIe), and the 28-byte EOF marker
last.  With --shard R/N shard 0 writes the header and only shard N - 1 the EOF marker, so the shard files
concatenated in order are one valid file that decompresses to the one-process SAM.  `align(ns, out=...)`
takes a binary stream then.  The reference has no compressed output.

--bam writes BAM: the header (gwa.FMIndexOnGenome.bam_header: magic, the `@SQ` text, the contig table) as BGZF
blocks from the host encoder, every batch's alignment records built and compressed on its GPU (include/gwa.h
states the record as a function of the SAM line), and the EOF marker last; --shard frames the shard files as
--bgzf does, so that they concatenate to one BAM.  -q aligns its read as one batch (gwa_batch_results_bam).
It excludes --bgzf, combines with --md, --devices and paired input, and is not written to a terminal: give
-o FILE or redirect stdout.  The records are in input order unless --sort is given.

--bam --sort writes the records in coordinate order (include/gwa.h "Sorted BAM": by refID and pos, refID -1
last, equal keys in input order) under an "@HD VN:1.6 SO:coordinate" header: every batch is sorted on its GPU,
the sorted runs are kept in host memory up to --sort-mem BYTES and spilled to --tmp-dir DIR beyond it, and
merged into one BGZF stream when the input ends.  --index (with -o FILE) also writes FILE.bai.  --sort refuses
--shard and --sync (shards would be sorted apart) and --warm-passes above 1; -q sorts its one batch.
--markdup (with --bam --sort) sets FLAG 0x400 on duplicate templates (include/gwa.h "Duplicate marking": equal
unclipped 5' ends and strands, the highest quality sum kept), decided on the device from the input-order stream.

Two read files (or one with --interleaved) are paired-end input: mate i of the first file with mate i
of the second, two SAM lines per pair, streamed through the same pipeline on every device of
--devices (gwa_pipeline_align_pair_files; --batch then counts pairs).  The reference prints only the
header for two read files: its paired reader is a stub (R/ReadReaderFactory.java:60-84); the pairing
rules are this build's own (include/gwa.h gwa_batch_create_pairs), -m bsf only.

Read input follows ReadReaderFactory.createReader (R/ReadReaderFactory.java:126-151): `.fa`,
`.fasta`, `.fan`, `.fastq`, `.fq`, optionally `.gz` or `.snap` (snappy-java stream); `-q` aligns one query named "read" with no
qualities (R/ReadReaderFactory.java:167-180).  Read names are the first whitespace-delimited token
of the header line (utgb FastqReader / FASTAPullParser are unvendored: parity unpinned).

A `.bam` file (unaligned or aligned; the reference reads none) is read input too: its BGZF members are inflated
and its alignment records decoded into reads on the GPU (include/gwa.h "BAM input").  A read is the record's
name, its SEQ (reverse-complemented back when FLAG has 0x10) and its quality (none when the record has none);
secondary and supplementary records are skipped; the input's alignment, tags and header are ignored.  The
output is byte for byte that of the same reads as FASTQ.  `--interleaved pairs.bam` takes mate 1 and mate 2 of
each pair in turn and checks their flags (0x1 with 0x40, then 0x1 with 0x80), so a coordinate-sorted BAM is
refused; two `.bam` mate files, or a `.bam` beside a FASTQ file, pair record i with record i.  --shard refuses a
`.bam` as it refuses a `.gz`.
"""
import argparse
import gzip
import io
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gwa  # noqa: E402


def _open(path):
    if path.endswith(".snap"):  # snappy-java stream (R/ReadReaderFactory.java:130-139)
        with open(path, "rb") as f:
            return io.TextIOWrapper(io.BytesIO(gwa.snappy_decompress(f.read())))
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")


def _kind(path):
    p = path[:-3] if path.endswith(".gz") else path[:-5] if path.endswith(".snap") else path
    if p.endswith((".fa", ".fasta", ".fan")):
        return "fasta"
    if p.endswith((".fastq", ".fq")):
        return "fastq"
    if path.endswith(".bam"):
        return "bam"
    raise gwa.GwaError("Unsupported file type: " + path)


def read_fasta(f):
    """(name, seq, None) per record; multi-line sequences are concatenated."""
    name, parts = None, []
    for line in f:
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            if name is not None:
                yield name, "".join(parts), None
            hdr = line[1:].split()
            name, parts = (hdr[0] if hdr else ""), []
        elif name is not None:
            parts.append(line.strip())
    if name is not None:
        yield name, "".join(parts), None


def read_fastq(f):
    """(name, seq, qual) per 4-line record."""
    while True:
        h = f.readline()
        if not h:
            return
        h = h.rstrip("\r\n")
        if not h:
            continue
        if not h.startswith("@"):
            raise gwa.GwaError("malformed FASTQ header: %r" % h[:80])
        seq = f.readline().rstrip("\r\n")
        plus = f.readline()
        qual = f.readline().rstrip("\r\n")
        if not plus.startswith("+") or len(qual) != len(seq):
            raise gwa.GwaError("malformed FASTQ record: %r" % h[:80])
        hdr = h[1:].split()
        yield (hdr[0] if hdr else ""), seq, qual


def reads_of(path):
    kind = _kind(path)  # unsupported suffixes fail before the file is opened
    if kind == "bam":  # inflated and decoded by the host builds of the library's decoders
        with open(path, "rb") as fb:
            data = gwa.bgzf_decompress(fb.read())
        yield from gwa.bam_reads_decode(data[gwa.bam_header_size(data):], device=-1)
        return
    f = _open(path)
    try:
        yield from (read_fasta(f) if kind == "fasta" else read_fastq(f))
    finally:
        f.close()


def build_parser():
    ap = argparse.ArgumentParser(prog="gwa", description="genome-weaver read alignment on MI355X")
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("align", help="read alignment")
    a.add_argument("-r", dest="refSeq", required=True, help="reference sequence (FASTA)")
    a.add_argument("-q", dest="query", help="single query sequence")
    a.add_argument("readFiles", nargs="*", help="read file (single-end), or two mate files (paired-end): FASTA, FASTQ (optionally .gz or .snap) or BAM")
    a.add_argument("--silent", action="store_true", help="disable output")
    a.add_argument("-m", dest="strategy", default="bsf", help="alignment strategy: bsf (default), sf, bd, bwa")
    a.add_argument("-R", dest="reportType", default="besthit", help="besthit (default), allhits, topL")
    a.add_argument("-L", dest="topL", type=int, default=5)
    a.add_argument("-k", dest="k", type=float, default=0.1,
                   help="maximum edit distances. float (fraction of read length) or int [0.1]")
    a.add_argument("-g", dest="numGapOpenAllowed", type=int, default=1)
    a.add_argument("-e", dest="numGapExtensionAllowed", type=int, default=4)
    a.add_argument("-s", dest="numSplitAlowed", type=int, default=1)
    a.add_argument("-M", dest="matchScore", type=int, default=1)
    a.add_argument("-N", dest="mismatchPenalty", type=int, default=3)
    a.add_argument("-G", dest="gapOpenPenalty", type=int, default=11)
    a.add_argument("-E", dest="gapExtensionPenalty", type=int, default=4)
    a.add_argument("-S", dest="splitOpenPenalty", type=int, default=11)
    a.add_argument("-P", dest="indelEndSkip", type=int, default=5)
    a.add_argument("-W", dest="bandWidth", type=int, default=31)
    a.add_argument("--md", dest="mdTag", action="store_true",
                   help="append MD:Z to every mapped line (computed on the device; not in the reference's output)")
    a.add_argument("--bgzf", action="store_true",
                   help="write the SAM as BGZF (blocked gzip, SAM specification 4.1), compressed on the device; "
                        "the header first, the EOF marker last")
    a.add_argument("--bam", action="store_true",
                   help="write BAM (SAM specification 4.2): records built and BGZF-compressed on the device, in input "
                        "order; not together with --bgzf, and not to a terminal")
    a.add_argument("--sort", action="store_true",
                   help="with --bam: write the records in coordinate order (refID, pos; refID -1 last; equal keys in "
                        "input order), sorted on the device, under an @HD SO:coordinate header.  Not together with "
                        "--shard or --sync (shards would be sorted apart) and not with --warm-passes above 1, which is "
                        "refused")
    a.add_argument("--index", action="store_true", help="with --sort and -o FILE: write the index FILE.bai")
    a.add_argument("--markdup", action="store_true",
                   help="with --bam --sort: mark duplicate templates with FLAG 0x400 (include/gwa.h \"Duplicate marking\")")
    a.add_argument("--sort-mem", type=int, default=4 << 30, metavar="BYTES",
                   help="--sort: bytes of records kept in host memory before sorted runs spill to --tmp-dir")
    a.add_argument("--tmp-dir", default=None, metavar="DIR", help="--sort: where runs beyond --sort-mem are spilled")
    a.add_argument("-o", dest="out", default=None, metavar="FILE", help="write the output to FILE instead of stdout")
    a.add_argument("--device", type=int, default=0, help="GPU ordinal (one device)")
    a.add_argument("--devices", default=None, help="comma-separated GPU ordinals: one index replica per GPU")
    a.add_argument("--workers", type=int, default=3, help="host worker threads per device")
    b = sub.add_parser("bwt", help="build and save the index of a FASTA (loaded by align -r)")
    b.add_argument("fasta")
    b.add_argument("-o", dest="out", default=None, help="index file (default: <fasta>.gwa.idx)")
    b.add_argument("--device", type=int, default=0)
    a.add_argument("--batch", type=int, default=1 << 20, help="reads per device batch")
    a.add_argument("--timing", action="store_true", help="index / align wall times and reads/s on stderr")
    a.add_argument("--warm-passes", type=int, default=1,
                   help="timing runs: align the read file N times, the first N - 1 into /dev/null; --timing then "
                        "reports the last pass only")
    a.add_argument("--insert-min", type=int, default=210, help="paired-end: smallest template length of a proper pair")
    a.add_argument("--insert-max", type=int, default=390,
                   help="paired-end: largest template length of a proper pair (mate rescue needs max - min + read "
                        "length + 2k <= 320 bases; wider ranges pair without rescue)")
    a.add_argument("--interleaved", action="store_true",
                   help="paired-end: the one read file holds both mates, records 2i and 2i + 1 forming pair i")
    a.add_argument("--check-mate-names", action="store_true",
                   help="paired-end: fail on the first pair whose mate names differ (one trailing /1 or /2 apart)")
    a.add_argument("--sync", default=None, metavar="DIR:N",
                   help="timing runs of N processes (--shard): after the warm passes, wait until all N have written a "
                        "ready file into DIR, so their timed passes run at the same time; --timing then also prints "
                        "the timed pass's CLOCK_MONOTONIC start and end")
    a.add_argument("--shard", default=None, metavar="R/N",
                   help="one process per GPU: align contiguous shard R of N of the (plain) read file; the SAM "
                        "header is written by shard 0 only, so the shards' outputs concatenated in order are "
                        "the one-process SAM")
    return ap


def sync_wait(spec, timeout=600.0):
    """--sync DIR:N: write DIR/ready.<pid>, then wait until N ready files exist"""
    d, n = spec.rsplit(":", 1)
    n = int(n)
    open(os.path.join(d, "ready.%d" % os.getpid()), "w").close()
    t0 = time.monotonic()
    while sum(1 for x in os.listdir(d) if x.startswith("ready.")) < n:
        if time.monotonic() - t0 > timeout:
            raise gwa.GwaError("--sync %s: the other processes did not arrive" % spec)
        time.sleep(0.0005)


def shard_of(ns):
    """--shard R/N as (R, N), or None"""
    if ns.shard is None:
        return None
    try:
        r, n = (int(x) for x in ns.shard.split("/"))
    except ValueError:
        raise gwa.GwaError("--shard takes R/N (e.g. 0/8), got %r" % ns.shard)
    if n < 1 or not 0 <= r < n:
        raise gwa.GwaError("--shard %s: need 0 <= R < N" % ns.shard)
    return r, n


def config_of(ns):
    cfg = gwa.AlignmentConfig(k=ns.k, strategy=ns.strategy, reportType=ns.reportType, topL=ns.topL,
                              numGapOpenAllowed=ns.numGapOpenAllowed, numGapExtensionAllowed=ns.numGapExtensionAllowed,
                              numSplitAlowed=ns.numSplitAlowed, matchScore=ns.matchScore,
                              mismatchPenalty=ns.mismatchPenalty, gapOpenPenalty=ns.gapOpenPenalty,
                              gapExtensionPenalty=ns.gapExtensionPenalty, splitOpenPenalty=ns.splitOpenPenalty,
                              indelEndSkip=ns.indelEndSkip, bandWidth=ns.bandWidth, mdTag=ns.mdTag)
    cfg._c()  # validates strategy / report type (raises GwaError)
    return cfg


def index_path(ref):
    """The saved index the `bwt` command writes for a FASTA (or the path itself when it is one)."""
    return ref + ".gwa.idx"


def load_indexes(ref, devices):
    """One FMIndexOnGenome per device (built in parallel; each GPU holds a full replica)."""
    import threading
    src = index_path(ref) if os.path.exists(index_path(ref)) else ref
    out, errs = [None] * len(devices), []

    def one(i, d):
        try:
            out[i] = gwa.FMIndexOnGenome.load(src, device=d)
        except gwa.GwaError as e:
            errs.append(e)

    th = [threading.Thread(target=one, args=(i, d)) for i, d in enumerate(devices)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        for x in out:
            if x is not None:
                x.close()
        raise errs[0]
    return out


def align(ns, out=sys.stdout):
    if ns.query is None and not ns.readFiles:
        raise gwa.GwaError("no query is given")
    if ns.query is None and len(ns.readFiles) not in (1, 2):
        raise gwa.GwaError("give one read file (single-end) or two mate files (paired-end)")
    if ns.interleaved and (ns.query is not None or len(ns.readFiles) != 1):
        raise gwa.GwaError("--interleaved takes one read file holding both mates of every pair")
    paired = ns.query is None and (len(ns.readFiles) == 2 or ns.interleaved)
    if ns.check_mate_names and not paired:
        raise gwa.GwaError("--check-mate-names needs paired-end input (two mate files, or --interleaved)")
    bam, bgzf = getattr(ns, "bam", False), getattr(ns, "bgzf", False)
    if bam and bgzf:
        raise gwa.GwaError("--bam and --bgzf exclude each other: BAM is its own BGZF file")
    if bam and out is sys.stdout and sys.stdout.isatty():
        raise gwa.GwaError("--bam writes binary data: give -o FILE or redirect stdout")
    sort, index = getattr(ns, "sort", False), getattr(ns, "index", False)
    if sort and not bam:
        raise gwa.GwaError("--sort needs --bam")
    if index and not (sort and ns.out is not None):
        raise gwa.GwaError("--index needs --sort and -o FILE (the index is written to FILE.bai)")
    markdup = getattr(ns, "markdup", False)
    if markdup and not (bam and sort):
        raise gwa.GwaError("--markdup needs --bam --sort (duplicates are marked in the sorted file)")
    if sort and (ns.shard is not None or ns.sync):
        raise gwa.GwaError("--sort does not combine with --shard or --sync: the shards would be sorted apart")
    if sort and ns.warm_passes > 1:
        raise gwa.GwaError("--sort does not combine with --warm-passes above 1")
    cfg = config_of(ns)
    shard = shard_of(ns)
    if shard is not None and (ns.query is not None or paired):
        raise gwa.GwaError("--shard splits one single-end read file")
    if paired and cfg.strategy.lower() != "bsf":
        raise gwa.GwaError("paired-end alignment runs -m bsf")
    if ns.query is None:
        for f in ns.readFiles:
            _kind(f)  # unsupported suffixes fail before the index is built
    if shard is not None:
        gwa.shard_range(ns.readFiles[0], *shard)  # (a .gz or missing file fails before the index is built)
    devices = [int(x) for x in ns.devices.split(",")] if ns.devices else [ns.device]
    t0 = time.perf_counter()
    fms = load_indexes(ns.refSeq, devices)
    t1 = time.perf_counter()
    binary = bgzf or bam
    if binary and out is sys.stdout:
        out = sys.stdout.buffer
    if ns.silent:
        w = lambda s: None  # noqa: E731
    elif bam:  # (only the header goes through w)
        w = lambda b: out.write(gwa.bgzf_compress(b))  # noqa: E731
    elif bgzf:  # (the header, or -q's few lines: the host build of the encoder)
        w = lambda s: out.write(gwa.bgzf_compress(s.encode()))  # noqa: E731
    else:
        w = out.write
    if shard is None or shard[0] == 0:
        w(fms[0].bam_header(sorted=sort) if bam else fms[0].samHeader())
    n = 0
    bai, bai_done = None, False  # FILE.bai: opened only when an index will be written, removed when the run fails
    t_open = 0.0
    mono0 = None

    def run_file(pipe, fd):
        """one pass over the read file(s) into fd; reads (single-end) or pairs (paired-end) aligned"""
        if paired:
            return pipe.align_pair_files(ns.readFiles[0], ns.readFiles[1] if len(ns.readFiles) == 2 else None, fd,
                                         (ns.insert_min, ns.insert_max), ns.check_mate_names)
        return pipe.align_file(ns.readFiles[0], fd, shard=shard)

    try:
        if index and not ns.silent:
            bai = open(ns.out + ".bai", "wb")
        if ns.query is not None:
            if bam:  # the one read as a batch, its records compressed on the device
                qb = gwa.Batch(fms[0], cfg, reads=[("read", ns.query, None)])
                try:
                    qb.run()
                    if sort:  # its one batch through the sorter: blocks (and the index) by way of a file
                        out.flush()
                        sorter = gwa.BamSorter(fms[0], tmp_dir=ns.tmp_dir, mem=ns.sort_mem, markdup=markdup)
                        try:
                            sorter.add_batch(0, qb)
                            if index and not ns.silent:  # (the index holds offsets of FILE: written in place)
                                sorter.finish(out.fileno(), bai.fileno())
                                blocks = b""
                            else:
                                with tempfile.TemporaryFile() as tf:
                                    sorter.finish(tf.fileno(), -1)
                                    tf.seek(0)
                                    blocks = tf.read()
                        finally:
                            sorter.close()
                    else:
                        blocks = qb.results_bam()
                finally:
                    qb.close()
                if not ns.silent:
                    out.write(blocks)
            else:
                w(gwa.aligner(fms[0], cfg).align_batch([("read", ns.query, None)]))
            n = 1
        else:
            out.flush()
            tp = time.perf_counter()
            pipe = gwa.Pipeline(fms, cfg, batch_reads=ns.batch, workers_per_device=ns.workers,
                                output="bam" if bam else "bgzf" if bgzf else "sam")  # pins host buffers
            t_open = time.perf_counter() - tp
            try:
                if sort:
                    pipe.set_sort(tmp_dir=ns.tmp_dir, mem=ns.sort_mem, index=bai.fileno() if bai else None)
                    if markdup:
                        pipe.set_markdup(True)
                # --warm-passes N: N - 1 untimed passes over the file into /dev/null first (pinned buffers,
                # device caches and the page cache warm), then the timed pass that writes the SAM
                for _ in range(max(0, ns.warm_passes - 1)):
                    with open(os.devnull, "wb") as dn:
                        run_file(pipe, dn.fileno())
                if ns.sync:
                    sync_wait(ns.sync)
                if ns.warm_passes > 1 or ns.sync:
                    t1, t_open = time.perf_counter(), 0.0
                mono0 = time.monotonic_ns()
                if ns.silent:
                    with open(os.devnull, "wb") as dn:
                        n = run_file(pipe, dn.fileno())
                else:
                    try:
                        fd = out.fileno()
                    except (AttributeError, io.UnsupportedOperation):
                        fd = None
                    if fd is not None:
                        n = run_file(pipe, fd)
                        if ns.timing:
                            st = pipe.stats()
                            print("[gwa] pipeline %.2fs: read %.2fs, frame %.2fs; summed over %d worker threads: parse %.2fs, "
                                  "set-up %.2fs, kernels %s s, SAM format %.2fs, write %.2fs, order wait %.2fs; %d bytes out"
                                  % (st.wall_s, st.read_s, st.frame_s, ns.workers * len(devices), st.parse_s, st.setup_s,
                                     "/".join("%.2f" % st.device_kernel_s[i] for i in range(len(devices))),
                                     st.format_s, st.write_s, st.order_wait_s, st.out_bytes), file=sys.stderr)
                            if sort:
                                ss = pipe.sort_stats()
                                print("[gwa] sort: %d records in %d runs (%d spilled), add %.2fs (summed over workers), order "
                                      "%.2fs, copy %.2fs, compress %.2fs, write %.2fs, index %.2fs; %d blocks"
                                      % (ss.records, ss.runs, ss.spilled_runs, ss.add_s, ss.order_s, ss.copy_s, ss.compress_s,
                                         ss.write_s, ss.index_s, ss.blocks), file=sys.stderr)
                            if markdup:
                                ms = pipe.markdup_stats()
                                print("[gwa] markdup: %d templates (%d pair, %d fragment), duplicates: %d pair and %d "
                                      "fragment templates, %d records; keys %.3fs (summed over batches), resolve %.3fs"
                                      % (ms.templates, ms.pair_templates, ms.frag_templates, ms.dup_pair_templates,
                                         ms.dup_frag_templates, ms.dup_records, ms.keys_s, ms.resolve_s), file=sys.stderr)
                            if st.inflate_blocks or st.in_bytes:
                                print("[gwa] BGZF input: %d compressed bytes read, %d members inflated on the device, "
                                      "inflate %.2fs (a part of read)" % (st.in_bytes, st.inflate_blocks, st.inflate_s),
                                      file=sys.stderr)
                    else:  # an in-memory stream (tests): through a temporary file
                        with tempfile.TemporaryFile() as tf:
                            n = run_file(pipe, tf.fileno())
                            tf.seek(0)
                            out.write(tf.read() if binary else tf.read().decode())
            finally:
                t2 = time.perf_counter()  # (the SAM is written; unpinning the buffers is teardown)
                if ns.timing and ns.sync and mono0 is not None:  # (None: a warm pass or the sync wait failed)
                    print("[gwa] timed pass monotonic_ns %d %d" % (mono0, time.monotonic_ns()), file=sys.stderr)
                pipe.close()
        if ns.query is not None:
            t2 = time.perf_counter()
        if binary and not ns.silent and (shard is None or shard[0] == shard[1] - 1):
            out.write(gwa.BGZF_EOF)
            out.flush()
        bai_done = True
    finally:
        if bai is not None:
            bai.close()
            if not bai_done:
                os.remove(bai.name)
        for fm in fms:
            fm.close()
    if ns.timing:
        nr = 2 * n if paired else n  # (reads per second count mates)
        print("[gwa] index load %.2fs (%d device(s)); align (read file -> SAM, index load excluded) %.2fs: %.0f reads/s; "
              "of which pipeline open (pinning host buffers) %.2fs, after it %.0f reads/s"
              % (t1 - t0, len(devices), t2 - t1, nr / max(t2 - t1, 1e-9), t_open, nr / max(t2 - t1 - t_open, 1e-9)),
              file=sys.stderr)
    return n


def bwt(ns):
    """Build the index of a FASTA on the GPU and save it (the reference's `bwt` command,
    A/BWTransform.java:72-179, in this build's own format: include/gwa.h gwa_index_save)."""
    out = ns.out or index_path(ns.fasta)
    fm = gwa.FMIndexOnGenome.load(ns.fasta, device=ns.device)
    try:
        fm.save(out)
    finally:
        fm.close()
    print("[gwa] index of %s saved to %s" % (ns.fasta, out), file=sys.stderr)


def main(argv=None):
    ns = build_parser().parse_args(argv)
    try:
        if ns.cmd == "align" and ns.out is not None:
            with open(ns.out, "wb" if ns.bam or ns.bgzf else "w") as f:
                n = align(ns, out=f)
            print("[gwa] %d reads aligned" % n, file=sys.stderr)
        elif ns.cmd == "align":
            n = align(ns)
            print("[gwa] %d reads aligned" % n, file=sys.stderr)
        elif ns.cmd == "bwt":
            bwt(ns)
    except gwa.GwaError as e:
        print("[gwa] error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
