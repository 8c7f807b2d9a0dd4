"""MD:Z as the project defines it (include/gwa.h GWA_SAM_TAG_MD), restated in plain Python:
the value follows from the printed SAM line and the contigs alone.  The checker of tests/test_md_host.py
and tests/test_gpu_md.py; the reference prints no MD, so there is nothing else to compare with."""
import re

_CIG = re.compile(r"(\d+)([MIDNSHP=X])")
MD_VALUE = re.compile(r"[0-9]+(([ACGTN]|\^[ACGTN]+)[0-9]+)*\Z")
MD_FIELD = re.compile(r"\tMD:Z:[^\t\n]*")


def md_of(line, contigs):
    """The MD value of one SAM line (contigs: name -> bases), None for a line that carries none: FLAG
    0x4 or an RNAME that is no contig."""
    f = line.rstrip("\n").split("\t")
    if int(f[1]) & 0x4 or f[2] not in contigs:
        return None
    ref, seq = contigs[f[2]].upper(), f[9]

    def ref_at(r):  # 1-based; outside the contig, and anything but A C G T, reads as N
        c = ref[r - 1] if 1 <= r <= len(ref) else "N"
        return c if c in "ACGT" else "N"

    q, r, run, out = 0, int(f[3]), 0, []
    for n, op in _CIG.findall(f[5]):
        n = int(n)
        if op in "M=X":
            for _ in range(n):
                s, c = (seq[q] if q < len(seq) else "N"), ref_at(r)
                if s in "ACGT" and s == c:
                    run += 1
                else:
                    out += [str(run), c]
                    run = 0
                q += 1
                r += 1
        elif op == "D":
            out += [str(run), "^"] + [ref_at(r + i) for i in range(n)]
            run = 0
            r += n
        elif op == "N":
            r += n
        elif op in "IS":
            q += n
    return "".join(out) + str(run)


def md_field(line):
    """The line's MD value and whether it is the last field, or (None, False)."""
    f = line.rstrip("\n").split("\t")
    hits = [i for i, x in enumerate(f) if x.startswith("MD:Z:")]
    if len(hits) != 1:
        return (None, False) if not hits else ("<%d MD fields>" % len(hits), False)
    return f[hits[0]][5:], hits[0] == len(f) - 1


def strip_md(sam):
    return MD_FIELD.sub("", sam)


def check_sam(sam, contigs):
    """Every line of `sam` carries exactly the MD the rule gives (last on the line), or none where the
    rule gives none.  Returns the number of lines with an MD."""
    n = 0
    for line in sam.splitlines():
        want = md_of(line, contigs)
        got, last = md_field(line)
        assert got == want, "MD %r, the rule gives %r: %s" % (got, want, line)
        if want is not None:
            assert last, "MD is not the last field: " + line
            assert MD_VALUE.match(got), got
            n += 1
    return n
