"""A plain restatement of the duplicate-marking rule of include/gwa.h ("Duplicate marking") in Python, over
BAM records as bytes (block_size included).  Written from the rule's text, not from csrc/bam_dup_core.h: the
end key from the unclipped 5' coordinate, the local pairing of neighbours, the classes, the score, the ordinal
and the decision, by dictionaries and max().  Shared by test_markdup_host.py (CPU) and test_gpu_markdup.py."""
import struct

NO_KEY = (1 << 64) - 1
STAT_NAMES = ("templates", "pair_templates", "frag_templates", "dup_pair_templates", "dup_frag_templates", "dup_records")


def head(rec):
    """(refID, pos, l_read_name, n_cigar_op, flag, l_seq)"""
    ref, pos, lname, _mapq, _bin, ncig, flag, lseq = struct.unpack_from("<iiBBHHHI", rec, 4)
    return ref, pos, lname, ncig, flag, lseq


def cigar(rec):
    _, _, lname, ncig, _, _ = head(rec)
    vals = struct.unpack_from("<%dI" % ncig, rec, 36 + lname)
    return [(v >> 4, v & 15) for v in vals]


def participates(rec):
    ref, _, _, _, flag, _ = head(rec)
    return flag & (0x4 | 0x100 | 0x800) == 0 and ref >= 0


def u5(rec):
    _, pos, _, ncig, flag, _ = head(rec)
    ops = cigar(rec)
    if ncig == 0:
        return pos
    if flag & 0x10 == 0:
        lead = 0
        for n, op in ops:
            if op not in (4, 5):
                break
            lead += n
        return pos - lead
    trail = 0
    for n, op in reversed(ops):
        if op not in (4, 5):
            break
        trail += n
    reflen = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
    return pos + reflen + trail - 1


def end_key(rec):
    """None for a record that does not participate"""
    if not participates(rec):
        return None
    ref, _, _, _, flag, _ = head(rec)
    return (ref & 0xFFFFFFFF) << 33 | ((u5(rec) + 0x80000000) & 0xFFFFFFFF) << 1 | (1 if flag & 0x10 else 0)


def own_score(rec):
    _, _, lname, ncig, _, lseq = head(rec)
    at = 36 + lname + 4 * ncig + (lseq + 1) // 2
    return sum(q for q in rec[at:at + lseq] if 15 <= q <= 93)


def name(rec):
    lname = rec[12]
    return rec[36:36 + lname]


def is_pair(a, b):
    fa, fb = head(a)[4], head(b)[4]
    if not (fa & 0x1 and fb & 0x1) or (fa | fb) & (0x100 | 0x800):
        return False
    if not (fa & 0x40 and not fa & 0x80 and fb & 0x80 and not fb & 0x40):
        return False
    return a[12] == b[12] and name(a) == name(b)


def templates_of(records):
    """[[index]]: the templates of one run's records, in input order"""
    out, i = [], 0
    while i < len(records):
        if i + 1 < len(records) and is_pair(records[i], records[i + 1]):
            out.append([i, i + 1])
            i += 2
        else:
            out.append([i])
            i += 1
    return out


def analyse(runs):
    """runs: [(run id, [record])], in any order.  Returns dict(marked: set of (run id, index in the run),
    stats: {name: count}, templates: [dict(run, first, members, part, cls, sig, score, dup, why)],
    dupinfo: {run id: [(endKey, mateKey, score, leader)] in input order})."""
    temps, dupinfo = [], {}
    for rid, recs in sorted(runs, key=lambda x: x[0]):
        info = [None] * len(recs)
        for members in templates_of(recs):
            part = [i for i in members if participates(recs[i])]
            score = sum(own_score(recs[i]) for i in part) & 0xFFFFFFFF
            keys = [end_key(recs[i]) for i in part]
            if len(members) == 2 and len(part) == 2:
                cls, sig = "pair", tuple(sorted(keys))
            elif len(part) == 1:
                cls, sig = "frag", keys[0]
            else:
                cls, sig = None, None
            temps.append(dict(run=rid, first=members[0], members=members, part=part, cls=cls, sig=sig, score=score,
                              dup=False, why=None))
            for i in members:
                k = end_key(recs[i])
                mate = NO_KEY
                if cls == "pair":
                    mate = end_key(recs[members[1] if i == members[0] else members[0]])
                info[i] = (NO_KEY if k is None else k, mate, score, members[0])
        dupinfo[rid] = info
    best = lambda group: max(group, key=lambda t: (t["score"], -t["run"], -t["first"]))
    by_sig = {}
    for t in temps:
        if t["cls"] == "pair":
            by_sig.setdefault(t["sig"], []).append(t)
    pair_ends = set()
    for sig, group in by_sig.items():
        pair_ends.update(sig)
        keep = best(group)
        for t in group:
            if t is not keep:
                t["dup"], t["why"] = True, "pair"
    by_key = {}
    for t in temps:
        if t["cls"] == "frag":
            by_key.setdefault(t["sig"], []).append(t)
    for k, group in by_key.items():
        if k in pair_ends:
            for t in group:
                t["dup"], t["why"] = True, "pair end"
        else:
            keep = best(group)
            for t in group:
                if t is not keep:
                    t["dup"], t["why"] = True, "frag"
    marked = set((t["run"], i) for t in temps if t["dup"] for i in t["part"])
    stats = dict(templates=len(temps), pair_templates=sum(t["cls"] == "pair" for t in temps),
                 frag_templates=sum(t["cls"] == "frag" for t in temps),
                 dup_pair_templates=sum(t["dup"] and t["cls"] == "pair" for t in temps),
                 dup_frag_templates=sum(t["dup"] and t["cls"] == "frag" for t in temps), dup_records=len(marked))
    return dict(marked=marked, stats=stats, templates=temps, dupinfo=dupinfo)


def set_dup(rec):
    b = bytearray(rec)
    b[19] |= 0x04  # FLAG 0x400: the high byte of the flag field
    return bytes(b)


def mark(runs):
    """(the runs with FLAG 0x400 set on the duplicates' participating records, analyse's result)"""
    res = analyse(runs)
    out = [(rid, [set_dup(r) if (rid, i) in res["marked"] else r for i, r in enumerate(recs)]) for rid, recs in runs]
    return out, res
