"""What tests/test_scan_cpu.py and tests/test_gpu_scan.py share: the queries'
prefixes, and rl_scan's definition written out in Python over the export's
records (the header's "Which keys" / "Which records" rules), so that the GPU
tests compare the scan with a filter of Backend.export_records()."""
import numpy as np

from ratelimit_amd import abi

# the edge stems of tests/test_gpu_forget.py (BASE cut at the layout's edges) and one more family
BASE = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ" * 4
EDGE_LEN = (4, 5, 31, 32, 33, 36, 37, 48, 49, 200)


def edge_stems():
    out = set()
    for L in EDGE_LEN:
        s = BASE[:L]
        out |= {s, s[:-1] + b"#", b"X" + s[1:], b"Y" + s[1:]}  # (the Y family: under none of p64's prefixes)
        if L > 34:
            out.add(s[:33] + b"#" + s[34:])
    return sorted(out)


DOMAIN = [b"fg_stem_"]  # the domain "fg" alone: "fg_b"'s stems begin "fg_b_stem_"
BOTH = [b"fg_"]         # ... and what SCAN MATCH fg_* sees: both domains


def p64():
    """64 prefixes over the stream's stems (fg_stream) and the edge stems: a
    proper subset of every kind of stem. In entry order, so a key is counted
    under the first that matches."""
    p = [
        b"fg_stem_s004_",              # equal to a whole stem (one unit)
        b"fg_stem_s005_?",             # a byte longer than a stem: matches nothing
        b"fg_stem_s00",                # overlaps the first one (takes what that one left) ...
        b"fg_stem_s005",               # ... and this one, which then counts nothing
        b"fg_b_stem_s00", b"fg_b_stem_s01", b"fg_stem_s01",
        b"fg_stem_s022_path_/a/rather/long/path/",  # reaches into a long stem's arena bytes
        b"fg_stem_never_",             # never seen
        BASE[:150],                    # deep in the arena: the 200-byte stem alone
        BASE[:33] + b"#",              # the arena's second byte differs (ahead of BASE[:33], which begins it)
        BASE[:37], BASE[:36], BASE[:33], BASE[:32],  # the inline / arena edge, longest first: each counts some
        BASE[:5], BASE[:4], BASE[:3],  # 5, 4 and 3 bytes around the first dword
        b"X",                          # 1 byte
    ]
    p += [b"zz_filler_%02d_" % i for i in range(64 - len(p))]
    assert len(p) == 64 and len(set(p)) == 64 and sum(map(len, p)) <= 4096
    return p


def rec_list(rec):
    """One page's arrays (export_range's layout) -> [(stem, unit, flags, ws, count, expire, lc)] in order."""
    off, sb = rec["stem_off"], rec["stem_bytes"]
    return [(bytes(sb[int(off[i]):int(off[i + 1])]),) + tuple(int(rec[k][i]) for k in abi.RECORD_DTYPES)
            for i in range(len(rec["ws"]))]


def export_list(be):
    """The whole table's records in the export's order (a key's records contiguous, oldest first)."""
    out = []
    for part in be.export_records():
        out += rec_list(part)
    return out


def groups_of(recs):
    """Consecutive records of one (stem, unit) -> [[record, ...], ...]; asserts
    that no key comes twice and every key's windows rise."""
    groups = []
    for r in recs:
        if groups and groups[-1][0][:2] == r[:2]:
            groups[-1].append(r)
        else:
            groups.append([r])
    keys = [g[0][:2] for g in groups]
    assert len(set(keys)) == len(keys), "a key's records are not contiguous (or a key came twice)"
    for g in groups:
        assert all(a[3] < b[3] for a, b in zip(g, g[1:])), "a key's records are not oldest first"
        assert not any(r[2] for r in g[1:]), "a flag on a record that is not its key's first"
    return groups


def expected(export, prefixes=(), units=None, newest=False, now=None):
    """rl_scan's answer as the header defines it, from the export's records.
    -> (records as a list, info sums as a dict, by_prefix as [max(n, 1)][3])."""
    prefixes = list(prefixes)
    byp = [[0, 0, 0] for _ in range(max(len(prefixes), 1))]
    out = []
    info = {"keys": 0, "records": 0, "stem_bytes": 0, "chains_lost": 0}
    for g in groups_of(export):
        stem, unit = g[0][:2]
        if units is not None and unit not in units:
            continue
        hit = [i for i, p in enumerate(prefixes) if stem.startswith(p)]
        if prefixes and not hit:
            continue
        lost = bool(g[0][2] & abi.RL_REC_CHAIN_LOST) and not newest
        recs = g[-1:] if newest else g
        if now is not None:
            recs = [r for r in recs if now <= r[5]]
        if not recs:
            continue  # (no key of the answer: counted nowhere)
        recs = [(r[0], r[1], abi.RL_REC_CHAIN_LOST if lost and j == 0 else 0) + r[3:] for j, r in enumerate(recs)]
        out += recs
        b = byp[hit[0] if prefixes else 0]
        b[0] += 1
        b[1] += len(recs)
        b[2] += sum(r[4] for r in recs)
        info["keys"] += 1
        info["records"] += len(recs)
        info["stem_bytes"] += len(stem) * len(recs)
        info["chains_lost"] += lost
    return out, info, byp


def scan_all(be, **kw):
    """Every page of Backend.scan -> (records in order, summed info, summed by_prefix, pages)."""
    recs, pages = [], 0
    info = {"keys": 0, "records": 0, "stem_bytes": 0, "chains_lost": 0, "slots_scanned": 0}
    byp = None
    for rec, d, b in be.scan(**kw):
        part = rec_list(rec)
        assert d["records"] == len(part) and d["stem_bytes"] == int(rec["stem_off"][-1]) == len(rec["stem_bytes"])
        assert rec["stem_off"][0] == 0
        recs += part
        for f in info:
            info[f] += d[f]
        byp = b.astype(np.int64) if byp is None else byp + b.astype(np.int64)
        pages += 1
    return recs, info, byp.tolist(), pages
