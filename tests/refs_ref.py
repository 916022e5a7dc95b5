"""Reference of yrwi_url_references (include/yrwi.h) over the {term hash: (n, 40) uint8 rows ascending by
url hash} dicts the other references use.  A helper for the tests, not an oracle of the query path.

The call has no reference method behind it; it is defined through calls the library already has, and so is
this module: a reference is a row that yrwi_remove_postings with the same arguments would remove, listed
here by construction -- every selected list in ascending term hash, its rows whose url hash is in the set
in the list's own order ("term"), and that listing sorted stably by url hash ("url").  check_remove() ties
the numbers to tests/update_ref.apply_remove, the sequential fold of the removal.

references(lists, urls, terms=None)   the Refs of a call; terms=None: every list
check_remove(lists, urls, terms, refs)   refs / lists_hit / lists_covered against apply_remove"""

import numpy as np

import update_ref as ur

STAT_KEYS = ("lists", "postings", "urls", "urls_found", "refs", "lists_hit", "lists_covered")
ORDERS = ("term", "url")
NO_TERMS, NO_ROWS = np.zeros((0, 12), np.uint8), np.zeros((0, 40), np.uint8)


def s12(a):
    """(n, >= 12) uint8 -> the hashes as (n,) S12 (no hash holds a NUL)"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint8)[:, :12]).view("S12").ravel()


class Refs:
    """counts: int64, one per url given; stats: the seven STAT_KEYS; by[order] = (terms (n, 12) uint8,
    rows (n, 40) uint8), the references in that order"""

    def __init__(self, counts, stats, by):
        self.counts, self.stats, self.by = counts, stats, by


def references(lists, urls, terms=None) -> Refs:
    urls = [bytes(u) for u in urls]
    uset = np.array(sorted(set(urls)), dtype="S12")
    names = list(lists) if terms is None else [bytes(t) for t in terms]
    sel = sorted({t for t in names if t in lists and len(lists[t])}, key=ur.url_key)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["lists"], st["urls"] = len(sel), len(uset)
    tparts, rparts = [NO_TERMS], [NO_ROWS]
    for t in sel:  # term ascending; a list's rows ascend by url hash
        l = lists[t]
        m = np.isin(s12(l), uset) if len(uset) else np.zeros(len(l), dtype=bool)
        k = int(m.sum())
        st["postings"] += len(l)
        st["refs"] += k
        st["lists_hit"] += k > 0
        st["lists_covered"] += k == len(l)
        if k:
            rparts.append(l[m])
            tparts.append(np.tile(np.frombuffer(t, dtype=np.uint8), (k, 1)))
    rows, tms = np.concatenate(rparts), np.concatenate(tparts)
    found, per = np.unique(s12(rows), return_counts=True)
    cnt = dict(zip((bytes(f) for f in found), (int(c) for c in per)))
    st["urls_found"] = len(found)
    counts = np.array([cnt.get(u, 0) for u in urls], dtype=np.int64)
    keys = [ur.url_key(bytes(r[:12])) for r in rows]
    order = np.array(sorted(range(len(rows)), key=keys.__getitem__), dtype=np.int64)  # (stable: terms stay ascending)
    return Refs(counts, st, {"term": (tms, rows), "url": (tms[order], rows[order])})


def check_remove(lists, urls, terms, refs: Refs):
    """the bridge to the call this is the read-only form of"""
    _, exp = ur.apply_remove(lists, urls, terms)
    got = (refs.stats["refs"], refs.stats["lists_hit"], refs.stats["lists_covered"])
    want = (exp["removed"], exp["terms"], exp["emptied_terms"])
    assert got == want, (got, want)
