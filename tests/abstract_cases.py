"""Named inputs for the index abstracts and the secondary search (a helper, no tests, no GPU code).

yrwi_abstract.hip has hand-made edges: a text parser with one thread per byte position and 16
positions per thread (4,096 bytes per workgroup), an atomicMin that ends a parse at the first bad
segment start, 72-bit url keys packed as 64 + 8 bits, two chained stable radix sorts, a 32-word
bit mask and Java's int overflow in `size * 1000 + count`.  Every generator here aims at one of
them.  tests/test_abstract_cases_ref.py shows with oracle/abstracts.py alone that each input is
what its name says; tests/test_gpu_abstracts_adversarial.py feeds the same inputs to the device.

compress_cases() / multi_term()   lists for yrwi_index_abstracts (compressIndex)
join_cases()                      abstracts for yrwi_secondary_search that the oracle accepts
peer_abstracts() / oracle_plan()  random well-formed abstracts of several peers (the caller's generator),
                                  and the oracle's join and plan for any abstracts
refusal_cases()                   abstracts that must be refused
wrap_case()                       the one large input: a map of 2,147,484 urls
expected()                        the oracle's answer in the shape RWIIndex.secondary_search returns

Everything is deterministic: counters run through an odd multiplier modulo 2^36 (a bijection),
no random generator."""

import functools
from collections import namedtuple

import numpy as np

import abstracts as ab

B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"  # Base64Order: code -> character
_CODE = bytes(B64.index(c) if c in B64 else 255 for c in range(256))
_B64A = np.frombuffer(B64, dtype=np.uint8)
M36 = (1 << 36) - 1


def b64key(u: bytes) -> bytes:
    """sorts url hashes in Base64Order (the order of a stored list)"""
    return bytes(u).translate(_CODE)


def enc6(x: int) -> bytes:
    return bytes(B64[(x >> (30 - 6 * j)) & 63] for j in range(6))


def scr(i: int, mul: int = 2654435761) -> int:
    """a bijection on 36 bits (odd multiplier): distinct counters give distinct prefixes"""
    return (i * mul + 12345) & M36


def make_rows(urls) -> np.ndarray:
    """a stored list as tests/test_abstracts.py builds it: 40-byte rows, the url hash in [:12],
    Base64Order, the language cell (bytes 22:24) set"""
    urls = sorted(set(urls), key=b64key)
    rows = np.zeros((len(urls), 40), dtype=np.uint8)
    if urls:
        rows[:, :12] = np.frombuffer(b"".join(urls), dtype=np.uint8).reshape(-1, 12)
    rows[:, 22:24] = ord("e")
    return rows


def row_list(rows):
    return [bytes(r) for r in rows]


def hashes(rows):
    return [bytes(r[:12]) for r in rows]


def peer_abstracts(rng, words, npeers, base):
    """every peer holds a random part of each word's url universe; arrival order shuffled"""
    peers = sorted({bytes(B64[int(x)] for x in rng.integers(0, 64, 12)) for _ in range(npeers)})
    out = []
    for p in peers:
        for w in words:
            sel = [u for u in base[w] if rng.random() < 0.4]
            out.append((w, p, ab.compress_index([u + bytes(28) for u in sel])))
    order = rng.permutation(len(out))
    return [out[i] for i in order], peers


def oracle_plan(abstracts, words, mypeer, checked=()):
    s = ab.SecondarySearch()
    s.checked = set(checked)
    for w, p, t in abstracts:
        s.add_abstract(w, ab.decompress_index(t, p))
    return s.prepare(words, mypeer)


# ------------------------------------------------------------------ compressIndex
# ex_mode: None (no exclude term), "absent" (an exclude term the index does not have), "self" (the
# term itself) or "list" (ex_rows stored under a term of their own)
CCase = namedtuple("CCase", "name rows ex_mode ex_rows")
SIZES = (1, 255, 256, 257, 1025)


def one_host_urls(n):
    return [enc6(scr(i)) + b"oneHST" for i in range(n)]


def own_host_urls(n):
    return [enc6(scr(i)) + enc6(scr(i, 0x9E3779B1)) for i in range(n)]


def host_order_hosts():
    """384 hosts: every character in each of the 6 host positions in turn.  Position p's base is
    six times one letter (another letter per position), so the 384 are distinct."""
    out = []
    for p in range(6):
        base = bytes([B64[10 + p]]) * 6
        for c in B64:
            out.append(base[:p] + bytes([c]) + base[p + 1:])
    return out


def host_order_urls():
    urls = []
    for i, host in enumerate(host_order_hosts()):
        for _ in range(1 + i % 3):
            urls.append(enc6(scr(len(urls))) + host)
    return urls


def exclusion_base():
    """300 postings over 23 hosts of uneven size"""
    hosts = [enc6(scr(h, 77773)) for h in range(23)]
    return make_rows(enc6(scr(i)) + hosts[scr(i) % 23] for i in range(300))


def one_host_of(rows):
    """a host of the list, in the middle of its raw-byte host order, with several postings"""
    hs = [h[6:] for h in hashes(rows)]
    many = sorted({h for h in hs if hs.count(h) >= 3})
    return many[len(many) // 2]


def larger_exclude(rows):
    """every third url of the list, 2 n foreign urls on the list's hosts, and the smallest and the
    largest key there is: more rows than the list, keys before and after all of its keys"""
    own = hashes(rows)
    hosts = sorted({h[6:] for h in own})
    foreign = [enc6(scr(i, 0x85EBCA6B)) + hosts[i % len(hosts)] for i in range(2 * len(own))]
    have = set(own)
    foreign = [u for u in foreign if u not in have]
    return make_rows(own[::3] + foreign + [B64[:1] * 12, B64[63:] * 12])


@functools.lru_cache(maxsize=None)
def compress_cases():
    out = []
    for n in SIZES:
        out.append(CCase("one_host_%d" % n, make_rows(one_host_urls(n)), None, None))
        out.append(CCase("own_host_%d" % n, make_rows(own_host_urls(n)), None, None))
    out.append(CCase("host_order", make_rows(host_order_urls()), None, None))
    base = exclusion_base()
    h = one_host_of(base)
    out += [
        CCase("ex_absent", base, "absent", None),
        CCase("ex_self", base, "self", None),
        CCase("ex_all_but_first", base, "list", base[1:]),
        CCase("ex_all_but_last", base, "list", base[:-1]),
        CCase("ex_one_host", base, "list", base[np.array([u[6:] == h for u in hashes(base)])]),
        CCase("ex_every_second", base, "list", base[1::2]),
        CCase("ex_larger", base, "list", larger_exclude(base)),
        # the exclusion meets the sizes of the block edges too
        CCase("ex_every_second_257", make_rows(own_host_urls(257)), "list", make_rows(own_host_urls(257))[::2]),
    ]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def excluded_rows(c):
    """the rows compressIndex is given as its excludeContainer, or None"""
    if c.ex_mode == "self":
        return c.rows
    return c.ex_rows if c.ex_mode == "list" else None


def compress_expected(c) -> bytes:
    ex = excluded_rows(c)
    return ab.compress_index(row_list(c.rows), row_list(ex) if ex is not None else None)


MT1, MT2, MT_ABSENT = b"ABSmulti1___", b"ABSmulti2___", b"ABSnolist___"


def multi_term():
    """(lists, calls): a call that names one term twice, and one whose last term has no list"""
    lists = {MT1: make_rows(host_order_urls()[:40]), MT2: make_rows(own_host_urls(70))}
    calls = [("same_term_twice", [MT1, MT2, MT1]), ("last_term_absent", [MT1, MT2, MT_ABSENT])]
    return lists, calls


# ------------------------------------------------------------------ decompressIndex, join, plan
JCase = namedtuple("JCase", "name abstracts nwords mypeer checked")  # abstracts: (word, peer, text), arrival order
NOBODY = b"nobody______"


def W(i: int) -> bytes:
    return b"word%02d______" % i


def P(i: int) -> bytes:
    return b"peer%04d____" % i


def text(urls) -> bytes:
    """the abstract a peer writes for these urls"""
    return ab.compress_index(row_list(make_rows(urls)))


def U(i: int, host: bytes = b"hostUU") -> bytes:
    return enc6(scr(i)) + host


def expected(case):
    """(join [(url, peer)], words, plan [(peer, urls, words)]) from the oracle, as
    RWIIndex.secondary_search returns them; raises ValueError where decompress_index does"""
    s = ab.SecondarySearch()
    s.checked = set(case.checked)
    for w, p, t in case.abstracts:
        s.add_abstract(w, ab.decompress_index(t, p))
    join, plan = s.prepare(list(range(case.nwords)), case.mypeer)  # only the number of include words counts
    return [(u, next(iter(join[u]))) for u in sorted(join)], sorted(s.cache), plan


def segment_starts(t: bytes):
    """where decompressIndex looks for a "host:" in an abstract: the body start and behind every ','"""
    return [1] + [i + 1 for i in range(1, len(t) - 1) if t[i] == 0x2C]


# ---- alphabet
def alphabet_urls():
    """every character in each of the 12 url positions in turn (a base per position, as
    host_order_hosts): 768 urls.  Positions 10 and 11 are the characters that the device splits
    between the 64-bit and the 8-bit key part."""
    out = []
    for p in range(12):
        base = bytes([B64[20 + p]]) * 12
        for c in B64:
            out.append(base[:p] + bytes([c]) + base[p + 1:])
    return out


def alphabet_case():
    urls = alphabet_urls()
    a = [(W(0), P(1 + j), text(urls[j::3])) for j in range(3)]
    a += [(W(1), P(4), text(urls[0::2])), (W(1), P(5), text(urls[0::5]))]
    order = [3, 0, 4, 2, 1]
    return JCase("alphabet", [a[i] for i in order], 2, NOBODY, ())


# ---- parser alignment
ALIGN_PREFIX = b",host00:AAAAAA,h"  # 16 bytes without braces: any cut of it is an empty abstract
NALIGN = 17


@functools.lru_cache(maxsize=None)
def alignment_body() -> bytes:
    """more than three 4,096-byte parse blocks: 120 hosts, each run length 1..40 three times, the
    lengths rotated until a segment starts 1..15 bytes before a block boundary -- a prefix of 0..16
    bytes then moves that start onto the last byte of the block, the boundary and one past it"""
    for rot in range(40):
        segs = []
        for h in range(120):
            r = 1 + (7 * h + rot) % 40
            segs.append(enc6(scr(h, 0x5BD1E995)) + b":" + b"".join(enc6(scr(1000 * h + j)) for j in range(r)))
        body = b"{" + b",".join(segs) + b"}"
        if any(4081 <= s % 4096 <= 4095 for s in segment_starts(body)):
            return body
    raise AssertionError("no rotation puts a segment start before a block boundary")


def alignment_cases():
    body = alignment_body()
    urls = sorted(ab.decompress_index(body, P(2)))
    other = text(urls + [U(i, b"foreig") for i in range(10)])  # larger: the body's word folds first
    return [JCase("align_%02d" % k, [(W(0), P(1), ALIGN_PREFIX[:k]), (W(0), P(2), body), (W(1), P(3), other)],
                  2, NOBODY, ()) for k in range(NALIGN)]


def alignment_starts(case):
    """segment starts of the body as positions in the call's concatenated text"""
    off = len(case.abstracts[0][2])
    return [off + s for s in segment_starts(case.abstracts[1][2])]


# ---- stop rules: the middle abstract of three, and the urls it contributes
A0, B1, C2 = b"AAAAAAhost00", b"BBBBBBhost01", b"CCCCCChost02"
STOPS = [
    ("empty_braces", b"{}", []),
    ("open_brace_only", b"{", []),
    ("close_brace_only", b"}", []),
    ("zero_length", b"", []),
    ("no_closing_brace", b"{host00:AAAAAA", []),
    ("host_without_urls", b"{host00:}", []),
    ("empty_host_then_host", b"{host00:,host01:BBBBBB}", [B1]),
    ("trailing_comma", b"{host00:AAAAAA,}", [A0]),
    ("leading_comma", b"{,host00:AAAAAA}", []),
    ("double_comma", b"{host00:AAAAAA,,host01:BBBBBB}", [A0]),
    ("last_segment_12_bytes", b"{host00:AAAAAA,host01:BBBBB}", [A0]),
    ("byte_6_not_colon", b"{host00:AAAAAA,host01xBBBBBB,host02:CCCCCC}", [A0]),
    ("run_of_7_behind_stop", b"{host00:AAAAAA,host01xBBBBBB,host02:CCCCCCC}", [A0]),
    ("bad_bytes_behind_stop", b"{host00:AAAAAA,host01xBB BBB,ho,t02:CC:CCC}", [A0]),
    ("url_twice_one_segment", b"{host00:AAAAAAAAAAAA}", [A0]),
    ("url_twice_two_segments", b"{host00:AAAAAA,host00:AAAAAA}", [A0]),
]


def stop_neighbours():
    first = [U(i, b"hostN1") for i in range(9)] + [U(i, b"-ostN1") for i in range(3)]
    last = [U(100 + i, b"hostN3") for i in range(7)] + [U(100 + i, b"zostN3") for i in range(4)]
    return first, last


def stop_cases():
    first, last = stop_neighbours()
    return [JCase("stop_" + name, [(W(0), P(1), text(first)), (W(0), P(2), mid), (W(0), P(3), text(last))], 1, NOBODY, ())
            for name, mid, _ in STOPS]


# ---- refusals
def well_formed_case():
    first, last = stop_neighbours()
    return JCase("well_formed", [(W(0), P(1), text(first)), (W(0), P(2), text([A0, B1])), (W(0), P(3), text(last))],
                 1, NOBODY, ())


REFUSED_TEXTS = [
    ("run_of_7_first_abstract", 0, b"{host00:AAAAAAA}"),
    ("run_of_7_last_abstract", 2, b"{host00:AAAAAA,host01:BBBBBBB}"),
    ("non_base64_in_run", 1, b"{host00:AAA:AA}"),
    ("non_base64_in_host", 1, b"{ab,cde:AAAAAA}"),
    ("comma_inside_url", 1, b"{host00:AAAAAABBB,BB}"),
    ("brace_inside_run", 1, b"{host00:AAAAAA}host01:BBBBBB}"),
]


def refusal_cases():
    """calls that must fail; all but words_33 because decompress_index raises"""
    good = well_formed_case().abstracts
    out = []
    for name, slot, t in REFUSED_TEXTS:
        a = list(good)
        a[slot] = (a[slot][0], a[slot][1], t)
        out.append(JCase("refuse_" + name, a, 1, NOBODY, ()))
    out.append(JCase("refuse_words_33", [(W(i), P(1), text([A0])) for i in range(33)], 33, NOBODY, ()))
    return out


# ---- addAbstract
def add_abstract_cases():
    u = U(0)
    newest = [(W(0), P(3), text([u, U(1)])), (W(0), P(2), text([u, U(2)])), (W(0), P(1), text([u, U(3)]))]
    twice = [(W(0), P(1), text([U(i) for i in range(0, 8)])), (W(0), P(2), text([U(i) for i in range(4, 12)])),
             (W(0), P(1), text([U(i) for i in range(6, 10)]))]
    return [JCase("add_newest_wins_over_rank", newest, 1, NOBODY, ()),
            JCase("add_same_peer_twice", twice, 1, NOBODY, ())]


# ---- fold order
def fold_cases():
    c = [U(0), U(1)]  # common to every word
    last_smallest = [(W(0), P(1), text(c + [U(i) for i in range(10, 13)])),
                     (W(1), P(2), text(c + [U(i) for i in range(20, 22)])),
                     (W(2), P(3), text(c + [U(30)]))]
    equal = [(W(1), P(2), text(c + [U(20)])), (W(0), P(1), text(c + [U(10)]))]
    single = [(W(5), P(1), text(c + [b"0singl_ostUU", b"-singl-ostUU", b"_singlhostUU", b"zsinglhostUU"]))]
    w32 = [(W(i), P(1), text(c)) for i in range(31)] + [(W(31), P(2), text(c[:1]))]
    one_empty = [(W(0), P(1), text(c)), (W(1), P(2), b"{}"), (W(1), P(3), b"")]
    disjoint = [(W(0), P(1), text([U(i) for i in range(0, 5)])), (W(1), P(2), text([U(i) for i in range(5, 9)]))]
    return [JCase("fold_smallest_is_last_word", last_smallest, 3, NOBODY, ()),
            JCase("fold_equal_sizes", equal, 2, NOBODY, ()),
            JCase("fold_single_word", single, 1, NOBODY, ()),
            JCase("fold_32_words_bit_31", w32, 32, NOBODY, ()),
            JCase("fold_one_word_all_empty", one_empty, 2, NOBODY, ()),
            JCase("fold_all_texts_zero_length", [(W(0), P(1), b""), (W(1), P(2), b"")], 2, NOBODY, ()),
            JCase("fold_disjoint_words", disjoint, 2, NOBODY, ()),
            JCase("fold_nwords_one_too_large", last_smallest, 4, NOBODY, ())]


# ---- plan
PEER_COUNTS = (1, 2, 255, 256, 257)


def plan_cases():
    five = [(W(0), P(i), text([U(10 * i + j) for j in range(3)])) for i in range(1, 6)]
    out = [JCase("plan_skip_mypeer_and_checked", five, 1, P(2), (P(4),))]
    for n in PEER_COUNTS:
        # arrival order is not peer order
        a = [(W(0), P((37 * i) % n), text([U(2 * i), U(2 * i + 1, b"-ostUU")])) for i in range(n)]
        out.append(JCase("plan_%d_peers" % n, a, 1, NOBODY, ()))
    alpha = alphabet_urls()
    mixed = alpha[0:64] + alpha[6 * 64:7 * 64]  # first url character and first host character sweep the alphabet
    out.append(JCase("plan_urls_in_string_order", [(W(0), P(1), text(mixed)), (W(0), P(2), text(alpha[64:80]))],
                     1, NOBODY, ()))
    u1, u2, u3 = U(1), U(2), U(3)
    partial = [(W(0), P(1), text([u1, u2, u3])), (W(1), P(2), text([u1, u2])), (W(1), P(1), text([u2]))]
    out.append(JCase("plan_peer_with_some_words", partial, 2, NOBODY, ()))
    return out


@functools.lru_cache(maxsize=None)
def join_cases():
    """every case the oracle accepts, the large one excepted"""
    out = ([alphabet_case()] + alignment_cases() + stop_cases() + [well_formed_case()] + add_abstract_cases()
           + fold_cases() + plan_cases())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---- the int wrap
NWRAP = 2_147_484  # the smallest map size whose size * 1000 is negative as a Java int
WRAP_HOST, WRAP_OTHER = b"wrapHS", b"otherH"


def wrap_in_range(n: int = NWRAP):
    return [0, n - 1] + [(n // 30) * k + 5 for k in range(1, 29)]


def wrap_y_urls(n: int = NWRAP):
    inside = [enc6(i) + WRAP_HOST for i in wrap_in_range(n)]
    outside = [enc6(n + i) + WRAP_HOST for i in range(10)] + [enc6(i) + WRAP_OTHER for i in range(10)]
    return inside, outside


@functools.lru_cache(maxsize=2)
def wrap_text(n: int = NWRAP) -> bytes:
    """one host, the urls enc6(0) .. enc6(n - 1): n distinct urls in 6 n + 9 bytes"""
    i = np.arange(n, dtype=np.int64)
    pre = np.empty((n, 6), dtype=np.uint8)
    for j in range(6):
        pre[:, j] = _B64A[(i >> (30 - 6 * j)) & 63]
    return b"{" + WRAP_HOST + b":" + pre.tobytes() + b"}"


def wrap_case(n: int = NWRAP):
    """word X (the first in String order) has n urls from peer 1, word Y 50 urls from peer 2, 30 of
    them among X's"""
    inside, outside = wrap_y_urls(n)
    return JCase("wrap_%d" % n, [(W(1), P(2), text(inside + outside)), (W(0), P(1), wrap_text(n))], 2, NOBODY, ())


def wrap_expected(n: int = NWRAP):
    """what expected() would give, from join_order and Y's small map: no map of n entries is built"""
    inside, outside = wrap_y_urls(n)
    peers = [P(1), P(2)]
    first = ab.join_order([n, len(inside) + len(outside)])[0]
    urls = sorted(inside)
    # the first map's peer sets stay; its peer is then asked for the words in which it holds those urls
    return [(u, peers[first]) for u in urls], [W(0), W(1)], [(peers[first], urls, [W(first)])]
