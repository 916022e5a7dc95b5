"""Adversarial 40-byte WordReferenceRow rows for the rank path (a helper, no tests).

synth.cpp draws plausible web data: lastModified in 10957..20454, wordsintext and
hitcount >= 1, worddistance 0, doctype 't', six languages, flag bits 0 and 19..29,
reserved bytes 0.  The rows here are valid (well-formed, distinct, ascending url
hashes; a language that is not 0x0000) and otherwise as hostile as the row format
allows: every cell is drawn from an edge palette or uniformly from its whole range.

Column letters are WordReferenceRow's (java_literal.COL)."""

import numpy as np

import java_literal as jl

NOW_DAY = 20741
BYTE_EDGES = np.array([0, 1, 2, 127, 128, 254, 255])
WORD_EDGES = np.array([0, 1, 255, 256, 257, 32767, 32768, 65534, 65535, NOW_DAY - 1, NOW_DAY, NOW_DAY + 1])
LANGS = [b"en", b"de", b"zz", b"\xff\xff", b"e\0", b"\0n", b"EN"]  # never 0x0000 (YRWI_E_NULL_LANGUAGE)

BYTE_COLS = "uxymncroi"            # one-byte cardinal cells
WORD_COLS = "aswpt"                # two-byte cardinal cells
MINMAX_COLS = "cxywptromnu"        # the 11 fields WordReferenceVars.min/max fold
CONST_COLS = list(MINMAX_COLS) + ["a", "cwu", "all"]
_ALPHA = np.frombuffer(jl.ALPHA, dtype=np.uint8)


def _off(c):
    return jl.COL[c][0]


def _put(rows, c, v):
    """Store the values v (array or scalar) into column c, big-endian."""
    o, w = jl.COL[c]
    v = np.broadcast_to(np.asarray(v, dtype=np.int64), (len(rows),))
    for j in range(w):
        rows[:, o + j] = (v >> (8 * (w - 1 - j))) & 0xFF


def col_values(rows, c):
    o, w = jl.COL[c]
    v = np.zeros(len(rows), dtype=np.int64)
    for j in range(w):
        v = (v << 8) | rows[:, o + j]
    return v


def _hashes(rows, rng, first_char_min=0, hosts=None):
    """n distinct url hashes in ascending Base64Order: chars 0..5 strictly rising
    (first char index >= first_char_min), chars 6..11 (the host hash) drawn from
    a pool of `hosts` hosts, so several urls share a host (authority)."""
    n = len(rows)
    base = first_char_min << 30
    cum = np.cumsum(rng.integers(1, 1 << 12, n + 1, dtype=np.int64))  # random gaps, scaled to fill the range
    hi = base + np.floor(cum[:-1] / cum[-1] * ((1 << 36) - base - 1)).astype(np.int64)
    assert hi[-1] < (1 << 36) and (np.diff(hi) > 0).all()
    pool = rng.integers(0, 1 << 36, hosts or max(1, n // 6), dtype=np.int64)
    lo = pool[rng.integers(0, len(pool), n)]
    for j in range(6):
        rows[:, j] = _ALPHA[(hi >> (6 * (5 - j))) & 63]
        rows[:, 6 + j] = _ALPHA[(lo >> (6 * (5 - j))) & 63]


def _edge_cells(rows, rng):
    n = len(rows)

    def draw(edges, top):
        v = edges[rng.integers(0, len(edges), n)]
        u = rng.random(n) < 0.3
        v[u] = rng.integers(0, top, int(u.sum()))
        return v

    for c in BYTE_COLS:
        _put(rows, c, draw(BYTE_EDGES, 256))
    for c in WORD_COLS:
        _put(rows, c, draw(WORD_EDGES, 65536))
    rows[:, _off("d")] = rng.integers(0, 256, n)                   # any doctype
    langs = np.frombuffer(b"".join(LANGS), dtype=np.uint8).reshape(-1, 2)
    rows[:, _off("l"):_off("l") + 2] = langs[rng.integers(0, len(langs), n)]
    rows[:, _off("z"):_off("z") + 4] = rng.integers(0, 256, (n, 4))  # any flag byte
    rows[:, _off("g")] = rng.integers(1, 256, n)                   # reserved, nonzero
    rows[:, _off("k")] = rng.integers(1, 256, n)


def adv_rows(n, seed, mode="edge", first_char_min=0, hosts=None):
    """n valid rows, ascending distinct url hashes, deterministic in (n, seed, mode).

    mode "edge":        every cell from the edge palette (70 %) or uniform (30 %)
    mode "few":         all 28 feature bytes copied from one of 2 or 3 template rows
    mode "const:<col>": edge rows with one column of CONST_COLS held constant
                        ("cwu": the tf triple; "all": every cardinal cell)
    mode "tight":       const:all, distance 0, flag bits 0, 24 and 25 only: every normalised
                        term is 0 (max == min), so an upper bound of the score built
                        from the terms' maxima equals the score, and scores tie in
                        long runs"""
    rng = np.random.default_rng([seed, n, sum(mode.encode())])
    rows = np.zeros((n, 40), dtype=np.uint8)
    if n == 0:
        return rows
    _hashes(rows, rng, first_char_min, hosts)
    if mode == "few":
        tpl = np.zeros((2 + seed % 2, 40), dtype=np.uint8)
        _edge_cells(tpl, rng)
        rows[:, 12:] = tpl[rng.integers(0, len(tpl), n), 12:]
        return rows
    _edge_cells(rows, rng)
    if mode.startswith("const:") or mode == "tight":
        col = "all" if mode == "tight" else mode[6:]
        assert col in CONST_COLS, col
        cols = MINMAX_COLS + "ai" if col == "all" else col
        for c in cols:
            edges = BYTE_EDGES if jl.COL[c][1] == 1 else WORD_EDGES
            _put(rows, c, int(edges[rng.integers(0, len(edges))]))
        if mode == "tight":
            rows[:, _off("z"):_off("z") + 4] &= np.array([1, 0, 0, 3], dtype=np.uint8)
            _put(rows, "i", 0)  # D = 0: the distance term is 0 as well
    elif mode != "edge":
        raise ValueError(mode)
    return rows


def span_rows(cols, lo, d, pad_to=0, seed=0):
    """One row per value lo..lo+d of every column in `cols` (each column walks the
    span rotated by its own offset, so no two columns agree row by row); all other
    feature cells fixed, so each column's min = lo and max = lo + d.  Repeated
    under fresh url hashes up to pad_to rows."""
    m = d + 1
    n = max(m, pad_to)
    rng = np.random.default_rng([seed, lo, d, n])
    rows = np.zeros((n, 40), dtype=np.uint8)
    _hashes(rows, rng, hosts=7)
    _put(rows, "a", 15000)
    _put(rows, "w", 50)
    _put(rows, "c", 3)
    _put(rows, "t", 9)
    rows[:, _off("d")] = ord("t")
    rows[:, _off("l"):_off("l") + 2] = np.frombuffer(b"en", dtype=np.uint8)
    v = np.arange(n, dtype=np.int64) % m
    for j, c in enumerate(cols):
        _put(rows, c, lo + (v + 37 * j) % m)
    return rows


def flag_walk_rows(n, seed=0):
    """Edge rows whose flag word walks one bit at a time (0..31), then all ones, then none."""
    rows = adv_rows(n, seed, "edge")
    z = np.array([1 << j for j in range(32)] + [0xFFFFFFFF, 0], dtype=np.int64)[np.arange(n) % 34]
    for j in range(4):  # Bitfield bit p is bit p % 8 of byte p >> 3
        rows[:, _off("z") + j] = (z >> (8 * j)) & 0xFF
    return rows


def universe_lists(seed, n, mode="edge", fracs=(1.0, 0.7, 0.5, 0.3)):
    """Lists over one universe of n urls (selection fractions `fracs`): the same url
    carries different cells in each list."""
    rng = np.random.default_rng(seed)
    uni = adv_rows(n, seed, mode)
    d = {}
    for j, frac in enumerate(fracs):
        r = adv_rows(n, seed + 100 + j, mode)
        r[:, :12] = uni[:, :12]
        d[b"TERMadv%s____" % bytes([65 + j])] = r[rng.random(n) < frac]
    return d


def url_keys(rows):
    """(hi, lo) 36-bit halves of the 72-bit Base64Order keys."""
    idx = np.array(jl.AHPLA, dtype=np.int64)[rows[:, :12]]
    hi = np.zeros(len(rows), dtype=np.int64)
    lo = np.zeros(len(rows), dtype=np.int64)
    for j in range(6):
        hi = (hi << 6) | idx[:, j]
        lo = (lo << 6) | idx[:, 6 + j]
    return hi, lo


def sort_rows(rows):
    hi, lo = url_keys(rows)
    return rows[np.lexsort((lo, hi))]


def hashcodes(rows):
    """ByteArray.hashCode of every url hash (ByteArray.java:80-84), as Java ints."""
    h = np.zeros(len(rows), dtype=np.int64)
    for j in range(12):
        h = (31 * h + rows[:, j]) & 0xFFFFFFFF
    return np.where(h >= 1 << 31, h - (1 << 32), h)


def shard_of(rows, r, world):
    """yrwi_open_shard's rule: the rows whose first url-hash char index >> (6 - log2 world) == r."""
    sh = 6 - (world.bit_length() - 1)
    first = np.array([jl.AHPLA[b] for b in rows[:, 0]], dtype=np.int64) if len(rows) else np.zeros(0, np.int64)
    return rows[(first >> sh) == r]


# ---------------------------------------------------------------- profiles
_FIELDS = [f for _, f in jl.PROFILE_FIELDS]
LOW, HIGH, WILD = (0, 1, 15), (15, 16, 22, 23, 24, 31), (-1, 32, 33, 47, 0, 12, 13)


def palette_profile(palette, seed):
    rng = np.random.default_rng(seed)
    p = jl.RankingProfile()
    for f in _FIELDS:
        setattr(p, f, int(palette[rng.integers(0, len(palette))]))
    return p


def single(field, c):
    """All zero except coeff_<field> = c: a wrong score names the field."""
    p = jl.RankingProfile()
    p.all_zero()
    setattr(p, "coeff_" + field, c)
    return p


# the terms of cardinal that read a posting's cells (ReferenceOrder.java:223-260)
CARDINAL_FIELDS = ["domlength", "urlcomps", "urllength", "posintext", "posofphrase", "posinphrase", "worddistance",
                   "date", "wordsintitle", "wordsintext", "phrasesintext", "llocal", "lother", "hitcount",
                   "termfrequency", "authority", "appurl", "app_dc_title", "app_dc_creator", "app_dc_subject",
                   "app_dc_description", "appemph", "catindexof", "cathasimage", "cathasaudio", "cathasvideo",
                   "cathasapp", "language"]


def adv_profiles(singles=True):
    """[(name, java_literal.RankingProfile)]: default, c5 (authority 13), /date, one
    profile per coefficient palette, the all-zero profile (every term << 0), and
    single(f, c) for every field with c cycling 15, 23, 7."""
    date = jl.RankingProfile()
    date.all_zero()
    date.coeff_date = 15
    out = [("default", jl.RankingProfile()),
           ("c5", jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")),
           ("date", date),
           ("low", palette_profile(LOW, 101)), ("high", palette_profile(HIGH, 102)),
           ("wild", palette_profile(WILD, 103))]
    if singles:
        zero = jl.RankingProfile()
        zero.all_zero()
        out.append(("single:none:0", zero))
        cs = (15, 23, 7)
        for i, f in enumerate(CARDINAL_FIELDS):
            c = cs[i % 3]
            if f == "authority" and c <= 12:
                c = 15  # the authority term exists only above 12
            out.append((f"single:{f}:{c}", single(f, c)))
    return out


FLAG_FIELDS = ["appurl", "app_dc_title", "app_dc_creator", "app_dc_subject", "app_dc_description", "appemph",
               "catindexof", "cathasimage", "cathasaudio", "cathasvideo", "cathasapp"]


def flag_profiles():
    """Distinct coefficients on all 11 flag terms (two assignments) and on language."""
    out = []
    for name, cs in (("flags_up", range(1, 12)), ("flags_down", range(15, 4, -1))):
        p = jl.RankingProfile()
        p.all_zero()
        for f, c in zip(FLAG_FIELDS, cs):
            setattr(p, "coeff_" + f, c)
        p.coeff_language = 13 if name == "flags_up" else 3
        out.append((name, p))
    return out


def distance_fold_rows(D, n, pad_to=0, seed=0):
    """n >= 2 rows whose max-distance fold (WordReferenceVars.max, :420-455) ends at
    D.  Up to the last row posintext is 1 and the stored distances walk 255, 248, ...
    over 0..255, so the fold stands at positions = [1 + 255]; the last row
    (distance 0) moves posintext to 256 -+ D.  For D > 511 posintext is 0 up to the
    last row, the fold stands at [0 + 1] and the last posintext is 1 + D.  With
    n == 2 the second row stores D itself (D <= 255).  Most stored distances lie
    above a small D: the negative term of cardinal.  pad_to appends rows (distance
    <= D, posintext as the last row's) that leave the fold alone."""
    assert n >= 2 and 1 <= D <= 65534
    m = max(n, pad_to)
    rng = np.random.default_rng([seed, D, m])
    rows = np.zeros((m, 40), dtype=np.uint8)
    _hashes(rows, rng, hosts=5)
    _put(rows, "a", 15000)
    _put(rows, "w", 50)
    _put(rows, "c", 3)
    rows[:, _off("d")] = ord("t")
    rows[:, _off("l"):_off("l") + 2] = np.frombuffer(b"en", dtype=np.uint8)
    od = (255 - 7 * np.arange(m, dtype=np.int64)) % 256
    od = np.roll(od, 1)  # row 0 is the clone (its distance is not folded), row 1 stores 255
    if n == 2:
        assert D <= 255
        p, od[1] = np.ones(m, dtype=np.int64), D
    elif D <= 511:
        p = np.ones(m, dtype=np.int64)
        p[n - 1:] = 256 - D if D <= 255 else 256 + D
        od[n - 1] = 0
    else:
        p = np.zeros(m, dtype=np.int64)
        od[n - 2] = 1
        p[n - 1:] = 1 + D
        od[n - 1] = 0
    od[n:] = np.minimum(od[n:], min(D, 255))
    _put(rows, "t", p)
    _put(rows, "i", od)
    return rows
