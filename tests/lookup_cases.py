"""Lookup cases shared by the oracle tests (no device), the emulator tests (CPU, tiny) and the GPU tests (through the product C ABI): STRUCTURED inputs for
permute_expression_pair (csrc/lookupperm.hip), chosen so that every data-dependent decision of that file is taken on purpose and not by what random values happen to
give: the position of the 64-bit key window (word and bit offset of its shift), the number of radix passes, what one wave of the histogram sees, the number of
refinement stages and the edges of the tie mask, the sizes around the sort tile (4096) and the scan tile (2048), the multiset shapes of halo2's rule and the values it
must refuse.

A case is Case(k, bf, inputs, tables, tabidx): Python integers, u = 2^k - bf - 1 values per column; lookup l reads inputs[l] against tables[tabidx[l]].  A table that
IS one of the inputs (the same list object) is given to the product as the same device buffer.

Every kind asserts, in plain Python and when it is built, the property it is named after.  Those asserts check INPUTS only; they are never an expected result.
Expected results come from two references that must agree: oracle.lookup_permute (C) and rule() below, a direct transcription of halo2's rule."""
import random
from collections import Counter, namedtuple

import numpy as np

import parity_cases as pc
import zk_dcap_verifier_amd as z

Case = namedtuple("Case", "k bf inputs tables tabidx")

SORT_TILE, SCAN_TILE = 4096, 2048                                          # FS_TILE and XS_TILE of lookupperm.hip

BIT_LENGTHS = (1, 8, 9, 16, 17, 24, 32, 40, 48, 56, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 223, 224, 225, 253, 254)
# what L must give: the shift of the window and its split into a word and a bit offset, written out (not computed) for the edges
WINDOW_OF = {1: (0, 0, 0), 64: (0, 0, 0), 65: (1, 0, 1), 95: (31, 0, 31), 96: (32, 1, 0), 97: (33, 1, 1), 127: (63, 1, 31), 128: (64, 2, 0), 129: (65, 2, 1),
             191: (127, 3, 31), 192: (128, 4, 0), 193: (129, 4, 1), 223: (159, 4, 31), 224: (160, 5, 0), 225: (161, 5, 1), 253: (189, 5, 29), 254: (190, 5, 30)}
PASSES_OF = {1: 1, 8: 1, 9: 2, 16: 2, 17: 3, 24: 3, 32: 4, 40: 5, 48: 6, 56: 7, 63: 8, 64: 8}      # radix passes of a call whose widest column has L <= 64 bits

DIGIT_PATTERNS = ("one", "two", "three", "lane0", "distinct64", "mod256", "all255", "last_tile_only")
DIGIT_PASSES = (0, 3, 4, 7)

TIE_RANGES = (  # (lo, hi, shift): one, two and three 64-bit stages below the window
    (0, 0, 100), (0, 63, 100), (99, 99, 100), (63, 63, 64),
    (0, 64, 96), (20, 130, 131),
    (0, 189, 190), (3, 188, 190))

MULTISET_KINDS = ("zeros", "const_table", "two_runs_larger", "two_runs_smaller", "perm_dups", "same_buffer", "all_distinct", "one_distinct", "rep_min", "rep_max")
NOT_IN_TABLE_KINDS = ("below_min", "above_max", "between_window_ties", "other_table")

SMALL_SIZES = ((1, 0), (2, 0), (2, 2), (3, 1), (4, 5), (6, 5))
TILE_SIZES = ((12, 2047), (13, 4095), (13, 4094), (13, 4096), (13, 0), (13, 2047), (14, 8191))
TILE_U = {(12, 2047): 2048, (13, 4095): 4096, (13, 4094): 4097, (13, 4096): 4095, (13, 0): 8191, (13, 2047): 6144, (14, 8191): 8192}


def usable(k, bf):
    return (1 << k) - bf - 1


# ---- the second reference -------------------------------------------------------------------------------------------------------------------------------------
def rule(inp, tab, u):
    """halo2's permute_expression_pair on integers -> (permuted_input, permuted_table), u rows each: the input sorted; at the first row of every distinct input value
    one copy of it leaves the table (ValueError if there is none); the leftover table values, ascending, go to the repeated rows from the LAST one backwards."""
    pin = sorted(inp[:u])
    left = Counter(tab[:u])
    ptab, rep = [None] * u, []
    for r, v in enumerate(pin):
        if r == 0 or v != pin[r - 1]:
            if left[v] == 0:
                raise ValueError("ConstraintSystemFailure: %#x is not in the table" % v)
            left[v] -= 1
            ptab[r] = v
        else:
            rep.append(r)
    rest = sorted(left.elements())
    assert len(rest) == len(rep)
    for v in rest:
        ptab[rep.pop()] = v
    return pin, ptab


# ---- what the sort will decide, recomputed here to assert the inputs ---------------------------------------------------------------------------------------------
def window(vals):
    """(L, shift, word offset, bit offset) of a column: L = bits of the OR of its values (1 for an all-zero column), the key is bits [shift, shift + 64)"""
    m = 0
    for v in vals:
        m |= v
    L = max(1, m.bit_length())
    s = max(0, L - 64)
    return L, s, s >> 5, s & 31


def key_of(v, shift):
    return (v >> shift) & ((1 << 64) - 1)


def tie_mask(vals, shift):
    """OR of x ^ y over the neighbours that tie on the window, in the order a STABLE sort by the window key leaves"""
    order = sorted(vals, key=lambda v: key_of(v, shift))
    m = 0
    for x, y in zip(order, order[1:]):
        if key_of(x, shift) == key_of(y, shift):
            m |= x ^ y
    return m


def needs_refinement(vals):
    """a stable sort by the window key alone leaves the column out of order"""
    _, s, _, _ = window(vals)
    order = sorted(vals, key=lambda v: key_of(v, s))
    return order != sorted(vals)


def _distinct(R, rnd, count):
    vals = set()
    while len(vals) < count:
        vals.add(rnd.randrange(R))
    vals = list(vals)
    rnd.shuffle(vals)
    return vals


def _draw(rnd, tab, u, must=()):
    """u input values drawn from the table, the values of `must` among them"""
    inp = [rnd.choice(tab) for _ in range(u)]
    for i, v in enumerate(must):
        if i < u:
            inp[i] = v
    rnd.shuffle(inp)
    return inp


# ---- bit_length ------------------------------------------------------------------------------------------------------------------------------------------------
def bit_length_column(R, u, L, rnd):
    top = 1 << (L - 1)
    if L == 254:
        vals = [rnd.randrange(top, R) if i % 3 == 0 else rnd.randrange(R) for i in range(u)]
        vals[0] = R - 1
    else:
        vals = [rnd.randrange(1 << L) for _ in range(u)]
        vals[0] = top | rnd.randrange(top)
    rnd.shuffle(vals)
    return vals


def bit_length_pair(R, u, L, seed=0):
    """(input, table): the OR of each column has exactly L bits, the values are otherwise random below 2^L (below r, with r - 1, at L = 254)"""
    rnd = random.Random(seed * 7919 + L)
    tab = bit_length_column(R, u, L, rnd)
    widest = max(tab)
    inp = _draw(rnd, tab, u, must=(widest,))
    for col in (inp, tab):
        got = window(col)
        assert got[0] == L and got[1] == max(0, L - 64) and got[2:] == (got[1] >> 5, got[1] & 31) and all(0 <= v < R for v in col), (L, got)
        if L in WINDOW_OF:
            assert got[1:] == WINDOW_OF[L], (L, got)
        assert got[2] + 2 < 8                                              # (a canonical value's window never reads past word 7: only a refinement stage does)
    assert L != 254 or (R - 1 in tab and R - 1 in inp)
    return inp, tab


def bit_length(R, k, bf, Ls, seed=0):
    """one lookup per L, each with a table of its own.  One L <= 64 alone pins the pass count PASSES_OF[L]"""
    u = usable(k, bf)
    pairs = [bit_length_pair(R, u, L, seed + i) for i, L in enumerate(Ls)]
    return Case(k, bf, [p[0] for p in pairs], [p[1] for p in pairs], list(range(len(Ls))))


def passes(case):
    """radix passes of the window stage of the call: from the widest key of any column"""
    bits = max(min(64, window(col[:usable(case.k, case.bf)])[0]) for col in case.inputs + case.tables)
    return (bits + 7) // 8


# ---- digit_pattern ---------------------------------------------------------------------------------------------------------------------------------------------
def pattern_digit(pattern, i, u):
    """digit of row i; a wave of the histogram kernel sees one aligned run of 64 rows"""
    j, run = i % 64, i // 64
    if pattern == "one":
        return 0xA5
    if pattern == "two":
        return (0x11, 0xEE)[j % 2]
    if pattern == "three":
        return (0x80, 0x01, 0x7F)[j % 3]
    if pattern == "lane0":
        return 0x42 if j == 0 else 0x99
    if pattern == "distinct64":
        return j + 64 * (run % 4)
    if pattern == "mod256":
        return i % 256
    if pattern == "all255":
        return 255
    if pattern == "last_tile_only":
        last = (u - 1) // SORT_TILE * SORT_TILE
        return 201 if i >= last and j % 2 else 7
    raise ValueError(pattern)


def digit_pattern_column(u, p, pattern):
    vals = [pattern_digit(pattern, i, u) << (8 * p) for i in range(u)]
    L, s, _, _ = window(vals)
    assert s == 0 and 8 * p < L <= 8 * (p + 1), (p, pattern, L)             # the key is the value, pass p is its last pass
    for i, v in enumerate(vals):
        # digit p follows the pattern, every lower digit is 0: passes 0 .. p - 1 move nothing (stable), pass p meets the rows in their original order
        assert (key_of(v, s) >> (8 * p)) & 255 == pattern_digit(pattern, i, u) and key_of(v, s) & ((1 << (8 * p)) - 1) == 0 and v >> (8 * (p + 1)) == 0
    runs = [set(pattern_digit(pattern, i, u) for i in range(b, min(u, b + 64))) for b in range(0, u, 64)]
    want = {"one": {1}, "two": {2}, "three": {3}, "lane0": {2}, "distinct64": {64}, "mod256": {64}, "all255": {1}, "last_tile_only": {1, 2}}[pattern]
    full = [len(r) for b, r in zip(range(0, u, 64), runs) if b + 64 <= u]
    assert set(full) <= want and (not full or max(full) == max(want)), (pattern, set(full))
    if pattern == "last_tile_only":
        last = (u - 1) // SORT_TILE * SORT_TILE
        assert all((v >> (8 * p)) == 7 for v in vals[:last]) and any((v >> (8 * p)) == 201 for v in vals[last:]) and u - last <= SORT_TILE
    return vals


def digit_pattern(k, bf, p, patterns=DIGIT_PATTERNS):
    """one lookup per pattern; its input column and its table column both follow the pattern by row (two buffers, equal values)"""
    u = usable(k, bf)
    cols = [digit_pattern_column(u, p, pat) for pat in patterns]
    case = Case(k, bf, [list(c) for c in cols], cols, list(range(len(cols))))
    assert passes(case) == p + 1
    return case


# ---- ties ------------------------------------------------------------------------------------------------------------------------------------------------------
def _windows(R, rnd, count, shift):
    """distinct 64-bit window values with the top bit set (the column's OR then has exactly shift + 64 bits), such that any bits below make a value below r"""
    assert 0 < shift and shift + 64 <= 254
    hi = min(1 << 64, R >> shift)
    ws = set()
    while len(ws) < count:
        ws.add(rnd.randrange(1 << 63, hi))
    return sorted(ws)


def ties_column(R, u, lo, hi, shift, rnd, unique=0):
    """u values in groups that agree on the window at `shift` and on everything below it except bits lo and hi; `unique` further windows hold one value each"""
    assert lo <= hi < shift and u - unique >= 8
    variants = [(a << lo) | (b << hi) for a in (0, 1) for b in (0, 1)] if lo != hi else [0, 1 << lo]
    groups = unique or max(1, (u - unique) // (2 * len(variants)))         # (some_groups: as many tied windows as unique ones)
    assert u - unique >= len(variants) * groups
    ws = _windows(R, rnd, groups + unique, shift)
    rnd.shuffle(ws)
    clear = ~((1 << lo) | (1 << hi))
    common = [rnd.randrange(1 << shift) & clear for _ in range(groups)]
    vals = [(ws[i % groups] << shift) | common[i % groups] | variants[(i // groups) % len(variants)] for i in range(u - unique)]
    vals += [(w << shift) | rnd.randrange(1 << shift) for w in ws[groups:]]
    rnd.shuffle(vals)
    assert len(vals) == u and all(v < R for v in vals)
    return vals


def assert_ties(col, lo, hi, shift):
    got = window(col)
    assert got[1] == shift, (got, shift)
    assert tie_mask(col, shift) == (1 << lo) | (1 << hi), (hex(tie_mask(col, shift)), lo, hi)
    assert needs_refinement(col)


def ties_pair(R, u, lo, hi, shift, seed=0, some_groups=False):
    rnd = random.Random(seed * 104729 + 1000 * lo + hi)
    unique = u // 5 if some_groups else 0
    tab = ties_column(R, u, lo, hi, shift, rnd, unique)
    if some_groups:                                                         # half the window values carry a tie group, half hold one value
        keys = Counter(key_of(v, shift) for v in tab)
        assert unique >= 1 and sum(1 for c in keys.values() if c == 1) == unique and sum(1 for c in keys.values() if c > 1) == unique
    for _ in range(64):                                                     # (a draw of u values shows both bits among window-tied neighbours almost surely: insist)
        inp = _draw(rnd, tab, u)
        if window(inp)[1] == shift and tie_mask(inp, shift) == (1 << lo) | (1 << hi) and needs_refinement(inp):
            break
    assert_ties(tab, lo, hi, shift)
    assert_ties(inp, lo, hi, shift)
    return inp, tab


def stages(lo, hi):
    return (hi - lo) // 64 + 1


def ties(R, k, bf, ranges=TIE_RANGES, seed=0, some_groups=False):
    """one lookup per (lo, hi, shift)"""
    u = usable(k, bf)
    pairs = [ties_pair(R, u, lo, hi, s, seed + i, some_groups) for i, (lo, hi, s) in enumerate(ranges)]
    return Case(k, bf, [p[0] for p in pairs], [p[1] for p in pairs], list(range(len(pairs))))


def straddle(R, k, bf, lo=7, shift=100, seed=0):
    """distinct windows except ONE tied pair, which sits at positions SORT_TILE - 1 and SORT_TILE of the sorted column, the larger of the two in the earlier row"""
    u = usable(k, bf)
    assert u > SORT_TILE
    rnd = random.Random(seed * 31337 + 5)
    ws = _windows(R, rnd, u - 1, shift)
    clear = ~(1 << lo)
    tab = [(w << shift) | rnd.randrange(1 << shift) for w in ws]
    small = tab[SORT_TILE - 1] & clear
    tab[SORT_TILE - 1] = small
    tab.insert(SORT_TILE, small | (1 << lo))
    pair = (small | (1 << lo), small)

    def place(col):
        a, b = col.index(pair[0]), col.index(pair[1])
        if a > b:
            col[a], col[b] = col[b], col[a]
        return col
    cols = []
    for _ in range(2):
        col = list(tab)
        rnd.shuffle(col)
        cols.append(place(col))
    for col in cols:
        order = sorted(col)
        assert len(col) == u and (order[SORT_TILE - 1], order[SORT_TILE]) == (pair[1], pair[0]) and col.index(pair[0]) < col.index(pair[1])
        assert tie_mask(col, shift) == 1 << lo and needs_refinement(col) and window(col)[1] == shift
        assert len(set(key_of(v, shift) for v in col)) == u - 1
    return Case(k, bf, [cols[0]], [cols[1]], [0])


# ---- multiset shapes -------------------------------------------------------------------------------------------------------------------------------------------
def multiset(R, k, bf, kind, seed=0):
    u = usable(k, bf)
    rnd = random.Random(seed * 2741 + MULTISET_KINDS.index(kind))
    n_rep = lambda inp: u - len(set(inp))
    if kind == "zeros":                                                     # a lookup whose selector is off
        inp, tab = [0] * u, [0] * u
    elif kind == "const_table":
        v = rnd.randrange(R)
        inp, tab = [v] * u, [v] * u
    elif kind in ("two_runs_larger", "two_runs_smaller"):
        a, b = sorted(_distinct(R, rnd, 2))
        h = max(1, u // 3)
        tab = [a] * h + [b] * (u - h) if u > 1 else [b if kind == "two_runs_larger" else a]
        inp = [b if kind == "two_runs_larger" else a] * u
        assert set(inp) < set(tab) or u == 1
    elif kind == "perm_dups":
        base = [rnd.randrange(R) for _ in range(max(1, u // 4))]
        tab = [base[rnd.randrange(len(base))] for _ in range(u)]
        inp = list(tab)
        rnd.shuffle(inp)
        assert sorted(inp) == sorted(tab) and (len(set(tab)) < u or u == 1)
    elif kind == "same_buffer":
        base = [rnd.randrange(R) for _ in range(max(1, u // 2))]
        tab = [base[rnd.randrange(len(base))] for _ in range(u)]
        inp = tab                                                           # the same list: the same device buffer
    elif kind == "all_distinct":
        tab = _distinct(R, rnd, u)
        inp = list(tab)
        rnd.shuffle(inp)
        assert n_rep(inp) == 0
    elif kind == "one_distinct":
        tab = _distinct(R, rnd, u)
        inp = [tab[u // 2]] * u
        assert n_rep(inp) == u - 1
    elif kind in ("rep_min", "rep_max"):
        e = 0 if kind == "rep_min" else R - 1
        m = max(1, u // 3)
        tab = [e] * m + [rnd.randrange(1, R - 1) for _ in range(u - m)]
        rnd.shuffle(tab)
        inp = _draw(rnd, tab, u, must=[e] * (u // 2 + 1))
        assert (min(tab) if kind == "rep_min" else max(tab)) == e and tab.count(e) == m and inp.count(e) > u // 2
    else:
        raise ValueError(kind)
    assert len(inp) == u and len(tab) == u
    return Case(k, bf, [inp], [tab], [0])


# ---- values the table does not hold ------------------------------------------------------------------------------------------------------------------------------
def not_in_table(R, k, bf, kind, seed=0):
    """every case is refused; good_twin() of it is accepted"""
    u = usable(k, bf)
    rnd = random.Random(seed * 6151 + NOT_IN_TABLE_KINDS.index(kind))
    if kind == "between_window_ties":
        # table values W | 0, W | 2, W | 4 .. tie on the window at shift 190; W | 1 lies strictly between two of them, ties with them on the window and is absent:
        # only a comparison of all 256 bits refuses it
        shift = 190
        w = _windows(R, rnd, 1, shift)[0] << shift
        tab = [w | (2 * rnd.randrange(1 << 20)) for _ in range(u - 2)] + [w, w | 2]
        rnd.shuffle(tab)
        inp = _draw(rnd, tab, u)
        bad = w | 1
        assert window(tab)[1] == shift and bad not in tab and min(tab) < bad < max(tab) and all(key_of(v, shift) == key_of(bad, shift) for v in tab)
        inp[rnd.randrange(u)] = bad
        return Case(k, bf, [inp], [tab], [0])
    tab = [rnd.randrange(1 << 100, R - (1 << 100)) for _ in range(u)]
    inp = _draw(rnd, tab, u)
    if kind == "below_min":
        bad = min(tab) - 1
        assert bad < min(tab)
    elif kind == "above_max":                                               # the lower bound runs off the end of the table
        bad = max(tab) + 1
        assert max(tab) < bad < R
    elif kind == "other_table":
        tab2 = [rnd.randrange(R) for _ in range(u)]
        bad = tab2[0]
        assert bad not in tab
        inp2 = _draw(rnd, tab2, u, must=(bad,))
        inp[rnd.randrange(u)] = bad
        return Case(k, bf, [inp, inp2], [tab, tab2], [0, 1])
    else:
        raise ValueError(kind)
    inp[rnd.randrange(u)] = bad
    return Case(k, bf, [inp], [tab], [0])


def good_twin(case):
    """the same tables with inputs the tables hold"""
    u = usable(case.k, case.bf)
    rnd = random.Random(99)
    return Case(case.k, case.bf, [_draw(rnd, case.tables[t], u) for t in case.tabidx], case.tables, case.tabidx)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------------------------
def mixed_column(R, u, rnd, parts=None):
    """by turns: values just below r (they tie on the window at shift 190 and differ in their low 16 bits), uniform values, narrow values (they all tie: their
    window is 0) and one group that ties high up and differs in bits 0 and 1.  parts, if given, receives the four lists."""
    w = _windows(R, rnd, 1, 190)[0] << 190
    sorts = ([], [], [], [])
    for i in range(u):
        sorts[i % 4].append((R - 1 - rnd.randrange(1 << 16), rnd.randrange(R), rnd.randrange(1 << 16), w | rnd.randrange(4))[i % 4])
    sorts[0][0] = R - 1
    if parts is not None:
        parts.extend(sorts)
    vals = [v for part in sorts for v in part]
    rnd.shuffle(vals)
    return vals


def sized(R, k, bf, seed=0):
    u = usable(k, bf)
    assert u >= 1 and ((k, bf) not in TILE_U or TILE_U[(k, bf)] == u)
    rnd = random.Random(seed * 127 + 1000 * k + bf)
    tab = mixed_column(R, u, rnd)
    inp = _draw(rnd, tab, u, must=(R - 1,))
    assert window(tab)[1] == 190 and window(inp)[1] == 190 and (u < 16 or needs_refinement(tab))
    return Case(k, bf, [inp], [tab], [0])


# ---- batch shapes ----------------------------------------------------------------------------------------------------------------------------------------------
def shared_table_batch(R, k, bf, lookups, tables=1, seed=0):
    """`lookups` lookups over `tables` distinct tables, each shared by several of them (the sgx circuit: 11 lookups, one table); the inputs are by turns tied on
    the window, narrow and wide, all drawn from a table that holds the three sorts of value"""
    u = usable(k, bf)
    rnd = random.Random(seed * 911 + lookups)
    parts = [[] for _ in range(tables)]
    tabs = [mixed_column(R, u, rnd, parts[t]) for t in range(tables)]
    ins, idx = [], []
    for l in range(lookups):
        t = l % tables
        sort_of = l // tables % 3
        top, _, narrow, group = parts[t]
        inp = _draw(rnd, (top + group, narrow, tabs[t])[sort_of], u)       # tied on the window at shift 190 / narrow / everything
        if sort_of == 0:
            assert window(inp)[1] > 0 and (needs_refinement(inp) or u < 16)
        if sort_of == 1:
            assert window(inp)[1] == 0
        ins.append(inp)
        idx.append(t)
    return Case(k, bf, ins, tabs, idx)


# ---- the sequence of the hint test -------------------------------------------------------------------------------------------------------------------------------
def low_order_ok(vals, shift, top):
    """a stable sort over bits [0, top] and then over the window orders the column"""
    order = sorted(sorted(vals, key=lambda v: v & ((1 << (top + 1)) - 1)), key=lambda v: key_of(v, shift))
    return order == sorted(vals)


def hinted_cover(hint, shift):
    """the highest bit a hinted column's low stage orders: the hinted range is [0, min(shift - 1, hint + 15)] (hint = the highest differing bit seen, as bit + 1),
    and a stage runs WHOLE 8-bit passes over it, so the bits up to the end of the range's last digit are ordered too"""
    top = min(shift - 1, hint + 15)
    return 8 * (top // 8 + 1) - 1


def _needs_bit(case, shift, hi):
    """both columns come out of order from a low stage that stops below bit hi, and in order from one that reaches it"""
    for col in case.inputs + case.tables:
        assert low_order_ok(col, shift, hi) and not low_order_ok(col, shift, hi - 1), hi


def _untied(R, k, bf, shift, rnd):
    u = usable(k, bf)
    wt = [(w << shift) | rnd.randrange(1 << shift) for w in _windows(R, rnd, u, shift)]
    rnd.shuffle(wt)
    case = Case(k, bf, [_draw(rnd, wt, u)], [wt], [0])
    assert all(window(c)[1] == shift and not needs_refinement(c) for c in case.inputs + case.tables)
    return case


def hint_steps(R, k, bf, shift=120, seed=0):
    """[(name, case, refined columns, hinted columns)] for ONE context that has never seen the shape (one lookup, two sorted columns, k).  After a refinement the
    context remembers hint = 1 + the highest differing bit; a hinted column is sorted over hinted_cover() and then over its window, and refined again (the hint
    grows) only where its ties differ above that.  After ties at (0, 3) the hint is 4, the hinted range [0, 19]: three passes, which order bits 0 .. 23.  So ties at
    hi = 19 (= hint + 15) AND at hi = 20 .. 23 are hinted only; hi = 24 is the first that is refined again.  (hint_steps_digit_edge: a hint whose range ends on a
    digit, where hint + 15 itself is the last bit covered.)"""
    u = usable(k, bf)
    rnd = random.Random(seed + 17)
    one = lambda lo, hi, s: Case(k, bf, *[[c] for c in ties_pair(R, u, lo, hi, shift, seed + s)], [0])
    first = one(0, 3, 1)
    at = {hi: one(0, hi, hi) for hi in (19, 20, 23, 24)}
    _needs_bit(first, shift, 3)
    for hi, case in at.items():
        _needs_bit(case, shift, hi)
    assert hinted_cover(4, shift) == 23 and hinted_cover(25, shift) == 47
    narrow = Case(k, bf, *[[c] for c in bit_length_pair(R, u, 64, seed + 4)], [0])
    assert all(window(c)[1] == 0 for c in narrow.inputs + narrow.tables)
    wide = _untied(R, k, bf, shift, rnd)
    return [("1. ties at (0, 3): refined", first, 2, 0),
            ("2. the same values: hinted", first, 0, 2),
            ("3. ties at hi = 19 = hint + 15: hinted only", at[19], 0, 2),
            ("4. ties at hi = 20: hinted only (bit 20 lies in the last digit of the range [0, 19])", at[20], 0, 2),
            ("4a. ties at hi = 23, the last bit of that digit: hinted only", at[23], 0, 2),
            ("4b. ties at hi = 24: hinted and refined again, the hint grows to 25", at[24], 2, 2),
            ("5. keys of 64 bits: plain sort", narrow, 0, 0),
            ("6. wide keys without ties: the hint stays", wide, 0, 2),
            ("7. ties at (0, 3) again: hinted", first, 0, 2),
            ("8. ties at hi = 47, the last bit the grown hint covers: hinted only", one(0, 47, 47), 0, 2)]


def hint_steps_digit_edge(R, k, bf, shift=120, seed=0):
    """ties at (0, 0) leave hint = 1: the range [0, 16] needs three passes, [0, 15] would need two.  Bit 16 = hint + 15 is the last bit of the range and the FIRST
    of its digit: a range one bit short drops that pass, and the column has to be refined"""
    u = usable(k, bf)
    one = lambda lo, hi, s: Case(k, bf, *[[c] for c in ties_pair(R, u, lo, hi, shift, seed + s)], [0])
    first, at16, at24 = one(0, 0, 31), one(0, 16, 32), one(0, 24, 33)
    _needs_bit(first, shift, 0)
    _needs_bit(at16, shift, 16)
    _needs_bit(at24, shift, 24)
    assert hinted_cover(1, shift) == 23 and min(shift - 1, 1 + 15) == 16 and 8 * (15 // 8 + 1) - 1 == 15
    return [("ties at (0, 0): refined", first, 2, 0),
            ("ties at hi = 16 = hint + 15: hinted only", at16, 0, 2),
            ("ties at hi = 24: hinted and refined again", at24, 2, 2)]


def swap_steps(R, k, bf, shift=120, seed=0):
    """two lookups with tables of their own; the tied one and a never-tied one change places between two calls"""
    u = usable(k, bf)
    rnd = random.Random(seed + 23)
    tin, ttab = ties_pair(R, u, 2, 9, shift, seed + 5)
    wide = _untied(R, k, bf, shift, rnd)
    win, wt = wide.inputs[0], wide.tables[0]
    return [("tied first", Case(k, bf, [tin, win], [ttab, wt], [0, 1]), 2, 0),
            ("places changed: the hinted columns hold no ties, the others tie for the first time", Case(k, bf, [win, tin], [wt, ttab], [0, 1]), 2, 2)]


# ---- references and checks -------------------------------------------------------------------------------------------------------------------------------------
def _pad(R, rnd, vals, n):
    return vals + [rnd.randrange(R) for _ in range(n - len(vals))]


def prepare(orc, pyref, case, seed=0):
    """columns of a case as (n, 4) Montgomery forms (the rows past u hold values that must not matter), blinding rows, and the expected columns of every lookup.
    Raises ValueError where the case holds a value its table does not, from BOTH references."""
    R, n, u, nb = pyref.R, 1 << case.k, usable(case.k, case.bf), case.bf + 1
    rnd = random.Random(seed + 4242)
    M = orc.fr_from_ints
    assert all(len(c) == u for c in case.inputs + case.tables) and len(case.tabidx) == len(case.inputs)
    cols = {}
    for c in case.inputs + case.tables:
        if id(c) not in cols:
            cols[id(c)] = M(_pad(R, rnd, list(c), n))
    count = len(case.inputs)
    bi = np.stack([pc.rand_fr(orc, pyref, nb, seed + 10 + l) for l in range(count)])
    bt = np.stack([pc.rand_fr(orc, pyref, nb, seed + 1000 + l) for l in range(count)])
    wants, errors = [], 0
    for l in range(count):
        inp, tab = case.inputs[l], case.tables[case.tabidx[l]]
        try:
            pin, ptab = rule(inp, tab, u)
        except ValueError:
            pin = None
        try:
            oi, ot = orc.lookup_permute(cols[id(inp)], cols[id(tab)], case.k, case.bf, bi[l], bt[l])
        except ValueError:
            assert pin is None, "the oracle refuses what the rule accepts"
            errors += 1
            wants.append(None)
            continue
        assert pin is not None, "the rule refuses what the oracle accepts"
        assert (oi[:u] == M(pin)).all() and (ot[:u] == M(ptab)).all(), ("oracle != rule", l)
        assert (oi[u:] == bi[l]).all() and (ot[u:] == bt[l]).all(), ("blinding rows", l)       # verbatim
        wants.append((oi, ot))
    if errors:
        raise ValueError("ConstraintSystemFailure in %d lookup(s)" % errors)
    return cols, bi, bt, wants


def run(be, orc, pyref, case, seed=0, entries=("single", "batch"), prepared=None):
    """the case through permute_expression_pair (one lookup) and / or permute_expression_pairs, all n x 4 limbs of both columns against the references"""
    n, u = 1 << case.k, usable(case.k, case.bf)
    cols, bi, bt, wants = prepared or prepare(orc, pyref, case, seed)
    cols = {id(c): cols[id(c)] for c in case.inputs + case.tables}       # (a prepared superset: only what this case reads goes up)
    dev = {key: be.to_device(arr) for key, arr in cols.items()}
    ins = [dev[id(c)] for c in case.inputs]
    tabs = [dev[id(case.tables[t])] for t in case.tabidx]
    try:
        for entry in entries:
            if entry == "single":
                if len(ins) != 1:
                    continue
                outs = [z.permutation.permute_expression_pair(ins[0], tabs[0], case.k, case.bf, bi[0], bt[0], backend=be)]
            else:
                outs = z.permutation.permute_expression_pairs(ins, tabs, case.k, case.bf, bi, bt, backend=be)
            try:
                for l, ((oa, ot), (wi, wt)) in enumerate(zip(outs, wants)):
                    ga, gt = oa.download((n, 4)), ot.download((n, 4))
                    assert (ga == wi).all() and (gt == wt).all(), (entry, "lookup", l, "first bad row", int(np.argmax((ga != wi).any(1) | (gt != wt).any(1))))
                    assert (ga[u:] == bi[l]).all() and (gt[u:] == bt[l]).all(), (entry, "blinding rows", l)
            finally:
                for pair in outs:
                    for d in pair:
                        d.free()
            for key, arr in cols.items():                                    # the call leaves its inputs alone
                assert (dev[key].download((n, 4)) == arr).all(), entry
    finally:
        for d in dev.values():
            d.free()


def run_refused(be, orc, pyref, case, seed=0):
    """a case with a missing value: ValueError from the references, ZkError from the product on both entries; then the good twin on the same context"""
    import pytest
    with pytest.raises(ValueError):
        prepare(orc, pyref, case, seed)
    R, n = pyref.R, 1 << case.k
    rnd = random.Random(seed + 4242)
    M = orc.fr_from_ints
    cols = {}
    for c in case.inputs + case.tables:
        if id(c) not in cols:
            cols[id(c)] = be.to_device(M(_pad(R, rnd, list(c), n)))
    count = len(case.inputs)
    b = np.stack([pc.rand_fr(orc, pyref, case.bf + 1, seed + l) for l in range(count)])
    ins, tabs = [cols[id(c)] for c in case.inputs], [cols[id(case.tables[t])] for t in case.tabidx]
    try:
        if count == 1:
            with pytest.raises(z.ZkError):
                z.permutation.permute_expression_pair(ins[0], tabs[0], case.k, case.bf, b[0], b[0], backend=be)
        with pytest.raises(z.ZkError):
            z.permutation.permute_expression_pairs(ins, tabs, case.k, case.bf, b, b, backend=be)
    finally:
        for d in cols.values():
            d.free()
    run(be, orc, pyref, good_twin(case), seed + 1)
