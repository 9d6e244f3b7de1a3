"""Scalar cases shared by the emulator tests (CPU, small) and the GPU tests (through the product C ABI): STRUCTURED scalar columns, chosen per window width c so that
the signed-digit recoders of msm.hip (for_each_digit, for_each_digit_static, for_each_digit16, for_each_digit16_static) and the bucket reduction meet, on every row,
what a uniform scalar meets with probability 2^-c per window: the digit 2^(c-1) (the last positive one: bucket B - 1, alone in the last row of the weight matrix and in
the class the host's fold starts from), 2^(c-1) + 1 (the first negative one), 2^c (magnitude 0 that still carries), carry chains through every window into the top one,
and every bucket weight with content of its own.  The tables are arithmetic progressions of generic points [k_i] G with KNOWN k_i, so that every bucket holds
something different, and the `all_equal` / `few` tables of point_cases.  Expected values are those of point_cases.expected: the closed form [sum s_i k_i mod r] G by
one g1_mul AND the oracle's best_multiexp (unsigned windows), all 12 limbs, bit for bit.

signed_digits below is a plain-Python recoder.  It is used ONLY to assert that the inputs have the property they are named after; it is never an expected result."""
import random

import numpy as np

import parity_cases as pc
import point_cases as ptc
import zk_dcap_verifier_amd as z

SCALAR_KINDS = ("half_digits", "half_plus_one", "all_ones", "carry_to_top", "edge_digit_each_window", "bucket_sweep", "top_bucket_heavy", "mixed_edges")
ALL_C = tuple(range(3, 23))


def windows(c):
    return 254 // c + 1


def signed_digits(v, c):
    """the digits d_j in [-(2^(c-1) - 1), 2^(c-1)] of 0 <= v < r, sum_j d_j 2^(c j) = v, lowest window first (input checks only)"""
    W, half, out, carry = windows(c), 1 << (c - 1), [], 0
    for j in range(W):
        d = ((v >> (c * j)) & ((1 << c) - 1)) + carry
        carry = 1 if d > half else 0
        out.append(d - (carry << c))
    assert carry == 0 and v >> (c * W) == 0 and sum(d << (c * j) for j, d in enumerate(out)) == v, (v, c)
    return out


# ---- the values of every kind, as integers ---------------------------------------------------------------------------------------------------------------------
def half_digits_values(R, c):
    """sum_{j < m} 2^(c-1) 2^(c j), m = 1 .. W - 1: every digit is exactly half = 2^(c-1), positive, no carry: every pair lands in bucket B - 1"""
    W, half = windows(c), 1 << (c - 1)
    vals = [sum(half << (c * j) for j in range(m)) for m in range(1, W)]
    assert vals and vals[-1] < R <= sum(half << (c * j) for j in range(W)), c          # (m = W - 1 is the longest that is a scalar)
    for m, v in enumerate(vals, 1):
        assert signed_digits(v, c) == [half] * m + [0] * (W - m), (c, m)
    return vals


def half_plus_one_values(R, c):
    """the same with the digit half + 1: window 0 goes negative with magnitude half - 1 and carries, the next windows see half + 2 (magnitude half - 2, carry), and a
    +1 lands in the window after the last"""
    W, half = windows(c), 1 << (c - 1)
    vals = [sum((half + 1) << (c * j) for j in range(m)) for m in range(1, W)]
    assert vals and vals[-1] < R, c
    for m, v in enumerate(vals, 1):
        assert signed_digits(v, c) == [-(half - 1)] + [-(half - 2)] * (m - 1) + [1] + [0] * (W - m - 1), (c, m)
    return vals


def all_ones_values(R, c):
    """2^m - 1 for m on, one below and one above every multiple of c, up to 253.  From m = c on the first digit is -1, windows 1 .. m / c - 1 see 2^c (magnitude 0,
    nothing emitted, the carry goes on) and +2^(m mod c) lands where the run of ones ends; at m = k c + c - 1 that is the digit half reached THROUGH a carry"""
    W, half = windows(c), 1 << (c - 1)
    ms = sorted({m for k in range(1, 254 // c + 2) for m in (k * c - 1, k * c, k * c + 1) if 1 <= m <= 253})
    vals = [(1 << m) - 1 for m in ms]
    assert vals[-1] < R
    silent = through_carry = 0
    for m, v in zip(ms, vals):
        d = signed_digits(v, c)
        if m >= c:
            assert d == [-1] + [0] * (m // c - 1) + [1 << (m % c)] + [0] * (W - 1 - m // c), (c, m)
            silent += m // c - 1
            through_carry += d[m // c] == half
        else:
            assert d == [v] + [0] * (W - 1) and v == half - 1, (c, m)
    assert silent > 0 and through_carry > 0, c
    return vals


def carry_to_top_values(R, c):
    """((t - 1) << c (W-1)) | (2^(c (W-1)) - 1) with t the top digit of r - 1: -1, then W - 2 silent carries, then t in the top window; r - 1, r - 2, .. and
    (t << c (W-1)) + small: the largest top digits a scalar can have"""
    W, half = windows(c), 1 << (c - 1)
    sh = c * (W - 1)
    t = (R - 1) >> sh
    assert 1 <= t < half, c                                            # (the top window holds fewer than c - 1 bits of r: its digit never goes negative)
    v = ((t - 1) << sh) | ((1 << sh) - 1)
    assert v < R and signed_digits(v, c) == [-1] + [0] * (W - 2) + [t], c
    vals = [v] + [R - 1 - i for i in range(8)] + [(t << sh) + i for i in range(8)]
    assert all(0 < x < R for x in vals)
    for x in vals[1:]:
        assert signed_digits(x, c)[-1] in (t, t + 1) and t + 1 <= half, (c, x)
    return vals


def edge_digit_values(R, c):
    """d 2^(c j) for every window j and d in {1, half - 1, half, half + 1, 2^c - 1}, those below r (in the top window: the ones that fit)"""
    W, half = windows(c), 1 << (c - 1)
    vals = []
    for j in range(W):
        here = [d << (c * j) for d in sorted({1, half - 1, half, half + 1, (1 << c) - 1}) if (d << (c * j)) < R]
        assert here and here[0] == 1 << (c * j) and (len(here) == 5 or j == W - 1), (c, j)   # every window below the top takes all five
        vals += here
    for v in vals:
        d = signed_digits(v, c)
        assert 1 <= sum(1 for x in d if x) <= 2, (c, v)               # the digit itself, and the carry of a negative one
    return vals


def bucket_sweep_values(R, c, seed=0, full=None, limit=None):
    """every bucket weight with a scalar of its own.
    full (default for c <= 13): 0 .. 2^c - 1 in window 0 — every weight once positive, and once negative with a carry digit 1 in window 1 — and again in a middle window.
    otherwise (c >= 14): every w = hi 2^L + lo, L = ceil((c-1)/2), over all hi (the rows of the weight matrix) with one seeded lo each, over all lo (its columns) with
    one seeded hi each, and w in {1, 2^L - 1, 2^L, 2^L + 1, B - 1, B}; the row sweep in window 0, the column sweep in a middle window.
    limit: cut to at most about that many values (the emulator), keeping both ends and the edges"""
    W, B, rnd = windows(c), 1 << (c - 1), random.Random(seed * 50021 + c)
    L = c // 2                                                         # ceil((c - 1) / 2)
    n_lo, n_hi, mid = 1 << L, (B >> L) + 1, W // 2
    assert 0 < mid < W - 1
    edges = sorted({1, n_lo - 1, n_lo, n_lo + 1, B - 1, B} - {0})
    if full is None:
        full = c <= 13
    if full:
        ds = list(range(1 << c))
        if limit and len(ds) > limit // 2:
            keep = set(edges) | {(1 << c) - w for w in edges} | {0, B + 1, (1 << c) - 1}
            ds = sorted(keep | set(rnd.sample(ds, max(0, limit // 2 - len(keep)))))
        elif c <= 13:
            mags = sorted(abs(signed_digits(d, c)[0]) for d in ds)
            assert mags == sorted([0] + list(range(1, B + 1)) + list(range(1, B))), c      # every weight once positive, every weight below B once negative
        for d in (B, B + 1, (1 << c) - 1):
            assert signed_digits(d, c)[:2] == ([B, 0] if d == B else [d - (1 << c), 1]), (c, d)
        vals = ds + ([d << (c * mid) for d in ds] if c <= 13 else [])       # (asked for at c >= 14, the full sweep is 2^c rows: window 0 only)
    else:
        his, los = list(range(n_hi)), list(range(n_lo))
        if limit and n_hi + n_lo > limit:
            his = sorted({0, 1, n_hi - 2, n_hi - 1} | set(rnd.sample(his, limit // 3)))
            los = sorted({0, 1, n_lo - 2, n_lo - 1} | set(rnd.sample(los, limit // 2)))
        rows = [(hi << L) | (rnd.randrange(1 if hi == 0 else 0, n_lo) if hi < n_hi - 1 else 0) for hi in his]
        cols = [(rnd.randrange(1 if lo == 0 else 0, n_hi - 1) << L) | lo for lo in los]
        assert all(1 <= w <= B for w in rows + cols + edges), c
        assert [w >> L for w in rows] == his and [w & (n_lo - 1) for w in cols] == los and rows[-1] == B
        vals = rows + edges + [w << (c * mid) for w in cols + edges]
        for w, v in zip(rows + edges + cols + edges, vals):
            assert sorted(signed_digits(v, c), key=abs)[-1] == w and sum(1 for x in signed_digits(v, c) if x) == 1, (c, w)
    assert all(v < R for v in vals) and any(vals)
    return vals


def top_bucket_value(R, c):
    """the longest of half_digits: W - 1 digits, all of them half"""
    return half_digits_values(R, c)[-1]


def kind_values(pyref, kind, c, seed=0, limit=None, full=None):
    R = pyref.R
    if kind == "half_digits":
        return half_digits_values(R, c)
    if kind == "half_plus_one":
        return half_plus_one_values(R, c)
    if kind == "all_ones":
        return all_ones_values(R, c)
    if kind == "carry_to_top":
        return carry_to_top_values(R, c)
    if kind == "edge_digit_each_window":
        return edge_digit_values(R, c)
    if kind == "bucket_sweep":
        return bucket_sweep_values(R, c, seed, full, limit)
    if kind == "top_bucket_heavy":
        return [top_bucket_value(R, c)]
    raise ValueError(kind)


def scalar_column(orc, pyref, n, kind, c, seed=0, limit=None, full=None):
    """an (m, 4) column of Montgomery forms of one of SCALAR_KINDS for window width c.  The values of the kind are repeated in order up to n rows; m = n except
    where the kind has more than n values (m = their number: nothing is dropped) and for bucket_sweep (m = the number of values, cut only by `limit`).
    mixed_edges: every third row takes the values of all the other kinds in turn (bucket_sweep cut to 48), the rows between are uniform scalars and zeros."""
    R, rnd = pyref.R, random.Random(seed * 9973 + 11 * c)
    if kind == "mixed_edges":
        lists = [kind_values(pyref, k, c, seed, limit=48) for k in SCALAR_KINDS[:-1]]
        for vs in lists:
            rnd.shuffle(vs)
        special = [vs[i] for i in range(max(map(len, lists))) for vs in lists if i < len(vs)]      # round robin: every kind is there from the first rows on
        assert n >= 3 * len(lists)
        sc = pc.rand_fr(orc, pyref, n, seed + 17)
        k3 = (n + 2) // 3
        sc[0::3] = orc.fr_from_ints([special[i % len(special)] for i in range(k3)])
        sc[2::6] = 0
        vals = orc.fr_to_ints(sc)
        assert vals[0::3] == [special[i % len(special)] for i in range(k3)] and all(v < R for v in vals) and not any(vals[2::6]) and any(vals[1::3])
        return np.ascontiguousarray(sc)
    vals = kind_values(pyref, kind, c, seed, limit, full)
    if kind != "bucket_sweep" and len(vals) < n:
        vals = [vals[i % len(vals)] for i in range(n)]
    assert any(vals) and all(0 <= v < R for v in vals), (kind, c)
    sc = orc.fr_from_ints(vals)
    assert orc.fr_to_ints(sc) == vals
    return np.ascontiguousarray(sc)


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------------
def arith_bases(orc, pyref, n, seed=0):
    """(table, ks): [(a0 + i d)] G, generic and all different, with the integers k_i as point_cases.structured_bases returns them"""
    R, rnd = pyref.R, random.Random(seed * 65537 + 19)
    a0, d = rnd.randrange(1, R), rnd.randrange(1, R)
    return orc.gen_bases_arith(a0, d, n), [(a0 + i * d) % R for i in range(n)]


def bases(orc, pyref, n, bkind, seed=0):
    return arith_bases(orc, pyref, n, seed) if bkind == "arith" else ptc.structured_bases(orc, pyref, n, bkind, seed)


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_on_handle(be, orc, pyref, h, table, sc, entries=("host", "dev"), what=()):
    """zk_msm / zk_msm_dev of the column sc over the first len(sc) rows of a registered table (table = (bases, ks))"""
    n = sc.shape[0]
    tab, ks = table
    assert n <= tab.shape[0]
    want, _ = ptc.expected(orc, pyref, sc, np.ascontiguousarray(tab[:n]), ks[:n])
    if "host" in entries:
        ptc.assert_point(be.msm(h.handle, sc), want, ("zk_msm", n) + tuple(what))
    if "dev" in entries:
        d = be.to_device(sc)
        try:
            ptc.assert_point(be.msm(h.handle, d, n), want, ("zk_msm_dev", n) + tuple(what))
        finally:
            d.free()


def check_kinds(be, orc, pyref, c, n, plan, bkind="arith", kinds=SCALAR_KINDS, seed=1, limit=None, entries=("host", "dev")):
    """every kind of `kinds` at width c over ONE registration of a table (of the longest column's length: shorter columns run on a prefix of the resident table).
    plan: the tunables of the case next to msm_c; the caller restores them."""
    be.tune(msm_c=c, **plan)
    cols = [(k, scalar_column(orc, pyref, n, k, c, seed + i, limit=limit)) for i, k in enumerate(kinds)]
    rows = max(col.shape[0] for _, col in cols)
    table = bases(orc, pyref, rows, bkind, seed)
    h = z.arithmetic.BasesHandle(be, table[0])
    try:
        for k, col in cols:
            check_on_handle(be, orc, pyref, h, table, col, entries, (bkind, k, c, sorted(plan.items())))
    finally:
        h.release()
    return rows


def check_batch(be, orc, pyref, c, n, kinds, plan, bkind="arith", seed=2, limit=None):
    """zk_msm_batch_dev: ONE batch of columns of different kinds (all cut or repeated to the same n rows) over one table; every column against both references and
    against the single call"""
    be.tune(msm_c=c, **plan)
    cols = []
    for i, k in enumerate(kinds):
        col = scalar_column(orc, pyref, n, k, c, seed + i, limit=limit)
        reps = -(-n // col.shape[0])
        cols.append(np.ascontiguousarray(np.concatenate([col] * reps)[:n]))
        assert cols[-1].any()
    tab, ks = bases(orc, pyref, n, bkind, seed)
    h = z.arithmetic.BasesHandle(be, tab)
    try:
        dcols = [be.to_device(col) for col in cols]
        try:
            got = be.msm_batch(h.handle, dcols, n)
        finally:
            for d in dcols:
                d.free()
        assert got.shape[0] == len(kinds)
        for i, (k, col) in enumerate(zip(kinds, cols)):
            want, _ = ptc.expected(orc, pyref, col, tab, ks)
            ptc.assert_point(got[i], want, ("batch", c, n, bkind, k))
            assert (z.arithmetic.best_multiexp(col, h) == got[i]).all(), ("single != batch", c, bkind, k)
    finally:
        h.release()


def check_prefix(be, orc, pyref, c, n, bkind="arith", seed=4, skind="mixed_edges"):
    """prefixes of a registered table, several MSMs on one registration"""
    be.tune(msm_c=c)
    sc = scalar_column(orc, pyref, n, skind, c, seed + 1)
    table = bases(orc, pyref, sc.shape[0], bkind, seed)
    h = z.arithmetic.BasesHandle(be, table[0])
    try:
        for m in (sc.shape[0], sc.shape[0] - 1, max(1, n // 3), 2, 1):
            check_on_handle(be, orc, pyref, h, table, np.ascontiguousarray(sc[:m]), ("dev",), ("prefix", bkind, skind, c))
    finally:
        h.release()


def check_partials(be, orc, pyref, c, n, bkind="arith", seed=3, skind="mixed_edges"):
    """zk_msm_partial_dev + zk_g1_sum_xyzz and zk_msm_batch_partial_dev + zk_g1_sum_xyzz_batch on a structured column s: s, s + s, s - s, and the batch (s, -s, s, 0)"""
    R = pyref.R
    be.tune(msm_c=c)
    s = scalar_column(orc, pyref, n, skind, c, seed + 1)
    n = s.shape[0]
    tab, ks = bases(orc, pyref, n, bkind, seed)
    neg = orc.fr_sub(np.zeros((n, 4), dtype=np.uint64), s)
    _, total = ptc.expected(orc, pyref, s, tab, ks)
    ptc.expected(orc, pyref, neg, tab, ks)                            # (-s is a structured column of its own: r - v goes through the recoder too)
    mul = lambda m: ptc._g1_12(orc, pyref, orc.g1_mul(orc.g1_generator(), orc.fr_from_ints([m * total % R])[0]))
    ident = np.zeros(12, dtype=np.uint64)
    assert total != 0
    h = z.arithmetic.BasesHandle(be, tab)
    ds, dn, dz = be.to_device(s), be.to_device(neg), be.to_device(np.zeros((n, 4), dtype=np.uint64))
    try:
        p1, pn = be.msm_partial(h.handle, ds, n), be.msm_partial(h.handle, dn, n)
        ptc.assert_point(be.g1_sum_xyzz(np.stack([p1])), mul(1), ("one partial", c, skind))
        ptc.assert_point(be.g1_sum_xyzz(np.stack([pn])), mul(R - 1), ("the negated partial", c, skind))
        ptc.assert_point(be.g1_sum_xyzz(np.stack([p1, p1])), mul(2), ("s + s", c, skind))
        ptc.assert_point(be.g1_sum_xyzz(np.stack([p1, pn])), ident, ("s + (-s)", c, skind))
        bp = be.msm_batch_partial(h.handle, [ds, dn, ds, dz], n)
        for i, want in enumerate((mul(1), mul(R - 1), mul(1), ident)):
            ptc.assert_point(be.g1_sum_xyzz(bp[i:i + 1]), want, ("one batch partial", c, skind, i))
        got = be.g1_sum_xyzz_batch(np.stack([bp, bp]))
        for i, want in enumerate((mul(2), mul(R - 2), mul(2), ident)):
            ptc.assert_point(got[i], want, ("batch partial doubled", c, skind, i))
    finally:
        for d in (ds, dn, dz):
            d.free()
        h.release()


def check_runs(be, orc, pyref, c, n, bkind="arith", seed=5):
    """zk_bases_enable_runs: a constant top_bucket_heavy column (its adjacent differences are zeros and, on the last row, the value whose every digit is half), an
    all_ones column in sorted order (runs of 2^m - 1; the differences are 2^m' - 2^m, recoded with carries) and a constant column with an all_ones tail go through the
    run-length path (msm_runs = 2) next to a mixed_edges column that stays direct; then msm_runs = 0 must give the same answers."""
    R = pyref.R
    be.tune(msm_c=c)
    tab, ks = bases(orc, pyref, n, bkind, seed)
    top = top_bucket_value(R, c)
    ones = all_ones_values(R, c)
    per = -(-n // len(ones))
    cols = [orc.fr_from_ints(col) for col in ([top] * n, sorted(ones * per)[:n], [top] * (n - len(ones)) + ones)]
    cols.append(scalar_column(orc, pyref, n, "mixed_edges", c, seed))
    assert all(col.shape[0] == n for col in cols)
    wants = [ptc.expected(orc, pyref, col, tab, ks)[0] for col in cols]
    h = z.arithmetic.BasesHandle(be, tab).enable_runs()
    be.timing(True)
    be.tune(msm_runs=2)
    try:
        got = z.arithmetic.best_multiexp_batch(cols, h)
        assert be.stat_get("msm_run_columns") >= 3
        for i, want in enumerate(wants):
            ptc.assert_point(got[i], want, ("runs", c, bkind, i))
        for i in (0, 1):
            ptc.assert_point(z.arithmetic.best_multiexp(cols[i], h), wants[i], ("runs, single", c, bkind, i))
        be.tune(msm_runs=0)
        got0 = z.arithmetic.best_multiexp_batch(cols, h)
        assert (got0 == got).all(), ("msm_runs = 0", c, bkind)
    finally:
        be.tune(msm_runs=1)
        be.timing(False)
        h.release()
