"""The NTT matrix of tests/test_ntt_matrix.py: the plan restated, the census of what a case list runs, the cases and their checks.

The product runs ntt_tile_log = 10, ntt_max_radix_log = 8: passes of radix 2^5 .. 2^8.  Every other emulator backend of the suite is tuned down to a 2^6 tile and
radices up to 2^4 (conftest's `emu`, history_cases.EMU_TUNE), so the halved Shoup-pair table of a radix >= 2^7, the Montgomery last step of ntt_tile_stages29, tw_slot
beyond 16 twiddles, tile_at at c_log 2 .. 4 and a final pass with q_log / p_log of 6 .. 8 never ran there.  The cases below leave every ntt_* tunable at the library's
default, on the emulator and on the GPU, and compare bit for bit with oracle.best_fft / oracle.Domain: no tolerance anywhere.

plan() restates csrc/ntt.hip's plan_passes and the geometry ntt_dev_batch derives from it; test_plan_restatement_matches_the_library pins it against the emulator
build's zk_test_ntt_plan.  census() is computed from plan() alone, so what it says a case list reaches is what the library launches."""
import contextlib
from collections import namedtuple

import numpy as np

import parity_cases as pc

DEFAULT_TUNE = dict(ntt_tile_log=10, ntt_max_radix_log=8, ntt_plan=0)      # csrc/ctx.h
HARSH = ("uniform", "minus_one", "top", "half_negated", "geometric")
LARGE = ("uniform", "minus_one")                                            # above 2^16
MAX_LOG = 21                                                                # the largest transform of the matrix

Pass = namedtuple("Pass", "role r c_log limbs29 q_log p_log")              # q_log, p_log: the final pass's output digits (0 elsewhere)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------------------------
def radices(log_n, tune=None):
    """plan_passes: (radix_log[3], passes)"""
    t = dict(DEFAULT_TUNE, **(tune or {}))
    rmax = max(1, min(t["ntt_max_radix_log"], t["ntt_tile_log"]))
    p = min(3, max(1, (log_n + rmax - 1) // rmax))
    if t["ntt_plan"] > 0:
        d = [t["ntt_plan"] // 100 % 10, t["ntt_plan"] // 10 % 10, t["ntt_plan"] % 10]
        if all(d) and sum(d) == log_n and max(d) <= rmax:
            return d, 3
    rl, rem = [0, 0, 0], log_n
    for i in range(p):
        rl[i] = (rem + (p - i) - 1) // (p - i)
        rem -= rl[i]
    return rl, p


def plan(log_n, tune=None):
    """the passes ntt_dev_batch launches for a transform of 2^log_n, in order.  (At log_n = 0 the library copies or scales the one element without a launch; the entry
    (only, 0, 0) stands for that path.)"""
    t = dict(DEFAULT_TUNE, **(tune or {}))
    tl = t["ntt_tile_log"]
    rl, P = radices(log_n, t)
    if max(rl) > tl:
        raise ValueError("radix 2^%d exceeds the LDS tile 2^%d" % (max(rl), tl))       # ZK_ERR_ARG in the library
    out, blk_log = [], log_n
    for p in range(P):
        r, last = rl[p], p == P - 1
        room = max(tl - r, 0)
        if not last:
            out.append(Pass("first" if p == 0 else "mid", r, min(room, blk_log - r), True, 0, 0))
        else:
            q_log, p_log = (rl[0] if P >= 2 else 0), (rl[1] if P == 3 else 0)
            out.append(Pass("only" if P == 1 else "last", r, min(room, q_log), False, q_log, p_log))
        blk_log -= r
    return out


def census(cases):
    """what a case list runs, from plan(): the pass geometries (role, r, c_log) and the last passes' (r, q_log, p_log)"""
    geo, last = set(), set()
    for c in cases:
        for log_n, ntt_plan in transforms(c):
            for p in plan(log_n, dict(ntt_plan=ntt_plan)):
                geo.add((p.role, p.r, p.c_log))
                if p.role == "last":
                    last.add((p.r, p.q_log, p.p_log))
    return dict(geometries=geo, last=last)


def default_census(lo=0, hi=24):
    """the same for plain transforms of 2^lo .. 2^hi under the default plan"""
    return census([Case("A", "plain", k, k, 0, False, False, 1) for k in range(lo, hi + 1)])


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------------
# section: A every size, B forced plans, C fused forms, D cosets, E launch order.  form: which check runs.  k, ek: the sizes (plain and forced: k = ek = log n;
# coset: ek - k = e).  plan: ntt_plan.  inverse: plain transforms under omega^-1.  batch: the *_batch_dev entry point.  col_major: ntt_col_major.
Case = namedtuple("Case", "section form k ek plan inverse batch col_major")

# ntt_plan values (B): 885 at 2^21 is (first,8,2) (mid,8,2), which the default plan has at 2^23 and 2^24 only; 588 and 858 at 2^21 and 488 at 2^20 put a final
# pass of radix 2^8 behind two passes (2^24's); 876 at 2^21 gives the final pass the digits (q_log, p_log) = (8, 7) of 2^22
FORCED = ((21, 885), (21, 588), (21, 858), (20, 488), (21, 876))

# (k, extended_k) of the fused forms: extended_k takes every value 1 .. 16, 17 (for E), 19, 20, 21; extended_k - k takes 0, 1, 2, 3 and 6 wherever it fits.
# (0, 2) and (1, 3) are single passes of radix 2^2 and 2^3 with the zero padding's stages skipped; (14, 16) and (13, 15) a first pass of radix 2^8; (19, 21) the headline.
PAIRS = ((1, 1), (1, 2), (0, 2), (1, 3), (2, 3), (1, 4), (4, 4), (3, 5), (5, 6), (3, 6), (1, 7), (5, 7), (2, 8), (7, 8), (6, 8), (6, 9), (9, 9), (8, 10), (4, 10), (9, 10),
         (10, 11), (8, 11), (10, 12), (6, 12), (12, 12), (10, 13), (12, 13), (12, 14), (8, 14), (14, 14), (13, 15), (12, 15), (14, 16), (10, 16), (16, 16), (15, 16), (15, 17),
         (17, 19), (17, 20), (19, 20), (19, 21), (15, 21))
LAGRANGE_K = tuple(range(1, 17)) + (19,)
DIVIDE = ((3, 4), (9, 11), (5, 8), (8, 12), (4, 9), (10, 16))               # extended_k - k = 1 .. 6
# (k, e): k <= 8 loads on the 32-bit form with two-level powers; k = 9, 10 on 29-bit limbs with two-level powers and ZETA; k >= 11 takes the one table (or not)
COSETS = ((3, 1), (5, 2), (7, 3), (8, 6), (2, 6), (9, 1), (9, 3), (10, 2), (10, 6), (11, 1), (11, 6), (12, 3), (13, 2), (14, 1), (14, 6), (19, 2))
LAUNCH_ORDER_LOGS = (9, 13, 16, 17)


def matrix(max_log=MAX_LOG):
    """every case whose transforms (and oracle columns) stay at or below 2^max_log"""
    cs = []
    for k in range(0, MAX_LOG + 1):
        for inverse in (False, True):
            for batch in (False, True):
                cs.append(Case("A", "plain", k, k, 0, inverse, batch, 1))
    for log_n, p in FORCED:
        cs.append(Case("B", "forced", log_n, log_n, p, False, True, 1))
    for k in LAGRANGE_K:
        for batch in (False, True):
            cs.append(Case("C", "lagrange", k, k, 0, False, batch, 1))
    for k, ek in PAIRS:
        for batch in (False, True):
            cs.append(Case("C", "c2e", k, ek, 0, False, batch, 1))
        cs.append(Case("C", "e2c", k, ek, 0, False, False, 1))
    for k, ek in DIVIDE:
        cs.append(Case("C", "div", k, ek, 0, False, False, 1))
    for k, e in COSETS:
        cs.append(Case("D", "coset", k, k + e, 0, False, True, 1))
    cs += [c._replace(section="E", col_major=0) for c in cs if c.section in "AC" and c.batch and c.ek in LAUNCH_ORDER_LOGS]
    return [c for c in cs if c.ek <= max_log]


def transforms(c):
    """(log n, ntt_plan) of the transforms a case runs"""
    return {"plain": [(c.k, 0)], "forced": [(c.k, c.plan)], "lagrange": [(c.k, 0)], "c2e": [(c.ek, 0)], "e2c": [(c.ek, 0)], "div": [], "coset": [(c.k, 0)]}[c.form]


def case_id(c):
    s = "%s-%s-%d" % (c.section, c.form, c.k) + ("-%d" % c.ek if c.ek != c.k else "")
    return s + ("-plan%d" % c.plan if c.plan else "") + ("-inv" if c.inverse else "") + ("-batch" if c.batch else "") + ("" if c.col_major else "-rowmajor")


# ---- columns and references: computed once, shared, read-only ------------------------------------------------------------------------------------------------------
_MEMO, _MEMO_MAX = {}, 32 << 17                                              # arrays up to 2^17 elements stay (E repeats A and C); larger ones are made per case


def memo(key, make):
    if key in _MEMO:
        return _MEMO[key]
    v = make()
    v.flags.writeable = False
    if v.nbytes <= _MEMO_MAX:
        _MEMO[key] = v
    return v


def col(orc, pyref, log_n, seed, kind):
    return memo(("col", log_n, seed, kind), lambda: pc.column(orc, pyref, 1 << log_n, seed, kind))


def kinds_for(log_n):
    return HARSH if log_n <= 16 else LARGE


def batch_kinds(log_n, shift=0):
    """three columns of different kinds (above 2^16: uniform, minus_one and a second uniform column — col() seeds them apart)"""
    ks = kinds_for(log_n)
    return [ks[(shift + i) % len(ks)] for i in range(3)]


@contextlib.contextmanager
def tuned(be, **kw):
    """move tunables for one check; every one of them is put back whatever the check does"""
    old = {k: be.tune_get(k) for k in kw}
    try:
        be.tune(**kw)
        yield
    finally:
        be.tune(**old)


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "rows differ:", int(bad.size), "first", bad[:4].tolist())


def _omega(orc, pyref, log_n, inverse):
    w = pyref.omega(log_n)
    return orc.fr_from_ints([pow(w, -1, pyref.R) if inverse else w])[0], orc.fr_from_ints([w if inverse else pow(w, -1, pyref.R)])[0]


def _fft(orc, a, key, w, log_n):
    return memo(("fft",) + key, lambda: orc.best_fft(a, w, log_n))


# ---- the checks: each a function of a backend ----------------------------------------------------------------------------------------------------------------------
def check_plain(be, orc, pyref, log_n, inverse=False, batch=False, ntt_plan=0, kinds=None):
    """zk_ntt_dev (one column after the other, in place, each with its round trip as parity_cases.check_ntt) or zk_ntt_batch_dev (three columns of different kinds)"""
    n = 1 << log_n
    w, wback = _omega(orc, pyref, log_n, inverse)
    kinds = list(kinds or (batch_kinds(log_n, shift=log_n) if batch else kinds_for(log_n)))
    cols = [col(orc, pyref, log_n, 400 + i, kd) for i, kd in enumerate(kinds)]
    want = [_fft(orc, a, (log_n, 400 + i, kd, inverse), w, log_n) for i, (a, kd) in enumerate(zip(cols, kinds))]
    with tuned(be, ntt_plan=ntt_plan):
        if batch:
            d = [be.to_device(a) for a in cols]
            try:
                be.ntt_batch_dev(d, log_n, w)
                for i, x in enumerate(d):
                    _same(x.download((n, 4)), want[i], ("ntt_batch_dev", log_n, kinds[i], "inverse" if inverse else "forward", "plan", ntt_plan))
            finally:
                for x in d:
                    x.free()
            return
        nm = orc.fr_from_ints([n % pyref.R])
        for a, kd, wt in zip(cols, kinds, want):
            d = be.to_device(a)
            try:
                be.ntt_dev(d, log_n, w)
                _same(d.download((n, 4)), wt, ("ntt_dev", log_n, kd, "inverse" if inverse else "forward", "plan", ntt_plan))
                be.ntt_dev(d, log_n, wback)                                # the round trip: n * a
                _same(d.download((n, 4)), orc.fr_mul(a, np.repeat(nm, n, axis=0)), ("ntt_dev round trip", log_n, kd))
            finally:
                d.free()


def _domain(orc, k, ek):
    od = orc.Domain((1 << (ek - k)) + 1, k)                                # quotient_poly_degree 2^(ek - k): the whole extended column is the result
    assert (od.k, od.extended_k) == (k, ek)
    return od


def check_lagrange(be, orc, pyref, k, batch=False):
    """zk_lagrange_to_coeff_dev / _batch_dev (the 1/n on the last strided pass's table, or the post-scale of a single pass), then zk_coeff_to_lagrange_dev back"""
    n, od = 1 << k, _domain(orc, k, k)
    kinds = batch_kinds(k, shift=k + 1) if batch else kinds_for(k)
    cols = [col(orc, pyref, k, 500 + i, kd) for i, kd in enumerate(kinds)]
    want = [memo(("l2c", k, 500 + i, kd), lambda a=a: od.lagrange_to_coeff(a)) for i, (a, kd) in enumerate(zip(cols, kinds))]
    d = [be.to_device(a) for a in cols]
    try:
        if batch:
            be.lagrange_to_coeff_batch_dev(d, k)
        else:
            for x in d:
                be.lagrange_to_coeff_dev(x, k)
        for x, wt, kd in zip(d, want, kinds):
            _same(x.download((n, 4)), wt, ("lagrange_to_coeff", k, kd, "batch" if batch else "single"))
        if not batch:
            for x, wt, kd in zip(d, want, kinds):
                be.coeff_to_lagrange_dev(x, k)
                _same(x.download((n, 4)), od.coeff_to_lagrange(wt), ("coeff_to_lagrange", k, kd))
    finally:
        for x in d:
            x.free()


def check_coeff_to_extended(be, orc, pyref, k, ek, batch=False):
    """zk_coeff_to_extended_dev / _batch_dev with ntt_quarter_input 1 and 0: both equal to the oracle (hence to each other)"""
    n, en, od = 1 << k, 1 << ek, _domain(orc, k, ek)
    kinds = batch_kinds(ek, shift=k + ek) if batch else kinds_for(ek)
    cols = [col(orc, pyref, k, 600 + i, kd) for i, kd in enumerate(kinds)]
    want = [memo(("c2e", k, ek, 600 + i, kd), lambda a=a: od.coeff_to_extended(a)) for i, (a, kd) in enumerate(zip(cols, kinds))]
    d = [be.to_device(a) for a in cols]
    outs = [be.alloc(en * 32) for _ in cols]
    try:
        for quarter in (1, 0):
            with tuned(be, ntt_quarter_input=quarter):
                if batch:
                    be.coeff_to_extended_batch_dev(d, outs, k, ek)
                else:
                    for x, o in zip(d, outs):
                        be.coeff_to_extended_dev(x, k, ek, o)
            for o, wt, kd in zip(outs, want, kinds):
                _same(o.download((en, 4)), wt, ("coeff_to_extended", k, ek, kd, "batch" if batch else "single", "quarter_input", quarter))
            for x, a in zip(d, cols):
                assert (x.download((n, 4)) == a).all(), "coeff_to_extended wrote its input"
    finally:
        for x in d + outs:
            x.free()


def check_extended_to_coeff(be, orc, pyref, k, ek):
    """zk_extended_to_coeff_dev with ntt_fuse_scale 1 and 0"""
    en, od = 1 << ek, _domain(orc, k, ek)
    for i, kd in enumerate(kinds_for(ek)):
        a = col(orc, pyref, ek, 700 + i, kd)
        want = memo(("e2c", ek, 700 + i, kd), lambda: np.ascontiguousarray(od.extended_to_coeff(a)))
        assert want.shape[0] == en
        for fuse in (1, 0):
            d = be.to_device(a)
            try:
                with tuned(be, ntt_fuse_scale=fuse):
                    be.extended_to_coeff_dev(d, k, ek)
                _same(d.download((en, 4)), want, ("extended_to_coeff", k, ek, kd, "fuse_scale", fuse))
            finally:
                d.free()


def check_divide(be, orc, pyref, k, ek):
    en, od = 1 << ek, _domain(orc, k, ek)
    for i, kd in enumerate(kinds_for(ek)):
        a = col(orc, pyref, ek, 800 + i, kd)
        d = be.to_device(a)
        try:
            be.divide_by_vanishing_poly_dev(d, k, ek)
            _same(d.download((en, 4)), od.divide_by_vanishing_poly(a), ("divide_by_vanishing_poly", k, ek, kd))
        finally:
            d.free()


def coset_indices(k, e):
    """0, 1, 2^e - 1 and one in the middle; all of them where that is cheap (then fr_interleave_dev rebuilds the extended column)"""
    if e <= 3 and k <= 14 or k + e <= 14:
        return list(range(1 << e))
    return sorted({0, 1, (1 << e) - 1, (1 << (e - 1)) + (5 if e >= 4 else 0)})


def check_cosets(be, orc, pyref, k, e):
    """zk_coeff_to_coset_batch_dev against the ORACLE's coeff_to_extended[j :: 2^e]; above the tile with ntt_coset_table 1 and 0"""
    n, ek, od = 1 << k, k + e, _domain(orc, k, k + e)
    kinds = batch_kinds(k, shift=k + e)
    cols = [col(orc, pyref, k, 900 + i, kd) for i, kd in enumerate(kinds)]
    ext = [memo(("c2e", k, ek, 900 + i, kd), lambda a=a: od.coeff_to_extended(a)) for i, (a, kd) in enumerate(zip(cols, kinds))]
    js = coset_indices(k, e)
    d = [be.to_device(a) for a in cols]
    keep = {}
    try:
        for table in ((1, 0) if k >= 11 else (1,)):
            with tuned(be, ntt_coset_table=table):
                for j in js:
                    outs = [be.alloc(n * 32) for _ in cols]
                    try:
                        be.coeff_to_coset_batch_dev(d, outs, k, ek, j)
                        for o, x, kd in zip(outs, ext, kinds):
                            _same(o.download((n, 4)), x[j::1 << e], ("coeff_to_coset", k, e, "coset", j, kd, "table", table))
                    finally:
                        if table == 1 and len(js) == 1 << e:
                            keep[j] = outs[1]
                            outs = [outs[0], outs[2]]
                        for o in outs:
                            o.free()
        if len(keep) == 1 << e:
            out = be.alloc((n << e) * 32)
            try:
                be.fr_interleave_dev([keep[j] for j in range(1 << e)], n, out)
                _same(out.download((n << e, 4)), ext[1], ("fr_interleave", k, e))
            finally:
                out.free()
    finally:
        for x in d + list(keep.values()):
            x.free()


def run(c, be, orc, pyref):
    with tuned(be, ntt_col_major=c.col_major):
        if c.form in ("plain", "forced"):
            check_plain(be, orc, pyref, c.k, c.inverse, c.batch, c.plan, kinds=LARGE if c.form == "forced" else None)
        elif c.form == "lagrange":
            check_lagrange(be, orc, pyref, c.k, c.batch)
        elif c.form == "c2e":
            check_coeff_to_extended(be, orc, pyref, c.k, c.ek, c.batch)
        elif c.form == "e2c":
            check_extended_to_coeff(be, orc, pyref, c.k, c.ek)
        elif c.form == "div":
            check_divide(be, orc, pyref, c.k, c.ek)
        elif c.form == "coset":
            check_cosets(be, orc, pyref, c.k, c.ek - c.k)
        else:
            raise ValueError(c.form)
