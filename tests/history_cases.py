"""Cases shared by the emulator tests (CPU, small) and the GPU tests (through the product C ABI) of tests/test_context_history.py: the same operation, bit for bit against
the oracle, on a context whose HISTORY was chosen to hurt it.  A zk_ctx keeps grow-only DevBuf workspaces (ws_sorted, ws_mid, ws_sub0/1, ws_cls0/1, ws_tmp, ws_ntt,
ws_quot, ws_quot_state, ws_runs, ws_scalars), up to 16 twiddle sets, the coset tables and the buffers zk_plonk_create_proof keeps between proofs; nearly every other
parity test runs on whatever the session-scoped fixtures happen to have left in them.  Here every case opens its OWN z.Backend (fresh()), so the history is exactly
what the case wrote, and follows one shape (sequence()):

    1. the victim on the fresh context      2. the polluter      3. the victim again      4. the polluter again

each step against the oracle (best_multiexp and the closed form, best_fft, Domain, the check_* helpers of the other case modules — never another run of the code under
test).  The polluter is at least as large as the victim and dense where the victim is sparse: a slot the victim's kernels read without writing then holds a valid point
or field element of the polluter, not the zero a first use finds.  Step 4 catches a victim that leaves state the next call trusts.

No byte pattern is ever written into a workspace: a stale count or offset read from a pattern would index outside every buffer, a real history keeps it inside buffers
that only grow."""
import contextlib
import random

import numpy as np
import pytest

import lookup_cases as lc
import parity_cases as pc
import point_cases as ptc
import program_cases as pg
import proof_cases as prc
import quotient_cases as qc
import scalar_cases as scs
import test_coset as tc
import test_create_proof as tcp
import test_eval_phase as tep
import test_grand_product as tgp
import test_structured_lookups as tsl
import test_structured_values as tsv
import zk_dcap_verifier_amd as z
from conftest import EMU_SO
from zk_dcap_verifier_amd import evaluation as ev
from zk_dcap_verifier_amd import plonk

ZK_ERR_ARG, ZK_ERR_LIMIT = -1, -5
MAX_TWIDDLE_SETS = 16                                                  # csrc/ntt.hip; no statistic reports the resident sets, so the cases count the sets they create

# the tunables of conftest.py's `emu` fixture (test_context_history.test_emulator_tunables_are_the_fixtures pins the copy): every work-item is a pthread there
EMU_TUNE = dict(msm_sort_threads=64, msm_sort_wgs=3, msm_block=32, ntt_threads=32, ntt_tile_log=6, ntt_max_radix_log=4, msm_target_threads=64, msm_min_chunk=2,
                vec_block=32, quot_threads=32)

# per backend: the sizes of every section.  The emulator's are cut to what CPU threads run in seconds; each keeps the paths of the GPU's (several workgroups, a short
# last chunk, two and three NTT passes under the fixture's 2^6 tile) and each polluter stays at least as large as its victim.
SIZES = {
    "emu": dict(msm_n=256, msm_narrow=5, msm_wide=17, msm_wide_n=64, msm_wide_short=True, runs_n=1100, runs_c=8, fanin2_tune={},
                walk=tuple(range(1, 13)), tile=6, radix=4, plans=((4, 2), (5, 5), (8, 3)), retune_log=8, coset_k=7, coset_e=2, ws_big=12, ws_sliced=13, forms_log=8,
                large_k=9, small_k=5, g1_large=6, g1_small=5, quot_big=6, quot_small=3, proof_a=6, proof_b=5, codec_n=77),
    "gpu": dict(msm_n=1 << 13, msm_narrow=8, msm_wide=17, msm_wide_n=1 << 13, msm_wide_short=False, runs_n=1 << 13, runs_c=8,
                fanin2_tune=dict(msm_min_chunk=128, msm_max_chunk=128),        # 2^13 rows x 32 windows in sub-buckets of 16 pairs would need 15 merge levels at fan-in 2; the library has 12
                walk=tuple(range(1, 13)), tile=10, radix=8, plans=((10, 5), (11, 11), (12, 10), (12, 6)), retune_log=14, coset_k=11, coset_e=2, ws_big=12, ws_sliced=13, forms_log=11,
                large_k=12, small_k=5, g1_large=7, g1_small=5, quot_big=8, quot_small=4, proof_a=6, proof_b=5, codec_n=1003),
}


@contextlib.contextmanager
def fresh(which):
    """a context of its own on the emulator ("emu", under the fixture's tunables) or on the product library ("gpu"); closed whatever the case does"""
    be = z.Backend(0, lib_path=EMU_SO) if which == "emu" else z.Backend(0)
    try:
        if which == "emu":
            assert "EMULATED" in be.version()
            be.tune(**EMU_TUNE)
        else:
            assert "gfx950" in be.version() and "EMULATED" not in be.version()
        yield be
    finally:
        be.close()


def sequence(victim, polluter):
    """the shape of every case; `victim` and `polluter` compare with the oracle themselves"""
    victim("1. victim on the fresh context")
    polluter("2. polluter")
    victim("3. victim after the polluter")
    polluter("4. polluter after the victim")


# ---- A. MSM workspaces -------------------------------------------------------------------------------------------------------------------------------------------
MSM_PLANS = (  # a reduced cross: every value of every axis is there, and every case runs its plan both as polluter and as victim
    dict(two_level=0, width="narrow", fanin=8, partial=False),
    dict(two_level=1, width="narrow", fanin=2, partial=False),
    dict(two_level=0, width="narrow", fanin=2, partial=True),
    dict(two_level=1, width="wide", fanin=8, partial=True),
    dict(two_level=1, width="wide", fanin=2, partial=False),
)
msm_plan_id = lambda p: "%s-sort%d-fanin%d-%s" % (p["width"], p["two_level"], p["fanin"], "partial" if p["partial"] else "normalised")


def bucket_census(pyref, orc, col, c):
    """from the INPUTS (scalar_cases.signed_digits, no device): (buckets 1 .. B that receive a pair from EVERY window below the top one, buckets that receive a pair at all,
    windows that emit a pair)"""
    W, B = scs.windows(c), 1 << (c - 1)
    seen = np.zeros((W, B + 1), dtype=bool)
    for v in orc.fr_to_ints(col):
        for j, d in enumerate(scs.signed_digits(v, c)):
            seen[j, abs(d)] = True
    return int(seen[: W - 1, 1:].all(axis=0).sum()), int(seen[:, 1:].any(axis=0).sum()), int(seen[:, 1:].any(axis=1).sum())


def dense_columns(orc, pyref, n, c, count=4, seed=1):
    """`count` uniform columns over n rows, from the first seed for which — c <= 16 — every bucket of every window below the top one receives a scalar in every column
    (the top window holds fewer than c - 1 bits of r: its digits stop at r's top digit).  Wider windows have more buckets than the table has pairs: there the columns
    must reach every window and more buckets than rows, which is what a column can do."""
    W, B = scs.windows(c), 1 << (c - 1)
    if (n, c, count, seed) in _DENSE:
        return _DENSE[n, c, count, seed]
    for s in range(seed, seed + 64):
        cols = [pc.rand_fr(orc, pyref, n, 1000 * s + i) for i in range(count)]
        census = [bucket_census(pyref, orc, col, c) for col in cols]
        if all(full == B for full, _, _ in census) if c <= 16 else all(windows == W and any_ > min(n, B // 2) for _, any_, windows in census):
            _DENSE[n, c, count, seed] = cols
            return cols
    raise AssertionError("no seed fills the buckets: n = %d, c = %d" % (n, c))


_DENSE = {}                                                            # (the census is Python integers: once per shape)


def _only_window(pyref, c, j):
    """scalar_cases.edge_digit_values whose ONLY non-zero signed digit lies in window j"""
    W = scs.windows(c)
    vals = [v for v in scs.edge_digit_values(pyref.R, c) if [i for i, d in enumerate(scs.signed_digits(v, c)) if d] == [j % W]]
    assert vals, (c, j)
    return vals


def sparse_columns(orc, pyref, n, c, seed=3):
    """the victims, by name: zeros; one non-zero scalar at row 0 / at the last row; scalars whose only non-zero digit is in the lowest / in the top window"""
    R, rnd = pyref.R, random.Random(seed)
    rep = lambda vals: [vals[i % len(vals)] for i in range(n)]
    cols = dict(zeros=[0] * n, first=[rnd.randrange(1, R)] + [0] * (n - 1), last=[0] * (n - 1) + [rnd.randrange(1, R)],
                low_window=rep(_only_window(pyref, c, 0)), top_window=rep(_only_window(pyref, c, -1)))
    assert sum(map(bool, cols["first"])) == 1 and sum(map(bool, cols["last"])) == 1 and cols["last"][-1] and not any(cols["zeros"])
    return {k: np.ascontiguousarray(orc.fr_from_ints(v)) for k, v in cols.items()}


class MsmTable:
    """one resident table [k_i] G (scalar_cases.arith_bases) and the two ways a case calls it; every result against point_cases.expected: the closed form
    [sum s_i k_i] G by one g1_mul AND the oracle's best_multiexp, all 12 limbs"""

    def __init__(self, be, orc, pyref, n, c, partial, runs=False, seed=7):
        self.be, self.orc, self.pyref, self.n, self.c, self.partial = be, orc, pyref, n, c, partial
        self.tab, self.ks = scs.arith_bases(orc, pyref, n, seed)
        be.tune(msm_c=c)
        self.h = z.arithmetic.BasesHandle(be, self.tab)
        if runs:
            self.h.enable_runs()
        self._want = {}

    def want(self, col, m):
        key = (col.ctypes.data, m)                                     # (the columns of a case live as long as the case)
        if key not in self._want:
            self._want[key] = ptc.expected(self.orc, self.pyref, np.ascontiguousarray(col[:m]), np.ascontiguousarray(self.tab[:m]), self.ks[:m])[0]
        return self._want[key]

    def check(self, cols, what, m=None, host=False):
        """one call over the first m rows: zk_msm_batch_dev / zk_msm_dev (one column), zk_msm_batch (host), or the partial sums and zk_g1_sum_xyzz"""
        be, m = self.be, self.n if m is None else m
        if host:
            got = be.msm_batch(self.h.handle, [np.ascontiguousarray(col[:m]) for col in cols])
        else:
            d = [be.to_device(np.ascontiguousarray(col[:m])) for col in cols]
            try:
                if self.partial:
                    parts = be.msm_batch_partial(self.h.handle, d, m) if len(d) > 1 else be.msm_partial(self.h.handle, d[0], m).reshape(1, 16)
                    got = np.stack([be.g1_sum_xyzz(parts[i:i + 1]) for i in range(len(d))])
                else:
                    got = be.msm_batch(self.h.handle, d, m) if len(d) > 1 else be.msm(self.h.handle, d[0], m).reshape(1, 12)
            finally:
                for x in d:
                    x.free()
        for i, col in enumerate(cols):
            ptc.assert_point(got[i], self.want(col, m), (what, "column", i, "rows", m, "of", self.n, "c", self.c))

    def release(self):
        self.h.release()


def msm_history(be, orc, pyref, S, plan):
    """the whole of section A for one plan, on one context"""
    wide = plan["width"] == "wide"
    c, n = S["msm_wide" if wide else "msm_narrow"], S["msm_wide_n" if wide else "msm_n"]
    assert (c > 16) == wide
    be.tune(msm_two_level_sort=plan["two_level"], msm_merge_fanin=plan["fanin"])
    if plan["fanin"] == 2:
        be.tune(**S["fanin2_tune"])
    t = MsmTable(be, orc, pyref, n, c, plan["partial"])
    try:
        dense = dense_columns(orc, pyref, n, c)
        sp = sparse_columns(orc, pyref, n, c)
        uni = [pc.rand_fr(orc, pyref, n, 90 + i) for i in range(2)]
        P = lambda what: t.check(dense, what)
        if wide and S["msm_wide_short"]:
            # the emulator walks the 2^16 buckets of every column work-item by work-item (about two seconds per column, whatever the rows): batches of two
            # columns instead of four, one prefix, one column after two, host scalars — under the plan's own sort, fan-in and partial sums
            sequence(lambda what: t.check([sp["last"], sp["zeros"]], what), lambda what: t.check(dense[:2], what))
            t.check([sp["low_window"], sp["first"]], "prefix after the full table", m=17)
            t.check([sp["top_window"]], "one column after two")
            t.check(dense[:1], "dense, one column")
            t.check([sp["first"]], "host scalars after a dense column", host=True)
            return
        # the same table, the same nb = 4: the layout is identical and every slot aliases exactly
        for batch in ([sp["zeros"], sp["first"], sp["last"], sp["low_window"]], [sp["top_window"], sp["zeros"], sp["last"], sp["first"]], [uni[0], sp["zeros"], sp["first"], uni[1]]):
            sequence(lambda what: t.check(batch, what), P)
        # shifted layouts: prefixes of the table ...
        for m in (n // 2 + 1, 17):
            sequence(lambda what: t.check([sp["low_window"], sp["zeros"], sp["last"], uni[0]], what, m=m), P)
        # ... one column after four (each victim alone, then the dense column alone) and four after one
        for name in sorted(sp):
            sequence(lambda what: t.check([sp[name]], (what, name)), P)
        sequence(lambda what: t.check([sp["zeros"], sp["first"], sp["last"], sp["top_window"]], what), lambda what: t.check(dense[:1], what))
        # host scalars: the upload goes through ws_scalars
        sequence(lambda what: t.check([sp["last"]], what, host=True), lambda what: t.check(dense, what, host=True))
    finally:
        t.release()


def runs_history(be, orc, pyref, S, first):
    """ws_runs / ws_scalars: one column through the run-length path (msm_runs = 2) and then direct (msm_runs = 0), or the other way round, with a dense batch between"""
    n, c, R = S["runs_n"], S["runs_c"], pyref.R
    t = MsmTable(be, orc, pyref, n, c, False, runs=True)
    try:
        ones = scs.all_ones_values(R, c)
        col = np.ascontiguousarray(orc.fr_from_ints([scs.top_bucket_value(R, c)] * (n - len(ones)) + ones))      # constant with an all_ones tail (scalar_cases.check_runs)
        dense = dense_columns(orc, pyref, n, c)

        def victim(mode):
            def run(what):
                be.tune(msm_runs=mode)
                be.timing(True)
                try:
                    t.check([col], (what, "msm_runs", mode), host=True)
                    assert (be.stat_get("msm_run_columns") >= 1) == (mode == 2), (what, mode)
                finally:
                    be.timing(False)
            return run
        other = 0 if first == 2 else 2
        sequence(victim(first), victim(other))
        sequence(victim(first), lambda what: t.check(dense, what, host=True))
        sequence(victim(other), lambda what: t.check(dense, what))
    finally:
        be.tune(msm_runs=1)
        t.release()


# ---- B. twiddle sets, coset tables, the NTT workspace -----------------------------------------------------------------------------------------------------------
def _w(orc, pyref, log_n, inverse=False):
    return orc.fr_from_ints([pow(pyref.omega(log_n), -1 if inverse else 1, pyref.R)])[0]


def transform(be, orc, pyref, log_n, inverse=False, seed=0, what=""):
    """zk_ntt of one uniform column against best_fft: creates, or finds, the set (log n, omega^+-1) of the plan in force"""
    a = pc.rand_fr(orc, pyref, 1 << log_n, 100 * log_n + seed + inverse)
    w = _w(orc, pyref, log_n, inverse)
    b = a.copy()
    z.arithmetic.best_fft(b, w, log_n, backend=be)
    assert (b == orc.best_fft(a, w, log_n)).all(), ("zk_ntt", log_n, "inverse" if inverse else "forward", what)


def eviction_walk(be, orc, pyref, S):
    """forward and inverse at every size of the walk: 23 sets (omega_2 = -1 is its own inverse) on a context that keeps 16; then the first size (evicted, rebuilt)
    and the last (still there)"""
    logs = S["walk"]
    assert 2 * len(logs) - 1 > MAX_TWIDDLE_SETS
    for log_n in logs:
        for inverse in (False, True):
            transform(be, orc, pyref, log_n, inverse, what="walk")
    for log_n in (logs[0], logs[-1], logs[0]):
        for inverse in (False, True):
            transform(be, orc, pyref, log_n, inverse, seed=5, what="revisit")


def fill_sets(be, orc, pyref, avoid, count=MAX_TWIDDLE_SETS, first=()):
    """bring exactly `count` sets into residence on a context that holds none of them: `first` (log n, inverse) pairs go in first — the oldest —, then forward and inverse
    transforms of the smallest sizes not in `avoid`"""
    pairs = list(first) + [(log_n, inv) for log_n in range(1, 28) if log_n not in avoid for inv in (False, True) if (log_n, inv) not in first and (log_n, inv) != (1, True)]
    # ((1, True) is no set of its own: the square root of one is its own inverse)
    pairs = pairs[:count]
    assert len(pairs) == count and len(set(pairs)) == count
    for log_n, inv in pairs:
        transform(be, orc, pyref, log_n, inv, what="fill")
    return pairs


def domain_of(orc, k, e):
    for j in range(2, 40):
        od = orc.Domain(j, k)
        if od.extended_k == k + e:
            return od
    raise AssertionError((k, e))


def check_coset(be, orc, pyref, k, e, coset, count=2, seed=0):
    """zk_coeff_to_coset_batch_dev against every 2^e-th entry of the ORACLE's coeff_to_extended"""
    od = domain_of(orc, k, e)
    n = 1 << k
    polys = [pc.rand_fr(orc, pyref, n, seed + 31 * i + coset) for i in range(count)]
    d, outs = [be.to_device(p) for p in polys], [be.alloc(n * 32) for _ in polys]
    try:
        be.coeff_to_coset_batch_dev(d, outs, k, k + e, coset)
        for i, (p, o) in enumerate(zip(polys, outs)):
            assert (o.download((n, 4)) == od.coeff_to_extended(p)[coset::1 << e]).all(), ("coset", coset, "k", k, "extended_k", k + e, "column", i)
            assert (d[i].download((n, 4)) == p).all(), "the call changed its input"
    finally:
        for x in d + outs:
            x.free()


def eviction_under_held_pointers(be, orc, pyref, S, op):
    """16 resident sets, then a caller of ntt_pow_tables that needs sets the context does not hold.
    coset_new_sets / coset_oldest_set_is_held: ONE call (coeff_to_coset) takes the power tables of the extended domain, holds pointers into them, and builds — and
    evicts for — the set of its transform: the only caller that holds a set's tables across the building of another.
    pieces / grand_product / g1_ntt: the helpers of test_coset, test_grand_product and point_cases on a full cache: every set they need is built as a 17th one and
    evicts the least recently used; none of these operations holds pointers into one set while it builds another (cosets_to_pieces finishes its inverse transforms
    before it asks for the extended domain's tables, and its helper's preparation has built them already), so what they show is that sets built under eviction, and
    rebuilt after it, are right"""
    k, e = S["coset_k"], S["coset_e"]
    ek = k + e
    assert k > S["tile"]                                               # (a coset transform of two passes and more: it takes the coset table as well)
    if op == "coset_new_sets":
        fill_sets(be, orc, pyref, avoid=(k, ek))
        check_coset(be, orc, pyref, k, e, 1)
        check_coset(be, orc, pyref, k, e, (1 << e) - 1, seed=3)       # (both sets and the table of coset 1 are resident now)
    elif op == "coset_oldest_set_is_held":
        # the extended domain's set is the OLDEST of the 16 and is found, not built: its stamp must move to the front before the transform's new set evicts the least
        # recently used one, or the call frees the tables it holds.  ntt_coset_table = 0: the transform itself reads the held power tables (with the table, only the
        # kernel that fills it does, before the second set is built)
        assert (_w(orc, pyref, ek) == domain_of(orc, k, e).extended_omega).all()      # (the set zk_ntt leaves is the one the coset transform looks up)
        fill_sets(be, orc, pyref, avoid=(k, ek), first=((ek, False),))
        be.tune(ntt_coset_table=0)
        try:
            check_coset(be, orc, pyref, k, e, 1)
        finally:
            be.tune(ntt_coset_table=1)
        transform(be, orc, pyref, ek, False, seed=9, what="the held set afterwards")
        check_coset(be, orc, pyref, k, e, 2, seed=5)
    elif op == "pieces":
        fill_sets(be, orc, pyref, avoid=(k, ek))
        tc._check_pieces(be, orc, pyref, k, e, 3, seed=k)
    elif op == "grand_product":
        fill_sets(be, orc, pyref, avoid=(k,))
        tgp._check_backend(be, orc, pyref, k, 2, seed=k)
    elif op == "g1_ntt":
        g = S["g1_large"]
        fill_sets(be, orc, pyref, avoid=(g,))
        ptc.check_g1_ntt(be, orc, pyref, g, "few", seed=g)
    else:
        raise ValueError(op)
    transform(be, orc, pyref, 1, False, seed=7, what="after the call")


HELD_POINTER_OPS = ("coset_new_sets", "coset_oldest_set_is_held", "pieces", "grand_product", "g1_ntt")


def check_lagrange_to_coeff(be, orc, pyref, k, seed=0, what=""):
    od = orc.Domain(4, k)
    a = pc.rand_fr(orc, pyref, 1 << k, 7 * k + seed)
    d = be.to_device(a)
    try:
        be.lagrange_to_coeff_dev(d, k)
        assert (d.download((1 << k, 4)) == od.lagrange_to_coeff(a)).all(), ("lagrange_to_coeff", k, what)
    finally:
        d.free()


def retuning(be, orc, pyref, S, knob):
    """the same (log n, omega) under setting A, then B, then A again: the second A finds the set the first one left"""
    log_n, base = S["retune_log"], dict(ntt_tile_log=S["tile"], ntt_max_radix_log=S["radix"])
    try:
        if knob == "plan":
            for tile, radix in S["plans"]:
                for setting in (base, dict(ntt_tile_log=tile, ntt_max_radix_log=radix), base, dict(ntt_tile_log=tile, ntt_max_radix_log=radix)):
                    be.tune(**setting)
                    pc.check_ntt(be, orc, pyref, log_n, seed=tile, kind="uniform")
                    pc.check_ntt(be, orc, pyref, log_n, seed=radix, kind="minus_one", inverse=True)
        elif knob == "fuse_scale":
            for i, v in enumerate((1, 0, 1, 0)):
                be.tune(ntt_fuse_scale=v)
                check_lagrange_to_coeff(be, orc, pyref, log_n, seed=i, what=("ntt_fuse_scale", v))
                pc.check_domain(be, orc, pyref, 4, S["coset_k"], seed=50 + i)
        elif knob == "full_twiddle":
            for i, v in enumerate((24, 0, 24, 0)):
                be.tune(ntt_full_twiddle_max_log=v)
                pc.check_ntt(be, orc, pyref, log_n, seed=i, inverse=bool(i % 2))
                check_lagrange_to_coeff(be, orc, pyref, log_n, seed=i, what=("ntt_full_twiddle_max_log", v))
        elif knob == "coset_table":
            k, e = S["coset_k"], S["coset_e"]
            check_coset(be, orc, pyref, k, e, 1)                     # (the table of coset 1 is cached from here on)
            for i, v in enumerate((1, 0, 1, 0, 1)):
                be.tune(ntt_coset_table=v)
                check_coset(be, orc, pyref, k, e, 1, seed=i)
                check_coset(be, orc, pyref, k, e, 3, seed=i)
        else:
            raise ValueError(knob)
    finally:
        be.tune(ntt_fuse_scale=1, ntt_full_twiddle_max_log=24, ntt_coset_table=1, **base)


RETUNE_KNOBS = ("plan", "fuse_scale", "full_twiddle", "coset_table")


def check_ntt_batch(be, orc, pyref, log_n, count, seed=0, what=""):
    n = 1 << log_n
    cols = [pc.rand_fr(orc, pyref, n, seed + 3 * i) for i in range(count)]
    w = _w(orc, pyref, log_n)
    d = [be.to_device(c) for c in cols]
    try:
        be.ntt_batch_dev(d, log_n, w) if count > 1 else be.ntt_dev(d[0], log_n, w)
        for i, (c, dd) in enumerate(zip(cols, d)):
            assert (dd.download((n, 4)) == orc.best_fft(c, w, log_n)).all(), (what, "log n", log_n, "column", i, "of", count)
    finally:
        for dd in d:
            dd.free()


def check_padded_extended(be, orc, pyref, k, e, seed=0):
    """coeff_to_extended: 3/4 and more of the transform's input is zero padding (the quarter-input path of the first pass)"""
    od = domain_of(orc, k, e)
    a = pc.rand_fr(orc, pyref, 1 << k, seed + k)
    d, o = be.to_device(a), be.alloc((32 << k) << e)
    try:
        be.coeff_to_extended_dev(d, k, k + e, o)
        assert (o.download(((1 << k) << e, 4)) == od.coeff_to_extended(a)).all(), ("coeff_to_extended", k, e)
    finally:
        d.free()
        o.free()


def ntt_workspace(be, orc, pyref, S):
    """ws_ntt through its shapes: a large batch; one small column through the single-pass copy; a batch cut into slices of 4, 4 and 1 columns by ntt_ws_limit_mb = 1
    (9 columns of 2^13 x 32 B = 256 KiB each); the mixed-kind batch; the zero-padded extension — then the first steps again.  No statistic says which path a batch
    took: that the limit cuts this batch into 4, 4 and 1 columns is asserted from the sizes (ntt_dev_batch's own rule), and what the test observes of the sliced path
    is the parity of all nine outputs"""
    steps = [lambda: check_ntt_batch(be, orc, pyref, S["ws_big"], 8, seed=1, what="batch of 8"),
             lambda: check_ntt_batch(be, orc, pyref, 3, 1, seed=2, what="one small column")]

    def sliced():
        assert (9 << S["ws_sliced"]) * 32 > (1 << 20) and (1 << 20) // (32 << S["ws_sliced"]) == 4
        be.tune(ntt_ws_limit_mb=1)
        try:
            check_ntt_batch(be, orc, pyref, S["ws_sliced"], 9, seed=3, what="slices of 4, 4 and 1")
        finally:
            be.tune(ntt_ws_limit_mb=24576)
    steps += [sliced,
              lambda: tsv._ntt_device_forms(be, orc, pyref, S["forms_log"], ("uniform",) + tsv.KINDS, single=False),
              lambda: check_padded_extended(be, orc, pyref, S["coset_k"], 2, seed=4)]
    for step in steps + steps[:3]:
        step()


# ---- C. the ws_tmp sharers ---------------------------------------------------------------------------------------------------------------------------------------
SMALL_KINDS = ("zeros", "const", "minus_one")
HINT_K = 9                                                             # lookup_cases.hint_steps: the rows its tie ranges need


def _structured(orc, pyref, n, count, seed):
    return [pc.structured_fr(orc, pyref, n, SMALL_KINDS[(seed + i) % 3], seed + i) for i in range(count)]


def check_interleave(be, orc, pyref, k, count, seed, cols=None):
    """zk_fr_interleave_dev is data movement: out[i * count + j] = cosets[j][i], by numpy"""
    n = 1 << k
    cols = cols if cols is not None else [pc.rand_fr(orc, pyref, n, seed + i) for i in range(count)]
    d, o = [be.to_device(c) for c in cols], be.alloc(n * len(cols) * 32)
    try:
        be.fr_interleave_dev(d, n, o)
        want = np.ascontiguousarray(np.stack(cols, axis=1).reshape(n * len(cols), 4))
        assert (o.download((n * len(cols), 4)) == want).all(), ("fr_interleave", k, len(cols))
    finally:
        for x in d + [o]:
            x.free()


def check_kate(be, orc, pyref, n, count, seed, polys=None):
    polys = polys if polys is not None else [pc.rand_fr(orc, pyref, n, seed + i) for i in range(count)]
    pts = pc.rand_fr(orc, pyref, len(polys), seed + 77)
    for p, b in zip(polys, pts):
        assert (z.arithmetic.kate_division(p, b, backend=be) == orc.kate_division(p, b)).all(), ("kate_division", n)


def sharer(name, be, orc, pyref, S, small, seed=0):
    """one of the nine operations that keep their arguments, counters or scratch in ws_tmp, in its large dense form (2^large_k rows, several columns) or its small one
    (2^small_k rows, one column where the operation takes a count, columns of zeros / a constant / r - 1); each against its oracle"""
    R = pyref.R
    k = S["small_k"] if small else S["large_k"]
    n, seed = 1 << k, seed + (1000 if small else 0)
    sfr = lambda count: _structured(orc, pyref, n, count, seed)
    if name == "permutation_product_all":
        inputs = (sfr(5), sfr(5)[::-1]) + tuple(pc.rand_fr(orc, pyref, 2, seed + 5)) if small else None
        tgp._check_commit(be, orc, pyref, k, inputs)
    elif name == "lookup_product_batch":
        inputs = (sfr(1), _structured(orc, pyref, n, 1, seed + 1)) + tuple(pc.rand_fr(orc, pyref, 2, seed + 5)) if small else None
        tgp._check_backend(be, orc, pyref, k, 1 if small else 4, seed=seed + k, inputs=inputs)
    elif name == "eval_polynomial_batch":
        tep._check(be, orc, pyref, n, 1 if small else 5, seed=seed + k, polys=sfr(1) if small else None)
    elif name == "kate_division":
        check_kate(be, orc, pyref, n, 1 if small else 3, seed + k, polys=_structured(orc, pyref, n, 1, seed + 2) if small else None)
    elif name == "fr_lincomb":
        tep._check_lincomb(be, orc, pyref, n, 1 if small else 4, seed=seed + k, polys=sfr(1) if small else None)
    elif name == "lookup_permute_batch":
        case = lc.multiset(R, k, 5, ("zeros", "const_table")[seed % 2], seed) if small else lc.shared_table_batch(R, k, 5, 3, tables=1, seed=seed)
        lc.run(be, orc, pyref, case, seed, entries=("batch",))
    elif name == "cosets_to_pieces":
        tc._check_pieces(be, orc, pyref, k, 2, 1 if small else 3, seed=seed + k, kinds=SMALL_KINDS[1:] if small else ("uniform",))
    elif name == "fr_interleave":
        check_interleave(be, orc, pyref, k, 1 if small else 4, seed + k, cols=sfr(1) if small else None)
    elif name == "g1_ntt":
        ptc.check_g1_ntt(be, orc, pyref, S["g1_small"] if small else S["g1_large"], "all_identity" if small else "few", seed=seed + k)
    else:
        raise ValueError(name)


SHARERS = ("permutation_product_all", "lookup_product_batch", "eval_polynomial_batch", "kate_division", "fr_lincomb", "lookup_permute_batch", "cosets_to_pieces",
           "fr_interleave", "g1_ntt")


def sharer_pairs(be, orc, pyref, S, polluter):
    """every ordered pair (large `polluter`, small victim != polluter) on ONE context: all the small forms on the fresh context first, then polluter, victim, polluter, .."""
    victims = [v for v in SHARERS if v != polluter]

    def run(name, small, what):
        try:
            sharer(name, be, orc, pyref, S, small)
        except AssertionError as e:
            raise AssertionError("%s: %s form of %s (the polluter is the large %s): %s" % (what, "small" if small else "large", name, polluter, e)) from e
    for v in victims:
        run(v, True, "1. victim on the fresh context")
    for v in victims:
        run(polluter, False, "2. polluter")
        run(v, True, "3. victim after the polluter")
    run(polluter, False, "4. polluter after the victim")


def counters(be, orc, pyref, S, which):
    """a counter in ws_tmp counts from zero on every call: planted bad words / values the table lacks, then clean input, after a dense call of another sharer"""
    sharer("eval_polynomial_batch", be, orc, pyref, S, small=False)
    if which == "g1_decompress":
        for sign_bit in (255, 254):
            ptc.check_codec(be, orc, pyref, S["codec_n"], sign_bit)  # clean, planted (the count is exact), clean again: 0
            sharer("fr_lincomb", be, orc, pyref, S, small=False)
    else:
        k = S["small_k"] + 1
        for kind in lc.NOT_IN_TABLE_KINDS:
            lc.run_refused(be, orc, pyref, lc.not_in_table(pyref.R, k, 5, kind, seed=2), seed=2)      # refused on both entries, then the good twin on the same context
            sharer("kate_division", be, orc, pyref, S, small=False)
        lookup_column_words(be, orc, pyref)


def lookup_column_words(be, orc, pyref):
    """the per-column words of lookup_permute (64 bytes per sorted column at `o_cs` in ws_tmp: the OR of the column's keys in words 0 .. 7, reused as the tie mask; the
    order violations in word 8) start from zero on every call.  The polluter has the victims' SHAPE — one lookup, two sorted columns, 2^HINT_K rows, so every piece of
    the workspace, `o_cs` among them, lies at the same offset — and keys whose 64-bit windows end at bit 253, all different: it is sorted without a refinement, so it
    leaves the OR of 254-bit keys in those words and no tie hint on the context (a tied polluter of this shape would set the hint, which is host state, and the hint
    sequence pins the path of a context without one).  The victim is a column of 64-bit keys: on stale words its window would end at bit 253 too, every key of the
    window would be zero, and the column would have to be refined.  The outputs are right either way — the refinement sorts exactly — so each step asserts the PATH:
    (refined, hinted) columns from the library's statistics, next to the oracle's values.  Then the hint sequence of lookup_cases, which must take the path of a
    context that has never seen its shape"""
    R = pyref.R
    steps = lc.hint_steps(R, HINT_K, 5)
    narrow = next(case for name, case, _, _ in steps if name.startswith("5."))
    wide = lc._untied(R, HINT_K, 5, 190, random.Random(5))
    assert all(lc.window(col)[1] == 190 for col in wide.inputs + wide.tables) and all(lc.window(col)[1] == 0 for col in narrow.inputs + narrow.tables)
    assert len(wide.inputs) == len(narrow.inputs) == 1 and all(len(case.inputs) == 1 and case.k == HINT_K for _, case, _, _ in steps)       # one shape throughout
    tsl._hint_sequence(be, orc, pyref, [("victim on the fresh context", narrow, 0, 0), ("polluter: wide keys, no ties", wide, 0, 0), ("victim after the polluter", narrow, 0, 0),
                                        ("polluter after the victim", wide, 0, 0)] + steps)


# ---- D. quotient state -------------------------------------------------------------------------------------------------------------------------------------------
def quotient_state(be, orc, pyref, S, jit=0, reload=False):
    """81 live intermediates on 2^quot_big rows per coset (four cosets: 2^10 rows on the GPU), then 5 on 2^quot_small, then 81 again — and 5 again.  run_case loads,
    runs (whole domain, cosets, parts, row slices) and releases the program; reload: a handle of the large program is held across the small one's run and released, and
    the program loaded again, between the runs"""
    big, small = pg.ladder_program(81, S["quot_big"]), pg.ladder_program(5, S["quot_small"])
    kw = dict(expect_kernels=1) if jit else {}
    if jit:
        be.tune(quot_jit=jit, quot_jit_group=48)
    try:
        run = lambda prog, seed, **more: qc.run_case(be, orc, pyref, pc, prog, seed=seed, **kw, **more)
        if jit:
            # the case is bound by the compiler, not by its rows: hiprtc builds the 81-slot program's kernels in 17.8 s at quot_jit_group = 48 (23.0 s at 12, 20.6 s at 100,
            # about 65 s at the default 200; docs/LOG_r11.md), so each program is built ONCE and kept loaded across the other's runs
            e_big, e_small = ev.Evaluator(big, backend=be), ev.Evaluator(small, backend=be)
            try:
                for prog, e, seed in ((big, e_big, 81), (small, e_small, 5), (big, e_big, 81), (small, e_small, 6)):
                    run(prog, seed, evaluator=e)
            finally:
                e_big.release()
                e_small.release()
        elif reload:
            h = be.quotient_program_load(big.to_blob())
            assert be.quotient_program_info(h)["slots"] == 81
            run(small, 5)
            run(big, 81)
            be.quotient_program_release(h)
            run(small, 6)
            h = be.quotient_program_load(big.to_blob())
            run(big, 82)
            be.quotient_program_release(h)
            run(small, 5)
        else:
            run(big, 81)
            run(small, 5)
            run(big, 81)
            run(small, 5)
    finally:
        if jit:
            be.tune(quot_jit=0, quot_jit_group=200)


# ---- E. whole proofs on a used context ---------------------------------------------------------------------------------------------------------------------------
_PROOFS = {}


def proof_circuit(k, with_lookup):
    """the toy circuit of test_create_proof (satisfied, so the verifier can accept): A with its lookup, B without — degree 3, one permutation column per set"""
    key = ("history", k, with_lookup)
    if key not in _PROOFS:
        cs, fixed, asm, advice, instances = tcp.toy_circuit(k, with_lookup=with_lookup)
        _PROOFS[key] = dict(key=key, k=k, cs=cs, fixed=fixed, asm=asm, advice=advice, instances=instances, want={})
    return _PROOFS[key]


def oracle_proof(circ, seed):
    """the independent CPU prover's bytes (oracle/prover.py, Python integers) — what a fresh context emits (tests/test_structured_proofs.py) —, accepted by verify_proof"""
    import verifier
    if seed not in circ["want"]:
        proof = prc.oracle_proof(circ["k"], tcp.TAU, circ["cs"], circ["fixed"], circ["asm"], circ["advice"], circ["instances"], np.random.default_rng(seed), circ["key"], require_satisfied=True)
        _, keys = prc.oracle_keys(circ["k"], tcp.TAU, circ["cs"], circ["fixed"], circ["asm"], circ["key"])
        assert verifier.verify_proof(keys, tcp.TAU, circ["instances"], proof) is True
        circ["want"][seed] = proof
    return circ["want"][seed]


def proofs_on_a_used_context(be, orc, S, side_lane, trim, mock):
    """A, B, A, B through zk_plonk_create_proof on one context: every proof the oracle's bytes, which verify_proof accepts"""
    circs = [proof_circuit(S["proof_a"], True), proof_circuit(S["proof_b"], False)]
    assert circs[0]["cs"].lookups and not circs[1]["cs"].lookups
    be.tune(prover_side_lane=side_lane)
    made = []
    try:
        for c in circs:
            params = z.kzg.ParamsKZG.setup(c["k"], tcp.TAU, backend=be)
            pk = plonk.keygen(params, c["cs"], c["fixed"], c["asm"])
            made.append((params, pk, plonk.NativeProver(params, pk)))
        for step, (i, seed) in enumerate(((0, 11), (1, 12), (0, 11), (1, 12))):
            c = circs[i]
            got = made[i][2].create_proof([a.copy() for a in c["advice"]], c["instances"], np.random.default_rng(seed))
            want = oracle_proof(c, seed)
            assert got == want, ("proof", step, "circuit", "AB"[i], "side lane", side_lane, "first differing 32-byte word", prc.first_difference(got, want))
            if trim:
                be.trim_pool()
            if mock and step == 1:
                a = circs[0]
                assert plonk.NativeMockProver.run(a["k"], a["cs"], a["fixed"], a["advice"], a["instances"], a["asm"], backend=be).verify() == []
    finally:
        for params, pk, _ in made:
            pk.release()
            params.release()
        be.tune(prover_side_lane=1)


PROOF_VARIANTS = (dict(side_lane=0, trim=False, mock=False), dict(side_lane=2, trim=True, mock=False), dict(side_lane=2, trim=False, mock=True), dict(side_lane=0, trim=True, mock=True))
proof_variant_id = lambda v: "lane%d%s%s" % (v["side_lane"], "-trim" if v["trim"] else "", "-mock" if v["mock"] else "")


# ---- F. a refused call leaves the context usable -----------------------------------------------------------------------------------------------------------------
def refused(be, orc, pyref, S, which, base):
    """argument refusals (negative return codes, nothing faults) in the middle of a call; with the tunable restored, the small victims on the same context.
    base: the backend's own value of every tunable the case moves"""
    if which == "msm_block":                                           # refused after the sort kernels of the call have run
        c, n = S["msm_narrow"], S["msm_n"]
        t = MsmTable(be, orc, pyref, n, c, False)
        try:
            dense, sp = dense_columns(orc, pyref, n, c), sparse_columns(orc, pyref, n, c)
            t.check(dense, "before")
            be.tune(msm_block=512)
            try:
                with pytest.raises(z.ZkError) as err:
                    t.check(dense, "refused")
                assert err.value.code == ZK_ERR_ARG and "msm_block" in str(err.value), err.value
            finally:
                be.tune(msm_block=base["msm_block"])
            sequence(lambda what: t.check([sp["zeros"], sp["first"], sp["last"], sp["top_window"]], what), lambda what: t.check(dense, what))
        finally:
            t.release()
        return
    if which in ("ntt_threads", "ntt_radix"):                          # refused after the twiddle set of the call has been built and cached
        log_n = 3 * S["tile"] // 2 + 2                                 # several passes under the backend's plan (ntt_threads is the strided passes' limit)
        moved = dict(ntt_threads=512) if which == "ntt_threads" else dict(ntt_tile_log=(log_n - 1) // 3)      # .. ntt_max_radix_log above the tile: three radices, the first exceeds it
        assert which == "ntt_threads" or base["ntt_max_radix_log"] > moved["ntt_tile_log"]
        transform(be, orc, pyref, log_n, what="before")
        be.tune(**moved)
        try:
            with pytest.raises(z.ZkError) as err:
                transform(be, orc, pyref, log_n, what="refused")
            assert err.value.code == ZK_ERR_ARG and ("ntt_threads" if which == "ntt_threads" else "exceeds the LDS tile") in str(err.value), err.value
        finally:
            be.tune(**{key: base[key] for key in moved})
        sequence(lambda what: check_ntt_batch(be, orc, pyref, 3, 1, seed=8, what=what), lambda what: check_ntt_batch(be, orc, pyref, log_n, 3, seed=9, what=what))
        transform(be, orc, pyref, log_n, inverse=True, what="after")
        return
    assert which == "slots"                                            # the 82nd live intermediate: refused when the program is loaded
    small = pg.ladder_program(5, S["quot_small"])
    qc.run_case(be, orc, pyref, pc, pg.ladder_program(81, S["quot_small"]), seed=1, check_cosets=False)
    with pytest.raises(z.ZkError) as err:
        be.quotient_program_load(pg.live_program(pg.MAX_SLOTS, S["quot_small"], 4, 2).to_blob())
    assert err.value.code == ZK_ERR_LIMIT, err.value
    qc.run_case(be, orc, pyref, pc, small, seed=5)


REFUSALS = ("msm_block", "ntt_threads", "ntt_radix", "slots")
