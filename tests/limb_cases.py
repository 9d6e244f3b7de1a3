"""The limb routines every kernel sits on (csrc/field.cuh, field29.cuh, ec.cuh), driven through tests/csrc/limb_cases.h: the case generators, the exact models and the
checks, as functions that take a RUNNER.  HostRunner drives libhostharness.so (the routines compiled for the CPU: the plain C++ branches of field_mac.inc /
field29_mac.inc; tests/test_field29.py, tests/test_host_logic.py); DeviceRunner drives libdevharness.so (the same functions in HIP kernels: the inline-assembly branches;
tests/test_limbs_device.py) and holds every device result against the host's, bit for bit.  A check never knows which of the two it talks to."""
import ctypes as C
import math
import random

import numpy as np

M29 = (1 << 29) - 1
RAD = 1 << 261


def P(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- runners ------------------------------------------------------------------------------------------------------------------------------------------------------
FIELD_OPS = {"fr_mul": 2, "fr_add": 2, "fr_sub": 2, "fr_neg": 1, "fr_inv": 1, "fr_from_mont": 1, "fq_mul": 2, "fq_add": 2, "fq_sub": 2, "fq_mul2_sub": 4}   # name: operands
PAIR_OPS = {"xyzz_add": 2, "xyzz_add_lazy": 2, "xyzz_dbl": 1}
CHAIN_KINDS = ("xyzz_sum", "xyzz_sum_lazy", "xyzz29_sum")


class Runner:
    """what the checks call.  The primitives (_f29_raw, _f29_forms, _fq_lazy, _field, _pair, _chains, _probe: arrays in, arrays out) are the subclasses'."""

    def f29_raw(self, field, op, *ops):
        """rows of 9 limbs (lists) -> rows of 9 limbs; missing operands are zero rows"""
        n = len(ops[0])
        bufs = [arr(o) for o in ops] + [arr([[0] * 9] * n)] * (4 - len(ops))
        return [[int(v) for v in row] for row in self._f29_raw(field, op, *bufs)]

    def f29_forms(self, field, op, A, B):
        """(n, 4) uint64 x 2 -> the 32-bit-limb output as (n, 4) uint64 and the 29-bit-limb one as rows of 9 ints"""
        o, o9 = self._f29_forms(field, op, A, B)
        return o, [[int(v) for v in row] for row in o9]

    def fq_lazy(self, op, A, B, C_, D):
        return self._fq_lazy(op, A, B, C_, D)

    def v2(self, name, A, B):                                    # "fr_mul", "fq_sub", ...
        return self._field(name, A, B)

    def v1(self, name, A):                                       # "fr_inv", "fr_neg", "fr_from_mont"
        return self._field(name, A)

    def mul2_sub(self, A, B, C_, D):
        return self._field("fq_mul2_sub", A, B, C_, D)

    def xyzz_add(self, a, b):                                    # one XYZZ point each, 16 uint64
        return self._pair("xyzz_add", a.reshape(1, 16), b.reshape(1, 16))[0]

    def xyzz_add_lazy(self, a, b):
        return self._pair("xyzz_add_lazy", a.reshape(1, 16), b.reshape(1, 16))[0]

    def xyzz_dbl(self, a):
        return self._pair("xyzz_dbl", a.reshape(1, 16))[0]

    def chains(self, kind, seqs):
        """seqs: [(affine points (n, 8) uint64, signs (n,) uint8)] -> [XYZZ (16,) uint64] per chain; for xyzz29_sum [(XYZZ, n_rare)]"""
        outs, rare = self._chains(kind, [np.ascontiguousarray(s[0]).reshape(-1, 8) for s in seqs], [np.ascontiguousarray(s[1], dtype=np.uint8) for s in seqs])
        return [(o, int(r)) for o, r in zip(outs, rare)] if kind == "xyzz29_sum" else list(outs)

    def xyzz_sum(self, pts, neg):
        return self.chains("xyzz_sum", [(pts, neg)])[0]

    def xyzz_sum_lazy(self, pts, neg):
        return self.chains("xyzz_sum_lazy", [(pts, neg)])[0]

    def xyzz29_sum(self, pts, neg):
        return self.chains("xyzz29_sum", [(pts, neg)])[0]

    def filter_probe(self, inputs, check=1, probes=True):
        """inputs: [(start (8,), steps (n_steps, 8), prefix (>= length, 8), length)], the same n_steps everywhere -> [(four counts, XYZZ)] per chain"""
        counts, outs = self._probe([i[0] for i in inputs], [i[1] for i in inputs], [np.ascontiguousarray(i[2][:i[3]]) for i in inputs] if probes else None,
                                   [i[3] for i in inputs], check)
        return [([int(v) for v in c], o) for c, o in zip(counts, outs)]


class HostRunner(Runner):
    """libhostharness.so: one call per op, one call per chain"""

    def __init__(self, lib):
        self.lib = lib

    def _f29_raw(self, field, op, a, b, c, d):
        out = np.zeros((len(a), 9), dtype=np.uint32)
        self.lib.hh_f29_raw(C.c_int(field), C.c_int(op), P(a), P(b), P(c), P(d), P(out), C.c_size_t(len(a)))
        return out

    def _f29_forms(self, field, op, A, B):
        o, o9 = np.zeros_like(A), np.zeros((len(A), 9), dtype=np.uint32)
        self.lib.hh_f29_forms(C.c_int(field), C.c_int(op), P(A), P(B), P(o), P(o9), C.c_size_t(len(A)))
        return o, o9

    def _fq_lazy(self, op, A, B, C_, D):
        out = np.empty_like(A)
        self.lib.hh_fq_lazy(C.c_int(op), P(A), P(B), P(C_), P(D), P(out), C.c_size_t(len(A)))
        return out

    def _field(self, name, *ins):
        assert len(ins) == FIELD_OPS[name]
        out = np.empty_like(ins[0])
        getattr(self.lib, "hh_" + name)(*[P(a) for a in ins], P(out), C.c_size_t(len(ins[0])))
        return out

    def _pair(self, name, *ins):
        assert len(ins) == PAIR_OPS[name]
        out = np.zeros_like(ins[0])
        for i in range(len(ins[0])):
            getattr(self.lib, "hh_" + name)(*[P(np.ascontiguousarray(a[i])) for a in ins], P(out[i]))
        return out

    def _chains(self, kind, pts, negs):
        outs, rares = np.zeros((len(pts), 16), dtype=np.uint64), np.zeros(len(pts), dtype=np.uint32)
        for i, (a, ng) in enumerate(zip(pts, negs)):
            if kind == "xyzz29_sum":
                rare = C.c_uint32()
                self.lib.hh_xyzz29_sum(P(a), P(ng), C.c_size_t(len(ng)), P(outs[i]), C.byref(rare))
                rares[i] = rare.value
            else:
                getattr(self.lib, "hh_" + kind)(P(a), P(ng), C.c_size_t(len(ng)), P(outs[i]))
        return outs, rares

    def _probe(self, starts, steps, prefixes, lens, check):
        counts, outs = np.zeros((len(starts), 4), dtype=np.uint64), np.zeros((len(starts), 16), dtype=np.uint64)
        for i in range(len(starts)):
            st = np.ascontiguousarray(steps[i])
            self.lib.hh_xyzz29_filter_probe(P(np.ascontiguousarray(starts[i])), P(st), C.c_size_t(len(st)), P(prefixes[i]) if prefixes is not None else None,
                                            C.c_size_t(lens[i]), C.c_int(check), P(counts[i]), P(outs[i]))
        return counts, outs


BLOCKS = (64, 256)


def layouts(n):
    """the row orders one element-wise op is launched in: index arrays into the caller's rows.  First the n rows under a fixed stride permutation — a generator's boundary
    rows sit together at one end of its list; the stride sends neighbours to different waves, so every wave of 64 mixes carry patterns — then, for n up to 256, the same
    stride walk continued to 293 rows: more than one block of 256, a partial last wave.  A count that is a multiple of 64 gets one more row: no launch is all full waves."""
    s = max(1, int(n * 0.618))
    while math.gcd(s, n) != 1:
        s += 1
    walk = lambda m: np.array([(j * s) % n for j in range(m)], dtype=np.int64)
    out = [walk(n + (n % 64 == 0))]
    if n <= 256:
        out.append(walk(293))
    return out


class DeviceRunner(Runner):
    """libdevharness.so.  Every element-wise op runs in each of layouts(n) with block 64 and with block 256; chains run `chains` to a launch, one chain per thread, with
    both block sizes.  What the checks get back is the DEVICE's output (first layout, block 64) in the caller's row order.  Every launch's output is also compared with the
    host harness's on all limbs — these are deterministic limb algorithms: one right representative inside the allowed range — and the differences are collected in
    `self.differs`, which the test asserts empty AFTER the models have had their say (the models remain the reference).  A non-zero HIP status fails the test and
    poisons the runner: it launches nothing more."""

    def __init__(self, lib, host):
        self.lib, self.host, self.status, self.differs, self.launches = lib, host, 0, [], 0

    def _launch(self, name, *args):
        assert self.status == 0, "an earlier device call returned HIP status %d: nothing more is launched" % self.status
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        self.launches += 1
        st = fn(*args)
        if st != 0:
            self.status = st
        assert st == 0, "%s returned HIP status %d" % (name, st)

    def _compare(self, what, got, want, rows=None):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        if bad.size:
            self.differs.append("%s: device != host at %d of %d rows, first %s" % (what, bad.size, len(got), (rows[bad] if rows is not None else bad)[:6].tolist()))

    def assert_equal_to_host(self):
        assert not self.differs, "\n".join(self.differs)

    def _elementwise(self, what, name, head, ins, host_outs):
        n = len(ins[0])
        result = None
        for idx in layouts(n):
            g = [np.ascontiguousarray(a[idx]) for a in ins]
            for block in BLOCKS:
                outs = [np.zeros((len(idx),) + h.shape[1:], dtype=h.dtype) for h in host_outs]
                self._launch(name, *head, *[P(a) for a in g], *[P(o) for o in outs], C.c_size_t(len(idx)), C.c_int(block))
                for o, h in zip(outs, host_outs):
                    self._compare("%s, %d rows, block %d" % (what, len(idx), block), o, h[idx], idx)
                if result is None:
                    result = [np.zeros_like(h) for h in host_outs]
                    for r, o in zip(result, outs):
                        r[idx] = o
        return result

    def _f29_raw(self, field, op, a, b, c, d):
        return self._elementwise("f29_raw field %d op %d" % (field, op), "dh_f29_raw", (C.c_int(field), C.c_int(op)), [a, b, c, d], [self.host._f29_raw(field, op, a, b, c, d)])[0]

    def _f29_forms(self, field, op, A, B):
        return self._elementwise("f29_forms field %d op %d" % (field, op), "dh_f29_forms", (C.c_int(field), C.c_int(op)), [A, B], list(self.host._f29_forms(field, op, A, B)))

    def _fq_lazy(self, op, A, B, C_, D):
        return self._elementwise("fq_lazy op %d" % op, "dh_fq_lazy", (C.c_int(op),), [A, B, C_, D], [self.host._fq_lazy(op, A, B, C_, D)])[0]

    def _field(self, name, *ins):
        assert len(ins) == FIELD_OPS[name]
        return self._elementwise(name, "dh_" + name, (), list(ins), [self.host._field(name, *ins)])[0]

    def _pair(self, name, *ins):
        assert len(ins) == PAIR_OPS[name]
        return self._elementwise(name, "dh_" + name, (), list(ins), [self.host._pair(name, *ins)])[0]

    def _chains(self, kind, pts, negs):
        off = np.concatenate([[0], np.cumsum([len(ng) for ng in negs])]).astype(np.uint64)
        allp = np.ascontiguousarray(np.concatenate(pts)) if int(off[-1]) else np.zeros((1, 8), dtype=np.uint64)
        alln = np.ascontiguousarray(np.concatenate(negs)) if int(off[-1]) else np.zeros(1, dtype=np.uint8)
        h_outs, h_rare = self.host._chains(kind, pts, negs)
        first = None
        for block in BLOCKS:
            outs, rares = np.zeros((len(pts), 16), dtype=np.uint64), np.zeros(len(pts), dtype=np.uint32)
            tail = (P(outs), P(rares)) if kind == "xyzz29_sum" else (P(outs),)
            self._launch("dh_" + kind, P(allp), P(alln), P(off), C.c_size_t(len(pts)), *tail, C.c_int(block))
            self._compare("%s, %d chains, block %d" % (kind, len(pts), block), outs, h_outs)
            self._compare("%s n_rare, %d chains, block %d" % (kind, len(pts), block), rares, h_rare)
            first = first or (outs, rares)
        return first

    def _probe(self, starts, steps, prefixes, lens, check):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        st, sp = np.ascontiguousarray(np.stack(starts)), np.ascontiguousarray(np.stack(steps))
        pre = np.ascontiguousarray(np.concatenate(prefixes)) if prefixes is not None else None
        assert pre is None or len(pre) == int(off[-1])
        h_counts, h_outs = self.host._probe(starts, steps, prefixes, lens, check)
        first = None
        for block in BLOCKS:
            counts, outs = np.zeros((len(starts), 4), dtype=np.uint64), np.zeros((len(starts), 16), dtype=np.uint64)
            self._launch("dh_xyzz29_filter_probe", P(st), P(sp), C.c_size_t(sp.shape[1]), P(pre) if pre is not None else None, P(off), C.c_size_t(len(starts)), C.c_int(check),
                         P(counts), P(outs), C.c_int(block))
            self._compare("filter probe counts, block %d" % block, counts, h_counts)
            self._compare("filter probe end points, block %d" % block, outs, h_outs)
            first = first or (counts, outs)
        return first


# ---- 29-bit limbs: rows and the exact column models ---------------------------------------------------------------------------------------------------------------
def limbs_of(x, loose=None, rnd=None):
    """x as 9 limbs; `loose` (bits) re-distributes value between neighbours so that limbs use up to that many bits (same integer)"""
    l = [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]
    if loose:
        for i in range(8, 0, -1):
            room = int(2 ** loose) - 1 - l[i - 1]
            take = min(l[i], room >> 29, rnd.randrange(0, 8))
            l[i] -= take
            l[i - 1] += take << 29
    return l


def value(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def arr(rows):
    return np.array(rows, dtype=np.uint32).reshape(len(rows), 9)


def model_mul(mod, pairs):
    """sum of a*b over `pairs` of limb vectors, times 2^-261: exact product scanning, every column checked against 2^64"""
    pl = limbs_of(mod)
    inv = (-pow(mod, -1, 1 << 29)) % (1 << 29)
    acc, m, r = 0, [], [0] * 9
    for k in range(17):
        for a, b in pairs:
            for i in range(max(0, k - 8), min(k, 8) + 1):
                acc += a[i] * b[k - i]
        for i in range(max(0, k - 8), min(k, 9)):
            if i < len(m) and k - i <= 8:
                acc += m[i] * pl[k - i]
        if k < 9:
            m.append((acc & M29) * inv & M29)
            acc += m[k] * pl[0]
            assert acc & M29 == 0
        else:
            r[k - 9] = acc & M29
        assert acc < 1 << 64, ("column overflows the 64-bit accumulator", k, acc.bit_length())
        acc >>= 29
    r[8] = acc
    assert acc < 1 << 32
    return r


def bias(mod, K, LOG):
    t = K * mod - sum(1 << (LOG + 29 * i) for i in range(8))
    assert t > 0
    return [(1 << LOG) + ((t >> (29 * i)) & M29) for i in range(8)] + [t >> 232]


def model_shoup(mod, a, w, wq):
    """the generated body, column for column: q from columns 7 .. 16 of a * wq, r = low 261 bits of a * w + q * (2^261 - p)"""
    npl = limbs_of(RAD - mod)
    acc, q = 0, [0] * 9
    for k in range(7, 17):
        acc += sum(a[i] * wq[k - i] for i in range(max(0, k - 8), min(k, 8) + 1))
        assert acc < 1 << 64
        if k >= 9:
            q[k - 9] = acc & M29
        acc >>= 29
    q[8] = acc
    assert acc < 1 << 32
    acc, r = 0, [0] * 9
    for k in range(9):
        acc += sum(a[i] * w[k - i] + q[i] * npl[k - i] for i in range(k + 1))
        assert acc < 1 << 64
        r[k] = acc & M29
        acc >>= 29
    return r, q


# ---- field29.cuh ----------------------------------------------------------------------------------------------------------------------------------------------------
def check_products_on_raw_limbs(run, pyref, field):
    mod = pyref.P if field == 0 else pyref.R
    rnd = random.Random(29 + field)
    vals = [0, 1, mod - 1, mod, 2 * mod - 1, 7 * mod - 1, 10 * mod - 3, 32 * mod - 1, (1 << 261) - 1] + [rnd.randrange(0, 12 * mod) for _ in range(40)]
    # mul: N-form x N-form, 2^30 x 2^30 (one un-normalised sum each), 2^31 x N-form (a biased difference against a product output)
    for la, lb in ((None, None), (30, 30), (31, None)):
        A = [limbs_of(rnd.choice(vals), la, rnd) for _ in range(60)]
        B = [limbs_of(rnd.choice(vals), lb, rnd) for _ in range(60)]
        A[0] = [(1 << (la or 29)) - 1] * 8 + [(1 << 27) - 1]            # every limb at its bound
        B[0] = [(1 << (lb or 29)) - 1] * 8 + [(1 << 27) - 1]
        got = run.f29_raw(field, 0, A, B)
        for a, b, g in zip(A, B, got):
            want = model_mul(mod, [(a, b)])
            assert g == want and value(g) * RAD % mod == value(a) * value(b) % mod and value(g) < value(a) * value(b) // RAD + mod + 1
    # sqr: limbs below 2^30
    A = [limbs_of(rnd.choice(vals), 30, rnd) for _ in range(60)] + [[(1 << 30) - 1] * 8 + [(1 << 27) - 1]]
    for a, g in zip(A, run.f29_raw(field, 1, A)):
        assert g == model_mul(mod, [(a, a)])
    # mul2 as the mixed addition uses it: R (N-form) * D1 (N-form) + Y1 (N-form product output) * D2 (limbs below 2^30 + 2^29)
    top = [M29 + 8] * 8 + [(1 << 26) - 1]
    rows = [(limbs_of(rnd.choice(vals)), limbs_of(rnd.choice(vals)), limbs_of(rnd.choice(vals)), limbs_of(rnd.choice(vals), 30, rnd)) for _ in range(40)]
    rows.append((top, top, [M29] * 8 + [(1 << 23) - 1], [(1 << 30) + (1 << 29) - 1] * 8 + [(1 << 24) - 1]))
    got = run.f29_raw(field, 2, *[[r[j] for r in rows] for j in range(4)])
    for (a, b, c, d), g in zip(rows, got):
        assert g == model_mul(mod, [(a, b), (c, d)])
        assert value(g) * RAD % mod == (value(a) * value(b) + value(c) * value(d)) % mod


def check_biased_differences_and_the_carry_round(run, pyref, field):
    mod = pyref.P if field == 0 else pyref.R
    rnd = random.Random(31 + field)
    for op, K, LOG, sub_bits in ((4, 8, 30, 29), (5, 3, 30, 29), (6, 5, 31, 31)):
        kp = bias(mod, K, LOG)
        assert value(kp) == K * mod and all((1 << LOG) <= v < (1 << LOG) + (1 << 29) for v in kp[:8])
        A = [limbs_of(rnd.randrange(0, 2 * mod)) for _ in range(50)]
        # subtrahends up to the documented bound: value below (K - 1) p, limbs up to 2^LOG (a sum PPP + 2 Q for LOG = 31, an N-form value otherwise)
        B = [limbs_of(rnd.randrange(0, (K - 1) * mod), 30 if sub_bits == 29 else 31, rnd) for _ in range(50)]
        B = [[min(v, (1 << LOG)) for v in b[:8]] + [b[8]] for b in B]
        B[0] = limbs_of((K - 1) * mod - 1)
        got = run.f29_raw(field, op, A, B)
        for a, b, g in zip(A, B, got):
            assert all(0 <= x + k - y < 1 << 32 for x, k, y in zip(a, kp, b))                # limb-wise non-negative, no wrap
            assert g == [x + k - y for x, k, y in zip(a, kp, b)] and value(g) == value(a) + K * mod - value(b)
    kp = bias(mod, 3, 30)
    B = [limbs_of(rnd.randrange(0, 2 * mod)) for _ in range(20)]
    for b, g in zip(B, run.f29_raw(field, 7, B)):
        assert value(g) == 3 * mod - value(b) and all(v < (1 << 30) + (1 << 29) for v in g[:8])
    # carry: any limbs below 2^32 -> N-form, same integer
    A = [[rnd.randrange(0, 1 << 32) for _ in range(8)] + [rnd.randrange(0, 1 << 26)] for _ in range(50)] + [[(1 << 32) - 1] * 8 + [5]]
    for a, g in zip(A, run.f29_raw(field, 3, A)):
        assert value(g) == value(a) and all(v < (1 << 29) + 8 for v in g[:8])
    assert value(run.f29_raw(field, 9, [[0] * 9])[0]) == RAD % mod                            # one() = 2^261 mod p


def check_between_the_two_montgomery_forms(run, orc, pyref, field):
    mod = pyref.P if field == 0 else pyref.R
    rnd = random.Random(33 + field)
    R256 = 1 << 256
    xs = [0, 1, mod - 1, mod - 2, (1 << 253) + 5] + [rnd.randrange(0, mod) for _ in range(60)]
    ys = [mod - 1, 0, 1, mod - 2, 7] + [rnd.randrange(0, mod) for _ in range(60)]
    A, B = orc.ints_to_limbs(xs), orc.ints_to_limbs(ys)

    def go(op):
        o, o9 = run.f29_forms(field, op, A, B)
        return orc.limbs_to_ints(o), o9
    back, ent = go(0)
    assert back == xs and all(value(e) % mod == x * 32 % mod and value(e) < 2 * mod for e, x in zip(ent, xs))       # enter: x 2^256 -> x 2^261, below 2 p
    rinv = pow(R256, -1, mod)
    for op in (1, 2):
        got, _ = go(op)
        assert got == [x * y * rinv % mod for x, y in zip(xs, ys)]                                                 # the library's Montgomery product, canonical
    got, _ = go(4)
    assert got == [x * x * rinv % mod for x in xs]
    got, l9 = go(3)
    assert got == xs and all(value(l) == x and all(v <= M29 for v in l[:8]) for l, x in zip(l9, xs))               # limb conversion is exact


def check_shoup_product_with_a_precomputed_quotient(run, orc, pyref, field):
    mod = pyref.P if field == 0 else pyref.R
    rnd = random.Random(41 + field)
    ws = [0, 1, 2, mod - 1, mod - 2, (mod + 1) // 2, 1 << 253] + [rnd.randrange(0, mod) for _ in range(80)]
    W = orc.ints_to_limbs(ws)
    _, wq = run.f29_forms(field, 5, W, W)
    assert [value(l) for l in wq] == [w * RAD // mod for w in ws] and all(v <= M29 for l in wq for v in l)
    avals = [0, 1, mod - 1, mod, 3 * mod - 1, 32 * mod, 150 * mod, RAD - 1] + [rnd.randrange(0, RAD) for _ in range(40)] + [rnd.randrange(0, 8 * mod) for _ in range(40)]
    A, Wl, Wq = [], [], []
    for j in range(len(ws)):
        for loose in (None, 30, 31.58):
            a = rnd.choice(avals)
            A.append(limbs_of(a, loose, rnd)); Wl.append(limbs_of(ws[j])); Wq.append(wq[j])
    A.append([(1 << 30) - 1] * 8 + [(1 << 28) - 1]); Wl.append(limbs_of(mod - 1)); Wq.append(limbs_of((mod - 1) * RAD // mod))     # every limb at its bound (the integer is still below 2^261)
    assert value(A[-1]) < RAD
    A.append([3 * (1 << 30)] * 8 + [(1 << 26)]); Wl.append(limbs_of(mod - 1)); Wq.append(limbs_of((mod - 1) * RAD // mod))           # ... and at the bound of a biased difference
    assert value(A[-1]) < RAD
    got = run.f29_raw(field, 10, A, Wl, Wq)
    low = 0
    for a, w, q_, g in zip(A, Wl, Wq, got):
        want, q = model_shoup(mod, a, w, q_)
        va, vw = value(a), value(w)
        assert g == want and all(v <= M29 for v in g)
        assert value(g) % mod == va * vw % mod and value(g) < 3 * mod
        exact = va * value(q_) // RAD
        assert value(q) in (exact, exact - 1) and value(g) == va * vw - value(q) * mod
        low += value(q) != exact
    print("quotient one below the exact one in", low, "of", len(A))


def affine29(orc, p, xyzz16):
    x, y, zz, zzz = orc.limbs_to_ints(xyzz16.reshape(4, 4))
    if zz == 0:
        return None
    rinv = pow(1 << 256, -1, p.P)
    x, y, zz, zzz = (v * rinv % p.P for v in (x, y, zz, zzz))
    return x * pow(zz, -1, p.P) % p.P, y * pow(zzz, -1, p.P) % p.P


def bucket_chain_cases(p):
    """(points, signs, the number of steps that must take the complete path)"""
    rnd = random.Random(11)
    pts = [p.g1_mul(p.G1_GEN, rnd.randrange(1, p.R)) for _ in range(48)]
    return [(pts[:40], [rnd.randrange(2) for _ in range(40)], 1),                              # the plain chain: only the first point is "rare"
            ([pts[0], pts[0]] + pts[1:9], [0] * 10, 2),                                         # doubling at step 2
            ([pts[0], pts[1], None, pts[2], None], [0, 1, 0, 0, 0], 1),                         # identity bases are skipped
            ([pts[3], pts[4], pts[5], pts[5], pts[6]], [0, 0, 0, 1, 0], 1),                     # P5 then -P5 is not the same x as the accumulator: plain steps
            ([pts[7], pts[7], pts[8]], [0, 1, 0], 3),                                           # P - P = identity, then the chain restarts from the identity
            ([pts[9], pts[10], pts[9], pts[10], pts[11]], [0, 0, 1, 1, 0], 3)]                  # ... + P + Q - P - Q: cancellation at the last-but-one step


def chain_sum(p, seq, neg):
    want = None
    for q_, s_ in zip(seq, neg):
        want = p.g1_add(want, p.g1_neg(q_) if s_ else q_)
    return want


def check_bucket_chain_on_29_bit_limbs(run, orc, pyref):
    p = pyref
    for seq, neg, rare_want in bucket_chain_cases(p):
        a, ng = orc.g1_affine_from_ints(seq), np.array(neg, dtype=np.uint8)
        got, rare = run.xyzz29_sum(a, ng)
        canon = run.xyzz_sum(a, ng)
        want = chain_sum(p, seq, neg)
        assert affine29(orc, p, got) == want == affine29(orc, p, canon)
        assert (got == canon).all(), "coordinates differ from the canonical chain's"
        assert rare == rare_want, (rare, rare_want)


# ---- field.cuh / ec.cuh on 32-bit limbs -------------------------------------------------------------------------------------------------------------------------------
def check_field_limb_ops(run, orc, pyref):
    rnd = random.Random(2)
    for mod, pre in ((pyref.R, "fr"), (pyref.P, "fq")):
        edge = [0, 1, mod - 1, mod - 2, 1 << 253, pyref.mont_r(mod), mod >> 1]
        a = [rnd.randrange(mod) for _ in range(3000)] + edge + edge
        b = [rnd.randrange(mod) for _ in range(3000)] + edge + edge[::-1]
        A, B = orc.ints_to_limbs(a), orc.ints_to_limbs(b)
        for op in ("mul", "add", "sub"):
            assert (run.v2(f"{pre}_{op}", A, B) == getattr(orc, f"{pre}_{op}")(A, B)).all(), (pre, op)
    A = orc.ints_to_limbs([rnd.randrange(pyref.R) for _ in range(16)] + [0])
    assert (run.v1("fr_inv", A) == orc.fr_inv(A)).all()
    assert (run.v1("fr_neg", A) == orc.fr_sub(np.zeros_like(A), A)).all()


def check_fused_two_product_reduction(run, orc, pyref):
    rnd = random.Random(9)
    P_ = pyref.P
    edge = [0, 1, P_ - 1, P_ - 2, P_ >> 1]
    vals = [[rnd.randrange(P_) for _ in range(500)] + edge for _ in range(4)]
    vals[1] = vals[1][:500] + edge[::-1]
    A, B, C_, D = (orc.ints_to_limbs(v) for v in vals)
    assert (run.mul2_sub(A, B, C_, D) == orc.fq_sub(orc.fq_mul(A, B), orc.fq_mul(C_, D))).all()


def xyzz_to_affine(orc, pyref, x):
    X, Y, ZZ, ZZZ = orc.fq_to_ints(np.asarray(x).reshape(4, 4))
    if ZZ == 0:
        return None
    return (X * pow(ZZ, -1, pyref.P) % pyref.P, Y * pow(ZZZ, -1, pyref.P) % pyref.P)


def group_law_sequences(p):
    """the chain of the group-law check — doubling first, identity base, repeats — and P + (-P)"""
    rnd = random.Random(6)
    pts = [p.g1_mul(p.G1_GEN, rnd.randrange(1, p.R)) for _ in range(24)]
    seq = [pts[0], pts[0]] + pts[1:] + [None, pts[3], pts[2]]
    neg = [0, 0] + [rnd.randrange(2) for _ in pts[1:]] + [0, 1, 0]
    return pts, [(seq, neg), ([pts[5], pts[5]], [0, 1])]


def check_xyzz_group_law_including_special_cases(run, orc, pyref):
    p = pyref
    pts, ((seq, neg), (two, two_neg)) = group_law_sequences(p)
    out = run.xyzz_sum(orc.g1_affine_from_ints(seq), np.array(neg, dtype=np.uint8))
    want = chain_sum(p, seq, neg)
    assert xyzz_to_affine(orc, p, out) == want
    # P + (-P) = identity through the mixed-add path
    o2 = run.xyzz_sum(orc.g1_affine_from_ints(two), np.array(two_neg, dtype=np.uint8))
    assert xyzz_to_affine(orc, p, o2) is None
    # full add: doubling branch, identity operands
    o3 = run.xyzz_add(out, out)
    assert xyzz_to_affine(orc, p, o3) == p.g1_add(want, want)
    o4 = run.xyzz_add(o3, o2)
    assert xyzz_to_affine(orc, p, o4) == p.g1_add(want, want)
    o5 = run.xyzz_dbl(out)
    assert xyzz_to_affine(orc, p, o5) == p.g1_add(want, want)


def check_redundant_range_arithmetic_on_the_range_boundaries(run, orc, pyref):
    q, rnd = pyref.P, random.Random(11)
    Rinv = pow(1 << 256, -1, q)
    lim = lambda xs: orc.ints_to_limbs(xs)
    ints = lambda arr: orc.limbs_to_ints(arr)

    def go(op, a, b=None, c=None, d=None):
        A = lim(a)
        B, C_, D = (lim(x) if x is not None else A for x in (b, c, d))
        return ints(run.fq_lazy(op, A, B, C_, D))
    e2 = [0, 1, q - 1, q, q + 1, 2 * q - 1]                           # [0, 2q)
    e4 = e2 + [2 * q, 2 * q + 1, 3 * q, 4 * q - 1]                    # [0, 4q)
    r2 = e2 + [rnd.randrange(2 * q) for _ in range(400)]
    r4 = e4 + [rnd.randrange(4 * q) for _ in range(400)]
    canon = [0, 1, q - 1] + [rnd.randrange(q) for _ in range(len(r4) - 3)]
    pairs2 = [(a, b) for a in e2 for b in e2] + [(rnd.randrange(2 * q), rnd.randrange(2 * q)) for _ in range(300)]
    a2, b2 = [p_[0] for p_ in pairs2], [p_[1] for p_ in pairs2]
    for got, a, b in zip(go(0, r4, canon), r4, canon):                # mul_lazy: [0, 4q) x [0, q) -> [0, 2q)
        assert got < 2 * q and got % q == a * b * Rinv % q
    for got, a, b in zip(go(0, a2, b2), a2, b2):                      # ... and [0, 2q) x [0, 2q) -> [0, 2q) (the accumulate chain)
        assert got < 2 * q and got % q == a * b * Rinv % q
    for got, a in zip(go(1, r2), r2):
        assert got < 2 * q and got % q == a * a * Rinv % q
    for got, a, b in zip(go(2, a2, b2), a2, b2):
        assert got < 2 * q and got % q == (a - b) % q
    for got, a in zip(go(3, r2), r2):
        assert got < 2 * q and got % q == 2 * a % q
    for got, a in zip(go(4, r2), r2):
        assert got <= 2 * q and got % q == -a % q
    top = [2 * q] * 8 + [rnd.randrange(2 * q + 1) for _ in range(300)]   # mul2_add_2p takes the closed range [0, 2q]
    aa, bb, cc, dd = ([rnd.choice(top) for _ in range(400)] for _ in range(4))
    aa[0] = bb[0] = cc[0] = dd[0] = 2 * q
    for got, a, b, c, d in zip(go(5, aa, bb, cc, dd), aa, bb, cc, dd):
        assert got < 2 * q and got % q == (a * b + c * d) * Rinv % q
    for got, a in zip(go(6, r4), r4):
        assert got < 2 * q and got % q == a % q
    for got, a, b in zip(go(7, a2, b2), a2, b2):
        assert got < 4 * q and got == a + b
    for got, a, b in zip(go(8, a2, b2), a2, b2):
        assert 0 < got < 4 * q and got == a + 2 * q - b
    for got, a in zip(go(9, r4), r4):
        assert got == a % q
    for got, a in zip(go(10, r2), r2):
        assert got == (1 if a % q == 0 else 0)
    for got, a, b in zip(go(11, r4, canon), r4, canon):               # the full product accepts a redundant left operand (ntt_post)
        assert got == a * b * Rinv % q
    # mul_shoup_lazy (the final NTT pass's twiddle products): a * w mod p, no Montgomery factor, for ANY a below 2^256 (the butterflies hand it [0, 4p)) and canonical w
    # with wq = floor(w 2^256 / p); result in [0, 2p).  Both fields; the edges of a's range and w in {0, 1, p - 1, ...} included.
    for op, mod in ((12, pyref.P), (13, pyref.R)):
        ws = [0, 1, 2, mod - 1, mod - 2, (mod + 1) // 2] + [rnd.randrange(mod) for _ in range(300)]
        As = [0, 1, mod - 1, mod, 2 * mod - 1, 2 * mod, 4 * mod - 1, (1 << 256) - 1] + [rnd.randrange(4 * mod) for _ in range(200)] + [rnd.randrange(1 << 256) for _ in range(98)]
        wqs = [w * (1 << 256) // mod for w in ws]
        assert go(op + 2, [w * (1 << 256) % mod for w in ws]) == wqs                                # shoup_quotient: from w's library form, exact
        for got, a, w in zip(go(op, As, ws, wqs), As, ws):
            assert got < 2 * mod and got % mod == a * w % mod, (op, a, w)


def lazy_chain_sequences(p):
    """the chain of the lazy check — doubling first, identity base, repeats, P then P again late in the chain — and ... + P + Q - P - Q"""
    rnd = random.Random(8)
    pts = [p.g1_mul(p.G1_GEN, rnd.randrange(1, p.R)) for _ in range(40)]
    seq = [pts[0], pts[0]] + pts[1:] + [None, pts[3], pts[2], pts[7], pts[7]]
    neg = [0, 0] + [rnd.randrange(2) for _ in pts[1:]] + [0, 1, 0, 0, 1]
    return pts, [(seq, neg), ([pts[5], pts[9], pts[5], pts[9]], [0, 0, 1, 1])]


def check_lazy_mixed_addition_chain_equals_the_canonical_one(run, orc, pyref):
    p = pyref
    pts, ((seq, neg), (two, two_neg)) = lazy_chain_sequences(p)
    arr_, ng = orc.g1_affine_from_ints(seq), np.array(neg, dtype=np.uint8)
    lazy = run.xyzz_sum_lazy(arr_, ng)
    canon = run.xyzz_sum(arr_, ng)
    want = chain_sum(p, seq, neg)
    assert xyzz_to_affine(orc, p, lazy) == xyzz_to_affine(orc, p, canon) == want
    assert all(v < p.P for v in orc.limbs_to_ints(lazy.reshape(4, 4)))             # normalised coordinates
    # the full addition in the lazy range: a + b + b, a + a + a (doubling branch first), identity operands
    other = run.xyzz_sum(orc.g1_affine_from_ints(pts[20:30]), np.zeros(10, dtype=np.uint8))
    w2 = chain_sum(p, pts[20:30], [0] * 10)
    o3 = run.xyzz_add_lazy(canon, other)
    assert xyzz_to_affine(orc, p, o3) == p.g1_add(p.g1_add(want, w2), w2)
    o4 = run.xyzz_add_lazy(canon, canon)
    assert xyzz_to_affine(orc, p, o4) == p.g1_add(p.g1_add(want, want), want)
    ident = np.zeros(16, dtype=np.uint64)
    o4 = run.xyzz_add_lazy(ident, other)
    assert xyzz_to_affine(orc, p, o4) == p.g1_add(w2, w2)
    o2 = run.xyzz_sum_lazy(orc.g1_affine_from_ints(two), np.array(two_neg, dtype=np.uint8))   # ... + P + Q - P - Q = identity through the lazy path
    assert xyzz_to_affine(orc, p, o2) is None


def filter_chain_inputs(orc, pyref, rnd, length):
    """one chain of the filter probe: start = [a] G, the steps alternate [d] G and [e] G, so the accumulator before step 2m is [a + m (d + e)] G and before step
    2m + 1 it is [a + d + m (d + e)] G — two arithmetic progressions of the oracle.  Returns the probe's inputs and the affine end point the oracle expects."""
    R = pyref.R
    a, d, e = (rnd.randrange(1, R) for _ in range(3))
    G = orc.g1_generator()
    aff = lambda k: orc.g1_to_affine(orc.g1_mul(G, orc.fr_from_ints([k % R])[0]))[0]
    start, steps = aff(a), np.ascontiguousarray(np.stack([aff(d), aff(e)]))
    half = (length + 1) // 2
    prefix = np.empty((2 * half, 8), dtype=np.uint64)
    prefix[0::2] = orc.gen_bases_arith(a, (d + e) % R, half)
    prefix[1::2] = orc.gen_bases_arith((a + d) % R, (d + e) % R, half)
    assert (prefix[0] == start).all()
    # the precondition, on the inputs: no step shares its x with the accumulator it meets (then every refusal of a step is a false alarm)
    assert not (prefix[:length, :4] == steps[np.arange(length) % 2, :4]).all(axis=1).any()
    end = (a + (length // 2) * (d + e) + (d if length % 2 else 0)) % R
    return (start, steps, np.ascontiguousarray(prefix), length), orc.g1_affine_to_ints(aff(end))[0]


def check_fast_chain_filter_refuses_every_same_x_addition(run, orc, pyref):
    rnd = random.Random(29)
    inputs, ends, steps = [], [], 0
    for i in range(600):
        length = 1 + (i * 37) % 128 if i >= 8 else (1, 2, 3, 127, 128, 64, 5, 96)[i]
        inp, end = filter_chain_inputs(orc, pyref, rnd, length)
        inputs.append(inp)
        ends.append(end)
        steps += length
    totals = [0, 0, 0, 0]
    for (counts, out), end in zip(run.filter_probe(inputs, check=1), ends):
        assert xyzz_to_affine(orc, pyref, out) == end
        totals = [t + c for t, c in zip(totals, counts)]
    print("xyzz29_madd_fast: %d same-x probes, %d passed the filter; %d distinct-x additions, %d false alarms" % (2 * steps, totals[0], steps, totals[2]))
    assert totals[0] == 0, "same-x additions went through the incomplete formulas"
    assert totals[1] == 0, "a refused step changed the accumulator"
    assert totals[3] == 0, "the 29-bit chain differs from the canonical one"


# ---- chains of different lengths side by side ------------------------------------------------------------------------------------------------------------------------
def divergent_chains(p):
    """135 chains for ONE launch (two full waves and a partial one): the planted sequences of the checks above — doublings, identity bases, cancellations, restarts — and
    random chains of 1 .. 128 points drawn (with repeats, random signs, now and then the identity) from the same points.  -> [(points, signs)]"""
    cases = [(seq, neg) for seq, neg, _ in bucket_chain_cases(p)]
    pool = [q for q in cases[0][0]]
    for gen in (group_law_sequences, lazy_chain_sequences):
        pts, seqs = gen(p)
        cases += seqs
        pool += pts
    rnd = random.Random(131)
    lengths = [1, 128, 2, 127, 64, 65] + [rnd.randrange(1, 129) for _ in range(119)]
    for n in lengths:
        seq = [None if rnd.randrange(40) == 0 else rnd.choice(pool) for _ in range(n)]
        neg = [rnd.randrange(2) for _ in range(n)]
        if n >= 4 and rnd.randrange(4) == 0:                     # a doubling or a cancellation somewhere inside: the next point is the accumulator's own, with either sign
            k = rnd.randrange(1, n - 1)
            acc = chain_sum(p, seq[:k], neg[:k])
            seq[k] = acc if acc is not None else seq[k]
        cases.append((seq, neg))
    order = list(range(len(cases)))
    rnd.shuffle(order)                                           # planted and random chains side by side in every wave
    return [cases[i] for i in order]


def expected_rare(p, seq, neg):
    """the steps of a chain that must take the complete path: the first point after the identity, and every point that shares its x with the accumulator"""
    acc, rare = None, 0
    for q_, s_ in zip(seq, neg):
        if q_ is None:
            continue
        q_ = p.g1_neg(q_) if s_ else q_
        rare += acc is None or acc[0] == q_[0]
        acc = p.g1_add(acc, q_)
    return rare


def check_divergent_chains_in_one_launch(run, orc, pyref):
    p = pyref
    cases = divergent_chains(p)
    assert len(cases) >= 130 and len(cases) % 64 != 0
    for seq, neg, rare_want in bucket_chain_cases(p):
        assert expected_rare(p, seq, neg) == rare_want
    seqs = [(orc.g1_affine_from_ints(seq), np.array(neg, dtype=np.uint8)) for seq, neg in cases]
    canon, lazy, on29 = run.chains("xyzz_sum", seqs), run.chains("xyzz_sum_lazy", seqs), run.chains("xyzz29_sum", seqs)
    planted = 0
    for i, (seq, neg) in enumerate(cases):
        want = chain_sum(p, seq, neg)
        assert xyzz_to_affine(orc, p, canon[i]) == want, ("xyzz_sum", i)
        assert xyzz_to_affine(orc, p, lazy[i]) == want, ("xyzz_sum_lazy", i)
        assert all(v < p.P for v in orc.limbs_to_ints(lazy[i].reshape(4, 4))), ("xyzz_sum_lazy: not normalised", i)
        got, rare = on29[i]
        assert affine29(orc, p, got) == want, ("xyzz29_sum", i)
        assert (got == canon[i]).all(), ("xyzz29_sum: coordinates differ from the canonical chain's", i)
        want_rare = expected_rare(p, seq, neg)
        assert rare == want_rare, ("xyzz29_sum: n_rare", i, rare, want_rare)
        planted += want_rare > 1
    assert planted >= 20                                         # the launch really mixes plain chains with ones that leave the fast path
