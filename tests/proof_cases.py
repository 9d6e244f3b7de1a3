"""TEST INFRASTRUCTURE ONLY — planted random draws and structured witnesses for whole proofs (tests/test_structured_proofs.py), and their reference.

Every other proof of the suite is made from a uniform witness and a `np.random.default_rng(seed)` stream: no committed column is zero, constant or a long run, no blinding
row is 0 or r - 1, no commitment is the identity and the rejection sampler never sees a draw that shares r's top limb.  The cases here feed the provers — the native one
(csrc/prover.hip), its Python twin (plonk/prover.py + shplonk.py) — exactly such input, and the reference is the independent CPU prover (oracle/prover.py: Python integers)
driven by an EQUAL stream.

PlantedRng is a duck-typed stand-in for the generator: `integers(0, 2^64, (rows, 4), uint64)` is all fields.rand_fr_array and oracle/prover.py:rand_fr ask of an rng
(fields.OsRng offers no more).  Two kinds of plan:
  cyclic pattern    raw 254-bit values served row after row, None = a seeded raw row (BOUNDARY: the values around r, limb by limb; values >= r are rejected by the samplers
                    and the rows that replace them come from the stream too, so a run of rejected rows makes the redraw loop go round several times)
  item-addressed    every planted value is below r and every seeded row is too (rejected here, with Python integers), so nothing is rejected by the samplers and row i of the
                    stream is draw i of the proof's draw plan (plonk.prover.draw_plan; draw_items() below for several circuits): {(purpose, index): fill} plants whole items.
                    `served` must end at the plan's total — assert_exhausted() — so the address arithmetic cannot drift unnoticed.
Fills: "zeros", "minus_one" (the raw limbs r - 1), ("const", v), ("delta_first", v), ("delta_last", v): v raw limbs below r, i.e. the Montgomery form of v / 2^256.
"""
import random

import numpy as np

from zk_dcap_verifier_amd.fields import R_MOD, fr_int_array, fr_mont_array
from zk_dcap_verifier_amd.plonk import ADVICE, FIXED, INSTANCE
from zk_dcap_verifier_amd.plonk.prover import draw_plan

R = R_MOD
_M64 = (1 << 64) - 1
_TOP = R >> 192                                                        # r's top limb


def _limbs(v):
    return [(v >> (64 * i)) & _M64 for i in range(4)]


# r - 1, r, r + 1, 0, 1, 2^254 - 1; r's top limb over lower limbs just below / just above r's (one off in limb 2, in limb 1, all zero, all ones); r's top three limbs
# over a limb 0 of 0 / one less / one more / all ones; the top limb one below and one above r's.  The nine values at or above r stand in a row: a batch of bf + 1 rows
# that falls into the run is rejected whole, and part of what replaces it is rejected again.  23 entries: coprime to every batch size a proof draws (1, bf, bf + 1, n).
BOUNDARY = [R - 1, None, 0, 1, R - (1 << 128), R - (1 << 64), _TOP << 192,
            R, R + 1, (1 << 254) - 1, R + (1 << 128), R + (1 << 64), R + 2, R | _M64, (_TOP << 192) | ((1 << 192) - 1), R + (1 << 192),
            None, R - (R & _M64), R - 2, R - (1 << 192), None, R - 3, None]
assert all(v is None or 0 <= v < (1 << 254) for v in BOUNDARY)        # the samplers mask the top limb to 62 bits: a larger value would be another value after the mask


class PlantedRng:
    def __init__(self, seed, pattern=None, rows=None, total=None):
        """pattern: the cyclic plan; rows: {stream row: raw value < r} of an item-addressed plan (for_items builds it), total: the rows that plan must serve"""
        assert (pattern is None) != (rows is None)
        self.gen = np.random.default_rng(seed)
        self.pattern, self.rows, self.total = pattern, rows, total
        self.served = 0                                                # rows handed out
        self.planted_rejected = 0                                      # planted rows at or above r among them
        self.calls = []                                                # the batch sizes asked for, in order

    @classmethod
    def for_items(cls, seed, items, fills):
        """items: [(purpose, index, count)] in stream order (draw_items); fills: {(purpose, index): fill}"""
        rows, at, known = {}, 0, {(p, i) for p, i, _ in items}
        assert set(fills) <= known, sorted(set(fills) - known)
        for purpose, index, count in items:
            fill = fills.get((purpose, index))
            if fill is not None:
                for j, v in enumerate(fill_values(fill, count)):
                    assert 0 <= v < R
                    rows[at + j] = v
            at += count
        return cls(seed, rows=rows, total=at)

    def _seeded_below_r(self):
        while True:
            a = self.gen.integers(0, 1 << 64, size=4, dtype=np.uint64)
            v = sum(int(a[j]) << (64 * j) for j in range(4)) & ((1 << 254) - 1)
            if v < R:
                return v

    def integers(self, low, high, size, dtype=np.uint64):
        assert low == 0 and high == 1 << 64 and dtype == np.uint64
        n, four = size
        assert four == 4
        self.calls.append(int(n))
        if self.pattern is not None:
            out = self.gen.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)      # (the seeded rows keep their top bits: the samplers' mask is part of what is compared)
            for i in range(n):
                v = self.pattern[(self.served + i) % len(self.pattern)]
                if v is not None:
                    out[i] = _limbs(v)
                    self.planted_rejected += v >= R
        else:
            out = np.empty((n, 4), dtype=np.uint64)
            for i in range(n):
                v = self.rows.get(self.served + i)
                out[i] = _limbs(v if v is not None else self._seeded_below_r())
        self.served += int(n)
        return out

    def assert_exhausted(self):
        assert self.pattern is None and self.served == self.total, ("the proof drew", self.served, "rows, its draw plan holds", self.total)


def fill_values(fill, count):
    """the raw limb values (below r) of one planted item of `count` rows"""
    if fill == "zeros":
        return [0] * count
    if fill == "minus_one":
        return [R - 1] * count
    kind, v = fill
    v %= R
    if kind == "const":
        return [v] * count
    if kind == "delta_first":
        return [v] + [0] * (count - 1)
    if kind == "delta_last":
        return [0] * (count - 1) + [v]
    raise ValueError(fill)


def n_sets(cs):
    chunk = cs.permutation_chunk_len()
    return -(-len(cs.permutation_columns) // chunk) if cs.permutation_columns else 0


def draw_items(cs, k, m=1):
    """[(purpose, index, count)] in the order a proof over m circuits of this key consumes the caller's rng.  m = 1: plonk.prover.draw_plan itself, the Blinds numbered in
    their order of appearance ("blind", 0), ("blind", 1), ..  m > 1 (the native prover only; include/zkmi355.h zk_rng_fn, csrc/prover.hip validate_and_plan): every
    per-circuit block of draw_plan once per circuit, circuit by circuit, and the vanishing argument once; circuit c's item i of a purpose has index c * (items per circuit) + i."""
    n, bf, A, L, S = 1 << k, cs.blinding_factors(), cs.num_advice_columns, len(cs.lookups), n_sets(cs)
    if m == 1:
        raw = [(p, i, c) for p, i, c, _ in draw_plan(A, L, S, cs.degree() - 1, n, bf)]
    else:
        raw = []
        for c in range(m):
            raw += [("advice", c * A + i, bf + 1) for i in range(A)] + [("blind", None, 1)] * A
        for cl in range(m * L):
            raw += [("bi", cl, bf + 1), ("bt", cl, bf + 1), ("blind", None, 1), ("blind", None, 1)]
        for cs_ in range(m * S):
            raw += [("perm_blind", cs_, bf), ("blind", None, 1)]
        for cl in range(m * L):
            raw += [("lookup_blind", cl, bf), ("blind", None, 1)]
        raw += [("random_poly", 0, n), ("blind", None, 1)] + [("blind", None, 1)] * (cs.degree() - 1)
    out, b = [], 0
    for p, i, c in raw:
        if p == "blind":
            i, b = b, b + 1
        out.append((p, i, c))
    return out


def every(cs, k, purpose, fill, m=1):
    """the fills dict that plants `fill` into every item of one purpose"""
    return {(p, i): fill for p, i, _ in draw_items(cs, k, m) if p == purpose}


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------------------
_PARAMS, _KEYS = {}, {}


def _ints(col):
    import oracle as orc
    return orc.fr_to_ints(col) if isinstance(col, np.ndarray) else [int(v) for v in col]


def oracle_keys(k, tau, cs, fixed, asm, key):
    """oracle/prover.py's Params (per k) and Keys (per `key`, the caller's name of the circuit), made once"""
    import prover as op
    if (k, tau) not in _PARAMS:
        _PARAMS[k, tau] = op.Params(k, tau)
    if key not in _KEYS:
        _KEYS[key] = op.keygen(_PARAMS[k, tau], cs, [_ints(c) for c in fixed], asm.copies)
    return _PARAMS[k, tau], _KEYS[key]


def oracle_proof(k, tau, cs, fixed, asm, advice, instances, rng, key, require_satisfied=False):
    """the independent CPU prover's bytes for this circuit, witness and rng (random_circuits.oracle_proof with the caller's generator and cached keys)"""
    import prover as op
    params, keys = oracle_keys(k, tau, cs, fixed, asm, key)
    return op.create_proof(params, keys, [_ints(c) for c in advice], instances, rng, require_satisfied=require_satisfied)


def first_difference(got, want):
    """the first differing 32-byte word of two proofs, or their lengths"""
    if len(got) != len(want):
        return ("lengths", len(got), len(want))
    return next((i // 32 for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]), None)


# ---- structured witnesses on random_circuits.random_circuit ---------------------------------------------------------------------------------------------------
def _columns_in(exprs, kind):
    """the columns of one kind ("advice", "fixed", "instance") an expression list reads, in first-use order"""
    from zk_dcap_verifier_amd.plonk import expression as ex
    q = {}
    for e in exprs:
        ex.queries(e, q)
    return list(dict.fromkeys(c for t, c, _ in q if t == kind))


def advice_columns_in(exprs):
    return _columns_in(exprs, "advice")


def fixed_columns_in(exprs):
    return _columns_in(exprs, "fixed")


def lookup_layout(cs):
    """per lookup of a random_circuit: (input advice columns, table fixed columns) pair by pair — its inputs are Advice(a) or selector * Advice(a), its tables Fixed(t)"""
    out = []
    for lk in cs.lookups:
        ins = [advice_columns_in([e]) for e in lk.input_expressions]
        tabs = [fixed_columns_in([e]) for e in lk.table_expressions]
        assert all(len(i) == 1 for i in ins) and all(len(t) == 1 for t in tabs)
        out.append(([i[0] for i in ins], [t[0] for t in tabs]))
    return out


def free_advice(cs):
    """the advice columns that feed no lookup"""
    fed = {a for ins, _ in lookup_layout(cs) for a in ins}
    return [c for c in range(cs.num_advice_columns) if c not in fed]


ADVICE_KINDS = ("zeros", "const", "minus_one", "selector", "mixed")
_MIX = ("zeros", "const", "minus_one", "selector", "ones", "delta_last", "alt_pm", "top")     # "mixed": column i of the free ones takes kind i of these (parity_cases.STRUCTURED_KINDS)


def structured_advice(orc, pyref, cs, k, advice, kind, seed=0):
    """the witness with every advice column that feeds no lookup replaced by a parity_cases.structured_fr column of `kind` ("mixed": another kind per column)"""
    import parity_cases as pc
    out = [a.copy() for a in advice]
    for j, c in enumerate(free_advice(cs)):
        out[c] = pc.structured_fr(orc, pyref, 1 << k, _MIX[j % len(_MIX)] if kind == "mixed" else kind, seed + c)
    return out


LOOKUP_KINDS = ("zero_row", "one_row", "table")


def structured_lookup_inputs(cs, k, fixed, advice, kind):
    """the witness with the input columns of every lookup taken from its table: every row the table's row 0 (the zero tuple), every row one non-zero table row, or row i the
    table's row i on the usable rows (then the zero tuple).  All legal: the inputs are tuples of the table on every row, whatever the lookup's selector does."""
    n, u = 1 << k, cs.usable_rows(k)
    out = [a.copy() for a in advice]
    for ins, tabs in lookup_layout(cs):
        assert not any(fixed[t][0] for t in tabs), "row 0 of a random_circuit table is the zero tuple"
        if kind == "zero_row":
            rows = [0] * n
        elif kind == "one_row":
            j = next(i for i in range(u) if any(fixed[t][i] for t in tabs))
            rows = [j] * n
        else:
            rows = [i if i < u else 0 for i in range(n)]
        for a, t in zip(ins, tabs):
            out[a] = fr_mont_array([fixed[t][i] for i in rows])
    return out


def gates_off(k, seed):
    """random_circuits.random_circuit(k, seed) made SATISFIED without touching its shape: the leading fixed factor of every gate is 0 on all rows (every gate column of
    the fixed part is zeroed), all cells of an equality class hold one value, lookup inputs stay tuples of their table.  The lookup and permutation arguments run as ever.
    A class that holds a fixed cell takes that cell's value (0: the equality-enabled fixed column is a gate column); a row of a lookup's inputs of which one cell is copied
    becomes the zero tuple and its classes take 0; every other class takes one seeded non-zero value.  Instance columns are as long as their copied cells need."""
    import random_circuits as rc
    cs, fixed, asm, advice, instances = rc.random_circuit(k, seed)
    n, u = 1 << k, cs.usable_rows(k)
    rnd = random.Random(seed * 31 + 5)
    gate_fixed = {c for g in cs.gates for c in fixed_columns_in([g])}
    table_or_selector = {c for lk in cs.lookups for c in fixed_columns_in(list(lk.input_expressions) + list(lk.table_expressions))}
    assert not gate_fixed & table_or_selector
    fixed = [[0] * n if c in gate_fixed else list(col) for c, col in enumerate(fixed)]
    adv = [fr_int_array(a) for a in advice]
    inst = [list(c) for c in instances]
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for left, right in asm.copies:
        parent[find(tuple(left))] = find(tuple(right))
    zero = {find(c) for c in list(parent) if c[0] == FIXED}
    for c in list(parent):
        assert c[0] != FIXED or fixed[c[1]][c[2]] == 0
    zero_rows = set()                                                  # (lookup, row): the input tuple of that row becomes the zero tuple
    layout = lookup_layout(cs)
    changed = True
    while changed:
        changed = False
        for l, (ins, _) in enumerate(layout):
            for i in range(n):
                cells = [(ADVICE, a, i) for a in ins]
                if (l, i) not in zero_rows and any(c in parent for c in cells):
                    zero_rows.add((l, i))
                    changed = True
                if (l, i) in zero_rows:
                    for c in cells:
                        if c in parent and find(c) not in zero:
                            zero.add(find(c))
                            changed = True
    for l, i in zero_rows:
        for a in layout[l][0]:
            adv[a][i] = 0
    value = {}
    for c in sorted(parent):
        root = find(c)
        v = 0 if root in zero else value.setdefault(root, rnd.randrange(1, R))
        t, col, row = c
        if t == ADVICE:
            adv[col][row] = v
        elif t == INSTANCE:
            inst[col] += [rnd.randrange(R) for _ in range(row + 1 - len(inst[col]))]
            inst[col][row] = v
    for t, col, row in sorted(parent):                                 # (an instance cell written before its column grew past it keeps its class's value)
        if t == INSTANCE:
            root = find((t, col, row))
            inst[col][row] = 0 if root in zero else value[root]
    assert all(len(c) <= u for c in inst)
    return cs, fixed, asm, [fr_mont_array(c) for c in adv], inst


# ---- the native entry points, called bare: what a refusal leaves behind ------------------------------------------------------------------------------------------
SENTINEL = 0xA5


class RawCall:
    """zk_plonk_create_proof (m = 0) or zk_plonk_create_proof_multi (m circuits, advice and instances flattened circuit-major) on host columns with an output buffer
    full of SENTINEL and *proof_len preset: .rc, .out, .len, .error (zk_last_error right after the call), and .draw_calls — the rng callback's calls so far; the callback
    stays alive with this object, so a late call would be counted, not crash."""

    LEN_BEFORE = 0x5EED

    def __init__(self, be, native, advice, instances, rng, m=0, cap=None):
        import ctypes as C
        from zk_dcap_verifier_amd.fields import rand_fr_array
        from zk_dcap_verifier_amd.plonk.native import RNG_FN
        self.draw_calls, self.errors = 0, []

        def draw(_user, count, out):
            try:
                self.draw_calls += 1
                a = rand_fr_array(rng, int(count))
                C.memmove(out, a.ctypes.data, a.nbytes)
            except BaseException as e:                                  # never let an exception cross the FFI
                self.errors.append(e)
        self._cb = RNG_FN(draw)
        self._keep = [np.ascontiguousarray(a, dtype=np.uint64) for a in advice]
        adv = (C.c_void_p * max(1, len(advice)))(*[a.ctypes.data for a in self._keep])
        inst = [np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in col) or bytes(32), dtype=np.uint8).copy() for col in instances]
        inst_ptrs = (C.c_void_p * max(1, len(inst)))(*[a.ctypes.data for a in inst])
        lens = (C.c_uint32 * max(1, len(inst)))(*[len(col) for col in instances])
        cap = native.proof_cap_for(max(m, 1)) if cap is None else cap
        self.out = np.full(cap, SENTINEL, dtype=np.uint8)
        ln = C.c_size_t(self.LEN_BEFORE)
        if m == 0:
            self.rc = be.lib.zk_plonk_create_proof(be.ctx, C.byref(native.desc), adv, C.c_int(0), inst_ptrs, lens, self._cb, None, self.out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(ln))
        else:
            self.rc = be.lib.zk_plonk_create_proof_multi(be.ctx, C.byref(native.desc), C.c_uint32(m), adv, C.c_int(0), inst_ptrs, lens, self._cb, None,
                                                         self.out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(ln))
        self.error = (be.lib.zk_last_error(be.ctx) or b"").decode()
        self.len = ln.value
        self.draw_calls_at_return = self.draw_calls
        assert not self.errors, self.errors

    @property
    def proof(self):
        assert self.rc == 0, (self.rc, self.error)
        return self.out[: self.len].tobytes()

    def untouched(self):
        return self.len == self.LEN_BEFORE and bool((self.out == SENTINEL).all())
