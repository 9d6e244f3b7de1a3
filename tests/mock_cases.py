"""TEST INFRASTRUCTURE ONLY — satisfiable circuits with PLANTED, sparse violations for the MockProver on the device (zk_mock_prover_verify, csrc/mockprover.hip; the
row-list mode of quotient_rows_kernel), and a predictor of the records they must give (tests/test_structured_mock.py).

build() lays out a circuit that holds BY CONSTRUCTION on all 2^k rows (the blinding rows and the wrap included), so that every record of a later check comes from a
cell a test changed on purpose:

  gates    polynomial g = q_g * (T0 + T1 * T2 - T3): T3 is gate g's own advice column d_g and q_g its own fixed column (one polynomial can be broken alone);
           T0 / T1 read the shared advice columns x / y at rotations that cycle with g — gate 0 always carries -1 (on x) and +ROT, the largest rotation (on y) —
           T2 is the shared advice column z, in the last gate the instance column.  x, y, z are non-zero on every row, the blinding rows too.
  lookups  one to three fixed table columns whose stored words the case gives (raw limbs: what the sort compares), one advice column per input expression,
           optionally switched by a selector (q * a); every row reads a table row < u unless planted otherwise.
  copies   explicit cycles over `extra` advice columns no gate or lookup reads, one fixed column and the instance column; the successor planes of the Assembly are
           written from the cycles as listed, so the records' other_column / other_row are known here.

Case.put / bump change cells and log them; Case.predict() gives the records as MockFailure tuples in the header's order — gates by (row, index), lookups by
(index, row), copies by (index, row).  The predictor is the reference: Python integers on the cells a change can reach (gates: the rows whose queries read a changed
cell; copies: the listed cycles; lookups: every row < u against the set of the table's rows < u).  It never calls the library and never evaluates an Expression; it is
itself checked against plonk.dev.MockProver at k <= 7 by a CPU test.  Columns are built with numpy and the oracle's conversions."""
import numpy as np

import oracle as orc
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.fields import R_MOD
from zk_dcap_verifier_amd.plonk import ADVICE, FIXED, INSTANCE, Advice, Fixed, Instance
from zk_dcap_verifier_amd.plonk.dev import MockFailure

ROT = 2                                              # the largest positive rotation of a gate
R_INV = pow(1 << 256, -1, R_MOD)
MONT_ONE = (1 << 256) % R_MOD
TILE = 2048                                          # MP_TILE of mockprover.hip
X, Y, Z, D0 = 0, 1, 2, 3                             # advice columns: the shared operands, then d_g
ROTS = ((-1, ROT), (0, 0), (ROT, -1))                # (rotation of x, rotation of y) of gate g, by g % 3


def mont(vals):
    """small non-negative integers (numpy, < 2^64) -> (n, 4) Montgomery limbs"""
    a = np.zeros((len(vals), 4), dtype=np.uint64)
    a[:, 0] = vals
    return orc.fr_to_mont(a)


def words(vals):
    """Python integers < 2^256 -> the limbs themselves (stored words, whatever value they stand for)"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def word_of(arr, row):
    return int.from_bytes(np.ascontiguousarray(arr[row]).tobytes(), "little")


def kinds(records):
    return tuple(sum(1 for f in records if f.kind == kd) for kd in ("gate", "lookup", "copy"))


def strings(records):
    """MockProver.verify()'s strings of the records"""
    out = []
    for f in records:
        if f.kind == "gate":
            out.append(f"gate {f.index} not satisfied on row {f.row}")
        elif f.kind == "lookup":
            out.append(f"lookup {f.index}: input of row {f.row} is not in the table")
        else:
            out.append(f"copy constraint violated: column {f.index} row {f.row} != column {f.other_column} row {f.other_row}")
    return out


class Case:
    """unpacks as (cs, fixed, asm, advice, instances)"""

    def __init__(self, k, cs, fixed, asm, advice, instances, gates, lookups, cycles, perm, extra0, fixed_copy):
        self.k, self.n, self.u = k, 1 << k, cs.usable_rows(k)
        self.cs, self.fixed, self.asm, self.advice, self.instances = cs, fixed, asm, advice, instances
        self.gates, self.lookups, self.cycles, self.perm = gates, lookups, cycles, perm
        self.extra0, self.fixed_copy = extra0, fixed_copy
        self.changed = set()
        self.readers = {}                            # (kind, column) -> [(gate, rotation)]
        for g, terms in enumerate(gates):
            for (kind, col, rot) in terms:
                self.readers.setdefault((kind, col), []).append((g, rot))

    def __iter__(self):
        return iter((self.cs, self.fixed, self.asm, self.advice, self.instances))

    # ---- cells ----------------------------------------------------------------------------------------------------------------------------------------------
    def cell(self, spec):
        """('e', i, row): extra copy column i; ('c', 0, row): the fixed copy column; ('a' | 'f' | 'i', column, row) as they are"""
        kind, col, row = spec
        if kind == "e":
            return ("a", self.extra0 + col, row)
        if kind == "c":
            return ("f", self.fixed_copy, row)
        return spec

    def value(self, kind, col, row):
        """the field element of a cell as a canonical integer (a stored word v + r stands for v)"""
        row %= self.n
        if kind == "i":
            return self.instances[col][row] if row < len(self.instances[col]) else 0
        return word_of((self.advice if kind == "a" else self.fixed)[col], row) * R_INV % R_MOD

    def put(self, spec, value=None, word=None):
        """a cell <- the Montgomery form of `value`, or the stored word `word` as it is"""
        kind, col, row = self.cell(spec)
        if kind == "i":
            self.instances[col][row] = int(value)
        else:
            w = (int(value) << 256) % R_MOD if word is None else int(word)
            (self.advice if kind == "a" else self.fixed)[col][row] = words([w])[0]
        self.changed.add((kind, col, row))

    def bump(self, spec, by=1):
        kind, col, row = self.cell(spec)
        self.put((kind, col, row), (self.value(kind, col, row) + by) % R_MOD)

    def bump_rows(self, col, rows):
        """advice column `col`, every row of `rows`, + 1 (vectorised)"""
        rows = np.asarray(rows, dtype=np.int64)
        one = np.repeat(words([MONT_ONE]), rows.size, axis=0)
        self.advice[col][rows] = orc.fr_add(self.advice[col][rows], one)
        self.changed.update(("a", col, int(r)) for r in rows)

    # ---- the predictor ----------------------------------------------------------------------------------------------------------------------------------------
    def predict_gates(self):
        n, u = self.n, self.u
        reach = set()
        for (kind, col, row) in self.changed:
            for g, rot in self.readers.get((kind, col), ()):
                r = (row - rot) % n
                if r < u:
                    reach.add((r, g))
        out = []
        for (r, g) in sorted(reach):
            q, t0, t1, t2, t3 = [self.value(kind, col, r + rot) for (kind, col, rot) in self.gates[g]]
            if q * (t0 + t1 * t2 - t3) % R_MOD:
                out.append(MockFailure("gate", g, r, 0, 0))
        return out

    def predict_lookups(self):
        out = []
        u = self.u
        col_words = lambda arr: [int.from_bytes(b[i:i + 32], "little") for b in [np.ascontiguousarray(arr[:u]).tobytes()] for i in range(0, 32 * u, 32)]
        for li, lk in enumerate(self.lookups):
            tcols = [col_words(self.fixed[c]) for c in lk["table"]]
            icols = [col_words(self.advice[c]) for c in lk["inputs"]]
            assert all(w < R_MOD for c in tcols + icols for w in c)                # canonical words: equal words <=> equal values
            table = set(zip(*tcols))
            sel = col_words(self.fixed[lk["selector"]]) if lk["selector"] is not None else [MONT_ONE] * u
            assert set(sel) <= {0, MONT_ONE}
            zero = (0,) * len(tcols)
            for row, tup in enumerate(zip(*icols)):
                if (tup if sel[row] else zero) not in table:
                    out.append(MockFailure("lookup", li, row, 0, 0))
        return out

    def predict_copies(self):
        out = []
        for cyc in self.cycles:
            for i, c in enumerate(cyc):
                s = cyc[(i + 1) % len(cyc)]
                if self.value(*c) != self.value(*s):
                    out.append(MockFailure("copy", self.perm[c[:2]], c[2], self.perm[s[:2]], s[2]))
        return sorted(out, key=lambda f: (f.index, f.row))

    def predict(self):
        return self.predict_gates() + self.predict_lookups() + self.predict_copies()


def build(k, n_gates=1, lookups=(), copy_layout=None, dup_gate=False, inst_len=None, seed=0):
    """-> Case (unpacks as (cs, fixed, asm, advice, instances)), satisfied on every row.
    lookups: dicts {table: [stored words per table column, n Python integers or an (n, 4) array each] | share: index of an earlier lookup whose table columns this one
             reads, selector: None | n integers 0 / 1}.
    copy_layout: {extra: number of advice columns read by the copies alone, cycles: [[cell, ...]]}, cell = ('e', extra column, row) | ('c', 0, row) (the fixed copy
             column) | ('i', 0, row); a cycle takes the value of its instance cell, else of its first cell.
    dup_gate: gate 0's expression registered once more, as the last polynomial."""
    rng = np.random.default_rng(seed)
    n = 1 << k
    copy_layout = copy_layout or dict(extra=0, cycles=[])
    n_extra = copy_layout["extra"]
    in_cols, next_adv = [], D0 + n_gates
    for lk in lookups:
        m = len(lookups[lk["share"]]["table"] if lk.get("share") is not None else lk["table"])
        in_cols.append(list(range(next_adv, next_adv + m)))
        next_adv += m
    extra0 = next_adv
    n_adv = extra0 + n_extra
    fixed_copy, next_fix = n_gates, n_gates + 1
    tab_cols, sel_cols = [], []
    for lk in lookups:
        if lk.get("share") is not None:
            tab_cols.append(tab_cols[lk["share"]])
        else:
            tab_cols.append(list(range(next_fix, next_fix + len(lk["table"]))))
            next_fix += len(lk["table"])
        sel_cols.append(next_fix if lk.get("selector") is not None else None)
        next_fix += lk.get("selector") is not None
    cs = plonk.ConstraintSystem(num_fixed_columns=next_fix, num_advice_columns=n_adv, num_instance_columns=1)

    # gates
    gates = []
    for g in range(n_gates):
        rx, ry = ROTS[g % 3]
        t2 = ("i", 0, 0) if g == n_gates - 1 else ("a", Z, 0)
        gates.append((("f", g, 0), ("a", X, rx), ("a", Y, ry), t2, ("a", D0 + g, 0)))
    if dup_gate:
        gates.append(gates[0])
    node = lambda t: {"a": Advice, "f": Fixed, "i": Instance}[t[0]](t[1], t[2])
    for q, t0, t1, t2, t3 in gates:
        cs.create_gate(node(q) * (node(t0) + node(t1) * node(t2) - node(t3)))
    for li, lk in enumerate(lookups):
        sel = sel_cols[li]
        cs.lookup([(Fixed(sel) * Advice(a) if sel is not None else Advice(a), Fixed(t)) for a, t in zip(in_cols[li], tab_cols[li])])
    u = cs.usable_rows(k)
    assert cs.blinding_factors() == 5 and u == n - 6

    # witness of the gates: d_g = x(rx) + y(ry) * (z | instance) on every row
    inst_len = u // 2 if inst_len is None else inst_len
    xs, ys, zs = (rng.integers(1, 1 << 20, n, dtype=np.uint64) for _ in range(3))
    inst = np.zeros(n, dtype=np.uint64)
    inst[:inst_len] = rng.integers(1, 1 << 20, inst_len, dtype=np.uint64)
    advice = [mont(xs), mont(ys), mont(zs)]
    for g in range(n_gates):
        rx, ry = ROTS[g % 3]
        advice.append(mont(np.roll(xs, -rx) + np.roll(ys, -ry) * (inst if g == n_gates - 1 else zs)))
    one_col = mont(np.ones(n, dtype=np.uint64))
    fixed = [one_col.copy() for _ in range(n_gates)] + [np.zeros((n, 4), dtype=np.uint64)]
    instances = [[int(v) for v in inst[:inst_len]]]

    # lookups: the tables as given, every input row a table row < u
    spec = []
    for li, lk in enumerate(lookups):
        if lk.get("share") is None:
            for t in lk["table"]:
                t = words(t) if not isinstance(t, np.ndarray) else np.ascontiguousarray(t, dtype=np.uint64)
                assert t.shape == (n, 4)
                fixed.append(t.copy())
        if sel_cols[li] is not None:
            fixed.append(mont(np.asarray(lk["selector"], dtype=np.uint64)))
        spec.append(dict(table=tab_cols[li], inputs=in_cols[li], selector=sel_cols[li]))
    assert len(fixed) == next_fix
    for li in range(len(lookups)):
        pick = rng.integers(0, u, n)
        for t in tab_cols[li]:
            advice.append(fixed[t][pick].copy())
    advice += [np.zeros((n, 4), dtype=np.uint64) for _ in range(n_extra)]
    assert len(advice) == n_adv

    # copies: the columns in order of appearance after the extra columns; successors as the cycles list them
    case = Case(k, cs, fixed, None, advice, instances, gates, spec, [], {}, extra0, fixed_copy)
    cycles = [[case.cell(c) for c in cyc] for cyc in copy_layout["cycles"]]
    for c in range(n_extra):
        cs.enable_equality(ADVICE, extra0 + c)
    for cyc in cycles:
        for (kind, col, _row) in cyc:
            cs.enable_equality({"a": ADVICE, "f": FIXED, "i": INSTANCE}[kind], col)
    ty = {ADVICE: "a", FIXED: "f", INSTANCE: "i"}
    perm = {(ty[t], i): j for j, (t, i) in enumerate(cs.permutation_columns)}
    asm = plonk.Assembly(cs, k)
    seen = set()
    for ci, cyc in enumerate(cycles):
        assert len(cyc) >= 2 and not seen & set(cyc) and len(set(cyc)) == len(cyc)
        seen |= set(cyc)
        anchor = next((c for c in cyc if c[0] == "i"), cyc[0])
        v = case.value(*anchor) if anchor[0] == "i" else 1000 + ci
        for c in cyc:
            if c[0] != "i":
                case.put(c, v)
        js = np.array([perm[c[:2]] for c in cyc]), np.array([c[2] for c in cyc])
        asm.map_c[js[0], js[1]] = np.roll(js[0], -1)
        asm.map_r[js[0], js[1]] = np.roll(js[1], -1)
    case.changed.clear()
    case.asm, case.cycles, case.perm = asm, cycles, perm
    return case


# ---- named violations -----------------------------------------------------------------------------------------------------------------------------------------
def plant(case, name, **kw):
    """apply the named violation to `case` (in place) and return the records the whole witness must now give"""
    n, u = case.n, case.u
    if name == "gate_cell":                          # polynomial g alone on one row: its own d_g cell
        case.bump(("a", D0 + kw["gate"], kw["row"]))
    elif name == "gate_all_on_row":                  # every polynomial on one row
        for col in sorted({terms[4][1] for terms in case.gates}):
            case.bump(("a", col, kw["row"]))
    elif name == "gate_rows":                        # polynomial g on every listed row
        case.bump_rows(D0 + kw["gate"], kw["rows"])
    elif name == "wrap_positive":                    # y on row u + 1, a blinding row: of the usable rows only u - 1 reads it, through rotation +ROT
        case.bump(("a", Y, u - 1 + ROT))
    elif name == "wrap_negative":                    # x on row n - 1: of the usable rows only row 0 reads it, through rotation -1
        case.bump(("a", X, n - 1))
    elif name == "unread":                           # x on row u + 2: read by rows u, u + 2 and u + 3 alone
        case.bump(("a", X, u + 2))
    elif name == "lookup_input":                     # the input tuple of lookup l on one row <- stored words
        for a, w in zip(case.lookups[kw["lookup"]]["inputs"], kw["words"]):
            case.put(("a", a, kw["row"]), word=w)
    elif name == "cell":                             # any cell <- a value or a stored word
        case.put(kw["cell"], kw.get("value"), kw.get("word"))
    elif name == "bump":
        case.bump(kw["cell"], kw.get("by", 1))
    else:
        raise KeyError(name)
    return case.predict()


# ---- sort and search: tables and inputs -------------------------------------------------------------------------------------------------------------------
TABLES = ("ascending", "descending", "all_equal", "two_values", "distinct", "word7_only", "word0_only", "r_minus_1")
INPUTS = ("smallest", "largest", "middle", "below_smallest", "above_largest", "only_above_u")


def sort_table(kind, k, seed=0):
    """-> (n stored words, the ghost): rows < u as the kind says, every row >= u the ghost, a canonical word that no row < u holds"""
    rng = np.random.default_rng(seed)
    n = 1 << k
    u = n - 6
    wide = lambda cnt: sorted({int.from_bytes(rng.bytes(25), "little") + 2 for _ in range(4 * cnt)})[:cnt]
    if kind in ("ascending", "descending", "distinct"):
        t = wide(u)
        if kind == "descending":
            t.reverse()
        if kind == "distinct":
            t = [t[i] for i in rng.permutation(u)]
    elif kind == "all_equal":
        t = [wide(1)[0]] * u
    elif kind == "two_values":
        a, b = wide(2)
        t = [b if i % 2 == 0 else a for i in range(u)]
    elif kind == "word7_only":                       # equal but for the top 32-bit word
        low = wide(1)[0]
        t = [low + (int(i) + 1 << 224) for i in rng.permutation(u)]
    elif kind == "word0_only":                       # equal but for the bottom 32-bit word
        high = wide(1)[0] << 32
        t = [high + int(i) + 1 for i in rng.permutation(u)]
    elif kind == "r_minus_1":                        # the largest canonical word pattern among small and middling values
        t = [R_MOD - 1 if i % 3 == 1 else R_MOD - 1 - (1 << 224) if i % 3 == 2 else 5 + i for i in range(u)]
    else:
        raise KeyError(kind)
    ghost = max(t) - 1 if kind == "r_minus_1" else (max(t) + min(t)) // 2
    while ghost in set(t) or ghost in (min(t) - 1, max(t) + 1):
        ghost -= 1
    assert len(t) == u and 0 < min(t) and max(t) < R_MOD and 0 < ghost < R_MOD
    return t + [ghost] * (n - u), ghost


def sort_inputs(table, ghost, u):
    """{input name: (stored word, hit?)}; the word above r - 1 does not exist as a canonical word and is left out for that table"""
    t = sorted(table[:u])
    out = dict(smallest=(t[0], True), largest=(t[-1], True), middle=(t[u // 2], True), below_smallest=(t[0] - 1, False), only_above_u=(ghost, False))
    if t[-1] + 1 < R_MOD:
        out["above_largest"] = (t[-1] + 1, False)
    return out
