"""zk_mock_prover_verify (csrc/mockprover.hip, the row-list mode of quotient_rows_kernel) on circuits that hold by construction but for a few PLANTED cells
(tests/mock_cases.py): the records must be exactly the predicted ones — as records, with exact counts, from host columns and from device buffers.

The existing MockProver tests know two regimes, "nearly every row fails" (random witnesses) and "nothing or a handful of convenient cells"; here every family puts
a single violation where a kernel can be one off: the bit words of 32 / 33 / 64 / 65 gate polynomials, the wave / round / tile edges of the compaction and its scan
over more than 256 tiles, the bitonic sort and the search on ordered, constant and word-boundary tables, the rows at and above u and the wrap, tuples, shared tables,
and copy cycles through all three column kinds.

Three layers, the same scenario functions in each:
  * CPU, no emulator: the predictor against plonk.dev.MockProver at k <= 7 (dev.py is O(rows x constraints)) — after which the larger sizes trust the predictor;
  * CPU, emulator: every family at the smallest size that still has its edge;
  * GPU: every family at the sizes where the launch structure changes (k up to 16).
The 257-, 272- and 544-tile compactions run on the emulator too: one call takes 0.6 s (257 tiles), 0.5 s (272) and 1.1 s (544) there."""
import numpy as np
import pytest

import mock_cases as mc
import phased_cases
from zk_dcap_verifier_amd._lib import ZkError
from zk_dcap_verifier_amd.fields import R_MOD
from zk_dcap_verifier_amd.plonk.dev import MockFailure, MockProver, NativeMockProver

ERR_ARG = -1


# ---- scenarios: (k, ...) -> (case, predicted records) ------------------------------------------------------------------------------------------------------------
def _edge_rows(u):
    return [r for r in (0, 1, 63, 64, 255, 256) if r < u - 1] + [u - 1]


def gates_single(k, n_gates):
    """the last polynomial alone on row u - 1: one row in the list, one bit in the last word"""
    case = mc.build(k, n_gates)
    want = mc.plant(case, "gate_cell", gate=n_gates - 1, row=case.u - 1)
    assert want == [MockFailure("gate", n_gates - 1, case.u - 1, 0, 0)]
    return case, want


def gates_each(k, n_gates):
    """one polynomial per failing row: the indices around the word boundaries on the rows around the wave / round edges"""
    case = mc.build(k, n_gates)
    polys = sorted({p for p in (0, 30, 31, 32, 33, 63, 64, n_gates - 1) if p < n_gates})
    rows = _edge_rows(case.u)
    rows += [r for r in range(2, case.u, 3) if r not in rows][: max(0, len(polys) - len(rows))]
    want = []
    for i, row in enumerate(rows):
        want = mc.plant(case, "gate_cell", gate=polys[i % len(polys)], row=row)
    assert sorted((f.row, f.index) for f in want) == sorted((row, polys[i % len(polys)]) for i, row in enumerate(rows))
    return case, want


def gates_all_on_row(k, n_gates):
    case = mc.build(k, n_gates)
    row = 64 if case.u > 64 else 1
    want = mc.plant(case, "gate_all_on_row", row=row)
    assert want == [MockFailure("gate", g, row, 0, 0) for g in range(n_gates)]
    return case, want


def gates_every_row(k, n_gates):
    """one polynomial on every row < u (and on the rows above, which must not count): n_rows = u, one bit per row"""
    case = mc.build(k, n_gates)
    g = min(32, n_gates - 1)
    want = mc.plant(case, "gate_rows", gate=g, rows=np.arange(case.n))
    assert want == [MockFailure("gate", g, r, 0, 0) for r in range(case.u)]
    return case, want


def gates_above_u(k, n_gates=2):
    """violations on rows u .. n - 1 alone, and a cell no usable row reads: nothing is reported"""
    case = mc.build(k, n_gates)
    mc.plant(case, "gate_rows", gate=0, rows=np.arange(case.u, case.n))
    want = mc.plant(case, "unread")
    assert want == []
    return case, want


def gates_wrap(k, which, n_gates=4):
    """the blinding-row cell that row u - 1 alone reads through +ROT / the row n - 1 cell that row 0 alone reads through -1: gates 0 and 3 carry that rotation"""
    case = mc.build(k, n_gates)
    want = mc.plant(case, "wrap_" + which)
    row = case.u - 1 if which == "positive" else 0
    # (gate 3 is the last gate: its T2 is the instance column, zero on row u - 1 and non-zero on row 0, and the positive wrap goes through T1 * T2)
    assert want == [MockFailure("gate", g, row, 0, 0) for g in ((0,) if which == "positive" else (0, 3))]
    return case, want


def gates_duplicate(k, n_gates=3):
    """gate 0's expression registered twice: both indices are reported"""
    case = mc.build(k, n_gates, dup_gate=True)
    want = mc.plant(case, "gate_cell", gate=0, row=5)
    assert want == [MockFailure("gate", 0, 5, 0, 0), MockFailure("gate", n_gates, 5, 0, 0)]
    return case, want


def gates_tile(k, full):
    """k = 13: rows 2047 and 2048 (the last flag of a compaction tile and the first of the next), or the whole tile 2048 .. 4095 between clean tiles"""
    case = mc.build(k, 2)
    rows = np.arange(2048, 4096) if full else np.array([2047, 2048])
    want = mc.plant(case, "gate_rows", gate=1, rows=rows)
    assert [f.row for f in want] == rows.tolist()
    return case, want


def _flat(case_n, e):
    return ("e", e // case_n, e % case_n)


def copies_compaction(k, m, singles, full_tile=None):
    """m copy columns x 2^k cells, flagged exactly at the flat indices `singles` and on the whole tile `full_tile`.  A violated cycle flags at least two cells, so
    the singles pair up with each other, or, where a tile is flagged as a whole, each with one cell of that tile (whose other cells form one cycle)."""
    n = 1 << k
    assert all(0 <= e < m * n for e in singles) and len(set(singles)) == len(singles)
    if full_tile is None:
        assert len(singles) % 2 == 0
        cycles = [[_flat(n, a), _flat(n, b)] for a, b in zip(singles[0::2], singles[1::2])]
        rest = []
    else:
        tile = list(range(full_tile * mc.TILE, (full_tile + 1) * mc.TILE))
        assert tile[-1] < m * n and not set(tile) & set(singles)
        cycles = [[_flat(n, a), _flat(n, b)] for a, b in zip(singles, tile)]
        rest = tile[len(singles):]
        cycles.append([_flat(n, e) for e in rest])
    case = mc.build(k, 1, copy_layout=dict(extra=m, cycles=cycles))
    assert case.predict() == [] and [case.perm[("a", case.extra0 + j)] for j in range(m)] == list(range(m))
    for cyc in cycles[: len(cycles) - (full_tile is not None)]:
        case.bump(cyc[0], 7)
    for i, e in enumerate(rest):
        case.put(_flat(n, e), 5000 + i)
    want = case.predict()
    flagged = sorted(set(singles) | set(range(full_tile * mc.TILE, (full_tile + 1) * mc.TILE) if full_tile is not None else ()))
    assert [f.index * n + f.row for f in want] == flagged
    return case, want


def _spread(tiles, full_tile):
    """one flagged cell in every 37th tile (at offsets that move through the tile), the first cell of the first tile, the last cell of the last tile"""
    assert full_tile % 37 != 36 and 0 < full_tile < tiles - 1
    return [0] + [t * mc.TILE + (t * 97) % mc.TILE for t in range(36, tiles - 1, 37)] + [tiles * mc.TILE - 1]


def copies_compaction_edges(k, m):
    """the edges of a wave (63 / 64), a round (255 / 256) and a tile (2047 / 2048), the first and last cell of the last tile, the last cell of all"""
    total = m << k
    last0 = (total - 1) // mc.TILE * mc.TILE
    singles = sorted({e for e in (0, 63, 64, 255, 256, 2047, 2048, last0 - 1, last0, total - 1) if 0 <= e < total})
    if len(singles) % 2:
        singles.append(next(e for e in range(1, total) if e not in singles))
    return copies_compaction(k, m, singles)


def copies_compaction_spread(k, m, full_tile):
    return copies_compaction(k, m, _spread((m << k) // mc.TILE, full_tile), full_tile)


def lookups_compaction(k, n_lookups):
    """L x u flags, lookup boundaries inside a tile: misses on the last row of lookup l and the first row of lookup l + 1 (e / u and e % u)"""
    tabs = [mc.sort_table("distinct", k, seed=l) for l in range(n_lookups)]
    case = mc.build(k, 1, lookups=[dict(table=[t]) for t, _ in tabs])
    assert (n_lookups * case.u) % mc.TILE
    want = []
    for l in range(n_lookups - 1):
        mc.plant(case, "lookup_input", lookup=l, row=case.u - 1, words=[tabs[l][1]])
        want = mc.plant(case, "lookup_input", lookup=l + 1, row=0, words=[tabs[l + 1][1]])
    assert want == sorted(MockFailure("lookup", l, r, 0, 0) for l in range(n_lookups) for r in (0, case.u - 1) if (l, r) not in ((0, 0), (n_lookups - 1, case.u - 1)))
    return case, want


def sort_search(k, table, group):
    """one single-column lookup: the table as `table` says, the inputs of `group` on the edge rows, every other row a hit"""
    t, ghost = mc.sort_table(table, k)
    case = mc.build(k, 1, lookups=[dict(table=[t])])
    inputs = mc.sort_inputs(t, ghost, case.u)
    names = [nm for nm in mc.INPUTS if nm in inputs]
    per = min(len(names), case.u)
    edge = [case.u - 1] + _edge_rows(case.u)[:-1]
    rows = (edge + [r for r in range(2, case.u - 1) if r not in edge])[:per]
    want, expect = [], []
    for nm, row in zip(names[group * per: (group + 1) * per], rows):
        word, hit = inputs[nm]
        want = mc.plant(case, "lookup_input", lookup=0, row=row, words=[word])
        expect += [] if hit else [MockFailure("lookup", 0, row, 0, 0)]
    assert want == sorted(expect)
    return case, want


def _tuple_tables(k, m, seed=0, base=0):
    """m table columns of n distinct words each, no word in two columns"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    return [[base + ((c + 1) << 200) + int(v) + 1 for v in rng.permutation(n)] for c in range(m)]


def tuples(k, m):
    """the cross-row tuple, the swapped tuple, the tuple that differs from a table row in its last expression alone; a hit on the row between them"""
    tabs = _tuple_tables(k, m)
    assert len({w for t in tabs for w in t}) == m << k
    case = mc.build(k, 1, lookups=[dict(table=tabs)])
    u = case.u
    cross = [tabs[0][1]] + [t[u - 1] for t in tabs[1:]]
    swapped = [tabs[1][2], tabs[0][2]] + [t[2] for t in tabs[2:]]
    last = [t[3] for t in tabs[:-1]] + [tabs[-1][4]]
    mc.plant(case, "lookup_input", lookup=0, row=0, words=cross)
    mc.plant(case, "lookup_input", lookup=0, row=1, words=swapped)
    mc.plant(case, "lookup_input", lookup=0, row=2, words=[t[u - 1] for t in tabs])            # the table's last usable row: a hit
    want = mc.plant(case, "lookup_input", lookup=0, row=u - 1, words=last)
    assert want == [MockFailure("lookup", 0, r, 0, 0) for r in (0, 1, u - 1)]
    return case, want


def tuples_swappable(k):
    """a two-column table whose columns hold the same words on different rows: (a, b) with a in T0 and b in T1, but never on one row"""
    n = 1 << k
    t0 = _tuple_tables(k, 1)[0]
    t1 = t0[1:] + t0[:1]
    case = mc.build(k, 1, lookups=[dict(table=[t0, t1])])
    mc.plant(case, "lookup_input", lookup=0, row=3, words=[t0[5], t1[6]])                       # both words in both columns, on different rows
    want = mc.plant(case, "lookup_input", lookup=0, row=4, words=[t1[7], t0[7]])                # the swapped tuple of row 7
    assert n > 16 and want == [MockFailure("lookup", 0, r, 0, 0) for r in (3, 4)]
    return case, want


def shared_table(k, bad):
    """two lookups on the same table columns (byte-equal table programs share one sorted column): lookup `bad` misses once, the other is clean"""
    t, ghost = mc.sort_table("distinct", k)
    case = mc.build(k, 1, lookups=[dict(table=[t]), dict(share=0)])
    want = mc.plant(case, "lookup_input", lookup=bad, row=case.u - 2, words=[ghost])
    assert want == [MockFailure("lookup", bad, case.u - 2, 0, 0)]
    return case, want


def disjoint_tables(k):
    """two lookups on tables with disjoint value sets: an input of lookup 0 drawn from lookup 1's table, and the other way round on another row"""
    t0, t1 = _tuple_tables(k, 2)
    case = mc.build(k, 1, lookups=[dict(table=[t0]), dict(table=[t1])])
    mc.plant(case, "lookup_input", lookup=0, row=2, words=[t1[2]])
    want = mc.plant(case, "lookup_input", lookup=1, row=case.u - 1, words=[t0[0]])
    assert want == [MockFailure("lookup", 0, 2, 0, 0), MockFailure("lookup", 1, case.u - 1, 0, 0)]
    return case, want


def selector_off(k, zero_in_table):
    """a lookup q * a whose selector is off on the planted row: input 0.  With 0 in the table no record; without, one on every selector-off row < u"""
    n = 1 << k
    t = _tuple_tables(k, 1)[0]
    if zero_in_table:
        t[n // 3] = 0
    sel = [0 if r % 5 == 2 else 1 for r in range(n)]
    case = mc.build(k, 1, lookups=[dict(table=[t], selector=sel)])
    want = mc.plant(case, "lookup_input", lookup=0, row=7, words=[t[-1] + 12345])               # row 7: selector off, the cell holds a word outside the table
    assert want == ([] if zero_in_table else [MockFailure("lookup", 0, r, 0, 0) for r in range(case.u) if r % 5 == 2])
    return case, want


def _copy_case(k, cycles, extra=3):
    return mc.build(k, 2, copy_layout=dict(extra=extra, cycles=cycles))


def copies(k, what):
    case0 = mc.build(k, 2)
    u, n, ilen = case0.u, case0.n, len(case0.instances[0])
    if what == "cycle3":                             # advice -> fixed -> instance, the advice cell changed: it and its predecessor differ from their successors
        case = _copy_case(k, [[("e", 0, 2), ("c", 0, 5), ("i", 0, 1)]])
        want = mc.plant(case, "bump", cell=("e", 0, 2))
        assert [(f.index, f.row) for f in want] == [(0, 2), (case.perm[("i", 0)], 1)]
    elif what == "cycle5":
        case = _copy_case(k, [[("e", 0, 2), ("e", 1, u - 1), ("c", 0, 5), ("e", 2, 0), ("i", 0, 3)]])
        want = mc.plant(case, "bump", cell=("c", 0, 5))
        assert len(want) == 2
    elif what == "two_same_wrong":                   # two cells of a 5-cycle, not neighbours, changed to the same wrong value: four pairs differ
        case = _copy_case(k, [[("e", 0, 2), ("e", 1, u - 1), ("c", 0, 5), ("e", 2, 0), ("i", 0, 3)]])
        mc.plant(case, "cell", cell=("e", 0, 2), value=99)
        want = mc.plant(case, "cell", cell=("c", 0, 5), value=99)
        assert len(want) == 4
    elif what == "two_same_wrong_neighbours":        # neighbours: they agree with each other, two pairs differ
        case = _copy_case(k, [[("e", 0, 2), ("e", 1, u - 1), ("c", 0, 5), ("e", 2, 0), ("i", 0, 3)]])
        mc.plant(case, "cell", cell=("e", 0, 2), value=99)
        want = mc.plant(case, "cell", cell=("e", 1, u - 1), value=99)
        assert len(want) == 2
    elif what == "instance_padding":                 # an instance cell beyond the given values reads as 0: clean against 0, two records against 1
        case = _copy_case(k, [[("e", 0, 7), ("i", 0, ilen + 3)], [("e", 1, 7), ("i", 0, n - 1)]])
        assert case.value("a", case.extra0, 7) == 0 and case.predict() == []
        want = mc.plant(case, "bump", cell=("e", 1, 7))
        assert [(f.index, f.row) for f in want] == [(1, 7), (case.perm[("i", 0)], n - 1)]
    elif what == "above_u":                          # cells on rows >= u are checked like any other (dev.py runs over all 2^k rows)
        case = _copy_case(k, [[("e", 0, u + 1), ("e", 1, n - 1), ("e", 2, u)]])
        want = mc.plant(case, "bump", cell=("e", 1, n - 1))
        assert [(f.index, f.row) for f in want] == [(0, u + 1), (1, n - 1)]
    elif what in ("v_plus_r", "v_plus_1_plus_r"):    # a cell stored as the representative v + r of its value: both sides are compared fully reduced
        case = _copy_case(k, [[("e", 2, 9), ("e", 1, 9)]])
        w = mc.word_of(case.advice[case.extra0 + 1], 9)
        assert 0 < w < R_MOD and w + 1 + R_MOD < 1 << 256
        if what == "v_plus_r":
            want = mc.plant(case, "cell", cell=("e", 2, 9), word=w + R_MOD)
            assert want == []                        # by the header's "fully reduced"; stated here, not asked of dev.py (which reduces too)
        else:
            want = mc.plant(case, "cell", cell=("e", 2, 9), word=(w + mc.MONT_ONE) % R_MOD + R_MOD)
            assert [(f.index, f.row, f.other_column, f.other_row) for f in want] == [(1, 9, 2, 9), (2, 9, 1, 9)]
    else:
        raise KeyError(what)
    return case, want


def all_three(k):
    """gates, lookups and copies violated on one witness (truncation)"""
    t, ghost = mc.sort_table("ascending", k)
    case = mc.build(k, 3, lookups=[dict(table=[t]), dict(share=0)], copy_layout=dict(extra=2, cycles=[[("e", 0, 2), ("e", 1, 3), ("c", 0, 4)], [("e", 1, 8), ("i", 0, 0)]]))
    assert case.predict() == []
    mc.plant(case, "gate_all_on_row", row=3)
    mc.plant(case, "gate_cell", gate=1, row=case.u - 1)
    mc.plant(case, "lookup_input", lookup=0, row=0, words=[ghost])
    mc.plant(case, "lookup_input", lookup=1, row=case.u - 1, words=[ghost])
    mc.plant(case, "lookup_input", lookup=1, row=1, words=[ghost])
    mc.plant(case, "bump", cell=("e", 1, 3))
    want = mc.plant(case, "bump", cell=("e", 1, 8))
    assert mc.kinds(want) == (4, 3, 4)
    return case, want


def clean(k):
    """everything at once and nothing planted"""
    t, _ = mc.sort_table("two_values", k)
    sel = [r % 2 for r in range(1 << k)]
    t2, t3 = list(t), list(reversed(t))
    t2[1] = t3[1] = 0                                # the all-zero tuple of the selector-off rows is in the table
    case = mc.build(k, 33, lookups=[dict(table=[t]), dict(table=[t2, t3], selector=sel)],
                    copy_layout=dict(extra=2, cycles=[[("e", 0, 2), ("e", 1, 3), ("c", 0, 4)], [("e", 1, 8), ("i", 0, 0)]]))
    want = case.predict()
    assert want == []
    return case, want


# ---- the three layers ----------------------------------------------------------------------------------------------------------------------------------------
N_GATES = (1, 31, 32, 33, 64, 65)
COPIES = ("cycle3", "cycle5", "two_same_wrong", "two_same_wrong_neighbours", "instance_padding", "above_u", "v_plus_r", "v_plus_1_plus_r")


def _p(fn, *args):
    return pytest.param(fn, args, id="-".join([fn.__name__] + [str(a) for a in args]))


def _families(kg, kc, kt, sort_ks, compaction, lookup_compaction):
    """kg / kc / kt: k of the gate, copy and tuple families"""
    out = []
    for ng in N_GATES:
        out += [_p(gates_single, kg, ng), _p(gates_each, kg, ng), _p(gates_all_on_row, kg, ng), _p(gates_every_row, kg, ng)]
    out += [_p(gates_above_u, kg), _p(gates_wrap, kg, "positive"), _p(gates_wrap, kg, "negative"), _p(gates_duplicate, kg), _p(clean, kg)]
    out += compaction + [_p(lookups_compaction, *lookup_compaction)]
    for k in sort_ks:
        groups = 3 if (1 << k) - 6 < 6 else 1
        out += [_p(sort_search, k, table, g) for table in mc.TABLES for g in range(groups)]
    out += [_p(tuples, kt, 2), _p(tuples, kt, 3), _p(tuples_swappable, kt), _p(shared_table, kt, 0), _p(shared_table, kt, 1), _p(disjoint_tables, kt),
            _p(selector_off, kt, True), _p(selector_off, kt, False)]
    out += [_p(copies, kc, what) for what in COPIES]
    return out


CPU_CASES = _families(6, 5, 5, (3, 5, 7), [_p(copies_compaction_edges, 7, 3), _p(copies_compaction_spread, 7, 100, 3)], (6, 3)) + [_p(all_three, 6)]
# one call of the emulator on 257 / 272 / 544 tiles of copies measured 0.6 s / 0.5 s / 1.1 s (each case makes two calls), far below the 20 s that would keep them off it
EMU_CASES = _families(6, 5, 5, (3, 5, 9, 10), [_p(copies_compaction_edges, 9, 3), _p(copies_compaction_edges, 10, 3), _p(copies_compaction_spread, 9, 12, 1),
                                               _p(copies_compaction_edges, 11, 257), _p(copies_compaction_spread, 15, 17, 100), _p(copies_compaction_spread, 16, 17, 300)],
                      (6, 3))
GPU_CASES = _families(11, 12, 9, (9, 10, 11, 13),
                      [_p(copies_compaction_edges, 9, 3),            # 1 tile, partial
                       _p(copies_compaction_edges, 10, 3),           # 2 tiles, the second partial
                       _p(copies_compaction_edges, 15, 16),          # exactly 256 tiles: per = 1, every thread of the scan owns a tile
                       _p(copies_compaction_edges, 11, 257),         # 257 tiles: per = 2
                       _p(copies_compaction_spread, 15, 17, 100),    # 272 tiles: per = 2, the last threads of the scan own no tile
                       _p(copies_compaction_spread, 16, 17, 300)],   # 544 tiles: per = 3
                      (10, 5)) + [_p(gates_tile, 13, False), _p(gates_tile, 13, True)]


def _check(be, case, want):
    """the three assertions of every device check, on host columns and on device buffers"""
    for on_device in (False, True):
        fixed, advice = case.fixed, case.advice
        if on_device:
            fixed, advice = [be.to_device(c) for c in fixed], [be.to_device(c) for c in advice]
        nm = NativeMockProver.run(case.k, case.cs, fixed, advice, case.instances, case.asm, backend=be)
        got = nm.failures()
        assert len(got) == len(want) and got == want, (on_device, [p for p in zip(got, want) if p[0] != p[1]][:5])
        assert nm.counts == mc.kinds(want)


# ---- CPU: the predictor against dev.py ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,args", CPU_CASES)
def test_predictor_matches_dev_py(fn, args):
    case, want = fn(*args)
    assert case.k <= 7
    assert MockProver.run(case.k, case.cs, case.fixed, case.advice, case.instances, case.asm).verify() == mc.strings(want)


def test_phased_predictor_matches_dev_py():
    for where in ("row_0", "row_u_minus_1"):
        c, fixed, advice, ch, want = _phased(where)
        assert MockProver.run(c.k, c.cs, fixed, advice, [], c.asm, challenges=ch).verify() == mc.strings(want)


# ---- CPU: the emulator build --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,args", EMU_CASES)
def test_planted_violations_emulated(emu, fn, args):
    _check(emu, *fn(*args))


def _truncation(be, k):
    case, want = all_three(k)
    nm = NativeMockProver.run(case.k, case.cs, case.fixed, case.advice, case.instances, case.asm, backend=be)
    g, l, c = mc.kinds(want)
    total = g + l + c
    for cap in (0, g, g + 1, g + l, g + l + 1, total, total + 5):    # .. the last gate record, the first / last lookup record, the first copy record ..
        recs, counts = nm._check(cap)
        assert counts == (g, l, c)
        assert recs == want[:cap] and len(recs) == min(cap, total)   # n_written records come back


def test_truncation_emulated(emu):
    _truncation(emu, 6)


def _bad_instance(be, k):
    """an instance value equal to r is not canonical: ZK_ERR_ARG, and the context checks a clean witness afterwards"""
    case, want = clean(k)
    nm = NativeMockProver.run(case.k, case.cs, case.fixed, case.advice, case.instances, case.asm, backend=be)
    args = dict(nm.args)
    args["instances"] = [[R_MOD] + list(case.instances[0][1:])]
    with pytest.raises(ZkError) as e:
        be.mock_prover_verify(cap=4, **args)
    assert e.value.code == ERR_ARG
    assert nm.failures() == want == [] and nm.counts == (0, 0, 0)


def test_bad_instance_then_clean_emulated(emu):
    _bad_instance(emu, 6)


def _phased(where, k=6):
    """phased_cases.case_a with the violation on row 0 or row u - 1 of gate 1, q (acc(+1) - acc c0 - a(+1)), the gate that reads the challenge.
    row_0: acc on row 0 is off by one — gate 0 (acc - a) and gate 1 on row 0, and the copy a[0] = acc[0] both ways.
    row_u_minus_1: the selector switched on on row u - 1, where gate 1 reads row u of acc and a through +1 (zero there): acc[u - 1] c0 is not zero."""
    c = phased_cases.case_a(k)
    ch = [0x1234567 + (1 << 200)]
    w = c.witness(ch)
    fixed = [list(col) for col in c.fixed]
    u, n = c.cs.usable_rows(k), 1 << k
    a, acc = w[0], w[2]
    if where == "row_0":
        acc[0] = (acc[0] + 1) % R_MOD
        assert (acc[1] - acc[0] * ch[0] - a[1]) % R_MOD and fixed[0][0] == fixed[1][0] == 1
        want = [MockFailure("gate", 0, 0, 0, 0), MockFailure("gate", 1, 0, 0, 0), MockFailure("copy", 0, 0, 1, 0), MockFailure("copy", 1, 0, 0, 0)]
        assert c.asm.columns[:2] == [(0, 0), (0, 2)]
    else:
        assert fixed[1][u - 1] == 0 and acc[u % n] == 0 and a[u % n] == 0 and acc[u - 1] * ch[0] % R_MOD
        fixed[1][u - 1] = 1
        want = [MockFailure("gate", 1, u - 1, 0, 0)]
    return c, fixed, w, ch, want


def _phased_check(be, where):
    c, fixed, advice, ch, want = _phased(where)
    nm = NativeMockProver.run(c.k, c.cs, fixed, advice, [], c.asm, backend=be, challenges=ch)
    assert nm.failures() == want and nm.counts == mc.kinds(want)


@pytest.mark.parametrize("where", ["row_0", "row_u_minus_1"])
def test_phased_planted_emulated(emu, where):
    _phased_check(emu, where)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fn,args", GPU_CASES)
def test_planted_violations_gpu(gpu, fn, args):
    _check(gpu, *fn(*args))


@pytest.mark.gpu
def test_truncation_gpu(gpu):
    _truncation(gpu, 11)


@pytest.mark.gpu
def test_bad_instance_then_clean_gpu(gpu):
    _bad_instance(gpu, 11)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["row_0", "row_u_minus_1"])
def test_phased_planted_gpu(gpu, where):
    _phased_check(gpu, where)
