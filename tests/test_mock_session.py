"""The MockProver session (zk_mock_prover_open / _check / _info / _close, csrc/mockprover.hip; plonk.dev.NativeMockSession): one circuit resident, many witnesses.

The reference of every check is the one-shot call on the same context - zk_mock_prover_verify(_phased) through NativeMockProver - which the session must equal record
for record; at the emulator sizes dev.py's MockProver is asked too.  The circuits and their planted violations are those of tests/mock_cases.py (and the scenario
functions of tests/test_structured_mock.py built on them); a session is opened on a case's fixed columns and mapping, the witnesses differ in advice cells only.

Sizes: k = 5, 6 on the emulator; k = 10, 12 on the GPU (at k = 10 the table sort passes its partner distance of 512; five copy columns of 2^10 rows pass the 2048-flag
tile of the compaction and the single-workgroup scan over its tiles)."""
import ctypes as C

import numpy as np
import pytest

import mock_cases as mc
import test_structured_mock as tsm
from conftest import EMU_SO
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd._lib import MockInfo, MockWitness, ZkError
from zk_dcap_verifier_amd.fields import R_MOD, fr_mont_array
from zk_dcap_verifier_amd.plonk import Advice
from zk_dcap_verifier_amd.plonk.dev import MockFailure, MockProver, NativeMockProver, NativeMockSession

ERR_ARG = -1
EMU_K, GPU_K = (5, 6), (10, 12)


# ---- the circuit of the parity tests: 3 gates, a single-column table read by two lookups (one blob), a 3-column tuple table, cycles over 5 copy columns ------------
def rich(k, plant=()):
    n, u = 1 << k, (1 << k) - 6
    t, ghost = mc.sort_table("distinct", k)
    tabs = tsm._tuple_tables(k, 3, base=1 << 180)
    cycles = [[("e", 0, 2), ("e", 1, 3), ("c", 0, 4), ("e", 4, n - 1)], [("e", 1, 8), ("i", 0, 0)], [("e", 2, 0), ("e", 3, u - 1)]]
    case = mc.build(k, 3, lookups=[dict(table=[t]), dict(share=0), dict(table=tabs)], copy_layout=dict(extra=5, cycles=cycles))
    assert case.predict() == []
    if "gate" in plant:                              # polynomial 1 alone on the last usable row, every polynomial on row 3
        mc.plant(case, "gate_cell", gate=1, row=u - 1)
        mc.plant(case, "gate_all_on_row", row=3)
    if "lookup" in plant:                            # the shared table through either lookup; a tuple that differs from the table's row 3 in its last expression alone
        mc.plant(case, "lookup_input", lookup=0, row=0, words=[ghost])
        mc.plant(case, "lookup_input", lookup=1, row=u - 1, words=[ghost])
        mc.plant(case, "lookup_input", lookup=2, row=1, words=[tabs[0][3], tabs[1][3], tabs[2][4]])
    if "copy" in plant:
        mc.plant(case, "bump", cell=("e", 1, 3))
        mc.plant(case, "bump", cell=("e", 1, 8))
    return case, case.predict()


PLANTS = dict(clean=(), gate=("gate",), lookup=("lookup",), copy=("copy",), all=("gate", "lookup", "copy"))
KINDS = dict(clean=(0, 0, 0), gate=(4, 0, 0), lookup=(0, 3, 0), copy=(0, 0, 4), all=(4, 3, 4))


def one_shot(be, case, cap=None, challenges=None):
    nm = NativeMockProver.run(case.k, case.cs, case.fixed, case.advice, case.instances, case.asm, backend=be, challenges=challenges)
    if cap is not None:
        return nm._check(cap)
    return nm.failures(), nm.counts


def open_session(be, case):
    return NativeMockSession(case.k, case.cs, case.fixed, case.asm, backend=be)


def same_as_one_shot(be, s, case, want=None, caps=()):
    """the session's records, counts and strings of case's witness against the one-shot call's (and the prediction, where there is one)"""
    ref, ref_counts = one_shot(be, case)
    got = s.check(case.advice, case.instances)
    assert got == ref and s.counts == ref_counts
    assert s.verify(case.advice, case.instances) == mc.strings(ref)
    if want is not None:
        assert got == want and s.counts == mc.kinds(want)
    for cap in caps:
        r, c = one_shot(be, case, cap=cap)
        assert s.check(case.advice, case.instances, cap=cap) == r == ref[:cap] and s.counts == c == ref_counts
    return got


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------------------------------
def parity(be, k, what, dev_py):
    case, want = rich(k, PLANTS[what])
    assert mc.kinds(want) == KINDS[what]
    g, l, c = KINDS["all"]
    caps = (0, 1, 2, g + 1, g + l + 2, g + l + c, g + l + c + 5) if what == "all" else (0, 1, 3)     # "all": cuts inside the gate, the lookup and the copy records
    with open_session(be, case) as s:
        got = same_as_one_shot(be, s, case, want, caps)
        if what == "clean":
            s.assert_satisfied(case.advice, case.instances)
        else:
            with pytest.raises(plonk.VerifyFailure):
                s.assert_satisfied(case.advice, case.instances)
        # device-resident advice (the buffers a following prove adopts): the same records, and the buffers are left as they were
        dev = [be.to_device(a) for a in case.advice]
        assert s.check(dev, case.instances) == got
        assert all(np.array_equal(d.download(a.shape), a) for d, a in zip(dev, case.advice))
    if dev_py:
        assert MockProver.run(case.k, case.cs, case.fixed, case.advice, case.instances, case.asm).verify() == mc.strings(got)


@pytest.mark.parametrize("what", list(PLANTS))
@pytest.mark.parametrize("k", EMU_K)
def test_parity_emulated(emu, k, what):
    parity(emu, k, what, dev_py=True)


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(PLANTS))
@pytest.mark.parametrize("k", GPU_K)
def test_parity_gpu(gpu, k, what):
    parity(gpu, k, what, dev_py=False)


# ---- 2. no state between checks ------------------------------------------------------------------------------------------------------------------------------------
def no_state(be, k):
    base, _ = rich(k)
    with open_session(be, base) as s:
        for what in ("clean", "gate", "lookup", "copy", "clean", "all"):
            case, want = rich(k, PLANTS[what])
            assert all(np.array_equal(a, b) for a, b in zip(case.fixed, base.fixed))      # the witnesses differ in advice cells only
            same_as_one_shot(be, s, case, want)
        case, want = rich(k, PLANTS["all"])
        with pytest.raises(ZkError) as e:                                                 # a check that fails on its arguments ...
            s.check([None] + case.advice[1:], case.instances)
        assert e.value.code == ERR_ARG
        with pytest.raises(ZkError) as e:
            s.check(case.advice, [[R_MOD] + list(case.instances[0][1:])])
        assert e.value.code == ERR_ARG and "not canonical" in str(e.value)
        same_as_one_shot(be, s, base, [])                                                 # ... is followed by a clean one
        same_as_one_shot(be, s, case, want)


@pytest.mark.parametrize("k", EMU_K)
def test_no_state_between_checks_emulated(emu, k):
    no_state(emu, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", GPU_K)
def test_no_state_between_checks_gpu(gpu, k):
    no_state(gpu, k)


# ---- 3. the edge list -------------------------------------------------------------------------------------------------------------------------------------------------
def _columns_for(k, cells):
    """copy columns of 2^k rows that hold at least `cells` cells, five at the least"""
    return max(5, -(-cells // (1 << k)))


def edges_identity(be, k):
    """permutation columns and no cycle: nothing is kept, nothing can fail - whatever the columns hold"""
    case = mc.build(k, 1, copy_layout=dict(extra=5, cycles=[]))
    rng = np.random.default_rng(k)
    for j in range(5):
        case.advice[case.extra0 + j] = mc.mont(rng.integers(1, 1 << 30, case.n, dtype=np.uint64))
    with open_session(be, case) as s:
        assert s.info["n_edges"] == 0 and s.info["n_cells"] == 5 << k
        assert same_as_one_shot(be, s, case, []) == []


def edges_every_cell(be, k, wgs):
    """one cycle through every cell of five columns: as many edges as cells (more than one compaction tile from k = 9), the edge kernels on a grid stride"""
    m, n = 5, 1 << k
    case = mc.build(k, 1, copy_layout=dict(extra=m, cycles=[[tsm._flat(n, e) for e in range(m * n)]]))
    be.tune(mock_edge_wgs=wgs)
    try:
        with open_session(be, case) as s:
            assert s.info["n_edges"] == s.info["n_cells"] == m * n
            same_as_one_shot(be, s, case, [])
            want = mc.plant(case, "bump", cell=tsm._flat(n, 2 * n + 7))
            assert [(f.index, f.row) for f in want] == [(2, 6), (2, 7)]
            same_as_one_shot(be, s, case, want, caps=(1,))
    finally:
        be.tune(mock_edge_wgs=2048)


def edges_three_kinds(be, k):
    """a cycle through an advice, a fixed and an instance column (test_structured_mock's cycle3 and cycle5), instance cells beyond the given values, and a cell
    stored as v + r: both sides of an edge are compared fully reduced"""
    for what in ("cycle3", "cycle5", "instance_padding", "v_plus_r", "v_plus_1_plus_r"):
        case, want = tsm.copies(k, what)
        with open_session(be, case) as s:
            same_as_one_shot(be, s, case, want)


def edges_first_and_last_cell(be, k):
    """an edge at cell 0 and one at the last cell of the mapping: last column, row 2^k - 1, a blinding row"""
    n = 1 << k
    case = mc.build(k, 1, copy_layout=dict(extra=5, cycles=[[("e", 0, 0), ("e", 4, n - 1)]]))
    want = mc.plant(case, "bump", cell=("e", 4, n - 1))
    assert want == [MockFailure("copy", 0, 0, 4, n - 1), MockFailure("copy", 4, n - 1, 0, 0)]
    with open_session(be, case) as s:
        assert s.info["n_edges"] == 2
        same_as_one_shot(be, s, case, want)


def edges_exactly(be, k, count):
    """one cycle of `count` cells spread over the mapping (cell 0 and the last cell among them): `count` edges, and one changed cell fails on the first edge (the
    cell itself) and on the last (its predecessor in the cycle)"""
    m = _columns_for(k, count + 8)
    n, total = 1 << k, m << k
    flat = sorted(set([0, total - 1] + [int(e) for e in np.random.default_rng(count).choice(np.arange(1, total - 1), count - 2, replace=False)]))
    assert len(flat) == count
    case = mc.build(k, 1, copy_layout=dict(extra=m, cycles=[[tsm._flat(n, e) for e in flat]]))
    want = mc.plant(case, "bump", cell=tsm._flat(n, 0))
    assert [f.index * n + f.row for f in want] == [0, total - 1]
    with open_session(be, case) as s:
        assert s.info["n_edges"] == count and s.info["n_cells"] == total
        same_as_one_shot(be, s, case, want, caps=(1,))


def edges_survive_the_callers_arrays(be, k):
    """the mapping planes are the caller's own memory (uint32, contiguous: the binding passes them as they are) and are overwritten after open"""
    case, want = rich(k, PLANTS["copy"])
    case.asm.map_c = np.ascontiguousarray(case.asm.map_c.astype(np.uint32))
    case.asm.map_r = np.ascontiguousarray(case.asm.map_r.astype(np.uint32))
    ref, ref_counts = one_shot(be, case)
    assert ref == want
    with open_session(be, case) as s:
        case.asm.map_c[:] = 0xFFFFFFFF
        case.asm.map_r[:] = 0xDEADBEEF
        assert s.check(case.advice, case.instances) == want and s.counts == ref_counts
        assert [(f.other_column, f.other_row) for f in s.check(case.advice, case.instances)] == [(f.other_column, f.other_row) for f in want]


EDGE_EMU = [(edges_identity, ()), (edges_every_cell, (1,)), (edges_three_kinds, ()), (edges_first_and_last_cell, ()), (edges_exactly, (2047,)),
            (edges_exactly, (2048,)), (edges_exactly, (2049,)), (edges_survive_the_callers_arrays, ())]
EDGE_GPU = [(fn, (3,) if fn is edges_every_cell else args) for fn, args in EDGE_EMU]
_edge_id = lambda p: "-".join([p[0].__name__] + [str(a) for a in p[1]])


@pytest.mark.parametrize("fn,args", EDGE_EMU, ids=[_edge_id(p) for p in EDGE_EMU])
@pytest.mark.parametrize("k", EMU_K)
def test_edge_list_emulated(emu, k, fn, args):
    fn(emu, k, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("fn,args", EDGE_GPU, ids=[_edge_id(p) for p in EDGE_GPU])
@pytest.mark.parametrize("k", GPU_K)
def test_edge_list_gpu(gpu, k, fn, args):
    fn(gpu, k, *args)


# ---- 4. tables ----------------------------------------------------------------------------------------------------------------------------------------------------
class AdviceTable:
    """one lookup whose table is an ADVICE column (no gate, no copy): the table belongs to the witness and is sorted per check"""

    def __init__(self, k):
        self.k, self.n = k, 1 << k
        self.cs = plonk.ConstraintSystem(num_fixed_columns=1, num_advice_columns=2, num_instance_columns=0)
        self.cs.lookup([(Advice(0), Advice(1))])
        self.u = self.cs.usable_rows(k)
        self.fixed, self.asm, self.instances = [np.zeros((self.n, 4), dtype=np.uint64)], None, []
        self.table = [1000 + 3 * r for r in range(self.n)]
        self.inputs = [self.table[(7 * r) % self.u] for r in range(self.n)]

    def witness(self, table):
        self.advice = [fr_mont_array(self.inputs), fr_mont_array(table)]
        return self

    def misses(self, table):
        present = set(table[: self.u])
        return [MockFailure("lookup", 0, r, 0, 0) for r in range(self.u) if self.inputs[r] not in present]


def tables(be, k, dev_py):
    case, _ = rich(k)
    with open_session(be, case) as s:                # fixed-only tables: the single-column blob (shared by lookups 0 and 1) and the tuple table
        assert s.info["n_tables"] == 2 and s.info["n_resident_tables"] == 2 and s.info["n_programs"] == 1 + 3 + 2
        for bad in (0, 1):                           # two lookups on one byte-equal table blob: either misses alone
            c2, want = tsm.shared_table(k, bad)
            with open_session(be, c2) as s2:
                assert s2.info["n_tables"] == 1 and s2.info["n_resident_tables"] == 1
                same_as_one_shot(be, s2, c2, want)
    c3, want = tsm.tuples(k, 3)                      # three expressions: cross-row, swapped, and the tuple that differs from a table row in its last expression only
    with open_session(be, c3) as s:
        assert s.info["n_resident_tables"] == 1
        same_as_one_shot(be, s, c3, want)
    at = AdviceTable(k)
    with open_session(be, at.witness(at.table)) as s:
        assert s.info["n_tables"] == 1 and s.info["n_resident_tables"] == 0 and s.info["n_edges"] == 0
        same_as_one_shot(be, s, at, [])
        t2 = list(at.table)
        t2[14] = 5                                   # inputs of the rows r with 7 r = 14 (mod u) lose their table row ...
        want2 = at.misses(t2)
        assert want2 and same_as_one_shot(be, s, at.witness(t2), want2) == want2
        t3 = list(at.table)
        t3[21] = 6                                   # ... then other rows do, and the first ones are back
        want3 = at.misses(t3)
        assert want3 and not set(want3) & set(want2)
        same_as_one_shot(be, s, at.witness(t3), want3)
        if dev_py:
            assert MockProver.run(k, at.cs, at.fixed, at.advice, [], None).verify() == mc.strings(want3)
        same_as_one_shot(be, s, at.witness(at.table), [])


@pytest.mark.parametrize("k", EMU_K)
def test_tables_emulated(emu, k):
    tables(emu, k, dev_py=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", GPU_K)
def test_tables_gpu(gpu, k):
    tables(gpu, k, dev_py=False)


# ---- 5. phased ----------------------------------------------------------------------------------------------------------------------------------------------------
def phased(be, k):
    """phased_cases.case_a: gates and a lookup table that read the challenge (the table is per-check), copies between the phases"""
    for where in ("row_0", "row_u_minus_1"):
        c, fixed, advice, ch, want = tsm._phased(where, k)
        ref = NativeMockProver.run(c.k, c.cs, fixed, advice, [], c.asm, backend=be, challenges=ch)
        with NativeMockSession(c.k, c.cs, fixed, c.asm, backend=be) as s:
            assert s.info["n_resident_tables"] == 0 and s.info["n_tables"] == 1
            assert s.check(advice, [], challenges=ch) == ref.failures() == want and s.counts == ref.counts
            assert s.check(advice, [], challenges=[ch[0] + 1]) == NativeMockProver.run(c.k, c.cs, fixed, advice, [], c.asm, backend=be, challenges=[ch[0] + 1]).failures()
            for bad in (None, [], [1, 2]):           # a wrong number of challenges
                with pytest.raises(ZkError) as e:
                    s.check(advice, [], challenges=bad)
                assert e.value.code == ERR_ARG
            assert s.check(advice, [], challenges=ch) == want


@pytest.mark.parametrize("k", EMU_K)
def test_phased_emulated(emu, k):
    phased(emu, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", GPU_K)
def test_phased_gpu(gpu, k):
    phased(gpu, k)


# ---- 6. refusals and lifetime ------------------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    with pytest.raises(ZkError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def refusals(be, k, other):
    case, want = rich(k, PLANTS["all"])
    inst = [[int(v) for v in c] for c in case.instances]
    # a mapping entry out of range: refused at open, named, no handle
    for plane, j, row, v in (("map_c", 1, 3, len(case.asm.columns)), ("map_r", 0, 0, 1 << k)):
        bad, _ = rich(k)
        getattr(bad.asm, plane)[j, row] = v
        code, text = _code(open_session, be, bad)
        assert code == ERR_ARG and "copy-mapping entry is out of range" in text
    s = open_session(be, case)
    h = s.handle
    assert s.check(case.advice, inst) == want
    assert _code(be.mock_prover_check, h, case.advice, inst, struct_size=C.sizeof(MockWitness) - 8)[0] == ERR_ARG
    assert _code(be.mock_prover_info, h, struct_size=C.sizeof(MockInfo) + 8)[0] == ERR_ARG
    assert _code(be.mock_prover_check, h, [case.advice[0], None] + case.advice[2:], inst)[0] == ERR_ARG
    assert _code(be.mock_prover_check, h, case.advice, inst, n_challenges=1)[0] == ERR_ARG
    # another context does not know the handle, and cannot close it
    for call in (lambda: other.mock_prover_check(h, case.advice, inst), lambda: other.mock_prover_info(h), lambda: other.mock_prover_close(h)):
        code, text = _code(call)
        assert code == ERR_ARG and "unknown handle" in text
    assert s.check(case.advice, inst) == want        # the handle is as usable as before
    s.close()
    for call in (lambda: be.mock_prover_check(h, case.advice, inst), lambda: be.mock_prover_info(h), lambda: be.mock_prover_close(h)):
        assert _code(call)[0] == ERR_ARG
    s.close()                                        # (a second close of the Python object is a no-op)
    # zk_ctx_destroy with a handle open; the same handle value means nothing to a context created afterwards
    s2 = open_session(other, case)
    assert s2.check(case.advice, inst) == want


def test_refusals_and_lifetime_emulated(emu):
    import zk_dcap_verifier_amd as z
    live = C.CDLL(EMU_SO).zk_test_live_device_allocs
    live.restype = C.c_long
    case, _ = rich(5)
    with open_session(emu, case) as s:               # (the context's own workspaces reach their sizes here)
        s.check(case.advice, case.instances)
    before = live()
    other = z.Backend(0, lib_path=EMU_SO)
    other.tune(quot_threads=32)
    refusals(emu, 5, other)
    assert live() > before
    other.close()                                    # the handle refusals() left open on it goes with the context
    assert live() == before


@pytest.mark.gpu
def test_refusals_and_lifetime_gpu(gpu):
    import zk_dcap_verifier_amd as z
    other = z.Backend(0)
    try:
        refusals(gpu, 10, other)
    finally:
        other.close()


def test_device_allocations_emulated(emu):
    """close returns what open took; from the second check on a check allocates nothing"""
    live = C.CDLL(EMU_SO).zk_test_live_device_allocs
    live.restype = C.c_long
    case, want = rich(6, PLANTS["all"])
    with open_session(emu, case) as s:               # (the context's own workspaces reach their sizes here)
        s.check(case.advice, case.instances)
    before = live()
    s = open_session(emu, case)
    assert live() > before
    assert s.check(case.advice, case.instances) == want
    assert s.check(case.advice, case.instances) == want
    steady = live()
    clean, _ = rich(6)
    for i in range(8):
        assert s.check((case if i % 2 else clean).advice, case.instances) == (want if i % 2 else [])
    assert live() == steady
    held = s.info["device_bytes"]
    assert held > 0
    s.close()
    assert live() == before
