"""plonk.dev.NativeMockProver — halo2's MockProver::verify on the device (zk_mock_prover_verify, csrc/mockprover.hip) against the host MockProver of
plonk/dev.py: the same failure strings in the same order, exact counts, truncation at `cap`, the argument errors of the entry point.  CPU tests run the
same kernel sources on the emulator; GPU tests run the product library on the MI355X, up to the sgx-shaped circuit at k = 19.

The existing ABI census (tests/test_shim_abi.py) enumerates the versioned structs that begin with struct_size; the two MockProver structs are declared apart
from their typedefs, so their Rust mirrors (shim/halo2_proofs_mi355x/src/mock_native.rs) are diffed against the header here, with the same parser."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import EMU_SO, ROOT
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd._lib import MockDesc, MockFailure, ZkError
from zk_dcap_verifier_amd.fields import R_MOD, fr_int_array, fr_mont, fr_mont_array
from zk_dcap_verifier_amd.plonk import expression as ex
from zk_dcap_verifier_amd.plonk.dev import MockProver, NativeMockProver

sys.path.insert(0, os.path.join(ROOT, "tools"))
from random_circuits import random_circuit  # noqa: E402
from test_create_proof import toy_circuit  # noqa: E402

ERR_ARG, ERR_PROGRAM = -1, -4


def _kinds(strings):
    return tuple(sum(1 for s in strings if s.startswith(p)) for p in ("gate ", "lookup ", "copy "))


def _corrupt_lookup(cs, fixed, advice, k, seed):
    """one input cell of a lookup set to a value absent from its table, on a row where the lookup's selector (if any) is on"""
    rnd = np.random.default_rng(seed)
    u = cs.usable_rows(k)
    for li in rnd.permutation(len(cs.lookups)):
        log = {}
        ex.queries(cs.lookups[li].input_expressions[0], log)
        adv = [c for (kind, c, _r) in log if kind == "advice"]
        sel = [c for (kind, c, _r) in log if kind == "fixed"]
        rows = [r for r in range(u) if not sel or int(fixed[sel[0]][r]) % R_MOD == 1]
        if adv and rows:
            r = int(rnd.choice(rows))
            advice[adv[0]][r] = fr_mont(R_MOD - 12345 - seed)
            return li, r
    return None


def _differential(be, k, seed):
    cs, fixed, asm, advice, instances = random_circuit(k, seed)
    advice = [a.copy() for a in advice]
    _corrupt_lookup(cs, fixed, advice, k, seed)
    want = MockProver.run(k, cs, fixed, advice, instances, asm).verify()
    nm = NativeMockProver.run(k, cs, fixed, advice, instances, asm, backend=be)
    assert nm.verify() == want
    assert nm.counts == _kinds(want)
    return want


# ---- CPU: the emulator build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_native_mock_prover_matches_dev_py_on_random_circuits_emulated(emu, seed):
    want = _differential(emu, 5 + seed % 4, seed)
    assert want                                                      # random witnesses violate gates and copies


def test_satisfied_circuits_give_no_failures_emulated(emu):
    cs, fixed, asm, advice, instances = toy_circuit(8)
    nm = NativeMockProver.run(8, cs, fixed, advice, instances, asm, backend=emu)
    assert nm.verify() == [] and nm.counts == (0, 0, 0)
    nm.assert_satisfied()
    import sgx_shaped_circuit as sgx
    import zk_dcap_verifier_amd as z
    for census, k in (("chip_estimate", 8), ("reference_exact", 9)):
        cs, fixed, asm, advice = sgx.build(z, emu, k, census=census)
        nm = NativeMockProver.run(k, cs, fixed, advice, [], asm, backend=emu)
        assert nm.counts == (0, 0, 0), census
        assert nm.verify() == []


@pytest.mark.parametrize("what", ["gate", "lookup", "copy", "instance"])
def test_single_corruptions_emulated(emu, what):
    cs, fixed, asm, advice, instances = toy_circuit(6, tamper=what)
    want = MockProver.run(6, cs, fixed, advice, instances, asm).verify()
    nm = NativeMockProver.run(6, cs, fixed, advice, instances, asm, backend=emu)
    assert want and nm.verify() == want
    with pytest.raises(plonk.VerifyFailure) as e:
        nm.assert_satisfied()
    with pytest.raises(plonk.VerifyFailure) as e_host:
        MockProver.run(6, cs, fixed, advice, instances, asm).assert_satisfied()
    assert str(e.value) == str(e_host.value)


def test_truncation_keeps_exact_counts_emulated(emu):
    k, seed = 7, 2
    cs, fixed, asm, advice, instances = random_circuit(k, seed)
    advice = [a.copy() for a in advice]
    _corrupt_lookup(cs, fixed, advice, k, seed)
    nm = NativeMockProver.run(k, cs, fixed, advice, instances, asm, backend=emu)
    full, counts = nm.failures(), nm.counts
    total = sum(counts)
    assert total == len(full) and counts[0] and counts[2]
    for cap in (0, 1, counts[0], total - 1):
        recs, cts = nm._check(cap)
        assert cts == counts
        assert recs == full[:cap]


def test_argument_errors_leave_the_context_usable_emulated(emu):
    cs, fixed, asm, advice, instances = toy_circuit(6, tamper="gate")
    want = MockProver.run(6, cs, fixed, advice, instances, asm).verify()
    nm = NativeMockProver.run(6, cs, fixed, advice, instances, asm, backend=emu)
    args = dict(nm.args)

    def code(**over):
        a = dict(args)
        st = over.pop("struct_size", None)
        a.update(over)
        with pytest.raises(ZkError) as e:
            emu.mock_prover_verify(cap=4, struct_size=st, **a)
        return e.value.code
    assert code(struct_size=C.sizeof(MockDesc) - 8) == ERR_ARG
    bad_map = np.array(asm.map_c, dtype=np.int64)
    bad_map[1, 3] = len(asm.columns)
    assert code(perm_map_column=bad_map) == ERR_ARG
    bad_row = np.array(asm.map_r, dtype=np.int64)
    bad_row[0, 0] = 1 << 6
    assert code(perm_map_row=bad_row) == ERR_ARG
    assert code(advice=[advice[0], None, advice[2]]) == ERR_ARG
    blob = bytearray(args["evaluator_blob"])
    blob[24:28] = (1).to_bytes(4, "little")                          # n_challenges = 1
    assert code(evaluator_blob=bytes(blob)) == ERR_PROGRAM
    lk = bytearray(args["lookup_input_blobs"][0])
    lk[24:28] = (2).to_bytes(4, "little")
    assert code(lookup_input_blobs=[bytes(lk)]) == ERR_PROGRAM
    assert code(n_advice=2) == ERR_ARG                               # the blob's column counts disagree with the descriptor
    # the same context checks a good witness afterwards
    assert nm.verify() == want
    cs, fixed, asm, advice, instances = toy_circuit(6)
    assert NativeMockProver.run(6, cs, fixed, advice, instances, asm, backend=emu).counts == (0, 0, 0)


def test_one_shot_call_returns_what_it_took_emulated(emu):
    """zk_mock_prover_verify checks its witness on a session of its own that ends with the call: whichever way the call returns, no device block stays behind, and
    no handle either"""
    import test_mock_session as tms
    live = C.CDLL(EMU_SO).zk_test_live_device_allocs
    live.restype = C.c_long
    k = 5
    clean, _ = tms.rich(k)
    case, want = tms.rich(k, tms.PLANTS["all"])
    g, l, c = tms.KINDS["all"]
    with tms.open_session(emu, clean) as s:          # the ids a one-shot call that filed its session would draw come after this one
        h0 = s.handle
    nm = NativeMockProver.run(k, case.cs, case.fixed, case.advice, case.instances, case.asm, backend=emu)
    assert nm._check(g + l + c) == (want, (g, l, c))                 # warm-up: the context's own workspaces reach their sizes
    before = live()
    assert NativeMockProver.run(k, clean.cs, clean.fixed, clean.advice, clean.instances, clean.asm, backend=emu)._check(8) == ([], (0, 0, 0))
    assert live() == before
    assert nm._check(g + l + 2) == (want[: g + l + 2], (g, l, c))    # `cap` inside the copy records
    assert live() == before

    def refused(**over):
        with pytest.raises(ZkError) as e:
            emu.mock_prover_verify(cap=4, **dict(nm.args, **over))
        assert e.value.code == ERR_ARG and live() == before
        return str(e.value)
    bad_map = np.array(case.asm.map_c, dtype=np.int64)
    bad_map[1, 3] = len(case.asm.columns)
    assert "copy-mapping entry is out of range" in refused(perm_map_column=bad_map)
    assert "not canonical" in refused(instances=[[R_MOD] + list(nm.instances[0][1:])])
    assert "advice column 1 is NULL" in refused(advice=[nm.advice[0], None] + nm.advice[2:])
    assert nm._check(g + l + c) == (want, (g, l, c)) and live() == before
    for h in range(h0, h0 + 16):
        with pytest.raises(ZkError) as e:
            emu.mock_prover_info(h)
        assert e.value.code == ERR_ARG


def test_rust_mock_structs_match_the_header():
    """mock_native.rs declares zk_mock_desc / zk_mock_failure and zk_mock_prover_verify field for field as include/zkmi355.h"""
    import test_shim_abi as sa
    hdr = open(sa.HEADER).read()
    # the two structs in the typedef form the shared parser reads
    for name in ("zk_mock_desc", "zk_mock_failure"):
        hdr = hdr.replace(f"typedef struct {name} {name};", "")
        hdr = re.sub(r"\bstruct %s \{(.*?)\};" % name, lambda m: "typedef struct %s {%s} %s;" % (name, m.group(1), name), hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "shim", "halo2_proofs_mi355x", "src", "mock_native.rs")).read()
    rs_plain = re.sub(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]", "#[repr(C)]", rs)
    structs, externs, _, _ = sa.parse_rust(rs_plain)
    assert {"ZkMockDesc", "ZkMockFailure"} <= set(structs) and "zk_mock_prover_verify" in externs
    bad = sa.diff_against_header(rs_plain, "mock_native.rs", header_text=hdr + "\n" + open(sa.RCCL_HEADER).read())
    assert not bad, "\n".join(bad)
    hs, _, _ = sa.parse_header(hdr)
    assert [n for n, _ in hs["zk_mock_desc"]] == [n for n, _ in MockDesc._fields_]
    assert [n for n, _ in hs["zk_mock_failure"]] == [n for n, _ in MockFailure._fields_]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(40))
def test_native_mock_prover_matches_dev_py_on_random_circuits_gpu(gpu, seed):
    _differential(gpu, 5 + seed % 6, 1000 + seed)


def _expected_near(k, cs, fixed, advice, asm, gate_rows, lookup_rows, cells):
    """dev.py's per-row logic on the rows the corrupted cells can reach only: gates on gate_rows, lookups on lookup_rows (membership in the full table),
    copies on every (column, row) that is or maps to a corrupted cell"""
    n, u = 1 << k, cs.usable_rows(k)
    ints = {}

    def col(kind, c):
        key = (kind, c)
        if key not in ints:
            ints[key] = (fixed if kind == "f" else advice)[c]
        return ints[key]

    def val(kind, c, row):
        return int(fr_int_array(col(kind, c)[row % n: row % n + 1])[0])
    out = []
    for row in sorted(r for r in set(gate_rows) if 0 <= r < u):
        fx = lambda c, r: val("f", c, row + r)
        ad = lambda c, r: val("a", c, row + r)
        for gi, g in enumerate(cs.gates):
            if ex.evaluate(g, fx, ad, lambda c, r: 0) != 0:
                out.append(f"gate {gi} not satisfied on row {row}")
    for li, lk in enumerate(cs.lookups):
        tcols = []
        for e in lk.table_expressions:
            assert isinstance(e, plonk.Fixed) and e.rotation == 0
            tcols.append(np.ascontiguousarray(fixed[e.column][:u]))
        table = set(np.concatenate(tcols, axis=1).view(np.dtype((np.void, 32 * len(tcols)))).reshape(-1).tolist())
        for row in sorted(r for r in set(lookup_rows) if 0 <= r < u):
            fx = lambda c, r: val("f", c, row + r)
            ad = lambda c, r: val("a", c, row + r)
            tup = b"".join(fr_mont(ex.evaluate(e, fx, ad, lambda c, r: 0)).tobytes() for e in lk.input_expressions)
            if tup not in table:
                out.append(f"lookup {li}: input of row {row} is not in the table")
    hits = set()
    for (j, row) in cells:
        hits.add((j, row))
        for jj, rr in zip(*np.nonzero((asm.map_c == j) & (asm.map_r == row))):
            hits.add((int(jj), int(rr)))
    for j, row in sorted(hits):
        cj, rj = int(asm.map_c[j, row]), int(asm.map_r[j, row])
        if (cj, rj) != (j, row):
            t, i = asm.columns[j]
            t2, i2 = asm.columns[cj]
            a = (advice if t == plonk.ADVICE else fixed)[i][row]
            b = (advice if t2 == plonk.ADVICE else fixed)[i2][rj]
            if not np.array_equal(a, b):
                out.append(f"copy constraint violated: column {j} row {row} != column {cj} row {rj}")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_sgx_shaped_k19_satisfied_then_three_corruptions_gpu(gpu, on_device):
    import sgx_shaped_circuit as sgx
    import zk_dcap_verifier_amd as z
    k = 19
    cs, fixed, asm, advice = sgx.build(z, gpu, k)
    fixed = [np.ascontiguousarray(c) for c in fixed]
    advice = [np.ascontiguousarray(c).copy() for c in advice]

    def check(adv):
        if not on_device:
            return NativeMockProver.run(k, cs, fixed, adv, [], asm, backend=gpu)
        return NativeMockProver.run(k, cs, [gpu.to_device(c) for c in fixed], [gpu.to_device(c) for c in adv], [], asm, backend=gpu)
    assert check(advice).counts == (0, 0, 0)
    G = sgx.N_GATE_COLS
    sel_of = {g % G: sgx.N_TABLE_COLS + g % (sgx.N_FIXED - sgx.N_TABLE_COLS) for g in range(sgx.N_GATES)}
    blk = next(b for b in range(10, 1000) if int(fr_int_array(fixed[sel_of[3]][4 * b: 4 * b + 1])[0]) == 1)
    d_row = 4 * blk + 3
    advice[3][d_row] = fr_mont((int(fr_int_array(advice[3][d_row: d_row + 1])[0]) + 1) % R_MOD)        # a block's d cell
    lk_sel = sgx.N_TABLE_COLS + 4 % (sgx.N_FIXED - sgx.N_TABLE_COLS)                                 # lookup 4 reads advice G + 4 where its selector is on
    lk_col, lk_row = G + 4, next(4 * b for b in range(200, 2000) if int(fr_int_array(fixed[lk_sel][4 * b: 4 * b + 1])[0]) == 1)
    advice[lk_col][lk_row] = fr_mont(1 << 16)                                                          # a 16-bit lookup cell set to 2^16
    b_row = 4 * (blk + 5) + 1
    advice[6][b_row] = fr_mont(12345)                                                                  # a shared b cell (copied to column 7)
    nm = check(advice)
    want = _expected_near(k, cs, fixed, advice, asm, gate_rows=[d_row - r for r in range(4)] + [b_row - r for r in range(4)],
                          lookup_rows=[lk_row], cells=[(3, d_row), (6, b_row)])
    assert want and _kinds(want)[1] == 1 and _kinds(want)[2] == 2
    assert nm.verify() == want
    assert nm.counts == _kinds(want)
