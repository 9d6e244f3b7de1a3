"""NTT parity on the shipped radices (tests/ntt_cases.py): every size, every forced plan, every fused form, the cosets and both launch orders, each on the emulator
(a backend of its own, every ntt_* tunable at the library's default) and on the GPU, bit for bit against the oracle.

The emulator stops at 2^20 (EMU_MAX_LOG): its slowest cases there, coeff_to_extended of three columns with ntt_quarter_input 1 and 0, take 13.6 s, and twice the
size would pass the 20 s a case may take on it.  What that leaves to the GPU twin alone: section A at 2^21, the four forced plans at 2^21 (488 at 2^20 stays), the
fused forms (19, 21) and (15, 21), the coset case (19, 2).  Every pass geometry (role, r, c_log) of the default plan still runs on the emulator (the census test)."""
import ctypes as C

import pytest

import ntt_cases as nc
import zk_dcap_verifier_amd as z
from conftest import EMU_SO

EMU_MAX_LOG = 20
GPU_CASES = nc.matrix()
EMU_CASES = nc.matrix(EMU_MAX_LOG)
by_section = lambda cases, s: [c for c in cases if c.section == s]


@pytest.fixture(scope="module")
def emu_default(built):
    """the emulator under the library's own tunables: the plan the product runs (conftest's `emu` is tuned down to a 2^6 tile and radix 2^4)"""
    be = z.Backend(0, lib_path=EMU_SO)
    try:
        assert "EMULATED" in be.version()
        assert all(be.tune_get(k) == v for k, v in nc.DEFAULT_TUNE.items()), "ntt_cases.DEFAULT_TUNE is not the library's default"
        yield be
    finally:
        be.close()


def _library_plan(be, log_n):
    rl, passes = (C.c_uint32 * 3)(), C.c_int()
    assert be.lib.zk_test_ntt_plan(be.ctx, C.c_uint32(log_n), rl, C.byref(passes)) == 0
    return list(rl), passes.value


# the default plan, every ntt_plan of the matrix, one plan that fits no size, and the tile / radix pairs the other emulator tests run under
PLAN_TUNES = [{}] + [dict(ntt_plan=p) for p in sorted({p for _, p in nc.FORCED})] + [dict(ntt_plan=990), dict(ntt_plan=80)] + \
    [dict(ntt_tile_log=t, ntt_max_radix_log=r) for t, r in ((6, 4), (4, 2), (5, 5), (8, 3), (10, 5), (11, 11), (12, 10), (12, 6))]


@pytest.mark.parametrize("tune", PLAN_TUNES, ids=lambda t: "-".join("%s%d" % (k[4:], v) for k, v in t.items()) or "default")
def test_plan_restatement_matches_the_library(emu_default, tune):
    """ntt_cases.radices against plan_passes itself (zk_test_ntt_plan of the emulator build), log n = 0 .. 27"""
    with nc.tuned(emu_default, **tune):
        for log_n in range(28):
            assert _library_plan(emu_default, log_n) == nc.radices(log_n, tune), (log_n, tune)


def test_forced_plans_are_taken():
    """every ntt_plan of section B fits its size (a plan that does not fit falls back to the balanced radices without a word)"""
    for log_n, p in nc.FORCED:
        assert nc.radices(log_n, dict(ntt_plan=p)) == ([p // 100, p // 10 % 10, p % 10], 3)
        assert nc.radices(log_n, dict(ntt_plan=p)) != nc.radices(log_n)


def test_default_plan_geometries_are_the_documented_ones():
    """the restated geometry at the sizes of the headline circuits (k = 19: 2^19 and 2^21; k = 21: 2^21 and 2^23), written out"""
    g = lambda log_n: [(p.role, p.r, p.c_log) for p in nc.plan(log_n)]
    assert g(7) == [("only", 7, 0)] and g(9) == [("first", 5, 4), ("last", 4, 5)] and g(16) == [("first", 8, 2), ("last", 8, 2)]
    assert g(19) == [("first", 7, 3), ("mid", 6, 4), ("last", 6, 4)] and g(21) == [("first", 7, 3), ("mid", 7, 3), ("last", 7, 3)]
    assert g(23) == [("first", 8, 2), ("mid", 8, 2), ("last", 7, 3)]
    assert [(p.limbs29, p.q_log, p.p_log) for p in nc.plan(23)] == [(True, 0, 0), (True, 0, 0), (False, 8, 8)]


def test_census_matrix_reaches_every_default_geometry():
    """at sizes <= 2^21 the matrix runs every (role, r, c_log) the default plan has for log n = 0 .. 24 — those of 2^22 .. 2^24 through ntt_plan — and every one of
    them on the emulator too.  The last passes' (r, q_log, p_log) of 2^22 .. 2^24 cannot be had below 2^22 (r + q_log + p_log = log n): they are printed, not hidden."""
    assert all(log_n <= nc.MAX_LOG for c in GPU_CASES for log_n, _ in nc.transforms(c))
    want, got, got_emu = nc.default_census(0, 24), nc.census(GPU_CASES), nc.census(EMU_CASES)
    assert len(want["geometries"]) == 22
    assert want["geometries"] <= got["geometries"], sorted(want["geometries"] - got["geometries"])
    assert want["geometries"] <= got_emu["geometries"], sorted(want["geometries"] - got_emu["geometries"])
    only_large = nc.default_census(22, 24)["geometries"] - nc.default_census(0, 21)["geometries"]
    assert only_large == {("mid", 8, 2)}                                   # (first, 8, 2) is 2^15's, (last, 8, 2) 2^16's
    unreached = sorted(want["last"] - got["last"])
    print("last passes (r, q_log, p_log) of the default plan the matrix does not run:", unreached)
    assert unreached == [(7, 8, 7), (7, 8, 8), (8, 8, 8)]                  # 2^22, 2^23, 2^24
    assert {(q, p) for _, q, p in unreached} <= {(q, p) for _, q, p in got["last"]}      # their digit ranges (q_log, p_log) are run, under other radices (876, 885)
    assert sorted(want["last"] - got_emu["last"]) == [(7, 7, 7)] + unreached                # the emulator stops at 2^20: 2^21's last pass is the GPU twin's alone


def test_matrix_covers_what_the_sections_promise():
    """the lists of ntt_cases, counted: a dropped size or form fails here, not silently"""
    A = by_section(GPU_CASES, "A")
    assert {(c.k, c.inverse, c.batch) for c in A} == {(k, i, b) for k in range(22) for i in (False, True) for b in (False, True)}
    pairs = {(c.k, c.ek) for c in GPU_CASES if c.form == "c2e"}
    assert {ek for _, ek in pairs} >= set(range(1, 17)) | {19, 20, 21} and {(14, 16), (13, 15), (19, 21), (0, 2), (1, 3)} <= pairs
    for first_r in (5, 6, 7, 8):                                           # every difference 0, 1, 2, 3, 6 meets every first-pass radix
        assert {ek - k for k, ek in pairs if nc.plan(ek)[0].r == first_r} >= {0, 1, 2, 3, 6}, first_r
    assert {ek - k for k, ek in pairs if ek > 16} >= {1, 2, 3, 6}
    assert {c.k for c in GPU_CASES if c.form == "lagrange"} == set(range(1, 17)) | {19}
    assert {c.ek - c.k for c in GPU_CASES if c.form == "div"} == set(range(1, 7))
    cos = {(c.k, c.ek - c.k) for c in GPU_CASES if c.form == "coset"}
    assert {e for _, e in cos} == {1, 2, 3, 6} and (19, 2) in cos and max(k for k, _ in cos if k != 19) == 14
    for lo, hi in ((1, 8), (9, 10), (11, 14)):
        assert {e for k, e in cos if lo <= k <= hi} >= {1, 6}, (lo, hi)
    E = by_section(GPU_CASES, "E")
    assert all(c.batch and c.col_major == 0 for c in E) and {c.ek for c in E} == set(nc.LAUNCH_ORDER_LOGS)
    assert len(E) == len([c for c in GPU_CASES if c.section in "AC" and c.batch and c.ek in nc.LAUNCH_ORDER_LOGS])


def _parametrize(cases, section):
    return pytest.mark.parametrize("case", by_section(cases, section), ids=nc.case_id)


@_parametrize(EMU_CASES, "A")
def test_emulated_every_size(emu_default, orc, pyref, case):
    nc.run(case, emu_default, orc, pyref)


@_parametrize(EMU_CASES, "B")
def test_emulated_forced_plans(emu_default, orc, pyref, case):
    nc.run(case, emu_default, orc, pyref)


@_parametrize(EMU_CASES, "C")
def test_emulated_fused_forms(emu_default, orc, pyref, case):
    nc.run(case, emu_default, orc, pyref)


@_parametrize(EMU_CASES, "D")
def test_emulated_cosets_against_the_oracle(emu_default, orc, pyref, case):
    nc.run(case, emu_default, orc, pyref)


@_parametrize(EMU_CASES, "E")
def test_emulated_launch_order(emu_default, orc, pyref, case):
    nc.run(case, emu_default, orc, pyref)


@pytest.mark.gpu
@_parametrize(GPU_CASES, "A")
def test_gpu_every_size(gpu, orc, pyref, case):
    nc.run(case, gpu, orc, pyref)


@pytest.mark.gpu
@_parametrize(GPU_CASES, "B")
def test_gpu_forced_plans(gpu, orc, pyref, case):
    nc.run(case, gpu, orc, pyref)


@pytest.mark.gpu
@_parametrize(GPU_CASES, "C")
def test_gpu_fused_forms(gpu, orc, pyref, case):
    nc.run(case, gpu, orc, pyref)


@pytest.mark.gpu
@_parametrize(GPU_CASES, "D")
def test_gpu_cosets_against_the_oracle(gpu, orc, pyref, case):
    nc.run(case, gpu, orc, pyref)


@pytest.mark.gpu
@_parametrize(GPU_CASES, "E")
def test_gpu_launch_order(gpu, orc, pyref, case):
    nc.run(case, gpu, orc, pyref)
