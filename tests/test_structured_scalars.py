"""The MSM on STRUCTURED scalars (scalar_cases.scalar_column): columns chosen per window width c whose every row is an edge of the signed-digit recoding or of the
bucket reduction.  On uniform scalars — what every other MSM test draws, next to 0, 1, r - 1 and bytes — a window meets the digit 2^(c-1) (the last positive one),
2^(c-1) + 1 (the first negative one) or 2^c (magnitude 0, nothing emitted, the carry goes on) with probability 2^-c, a carry never runs through every window into the
top one, and at c >= 17 the top bucket B - 1 — alone in row n_hi - 1 of the weight matrix, the only member of the class the host's fold starts from — is empty as often
as not.  So the four copies of the recoder in msm.hip may disagree with each other, and n_hi, `w <= B` or the start of the Horner fold may be off by one, without a test
noticing.  Here every row is such a case, over tables whose every bucket holds something different, at EVERY window width (3 .. 22 on the GPU, 3 .. 18 and 20 on the
emulator) and under both sorts.  Every MSM is compared bit for bit, over all 12 limbs, with the oracle's best_multiexp AND with the closed form [sum s_i k_i] G.
Emulator (CPU, a few hundred rows) and product C ABI on the GPU."""
import pytest

import scalar_cases as scs
import zk_dcap_verifier_amd as z

EMU_C = tuple(range(3, 19)) + (20,)
HEAVY = ("top_bucket_heavy", "half_digits", "half_plus_one", "mixed_edges")         # whole columns in one or two edge buckets: what meets the doubling / cancelling branches


def _sorts(c, chunk):
    """the plans of a width: both sorts up to 16 bits (wider windows always take the two-level sort), bins cut into chunks"""
    return [dict(msm_two_level_sort=t, msm_bsort_chunk=chunk if t else 8192) for t in ((0, 1) if c <= 16 else (1,))]


def _restore(be):
    be.tune(msm_c=0, msm_two_level_sort=0, msm_bsort_chunk=8192)


def _rows(c, small, large):
    return small if c >= 19 else large


# ---- every kind at every width, both sorts, both entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EMU_C)
def test_emulated_scalar_kinds(emu, orc, pyref, c):
    n = _rows(c, 64, 100)
    try:
        for i, plan in enumerate(_sorts(c, 64)):
            scs.check_kinds(emu, orc, pyref, c, n, plan, seed=c, limit=n, entries=(("host",), ("dev",))[(c + i) % 2])
    finally:
        _restore(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("c", scs.ALL_C)
def test_gpu_scalar_kinds(gpu, orc, pyref, c):
    try:
        for plan in _sorts(c, 256):
            assert scs.check_kinds(gpu, orc, pyref, c, 3000, plan, seed=c) >= 3000
    finally:
        _restore(gpu)


# ---- the heavy edge buckets over tables of equal and opposite points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EMU_C)
def test_emulated_edge_buckets_on_structured_tables(emu, orc, pyref, c):
    """all_equal: the last bucket holds every pair, all references to ONE point (every chain doubles, equal partial sums meet in the merge rounds); few: +-[1..4] G"""
    n = _rows(c, 64, 80)
    try:
        plan = _sorts(c, 64)[-1 if c % 2 else 0]
        for bkind in ("all_equal", "few") if c <= 17 else (("few", "all_equal")[c % 4 == 0],):      # (2^17 buckets and more: seconds per MSM here, so one table each)
            scs.check_kinds(emu, orc, pyref, c, n, plan, bkind=bkind, kinds=HEAVY, seed=c + 40, entries=("dev",))
    finally:
        _restore(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("c", scs.ALL_C)
def test_gpu_edge_buckets_on_structured_tables(gpu, orc, pyref, c):
    try:
        for plan in _sorts(c, 256):
            for bkind in ("all_equal", "few"):
                scs.check_kinds(gpu, orc, pyref, c, 3000, plan, bkind=bkind, kinds=HEAVY, seed=c + 40, entries=("dev",))
    finally:
        _restore(gpu)


# ---- batches: msm_rowcol_kernel<16> (four columns and more) and <64> (fewer) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (4, 11, 16, 17))
def test_emulated_scalar_batches(emu, orc, pyref, c):
    try:
        scs.check_batch(emu, orc, pyref, c, 64, ("half_digits", "carry_to_top", "bucket_sweep", "top_bucket_heavy", "mixed_edges"), {}, limit=64)
        scs.check_batch(emu, orc, pyref, c, 64, ("top_bucket_heavy", "edge_digit_each_window"), {}, bkind="few")
    finally:
        _restore(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("c", scs.ALL_C)
def test_gpu_scalar_batches(gpu, orc, pyref, c):
    try:
        for plan in _sorts(c, 256):
            scs.check_batch(gpu, orc, pyref, c, 3000, scs.SCALAR_KINDS, plan, limit=3000)
            scs.check_batch(gpu, orc, pyref, c, 2500, ("top_bucket_heavy", "mixed_edges"), plan, bkind="few" if c % 2 else "all_equal")
    finally:
        _restore(gpu)


# ---- one scalar for every bucket -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", (16, 17))
def test_gpu_full_bucket_sweep(gpu, orc, pyref, c):
    """0 .. 2^c - 1 in window 0 over 2^c different points: every bucket holds exactly one positive and (below B) one negative reference, its own"""
    try:
        gpu.tune(msm_c=c)
        col = scs.scalar_column(orc, pyref, 0, "bucket_sweep", c, seed=c, full=True)
        assert col.shape[0] == 1 << c
        table = scs.arith_bases(orc, pyref, 1 << c, seed=c)
        h = z.arithmetic.BasesHandle(gpu, table[0])
        try:
            scs.check_on_handle(gpu, orc, pyref, h, table, col, what=("full sweep", c))
        finally:
            h.release()
    finally:
        _restore(gpu)


# ---- prefixes, partial sums, the run-length path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (7, 16, 17))
def test_emulated_prefix_partials(emu, orc, pyref, c):
    try:
        scs.check_prefix(emu, orc, pyref, c, 60)
        scs.check_partials(emu, orc, pyref, c, 60)
    finally:
        _restore(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("c", (5, 12, 16, 17, 20, 22))
def test_gpu_prefix_partials(gpu, orc, pyref, c):
    try:
        scs.check_prefix(gpu, orc, pyref, c, 4000)
        scs.check_prefix(gpu, orc, pyref, c, 4000, bkind="few", skind="top_bucket_heavy")
        scs.check_partials(gpu, orc, pyref, c, 4000)
        scs.check_partials(gpu, orc, pyref, c, 3000, bkind="all_equal", skind="half_plus_one")
    finally:
        _restore(gpu)


@pytest.mark.parametrize("c", (16, 17))
def test_emulated_run_length_path(emu, orc, pyref, c):
    try:
        scs.check_runs(emu, orc, pyref, c, 1100)                       # (the run path needs 1024 rows)
    finally:
        _restore(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("c", (6, 14, 16, 17, 20))
def test_gpu_run_length_path(gpu, orc, pyref, c):
    try:
        scs.check_runs(gpu, orc, pyref, c, 6000)
        scs.check_runs(gpu, orc, pyref, c, 5000, bkind="all_equal")
    finally:
        _restore(gpu)


# ---- the input helpers themselves (no kernel) ----------------------------------------------------------------------------------------------------------------
def test_every_kind_has_values_at_every_width(orc, pyref):
    """no (kind, c) pair is empty or filtered away for c in 3 .. 22 (the helpers assert each kind's property on the integer side)"""
    for c in scs.ALL_C:
        for kind in scs.SCALAR_KINDS:
            col = scs.scalar_column(orc, pyref, 40, kind, c, seed=c, limit=60)
            assert col.shape[0] >= (40 if kind != "bucket_sweep" else 16) and col.any(), (kind, c)
        top = scs.signed_digits(scs.top_bucket_value(pyref.R, c), c)
        assert top == [1 << (c - 1)] * (scs.windows(c) - 1) + [0]
