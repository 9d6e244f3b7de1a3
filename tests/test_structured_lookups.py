"""permute_expression_pair on STRUCTURED lookups (lookup_cases): key windows at every word and bit offset, every pass count, digit patterns laid out per wave of
the histogram, ties refined in one, two and three stages, sizes on and around the sort and scan tiles, the multiset shapes of halo2's rule, values the table does not
hold, and what a context remembers between calls.  lookupperm.hip decides all of that from the data; on the random values of test_lookup_permute.py it decides the
same way every time.  Every result is compared on all n x 4 limbs of both columns, bit for bit, with oracle.lookup_permute, which is itself held against
lookup_cases.rule (halo2's rule in plain Python) on every case.  Three levels: the references alone (no device), the kernel emulator (k = 5, and k = 9 where a kind
needs the rows), the product C ABI on the GPU."""
import pytest

import lookup_cases as lc
import zk_dcap_verifier_amd as z

ALONE = tuple(L for L in lc.BIT_LENGTHS if L <= 64)                         # one column width per call: the pass counts 1 .. 8
WIDE = tuple(L for L in lc.BIT_LENGTHS if L > 64)


def _emu_tuned(emu):
    emu.tune(vec_block=64)


def _emu_restore(emu):
    emu.tune(vec_block=32)


# ---- the references alone: oracle.lookup_permute against rule() on every kind (lc.prepare asserts it) ------------------------------------------------------------
def test_oracle_bit_lengths(orc, pyref):
    for L in lc.BIT_LENGTHS:
        case = lc.bit_length(pyref.R, 6, 5, (L,), seed=L)
        if L <= 64:
            assert lc.passes(case) == lc.PASSES_OF[L]
        lc.prepare(orc, pyref, case, seed=L)
    assert sorted(set(lc.PASSES_OF.values())) == list(range(1, 9))
    lc.prepare(orc, pyref, lc.bit_length(pyref.R, 6, 5, (8, 64, 254)))


def test_oracle_digit_patterns(orc, pyref):
    for p in lc.DIGIT_PASSES:
        lc.prepare(orc, pyref, lc.digit_pattern(9, 5, p))
    lc.digit_pattern(13, 5, 7)                                              # (the property asserts at the GPU size: a partial last wave, a partial last tile)
    assert lc.usable(13, 5) % 64 and lc.usable(13, 5) % lc.SORT_TILE


def test_oracle_ties(orc, pyref):
    assert sorted({lc.stages(lo, hi) for lo, hi, _ in lc.TIE_RANGES}) == [1, 2, 3]
    assert any(hi == s - 1 for _, hi, s in lc.TIE_RANGES)
    lc.prepare(orc, pyref, lc.ties(pyref.R, 7, 5))
    lc.prepare(orc, pyref, lc.ties(pyref.R, 7, 5, ((0, 63, 100), (3, 188, 190)), seed=3, some_groups=True))
    lc.prepare(orc, pyref, lc.straddle(pyref.R, 13, 5))


def test_oracle_multisets(orc, pyref):
    for kind in lc.MULTISET_KINDS:
        for k, bf in ((6, 5), (1, 0)):
            lc.prepare(orc, pyref, lc.multiset(pyref.R, k, bf, kind))


def test_oracle_refuses_what_the_table_does_not_hold(orc, pyref):
    for kind in lc.NOT_IN_TABLE_KINDS:
        case = lc.not_in_table(pyref.R, 6, 5, kind)
        with pytest.raises(ValueError):
            lc.prepare(orc, pyref, case)
        lc.prepare(orc, pyref, lc.good_twin(case))


def test_oracle_sizes(orc, pyref):
    for k, bf in lc.SMALL_SIZES + lc.TILE_SIZES:
        lc.prepare(orc, pyref, lc.sized(pyref.R, k, bf))
    assert [lc.usable(k, bf) for k, bf in lc.TILE_SIZES] == [2048, 4096, 4097, 4095, 8191, 6144, 8192]


def test_oracle_batches_and_hint_sequences(orc, pyref):
    lc.prepare(orc, pyref, lc.shared_table_batch(pyref.R, 6, 5, 11))
    lc.prepare(orc, pyref, lc.shared_table_batch(pyref.R, 6, 5, 6, tables=2))
    for _, case, _, _ in lc.hint_steps(pyref.R, 9, 5) + lc.hint_steps_digit_edge(pyref.R, 9, 5) + lc.swap_steps(pyref.R, 9, 5):
        lc.prepare(orc, pyref, case)


def test_rule_is_halo2s_rule():
    """known answers, by hand: first occurrences take their own value; the leftovers 1, 5, 5 go to the repeated rows 4, 2, 1 (the last one first)"""
    pin, ptab = lc.rule([3, 2, 3, 3, 9, 3], [9, 5, 3, 2, 5, 1], 6)
    assert pin == [2, 3, 3, 3, 3, 9] and ptab == [2, 3, 5, 5, 1, 9]
    with pytest.raises(ValueError):
        lc.rule([3, 4], [3, 3], 2)
    assert lc.rule([7], [7], 1) == ([7], [7])


# ---- the emulator: the same kernel sources on CPU threads (every work-item is a thread: k = 5, k = 9 for the kinds that need rows) -------------------------------
# The tile-edge sizes (u = 2048 .. 8192) and `straddle` (u > 4096) are GPU only: thousands of rows are out of the emulator's reach.  The wave aggregation of the
# histogram does not exist in the emulator build; the digit patterns run here for the scatter.
@pytest.mark.parametrize("Ls", [ALONE[:4], ALONE[4:8], ALONE[8:], WIDE[:5], WIDE[5:10], WIDE[10:]], ids=lambda Ls: "L%d_%d" % (Ls[0], Ls[-1]))
def test_emulated_bit_lengths(emu, orc, pyref, Ls):
    _emu_tuned(emu)
    try:
        if Ls[0] <= 64:
            for L in Ls:                                                    # alone in a call
                lc.run(emu, orc, pyref, lc.bit_length(pyref.R, 5, 5, (L,), seed=L), seed=L, entries=(("single",), ("batch",))[L % 2])
        else:
            lc.run(emu, orc, pyref, lc.bit_length(pyref.R, 5, 5, Ls, seed=Ls[0]), seed=Ls[0])
    finally:
        _emu_restore(emu)


def test_emulated_bit_lengths_mixed(emu, orc, pyref):
    """a narrow column sorted under a wide call's pass count"""
    _emu_tuned(emu)
    try:
        lc.run(emu, orc, pyref, lc.bit_length(pyref.R, 5, 5, (8, 64, 254)))
    finally:
        _emu_restore(emu)


@pytest.mark.parametrize("p", lc.DIGIT_PASSES)
def test_emulated_digit_patterns(emu, orc, pyref, p):
    _emu_tuned(emu)
    try:
        lc.run(emu, orc, pyref, lc.digit_pattern(5, 5, p))
        lc.run(emu, orc, pyref, lc.digit_pattern(9, 5, p, ("mod256", "distinct64")), entries=("batch",))      # more than one run of 64 rows
    finally:
        _emu_restore(emu)


@pytest.mark.parametrize("some_groups", (False, True), ids=("all_groups", "some_groups"))
def test_emulated_ties(emu, orc, pyref, some_groups):
    _emu_tuned(emu)
    try:
        emu.timing(True)
        case = lc.ties(pyref.R, 5 if not some_groups else 6, 5, seed=int(some_groups), some_groups=some_groups)
        lc.run(emu, orc, pyref, case, entries=("batch",))
        assert emu.stat_get("lookup_refined_sorts") + emu.stat_get("lookup_hinted_sorts") >= 2 * len(lc.TIE_RANGES)
        for i in (0, 7):                                                    # one and three stages through the single entry
            emu.timing(True)
            lc.run(emu, orc, pyref, lc.Case(case.k, case.bf, [case.inputs[i]], [case.tables[i]], [0]), entries=("single",))
            assert emu.stat_get("lookup_refined_sorts") + emu.stat_get("lookup_hinted_sorts") >= 2
    finally:
        emu.timing(False)
        _emu_restore(emu)


@pytest.mark.parametrize("kind", lc.MULTISET_KINDS)
def test_emulated_multisets(emu, orc, pyref, kind):
    _emu_tuned(emu)
    try:
        lc.run(emu, orc, pyref, lc.multiset(pyref.R, 5, 5, kind))
    finally:
        _emu_restore(emu)


@pytest.mark.parametrize("kind", lc.NOT_IN_TABLE_KINDS)
def test_emulated_not_in_table(emu, orc, pyref, kind):
    _emu_tuned(emu)
    try:
        lc.run_refused(emu, orc, pyref, lc.not_in_table(pyref.R, 5, 5, kind))
    finally:
        _emu_restore(emu)


@pytest.mark.parametrize("k,bf", lc.SMALL_SIZES)
def test_emulated_sizes(emu, orc, pyref, k, bf):
    _emu_tuned(emu)
    try:
        lc.run(emu, orc, pyref, lc.sized(pyref.R, k, bf))
    finally:
        _emu_restore(emu)


def test_emulated_batch_shapes(emu, orc, pyref):
    _emu_tuned(emu)
    try:
        lc.run(emu, orc, pyref, lc.shared_table_batch(pyref.R, 5, 5, 11))             # the sgx circuit's shape: 11 lookups, one table
        lc.run(emu, orc, pyref, lc.shared_table_batch(pyref.R, 5, 5, 6, tables=2))
        lc.run(emu, orc, pyref, lc.sized(pyref.R, 5, 5), entries=("batch",))          # count = 1 through the batch entry
    finally:
        _emu_restore(emu)


# ---- what a context remembers between calls: on a context of its own, so that the path of every step is known ------------------------------------------------------
def _hint_sequence(be, orc, pyref, steps):
    for name, case, refined, hinted in steps:
        be.timing(True)                                                     # (clears the statistics)
        lc.run(be, orc, pyref, case, entries=("batch",))
        got = (be.stat_get("lookup_refined_sorts"), be.stat_get("lookup_hinted_sorts"))
        assert got == (refined, hinted), (name, "refined, hinted columns", got, "expected", (refined, hinted))


def test_emulated_hint_state(built, orc, pyref):
    from conftest import EMU_SO
    for steps in (lc.hint_steps, lc.hint_steps_digit_edge, lc.swap_steps):
        be = z.Backend(0, lib_path=EMU_SO)
        be.tune(vec_block=64)
        try:
            _hint_sequence(be, orc, pyref, steps(pyref.R, 9, 5))
        finally:
            be.close()


@pytest.mark.gpu
def test_gpu_hint_state(gpu, orc, pyref):
    for k in (9, 13):
        for steps in (lc.hint_steps, lc.hint_steps_digit_edge, lc.swap_steps):
            be = z.Backend(0)
            try:
                _hint_sequence(be, orc, pyref, steps(pyref.R, k, 5))
            finally:
                be.close()


# ---- the GPU, through the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def _refined(gpu):
    # which of the two moved depends on what earlier tests left in the shared context
    return gpu.stat_get("lookup_refined_sorts") + gpu.stat_get("lookup_hinted_sorts")


@pytest.mark.gpu
@pytest.mark.parametrize("L", ALONE)
def test_gpu_bit_length_alone(gpu, orc, pyref, L):
    """one column width per call: 1 .. 8 radix passes, the result in either half of the ping-pong buffers"""
    case = lc.bit_length(pyref.R, 13, 5, (L,), seed=L)
    assert lc.passes(case) == lc.PASSES_OF[L]
    lc.run(gpu, orc, pyref, case, seed=L)


@pytest.mark.gpu
@pytest.mark.parametrize("Ls", [WIDE[:5], WIDE[5:10], WIDE[10:], (8, 64, 254), lc.BIT_LENGTHS], ids=lambda Ls: "L%d_%d_x%d" % (Ls[0], Ls[-1], len(Ls)))
def test_gpu_bit_lengths(gpu, orc, pyref, Ls):
    """windows at every word offset with bit offsets 0, 1 and 31; (8, 64, 254): a narrow column under a wide call's pass count"""
    lc.run(gpu, orc, pyref, lc.bit_length(pyref.R, 12, 5, Ls, seed=len(Ls)), entries=("batch",))
    for L in Ls[:: max(1, len(Ls) // 3)]:
        lc.run(gpu, orc, pyref, lc.bit_length(pyref.R, 12, 5, (L,), seed=L), seed=L, entries=("single",))


@pytest.mark.gpu
@pytest.mark.parametrize("p", lc.DIGIT_PASSES)
def test_gpu_digit_patterns(gpu, orc, pyref, p):
    """u = 8186: 127 full waves and one of 58 lanes, one full sort tile and a partial one"""
    case = lc.digit_pattern(13, 5, p)
    prepared = lc.prepare(orc, pyref, case)
    lc.run(gpu, orc, pyref, case, entries=("batch",), prepared=prepared)
    for i in range(len(case.inputs)):
        one = lc.Case(case.k, case.bf, [case.inputs[i]], [case.tables[i]], [0])
        lc.run(gpu, orc, pyref, one, entries=("single",), prepared=(prepared[0], prepared[1][i:i + 1], prepared[2][i:i + 1], prepared[3][i:i + 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("k,some_groups", [(10, False), (13, False), (12, True)])
def test_gpu_ties(gpu, orc, pyref, k, some_groups):
    gpu.timing(True)
    try:
        case = lc.ties(pyref.R, k, 5, seed=k, some_groups=some_groups)
        lc.run(gpu, orc, pyref, case, entries=("batch",))
        assert _refined(gpu) >= 2 * len(lc.TIE_RANGES)
        for i in range(len(case.inputs)):
            gpu.timing(True)
            lc.run(gpu, orc, pyref, lc.Case(case.k, case.bf, [case.inputs[i]], [case.tables[i]], [0]), entries=("single",))
            assert _refined(gpu) >= 2, lc.TIE_RANGES[i]
    finally:
        gpu.timing(False)


@pytest.mark.gpu
def test_gpu_tie_straddles_a_sort_tile(gpu, orc, pyref):
    gpu.timing(True)
    try:
        lc.run(gpu, orc, pyref, lc.straddle(pyref.R, 13, 5))
        assert _refined(gpu) >= 2
    finally:
        gpu.timing(False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", lc.MULTISET_KINDS)
def test_gpu_multisets(gpu, orc, pyref, kind):
    for k, bf in ((13, 5), (9, 0)):
        lc.run(gpu, orc, pyref, lc.multiset(pyref.R, k, bf, kind, seed=k))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", lc.NOT_IN_TABLE_KINDS)
def test_gpu_not_in_table(gpu, orc, pyref, kind):
    lc.run_refused(gpu, orc, pyref, lc.not_in_table(pyref.R, 13, 5, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("k,bf", lc.SMALL_SIZES + lc.TILE_SIZES)
def test_gpu_sizes(gpu, orc, pyref, k, bf):
    gpu.timing(True)
    try:
        lc.run(gpu, orc, pyref, lc.sized(pyref.R, k, bf))
        if lc.usable(k, bf) >= 16:
            assert _refined(gpu) >= 1
    finally:
        gpu.timing(False)


@pytest.mark.gpu
@pytest.mark.parametrize("lookups,tables", [(11, 1), (6, 2), (1, 1)])
def test_gpu_batch_shapes(gpu, orc, pyref, lookups, tables):
    lc.run(gpu, orc, pyref, lc.shared_table_batch(pyref.R, 13, 5, lookups, tables), entries=("batch",))
