"""The elliptic-curve kernels on STRUCTURED points (point_cases.structured_bases): one point on every row, P / -P alternating, a few small multiples of G, pairs, tables
that are mostly identities.  On an arithmetic progression of distinct generic points — what every other EC test runs on — the group law's exceptional cases (P + P,
P + (-P), identity operands) almost never happen, so the hand-off of msm_accumulate_kernel from the carry-free chain to the complete one, the doubling and cancellation
branches of xyzz_madd_lazy / xyzz_add_lazy in every reduction level, the host fold, the prefix-sum table of the run-length path, the butterflies of the G1 NTT and the
all-identity chunks of the affine conversion can be wrong without a test noticing.  Here they happen on every row.  Every MSM is compared bit for bit, over all 12 limbs,
with the oracle's best_multiexp AND with the closed form [sum s_i k_i] G.  Emulator (CPU, a few hundred rows) and product C ABI on the GPU."""
import numpy as np
import pytest

import point_cases as ptc

PLAN_C = (3, 8, 13, 16, 17, 20)
MSM_PAIRS = [("all_equal", "ones"), ("all_equal", "paired"), ("all_equal", "uniform"), ("alt_neg", "ones"), ("alt_neg", "paired"), ("alt_neg", "minus_one"),
             ("few", "uniform"), ("few", "ones"), ("few", "byte"), ("few", "one_digit"), ("small_multiples", "ones"), ("small_multiples", "witness"),
             ("pairs", "paired"), ("pairs", "neg_paired"), ("neg_pairs", "paired"), ("neg_pairs", "neg_paired"), ("identity_heavy", "ones"), ("identity_heavy", "uniform"),
             ("identity_heavy", "byte"), ("all_identity", "uniform"), ("all_identity", "ones"), ("all_identity", "minus_one"), ("few", "zeros")]


def _plans(be, body, cs, chunk, fanins):
    """body(c) under every forced plan: window widths, both sorts, bins cut into chunks, merge / tree fan-ins small and default; everything restored at the end.
    (The merge depth is planned for one bucket holding every pair and capped at 12 levels: fan-in 2 only fits a few hundred rows, the GPU sizes take 4.)"""
    try:
        for c in cs:
            for two_level in ((0, 1) if c <= 16 else (1,)):              # (windows above 16 bits always take the two-level sort)
                for merge, tree in fanins:
                    be.tune(msm_c=c, msm_two_level_sort=two_level, msm_bsort_chunk=chunk if two_level else 8192, msm_merge_fanin=merge, msm_tree_fanin=tree)
                    body(c)
    finally:
        be.tune(msm_c=0, msm_two_level_sort=0, msm_bsort_chunk=8192, msm_merge_fanin=8, msm_tree_fanin=2)


# ---- MSM: every pair of table and column, both entry points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bkind,skind", MSM_PAIRS)
def test_emulated_msm(emu, orc, pyref, bkind, skind):
    for n in (1, 2, 33, 300):
        ptc.check_structured_msm(emu, orc, pyref, n, bkind, skind, seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("bkind,skind", MSM_PAIRS)
def test_gpu_msm(gpu, orc, pyref, bkind, skind):
    for n in (2, 5000, 30000):
        ptc.check_structured_msm(gpu, orc, pyref, n, bkind, skind, seed=n)


@pytest.mark.parametrize("bkind,skind", [("all_equal", "paired"), ("alt_neg", "ones"), ("few", "uniform"), ("neg_pairs", "paired"), ("pairs", "neg_paired"), ("identity_heavy", "ones")])
def test_emulated_msm_plans(emu, orc, pyref, bkind, skind):
    _plans(emu, lambda c: ptc.check_structured_msm(emu, orc, pyref, 257, bkind, skind, seed=c, c=c, entries=("dev",)), PLAN_C[:5], 64, fanins=((8, 2), (2, 4)))
    _plans(emu, lambda c: ptc.check_structured_msm(emu, orc, pyref, 130, bkind, skind, seed=c, c=c, entries=("host",)), (20,), 64, fanins=((2, 2),))


@pytest.mark.gpu
@pytest.mark.parametrize("bkind,skind", [("all_equal", "paired"), ("all_equal", "ones"), ("alt_neg", "ones"), ("few", "uniform"), ("few", "one_digit"), ("neg_pairs", "paired"),
                                         ("pairs", "neg_paired"), ("identity_heavy", "ones"), ("small_multiples", "byte")])
def test_gpu_msm_plans(gpu, orc, pyref, bkind, skind):
    _plans(gpu, lambda c: ptc.check_structured_msm(gpu, orc, pyref, 6000, bkind, skind, seed=c, c=c, entries=("dev",)), PLAN_C, 256, fanins=((8, 2), (4, 4)))


# ---- cases that reach a branch by construction ---------------------------------------------------------------------------------------------------------------
def _every_chain_hands_off(be, orc, pyref, n):
    """all_equal + paired.  Rows 2i and 2i + 1 hold the same point and the same scalar, so in every window they get the same digit and the same sign, whatever the
    recoding: every non-empty bucket holds an even number (>= 2) of references to ONE point with ONE sign.  A sub-bucket chain of two or more references therefore adds
    P to P at its second step — the fast chain refuses, the kernel restores the point and the complete chain doubles, then adds P to 2P, 3P, .. (ZZ != 1) — and equal
    sub-bucket sums meet again in the merge levels (P + P with ZZ != 1 on both sides) and in the row / column / class sums."""
    bases, ks = ptc.structured_bases(orc, pyref, n, "all_equal", 1)
    sc = ptc.scalar_column(orc, pyref, n, "paired", 2)
    assert n % 2 == 0 and (bases == bases[0]).all() and bases[0].any() and (sc[0::2] == sc[1::2]).all()
    ptc.check_structured_msm(be, orc, pyref, n, "all_equal", "paired", seed=1, table=(bases, ks))
    ptc.check_structured_batch(be, orc, pyref, n, "all_equal", seed=1, device=True, skinds=("paired", "ones", "paired", "byte"))


def _equal_partial_sums_merge(be, orc, pyref, n, max_chunk, fanins=(2, 8)):
    """all_equal + ones: ONE bucket (digit 1 of window 0) holds all n references to one point.  With sub-buckets of at most max_chunk references (set here, not read
    back) and n >= 4 max_chunk + 1 there are at least four FULL sub-buckets of one length L <= max_chunk, each summing to [L] P: msm_merge_kernel adds equal points with
    ZZ != 1 — the doubling branch of xyzz_add_lazy, which normalises first — and, at fan-in 2, again one level up ([2 L] P twice)."""
    assert n >= 4 * max_chunk + 1
    try:
        for fanin in fanins:
            be.tune(msm_max_chunk=max_chunk, msm_max_chunk_wide=max_chunk, msm_merge_fanin=fanin)
            ptc.check_structured_msm(be, orc, pyref, n, "all_equal", "ones", seed=3)
            ptc.check_structured_msm(be, orc, pyref, n, "all_equal", "minus_one", seed=4, entries=("dev",))
    finally:
        be.tune(msm_max_chunk=48, msm_max_chunk_wide=128, msm_merge_fanin=8)


def _chains_continue_from_the_identity(be, orc, pyref, n, max_chunk):
    """alt_neg + ones: the one bucket holds n / 2 references to P and n / 2 to -P and nothing else, so whatever order the sort leaves them in, the second step of every
    chain adds P or -P to P or -P: a same-x addition, and the fast chain hands off.  In row order (P, -P, P, ..) that step cancels to the identity, the third starts again
    from it, and so on: even-length sub-buckets sum to the identity, which the merge level then meets as an operand; in any other order doublings and cancellations mix.
    The answer is the identity."""
    assert n % 2 == 0 and n >= 4 * max_chunk
    try:
        for chunk in (max_chunk, max_chunk - 1):                      # odd sub-bucket length: sums alternate P, -P and cancel in the merge instead
            be.tune(msm_max_chunk=chunk, msm_max_chunk_wide=chunk)
            assert ptc.check_structured_msm(be, orc, pyref, n, "alt_neg", "ones", seed=5) == 0
    finally:
        be.tune(msm_max_chunk=48, msm_max_chunk_wide=128)


def test_emulated_every_chain_hands_off(emu, orc, pyref):
    _every_chain_hands_off(emu, orc, pyref, 300)


def test_emulated_equal_partial_sums_merge(emu, orc, pyref):
    _equal_partial_sums_merge(emu, orc, pyref, 300, 16)


def test_emulated_chains_continue_from_the_identity(emu, orc, pyref):
    _chains_continue_from_the_identity(emu, orc, pyref, 300, 16)


@pytest.mark.gpu
def test_gpu_every_chain_hands_off(gpu, orc, pyref):
    _every_chain_hands_off(gpu, orc, pyref, 20000)


@pytest.mark.gpu
def test_gpu_equal_partial_sums_merge(gpu, orc, pyref):
    _equal_partial_sums_merge(gpu, orc, pyref, 20001, 48, fanins=(4, 8))
    _equal_partial_sums_merge(gpu, orc, pyref, 600, 16, fanins=(2,))    # (fan-in 2 reaches 2^12 sub-buckets: 600 rows whatever the window)


@pytest.mark.gpu
def test_gpu_chains_continue_from_the_identity(gpu, orc, pyref):
    _chains_continue_from_the_identity(gpu, orc, pyref, 20000, 48)


# ---- batches, partial sums, prefixes, the run-length path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bkind", ["all_equal", "few", "neg_pairs", "identity_heavy"])
def test_emulated_msm_batch(emu, orc, pyref, bkind):
    ptc.check_structured_batch(emu, orc, pyref, 200, bkind, seed=2)
    ptc.check_structured_batch(emu, orc, pyref, 90, bkind, seed=3, device=True, skinds=("paired", "neg_paired", "ones", "zeros"))


@pytest.mark.gpu
@pytest.mark.parametrize("bkind", ptc.POINT_KINDS)
def test_gpu_msm_batch(gpu, orc, pyref, bkind):
    ptc.check_structured_batch(gpu, orc, pyref, 8000, bkind, seed=2, device=True)
    ptc.check_structured_batch(gpu, orc, pyref, 3000, bkind, seed=3, device=False)


@pytest.mark.parametrize("bkind", ["all_equal", "alt_neg", "few", "pairs", "all_identity"])
def test_emulated_partial_sums(emu, orc, pyref, bkind):
    ptc.check_partials(emu, orc, pyref, 150, bkind)


@pytest.mark.gpu
@pytest.mark.parametrize("bkind", ptc.POINT_KINDS)
def test_gpu_partial_sums(gpu, orc, pyref, bkind):
    ptc.check_partials(gpu, orc, pyref, 6000, bkind)
    ptc.check_partials(gpu, orc, pyref, 6000, bkind, seed=9, skind="paired")


def test_emulated_prefix_of_a_structured_table(emu, orc, pyref):
    for bkind, skind in (("all_equal", "paired"), ("alt_neg", "ones"), ("identity_heavy", "uniform"), ("neg_pairs", "paired")):
        ptc.check_prefix(emu, orc, pyref, 120, bkind, skind)


@pytest.mark.gpu
def test_gpu_prefix_of_a_structured_table(gpu, orc, pyref):
    for bkind, skind in (("all_equal", "paired"), ("alt_neg", "ones"), ("identity_heavy", "uniform"), ("neg_pairs", "paired"), ("few", "uniform")):
        ptc.check_prefix(gpu, orc, pyref, 6000, bkind, skind)


@pytest.mark.parametrize("bkind", ["all_equal", "alt_neg", "identity_heavy"])
def test_emulated_run_length_path(emu, orc, pyref, bkind):
    ptc.check_runs(emu, orc, pyref, 1500, bkind)                        # (the run path needs 1024 rows)


@pytest.mark.gpu
@pytest.mark.parametrize("bkind", ["all_equal", "alt_neg", "identity_heavy", "few"])
def test_gpu_run_length_path(gpu, orc, pyref, bkind):
    ptc.check_runs(gpu, orc, pyref, 20000, bkind)


@pytest.mark.gpu
@pytest.mark.parametrize("bkind,skind", [("all_equal", "paired"), ("few", "uniform")])
def test_gpu_msm_2p18_closed_form(gpu, orc, pyref, bkind, skind):
    ptc.check_structured_msm(gpu, orc, pyref, 1 << 18, bkind, skind, seed=18, closed_only=True)


# ---- G1 NTT ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ptc.NTT_POINT_KINDS)
def test_emulated_g1_ntt(emu, orc, pyref, kind):
    for log_n in (0, 1, 3, 5):
        ptc.check_g1_ntt(emu, orc, pyref, log_n, kind, seed=log_n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ptc.NTT_POINT_KINDS)
def test_gpu_g1_ntt(gpu, orc, pyref, kind):
    """2^5 is one chunk of the affine conversion, 2^6 and 2^10 are several: for all_equal / alt_neg / delta every chunk but one is all identities"""
    for log_n in (1, 5, 6, 10):
        ptc.check_g1_ntt(gpu, orc, pyref, log_n, kind, seed=log_n)


# ---- fixed-base multiplication, point codec ------------------------------------------------------------------------------------------------------------------
def test_emulated_fixed_base_structured(emu, orc, pyref):
    assert ptc.check_fixed_base_structured(emu, orc, pyref) % 32 != 0   # (the fixture's block)


@pytest.mark.gpu
def test_gpu_fixed_base_structured(gpu, orc, pyref):
    assert ptc.check_fixed_base_structured(gpu, orc, pyref, pad_to=3001) % 256 != 0


@pytest.mark.parametrize("sign_bit", [255, 254])
def test_emulated_point_codec(emu, orc, pyref, sign_bit):
    ptc.check_codec(emu, orc, pyref, 203, sign_bit)


@pytest.mark.gpu
@pytest.mark.parametrize("sign_bit", [255, 254])
def test_gpu_point_codec(gpu, orc, pyref, sign_bit):
    ptc.check_codec(gpu, orc, pyref, 5003, sign_bit)
