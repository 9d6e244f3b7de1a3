"""Parity on a USED context (tests/history_cases.py): the prover keeps one zk_ctx for hours — its DevBuf workspaces only grow, its 16 twiddle sets, coset tables and
the buffers zk_plonk_create_proof keeps between proofs stay resident — so every call runs on what the previous call left behind.  The rest of the suite meets that state
only in the order pytest happens to collect its tests.  Here every test opens a context of its own and writes the history itself: victim on the fresh context, polluter,
victim, polluter, each step bit for bit against the oracle, with a polluter that is dense where the victim is sparse, at least as large, and of the same layout (or a
shifted one).  Sections: A the MSM workspaces, B twiddle sets / coset tables / the NTT workspace, C the operations that share ws_tmp, D the quotient's state planes,
E whole proofs, F refused calls.  Every case runs on the kernel emulator (CPU) and on the product library (GPU)."""
import pytest

import history_cases as hc
import parity_cases as pc


def _base(be):
    return {key: be.tune_get(key) for key in ("msm_block", "ntt_threads", "ntt_tile_log", "ntt_max_radix_log")}


def test_emulator_tunables_are_the_fixtures(emu):
    """history_cases.EMU_TUNE restates conftest.py's `emu` fixture (a context of one's own cannot borrow the fixture's)"""
    assert {key: emu.tune_get(key) for key in hc.EMU_TUNE} == hc.EMU_TUNE


def test_dense_polluter_fills_every_bucket(orc, pyref):
    """from the inputs alone: in every column of the narrow polluters every bucket receives a scalar from every window below the top one; the wide ones reach every
    window and more buckets than the table has rows; the sparse victims are what their names say"""
    for which, S in hc.SIZES.items():
        c, n = S["msm_narrow"], S["msm_n"]
        for col in hc.dense_columns(orc, pyref, n, c):
            assert hc.bucket_census(pyref, orc, col, c)[0] == 1 << (c - 1), (which, c)
        if which == "emu":                                             # (the wide GPU columns are counted by the GPU case itself)
            hc.dense_columns(orc, pyref, S["msm_wide_n"], S["msm_wide"])
        for c, n in ((S["msm_narrow"], 40), (S["msm_wide"], 40)):
            sp = hc.sparse_columns(orc, pyref, n, c)
            W = hc.scs.windows(c)
            for name, at in (("low_window", 0), ("top_window", W - 1)):
                for v in orc.fr_to_ints(sp[name]):
                    assert [j for j, d in enumerate(hc.scs.signed_digits(v, c)) if d] == [at], (name, c)


# ---- A. MSM workspaces -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", hc.MSM_PLANS, ids=hc.msm_plan_id)
def test_emulated_msm_history(emu, orc, pyref, plan):
    with hc.fresh("emu") as be:
        hc.msm_history(be, orc, pyref, hc.SIZES["emu"], plan)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", hc.MSM_PLANS, ids=hc.msm_plan_id)
def test_gpu_msm_history(gpu, orc, pyref, plan):
    with hc.fresh("gpu") as be:
        hc.msm_history(be, orc, pyref, hc.SIZES["gpu"], plan)


@pytest.mark.parametrize("first", (2, 0))
def test_emulated_run_length_history(emu, orc, pyref, first):
    with hc.fresh("emu") as be:
        hc.runs_history(be, orc, pyref, hc.SIZES["emu"], first)


@pytest.mark.gpu
@pytest.mark.parametrize("first", (2, 0))
def test_gpu_run_length_history(gpu, orc, pyref, first):
    with hc.fresh("gpu") as be:
        hc.runs_history(be, orc, pyref, hc.SIZES["gpu"], first)


# ---- B. twiddle sets, coset tables, NTT workspace ----------------------------------------------------------------------------------------------------------------
def test_emulated_eviction_walk(emu, orc, pyref):
    with hc.fresh("emu") as be:
        hc.eviction_walk(be, orc, pyref, hc.SIZES["emu"])


@pytest.mark.gpu
def test_gpu_eviction_walk(gpu, orc, pyref):
    with hc.fresh("gpu") as be:
        hc.eviction_walk(be, orc, pyref, hc.SIZES["gpu"])


@pytest.mark.parametrize("op", hc.HELD_POINTER_OPS)
def test_emulated_eviction_under_held_pointers(emu, orc, pyref, op):
    with hc.fresh("emu") as be:
        hc.eviction_under_held_pointers(be, orc, pyref, hc.SIZES["emu"], op)


@pytest.mark.gpu
@pytest.mark.parametrize("op", hc.HELD_POINTER_OPS)
def test_gpu_eviction_under_held_pointers(gpu, orc, pyref, op):
    with hc.fresh("gpu") as be:
        hc.eviction_under_held_pointers(be, orc, pyref, hc.SIZES["gpu"], op)


@pytest.mark.parametrize("knob", hc.RETUNE_KNOBS)
def test_emulated_retuning_mid_life(emu, orc, pyref, knob):
    with hc.fresh("emu") as be:
        hc.retuning(be, orc, pyref, hc.SIZES["emu"], knob)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", hc.RETUNE_KNOBS)
def test_gpu_retuning_mid_life(gpu, orc, pyref, knob):
    with hc.fresh("gpu") as be:
        hc.retuning(be, orc, pyref, hc.SIZES["gpu"], knob)


def test_emulated_ntt_workspace(emu, orc, pyref):
    with hc.fresh("emu") as be:
        hc.ntt_workspace(be, orc, pyref, hc.SIZES["emu"])


@pytest.mark.gpu
def test_gpu_ntt_workspace(gpu, orc, pyref):
    """the first GPU run of the column slices under ntt_ws_limit_mb"""
    with hc.fresh("gpu") as be:
        hc.ntt_workspace(be, orc, pyref, hc.SIZES["gpu"])


# ---- C. the ws_tmp sharers ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polluter", hc.SHARERS)
def test_emulated_ws_tmp_sharers(emu, orc, pyref, polluter):
    with hc.fresh("emu") as be:
        hc.sharer_pairs(be, orc, pyref, hc.SIZES["emu"], polluter)


@pytest.mark.gpu
@pytest.mark.parametrize("polluter", hc.SHARERS)
def test_gpu_ws_tmp_sharers(gpu, orc, pyref, polluter):
    with hc.fresh("gpu") as be:
        hc.sharer_pairs(be, orc, pyref, hc.SIZES["gpu"], polluter)


@pytest.mark.parametrize("which", ("g1_decompress", "lookup"))
def test_emulated_counters_start_from_zero(emu, orc, pyref, which):
    with hc.fresh("emu") as be:
        hc.counters(be, orc, pyref, hc.SIZES["emu"], which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("g1_decompress", "lookup"))
def test_gpu_counters_start_from_zero(gpu, orc, pyref, which):
    with hc.fresh("gpu") as be:
        hc.counters(be, orc, pyref, hc.SIZES["gpu"], which)


# ---- D. quotient state -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reload", (False, True), ids=("runs", "reload"))
def test_emulated_quotient_state(emu, orc, pyref, reload):
    with hc.fresh("emu") as be:
        hc.quotient_state(be, orc, pyref, hc.SIZES["emu"], reload=reload)


@pytest.mark.gpu
@pytest.mark.parametrize("jit,reload", ((0, False), (1, False), (0, True)), ids=("interpreter", "generated", "reload"))
def test_gpu_quotient_state(gpu, orc, pyref, jit, reload):
    """(the generated kernels exist on the GPU only: hiprtc.  `generated` takes about 20 s, 18 of them the one hiprtc build of the 81-slot program's kernels, whatever the
    rows: docs/LOG_r11.md has the build times by quot_jit_group)"""
    with hc.fresh("gpu") as be:
        hc.quotient_state(be, orc, pyref, hc.SIZES["gpu"], jit=jit, reload=reload)


# ---- E. whole proofs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", hc.PROOF_VARIANTS, ids=hc.proof_variant_id)
def test_emulated_proofs_on_a_used_context(emu, orc, variant):
    with hc.fresh("emu") as be:
        hc.proofs_on_a_used_context(be, orc, hc.SIZES["emu"], **variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", hc.PROOF_VARIANTS, ids=hc.proof_variant_id)
def test_gpu_proofs_on_a_used_context(gpu, orc, variant):
    with hc.fresh("gpu") as be:
        hc.proofs_on_a_used_context(be, orc, hc.SIZES["gpu"], **variant)


# ---- F. refused calls --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", hc.REFUSALS)
def test_emulated_refused_call_leaves_the_context_usable(emu, orc, pyref, which):
    with hc.fresh("emu") as be:
        hc.refused(be, orc, pyref, hc.SIZES["emu"], which, _base(be))


@pytest.mark.gpu
@pytest.mark.parametrize("which", hc.REFUSALS)
def test_gpu_refused_call_leaves_the_context_usable(gpu, orc, pyref, which):
    with hc.fresh("gpu") as be:
        hc.refused(be, orc, pyref, hc.SIZES["gpu"], which, _base(be))
