"""The quotient on programs of a CHOSEN shape (tests/program_cases.py).  The random programs of tests/quotient_cases.py and the program bench.py times all compile to
three or four slots (live intermediates), which is ONE launch shape of the interpreter and a few carried planes in the generated kernels.  Here:

* the slot ladder: programs of 5, 6, 9, 10, 33, 34 and 81 slots — on either side of every threshold of quotient_run's launch shape (threads per
  workgroup 256 / 128 / 64, dynamic LDS up to 32 KiB, 64 KiB, above 64 KiB, 160 KiB) — and the refusal of the 82nd slot;
* graph forms halo2's Evaluator never emits but the blob reader accepts, the rotation limits, and the compiler settings no other test moves.

Every case goes through quotient_cases.run_case: whole domain, first and last coset, coset parts, four row slices per coset and the two degree parts, each bit for bit
against the oracle (oracle/evaluate_h_oracle.inc).  CPU: the kernel emulator.  GPU: the product library, on the interpreter and on the generated kernels."""
import ctypes as C
import re
import time

import pytest

import parity_cases as pc
import program_cases as pg
import quotient_cases as qc
import zk_dcap_verifier_amd as z
from test_quotient import DENSE, SHAPES
from test_quotient_jit import _source

ZK_ERR_PROGRAM, ZK_ERR_LIMIT = -4, -5
LADDER = sorted(pg.LADDER)


def _slots(be, prog):
    h = be.quotient_program_load(prog.to_blob())
    info, split = be.quotient_program_info(h), be.quotient_program_split(h)
    be.quotient_program_release(h)
    return info["slots"], split


def _check_rung(be, slots, k):
    """the program of that rung at 2^k rows: the compiler's own slot count (the count belongs to the compiler, not to program_cases) and, where the program carries a
    permutation and lookups, a degree split whose two parts both hold instructions"""
    prog = pg.ladder_program(slots, k)
    got, split = _slots(be, prog)
    assert got == slots, (got, slots)
    if pg.LADDER[slots][1]:
        assert split["low_cosets"] == 2 and split["instructions_high"] and split["instructions_low"], split
    return prog


# slots of the high and low part of every rung's program.  The C ABI reports the whole program's count only; the emulator build hands out a part's program
# (program_cases.part_slots), the census below pins these there, and the GPU cases — same host compiler in the product library — quote them.  A low part of 1 (the rungs
# without permutation and lookups) writes NO slot: it is the small gate alone, held in the accumulator
PART_SLOTS = {5: (5, 1), 6: (6, 1), 9: (9, 3), 10: (10, 1), 33: (33, 1), 34: (34, 3), 81: (81, 3)}


def _shape_report(slots, k, threads):
    """slots of the program and of its parts, and the launch shape (threads per workgroup, LDS bytes) of each on its rows and of the whole program on a quarter of a coset"""
    hi, lo = PART_SLOTS[slots]
    n = 1 << k
    return dict(slots=slots, slots_high=hi, slots_low=lo, quot_threads=threads,
                shape_whole=pg.launch_shape(slots, 4 * n, threads), shape_high=pg.launch_shape(hi, 4 * n, threads), shape_low=pg.launch_shape(lo, 2 * n, threads),
                shape_row_slice=pg.launch_shape(slots, max(n // 4, 1), threads))


# ---- CPU: the census --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slots", LADDER)
def test_emulated_slot_ladder(emu, orc, pyref, slots):
    prog = _check_rung(emu, slots, 3)
    for k in (3, 8):                                                  # (the counts do not depend on the domain)
        h = emu.quotient_program_load(pg.ladder_program(slots, k).to_blob())
        assert pg.part_slots(emu, _source, h) == (slots,) + PART_SLOTS[slots]
        emu.quotient_program_release(h)
    qc.run_case(emu, orc, pyref, pc, prog, seed=slots)


def _library_shape(be, slots, rows, threads):
    """quot_launch_shape / quot_slots_fit of the emulator build (csrc/quotient.hip, through the test-only export): ((T, LDS bytes), a program of that many slots is loaded)"""
    t, lds = C.c_uint32(), C.c_size_t()
    fits = be.lib.zk_test_quot_launch_shape(C.c_uint32(slots), C.c_int(threads), C.c_uint64(rows), C.byref(t), C.byref(lds))
    return (t.value, lds.value), bool(fits)


def test_launch_shape_of_every_rung(emu):
    """program_cases.launch_shape is a restatement in Python of quot_launch_shape (csrc/quotient.hip), the one function quotient_run takes the threads and the LDS bytes
    of every launch from; it is pinned here against that function (zk_test_quot_launch_shape of the emulator build) and against the literal table below.  What the table
    shows is that the ladder's slot counts stand on either side of every threshold of the rule.  The GPU cases quote these figures in their messages, they do not measure
    them (a kernel trace of the ladder shows the workgroup sizes: DESIGN.md 3.3)."""
    shapes = {s: pg.launch_shape(s, 256, 256) for s in LADDER}
    assert shapes == {5: (256, 32768), 6: (128, 20480), 9: (128, 32768), 10: (64, 18432), 33: (64, 65536), 34: (64, 67584), 81: (64, 163840)}
    # under the default quot_threads = 128 the first three rungs share 128 threads
    assert [pg.launch_shape(s, 256, 128)[0] for s in LADDER] == [128, 128, 128, 64, 64, 64, 64]
    # 16 rows per coset, row slices of 4: clipped to the row count
    assert pg.launch_shape(34, 4, 128) == (4, 33 * 4 * 32)
    # the library's own function: every rung at both thread settings, the clipped case, slots 1 and 2 (no LDS / the first LDS slot) and the slot that is refused
    for slots, rows, threads in [(s, 256, t) for s in LADDER for t in (256, 128)] + [(34, 4, 128)] + [(s, 256, t) for s in (1, 2, pg.MAX_SLOTS + 1) for t in (256, 128)]:
        assert _library_shape(emu, slots, rows, threads) == (pg.launch_shape(slots, rows, threads), slots <= pg.MAX_SLOTS), (slots, rows, threads)
    assert _library_shape(emu, 1, 256, 256)[0] == (256, 0) and _library_shape(emu, 2, 256, 256)[0] == (256, 256 * 32)


def test_emulated_one_slot_too_many_is_refused(emu, orc, pyref):
    """82 slots would need 162 KiB of LDS at 64 threads: refused when the program is loaded, with the limit code, and the context goes on loading and running programs"""
    for perm, lookups in ((0, 0), (4, 2)):
        with pytest.raises(z.ZkError) as err:
            emu.quotient_program_load(pg.live_program(pg.MAX_SLOTS, 3, perm, lookups).to_blob())
        assert err.value.code == ZK_ERR_LIMIT, err.value
    qc.run_case(emu, orc, pyref, pc, _check_rung(emu, 9, 3), seed=2)


def test_random_programs_stay_below_six_slots(emu, orc, pyref):
    """what the REST of the suite reaches: the random programs of test_quotient.py / test_quotient_jit.py and the program bench.py times.  If a change to
    quotient_cases.build_program or to the compiler moves this, the slot ladder of THIS file is what still covers the other launch shapes — keep it, and say in
    DESIGN.md 3.3 which rungs the random programs now reach."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import bench
    progs = [qc.build_program(orc, pyref, seed=seed, **shape) for seed, shape in SHAPES]
    progs += [qc.build_program(orc, pyref, seed=seed, gate_ops=60, **DENSE) for seed in (1, 2, 3, 4, 5, 8)]
    progs.append(bench.sgx_shaped_program(z, 3, 5, 25, 18, 11, 16, 5))
    slots = [_slots(emu, p)[0] for p in progs]
    assert 3 <= min(slots) and max(slots) < 6, slots


def _carried_planes(src):
    """state planes each generated kernel stores for its successors"""
    return [len(set(re.findall(r"store_u256\(PLANE\((\d+)\), oidx", body))) for body in src.split('extern "C" __global__')[1:]]


def test_generated_kernels_of_the_ladder_carry_many_planes(emu):
    """cut after every 6 products, the 34-slot program cannot wait for a position with one live slot: its kernels hand dozens of planes to their successors through
    QuotArgs::state (the random programs: a few).  This is what the generated-kernel cases of the ladder are for."""
    for slots, least in ((34, 9), (81, 9)):                           # (more than 8; measured: 33 and 79)
        h = emu.quotient_program_load(pg.ladder_program(slots, 8).to_blob())
        for part in (0, 1):
            src, n_kernels, n_planes = _source(emu, h, part, 6)
            carried = _carried_planes(src)
            assert n_kernels >= 2 and max(carried) >= least and max(carried) <= n_planes <= slots, (slots, part, carried, n_planes)
        emu.quotient_program_release(h)


# ---- CPU: forms, rotations, settings ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", pg.FORMS, ids=lambda f: f.__name__[5:])
def test_emulated_program_forms(emu, orc, pyref, form):
    qc.run_case(emu, orc, pyref, pc, form(orc, 3), seed=7)


def _zero_numerator_case(be, orc, pyref, k, **kw):
    got = qc.run_case(be, orc, pyref, pc, pg.form_difference_of_a_value_with_itself(orc, k), seed=9, **kw)
    assert not got.any(), "v - v must be the canonical zero, all limbs"


def test_emulated_difference_of_a_value_with_itself(emu, orc, pyref):
    _zero_numerator_case(emu, orc, pyref, 3)


def test_emulated_rotations_beyond_the_domain(emu, orc, pyref):
    qc.run_case(emu, orc, pyref, pc, pg.form_rotations_beyond_the_domain(orc, 2), seed=4)


# rotations at k = 8: 255 values are distinct modulo the 256 rows of a coset (and, scaled by 4, modulo the 1024 of the domain)
ROT_K = 8
GATE_ROTATIONS = list(range(-100, 100))                                # 200
LOOKUP_ROTATIONS = list(range(100, 128)) + list(range(-127, -100))     # 55 more; the lookup argument's own 0, 1, -1 are among the gate's


def _rotation_cases(be, orc, pyref, **kw):
    qc.run_case(be, orc, pyref, pc, pg.rotations_program(ROT_K, GATE_ROTATIONS), seed=11, **kw)
    assert len(set(r % (1 << ROT_K) for r in GATE_ROTATIONS + LOOKUP_ROTATIONS)) == 255
    qc.run_case(be, orc, pyref, pc, pg.rotations_program(ROT_K, GATE_ROTATIONS, LOOKUP_ROTATIONS), seed=12, **kw)


def test_emulated_rotation_limits(emu, orc, pyref):
    _rotation_cases(emu, orc, pyref)
    with pytest.raises(z.ZkError) as err:                             # 256 distinct rotations over the two graphs, each within its own limit
        emu.quotient_program_load(pg.rotations_program(ROT_K, GATE_ROTATIONS, LOOKUP_ROTATIONS + [-128]).to_blob())
    assert err.value.code == ZK_ERR_LIMIT, err.value
    with pytest.raises(z.ZkError) as err:                             # 256 in one graph: the blob reader refuses the graph
        emu.quotient_program_load(pg.rotations_program(ROT_K, list(range(-128, 128))).to_blob())
    assert err.value.code == ZK_ERR_PROGRAM and "malformed" in str(err.value), err.value
    qc.run_case(emu, orc, pyref, pc, _check_rung(emu, 5, 3), seed=3)


SETTINGS = [dict(quot_group_factors=0), dict(quot_remat_ops=0), dict(quot_remat_ops=1000, quot_remat_distance=0)]
DEFAULT_SETTINGS = dict(quot_group_factors=1, quot_remat_ops=4, quot_remat_distance=24)


SETTINGS_PROGRAMS = ("shape1", "shape4", "ladder34")
setting_id = lambda s: ",".join("%s=%d" % kv for kv in s.items())


def _settings_case(be, orc, pyref, setting, which, k, **kw):
    """one program under one setting.  The setting is in force when run_case loads the program (the settings are the COMPILER's).  The 34-slot ladder program must still
    compile to 34 slots there — it is in this list for its launch shape and for what its generated kernels carry — and the random shapes to their 3 or 4"""
    prog = {"shape1": lambda: qc.build_program(orc, pyref, seed=SHAPES[0][0], **SHAPES[0][1]), "shape4": lambda: qc.build_program(orc, pyref, seed=SHAPES[3][0], **SHAPES[3][1]),
            "ladder34": lambda: pg.ladder_program(34, k)}[which]()
    assert all(be.tune_get(key) == v for key, v in DEFAULT_SETTINGS.items())
    try:
        be.tune(**setting)
        slots, split = _slots(be, prog)
        assert (slots == 34 if which == "ladder34" else slots in (3, 4)) and split["low_cosets"] == 2, (setting, which, slots, split)
        try:
            qc.run_case(be, orc, pyref, pc, prog, seed=6, **kw)
        except (AssertionError, z.ZkError) as e:
            raise AssertionError("%r, %s, %d slots: %s" % (setting, which, slots, e)) from e
    finally:
        be.tune(**DEFAULT_SETTINGS)


@pytest.mark.parametrize("which", SETTINGS_PROGRAMS)
@pytest.mark.parametrize("setting", SETTINGS, ids=setting_id)
def test_emulated_compiler_settings(emu, orc, pyref, setting, which):
    _settings_case(emu, orc, pyref, setting, which, 3)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------------------

def _gpu_rung(gpu, orc, pyref, slots, k, kind="uniform", threads=128, **kw):
    """threads: the value of tune quot_threads the case runs under.  The report (slot counts pinned by the census, shapes COMPUTED by program_cases.launch_shape) is printed and
    goes into the message of a failure; what is asserted on the GPU is the slot count the library reports and every value against the oracle"""
    assert gpu.tune_get("quot_threads") == threads
    report = _shape_report(slots, k, threads)
    prog = _check_rung(gpu, slots, k)
    print("ladder", report)
    try:
        qc.run_case(gpu, orc, pyref, pc, prog, seed=slots, kind=kind, **kw)
    except (AssertionError, z.ZkError) as e:
        raise AssertionError("%r: %s" % (report, e)) from e
    return report


@pytest.mark.gpu
@pytest.mark.parametrize("slots,kind", [(s, "uniform") for s in LADDER] + [(s, "minus_one") for s in (10, 34, 81)])
def test_gpu_slot_ladder_interpreter(gpu, orc, pyref, slots, kind):
    """2^8 rows per coset, 2^10 in the domain, row slices of 64: every workgroup of every rung is full and every launch has several.  minus_one: the largest canonical
    word in every column, so the lazy values the LDS slots hold reach into [p, 2p]"""
    assert gpu.tune_get("quot_jit") == 0 and gpu.tune_get("quot_threads") == 128
    _gpu_rung(gpu, orc, pyref, slots, 8, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [5, 6])
def test_gpu_slot_ladder_at_256_threads(gpu, orc, pyref, slots):
    """the default quot_threads is 128; asked for 256, five slots (32 KiB) keep them and six are halved to 128 (test_launch_shape_of_every_rung)"""
    try:
        gpu.tune(quot_threads=256)
        _gpu_rung(gpu, orc, pyref, slots, 8, threads=256)
    finally:
        gpu.tune(quot_threads=128)


@pytest.mark.gpu
def test_gpu_slot_ladder_below_a_wavefront(gpu, orc, pyref):
    """16 rows per coset and row slices of 4: the workgroup is clipped to the row count, 66 KiB of LDS slots shrink with it"""
    _gpu_rung(gpu, orc, pyref, 34, 4)


def _with_generated_kernels(gpu, fn, group=6):
    """group 6, as tests/test_quotient_jit.py: whole program and parts, cut after every 6 products.  The forms and rotation programs, which are not about the cuts, take
    24 — hiprtc costs more than half a second per kernel, whatever its size"""
    gpu.tune(quot_jit=2, quot_jit_group=group)
    try:
        return fn()
    finally:
        gpu.tune(quot_jit=0, quot_jit_group=200)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [10, 34])
def test_gpu_slot_ladder_generated_kernels(gpu, orc, pyref, slots):
    """every slot is a u256 local of the generated kernels and a plane of QuotArgs::state at a cut (test_generated_kernels_of_the_ladder_carry_many_planes)"""
    t0 = time.time()
    _with_generated_kernels(gpu, lambda: _gpu_rung(gpu, orc, pyref, slots, 8, expect_kernels=True))
    print("generated kernels, %d slots: %.1f s" % (slots, time.time() - t0))


@pytest.mark.gpu
def test_gpu_slot_ladder_generated_kernels_81_slots(gpu, orc, pyref):
    """the largest program the library loads, on generated kernels: hiprtc builds it (a failure is an error of zk_quotient_program_load, never a silent return to the
    interpreter: run_case asserts the kernels exist) and 81 locals of 32 bytes per row give the oracle's values"""
    t0 = time.time()
    _with_generated_kernels(gpu, lambda: _gpu_rung(gpu, orc, pyref, 81, 8, expect_kernels=True))
    print("generated kernels, 81 slots: %.1f s" % (time.time() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
@pytest.mark.parametrize("form", pg.FORMS, ids=lambda f: f.__name__[5:])
def test_gpu_program_forms(gpu, orc, pyref, form, jit):
    run = lambda **kw: qc.run_case(gpu, orc, pyref, pc, form(orc, 6), seed=7, **kw)
    if jit:
        _with_generated_kernels(gpu, lambda: run(expect_kernels=True), group=24)
    else:
        run()


@pytest.mark.gpu
def test_gpu_difference_of_a_value_with_itself(gpu, orc, pyref):
    _zero_numerator_case(gpu, orc, pyref, 6)
    _with_generated_kernels(gpu, lambda: _zero_numerator_case(gpu, orc, pyref, 6, expect_kernels=1))


@pytest.mark.gpu
def test_gpu_rotations_beyond_the_domain(gpu, orc, pyref):
    prog = pg.form_rotations_beyond_the_domain(orc, 2)
    qc.run_case(gpu, orc, pyref, pc, prog, seed=4)
    _with_generated_kernels(gpu, lambda: qc.run_case(gpu, orc, pyref, pc, prog, seed=4, expect_kernels=True), group=24)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
def test_gpu_rotation_limits(gpu, orc, pyref, jit):
    if jit:
        _with_generated_kernels(gpu, lambda: _rotation_cases(gpu, orc, pyref, expect_kernels=True), group=24)
    else:
        _rotation_cases(gpu, orc, pyref)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
@pytest.mark.parametrize("which", SETTINGS_PROGRAMS)
@pytest.mark.parametrize("setting", SETTINGS, ids=setting_id)
def test_gpu_compiler_settings(gpu, orc, pyref, setting, which, jit):
    """the settings change the micro-op stream and the liveness of the slots, which is what the generated kernels are cut by and carry: both executors"""
    if jit:
        _with_generated_kernels(gpu, lambda: _settings_case(gpu, orc, pyref, setting, which, 6, expect_kernels=True), group=24)
    else:
        _settings_case(gpu, orc, pyref, setting, which, 6)
