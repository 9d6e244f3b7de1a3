"""The two batched entry points of the GWC multi-open — zk_fr_lincomb_batch_dev and zk_kate_division_batch_dev — at the smallest shapes at which their kernels can go
wrong: against the single calls bit for bit (the batch is another launch geometry of the same arithmetic) and against Python integers (Horner, sums of products).

Lincomb: list lengths around the six-term chunk (1, 5, 6, 7, 12, 13) and around the 16-chunk reduce_small (96, 97 terms = 16, 17 chunks), a polynomial shared by three
lists, scalars 0, 1, r - 1, n around one workgroup of the GPU's vec_block (255, 256, 257), n = 1, and one n that makes the grid-stride loop go round twice (the grid
is capped at 8192 workgroups: 8192 x vec_block + 1 coefficients with vec_block at 32, the smallest the suite sets).
Division: n around the 2048-coefficient span of a workgroup (2047, 2048, 2049, 4097), n = 2, 3, divisors 0, 1, r - 1 and uniform, one column divided by three points,
an all-zero column; on the GPU one case of 2^19 + 2049 coefficients = 258 workgroups per column, which takes the carry kernel into its second round of 256.
"""
import numpy as np
import pytest

import parity_cases as pc
import zk_dcap_verifier_amd as z

LIST_LENGTHS = [1, 5, 6, 7, 12, 13, 96, 97]
POOL = 100                                                            # distinct polynomials; list p takes pool[0], then pool[p + 1 ..] (so pool[0] stands in every list)
SHAPES = {1: [97], 2: [96, 1], 5: [5, 6, 7, 12, 13], 9: LIST_LENGTHS + [6]}


def _lists(count):
    """per list: indices into the pool — pool[0] is shared by all lists (by three at least wherever count >= 3), the rest are taken round the pool from a start of its own"""
    return [[0] + [1 + (7 * p + j) % (POOL - 1) for j in range(length - 1)] for p, length in enumerate(SHAPES[count])]


def _scalars(orc, pyref, length, seed):
    """uniform scalars with 0, 1 and r - 1 planted where the list is long enough (a list of one term takes r - 1, 1 or 0 in turn)"""
    s = orc.fr_to_ints(pc.rand_fr(orc, pyref, length, seed))
    special = [pyref.R - 1, 1, 0]
    if length == 1:
        return [special[seed % 3]]
    for i, v in enumerate(special[:length]):
        s[(i * 5) % length] = v
    return s


def _check_lincomb_batch(be, orc, pyref, n, count, seed=0):
    R = pyref.R
    used = sorted({i for lst in _lists(count) for i in lst})
    pool = {i: pc.rand_fr(orc, pyref, n, 1000 * seed + i) for i in used}
    ints = {i: orc.fr_to_ints(pool[i]) for i in used}
    dev = {i: be.to_device(pool[i]) for i in used}
    lists = _lists(count)
    scal = [_scalars(orc, pyref, len(lst), seed + p) for p, lst in enumerate(lists)]
    outs = [be.alloc(n * 32) for _ in lists]
    single = be.alloc(n * 32)
    try:
        be.fr_lincomb_batch_dev([[dev[i] for i in lst] for lst in lists], [orc.fr_from_ints(s) for s in scal], n, outs)
        for p, lst in enumerate(lists):
            got = outs[p].download((n, 4))
            be.fr_lincomb_dev([dev[i] for i in lst], orc.fr_from_ints(scal[p]), n, single)
            assert (got == single.download((n, 4))).all(), ("batch vs single call", p)
            want = [sum(s * ints[i][r] for s, i in zip(scal[p], lst)) % R for r in range(n)]
            assert (got == orc.fr_from_ints(want)).all(), ("batch vs Python integers", p)
    finally:
        for d in list(dev.values()) + outs + [single]:
            d.free()


LINCOMB_CASES = [(n, count) for n in (1, 255, 256, 257) for count in (1, 2, 5, 9)]


@pytest.mark.parametrize("n,count", LINCOMB_CASES)
def test_emulated_lincomb_batch(emu, orc, pyref, n, count):
    _check_lincomb_batch(emu, orc, pyref, n, count, seed=n + count)


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", LINCOMB_CASES)
def test_gpu_lincomb_batch(gpu, orc, pyref, n, count):
    _check_lincomb_batch(gpu, orc, pyref, n, count, seed=n + count)


def _check_grid_stride(be, orc, pyref):
    """8192 x 32 + 1 coefficients at vec_block = 32: the last coefficient is the second trip of workgroup 0's first thread; short lists keep the reference cheap"""
    R = pyref.R
    before = be.tune_get("vec_block")
    be.tune(vec_block=32)
    n = 8192 * 32 + 1
    cols = [pc.rand_fr(orc, pyref, n, 40 + i) for i in range(2)]
    ints = [orc.fr_to_ints(c) for c in cols]
    dev = [be.to_device(c) for c in cols]
    lists, scal = [[0], [1, 0]], [[R - 1], [3, 1]]
    outs = [be.alloc(n * 32) for _ in lists]
    single = be.alloc(n * 32)
    try:
        be.fr_lincomb_batch_dev([[dev[i] for i in lst] for lst in lists], [orc.fr_from_ints(s) for s in scal], n, outs)
        for p, lst in enumerate(lists):
            got = outs[p].download((n, 4))
            be.fr_lincomb_dev([dev[i] for i in lst], orc.fr_from_ints(scal[p]), n, single)
            assert (got == single.download((n, 4))).all(), p
            want = [sum(s * ints[i][r] for s, i in zip(scal[p], lst)) % R for r in range(n)]
            assert (got == orc.fr_from_ints(want)).all(), p
    finally:
        be.tune(vec_block=before)
        for d in dev + outs + [single]:
            d.free()


def test_emulated_lincomb_batch_grid_stride(emu, orc, pyref):
    _check_grid_stride(emu, orc, pyref)


@pytest.mark.gpu
def test_gpu_lincomb_batch_grid_stride(gpu, orc, pyref):
    _check_grid_stride(gpu, orc, pyref)


def _check_lincomb_refusals(be, orc, pyref):
    n = 8
    a, b = be.to_device(pc.rand_fr(orc, pyref, n, 1)), be.to_device(pc.rand_fr(orc, pyref, n, 2))
    o1, o2 = be.alloc(n * 32), be.alloc(n * 32)
    one = orc.fr_from_ints([1])
    two = orc.fr_from_ints([1, 2])
    sentinel = pc.rand_fr(orc, pyref, n, 3)
    o1.upload(sentinel)
    o2.upload(sentinel)

    def refused(poly_lists, scalar_lists, outs, needle):
        with pytest.raises(z.ZkError) as e:
            be.fr_lincomb_batch_dev(poly_lists, scalar_lists, n, outs)
        assert e.value.code == -1 and needle in str(e.value), str(e.value)
        assert (o1.download((n, 4)) == sentinel).all() and (o2.download((n, 4)) == sentinel).all(), "a refused call wrote an output"
    try:
        refused([[a, 0], [b]], [two, one], [o1, o2], "null polynomial")
        refused([[a, b], [b]], [two, one], [o1, 0], "null output")
        refused([[a, b], []], [two, np.zeros((0, 4), dtype=np.uint64)], [o1, o2], "empty")
        refused([[a, b], [b, o1]], [two, two], [o1, o2], "also an input")          # the output of one list is an input of another
        refused([[a, o1]], [two], [o1], "also an input")                           # ... or of its own (the single call allows that, the batch does not)
        refused([[a, b], [b]], [two, one], [o1, o1], "same buffer")
        be.fr_lincomb_batch_dev([[a, b], [b]], [two, one], n, [o1, o2])            # the context is as usable as before
        assert (o2.download((n, 4)) == b.download((n, 4))).all()
    finally:
        for d in (a, b, o1, o2):
            d.free()


def test_emulated_lincomb_batch_refusals(emu, orc, pyref):
    _check_lincomb_refusals(emu, orc, pyref)


@pytest.mark.gpu
def test_gpu_lincomb_batch_refusals(gpu, orc, pyref):
    _check_lincomb_refusals(gpu, orc, pyref)


# ---- division ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _horner_quotient(a, b, R):
    """kate_division over Python integers: q[n-2] = a[n-1], q[i-1] = a[i] + b q[i]"""
    q = [0] * (len(a) - 1)
    acc = 0
    for i in range(len(a) - 1, 0, -1):
        acc = (a[i] + b * acc) % R
        q[i - 1] = acc
    return q


def _division_columns(orc, pyref, n, count, seed):
    """(columns, which column every division reads, divisors): count = 1: a uniform column by a uniform point; count = 3: ONE column by 0, 1 and r - 1; count = 8: those
    three, then a uniform column, an all-zero column and three more uniform ones, each by a uniform point of its own"""
    R = pyref.R
    uniform = orc.fr_to_ints(pc.rand_fr(orc, pyref, 8, seed + 77))
    assert len(set(uniform) | {0, 1, R - 1}) == 11
    if count == 1:
        return [pc.rand_fr(orc, pyref, n, seed)], [0], [uniform[0]]
    cols = [pc.rand_fr(orc, pyref, n, seed)]
    which, points = [0, 0, 0], [0, 1, R - 1]
    if count == 8:
        cols += [pc.rand_fr(orc, pyref, n, seed + 1), np.zeros((n, 4), dtype=np.uint64)] + [pc.rand_fr(orc, pyref, n, seed + 2 + i) for i in range(3)]
        which += [1, 2, 3, 4, 5]
        points += uniform[:5]
    return cols, which, points


def _check_division_batch(be, orc, pyref, n, count, seed=0, columns=None):
    R = pyref.R
    cols, which, points = columns if columns is not None else _division_columns(orc, pyref, n, count, seed)
    assert len(which) == len(points) == count and len(set(points)) == count
    ints = [orc.fr_to_ints(c) for c in cols]
    dev = [be.to_device(c) for c in cols]
    outs = [be.alloc(n * 32) for _ in range(count)]
    single = be.alloc(n * 32)
    pts = orc.fr_from_ints(points)
    try:
        be.kate_division_batch_dev([dev[w] for w in which], n, pts, outs)
        for c in range(count):
            got = outs[c].download((n - 1, 4))
            be.kate_division_dev(dev[which[c]], n, pts[c], single)
            assert (got == single.download((n - 1, 4))).all(), ("batch vs single call", c)
            assert (got == orc.fr_from_ints(_horner_quotient(ints[which[c]], points[c], R))).all(), ("batch vs Horner over Python integers", c)
        for w, col in enumerate(cols):
            assert (dev[w].download((n, 4)) == col).all(), "a division changed its input"
    finally:
        for d in dev + outs + [single]:
            d.free()


DIVISION_CASES = [(n, count) for n in (2, 3, 2047, 2048, 2049, 4097) for count in (1, 3, 8)]


@pytest.mark.parametrize("n,count", DIVISION_CASES)
def test_emulated_division_batch(emu, orc, pyref, n, count):
    _check_division_batch(emu, orc, pyref, n, count, seed=n + count)


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", DIVISION_CASES)
def test_gpu_division_batch(gpu, orc, pyref, n, count):
    _check_division_batch(gpu, orc, pyref, n, count, seed=n + count)


@pytest.mark.gpu
def test_gpu_division_batch_second_carry_round(gpu, orc, pyref):
    """258 workgroups per column: the carry kernel's one workgroup per column handles 256 pairs a round, so the last two carry-ins come from its second round"""
    n = (1 << 19) + 2049
    assert -(-n // 2048) == 258
    R = pyref.R
    cols = [pc.rand_fr(orc, pyref, n, 5), pc.rand_fr(orc, pyref, n, 6)]
    points = [R - 1] + orc.fr_to_ints(pc.rand_fr(orc, pyref, 2, 7))
    _check_division_batch(gpu, orc, pyref, n, 3, columns=(cols, [0, 1, 0], points))


def _check_division_refusals(be, orc, pyref):
    n = 5
    a = be.to_device(pc.rand_fr(orc, pyref, n, 1))
    q1, q2 = be.alloc(n * 32), be.alloc(n * 32)
    pts = orc.fr_from_ints([3, 4])

    def refused(a_devs, n_, q_devs):
        with pytest.raises(z.ZkError) as e:
            be.kate_division_batch_dev(a_devs, n_, pts, q_devs)
        assert e.value.code == -1, str(e.value)
    try:
        refused([a, 0], n, [q1, q2])
        refused([a, a], n, [q1, 0])
        refused([a, a], n, [q1, q1])
        refused([a, a], n, [q1, a])
        refused([a, a], 1, [q1, q2])                                              # n below 2, as for the single call
        refused([a, a], (1 << 27) + 1, [q1, q2])
    finally:
        for d in (a, q1, q2):
            d.free()


def test_emulated_division_batch_refusals(emu, orc, pyref):
    _check_division_refusals(emu, orc, pyref)


@pytest.mark.gpu
def test_gpu_division_batch_refusals(gpu, orc, pyref):
    _check_division_refusals(gpu, orc, pyref)
