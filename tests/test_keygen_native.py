"""Native keygen — zk_plonk_keygen_vk / _columns / _pk / _release (include/zkmi355.h; csrc/pk.hip: mapping_check + sigma_from_mapping) and their Python side
(Backend.plonk_keygen_*, plonk.keygen_vk_native, plonk.NativeKey.from_keygen).

The reference is oracle/prover.py — the sigma values its keygen derives from an Assembly's mapping and its commit_lagrange — compared exactly: sigma columns bit for
bit, commitments as canonical affine points (and the 96-byte form: z = Montgomery 1, or all zero for the identity).  The mappings are tests/keygen_cases.py.
Every check runs on the kernel emulator and, marked gpu, on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd._lib import KeygenDesc
from zk_dcap_verifier_amd.fields import g1_affine_ints

import keygen_cases as kc
import phased_cases as pc
import phased_verifier as pv
import random_circuits as rc
import test_create_proof as tcp

ZK_ERR_ARG = -1
KS, MS, FIXED_COUNTS = (1, 2, 5, 6, 7, 11), (1, 3, 17), (0, 1, 5)
STRIDE_WGS = {7: 1, 11: 3}                            # keygen_wgs for the grid-stride runs: 2^7 m and 2^11 m cells on 256 and 768 threads
ORACLE_MAX_K = 7                                      # the oracle's SRS is built point by point: above this the commitments are compared with zk_msm_batch_dev


# ---- the reference, computed once per process and shared ------------------------------------------------------------------------------------------------
_REF = {}


def _oracle_params(k):
    import prover as op
    if ("params", k) not in _REF:
        _REF["params", k] = op.Params(k, tcp.TAU)
    return _REF["params", k]


def _srs(be, orc, k):
    """a g_lagrange table of 2^k points on `be`: the oracle's own up to ORACLE_MAX_K, a synthetic table above (there the reference is the library's MSM on the same table)"""
    key = ("srs", id(be), k)
    if key not in _REF:
        bases = _oracle_params(k).g_lagrange if k <= ORACLE_MAX_K else orc.gen_bases_arith(5, 3, 1 << k)
        _REF[key] = be.bases_register(np.ascontiguousarray(bases))
    return _REF[key]


def _mapping_ref(orc, k, m, name):
    key = ("map", k, m, name)
    if key not in _REF:
        mc, mr = kc.MAPPINGS[name](m, 1 << k)
        assert kc.is_permutation(mc, mr), name
        ints = kc.sigma_ints(mc, mr, k)
        if name == "random_copies":
            assert ints == kc.oracle_keygen_sigma(m, k, kc.random_copies_list(m, 1 << k)), "sigma_ints() has drifted from oracle/prover.py's keygen"
        _REF[key] = (mc, mr, [orc.fr_from_ints(col) for col in ints])
    return _REF[key]


def _fixed_ref(orc, k, count, seed):
    key = ("fixed", k, count, seed)
    if key not in _REF:
        ints = kc.fixed_columns(1 << k, count, seed)
        _REF[key] = (ints, [orc.fr_from_ints(col) for col in ints])
    return _REF[key]


def _commit_ref(k, name, ints):
    """oracle commit_lagrange of one column -> canonical affine (x, y) or None for the identity"""
    key = ("commit", k, name)
    if key not in _REF:
        pt = _oracle_params(k).commit_lagrange(ints)
        _REF[key] = None if pt is None or not any(pt) else tuple(int(v) for v in pt)
    return _REF[key]


def _check_points(points, want):
    """96-byte points of zk_msm's normalised form against canonical affine points (None = identity)"""
    from zk_dcap_verifier_amd.fields import fq_mont
    one = np.asarray(fq_mont(1), dtype=np.uint64).reshape(4)
    assert len(points) == len(want)
    for row, w in zip(points, want):
        if w is None:
            assert not row.any(), "an all-zero column commits to (0, 0, 0)"
        else:
            assert (row[8:12] == one).all() and g1_affine_ints(row) == w


# ---- 1 + 2: sigma columns bit for bit, commitments --------------------------------------------------------------------------------------------------------
def _sigma_and_commitments(be, orc, k, m):
    """all six mappings at (k, m); mapping i meets FIXED_COUNTS[(i + k + m) % 3] fixed columns, so every (k, m) sees 0, 1 and 5 fixed columns and every mapping each
    of them at some size.  Two further runs, independent of each other: the fixed columns borrowed from the device wherever there are five, and at k = 7 and 11 the
    launch capped to 1 and 3 workgroups on host pointers: more cells than one grid stride on any device."""
    n = 1 << k
    srs = _srs(be, orc, k)
    for i, name in enumerate(kc.MAPPINGS):
        mc, mr, sigma_ref = _mapping_ref(orc, k, m, name)
        n_fixed = FIXED_COUNTS[(i + k + m) % 3]
        fixed_ints, fixed_ref = _fixed_ref(orc, k, n_fixed, i)
        fc, pcm, kg = be.plonk_keygen_vk(k, fixed_ref, mc, mr, srs)
        h = plonk.NativeKeygen(be, kg, k, n_fixed, m)
        fixed_dev, sigma_dev = h.columns()
        got_fixed, got_sigma = h.download()
        for j in range(m):
            assert (got_sigma[j] == sigma_ref[j]).all(), f"k = {k}, m = {m}, {name}: sigma column {j}"
        for c in range(n_fixed):
            assert (got_fixed[c] == fixed_ref[c]).all()
        if k <= ORACLE_MAX_K:
            _check_points(fc, [_commit_ref(k, ("fixed", n_fixed, i, c), fixed_ints[c]) for c in range(n_fixed)])
            _check_points(pcm, [_commit_ref(k, ("sigma", m, name, j), orc.fr_to_ints(sigma_ref[j])) for j in range(m)])
        else:
            want = be.msm_batch(srs, fixed_dev + sigma_dev, n)
            assert (np.concatenate([fc, pcm]) == want).all()
        if n_fixed == FIXED_COUNTS[-1]:
            # the same fixed columns already on the device (borrowed, never copied): the same bytes
            dev = [be.to_device(a) for a in fixed_ref]
            fc2, pc2, kg2 = be.plonk_keygen_vk(k, dev, mc, mr, srs)
            h2 = plonk.NativeKeygen(be, kg2, k, n_fixed, m)
            assert dev and h2.columns()[0] == [int(d.ptr) for d in dev]
            assert (fc2 == fc).all() and (pc2 == pcm).all() and all((a == b).all() for a, b in zip(h2.download()[1], got_sigma))
            h2.release()
            for d in dev:
                d.free()
        if k in STRIDE_WGS and name in ("full_cycle", "random_copies"):
            # host pointers again with the launch capped so that every thread walks several grid strides (the default cap is never reached at these sizes)
            assert (m << k) > 256 * STRIDE_WGS[k] or m == 1
            be.tune(keygen_wgs=STRIDE_WGS[k])
            try:
                fc3, pc3, kg3 = be.plonk_keygen_vk(k, fixed_ref, mc, mr, srs)
            finally:
                be.tune(keygen_wgs=2048)
            h3 = plonk.NativeKeygen(be, kg3, k, n_fixed, m)
            assert (fc3 == fc).all() and (pc3 == pcm).all() and all((a == b).all() for a, b in zip(h3.download()[1], sigma_ref))
            h3.release()
        h.release()


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
def test_sigma_columns_and_commitments_equal_the_oracle_emulated(emu, orc, k, m):
    _sigma_and_commitments(emu, orc, k, m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
def test_sigma_columns_and_commitments_equal_the_oracle_gpu(gpu, orc, k, m):
    _sigma_and_commitments(gpu, orc, k, m)


def _no_columns_at_all(be, orc):
    """n_fixed = 0 and n_perm_columns = 0 are legal: a handle with nothing in it, NULL outputs"""
    fc, pcm, kg = be.plonk_keygen_vk(5, [], None, None, _srs(be, orc, 5))
    assert fc.shape == (0, 12) and pcm.shape == (0, 12) and be.plonk_keygen_columns(kg, 0, 0) == ([], [])
    be.plonk_keygen_release(kg)
    with pytest.raises(z.ZkError):
        be.plonk_keygen_release(kg)


def test_no_columns_at_all_emulated(emu, orc):
    _no_columns_at_all(emu, orc)


@pytest.mark.gpu
def test_no_columns_at_all_gpu(gpu, orc):
    _no_columns_at_all(gpu, orc)


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _refused_vk(be, srs, k, fixed, mc, mr, text, struct_size=None):
    """ZK_ERR_ARG with `text` in zk_last_error, no byte of the outputs touched, no handle"""
    m = mc.shape[0]
    fc, pcm = np.full((len(fixed), 12), SENTINEL, dtype=np.uint64), np.full((m, 12), SENTINEL, dtype=np.uint64)
    cols = [np.ascontiguousarray(c) for c in fixed]
    arr = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
    mc32, mr32 = np.ascontiguousarray(mc, dtype=np.uint32), np.ascontiguousarray(mr, dtype=np.uint32)
    d = KeygenDesc()
    d.struct_size = C.sizeof(KeygenDesc) if struct_size is None else struct_size
    d.k, d.n_fixed, d.n_perm_columns = k, len(cols), m
    d.fixed_values, d.perm_map_column, d.perm_map_row = C.cast(arr, C.c_void_p).value, mc32.ctypes.data, mr32.ctypes.data
    kg = C.c_uint64(SENTINEL)
    rc_ = be.lib.zk_plonk_keygen_vk(be.ctx, C.byref(d), C.c_uint64(srs), fc.ctypes.data_as(C.c_void_p), pcm.ctypes.data_as(C.c_void_p), C.byref(kg))
    msg = (be.lib.zk_last_error(be.ctx) or b"").decode()
    assert rc_ == ZK_ERR_ARG and text in msg, (rc_, msg)
    assert (fc == SENTINEL).all() and (pcm == SENTINEL).all() and kg.value == SENTINEL


def _refusals_vk(be, orc):
    k, m = 5, 3
    n = 1 << k
    srs = _srs(be, orc, k)
    _, fixed = _fixed_ref(orc, k, 1, 0)
    good_c, good_r, _ = _mapping_ref(orc, k, m, "random_copies")
    mc, mr = good_c.copy(), good_r.copy()
    mc[1, 7] = m                                                      # a column index == m
    mc[2, 9] = m + 5                                                  # (a later one: the FIRST is named)
    _refused_vk(be, srs, k, fixed, mc, mr, f"cell (column 1, row 7) to (column {m}, row {int(mr[1, 7])})")
    mc, mr = good_c.copy(), good_r.copy()
    mr[2, 30] = n                                                     # a row == n
    _refused_vk(be, srs, k, fixed, mc, mr, f"cell (column 2, row 30) to (column {int(mc[2, 30])}, row {n})")
    mc, mr = good_c.copy(), good_r.copy()
    mc[0, 3], mr[0, 3] = mc[2, 4], mr[2, 4]                           # two cells with the same image ...
    mc[1, 1], mr[1, 1] = mc[2, 4], mr[2, 4]                           # ... and a third
    assert not kc.is_permutation(mc, mr)
    _refused_vk(be, srs, k, fixed, mc, mr, "not a permutation of the cells: 2 cells")
    _refused_vk(be, srs, k, fixed, good_c, good_r, "struct_size", struct_size=C.sizeof(KeygenDesc) - 8)
    half = be.bases_register(np.ascontiguousarray(_oracle_params(k).g_lagrange[: n // 2]))      # a rank's slice of a sharded SRS
    _refused_vk(be, half, k, fixed, good_c, good_r, f"srs_g_lagrange holds {n // 2} points")
    be.bases_release(half)
    _refused_vk(be, _srs(be, orc, k + 1), k, fixed, good_c, good_r, f"srs_g_lagrange holds {2 * n} points")      # the table of another k
    _refused_vk(be, 0xDEAD, k, fixed, good_c, good_r, "not a registered table")
    # the context is as usable as before
    fc, pcm, kg = be.plonk_keygen_vk(k, fixed, good_c, good_r, srs)
    _check_points(pcm, [_commit_ref(k, ("sigma", m, "random_copies", j), orc.fr_to_ints(_mapping_ref(orc, k, m, "random_copies")[2][j])) for j in range(m)])
    be.plonk_keygen_release(kg)


def test_keygen_vk_refusals_emulated(emu, orc):
    _refusals_vk(emu, orc)


@pytest.mark.gpu
def test_keygen_vk_refusals_gpu(gpu, orc):
    _refusals_vk(gpu, orc)


def _refusals_pk(be, orc):
    cs, fixed, asm, advice, instances = tcp.toy_circuit(6)
    params = z.kzg.ParamsKZG.setup(6, tcp.TAU, backend=be)
    vk, kg = plonk.keygen_vk_native(params, cs, fixed, asm)
    key = plonk.NativeKey.from_keygen(params, kg, vk)
    good = plonk.PhasedProver(params, key.pk, key=key).create_proof([[a.copy() for a in advice]], [instances], np.random.default_rng(7))

    def refused(text, srs_g=None, srs_g_lagrange=None, **changes):
        host = type(key.host).from_buffer_copy(key.host)
        for name, value in changes.items():
            setattr(host, name, value)
        out = C.c_uint64(SENTINEL)
        rc_ = be.lib.zk_plonk_keygen_pk(be.ctx, C.c_uint64(kg.handle), C.byref(host), C.byref(key.phases), C.c_uint64(params.g.handle if srs_g is None else srs_g),
                                        C.c_uint64(params.g_lagrange.handle if srs_g_lagrange is None else srs_g_lagrange), C.byref(out))
        msg = (be.lib.zk_last_error(be.ctx) or b"").decode()
        assert rc_ == ZK_ERR_ARG and text in msg and out.value == SENTINEL, (rc_, msg, out.value)
    column = np.zeros((64, 4), dtype=np.uint64)
    ptrs = (C.c_void_p * max(1, cs.num_fixed_columns))(*[column.ctypes.data] * cs.num_fixed_columns)
    refused("must be NULL", fixed_values=C.cast(ptrs, C.c_void_p).value)
    refused("must be NULL", sigma_values=C.cast(ptrs, C.c_void_p).value)
    refused("the keygen handle holds k = 6", k=7)
    refused("the keygen handle holds", n_fixed=cs.num_fixed_columns + 1)
    refused("shard_world 2", shard_world=2)
    refused("struct_size", struct_size=C.sizeof(key.host) + 8)
    half = be.bases_register(np.ascontiguousarray(_oracle_params(6).g[:32]))                      # a rank's slice of a sharded SRS in either place
    refused("srs_g holds 32 points", srs_g=half)
    refused("srs_g_lagrange holds 32 points", srs_g_lagrange=half)
    be.bases_release(half)
    # the context, the handle and the key are as usable as before
    again = plonk.NativeKey.from_keygen(params, kg, vk)
    for k_ in (key, again):
        assert plonk.PhasedProver(params, k_.pk, key=k_).create_proof([[a.copy() for a in advice]], [instances], np.random.default_rng(7)) == good == tcp._golden(tcp.GOLDEN_PROOF)
        k_.release()
    kg.release()
    params.release()


def test_keygen_pk_refusals_emulated(emu, orc):
    _refusals_pk(emu, orc)


@pytest.mark.gpu
def test_keygen_pk_refusals_gpu(gpu, orc):
    _refusals_pk(gpu, orc)


# ---- 4: the whole path -------------------------------------------------------------------------------------------------------------------------------------
def _both_routes(be, params, cs, fixed, asm, advices, instances_list, seed, next_phase=None, piece_cosets=None):
    """keygen() + NativeKey against keygen_vk_native + from_keygen under the same seed -> (the one proof both emit, the vk of the new route)"""
    pk = plonk.keygen(params, cs, fixed, asm, piece_cosets=piece_cosets)
    old = plonk.PhasedProver(params, pk)
    want = old.create_proof([[c if c is None else c.copy() for c in per] for per in advices], instances_list, np.random.default_rng(seed), next_phase)
    old.release()
    vk, kg = plonk.keygen_vk_native(params, cs, fixed, asm)
    assert vk.fixed_commitments == pk.vk.fixed_commitments and vk.permutation_commitments == pk.vk.permutation_commitments and vk.transcript_repr == pk.vk.transcript_repr
    for a, b in zip(kg.download()[1], pk.sigma_values):
        assert (a == b.download(a.shape)).all()
    pk.release()
    key = plonk.NativeKey.from_keygen(params, kg, vk)
    kg.release()                                                      # (the key keeps the columns)
    prover = plonk.PhasedProver(params, key.pk, key=key)
    got = prover.create_proof([[c if c is None else c.copy() for c in per] for per in advices], instances_list, np.random.default_rng(seed), next_phase)
    key.release()
    assert got == want, "the two keygen routes prove different bytes"
    return got, vk


def _goldens(be):
    import verifier
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sgx_shaped_circuit as sc
    cs, fixed, asm, advice, instances = tcp.toy_circuit(6)
    params = z.kzg.ParamsKZG.setup(6, tcp.TAU, backend=be)
    proof, vk = _both_routes(be, params, cs, fixed, asm, [advice], [instances], 7)
    assert proof == tcp._golden(tcp.GOLDEN_PROOF) and verifier.verify_proof(vk, tcp.TAU, instances, proof) is True
    params.release()
    cs, fixed, asm, advice = sc.build(z, be, 8, census="chip_estimate")
    params = z.kzg.ParamsKZG.setup(8, tcp.TAU, backend=be)
    proof, vk = _both_routes(be, params, cs, fixed, asm, [advice], [[]], 3)
    assert proof == tcp._golden(tcp.GOLDEN_SGX) and verifier.verify_proof(vk, tcp.TAU, [], proof) is True
    params.release()


def test_goldens_through_native_keygen_emulated(emu, orc):
    _goldens(emu)


@pytest.mark.gpu
def test_goldens_through_native_keygen_gpu(gpu, orc):
    _goldens(gpu)


RANDOM_CIRCUITS = ((6, 5), (8, 11))                                   # (k, seed); asserted below: both have lookups, equality-enabled columns and copies


def _random_circuit(be, k, seed):
    cs, fixed, asm, advice, instances = rc.random_circuit(k, seed)
    assert cs.permutation_columns and cs.lookups and asm.copies
    params = z.kzg.ParamsKZG.setup(k, tcp.TAU, backend=be)
    # The witness of a random circuit does not satisfy its gates (tests/random_circuits.py: create_proof never checks them), so the oracle's verifier has nothing to
    # accept here; its independent CPU prover has: the same circuit, copies and draws give the same bytes.  For an unsatisfied witness that holds on halo2's own
    # route only — every identity on every row of the whole extended domain (include/zkmi355.h, "quot_degree_split"; tests/test_random_circuits.py does the same).
    be.tune(quot_degree_split=0, quot_piece_cosets=0)
    try:
        proof, vk = _both_routes(be, params, cs, fixed, asm, [advice], [instances], 11, piece_cosets=False)
    finally:
        be.tune(quot_degree_split=1, quot_piece_cosets=1)
    params.release()
    if ("oracle_proof", k, seed) not in _REF:
        _REF["oracle_proof", k, seed] = rc.oracle_proof(k, tcp.TAU, cs, fixed, asm, advice, instances, 11)
    assert proof == _REF["oracle_proof", k, seed]


@pytest.mark.parametrize("k,seed", RANDOM_CIRCUITS)
def test_random_circuits_through_native_keygen_emulated(emu, orc, k, seed):
    _random_circuit(emu, k, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("k,seed", RANDOM_CIRCUITS)
def test_random_circuits_through_native_keygen_gpu(gpu, orc, k, seed):
    _random_circuit(gpu, k, seed)


def _phased(be, name, k):
    case = pc.CASES[name](k)
    params = z.kzg.ParamsKZG.setup(k, tcp.TAU, backend=be)
    proof, vk = _both_routes(be, params, case.cs, case.fixed, case.asm, case.phase0(), case.instances, 5, case.next_phase())
    assert pv.verify_proof_phased(vk, tcp.TAU, case.instances, proof) is True
    params.release()


@pytest.mark.parametrize("name,k", [("A", 6), ("B", 8)])
def test_phased_circuits_through_native_keygen_emulated(emu, orc, name, k):
    _phased(emu, name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("A", 6), ("B", 8)])
def test_phased_circuits_through_native_keygen_gpu(gpu, orc, name, k):
    _phased(gpu, name, k)


# ---- 5: lifetime -------------------------------------------------------------------------------------------------------------------------------------------
def _lifetime(be, second):
    """the columns live as long as the handle OR any key built from it: handle first, key first with a shared key on a second context, and a context destroyed
    with a handle and a key still on it"""
    cs, fixed, asm, advice, instances = tcp.toy_circuit(6)
    golden = tcp._golden(tcp.GOLDEN_PROOF)
    params = z.kzg.ParamsKZG.setup(6, tcp.TAU, backend=be)

    def prove(key, prm):
        return plonk.PhasedProver(prm, key.pk, key=key).create_proof([[a.copy() for a in advice]], [instances], np.random.default_rng(7))
    vk, kg = plonk.keygen_vk_native(params, cs, fixed, asm)
    key = plonk.NativeKey.from_keygen(params, kg, vk)
    kg.release()                                                      # the handle before the key
    assert prove(key, params) == golden
    key.release()
    vk, kg = plonk.keygen_vk_native(params, cs, fixed, asm)
    key = plonk.NativeKey.from_keygen(params, kg, vk)
    params2 = z.kzg.ParamsKZG.shared_with(params, second)
    shared = key.shared_with(second, params2)
    shared.pk = plonk.KeyView(vk, second)
    key.release()                                                     # the key before the handle; its share on the other context lives on
    assert prove(shared, params2) == golden
    kg.release()
    assert prove(shared, params2) == golden                           # ... after the handle is gone too
    shared.release()
    # what a context still holds goes with it
    vk, kg2 = plonk.keygen_vk_native(params2, cs, fixed, asm)
    plonk.NativeKey.from_keygen(params2, kg2, vk)
    params2.release()
    second.close()
    params.release()


def test_lifetime_of_the_shared_columns_emulated(emu, orc):
    from conftest import EMU_SO
    second = z.Backend(0, lib_path=EMU_SO)
    second.tune(msm_sort_threads=64, msm_sort_wgs=3, msm_block=32, ntt_threads=32, ntt_tile_log=6, ntt_max_radix_log=4, msm_target_threads=64, msm_min_chunk=2, vec_block=32,
                quot_threads=32)
    _lifetime(emu, second)
    # every device buffer of a handle and its key comes back (the context's caches are warm by now: a second round allocates what it frees)
    live = emu.lib.zk_test_live_device_allocs
    live.restype = C.c_long
    cs, fixed, asm, advice, instances = tcp.toy_circuit(6)
    params = z.kzg.ParamsKZG.setup(6, tcp.TAU, backend=emu)
    counts = []
    for release_key_first in (False, True, False):
        vk, kg = plonk.keygen_vk_native(params, cs, fixed, asm)
        key = plonk.NativeKey.from_keygen(params, kg, vk)
        for obj in ((key, kg) if release_key_first else (kg, key)):
            obj.release()
        emu.trim_pool()
        counts.append(live())
    params.release()
    assert counts[0] == counts[1] == counts[2], counts


@pytest.mark.gpu
def test_lifetime_of_the_shared_columns_gpu(gpu, orc):
    _lifetime(gpu, z.Backend(0))
