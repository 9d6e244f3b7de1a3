"""halo2_proofs::plonk::{keygen_vk, keygen_pk}, MI355X edition.

Mirrors (halo2_proofs 0.2.0 @ zkwebauthn c254c75, Cargo.lock:1314-1327) src/plonk/keygen.rs as the reference calls it at
circuits/src/sgx_dcap_verifier.rs:803,807: commit the fixed and permutation (sigma) columns (MSM),
bring them to coefficient form and to the extended coset (NTT), build l_0 / l_last / l_active_row, and compile the
Evaluator (`Evaluator::new(cs)`, src/plonk/evaluation.rs) — here into the ZKQ1 program the quotient kernel runs.
Everything a proof reuses stays resident in HBM inside the ProvingKey.

Deviation that cannot be closed without the pinned crate: `vk.transcript_repr` (halo2 hashes the Debug rendering of the
pinned verifying key) is replaced by a Blake2b digest of (k, column counts, commitments) — same role, different bytes.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .. import evaluation as ev
from .._lib import Backend
from ..domain import EvaluationDomain
from ..fields import DELTA, R_MOD, fr_mont, fr_mont_array, g1_affine_ints
from ..kzg import ParamsKZG
from .circuit import Assembly, ConstraintSystem
from .expression import GraphBuilder


@dataclass
class VerifyingKey:
    k: int
    cs: ConstraintSystem
    fixed_commitments: list          # canonical affine (x, y) or None
    permutation_commitments: list
    transcript_repr: int = 0

    def hash_into(self, transcript) -> None:
        transcript.common_scalar(self.transcript_repr)


@dataclass
class ProvingKey:
    vk: VerifyingKey
    domain: EvaluationDomain
    backend: Backend
    fixed_values: list               # device, Lagrange
    fixed_polys: list                # device, coefficient form
    fixed_cosets: list               # device, extended coset
    sigma_values: list
    sigma_polys: list
    sigma_cosets: list
    l0: object
    l_last: object
    l_active_row: object
    evaluator: ev.Evaluator
    program: ev.Program
    lookup_compressors: list = field(default_factory=list)   # per lookup: (input Evaluator, table Evaluator) over the 2^k rows
    coset_parts: Optional[dict] = None   # params.by_cosets(): coset j -> {"fixed", "sigma", "l"}: the 2^k values of that coset only (this rank's cosets)
    borrowed: bool = False               # shared_with(): the columns belong to another ProvingKey of the process (same GPU); only the program handles are this key's
    owner: Optional["ProvingKey"] = None  # shared_with(): whose columns these are
    borrowers: int = 0                   # keys of other contexts that share this key's columns (an owner with borrowers refuses release())
    pieces_from_cosets: bool = False     # one GPU, cs_degree - 1 < 2^(extended_k - k): coset_parts holds cosets 0 .. cs_degree-2 and there are NO extended forms — the prover
                                         # evaluates h(X)'s numerator on those cosets only and takes the pieces from zk_cosets_to_pieces_dev

    @classmethod
    def shared_with(cls, other: "ProvingKey", backend: Backend) -> "ProvingKey":
        """The same proving key for another context on the same GPU (one context per host thread that proves concurrently): every column and every compiled
        program is SHARED with `other` — one proving key per process (≈2.3 GB at k = 19) instead of one per context, one keygen instead of N.  `other` must
        outlive the borrower's proofs; release() of a borrower returns only its program handles."""
        assert other.coset_parts is None or other.pieces_from_cosets, "sharded keys are per rank"
        ev_ = ev.Evaluator.shared(other.evaluator, backend)
        comps = [(ev.Evaluator.shared(a, backend), ev.Evaluator.shared(b, backend)) for a, b in other.lookup_compressors]
        root = other.owner or other
        root.borrowers += 1
        return cls(other.vk, EvaluationDomain(other.vk.cs.degree(), other.vk.k, backend=backend), backend, other.fixed_values, other.fixed_polys, other.fixed_cosets,
                   other.sigma_values, other.sigma_polys, other.sigma_cosets, other.l0, other.l_last, other.l_active_row, ev_, other.program, comps, other.coset_parts, True,
                   owner=root, pieces_from_cosets=other.pieces_from_cosets)

    def release(self):
        if not self.borrowed and self.borrowers:
            raise RuntimeError(f"ProvingKey.release: {self.borrowers} borrowed key(s) still share these columns (shared_with): release them first")
        self.evaluator.release()
        for a, b in self.lookup_compressors:
            a.release()
            b.release()
        if self.borrowed:
            if self.owner is not None:
                self.owner.borrowers -= 1
                self.owner = None
            return
        for grp in (self.fixed_values, self.fixed_polys, self.fixed_cosets, self.sigma_values, self.sigma_polys, self.sigma_cosets,
                    [d for d in (self.l0, self.l_last, self.l_active_row) if d is not None],
                    *[v for part in (self.coset_parts or {}).values() for v in part.values()]):
            for d in grp:
                d.free()


def compile_program(cs: ConstraintSystem, k: int, extended_k: int) -> ev.Program:
    """Evaluator::new(cs): custom gates folded with Horner in y; one graph per lookup ending in
    (theta-compressed input + beta) * (theta-compressed table + gamma)."""
    gb = GraphBuilder()
    parts = [gb.add_expression(g) for g in cs.gates]
    gb.add_calculation(ev.HORNER, ev.vs(ev.PREVIOUS), parts, ev.vs(ev.Y))
    lookups = []
    for lk in cs.lookups:
        lb = GraphBuilder()

        def lc(exprs, lb=lb):
            ps = [lb.add_expression(e) for e in exprs]
            return lb.add_calculation(ev.HORNER, ev.vs(ev.CONSTANT, 0), ps, ev.vs(ev.THETA))
        cin, ctab = lc(lk.input_expressions), lc(lk.table_expressions)
        right = lb.add_calculation(ev.ADD, ctab, ev.vs(ev.GAMMA))
        left = lb.add_calculation(ev.ADD, cin, ev.vs(ev.BETA))
        lb.add_calculation(ev.MUL, left, right)
        lookups.append(lb.graph)
    return ev.Program(k=k, extended_k=extended_k, n_fixed=cs.num_fixed_columns, n_advice=cs.num_advice_columns,
                      n_instance=cs.num_instance_columns, n_challenges=cs.num_challenges, blinding_factors=cs.blinding_factors(), cs_degree=cs.degree(),
                      perm_columns=list(cs.permutation_columns), custom_gates=gb.graph, lookups=lookups)


def compressor_program(cs: ConstraintSystem, k: int, exprs) -> ev.Program:
    """lookup::Argument::commit_permuted's compress_expressions as a program over the Lagrange columns (extended_k = k)."""
    gb = GraphBuilder()
    ps = [gb.add_expression(e) for e in exprs]
    gb.add_calculation(ev.HORNER, ev.vs(ev.CONSTANT, 0), ps, ev.vs(ev.THETA))
    return ev.expression_program(k, cs.num_fixed_columns, cs.num_advice_columns, cs.num_instance_columns, cs.num_challenges, gb.graph)


def _extended_k(cs: ConstraintSystem, k: int) -> int:
    """EvaluationDomain::new(cs.degree(), k): the smallest extended domain that holds a quotient of degree (cs.degree() - 1) * 2^k"""
    ek = k
    while (1 << ek) < (1 << k) * (cs.degree() - 1):
        ek += 1
    return ek


def _programs(cs: ConstraintSystem, k: int, extended_k: int):
    """every ZKQ1 program of a key -> (Evaluator program, per lookup its input program, per lookup its table program): one place for keygen() and
    NativeKey.from_keygen, whose proofs are equal byte for byte only while they compile the same programs"""
    return (compile_program(cs, k, extended_k), [compressor_program(cs, k, lk.input_expressions) for lk in cs.lookups],
            [compressor_program(cs, k, lk.table_expressions) for lk in cs.lookups])


@dataclass
class KeyView:
    """what a key built by NativeKey.from_keygen has in a ProvingKey's place: the verifying key and the backend (the columns are the library's)"""
    vk: VerifyingKey
    backend: Backend


class NativeKeygen:
    """The handle of zk_plonk_keygen_vk: the fixed and sigma columns in Lagrange form, resident in HBM, shared with every key built from it (NativeKey.from_keygen)."""

    def __init__(self, backend: Backend, handle: int, k: int, n_fixed: int, n_perm_columns: int):
        self.backend, self.handle, self.k, self.n_fixed, self.n_perm_columns = backend, handle, k, n_fixed, n_perm_columns

    def columns(self):
        """(fixed, sigma): device pointers of the Lagrange columns, valid until release()"""
        return self.backend.plonk_keygen_columns(self.handle, self.n_fixed, self.n_perm_columns)

    def download(self):
        """(fixed, sigma) as (2^k, 4) uint64 Montgomery arrays"""
        import ctypes as C
        be, n = self.backend, 1 << self.k

        def get(ptr):
            out = np.empty((n, 4), dtype=np.uint64)
            be._ck(be.lib.zk_dev_download(be.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes)))
            return out
        fx, sg = self.columns()
        return [get(p) for p in fx], [get(p) for p in sg]

    def release(self):
        if self.handle:
            self.backend.plonk_keygen_release(self.handle)
            self.handle = 0


def keygen_vk_native(params: ParamsKZG, cs: ConstraintSystem, fixed_columns, assembly: Optional[Assembly] = None):
    """keygen_vk through zk_plonk_keygen_vk -> (VerifyingKey, NativeKeygen): the sigma columns are built on the device from the copy mapping (Assembly.map_c / map_r;
    None = the identity mapping) and every fixed and sigma column is committed in one batch — no identity column is downloaded, no sigma column uploaded.  The
    VerifyingKey equals keygen()'s (same commitments, same transcript_repr), so both routes prove the same bytes; NativeKey.from_keygen builds the proving key."""
    be, k, n = params.backend, params.k, params.n
    assert params.world == 1, "keygen runs on one GPU with the whole table"
    assert len(fixed_columns) == cs.num_fixed_columns
    assert n > cs.blinding_factors() + 1 + 1, "circuit does not fit: not enough usable rows"
    m = len(cs.permutation_columns)
    asm = (assembly or Assembly(cs, k)) if m else None
    fc, pc, handle = be.plonk_keygen_vk(k, [_as_mont(c, n) for c in fixed_columns], asm.map_c if m else None, asm.map_r if m else None, params.g_lagrange.handle)
    fixed_commitments = [g1_affine_ints(r) for r in fc]
    permutation_commitments = [g1_affine_ints(r) for r in pc]
    vk = VerifyingKey(k, cs, fixed_commitments, permutation_commitments, _transcript_repr(k, cs, fixed_commitments, permutation_commitments))
    return vk, NativeKeygen(be, handle, k, cs.num_fixed_columns, m)


class NativeKey:
    """The library's own proving-key object for `pk` (zk_plonk_pk_build_phased, csrc/pk.hip): built from the Lagrange columns keygen left on the device (borrowed: `pk` must
    outlive it), the ZKQ1 blobs and the circuit's phase lists.  What a Rust or C caller holds instead of a ProvingKey; plonk.native.PhasedProver proves with it."""

    def __init__(self, params: ParamsKZG, pk: "ProvingKey", transcript: int = 0):
        import ctypes as C
        from .._lib import _dptr
        be = pk.backend
        assert params.world == 1, "one proof over several GPUs is single-phase (zk_plonk_pk_build_phased refuses shard_world > 1)"
        h, ph, keep, ptrs = self._host(params, pk.vk, pk.program, [a.program for a, _ in pk.lookup_compressors], [b.program for _, b in pk.lookup_compressors], transcript)
        h.fixed_values, h.sigma_values, h.values_on_device = ptrs([_dptr(d) for d in pk.fixed_values]), ptrs([_dptr(d) for d in pk.sigma_values]), 1
        self.host, self.phases, self._keep = h, ph, keep               # (kept: tests rebuild with altered copies)
        self.backend, self.pk = be, pk
        out = C.c_uint64()
        be._ck(be.lib.zk_plonk_pk_build_phased(be.ctx, C.byref(h), C.byref(ph), C.c_uint64(params.g.handle), C.c_uint64(params.g_lagrange.handle), C.byref(out)))
        self.handle = out.value

    @staticmethod
    def _host(params: ParamsKZG, vk: "VerifyingKey", program, input_programs, table_programs, transcript: int):
        """zk_plonk_pk_host and zk_plonk_phases of a circuit, the column pointers left NULL -> (host, phases, what they point into, ptrs())"""
        import ctypes as C
        from .._lib import PlonkPhases
        from .native import PkHost
        cs = vk.cs
        keep = []

        def u32(vals):
            a = np.ascontiguousarray(np.asarray(vals, dtype=np.int64).astype(np.uint32).reshape(-1))
            keep.append(a)
            return a.ctypes.data if a.size else None

        def ptrs(vals):
            arr = (C.c_void_p * max(1, len(vals)))(*vals)
            keep.append(arr)
            return C.cast(arr, C.c_void_p).value

        def blobs(programs):
            bufs = [(C.c_char * len(b)).from_buffer_copy(b) for b in (p.to_blob() for p in programs)]
            keep.extend(bufs)
            lens = (C.c_size_t * max(1, len(bufs)))(*[len(b) for b in bufs])
            keep.append(lens)
            return ptrs([C.addressof(b) for b in bufs]), C.cast(lens, C.c_void_p).value
        keys, key_ids = {}, []
        for lk in cs.lookups:
            key_ids.append(keys.setdefault(tuple(lk.table_expressions), len(keys)))
        h = PkHost()
        h.struct_size = C.sizeof(PkHost)
        h.k, h.cs_degree, h.blinding_factors = params.k, cs.degree(), cs.blinding_factors()
        h.n_fixed, h.n_advice, h.n_instance = cs.num_fixed_columns, cs.num_advice_columns, cs.num_instance_columns
        h.n_lookups, h.n_perm_columns = len(cs.lookups), len(cs.permutation_columns)
        h.perm_columns = u32([v for t, i in cs.permutation_columns for v in (t, i)])
        aq, fq = cs.advice_queries(), cs.fixed_queries()
        h.advice_queries, h.n_advice_queries = u32([v for c, r in aq for v in (c, r)]), len(aq)
        h.fixed_queries, h.n_fixed_queries = u32([v for c, r in fq for v in (c, r)]), len(fq)
        ev_blob = (C.c_char * len(program.to_blob())).from_buffer_copy(program.to_blob())
        keep.append(ev_blob)
        h.evaluator_zkq1, h.evaluator_zkq1_len = C.addressof(ev_blob), len(ev_blob)
        h.lookup_input_zkq1, h.lookup_input_zkq1_len = blobs(input_programs)
        h.lookup_table_zkq1, h.lookup_table_zkq1_len = blobs(table_programs)
        h.lookup_table_key = u32(key_ids)
        repr_bytes = np.frombuffer(int(vk.transcript_repr).to_bytes(32, "little"), dtype=np.uint8).copy()
        keep.append(repr_bytes)
        h.transcript_repr, h.transcript, h.draw_schedule = repr_bytes.ctypes.data, transcript, 1
        ph = PlonkPhases()
        ph.struct_size = C.sizeof(PlonkPhases)
        ap = np.asarray(cs._advice_phases(), dtype=np.uint8)
        cp = np.asarray(cs.challenge_phase, dtype=np.uint8)
        keep += [ap, cp]
        ph.n_advice, ph.advice_phase = len(ap), ap.ctypes.data if ap.size else None
        ph.n_challenges, ph.challenge_phase = len(cp), cp.ctypes.data if cp.size else None
        return h, ph, keep, ptrs

    @classmethod
    def from_keygen(cls, params: ParamsKZG, kg: "NativeKeygen", vk: "VerifyingKey", transcript: int = 0) -> "NativeKey":
        """keygen_pk on the columns keygen_vk_native left in HBM (zk_plonk_keygen_pk): no column crosses the link again and sigma is not recomputed.  The key shares
        the columns with `kg`: either may be released first.  `.pk` is a KeyView (vk + backend), which is what plonk.PhasedProver(params, key.pk, key=key) reads."""
        assert params.world == 1, "keygen runs on one GPU with the whole table (zk_plonk_keygen_pk refuses shard_world > 1)"
        program, input_programs, table_programs = _programs(vk.cs, params.k, _extended_k(vk.cs, params.k))
        self = cls.__new__(cls)
        self.host, self.phases, self._keep, _ = cls._host(params, vk, program, input_programs, table_programs, transcript)
        self.backend, self.pk = kg.backend, KeyView(vk, kg.backend)
        self.handle = kg.backend.plonk_keygen_pk(kg.handle, self.host, self.phases, params.g.handle, params.g_lagrange.handle)
        return self

    def shared_with(self, backend, params: ParamsKZG) -> "NativeKey":
        """the same key for another context of the same GPU (zk_plonk_pk_share); `params` is that context's SRS"""
        import ctypes as C
        other = NativeKey.__new__(NativeKey)
        other.host, other.phases, other._keep, other.backend, other.pk = self.host, self.phases, self._keep, backend, self.pk
        out = C.c_uint64()
        backend._ck(backend.lib.zk_plonk_pk_share(backend.ctx, self.backend.ctx, C.c_uint64(self.handle), C.c_uint64(params.g.handle), C.c_uint64(params.g_lagrange.handle), C.byref(out)))
        other.handle = out.value
        return other

    def release(self):
        import ctypes as C
        if self.handle:
            self.backend._ck(self.backend.lib.zk_plonk_pk_release(self.backend.ctx, C.c_uint64(self.handle)))
            self.handle = 0


def _transcript_repr(k: int, cs: ConstraintSystem, fixed_commitments, permutation_commitments) -> int:
    """vk.transcript_repr of this package (module docstring): one hash for keygen() and keygen_vk_native(), so that both routes prove the same bytes"""
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    h.update(repr((k, cs.num_fixed_columns, cs.num_advice_columns, cs.num_instance_columns, len(cs.gates), len(cs.lookups),
                   cs.permutation_columns, cs.degree(), fixed_commitments, permutation_commitments)).encode())
    if cs.is_phased():                                                   # (halo2's pinned vk renders advice_column_phase / challenge_phase too; single-phase circuits keep their bytes)
        h.update(repr(("phases", cs._advice_phases(), list(cs.challenge_phase))).encode())
    return int.from_bytes(h.digest(), "little") % R_MOD


def _as_mont(col, n) -> np.ndarray:
    if isinstance(col, np.ndarray) and col.dtype == np.uint64:
        a = np.ascontiguousarray(col).reshape(-1, 4)
    else:
        a = fr_mont_array(col)
    assert a.shape[0] == n, "column length must be 2^k"
    return a


def keygen(params: ParamsKZG, cs: ConstraintSystem, fixed_columns, assembly: Optional[Assembly] = None, piece_cosets: Optional[bool] = None) -> ProvingKey:
    """keygen_vk + keygen_pk.  fixed_columns: cs.num_fixed_columns columns of n = 2^k rows, either (n, 4) uint64
    Montgomery arrays or lists of canonical ints (selectors included, as halo2 hands them over after compression);
    assembly: the copy constraints (None = no equality-enabled columns).  piece_cosets (default on): on one GPU, when cs_degree - 1 is not a power of two, keep the
    key's columns on cosets 0 .. cs_degree-2 only (ProvingKey.pieces_from_cosets) — False builds the extended forms halo2's keygen_pk builds."""
    be, k, n = params.backend, params.k, params.n
    assert len(fixed_columns) == cs.num_fixed_columns
    dom = EvaluationDomain(cs.degree(), k, backend=be)
    ek = dom.extended_k
    bf = cs.blinding_factors()
    assert n > bf + 1 + 1, "circuit does not fit: not enough usable rows"

    fixed_values = [be.to_device(_as_mont(c, n)) for c in fixed_columns]
    # permutation columns: identity columns DELTA^j * omega^i = evaluations of DELTA^j * X (one NTT each), then the gather
    m = len(cs.permutation_columns)
    sigma_values = []
    if m:
        asm = assembly or Assembly(cs, k)
        ident = np.zeros((m, n, 4), dtype=np.uint64)
        bufs = []
        for j in range(m):
            col = np.zeros((n, 4), dtype=np.uint64)
            col[1] = fr_mont(pow(DELTA, j, R_MOD))
            d = be.to_device(col)
            be.coeff_to_lagrange_dev(d, k)
            bufs.append(d)
        for j, d in enumerate(bufs):
            ident[j] = d.download((n, 4))
            d.free()
        sig = asm.sigma_from_identity(ident)
        sigma_values = [be.to_device(np.ascontiguousarray(sig[j])) for j in range(m)]

    # commitments (keygen_vk): commit_lagrange of every fixed and sigma column — one batched MSM each
    fc = params.commit_columns("g_lagrange", fixed_values)
    pc = params.commit_columns("g_lagrange", sigma_values)
    fixed_commitments = [g1_affine_ints(r) for r in fc]
    permutation_commitments = [g1_affine_ints(r) for r in pc]
    vk = VerifyingKey(k, cs, fixed_commitments, permutation_commitments, _transcript_repr(k, cs, fixed_commitments, permutation_commitments))

    # keygen_pk: polys and extended cosets (when the quotient is sharded: only this rank's cosets, 2^k values each)
    by_cosets = params.by_cosets()
    my_cosets = params.my_cosets(1 << (ek - k)) if by_cosets else []
    n_pieces = cs.degree() - 1
    if piece_cosets is None:
        piece_cosets = True
    pieces_from_cosets = bool(piece_cosets) and not by_cosets and n_pieces < (1 << (ek - k)) and n_pieces <= 8
    if pieces_from_cosets:                                               # h(X) needs its numerator on cs_degree - 1 cosets only: keep those, build no extended form
        by_cosets, my_cosets = True, list(range(n_pieces))
    coset_parts = {j: {} for j in my_cosets} if by_cosets else None

    def to_poly_and_coset(values, name=None):
        polys = []
        for v in values:
            p = be.alloc(n * 32)
            be.fr_scale_dev(v, fr_mont(1), p, n)                         # device copy
            polys.append(p)
        if polys:
            be.lagrange_to_coeff_batch_dev(polys, k)
        if by_cosets:
            for j in my_cosets:
                outs = [be.alloc(n * 32) for _ in polys]
                if polys:
                    be.coeff_to_coset_batch_dev(polys, outs, k, ek, j)
                coset_parts[j][name] = outs
            return polys, []
        cosets = [be.alloc((1 << ek) * 32) for _ in polys]
        if polys:
            be.coeff_to_extended_batch_dev(polys, cosets, k, ek)
        return polys, cosets
    fixed_polys, fixed_cosets = to_poly_and_coset(fixed_values, "fixed")
    sigma_polys, sigma_cosets = to_poly_and_coset(sigma_values, "sigma")
    one = fr_mont(1)
    l0 = np.zeros((n, 4), dtype=np.uint64)
    l0[0] = one
    l_last = np.zeros((n, 4), dtype=np.uint64)
    l_last[n - bf - 1] = one
    l_act = np.zeros((n, 4), dtype=np.uint64)
    l_act[: n - bf - 1] = one                                            # 1 - (l_last + l_blind)
    lvals = [be.to_device(a) for a in (l0, l_last, l_act)]
    lpolys, lcosets = to_poly_and_coset(lvals, "l")
    for d in lvals + lpolys:
        d.free()
    if by_cosets:
        lcosets = [None, None, None]

    assert ek == _extended_k(cs, k)
    program, input_programs, table_programs = _programs(cs, k, ek)
    evaluator = ev.Evaluator(program, backend=be)
    comps = [(ev.Evaluator(a, backend=be), ev.Evaluator(b, backend=be)) for a, b in zip(input_programs, table_programs)]
    return ProvingKey(vk, dom, be, fixed_values, fixed_polys, fixed_cosets, sigma_values, sigma_polys, sigma_cosets,
                      lcosets[0], lcosets[1], lcosets[2], evaluator, program, comps, coset_parts, False, pieces_from_cosets=pieces_from_cosets)
