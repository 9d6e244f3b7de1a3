"""halo2_proofs::plonk — the prover side the reference calls (keygen_vk / keygen_pk / create_proof at
circuits/src/sgx_dcap_verifier.rs:803,807,814-822), as a host-side mirror over the MI355X product API.

    ConstraintSystem, Assembly, Expression (Advice / Fixed / Instance / Constant …)      circuit description
    keygen(params, cs, fixed_columns, assembly) -> ProvingKey                            keygen_vk + keygen_pk
    keygen_vk_native(params, cs, fixed_columns, assembly) -> (VerifyingKey, NativeKeygen) keygen_vk in the library: sigma from the copy mapping on the GPU (zk_plonk_keygen_vk)
    NativeKey.from_keygen(params, kg, vk)                                                keygen_pk on those resident columns (zk_plonk_keygen_pk)
    create_proof(params, pk, advice_columns, instances, rng, transcript)                 plonk::create_proof + ProverSHPLONK (Python twin; multi-GPU driver)
    NativeProver(params, pk).create_proof(advice_columns, instances, rng) -> bytes       the same per-proof path in C++ (zk_plonk_create_proof)
    PhasedProver(params, pk).create_proof(advices, instances, rng, next_phase) -> bytes  advice in phases with halo2's Challenge API (zk_plonk_prove_phased)
    MockProver.run(k, cs, fixed, advice, instances, assembly).assert_satisfied()         dev::MockProver (host-only constraint check)
    NativeMockProver.run(k, cs, fixed, advice, instances, assembly).assert_satisfied()   the same check on the GPU (zk_mock_prover_verify)
    NativeMockSession(k, cs, fixed, assembly).assert_satisfied(advice, instances)          one circuit resident, many witnesses (zk_mock_prover_open / _check)

verify_proof is not part of the product (verifier side, out of scope); the tests carry their own
pure-Python verifier as the acceptance check, outside this package.
"""
from .circuit import ADVICE, FIXED, INSTANCE, Assembly, ConstraintSystem, LookupArgument  # noqa: F401
from .dev import MockProver, NativeMockProver, NativeMockSession, VerifyFailure  # noqa: F401
from .expression import Advice, Challenge, Constant, Expression, Fixed, Instance  # noqa: F401
from .keygen import KeyView, NativeKey, NativeKeygen, ProvingKey, VerifyingKey, compile_program, keygen, keygen_vk_native  # noqa: F401
from .prover import create_proof  # noqa: F401
from .native import NativeProver, PhasedProver, create_proof_native, last_challenges  # noqa: F401
from .shplonk import ProverSHPLONK  # noqa: F401
from .gwc import ProverGWC  # noqa: F401
