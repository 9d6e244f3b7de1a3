// What the proving-key object (pk.hip) and the proof (prover.hip) share, and nothing else: the way both report an error, the phase lists of a phased key, and the rule that gives every rank of a
// sharded key its quotient units — the key keeps the cosets those units live on, the proof evaluates the quotient on them, so the two must agree on it.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <vector>
#include "../../include/zkmi355.h"

int zk_internal_fail(zk_ctx* ctx, int code, const char* msg);   // capi.hip: sets zk_last_error(ctx)

namespace zk {
inline int pk_fail(zk_ctx* ctx, int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return zk_internal_fail(ctx, code, buf);
}

// Advice phases and user challenges of one proof ([3P-MEM] halo2_proofs v2023_01_20 plonk/circuit.rs: advice_column_phase, challenge_phase): the key's lists (pk.hip
// validates and keeps them) and the caller's callback and pointer array (zk_plonk_prove_phased), handed to the proof (prover.hip)
struct PhaseSpec {
    const uint8_t* advice_phase = nullptr;                             // n_advice entries
    const uint8_t* challenge_phase = nullptr; uint32_t n_challenges = 0;
    zk_phase_fn next_phase = nullptr; void* next_phase_user = nullptr;
    const void** advice_out = nullptr;                                 // the caller's n_circuits x n_advice array: read by the proof, written by the callback
};
int create_proof_phased(zk_ctx* ctx, const zk_plonk_pk_desc* pk, const PhaseSpec* ph, uint32_t n_circuits, int advice_on_device, const void* const* instances,
                        const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len);   // prover.hip

// the quotient's units of one rank (see zk_plonk_pk_desc): (coset, first row, rows).  A single GPU (world = 1) has none: parts = 1, unit_rows = n, slots = 0
struct QuotUnits {
    struct Unit { uint32_t coset; uint64_t lo, rows; };
    std::vector<Unit> units;
    std::vector<uint32_t> my_cosets;                                   // the cosets of `units`, ascending, each once: the order of a sharded key's coset_* arrays
    uint32_t n_cosets = 1, parts = 1; size_t slots = 0, unit_rows = 0;
};
inline QuotUnits quotient_units(uint32_t world, uint32_t rank, uint32_t k, uint32_t ek) {
    QuotUnits q;
    const size_t n = (size_t)1 << k;
    q.n_cosets = 1u << (ek - k);
    q.unit_rows = n;
    if (world <= 1) return q;
    if (world > q.n_cosets && world % q.n_cosets == 0) { const uint32_t p = world / q.n_cosets; if ((p & (p - 1)) == 0 && n % p == 0) q.parts = p; }
    const size_t n_units = (size_t)q.n_cosets * q.parts;
    q.unit_rows = n / q.parts;
    q.slots = (n_units + world - 1) / world;
    for (size_t u = (size_t)rank * q.slots; u < (size_t)(rank + 1) * q.slots && u < n_units; u++) {
        q.units.push_back({(uint32_t)(u / q.parts), (u % q.parts) * q.unit_rows, q.unit_rows});
        if (q.my_cosets.empty() || q.my_cosets.back() != q.units.back().coset) q.my_cosets.push_back(q.units.back().coset);
    }
    return q;
}
}  // namespace zk
