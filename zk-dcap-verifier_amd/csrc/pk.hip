// ---- the proving key as a library object (zk_plonk_pk_build / share / release / prove) -------------------------------------------------------------------------
// The device half of keygen_pk, written — like create_proof (prover.hip) — as a CLIENT of the public entry points: upload the Lagrange columns, lagrange_to_coeff,
// coeff_to_extended, l0 / l_last / l_active_row, load the ZKQ1 programs.  One PkMem per key per process (columns + the host arrays the descriptor points into);
// every holding context has a PkHandle with its own program handles (zk_quotient_program_share) and SRS handles.
//
// Keygen (zk_plonk_keygen_vk / _pk, at the end of this file) is the one part that is NOT a client: its two kernels — mapping_check and sigma_from_mapping — are
// launched here on the context's stream, under the context's lock, like every other kernel of the library.
#include <string.h>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "ctx.h"
#include "bn254_consts.h"
#include "plonk_shared.h"

using namespace zk;
namespace zk { u256 domain_omega(uint32_t k); }                       // ntt.hip

#define PK(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

namespace {
struct KgCols {                                                       // the Lagrange columns of a keygen handle (zk_plonk_keygen_vk): shared by the handle and every key built
    int device = 0;                                                   // from it (zk_plonk_keygen_pk), freed with the last of them, whichever that is
    std::vector<void*> owned;
    ~KgCols() {
        if (owned.empty()) return;
        (void)hipSetDevice(device);
        for (void* p : owned) (void)hipFree(p);
    }
};
struct PkMem {
    std::shared_ptr<KgCols> keygen_cols;                              // a key of zk_plonk_keygen_pk: its fixed / sigma values are these (not in `owned`)
    std::vector<void*> owned;                                         // device allocations, freed by whoever drops the last handle
    std::vector<const void*> fixed_values, fixed_polys, fixed_cosets, sigma_values, sigma_polys, sigma_cosets;
    void* l[3] = {nullptr, nullptr, nullptr};
    std::vector<const void*> coset_fixed, coset_sigma, coset_l;      // a sharded key: [this rank's cosets][columns], n values each
    std::vector<uint32_t> perm_columns, advice_queries, fixed_queries, table_key;
    uint8_t transcript_repr[32];
    bool phased = false;                                              // built by zk_plonk_pk_build_phased: the two lists below are the circuit's
    std::vector<uint8_t> advice_phase, challenge_phase;               // ([3P-MEM] plonk/circuit.rs advice_column_phase, challenge_phase)
    int holders = 0;
};
struct PkHandle {
    PkMem* mem = nullptr;
    zk_plonk_pk_desc desc;
    uint64_t program = 0;
    std::vector<uint64_t> in_prog, tab_prog;
    int in_use = 0;              // zk_plonk_prove calls running on this handle (g_pk_mu)
    bool released = false;       // zk_plonk_pk_release / zk_ctx_destroy arrived meanwhile: the last of those calls drops the handle
};
std::mutex g_pk_mu;
std::map<std::pair<zk_ctx*, uint64_t>, PkHandle*> g_pk_handles;
uint64_t g_pk_next = 1;

void pk_fill_desc(PkHandle* h, const zk_plonk_pk_desc& shape, uint64_t srs_g, uint64_t srs_g_lagrange) {
    PkMem* m = h->mem;
    zk_plonk_pk_desc& d = h->desc;
    d = shape;
    d.perm_columns = m->perm_columns.data(); d.advice_queries = m->advice_queries.data(); d.fixed_queries = m->fixed_queries.data();
    d.srs_g = srs_g; d.srs_g_lagrange = srs_g_lagrange; d.program = h->program;
    d.lookup_input_programs = h->in_prog.data(); d.lookup_table_programs = h->tab_prog.data(); d.lookup_table_key = m->table_key.data();
    d.fixed_values = m->fixed_values.data(); d.fixed_polys = m->fixed_polys.data(); d.fixed_cosets = m->fixed_cosets.data();
    d.sigma_values = m->sigma_values.data(); d.sigma_polys = m->sigma_polys.data(); d.sigma_cosets = m->sigma_cosets.data();
    d.l0 = m->l[0]; d.l_last = m->l[1]; d.l_active_row = m->l[2];
    d.coset_fixed = m->coset_fixed.data(); d.coset_sigma = m->coset_sigma.data(); d.coset_l = m->coset_l.data();
    d.transcript_repr = m->transcript_repr;
}
void pk_drop(zk_ctx* ctx, PkHandle* h) {                              // g_pk_mu held
    if (h->program) (void)zk_quotient_program_release(ctx, h->program);
    for (uint64_t p : h->in_prog) if (p) (void)zk_quotient_program_release(ctx, p);
    for (uint64_t p : h->tab_prog) if (p) (void)zk_quotient_program_release(ctx, p);
    if (h->mem && --h->mem->holders == 0) {
        for (void* p : h->mem->owned) (void)zk_dev_free(ctx, p);
        delete h->mem;
    }
    delete h;
}
}  // namespace

// The phase lists of a phased key against halo2's rules and against the blobs the key is built from (word 6 of a ZKQ1 header: n_challenges; word 4: n_advice)
static int check_phases(zk_ctx* ctx, const zk_plonk_pk_host* host, const zk_plonk_phases* ph) {
    if (ph->struct_size != sizeof(zk_plonk_phases))
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: zk_plonk_phases.struct_size %u, expected %zu (ABI version %u)", ph->struct_size, sizeof(zk_plonk_phases), ZK_ABI_VERSION);
    if (host->shard_world > 1) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: shard_world %u: one proof over several GPUs is single-phase", host->shard_world);
    if (ph->n_challenges > ZK_MAX_CHALLENGES)
        return pk_fail(ctx, ZK_ERR_LIMIT, "zk_plonk_pk_build_phased: %u challenges, the quotient interpreter's constant bank is sized for %u", ph->n_challenges, ZK_MAX_CHALLENGES);
    if (ph->n_advice != host->n_advice) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: phases for %u advice columns, the key has %u", ph->n_advice, host->n_advice);
    if ((ph->n_advice && !ph->advice_phase) || (ph->n_challenges && !ph->challenge_phase)) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: null phase list");
    uint32_t count[3] = {0, 0, 0};
    for (uint32_t i = 0; i < ph->n_advice; i++) {
        if (ph->advice_phase[i] > 2) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: advice column %u in phase %u (0 .. 2)", i, ph->advice_phase[i]);
        count[ph->advice_phase[i]]++;
    }
    for (uint32_t p = 1; p < 3; p++)
        if (count[p] && !count[p - 1]) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: an advice column in phase %u and none in phase %u", p, p - 1);
    const uint32_t last = count[2] ? 2 : count[1] ? 1 : 0;
    for (uint32_t i = 0; i < ph->n_challenges; i++)
        if (ph->challenge_phase[i] > last) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: challenge %u after phase %u, the last phase in use is %u", i, ph->challenge_phase[i], last);
    auto header = [&](const void* blob, size_t len, const char* what, uint32_t i) -> int {
        uint32_t w[7];
        if (!blob || len < sizeof w) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: bad %s blob %u", what, i);
        memcpy(w, blob, sizeof w);
        if (w[4] != ph->n_advice || w[6] != ph->n_challenges)
            return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build_phased: %s blob %u declares %u advice columns and %u challenges, the phase lists %u and %u", what, i, w[4], w[6], ph->n_advice, ph->n_challenges);
        return ZK_OK;
    };
    PK(header(host->evaluator_zkq1, host->evaluator_zkq1_len, "evaluator", 0));
    for (uint32_t l = 0; l < host->n_lookups; l++) {
        PK(header(host->lookup_input_zkq1[l], host->lookup_input_zkq1_len[l], "lookup input", l));
        PK(header(host->lookup_table_zkq1[l], host->lookup_table_zkq1_len[l], "lookup table", l));
    }
    return ZK_OK;
}

static int pk_build(zk_ctx* ctx, const zk_plonk_pk_host* host, const zk_plonk_phases* phases, uint64_t srs_g, uint64_t srs_g_lagrange, uint64_t* pk,
                    const std::shared_ptr<KgCols>& keygen_cols = nullptr) {
    if (!ctx || !host || !pk) return ZK_ERR_ARG;
    if (host->struct_size != sizeof(zk_plonk_pk_host))
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_pk_build: zk_plonk_pk_host.struct_size %u, expected %zu (ABI version %u)", host->struct_size, sizeof(zk_plonk_pk_host), ZK_ABI_VERSION);
    const uint32_t k = host->k, L = host->n_lookups;
    if (k < 1 || k > 27 || host->cs_degree < 3 || host->transcript > 2 || host->draw_schedule != 1 || !host->transcript_repr || !host->evaluator_zkq1) return ZK_ERR_ARG;
    if ((host->n_fixed && !host->fixed_values) || (host->n_perm_columns && (!host->sigma_values || !host->perm_columns)) || (host->n_advice_queries && !host->advice_queries) ||
        (host->n_fixed_queries && !host->fixed_queries) ||
        (L && (!host->lookup_input_zkq1 || !host->lookup_input_zkq1_len || !host->lookup_table_zkq1 || !host->lookup_table_zkq1_len || !host->lookup_table_key)))
        return ZK_ERR_ARG;
    if (phases) PK(check_phases(ctx, host, phases));
    const size_t n = (size_t)1 << k, col_bytes = n * 32;
    if ((size_t)host->blinding_factors + 2 >= n) return ZK_ERR_ARG;
    uint32_t ek = k;                                                  // EvaluationDomain::new(j, k): the smallest extended domain that holds a quotient of degree (j - 1) n
    while (((size_t)1 << ek) < n * (host->cs_degree - 1)) ek++;
    if (ek > 27) return ZK_ERR_LIMIT;
    const size_t ext_bytes = (size_t)32 << ek;
    PkHandle* h = new PkHandle();
    struct Undo { zk_ctx* ctx; PkHandle* h; ~Undo() { if (h) { std::lock_guard<std::mutex> lk(g_pk_mu); pk_drop(ctx, h); } } } undo{ctx, h};      // every way out but the last line drops the half-built key
    h->mem = new PkMem();
    h->mem->holders = 1;
    PkMem* m = h->mem;
    m->keygen_cols = keygen_cols;
    auto alloc = [&](size_t bytes) -> void* {
        m->owned.reserve(m->owned.size() + 1);                         // (the slot first: a buffer is never allocated without an owner to free it)
        void* p = nullptr;
        if (zk_dev_alloc(ctx, bytes, &p) != ZK_OK) return nullptr;
        m->owned.push_back(p);
        return p;
    };
    // values -> (values, polys, cosets); `src` are host columns, or device columns that are borrowed as they are
    // a sharded key keeps only the cosets this rank's quotient units live on (the unit rule of zk_plonk_pk_desc), n values per column
    const uint32_t world = host->shard_world > 1 ? host->shard_world : 1;
    if (world > 1 && (host->shard_rank >= world || n % world || !host->allgather)) return ZK_ERR_ARG;
    std::vector<uint32_t> my_cosets = quotient_units(world, host->shard_rank, k, ek).my_cosets;
    // a single GPU needs h(X)'s numerator on cs_degree - 1 cosets only (zk_cosets_to_pieces_dev): when that is fewer than the 2^(ek - k) of the extended domain the key
    // keeps cosets 0 .. cs_degree-2, n values per column, and no extended form at all (tunable "quot_piece_cosets", default on)
    bool whole_domain = world == 1;
    if (world == 1 && host->cs_degree - 1 < (1u << (ek - k)) && host->cs_degree - 1 <= 8) {
        int on = 1;
        (void)zk_tune_get(ctx, "quot_piece_cosets", &on);
        if (on) { whole_domain = false; for (uint32_t j = 0; j + 1 < host->cs_degree; j++) my_cosets.push_back(j); }
    }
    // coeffs -> extended cosets (`cosets`) or the cosets this key keeps (`by_coset`, [coset][column])
    auto to_cosets = [&](std::vector<void*>& pl, std::vector<const void*>& cosets, std::vector<const void*>& by_coset) -> int {
        const size_t count = pl.size();
        if (whole_domain) {
            std::vector<void*> cs(count);
            for (auto& c : cs) { c = alloc(ext_bytes); if (!c) return ZK_ERR_HIP; }
            if (count) PK(zk_coeff_to_extended_batch_dev(ctx, (const void* const*)pl.data(), cs.data(), count, k, ek));
            cosets.assign(cs.begin(), cs.end());
            return ZK_OK;
        }
        for (uint32_t j : my_cosets) {
            std::vector<void*> cs(count);
            for (auto& c : cs) { c = alloc(col_bytes); if (!c) return ZK_ERR_HIP; }
            if (count) PK(zk_coeff_to_coset_batch_dev(ctx, (const void* const*)pl.data(), cs.data(), count, k, ek, j));
            by_coset.insert(by_coset.end(), cs.begin(), cs.end());
        }
        return ZK_OK;
    };
    auto three_forms = [&](const void* const* src, size_t count, bool on_device, std::vector<const void*>& values, std::vector<const void*>& polys, std::vector<const void*>& cosets,
                           std::vector<const void*>& by_coset) -> int {
        std::vector<void*> dst, pl;
        std::vector<const void*> hs;
        for (size_t i = 0; i < count; i++) {
            if (!src[i]) return ZK_ERR_ARG;
            if (on_device) values.push_back(src[i]);
            else { void* v = alloc(col_bytes); if (!v) return ZK_ERR_HIP; values.push_back(v); dst.push_back(v); hs.push_back(src[i]); }
            void* p = alloc(col_bytes);
            if (!p) return ZK_ERR_HIP;
            pl.push_back(p);
        }
        if (!dst.empty()) PK(zk_dev_upload_batch(ctx, dst.data(), hs.data(), dst.size(), col_bytes));
        for (size_t i = 0; i < count; i++) PK(zk_dev_copy(ctx, pl[i], values[i], col_bytes));
        if (count) PK(zk_lagrange_to_coeff_batch_dev(ctx, pl.data(), count, k));
        polys.assign(pl.begin(), pl.end());
        return to_cosets(pl, cosets, by_coset);
    };
    int rc = three_forms(host->fixed_values, host->n_fixed, host->values_on_device != 0, m->fixed_values, m->fixed_polys, m->fixed_cosets, m->coset_fixed);
    if (!rc) rc = three_forms(host->sigma_values, host->n_perm_columns, host->values_on_device != 0, m->sigma_values, m->sigma_polys, m->sigma_cosets, m->coset_sigma);
    if (rc) return rc;
    {   // l0 = [row 0], l_last = [row n - bf - 1], l_active_row = [rows below it]: Lagrange columns -> extended cosets (keygen.rs)
        const size_t last = n - host->blinding_factors - 1;
        std::vector<uint64_t> col(3 * n * 4, 0);
        const u256 one = Fr::one();
        memcpy(&col[0], one.v, 32);
        memcpy(&col[(n + last) * 4], one.v, 32);
        for (size_t i = 0; i < last; i++) memcpy(&col[(2 * n + i) * 4], one.v, 32);
        struct Tmp { zk_ctx* ctx; std::vector<void*> v; ~Tmp() { for (void* p : v) if (p) (void)zk_dev_free(ctx, p); } } t{ctx, std::vector<void*>(3, nullptr)};
        std::vector<void*>& tmp = t.v;
        const void* hs[3];
        for (int i = 0; i < 3; i++) {
            if (zk_dev_alloc(ctx, col_bytes, &tmp[i]) != ZK_OK) return ZK_ERR_HIP;
            hs[i] = &col[(size_t)i * n * 4];
        }
        rc = zk_dev_upload_batch(ctx, tmp.data(), hs, 3, col_bytes);
        if (!rc) rc = zk_lagrange_to_coeff_batch_dev(ctx, tmp.data(), 3, k);
        std::vector<const void*> ext;
        if (!rc) rc = to_cosets(tmp, ext, m->coset_l);
        if (rc) return rc;
        for (int i = 0; i < 3 && whole_domain; i++) m->l[i] = (void*)ext[i];
    }
    rc = zk_quotient_program_load(ctx, host->evaluator_zkq1, host->evaluator_zkq1_len, &h->program);
    h->in_prog.assign(L, 0); h->tab_prog.assign(L, 0);
    for (uint32_t l = 0; l < L && !rc; l++) {
        rc = zk_quotient_program_load(ctx, host->lookup_input_zkq1[l], host->lookup_input_zkq1_len[l], &h->in_prog[l]);
        if (!rc) rc = zk_quotient_program_load(ctx, host->lookup_table_zkq1[l], host->lookup_table_zkq1_len[l], &h->tab_prog[l]);
    }
    if (rc) return rc;
    m->perm_columns.assign(host->perm_columns, host->perm_columns + 2 * (size_t)host->n_perm_columns);
    m->advice_queries.assign(host->advice_queries, host->advice_queries + 2 * (size_t)host->n_advice_queries);
    m->fixed_queries.assign(host->fixed_queries, host->fixed_queries + 2 * (size_t)host->n_fixed_queries);
    m->table_key.assign(host->lookup_table_key, host->lookup_table_key + L);
    m->perm_columns.push_back(0); m->advice_queries.push_back(0); m->fixed_queries.push_back(0); m->table_key.push_back(0);      // .data() of an empty vector may be null: the prover refuses null arrays
    h->in_prog.push_back(0); h->tab_prog.push_back(0);
    for (auto* v : {&m->fixed_values, &m->fixed_polys, &m->fixed_cosets, &m->sigma_values, &m->sigma_polys, &m->sigma_cosets, &m->coset_fixed, &m->coset_sigma, &m->coset_l}) v->push_back(nullptr);
    memcpy(m->transcript_repr, host->transcript_repr, 32);
    if (phases) {
        m->phased = true;
        m->advice_phase.assign(phases->advice_phase, phases->advice_phase + phases->n_advice);
        m->challenge_phase.assign(phases->challenge_phase, phases->challenge_phase + phases->n_challenges);
    }
    zk_plonk_pk_desc shape;
    ZK_STRUCT_INIT(shape);
    shape.k = k; shape.extended_k = ek; shape.cs_degree = host->cs_degree; shape.blinding_factors = host->blinding_factors;
    shape.n_fixed = host->n_fixed; shape.n_advice = host->n_advice; shape.n_instance = host->n_instance; shape.n_lookups = L; shape.n_perm_columns = host->n_perm_columns;
    shape.n_advice_queries = host->n_advice_queries; shape.n_fixed_queries = host->n_fixed_queries;
    shape.transcript = host->transcript; shape.draw_schedule = host->draw_schedule;
    shape.shard_world = host->shard_world; shape.shard_rank = host->shard_rank; shape.allgather = host->allgather; shape.allgather_user = host->allgather_user;
    pk_fill_desc(h, shape, srs_g, srs_g_lagrange);
    {
        std::lock_guard<std::mutex> lk(g_pk_mu);
        g_pk_handles[{ctx, g_pk_next}] = h;
        *pk = g_pk_next++;
    }
    undo.h = nullptr;
    return ZK_OK;
}

extern "C" int zk_plonk_pk_build(zk_ctx* ctx, const zk_plonk_pk_host* host, uint64_t srs_g, uint64_t srs_g_lagrange, uint64_t* pk) ZK_ABI_TRY {
    return pk_build(ctx, host, nullptr, srs_g, srs_g_lagrange, pk);
} ZK_ABI_CATCH(ctx)

// zk_plonk_pk_build for a circuit with advice in several phases and user challenges: the same key, and the two lists kept with it
extern "C" int zk_plonk_pk_build_phased(zk_ctx* ctx, const zk_plonk_pk_host* host, const zk_plonk_phases* phases, uint64_t srs_g, uint64_t srs_g_lagrange, uint64_t* pk) ZK_ABI_TRY {
    if (!ctx || !host || !phases || !pk) return ZK_ERR_ARG;
    return pk_build(ctx, host, phases, srs_g, srs_g_lagrange, pk);
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_pk_share(zk_ctx* ctx, zk_ctx* owner, uint64_t owner_pk, uint64_t srs_g, uint64_t srs_g_lagrange, uint64_t* pk) ZK_ABI_TRY {
    if (!ctx || !owner || !pk) return ZK_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_pk_mu);
    auto it = g_pk_handles.find({owner, owner_pk});
    if (it == g_pk_handles.end()) return ZK_ERR_ARG;
    const PkHandle* src = it->second;
    PkHandle* h = new PkHandle();
    struct Undo { zk_ctx* ctx; PkHandle* h; ~Undo() { if (h) pk_drop(ctx, h); } } undo{ctx, h};      // (g_pk_mu is held for the whole function)
    h->mem = src->mem;
    h->mem->holders++;
    const size_t L = src->desc.n_lookups;
    h->in_prog.assign(L + 1, 0); h->tab_prog.assign(L + 1, 0);
    int rc = zk_quotient_program_share(ctx, owner, src->program, &h->program);                  // (refuses contexts on different devices)
    for (size_t l = 0; l < L && !rc; l++) {
        rc = zk_quotient_program_share(ctx, owner, src->in_prog[l], &h->in_prog[l]);
        if (!rc) rc = zk_quotient_program_share(ctx, owner, src->tab_prog[l], &h->tab_prog[l]);
    }
    if (rc) return rc;
    pk_fill_desc(h, src->desc, srs_g, srs_g_lagrange);
    g_pk_handles[{ctx, g_pk_next}] = h;
    *pk = g_pk_next++;
    undo.h = nullptr;
    return ZK_OK;
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_pk_release(zk_ctx* ctx, uint64_t pk) ZK_ABI_TRY {
    if (!ctx) return ZK_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_pk_mu);
    auto it = g_pk_handles.find({ctx, pk});
    if (it == g_pk_handles.end()) return ZK_ERR_ARG;
    if (it->second->in_use) it->second->released = true;             // a proof is running through this handle on another thread: it drops the handle when it returns
    else pk_drop(ctx, it->second);
    g_pk_handles.erase(it);
    return ZK_OK;
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_pk_descriptor(zk_ctx* ctx, uint64_t pk, const zk_plonk_pk_desc** desc) ZK_ABI_TRY {
    if (!ctx || !desc) return ZK_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_pk_mu);
    auto it = g_pk_handles.find({ctx, pk});
    if (it == g_pk_handles.end()) return ZK_ERR_ARG;
    *desc = &it->second->desc;
    return ZK_OK;
} ZK_ABI_CATCH(ctx)

// zk_plonk_prove / zk_plonk_prove_multi: the handle (descriptor, programs, its share of the columns) stays alive for the whole proof whatever other threads release meanwhile
static int prove_with_key(const char* fn, zk_ctx* ctx, uint64_t pk, uint32_t n_circuits, const void* const* advice, int advice_on_device, const void* const* instances,
                          const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len,
                          bool phased = false, const void** advice_out = nullptr, zk_phase_fn next_phase = nullptr, void* next_phase_user = nullptr) {
    if (!ctx) return ZK_ERR_ARG;
    PkHandle* h = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pk_mu);
        auto it = g_pk_handles.find({ctx, pk});
        if (it == g_pk_handles.end()) return pk_fail(ctx, ZK_ERR_ARG, "%s: unknown key %llu", fn, (unsigned long long)pk);
        h = it->second;
        h->in_use++;
    }
    struct Done { zk_ctx* ctx; PkHandle* h; ~Done() { std::lock_guard<std::mutex> lk(g_pk_mu); if (--h->in_use == 0 && h->released) pk_drop(ctx, h); } } done{ctx, h};
    if (phased && h->mem->phased) {                                   // (a key of zk_plonk_pk_build has no later phase and no challenge: zk_plonk_prove_multi, byte for byte)
        PhaseSpec ph;
        ph.advice_phase = h->mem->advice_phase.data(); ph.challenge_phase = h->mem->challenge_phase.data(); ph.n_challenges = (uint32_t)h->mem->challenge_phase.size();
        ph.next_phase = next_phase; ph.next_phase_user = next_phase_user; ph.advice_out = advice_out;
        return create_proof_phased(ctx, &h->desc, &ph, n_circuits, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len);
    }
    return zk_plonk_create_proof_multi(ctx, &h->desc, n_circuits, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len);
}
extern "C" int zk_plonk_prove(zk_ctx* ctx, uint64_t pk, const void* const* advice, int advice_on_device, const void* const* instances, const uint32_t* instance_lens,
                              zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len) ZK_ABI_TRY {
    return prove_with_key("zk_plonk_prove", ctx, pk, 1, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len);
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_prove_multi(zk_ctx* ctx, uint64_t pk, uint32_t n_circuits, const void* const* advice, int advice_on_device, const void* const* instances,
                                    const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len) ZK_ABI_TRY {
    return prove_with_key("zk_plonk_prove_multi", ctx, pk, n_circuits, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len);
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_prove_phased(zk_ctx* ctx, uint64_t pk, uint32_t n_circuits, const void** advice, int advice_on_device, const void* const* instances,
                                     const uint32_t* instance_lens, zk_phase_fn next_phase, void* next_phase_user, zk_rng_fn rng, void* rng_user,
                                     void* proof_out, size_t proof_cap, size_t* proof_len) ZK_ABI_TRY {
    return prove_with_key("zk_plonk_prove_phased", ctx, pk, n_circuits, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len,
                          true, advice, next_phase, next_phase_user);
} ZK_ABI_CATCH(ctx)

// ---- keygen: keygen_vk + keygen_pk after synthesis (include/zkmi355.h, zk_plonk_keygen_vk) ---------------------------------------------------------------------
// halo2's permutation::keygen::Assembly::build_vk / build_pk: sigma_j[i] = DELTA^c * omega^r for (c, r) = mapping[j][i].  A table of all omega^r would be n x 32 B per
// key and every cell a random 32-byte read of it; the row exponent is split instead, omega^r = HI[r >> s] * LO[r & (2^s - 1)] with s = ceil(k / 2), and DELTA^c comes
// from a third table of n_perm_columns entries: 2^s + 2^(k-s) + m elements (48 KiB + 32 m bytes at k = 19) that every workgroup re-reads, two products per cell.
// The tables are built on the host with the same Field routines and uploaded once per call.  (chosen by construction, not measured against the gather.)
namespace {
constexpr uint32_t KG_T = 256;

// Every entry in range, every cell the image of exactly one cell.  status[0]: 0, or 2^32 - 1 - e for the FIRST cell e = j * 2^k + i whose entry is out of range (such an
// entry is not used); status[1]: the cells whose image another cell had marked already.  seen: one bit per cell, zeroed by the caller.  (m << k < 2^32: the caller.)
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mapping_check_kernel(const uint32_t* map_c, const uint32_t* map_r, uint32_t m, uint32_t k, uint32_t* seen, uint32_t* status) {
    const uint64_t cells = (uint64_t)m << k, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += stride) {
        const uint32_t c = map_c[e], r = map_r[e];
        if (c >= m || r >= (1u << k)) { atomicMax(&status[0], 0xffffffffu - (uint32_t)e); continue; }
        const uint32_t t = (c << k) | r, bit = 1u << (t & 31u);
        if (atomicOr(&seen[t >> 5], bit) & bit) atomicAdd(&status[1], 1u);
    }
}
// sigma[e >> k][e & (2^k - 1)] = dpow[map_c[e]] * hi[map_r[e] >> s] * lo[map_r[e] & (2^s - 1)] over a mapping mapping_check_kernel has passed
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) sigma_from_mapping_kernel(const uint32_t* map_c, const uint32_t* map_r, uint32_t m, uint32_t k, uint32_t s, const void* lo, const void* hi,
                                                               const void* dpow, void* const* sigma) {
    const uint64_t cells = (uint64_t)m << k, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lo_mask = (1u << s) - 1u, row_mask = (1u << k) - 1u;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += stride) {
        const uint32_t c = map_c[e], r = map_r[e];
        const u256 w = Fr::mul(load_u256(hi, r >> s), load_u256(lo, r & lo_mask));
        store_u256(sigma[e >> k], (uint32_t)e & row_mask, Fr::mul(w, load_u256(dpow, c)));
    }
}

// mapping planes (HOST) -> the m sigma columns (`sigma`: HOST array of DEVICE columns, 2^k x 32 B each); the mapping is checked first and nothing is written for a bad one
int keygen_sigma(zk_ctx* ctx, const uint32_t* map_c, const uint32_t* map_r, uint32_t m, uint32_t k, void* const* sigma) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ZK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t cells = (size_t)m << k;
    const uint32_t s = (k + 1) / 2, n_lo = 1u << s, n_hi = 1u << (k - s);
    std::vector<u256> tab((size_t)n_lo + n_hi + m);
    {
        const uint64_t dl[4] = BN254_FR_DELTA_M;
        u256 delta, w = domain_omega(k), ws = w;
        memcpy(delta.v, dl, 32);
        for (uint32_t i = 0; i < s; i++) ws = Fr::sqr(ws);             // omega^(2^s)
        u256 acc = Fr::one();
        for (uint32_t i = 0; i < n_lo; i++) { tab[i] = acc; acc = Fr::mul(acc, w); }
        acc = Fr::one();
        for (uint32_t i = 0; i < n_hi; i++) { tab[n_lo + i] = acc; acc = Fr::mul(acc, ws); }
        acc = Fr::one();
        for (uint32_t i = 0; i < m; i++) { tab[(size_t)n_lo + n_hi + i] = acc; acc = Fr::mul(acc, delta); }
    }
    const size_t seen_bytes = (cells + 31) / 32 * 4;
    DevTmp d_mc, d_mr, d_seen, d_status, d_tab, d_out;
    ZK_HIP(hipMalloc(&d_mc.p, cells * 4));
    ZK_HIP(hipMalloc(&d_mr.p, cells * 4));
    ZK_HIP(hipMalloc(&d_seen.p, seen_bytes));
    ZK_HIP(hipMalloc(&d_status.p, 8));
    ZK_HIP(hipMalloc(&d_tab.p, tab.size() * 32));
    ZK_HIP(hipMalloc(&d_out.p, (size_t)m * sizeof(void*)));
    ZK_HIP(hipMemcpyAsync(d_mc.p, map_c, cells * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_mr.p, map_r, cells * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 32, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_out.p, sigma, (size_t)m * sizeof(void*), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemsetAsync(d_seen.p, 0, seen_bytes, st));
    ZK_HIP(hipMemsetAsync(d_status.p, 0, 8, st));
    const size_t want = (cells + KG_T - 1) / KG_T, cap = ctx->tune.keygen_wgs > 0 ? (size_t)ctx->tune.keygen_wgs : 1;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    uint32_t status[2] = {0, 0};
    {
        EvTimer t(ctx, "keygen_mapping_check");
        ZK_LAUNCH(mapping_check_kernel, grid, KG_T, 0, st, (const uint32_t*)d_mc.p, (const uint32_t*)d_mr.p, m, k, (uint32_t*)d_seen.p, (uint32_t*)d_status.p);
        ZK_CHECK_LAUNCH();
        t.stop();
        ZK_HIP(hipMemcpyAsync(status, d_status.p, 8, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        t.resolve();
    }
    if (status[0]) {
        const uint32_t e = 0xffffffffu - status[0];
        return ctx->fail(ZK_ERR_ARG, "zk_plonk_keygen_vk: the copy mapping sends cell (column %u, row %u) to (column %u, row %u), outside %u columns of 2^%u rows",
                         e >> k, e & ((1u << k) - 1u), map_c[e], map_r[e], m, k);
    }
    if (status[1])
        return ctx->fail(ZK_ERR_ARG, "zk_plonk_keygen_vk: the copy mapping is not a permutation of the cells: %u cells have an image that another cell has too", status[1]);
    EvTimer t(ctx, "keygen_sigma");
    ZK_LAUNCH(sigma_from_mapping_kernel, grid, KG_T, 0, st, (const uint32_t*)d_mc.p, (const uint32_t*)d_mr.p, m, k, s, (const void*)d_tab.p,
              (const void*)((const char*)d_tab.p + (size_t)n_lo * 32), (const void*)((const char*)d_tab.p + ((size_t)n_lo + n_hi) * 32), (void* const*)d_out.p);
    ZK_CHECK_LAUNCH();
    t.stop();
    ZK_HIP(hipStreamSynchronize(st));
    t.resolve();
    return ZK_OK;
}

// Keygen runs on one GPU with the whole table: `handle` must be a registered table of exactly 2^k points (params.g_lagrange) or, with at_least, of 2^k or more
// (params.g).  A rank's slice of a sharded SRS holds fewer and is refused.
int kg_whole_table(zk_ctx* ctx, const char* fn, const char* what, uint64_t handle, uint32_t k, bool at_least) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->bases.find(handle);
    if (it == ctx->bases.end()) return ctx->fail(ZK_ERR_ARG, "%s: %s = %llu is not a registered table", fn, what, (unsigned long long)handle);
    const size_t n = (size_t)1 << k, have = it->second.n;
    if (have < n || (!at_least && have != n))
        return ctx->fail(ZK_ERR_ARG, "%s: %s holds %zu points, keygen at k = %u needs the whole table of 2^%u (a slice of a sharded SRS is refused)", fn, what, have, k, k);
    return ZK_OK;
}

struct KgHandle {
    std::shared_ptr<KgCols> cols;
    uint32_t k = 0;
    std::vector<const void*> fixed, sigma;                            // DEVICE, Lagrange
};
std::map<std::pair<zk_ctx*, uint64_t>, KgHandle> g_kg_handles;       // (g_pk_mu; handle numbers are g_pk_next's)
}  // namespace

extern "C" int zk_plonk_keygen_vk(zk_ctx* ctx, const zk_plonk_keygen_desc* d, uint64_t srs_g_lagrange, void* fixed_commitments, void* permutation_commitments,
                                  uint64_t* kg) ZK_ABI_TRY {
    if (!ctx || !d || !kg) return ZK_ERR_ARG;
    if (d->struct_size != sizeof(zk_plonk_keygen_desc))
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_vk: zk_plonk_keygen_desc.struct_size %u, expected %zu (ABI version %u)", d->struct_size, sizeof(zk_plonk_keygen_desc), ZK_ABI_VERSION);
    const uint32_t k = d->k, F = d->n_fixed, M = d->n_perm_columns;
    if (k < 1 || k > 27) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_vk: k = %u (1 .. 27)", k);
    if ((F && (!d->fixed_values || !fixed_commitments)) || (M && (!d->perm_map_column || !d->perm_map_row || !permutation_commitments)))
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_vk: null column / mapping / output array");
    for (uint32_t i = 0; i < F; i++) if (!d->fixed_values[i]) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_vk: fixed column %u is NULL", i);
    if (((uint64_t)M << k) >= (1ull << 32)) return pk_fail(ctx, ZK_ERR_LIMIT, "zk_plonk_keygen_vk: %u permutation columns of 2^%u rows: 2^32 mapping cells or more", M, k);
    PK(kg_whole_table(ctx, "zk_plonk_keygen_vk", "srs_g_lagrange", srs_g_lagrange, k, false));
    const size_t n = (size_t)1 << k, col_bytes = n * 32;
    KgHandle h;
    h.k = k;
    h.cols = std::make_shared<KgCols>();                              // (every way out but the last frees what was allocated so far)
    h.cols->device = ctx->device;
    auto alloc = [&]() -> void* {
        h.cols->owned.reserve(h.cols->owned.size() + 1);
        void* p = nullptr;
        if (zk_dev_alloc(ctx, col_bytes, &p) != ZK_OK) return nullptr;
        h.cols->owned.push_back(p);
        return p;
    };
    std::vector<void*> up, sig;
    for (uint32_t i = 0; i < F; i++) {
        if (d->values_on_device) { h.fixed.push_back(d->fixed_values[i]); continue; }
        void* p = alloc();
        if (!p) return ZK_ERR_HIP;
        up.push_back(p); h.fixed.push_back(p);
    }
    if (!up.empty()) PK(zk_dev_upload_batch(ctx, up.data(), d->fixed_values, up.size(), col_bytes));
    for (uint32_t j = 0; j < M; j++) {
        void* p = alloc();
        if (!p) return ZK_ERR_HIP;
        sig.push_back(p); h.sigma.push_back(p);
    }
    if (M) PK(keygen_sigma(ctx, d->perm_map_column, d->perm_map_row, M, k, sig.data()));
    std::vector<const void*> all(h.fixed);
    all.insert(all.end(), h.sigma.begin(), h.sigma.end());
    std::vector<unsigned char> points(all.size() * 96 + 1);
    if (!all.empty()) PK(zk_msm_batch_dev(ctx, srs_g_lagrange, all.data(), all.size(), n, points.data()));
    if (F) memcpy(fixed_commitments, points.data(), (size_t)F * 96);
    if (M) memcpy(permutation_commitments, points.data() + (size_t)F * 96, (size_t)M * 96);
    std::lock_guard<std::mutex> lk(g_pk_mu);
    g_kg_handles[{ctx, g_pk_next}] = std::move(h);
    *kg = g_pk_next++;
    return ZK_OK;
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_keygen_columns(zk_ctx* ctx, uint64_t kg, const void** fixed_dev, const void** sigma_dev) ZK_ABI_TRY {
    if (!ctx) return ZK_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_pk_mu);
    auto it = g_kg_handles.find({ctx, kg});
    if (it == g_kg_handles.end()) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_columns: unknown keygen handle %llu", (unsigned long long)kg);
    const KgHandle& h = it->second;
    if ((!h.fixed.empty() && !fixed_dev) || (!h.sigma.empty() && !sigma_dev)) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_columns: null output array");
    for (size_t i = 0; i < h.fixed.size(); i++) fixed_dev[i] = h.fixed[i];
    for (size_t j = 0; j < h.sigma.size(); j++) sigma_dev[j] = h.sigma[j];
    return ZK_OK;
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_keygen_pk(zk_ctx* ctx, uint64_t kg, const zk_plonk_pk_host* host, const zk_plonk_phases* phases, uint64_t srs_g, uint64_t srs_g_lagrange,
                                  uint64_t* pk) ZK_ABI_TRY {
    if (!ctx || !host || !pk) return ZK_ERR_ARG;
    if (host->struct_size != sizeof(zk_plonk_pk_host))
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_pk: zk_plonk_pk_host.struct_size %u, expected %zu (ABI version %u)", host->struct_size, sizeof(zk_plonk_pk_host), ZK_ABI_VERSION);
    if (host->fixed_values || host->sigma_values)
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_pk: host->fixed_values / sigma_values must be NULL: the key is built on the keygen handle's columns");
    if (host->shard_world > 1) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_pk: shard_world %u: keygen runs on one GPU with the whole table", host->shard_world);
    KgHandle h;                                                       // a copy: the columns stay alive through the build whatever another thread releases meanwhile
    {
        std::lock_guard<std::mutex> lk(g_pk_mu);
        auto it = g_kg_handles.find({ctx, kg});
        if (it == g_kg_handles.end()) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_pk: unknown keygen handle %llu", (unsigned long long)kg);
        h = it->second;
    }
    if (host->k != h.k || host->n_fixed != h.fixed.size() || host->n_perm_columns != h.sigma.size())
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_keygen_pk: host describes k = %u with %u fixed and %u permutation columns, the keygen handle holds k = %u with %zu and %zu",
                       host->k, host->n_fixed, host->n_perm_columns, h.k, h.fixed.size(), h.sigma.size());
    PK(kg_whole_table(ctx, "zk_plonk_keygen_pk", "srs_g", srs_g, h.k, true));
    PK(kg_whole_table(ctx, "zk_plonk_keygen_pk", "srs_g_lagrange", srs_g_lagrange, h.k, false));
    zk_plonk_pk_host on_handle = *host;
    h.fixed.push_back(nullptr); h.sigma.push_back(nullptr);           // (.data() of an empty vector may be null)
    on_handle.fixed_values = h.fixed.data(); on_handle.sigma_values = h.sigma.data(); on_handle.values_on_device = 1;
    return pk_build(ctx, &on_handle, phases, srs_g, srs_g_lagrange, pk, h.cols);
} ZK_ABI_CATCH(ctx)

extern "C" int zk_plonk_keygen_release(zk_ctx* ctx, uint64_t kg) ZK_ABI_TRY {
    if (!ctx) return ZK_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_pk_mu);
    auto it = g_kg_handles.find({ctx, kg});
    if (it == g_kg_handles.end()) return ZK_ERR_ARG;
    g_kg_handles.erase(it);
    return ZK_OK;
} ZK_ABI_CATCH(ctx)

// zk_ctx_destroy (capi.hip): the keys this context still holds go with it (before its programs are released)
void zk_internal_plonk_ctx_destroyed(zk_ctx* ctx) {
    std::lock_guard<std::mutex> lk(g_pk_mu);
    for (auto it = g_pk_handles.begin(); it != g_pk_handles.end();) {
        if (it->first.first == ctx) { if (it->second->in_use) it->second->released = true; else pk_drop(ctx, it->second); it = g_pk_handles.erase(it); }
        else ++it;
    }
    for (auto it = g_kg_handles.begin(); it != g_kg_handles.end();) it = it->first.first == ctx ? g_kg_handles.erase(it) : std::next(it);
}
