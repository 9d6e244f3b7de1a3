// Native create_proof: halo2_proofs::plonk::create_proof + ProverSHPLONK (zkwebauthn/halo2 @ c254c75, Cargo.lock:1314-1327) as the reference calls
// them at circuits/src/sgx_dcap_verifier.rs:814-822 — the per-proof path of a phase-batched, HBM-resident `plonk/prover.rs`, written in C++ because the
// reference's host side is compiled code (Rust) and no Rust toolchain exists in the build image.  It is a CLIENT of the C ABI (include/zkmi355.h): every
// O(n) step is one of the zk_* entry points the Rust prover would call, in the order of INTEGRATION.md's phase table; what stays on the host is what
// stays on the host in the reference — Fiat-Shamir hashing (transcript.h; src/transcript.rs), point encoding, rotation-set bookkeeping and the O(#points^2)
// interpolations of SHPLONK.  zk-dcap-verifier_amd/plonk/prover.py + shplonk.py are the Python twin (phase by phase, draw by draw): `Proof` below has one member
// function per phase of prover.py, and both must emit the bytes of the independent CPU prover's goldens (tests/test_native_prover.py).  One circuit instance or
// several (zk_plonk_create_proof_multi: one proof over m circuits that share the key); advice in up to three phases with user challenges between them when the key
// carries phase lists (zk_plonk_prove_phased, PhaseSpec in plonk_shared.h).  The key object (pk.hip) enters through those two functions only.
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "field.cuh"
#include "../../include/zkmi355.h"
#include "abi_guard.h"
#include "plonk_shared.h"
#include "transcript.h"

using namespace zk;

zk_ctx* zk_internal_helper_ctx(zk_ctx* ctx);                      // capi.hip: the helper context of ctx (ctx.h), or null
void zk_internal_trim_helper(zk_ctx* ctx);                        // capi.hip: give the helper context's grow-only device memory back (zk_plonk_trim)
int zk_internal_permutation_products(zk_ctx* ctx, const void* const* values, const void* const* sigmas, size_t n_columns, size_t n_circuits, uint32_t chunk_len, uint32_t k,
                                     const void* beta, const void* gamma, const void* blinding, uint32_t blinding_factors, void* const* z_devs);   // capi.hip: the m-circuit permutation products
#define PK(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

namespace {
// ---- device memory of one proof: size-keyed free lists kept per context across proofs ------------------------------------------------------------------
struct Pool {
    std::mutex mu;
    std::map<size_t, std::vector<void*>> free_;
    std::vector<std::vector<uint64_t>> draw_bufs;                     // host buffers of the rng draws of finished proofs (one per proof in flight on the context), reused: a proof
                                                                      // draws n + O(columns) field elements — 16 MiB at k = 19 — and fresh pages every proof cost mmap churn
    bool retired = false;                                             // zk_plonk_trim ran while a proof of this context still held buffers: they are freed as they come back
};
std::mutex g_pools_mu;
std::map<zk_ctx*, std::shared_ptr<Pool>> g_pools;
std::shared_ptr<Pool> pool_of(zk_ctx* ctx) {
    std::lock_guard<std::mutex> lk(g_pools_mu);
    std::shared_ptr<Pool>& p = g_pools[ctx];
    if (!p) p = std::make_shared<Pool>();
    return p;
}
struct Arena {                                                        // everything a proof allocates goes back to the pool when it ends
    zk_ctx* ctx; std::shared_ptr<Pool> pool; std::vector<std::pair<void*, size_t>> held;
    explicit Arena(zk_ctx* c) : ctx(c), pool(pool_of(c)) {}
    void* get(size_t bytes) {
        void* p = nullptr;
        {
            std::lock_guard<std::mutex> lk(pool->mu);
            auto& v = pool->free_[bytes];
            if (!v.empty()) { p = v.back(); v.pop_back(); }
        }
        if (!p && zk_dev_alloc(ctx, bytes, &p) != ZK_OK) return nullptr;
        try { held.push_back({p, bytes}); } catch (...) { put(p, bytes); throw; }
        return p;
    }
    int take(void*& p, size_t bytes) { p = get(bytes); return p ? ZK_OK : ZK_ERR_HIP; }      // an arena buffer, or ZK_ERR_HIP ...
    int take(std::vector<void*>& v, size_t bytes) { for (void*& p : v) PK(take(p, bytes)); return ZK_OK; }     // ... one for every element of v
    void put(void* p, size_t bytes) noexcept {                         // (runs in destructors: a buffer the free list cannot take is freed instead)
        bool keep = false;
        try { std::lock_guard<std::mutex> lk(pool->mu); if (!pool->retired) { pool->free_[bytes].push_back(p); keep = true; } } catch (...) {}
        if (!keep) (void)zk_dev_free(ctx, p);
    }
    void give_back(void* p) {
        for (auto& h : held) if (h.first == p) { put(p, h.second); h.first = nullptr; return; }
    }
    ~Arena() { for (auto& h : held) if (h.first) put(h.first, h.second); }
};

// ---- transforms that need no challenge, beside the commitments that do ------------------------------------------------------------------------------------------------
// A proof alone on the GPU spends a third of phases 2-5 in the MSM's sort, its reduction tail and the host's folds — latency, not arithmetic — and every commitment waits for
// the transcript.  The coefficient and extended forms of a phase's columns depend on no challenge: as soon as a phase's values are final they go to the context's HELPER
// context (own stream, workspaces, lock: ctx.h) from a helper host thread, jobs in submission order, while the proof's own thread commits the same columns; phase 6 waits
// for them instead of transforming everything at once.  Same field elements, same bytes.
struct SideLane {
    zk_ctx* h = nullptr;
    std::thread th;
    std::mutex mu; std::condition_variable cv;
    std::deque<std::function<int()>> q;
    size_t open = 0; bool closing = false; int rc = ZK_OK;
    void start(zk_ctx* helper) {
        h = helper;
        fault_thread_tick();
        th = std::thread([this]() {
            std::unique_lock<std::mutex> lk(mu);
            while (true) {
                cv.wait(lk, [&] { return closing || !q.empty(); });
                if (q.empty()) break;
                std::function<int()> f = std::move(q.front());
                q.pop_front();
                const int before = rc;
                lk.unlock();
                int r = before;                                       // (after an error the remaining jobs are dropped)
                if (!r) { try { r = f(); } catch (...) { r = abi_exception(h, "zk_plonk_create_proof (helper thread)"); } }      // nothing may leave a thread's entry function: it becomes the lane's rc
                lk.lock();
                if (r && !rc) rc = r;
                open--;
                cv.notify_all();
            }
        });
    }
    void submit(std::function<int()> f) { { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(f)); open++; } cv.notify_all(); }
    int wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return open == 0; }); return rc; }
    ~SideLane() {
        if (!th.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu); closing = true; }
        cv.notify_all();
        th.join();                                                     // (jobs in flight finish: they write buffers of the proof's arena, which outlives this object)
    }
};

// ---- the caller's Fr::random draws, made on a helper thread in the order the phases consume them ---------------------------------------------------------
struct Draws {
    std::vector<uint64_t> buf;                                        // all items back to back (count x 4 limbs each), borrowed from the context's pool
    std::vector<size_t> counts, offs;
    std::shared_ptr<Pool> pool;
    std::mutex mu; std::condition_variable cv; size_t done = 0;
    std::thread th;
    std::atomic<bool> abandoned{false};                                // the proof ended early (an error): stop asking the caller for randomness nobody will use
    int failed = 0;                                                    // the helper thread could not get its buffer (mu): every take() from then on throws the code to the proof's thread
    void start(zk_rng_fn rng, void* user, std::shared_ptr<Pool> p) {
        pool = std::move(p);
        size_t total = 4;
        for (size_t c : counts) { offs.push_back(total); total += c * 4; }
        {
            std::lock_guard<std::mutex> lk(pool->mu);
            if (!pool->draw_bufs.empty()) { buf.swap(pool->draw_bufs.back()); pool->draw_bufs.pop_back(); }
        }
        fault_thread_tick();
        th = std::thread([this, rng, user, total]() {
            try {
                if (buf.size() < total) buf.resize(total);             // (first proof of a context only; on the helper thread, off the proof's critical path)
            } catch (...) {
                { std::lock_guard<std::mutex> lk(mu); failed = abi_exception(nullptr, "zk_plonk_create_proof (rng thread)"); }
                cv.notify_all();
                return;
            }
            for (size_t i = 0; i < counts.size() && !abandoned.load(); i++) {
                if (counts[i]) rng(user, counts[i], buf.data() + offs[i]);
                { std::lock_guard<std::mutex> lk(mu); done = i + 1; }
                cv.notify_all();
            }
        });
    }
    const uint64_t* take(size_t i) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done > i || failed; });
        if (failed) throw AbiError{failed, "the rng helper thread could not allocate its draw buffer"};
        return buf.data() + offs[i];
    }
    void finish() { if (!counts.empty()) (void)take(counts.size() - 1); }     // a successful proof leaves the caller's stream where halo2 would: every planned draw made
    ~Draws() {
        abandoned.store(true);
        if (th.joinable()) th.join();
        try {
            if (pool && !buf.empty()) { std::lock_guard<std::mutex> lk(pool->mu); if (!pool->retired && pool->draw_bufs.size() < 8) pool->draw_bufs.emplace_back(std::move(buf)); }
        } catch (...) {}                                              // (a destructor: the buffer is simply not kept)
    }
};

struct Query { const void* poly; Fe point; Fe eval; uint64_t open; };  // ProverQuery { point, poly } + its evaluation + its place in the multi-open order (Proof::evaluations)

// coefficients of the Lagrange basis polynomials of a point set: every commitment of a rotation set is interpolated over the SAME points, so the products
// and the field inversions (one Fermat exponentiation each on the host) are done once per set
std::vector<std::vector<Fe>> lagrange_basis(const std::vector<Fe>& pts) {
    const size_t n = pts.size();
    std::vector<std::vector<Fe>> basis(n);
    for (size_t j = 0; j < n; j++) {
        std::vector<Fe> num{Fr::one()};
        Fe den = Fr::one();
        for (size_t m = 0; m < n; m++) {
            if (m == j) continue;
            std::vector<Fe> nx(num.size() + 1);
            nx[0] = Fr::neg(Fr::mul(pts[m], num[0]));
            for (size_t i = 1; i < num.size(); i++) nx[i] = Fr::sub(num[i - 1], Fr::mul(pts[m], num[i]));
            nx[num.size()] = num.back();
            num.swap(nx);
            den = Fr::mul(den, Fr::sub(pts[j], pts[m]));
        }
        const Fe sc = Fr::inv(den);
        basis[j].resize(n);
        for (size_t i = 0; i < n; i++) basis[j][i] = Fr::mul(num[i], sc);
    }
    return basis;
}
std::vector<Fe> interpolate_with_basis(const std::vector<std::vector<Fe>>& basis, const std::vector<Fe>& evals) {
    const size_t n = basis.size();
    std::vector<Fe> coeffs(n, Fr::zero());
    for (size_t j = 0; j < n; j++) for (size_t i = 0; i < n; i++) coeffs[i] = Fr::add(coeffs[i], Fr::mul(evals[j], basis[j][i]));
    return coeffs;
}
Fe eval_small(const std::vector<Fe>& c, const Fe& x) { Fe acc = Fr::zero(); for (size_t i = c.size(); i-- > 0;) acc = Fr::add(Fr::mul(acc, x), c[i]); return acc; }
Fe vanishing_at(const std::vector<Fe>& roots, const Fe& z) { Fe acc = Fr::one(); for (auto& r : roots) acc = Fr::mul(acc, Fr::sub(z, r)); return acc; }
// field elements as the uint64_t[4] limbs the ABI takes, back to back (zero-padded to `pad` elements)
std::vector<uint64_t> packed(const std::vector<Fe>& xs, size_t pad = 0) {
    std::vector<uint64_t> out(std::max(xs.size(), pad) * 4, 0);
    for (size_t i = 0; i < xs.size(); i++) memcpy(&out[4 * i], xs[i].v, 32);
    return out;
}

// what the calling thread's last proof squeezed (zk_plonk_last_challenges): the user challenges in index order, then theta, beta, gamma, y, x, SHPLONK's y, v, u in squeeze order
struct Squeezed { std::vector<Fe> user, rest; };
thread_local Squeezed g_squeezed;
Fe squeeze_noted(Transcript& tr) { const Fe c = tr.squeeze(); g_squeezed.rest.push_back(c); return c; }

// ProverSHPLONK::create_proof(transcript, queries) — plonk/shplonk.py's function of the same name: `queries` in halo2's multi-open order, polynomials of n
// coefficients on the device; `commit` commits one of them against the monomial SRS and writes the point to the transcript
int shplonk_create_proof(zk_ctx* ctx, Arena& mem, Transcript& tr, const std::vector<Query>& queries, size_t n, const std::function<int(void*)>& commit) {
    const size_t col_bytes = n * 32;
    const Fe one = Fr::one(), yy = squeeze_noted(tr);
    // construct_intermediate_sets: commitments (by polynomial) in first-appearance order, their point sets ascending by canonical value, sets in first-appearance order
    struct Com { const void* poly; std::map<u256, Fe, CanonLess> pts; };          // canonical point -> eval
    std::vector<Com> coms;
    std::map<u256, Fe, CanonLess> super;                                          // canonical -> Montgomery point
    for (auto& qq : queries) {
        const u256 cp = Fr::from_mont(qq.point);
        super.emplace(cp, qq.point);
        size_t ci = 0;
        while (ci < coms.size() && coms[ci].poly != qq.poly) ci++;
        if (ci == coms.size()) coms.push_back(Com{qq.poly, {}});
        coms[ci].pts.emplace(cp, qq.eval);
    }
    struct RSet { std::vector<u256> keys; std::vector<size_t> members; };
    std::vector<RSet> sets;
    for (size_t ci = 0; ci < coms.size(); ci++) {
        std::vector<u256> keys;
        for (auto& kv : coms[ci].pts) keys.push_back(kv.first);
        size_t si = 0;
        for (; si < sets.size(); si++) {
            if (sets[si].keys.size() != keys.size()) continue;
            bool same = true;
            for (size_t i = 0; i < keys.size() && same; i++) same = Fr::eq(sets[si].keys[i], keys[i]);
            if (same) break;
        }
        if (si == sets.size()) sets.push_back(RSet{keys, {}});
        sets[si].members.push_back(ci);
    }
    const Fe v = squeeze_noted(tr);
    size_t pad = 1;
    for (auto& s : sets) pad = std::max(pad, s.keys.size());
    void* rbuf = mem.get(col_bytes);
    void* tmp0 = mem.get(col_bytes);
    void* tmp1 = mem.get(col_bytes);
    if (!rbuf || !tmp0 || !tmp1) return ZK_ERR_HIP;
    PK(zk_dev_zero(ctx, rbuf, col_bytes));
    std::vector<void*> quotients;
    std::vector<std::vector<std::vector<Fe>>> low(sets.size());                    // per set, per member: r(X) coefficients
    for (size_t si = 0; si < sets.size(); si++) {
        const RSet& s = sets[si];
        std::vector<Fe> pts;
        for (auto& key : s.keys) pts.push_back(super[key]);
        std::vector<Fe> rsum(pts.size(), Fr::zero());
        std::vector<const void*> polys;
        std::vector<Fe> scal;
        Fe ypow = Fr::one();
        const std::vector<std::vector<Fe>> basis = lagrange_basis(pts);
        for (size_t ci : s.members) {
            std::vector<Fe> evals;
            for (auto& key : s.keys) evals.push_back(coms[ci].pts[key]);
            const std::vector<Fe> r = interpolate_with_basis(basis, evals);
            for (size_t i = 0; i < r.size(); i++) rsum[i] = Fr::sub(rsum[i], Fr::mul(ypow, r[i]));
            low[si].push_back(r);
            polys.push_back(coms[ci].poly);
            scal.push_back(ypow);
            ypow = Fr::mul(ypow, yy);
        }
        PK(zk_dev_upload(ctx, rbuf, packed(rsum, pad).data(), pad * 32));
        polys.push_back(rbuf);
        scal.push_back(one);
        PK(zk_fr_lincomb_dev(ctx, polys.data(), packed(scal).data(), polys.size(), n, tmp0));
        void* cur = tmp0; void* oth = tmp1;
        size_t ln = n;
        for (auto& p : pts) { PK(zk_kate_division_dev(ctx, cur, ln, p.v, oth)); std::swap(cur, oth); ln--; }
        void* qi = nullptr;
        PK(mem.take(qi, col_bytes));
        PK(zk_fr_scale_dev(ctx, cur, one.v, qi, ln));
        if (n > ln) PK(zk_dev_zero(ctx, (char*)qi + ln * 32, (n - ln) * 32));
        quotients.push_back(qi);
    }
    std::vector<Fe> vp(sets.size());
    { Fe p = Fr::one(); for (size_t i = 0; i < sets.size(); i++) { vp[i] = p; p = Fr::mul(p, v); } }
    void* h_x = nullptr;
    PK(mem.take(h_x, col_bytes));
    PK(zk_fr_lincomb_dev(ctx, (const void* const*)quotients.data(), packed(vp).data(), quotients.size(), n, h_x));
    PK(commit(h_x));
    const Fe u = squeeze_noted(tr);
    std::vector<Fe> super_pts;
    for (auto& kv : super) super_pts.push_back(kv.second);
    std::vector<Fe> z_diffs(sets.size());
    std::vector<const void*> polys;
    std::vector<Fe> scal;
    Fe cst = Fr::zero();
    for (size_t si = 0; si < sets.size(); si++) {
        std::vector<Fe> diffs;
        for (auto& kv : super) {
            bool in_set = false;
            for (auto& key : sets[si].keys) in_set |= Fr::eq(key, kv.first);
            if (!in_set) diffs.push_back(kv.second);
        }
        z_diffs[si] = vanishing_at(diffs, u);
        Fe ypow = Fr::one();
        for (size_t m = 0; m < sets[si].members.size(); m++) {
            const Fe w = Fr::mul(Fr::mul(vp[si], z_diffs[si]), ypow);
            polys.push_back(coms[sets[si].members[m]].poly);
            scal.push_back(w);
            cst = Fr::sub(cst, Fr::mul(w, eval_small(low[si][m], u)));
            ypow = Fr::mul(ypow, yy);
        }
    }
    const Fe zt = vanishing_at(super_pts, u), z0_inv = Fr::inv(z_diffs[0]);
    polys.push_back(h_x);
    scal.push_back(Fr::neg(zt));
    PK(zk_dev_upload(ctx, rbuf, packed({Fr::mul(cst, z0_inv)}, pad).data(), pad * 32));
    polys.push_back(rbuf);
    for (Fe& w : scal) w = Fr::mul(w, z0_inv);
    scal.push_back(one);
    PK(zk_fr_lincomb_dev(ctx, polys.data(), packed(scal).data(), polys.size(), n, tmp0));
    PK(zk_kate_division_dev(ctx, tmp0, n, u.v, tmp1));
    PK(zk_dev_zero(ctx, (char*)tmp1 + (n - 1) * 32, 32));
    return commit(tmp1);
}

// ProverGWC::create_proof(transcript, queries) — plonk/gwc.py's function of the same name ([3P-MEM] halo2_proofs v2023_01_20 src/poly/kzg/multiopen/gwc/prover.rs): the
// same `queries`; squeeze v, group them by point in order of first appearance (a linear scan: points unsorted, queries not deduplicated, their order kept), and per
// group commit W = kate_division(sum_j v^j poly_j, point) — the constant term, hence the "- eval" of halo2's poly_batch, never enters the quotient.  All groups at
// once: one batched combination, one batched division, and `commit` takes the P witness columns as one batch and writes their points in group order.
int gwc_create_proof(zk_ctx* ctx, Arena& mem, Transcript& tr, const std::vector<Query>& queries, size_t n, const std::function<int(const std::vector<void*>&)>& commit) {
    const size_t col_bytes = n * 32;
    const Fe v = squeeze_noted(tr);
    struct Group { u256 key; Fe point; std::vector<size_t> members; };            // key: the canonical point
    std::vector<Group> groups;
    for (size_t i = 0; i < queries.size(); i++) {
        const u256 cp = Fr::from_mont(queries[i].point);
        size_t gi = 0;
        while (gi < groups.size() && !Fr::eq(groups[gi].key, cp)) gi++;
        if (gi == groups.size()) groups.push_back(Group{cp, queries[i].point, {}});
        groups[gi].members.push_back(i);
    }
    const size_t P = groups.size();
    if (!P) return ZK_OK;
    std::vector<const void*> polys;
    std::vector<Fe> scal, pts;
    std::vector<uint32_t> offsets{0};
    for (const Group& g : groups) {
        Fe vp = Fr::one();                                                        // the j-th query of a group gets v^j, from v^0 in every group
        for (size_t qi : g.members) { polys.push_back(queries[qi].poly); scal.push_back(vp); vp = Fr::mul(vp, v); }
        offsets.push_back((uint32_t)polys.size());
        pts.push_back(g.point);
    }
    std::vector<void*> batch(P, nullptr), wit(P, nullptr);
    PK(mem.take(batch, col_bytes));
    PK(mem.take(wit, col_bytes));
    PK(zk_fr_lincomb_batch_dev(ctx, polys.data(), packed(scal).data(), offsets.data(), P, n, batch.data()));
    PK(zk_kate_division_batch_dev(ctx, (const void* const*)batch.data(), P, n, packed(pts).data(), wit.data()));
    for (void* b : batch) mem.give_back(b);
    for (void* w : wit) PK(zk_dev_zero(ctx, (char*)w + (n - 1) * 32, 32));         // n - 1 coefficients: the column the commitment reads has n
    return commit(wit);
}

thread_local double g_phase_ms[9];                                    // wall time of the phases of the calling thread's last proof (zk_plonk_last_phase_ms)
struct PhaseClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(int phase) {
        const auto now = std::chrono::steady_clock::now();
        g_phase_ms[phase] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    }
};

// One proof over several ranks: the ranks run in lockstep from collective to collective, so a rank that fails on its own (out of memory, a HIP error, its witness
// outside a lookup table, an rng callback error) must not simply return — the others would wait in the next all-gather for ever.  It enters that NEXT exchange once more
// with a poisoned block (first 32 bytes 0xFF: no field element and no point coordinate has that value) and returns its error; every other rank finds the mark in
// the gathered blocks and returns ZK_ERR_COMM from the same exchange.  Not covered: a failing collective itself, and a rank that cannot even allocate its exchange
// buffers — the callback must enforce a timeout for those (include/zkmi355.h, zk_allgather_fn).
struct ShardSignal {
    std::vector<size_t> sizes;                                         // bytes of every exchange of this proof, in order (the same list on every rank)
    size_t next = 0;                                                   // the exchange every healthy rank enters next
    void* xsend = nullptr; void* xrecv = nullptr;
    bool armed = false;
    Arena* xmem = nullptr;                                             // the wrapper's arena: library-owned exchange buffers must outlive the body, whose failure they announce
};
static const uint64_t POISON[4] = {~0ull, ~0ull, ~0ull, ~0ull};

// proofs this process has in flight (every device together: a prover process drives one GPU): the side lane fills a lone proof's idle issue slots — with three and more
// in flight the other proofs do that already, and a helper context per proof only adds kernels to the crowd (measured: DESIGN 3.7)
static std::atomic<int> g_proofs_in_flight{0};
struct InFlight { InFlight() { g_proofs_in_flight.fetch_add(1); } ~InFlight() { g_proofs_in_flight.fetch_sub(1); } };

// One column of a proof.  The side lane fills `coef` and `ext` while `val` is committed, and `val` goes back to the pool; without it `val` is brought to
// coefficient form in place (coef = val) and the extended form is made per circuit inside the quotient phase.
struct Column { void* val = nullptr; void* coef = nullptr; void* ext = nullptr; bool owned = false; };   // value (Lagrange), coefficient, extended form; the arena owns `val`

// m circuits that share the key (m = 1: the single-circuit proof, byte for byte).  Where halo2 loops over the circuits ([3P-MEM] plonk/prover.rs, evaluation.rs), so do
// the transcript and the draws: per circuit in order 0 .. m-1; what the key holds (fixed, sigma, l0 / l_last / l_active_row) and the vanishing argument exist once.  Every
// phase gathers the columns of all m circuits into its batched launch; the quotient runs per (circuit, coset or part), circuit 0 plain and the others in accumulate mode.
struct Proof {
    zk_ctx* const ctx; const zk_plonk_pk_desc* const pk; const uint32_t m;
    const void* const* const advice; const int advice_on_device; const void* const* const instances; const uint32_t* const instance_lens;
    const zk_rng_fn rng; void* const rng_user; void* const proof_out; const size_t proof_cap; size_t* const proof_len; ShardSignal& sig;
    const PhaseSpec* const ph;                                         // the key's phase lists and the caller's callback (zk_plonk_prove_phased), or null: every column in phase 0, no challenge
    // sizes derived from the descriptor (validate_and_plan)
    uint32_t k = 0, ek = 0, bf = 0, L = 0, A = 0, I = 0, chunk = 0, n_sets = 0, n_pieces = 0, world = 1, rank = 0, n_phases = 1, n_chal = 0;
    size_t n = 0, en = 0, col_bytes = 0, usable = 0, n_loc = 0, shard_lo = 0, mA = 0, mI = 0, mL = 0, mS = 0, W = 0;
    bool sharded = false, by_cosets = false, side = false;
    uint32_t multiopen = ZK_MULTIOPEN_SHPLONK;                         // the context's setting when the proof began (zk_plonk_multiopen_set)
    QuotUnits qu;                                                      // the quotient's units of this rank (sharded)
    // Destruction runs upwards from here and the order matters: `draws` joins the rng thread first, then `lane` joins the helper thread, and only then `mem` returns
    // the buffers those threads write to the pool.  The exchange arena (ShardSignal::xmem, the entry's) outlives all of it.
    Arena mem{ctx};
    SideLane lane;
    Transcript tr{0};
    Draws draws;
    PhaseClock clk;
    std::vector<size_t> d_ar, d_bi, d_bt, d_pb, d_lb;                  // items of the draw plan: advice rows | lookup input, table rows | permutation, lookup product rows
    size_t d_rp = 0;                                                   // ... and the random polynomial
    const Fe one = Fr::one();
    Fe theta, beta, gamma, y, x;
    std::vector<uint64_t> chal;                                        // the user challenges, Montgomery limbs back to back (zero until squeezed); what the programs and the callback read
    // the proof's columns: m x n_advice, m x n_instance, m x n_sets, m x n_lookups (three times), circuit-major
    std::vector<Column> adv, inst, zs, lzs, pin, ptab;
    std::vector<void*> cin, ctab;                                      // compressed lookup expressions (m x n_lookups; value form only)
    void* random_poly = nullptr; void* h_ext = nullptr; void* h_poly = nullptr;
    uint32_t low_cosets = 0;
    std::vector<void*> numer, numer_low, pieces;
    std::vector<Query> q;
    size_t plan(size_t count) { draws.counts.push_back(count); return draws.counts.size() - 1; }
    std::vector<uint64_t> drawn(const std::vector<size_t>& items, size_t count) {      // the rows of several draw items back to back, as the batched entry points take them
        std::vector<uint64_t> v(items.size() * count * 4);
        for (size_t i = 0; i < items.size(); i++) memcpy(&v[i * count * 4], draws.take(items[i]), count * 32);
        return v;
    }
    uint32_t phase_of(uint32_t column) const { return ph && ph->advice_phase ? ph->advice_phase[column] : 0; }
    const void* challenges() const { return n_chal ? (const void*)chal.data() : (const void*)one.v; }
    int fresh(Column& c) { c.owned = true; return mem.take(c.val, col_bytes); }
    static std::vector<void*> vals_of(const std::vector<Column*>& cols) { std::vector<void*> v; for (Column* c : cols) v.push_back(c->val); return v; }
    static std::vector<Column*> ptrs(std::vector<Column>& a) { std::vector<Column*> v; for (Column& c : a) v.push_back(&c); return v; }
    static std::vector<Column*> ptrs(std::vector<Column>& a, std::vector<Column>& b) { std::vector<Column*> v = ptrs(a), w = ptrs(b); v.insert(v.end(), w.begin(), w.end()); return v; }
    int validate_and_plan() {
        if (!ctx || !pk || !m) return ZK_ERR_ARG;
        if (pk->struct_size != sizeof(zk_plonk_pk_desc))
            return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof: zk_plonk_pk_desc.struct_size %u, expected %zu (ABI version %u)", pk->struct_size, sizeof(zk_plonk_pk_desc), ZK_ABI_VERSION);
        if (!rng || !proof_len || (pk->n_advice && !advice)) return ZK_ERR_ARG;
        k = pk->k; ek = pk->extended_k; bf = pk->blinding_factors; L = pk->n_lookups;
        if (k < 1 || ek < k || ek > 27) return ZK_ERR_ARG;
        n = (size_t)1 << k; en = (size_t)1 << ek; col_bytes = n * 32;
        if (bf + 2 >= n || pk->cs_degree < 3) return ZK_ERR_ARG;
        usable = n - (bf + 1);
        chunk = pk->cs_degree - 2;
        n_sets = pk->n_perm_columns ? (pk->n_perm_columns + chunk - 1) / chunk : 0;
        n_pieces = pk->cs_degree - 1;
        // the descriptor is the caller's: refuse indices that would read outside its arrays
        world = pk->shard_world > 1 ? pk->shard_world : 1; rank = world > 1 ? pk->shard_rank : 0;
        sharded = world > 1;
        if (sharded && m > 1) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof_multi: %u circuits on a sharded key (shard_world %u): one proof over several circuits runs on one GPU", m, world);
        PK(zk_plonk_multiopen_get(ctx, &multiopen));
        if (sharded && multiopen == ZK_MULTIOPEN_GWC)
            return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof: the GWC multi-open on a sharded key (shard_world %u): one proof over several GPUs ends with SHPLONK", world);
        A = pk->n_advice; I = pk->n_instance;                         // per circuit; circuit c's columns are [c * A, (c + 1) * A) etc. (circuit-major)
        if ((pk->n_fixed && (!pk->fixed_values || !pk->fixed_polys)) || (pk->n_perm_columns && (!pk->perm_columns || !pk->sigma_values || !pk->sigma_polys)) ||
            (L && (!pk->lookup_input_programs || !pk->lookup_table_programs || !pk->lookup_table_key)) || (pk->n_advice_queries && !pk->advice_queries) ||
            (pk->n_fixed_queries && !pk->fixed_queries) || !pk->transcript_repr)
            return ZK_ERR_ARG;
        // a single-GPU key that holds cosets 0 .. n_pieces-1 instead of the extended domain (zk_plonk_pk_build does when cs_degree - 1 is not a power of two): the quotient is
        // evaluated on those cosets only and the pieces of h(X) come from zk_cosets_to_pieces_dev
        by_cosets = !sharded && pk->coset_l && pk->coset_l[0] && n_pieces < (1u << (ek - k)) && n_pieces <= 8;
        if (!sharded && !by_cosets && ((pk->n_fixed && !pk->fixed_cosets) || (pk->n_perm_columns && !pk->sigma_cosets) || !pk->l0 || !pk->l_last || !pk->l_active_row)) return ZK_ERR_ARG;
        if (by_cosets && ((pk->n_fixed && !pk->coset_fixed) || (pk->n_perm_columns && !pk->coset_sigma))) return ZK_ERR_ARG;
        if (sharded && (rank >= world || n % world || !pk->allgather || (pk->n_fixed && !pk->coset_fixed) || (pk->n_perm_columns && !pk->coset_sigma) || !pk->coset_l)) return ZK_ERR_ARG;
        qu = quotient_units(world, rank, k, ek);
        n_loc = n / world; shard_lo = (size_t)rank * n_loc;
        for (uint32_t j = 0; j < pk->n_perm_columns; j++) {
            const uint32_t ty = pk->perm_columns[2 * j], ix = pk->perm_columns[2 * j + 1];
            if (ty > 2 || ix >= (ty == 0 ? pk->n_advice : ty == 1 ? pk->n_fixed : pk->n_instance)) return ZK_ERR_ARG;
        }
        for (uint32_t i = 0; i < pk->n_advice_queries; i++) if (pk->advice_queries[2 * i] >= pk->n_advice) return ZK_ERR_ARG;
        for (uint32_t i = 0; i < pk->n_fixed_queries; i++) if (pk->fixed_queries[2 * i] >= pk->n_fixed) return ZK_ERR_ARG;
        // phases ([3P-MEM] plonk/circuit.rs: advice_column_phase, challenge_phase; pk.hip has validated the key's lists): later-phase entries of `advice` are the callback's to fill
        if (ph) {
            n_chal = ph->n_challenges;
            for (uint32_t i = 0; i < A; i++) n_phases = std::max(n_phases, phase_of(i) + 1u);
            if (n_phases > 1 && sharded) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_prove_phased: a sharded key (shard_world %u): one proof over several GPUs is single-phase", world);
            if (n_phases > 1 && !ph->next_phase) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_prove_phased: the key has advice columns in %u phases and next_phase is NULL", n_phases);
            for (size_t i = 0; i < (size_t)m * A && n_phases > 1; i++) if (phase_of((uint32_t)(i % A))) ph->advice_out[i] = nullptr;
        }
        chal.assign(4 * (size_t)std::max(n_chal, 1u), 0);
        g_squeezed.user.clear(); g_squeezed.rest.clear();
        g_squeezed.user.reserve(n_chal); g_squeezed.rest.reserve(8);
        for (size_t i = 0; i < (size_t)m * A; i++) if (!phase_of((uint32_t)(i % A)) && !advice[i]) return ZK_ERR_ARG;
        if (pk->transcript > 2) return ZK_ERR_ARG;
        tr.kind = (int)pk->transcript;
        // exchange buffers of a sharded proof: the caller's (e.g. two torch tensors, so that its callback can hand RCCL tensors) or the proof's own.  First thing of all:
        // from here on this rank can tell the others about a failure of its own (ShardSignal)
        if (sharded) {
            const size_t most_cols = std::max<size_t>({pk->n_advice, 2 * (size_t)L, (size_t)n_sets + L, n_pieces, 1});
            const size_t need = std::max(qu.slots * qu.unit_rows * 32, most_cols * 128);
            if (pk->xchg_send && pk->xchg_recv) { if (pk->xchg_cap < need) return ZK_ERR_LIMIT; sig.xsend = pk->xchg_send; sig.xrecv = pk->xchg_recv; }
            else { sig.xsend = sig.xmem->get(need); sig.xrecv = sig.xmem->get(need * world); if (!sig.xsend || !sig.xrecv) return ZK_ERR_HIP; }
            for (size_t cols : {(size_t)pk->n_advice, 2 * (size_t)L, (size_t)n_sets + L, (size_t)1}) if (cols) sig.sizes.push_back(cols * 128);   // advice, permuted pairs, grand products, random poly
            sig.sizes.push_back(qu.slots * qu.unit_rows * 32);                                                                                 // the quotient's numerators
            for (size_t cols : {(size_t)n_pieces, (size_t)1, (size_t)1}) sig.sizes.push_back(cols * 128);                                        // h pieces, SHPLONK h(X) and quotient
            sig.armed = true;
        }
        for (double& v : g_phase_ms) v = 0;
        clk = PhaseClock();
        // The caller's `&mut rng` is consumed in halo2's order (plonk/prover.rs and the argument provers it calls; [3P-MEM]).  draw_schedule 1 (the only one:
        // every binding sets it): the blinding rows of every advice column, then one Blind(Fr::random) per advice column (KZG ignores the value, the stream advances); per lookup, in order:
        // permute_expression_pair's input rows then table rows, then commit_values' two Blinds; per permutation set its rows + one Blind; per lookup product its rows + one Blind; the
        // vanishing argument's n coefficients + one Blind; one Blind per h(X) piece.
        if (pk->draw_schedule != 1) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof: draw_schedule %u (1 = halo2_proofs v2023_01_20, the only schedule this build knows)", pk->draw_schedule);
        // m circuits: each per-circuit block below runs for circuit 0, 1, .., m-1 in turn (circuit c + 1's advice draws start after circuit c's Blinds); the vanishing argument once.
        // Advice phases: the advice block runs phase-major — per phase, per circuit, the rows of that phase's columns and then their Blinds.  No draw depends on a challenge,
        // so the helper thread still makes them all ahead of the phases.
        mA = (size_t)m * A; mI = (size_t)m * I; mL = (size_t)m * L; mS = (size_t)m * n_sets;
        W = (size_t)A + I + n_sets + 3 * (size_t)L;
        d_ar.resize(mA); d_bi.resize(mL); d_bt.resize(mL); d_pb.resize(mS); d_lb.resize(mL);
        for (uint32_t p = 0; p < n_phases; p++)
            for (uint32_t c = 0; c < m; c++) {
                for (uint32_t i = 0; i < A; i++) if (phase_of(i) == p) d_ar[(size_t)c * A + i] = plan(n - usable);      // (m = 1, one phase: items [0, n_advice))
                for (uint32_t i = 0; i < A; i++) if (phase_of(i) == p) plan(1);
            }
        for (size_t cl = 0; cl < mL; cl++) { d_bi[cl] = plan(bf + 1); d_bt[cl] = plan(bf + 1); plan(1); plan(1); }
        for (size_t cs = 0; cs < mS; cs++) { d_pb[cs] = plan(bf); plan(1); }
        for (size_t cl = 0; cl < mL; cl++) { d_lb[cl] = plan(bf); plan(1); }
        d_rp = plan(n);
        for (uint32_t i = 0; i < 1 + n_pieces; i++) plan(1);
        draws.start(rng, rng_user, mem.pool);
        return ZK_OK;
    }
    // one exchange: the caller's collective (the library's stream is idle when it runs), then the other ranks' failure marks — the first 32 bytes of every rank's block,
    // read from `gathered_host` when the caller has downloaded the blocks anyway
    int exchange(size_t bytes, uint64_t* gathered_host) {
        if (sig.next >= sig.sizes.size() || sig.sizes[sig.next] != bytes) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof: exchange %zu of %zu bytes is not in the proof's schedule", sig.next, bytes);
        PK(zk_dev_sync(ctx));
        const size_t ex = sig.next;
        sig.next = sig.sizes.size();                                   // (no signalling after a failure in here: the collective itself is in doubt)
        if (pk->allgather(pk->allgather_user, sig.xsend, sig.xrecv, bytes)) return pk_fail(ctx, ZK_ERR_COMM, "zk_plonk_create_proof: the caller's all-gather failed in exchange %zu", ex);
        if (gathered_host) PK(zk_dev_download(ctx, gathered_host, sig.xrecv, bytes * world));
        for (uint32_t r = 0; r < world; r++) {
            uint64_t head[4];
            if (gathered_host) memcpy(head, gathered_host + (size_t)r * bytes / 8, 32);
            else PK(zk_dev_download(ctx, head, (const char*)sig.xrecv + (size_t)r * bytes, 32));
            if (!memcmp(head, POISON, 32)) return pk_fail(ctx, ZK_ERR_COMM, "zk_plonk_create_proof: rank %u reported a failure of its own in exchange %zu", r, ex);
        }
        sig.next = ex + 1;
        return ZK_OK;
    }
    // side lane: the coefficient and extended forms of columns whose values are final, made on the helper context while this context commits them
    int early(const std::vector<Column*>& cols) {
        std::vector<void*> vals = vals_of(cols), coefs, exts;
        for (Column* c : cols) { PK(mem.take(c->coef, col_bytes)); PK(mem.take(c->ext, en * 32)); coefs.push_back(c->coef); exts.push_back(c->ext); }
        if (vals.empty()) return ZK_OK;
        PK(zk_dev_sync(ctx));                                         // the values are final: everything that wrote them ran on this context's stream
        zk_ctx* h = lane.h;
        lane.submit([h, vals, coefs, exts, col_bytes = col_bytes, k = k, ek = ek]() -> int {
            for (size_t i = 0; i < vals.size(); i++) { const int r = zk_dev_copy(h, coefs[i], vals[i], col_bytes); if (r) return r; }
            int r = zk_lagrange_to_coeff_batch_dev(h, coefs.data(), coefs.size(), k);
            if (!r) r = zk_coeff_to_extended_batch_dev(h, (const void* const*)coefs.data(), exts.data(), coefs.size(), k, ek);
            return r ? r : zk_dev_sync(h);
        });
        return ZK_OK;
    }
    // commit the value (or coefficient) forms `cols` against an SRS table and write the points to the transcript
    int commit(uint64_t table, const std::vector<void*>& cols) {
        if (cols.empty()) return ZK_OK;
        std::vector<uint64_t> out(cols.size() * 12);
        if (!sharded) PK(zk_msm_batch_dev(ctx, table, (const void* const*)cols.data(), cols.size(), n, out.data()));
        else {
            // this rank's index range of every column against its slice of the table; the 128-byte partial points of the phase travel in ONE all-gather
            std::vector<const void*> slice(cols.size());
            for (size_t i = 0; i < cols.size(); i++) slice[i] = (const char*)cols[i] + shard_lo * 32;
            const size_t bytes = cols.size() * 128;
            std::vector<uint64_t> part(cols.size() * 16), all((size_t)world * cols.size() * 16);
            PK(zk_msm_batch_partial_dev(ctx, table, slice.data(), cols.size(), n_loc, part.data()));
            PK(zk_dev_upload(ctx, sig.xsend, part.data(), bytes));
            PK(exchange(bytes, all.data()));
            PK(zk_g1_sum_xyzz_batch(all.data(), world, cols.size(), out.data()));
        }
        for (size_t i = 0; i < cols.size(); i++) tr.write_point(&out[12 * i]);
        return ZK_OK;
    }
    // ---- 1. vk, instances ----------------------------------------------------------------------------------------------------------------------------
    int instance_columns() {
        tr.common_scalar(Fr::to_mont(load32(pk->transcript_repr)));
        for (size_t c = 0; c < mI; c++) {
            const uint32_t len = instance_lens ? instance_lens[c] : 0;
            if (len > usable || (len && (!instances || !instances[c]))) return ZK_ERR_ARG;
            std::vector<Fe> col(len);
            for (uint32_t i = 0; i < len; i++) {
                const u256 canon = load32((const char*)instances[c] + 32 * i);
                if (!Fr::eq(Fr::reduce_once(canon), canon)) return ZK_ERR_ARG;          // not a canonical scalar (Fr::from_repr would refuse it)
                col[i] = Fr::to_mont(canon);
                tr.common_scalar(col[i]);
            }
            Column d;
            PK(fresh(d));
            PK(zk_dev_zero(ctx, d.val, col_bytes));
            if (len) PK(zk_dev_upload(ctx, d.val, packed(col).data(), (size_t)len * 32));
            inst.push_back(d);
        }
        return ZK_OK;
    }
    // ---- 2. advice, phase by phase: upload (host columns), blind, commit, squeeze the phase's challenges ---------------------------------------------------
    // the columns of advice phase p, circuit-major, ascending index within a circuit: halo2's commitment order ([3P-MEM] plonk/prover.rs)
    std::vector<Column*> phase_columns(uint32_t p) {
        std::vector<Column*> v;
        for (uint32_t c = 0; c < m; c++) for (uint32_t i = 0; i < A; i++) if (phase_of(i) == p) v.push_back(&adv[(size_t)c * A + i]);
        return v;
    }
    // the caller synthesises phase p with the challenges known so far (zk_phase_fn): on this thread, between two library calls — no lock of the library is held, and the
    // side lane goes on transforming the columns of the phases before
    int next_phase_columns(uint32_t p) {
        const int r = ph->next_phase(ph->next_phase_user, p, chal.data(), n_chal, ph->advice_out);
        if (r) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_prove_phased: the caller's callback returned %d for phase %u", r, p);
        for (uint32_t c = 0; c < m; c++)
            for (uint32_t i = 0; i < A; i++)
                if (phase_of(i) == p && !advice[(size_t)c * A + i])
                    return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_prove_phased: the caller's callback left advice column %u of circuit %u NULL in phase %u", i, c, p);
        return ZK_OK;
    }
    int advice_phase(uint32_t p) {
        const std::vector<Column*> cols = phase_columns(p);
        std::vector<void*> dst, bdst;
        std::vector<const void*> src, bsrc;
        for (uint32_t c = 0; c < m; c++)
            for (uint32_t i = 0; i < A; i++) {
                if (phase_of(i) != p) continue;
                const size_t at = (size_t)c * A + i;
                if (advice_on_device) adv[at].val = (void*)advice[at];
                else { PK(fresh(adv[at])); dst.push_back(adv[at].val); src.push_back(advice[at]); }
                bdst.push_back((char*)adv[at].val + usable * 32); bsrc.push_back(draws.take(d_ar[at]));
            }
        if (!dst.empty()) PK(zk_dev_upload_batch(ctx, dst.data(), src.data(), dst.size(), col_bytes));
        if (!bdst.empty()) PK(zk_dev_upload_batch(ctx, bdst.data(), bsrc.data(), bdst.size(), (n - usable) * 32));
        if (side) {
            std::vector<Column*> final_now = cols;
            if (!p) { const std::vector<Column*> in = ptrs(inst); final_now.insert(final_now.end(), in.begin(), in.end()); }
            PK(early(final_now));
        }
        PK(commit(pk->srs_g_lagrange, vals_of(cols)));                     // (one batch: the phase's commitments of all m circuits, circuit by circuit in the transcript)
        for (uint32_t i = 0; i < n_chal; i++)
            if (ph->challenge_phase[i] == p) { const Fe c = tr.squeeze(); memcpy(&chal[4 * (size_t)i], c.v, 32); }
        return ZK_OK;
    }
    int advice_columns() {
        adv.resize(mA);
        // the side lane (SideLane above): a single-GPU proof on the extended domain hands every phase's columns to the helper context as soon as their values are final
        int want = 0;
        if (!sharded && !by_cosets && zk_tune_get(ctx, "prover_side_lane", &want) == ZK_OK && (want >= 2 || (want == 1 && g_proofs_in_flight.load() <= 2))) {
            zk_ctx* h = zk_internal_helper_ctx(ctx);
            if (h) { try { lane.start(h); side = true; } catch (const std::system_error&) { side = false; } }      // no thread to be had: the proof runs in one lane, as with three proofs in flight
        }
        for (uint32_t p = 0; p < n_phases; p++) {
            if (p) PK(next_phase_columns(p));
            PK(advice_phase(p));
        }
        for (uint32_t i = 0; i < n_chal; i++) { Fe c; memcpy(c.v, &chal[4 * (size_t)i], 32); g_squeezed.user.push_back(c); }
        return ZK_OK;
    }
    // one lookup expression of circuit c, compressed with theta (a ZKQ1 program of its own over the circuit's value forms)
    int compress(uint32_t c, uint64_t prog, void*& out) {
        const void* anycol = pk->n_fixed ? pk->fixed_values[0] : (A ? adv[(size_t)c * A].val : nullptr);
        std::vector<const void*> a_vals, i_vals;
        for (uint32_t i = 0; i < A; i++) a_vals.push_back(adv[(size_t)c * A + i].val);
        for (uint32_t i = 0; i < I; i++) i_vals.push_back(inst[(size_t)c * I + i].val);
        PK(mem.take(out, col_bytes));
        zk_quotient_args a;
        ZK_STRUCT_INIT(a);
        a.fixed = pk->fixed_values; a.advice = a_vals.data(); a.instance = i_vals.data();
        a.l0 = a.l_last = a.l_active_row = anycol;
        a.beta = a.gamma = a.y = one.v; a.theta = theta.v; a.challenges = challenges();
        a.out = out;
        return zk_quotient_run_dev(ctx, prog, &a);
    }
    // ---- 3. theta; lookups: compress, permute, commit ---------------------------------------------------------------------------------------------------
    int lookups() {
        theta = squeeze_noted(tr);
        cin.resize(mL); ctab.resize(mL); pin.resize(mL); ptab.resize(mL);
        std::map<std::pair<uint32_t, uint32_t>, void*> table_cache;     // (circuit, table key): a table expression may read the circuit's own columns
        for (uint32_t c = 0; c < m; c++)
            for (uint32_t l = 0; l < L; l++) {
                const size_t cl = (size_t)c * L + l;
                auto it = table_cache.find({c, pk->lookup_table_key[l]});
                if (it == table_cache.end()) { void* t = nullptr; PK(compress(c, pk->lookup_table_programs[l], t)); it = table_cache.emplace(std::make_pair(c, pk->lookup_table_key[l]), t).first; }
                PK(compress(c, pk->lookup_input_programs[l], cin[cl]));
                ctab[cl] = it->second;
            }
        if (!mL) return ZK_OK;
        const std::vector<uint64_t> bi = drawn(d_bi, bf + 1), bt = drawn(d_bt, bf + 1);
        std::vector<Column*> flat;
        for (size_t cl = 0; cl < mL; cl++) { PK(fresh(pin[cl])); PK(fresh(ptab[cl])); flat.push_back(&pin[cl]); flat.push_back(&ptab[cl]); }
        const std::vector<void*> pi = vals_of(ptrs(pin)), pt = vals_of(ptrs(ptab));
        PK(zk_lookup_permute_batch_dev(ctx, (const void* const*)cin.data(), (const void* const*)ctab.data(), mL, k, bf, bi.data(), bt.data(), pi.data(), pt.data()));
        if (side) PK(early(flat));
        return commit(pk->srs_g_lagrange, vals_of(flat));
    }
    // ---- 4. beta, gamma; grand products -------------------------------------------------------------------------------------------------------------------
    int grand_products() {
        beta = squeeze_noted(tr); gamma = squeeze_noted(tr);
        zs.resize(mS); lzs.resize(mL);
        if (n_sets) {
            std::vector<const void*> vals((size_t)m * pk->n_perm_columns);
            for (uint32_t c = 0; c < m; c++)
                for (uint32_t j = 0; j < pk->n_perm_columns; j++) {
                    const uint32_t ty = pk->perm_columns[2 * j], ix = pk->perm_columns[2 * j + 1];
                    vals[(size_t)c * pk->n_perm_columns + j] = ty == 0 ? adv[(size_t)c * A + ix].val : ty == 1 ? pk->fixed_values[ix] : inst[(size_t)c * I + ix].val;
                }
            const std::vector<uint64_t> blind = drawn(d_pb, bf);
            for (Column& z : zs) PK(fresh(z));
            PK(zk_internal_permutation_products(ctx, vals.data(), pk->sigma_values, pk->n_perm_columns, m, chunk, k, beta.v, gamma.v, blind.data(), bf, vals_of(ptrs(zs)).data()));
        }
        if (mL) {
            std::vector<const void*> quads;
            for (size_t cl = 0; cl < mL; cl++) { quads.push_back(cin[cl]); quads.push_back(ctab[cl]); quads.push_back(pin[cl].val); quads.push_back(ptab[cl].val); }
            const std::vector<uint64_t> blind = drawn(d_lb, bf);
            for (Column& z : lzs) PK(fresh(z));
            PK(zk_lookup_product_batch_dev(ctx, quads.data(), mL, k, beta.v, gamma.v, blind.data(), bf, vals_of(ptrs(lzs)).data()));
        }
        const std::vector<Column*> both = ptrs(zs, lzs);              // every circuit's permutation products, then every circuit's lookup products (halo2's two loops)
        if (side) PK(early(both));
        return commit(pk->srs_g_lagrange, vals_of(both));
    }
    // ---- 5. vanishing argument: random polynomial ------------------------------------------------------------------------------------------------------------
    int random_polynomial() {
        PK(mem.take(random_poly, col_bytes));
        PK(zk_dev_upload(ctx, random_poly, draws.take(d_rp), col_bytes));
        return commit(pk->srs_g, {random_poly});
    }
    // The one quotient call.  `cols`: circuit c's block of W columns, extended or on one coset; the key's columns of the whole domain (coset = UINT32_MAX) or entry
    // `key_at` of the key's coset arrays; `rows`: a unit's row range of the coset, or null for all rows; `part`: 0 = the whole program, 1 / 2 = the high / low part of
    // the degree split.  Circuit 0 writes `out`; a later circuit accumulates into it (halo2's fold across circuits: evaluate_h keeps `values` from one circuit to the
    // next): out <- out * y^E + N_c, so the output ends as sum_c y^(E (m - 1 - c)) N_c — in the same launches, one read of out more each.
    int quotient_run(void* const* cols, uint32_t coset, size_t key_at, const QuotUnits::Unit* rows, uint32_t part, uint32_t c, void* out) {
        const bool whole = coset == UINT32_MAX;
        std::vector<const void*> e_in, e_tab;
        for (uint32_t l = 0; l < L; l++) { e_in.push_back(cols[A + I + n_sets + L + 2 * l]); e_tab.push_back(cols[A + I + n_sets + L + 2 * l + 1]); }
        zk_quotient_args a;
        ZK_STRUCT_INIT(a);
        a.advice = (const void* const*)cols; a.instance = (const void* const*)cols + A;
        a.perm_products = (const void* const*)cols + A + I; a.n_sets = n_sets;
        a.lookup_product = (const void* const*)cols + A + I + n_sets; a.lookup_input = e_in.data(); a.lookup_table = e_tab.data();
        a.challenges = challenges(); a.beta = beta.v; a.gamma = gamma.v; a.theta = theta.v; a.y = y.v;
        a.fixed = whole ? pk->fixed_cosets : pk->coset_fixed + key_at * pk->n_fixed;
        a.perm_cosets = whole ? pk->sigma_cosets : pk->coset_sigma + key_at * pk->n_perm_columns;
        a.l0 = whole ? pk->l0 : pk->coset_l[3 * key_at]; a.l_last = whole ? pk->l_last : pk->coset_l[3 * key_at + 1]; a.l_active_row = whole ? pk->l_active_row : pk->coset_l[3 * key_at + 2];
        a.out = out;
        if (c) return zk_quotient_run_acc_dev(ctx, pk->program, &a, coset, part);
        if (whole) return part == 0 ? zk_quotient_run_dev(ctx, pk->program, &a) : part == 1 ? zk_quotient_run_high_dev(ctx, pk->program, &a) : zk_quotient_run_low_dev(ctx, pk->program, &a, low_cosets);
        if (rows) return zk_quotient_run_coset_rows_dev(ctx, pk->program, &a, coset, rows->lo, rows->rows);
        return part ? zk_quotient_run_coset_part_dev(ctx, pk->program, &a, coset, part) : zk_quotient_run_coset_dev(ctx, pk->program, &a, coset);
    }
    // ---- 6. y; coefficient form; extended cosets; h(X) numerator ----------------------------------------------------------------------------------------------
    int quotient() {
        y = squeeze_noted(tr);
        // the proof's columns, one block of W per circuit in the order the quotient's arguments take them: advice, instance, permutation products, lookup products, permuted pairs
        std::vector<Column*> cols;
        for (uint32_t c = 0; c < m; c++) {
            for (uint32_t i = 0; i < A; i++) cols.push_back(&adv[(size_t)c * A + i]);
            for (uint32_t i = 0; i < I; i++) cols.push_back(&inst[(size_t)c * I + i]);
            for (uint32_t s = 0; s < n_sets; s++) cols.push_back(&zs[(size_t)c * n_sets + s]);
            for (uint32_t l = 0; l < L; l++) cols.push_back(&lzs[(size_t)c * L + l]);
            for (uint32_t l = 0; l < L; l++) { cols.push_back(&pin[(size_t)c * L + l]); cols.push_back(&ptab[(size_t)c * L + l]); }
        }
        if (side) {                                                   // the helper context has brought every column to both forms
            const int rc_side = lane.wait();
            if (rc_side) return pk_fail(ctx, rc_side, "zk_plonk_create_proof: transforms on the helper context: %s", zk_last_error(lane.h));
            // the Lagrange forms have been committed (this context, synchronous calls) and copied (the lane, waited for above): nothing reads them again.  Back to the pool now
            // rather than at the end of the proof — the lane's copies would otherwise double the columns a proof holds through its quotient phase.  Not the caller's own
            // advice_on_device columns (Column::owned).
            for (Column* c : cols) if (c->owned) mem.give_back(c->val);
            for (size_t cl = 0; cl < mL; cl++) { mem.give_back(cin[cl]); mem.give_back(ctab[cl]); }
        }
        std::vector<void*> coefs, exts;
        for (Column* c : cols) { if (!side) c->coef = c->val; coefs.push_back(c->coef); exts.push_back(c->ext); }
        if (!side) PK(zk_lagrange_to_coeff_batch_dev(ctx, coefs.data(), coefs.size(), k));
        if (!by_cosets) PK(mem.take(h_ext, en * 32));
        // Degree split (zkmi355.h, zk_quotient_program_split): the identities of degree <= 3 — about half of the sgx-shaped program's arithmetic — are evaluated on
        // low_cosets = 2 cosets only; their share of h(X) has degree below 2 n and is added to the first two pieces.  Single-GPU proofs only (a sharded proof keeps the whole program).
        int want = 0;
        if (!sharded && zk_tune_get(ctx, "quot_degree_split", &want) == ZK_OK && want) PK(zk_quotient_program_split(ctx, pk->program, &low_cosets, nullptr, nullptr));
        if (low_cosets >= n_pieces || low_cosets > qu.n_cosets) low_cosets = 0;
        numer_low.resize(low_cosets);
        if (low_cosets) {
            void* blk = nullptr;                                      // (one block: zk_quotient_run_low_dev writes the cosets back to back)
            PK(mem.take(blk, low_cosets * col_bytes));
            for (uint32_t j = 0; j < low_cosets; j++) numer_low[j] = (char*)blk + (size_t)j * col_bytes;
        }
        return by_cosets ? quotient_by_cosets(coefs) : sharded ? quotient_sharded(coefs) : quotient_whole_domain(coefs, exts);
    }
    int quotient_by_cosets(const std::vector<void*>& coefs) {
        std::vector<void*> cols(W);                                   // (circuit c's coset columns reuse circuit c - 1's buffers)
        PK(mem.take(cols, col_bytes));
        numer.resize(n_pieces);
        PK(mem.take(numer, col_bytes));
        for (uint32_t j = 0; j < n_pieces; j++)
            for (uint32_t c = 0; c < m; c++) {
                PK(zk_coeff_to_coset_batch_dev(ctx, (const void* const*)coefs.data() + (size_t)c * W, cols.data(), cols.size(), k, ek, j));
                PK(quotient_run(cols.data(), j, j, nullptr, low_cosets ? 1 : 0, c, numer[j]));
                if (low_cosets && j < low_cosets) PK(quotient_run(cols.data(), j, j, nullptr, 2, c, numer_low[j]));
            }
        for (auto e : cols) mem.give_back(e);
        return ZK_OK;
    }
    // the extended domain at once: from the side lane's extended columns (every circuit's exist already), or one circuit's at a time
    int quotient_whole_domain(const std::vector<void*>& coefs, const std::vector<void*>& side_ext) {
        std::vector<void*> ext(side ? 0 : W);
        if (side) ext = side_ext;
        else PK(mem.take(ext, en * 32));
        for (uint32_t c = 0; c < m; c++) {
            void* const* ec = ext.data() + (side ? (size_t)c * W : 0);
            if (!side) PK(zk_coeff_to_extended_batch_dev(ctx, (const void* const*)coefs.data() + (size_t)c * W, ext.data(), W, k, ek));
            PK(quotient_run(ec, UINT32_MAX, 0, nullptr, low_cosets ? 1 : 0, c, h_ext));
            if (low_cosets) PK(quotient_run(ec, UINT32_MAX, 0, nullptr, 2, c, numer_low[0]));
        }
        for (auto e : ext) mem.give_back(e);
        return ZK_OK;
    }
    // this rank brings the columns to ITS cosets only (size-n NTTs), evaluates the numerator on its units straight into the send buffer; one all-gather
    // carries every rank's numerators (unit order = coset order, rows ascending: rank r's block starts at unit r * slots), then the cosets are interleaved
    int quotient_sharded(const std::vector<void*>& coefs) {
        std::vector<void*> cols(coefs.size());
        PK(mem.take(cols, col_bytes));
        int at = -1;
        for (size_t s_ = 0; s_ < qu.units.size(); s_++) {
            const QuotUnits::Unit& u = qu.units[s_];
            size_t ci = 0;
            while (qu.my_cosets[ci] != u.coset) ci++;
            if ((int)u.coset != at) { PK(zk_coeff_to_coset_batch_dev(ctx, (const void* const*)coefs.data(), cols.data(), cols.size(), k, ek, u.coset)); at = (int)u.coset; }
            PK(quotient_run(cols.data(), u.coset, ci, qu.parts == 1 ? nullptr : &u, 0, 0, (char*)sig.xsend + s_ * qu.unit_rows * 32));
        }
        if (qu.units.empty()) PK(zk_dev_zero(ctx, sig.xsend, 32));       // (more ranks than units: nothing of this rank's travels, but its block's head is read as a status)
        PK(exchange(qu.slots * qu.unit_rows * 32, nullptr));
        std::vector<const void*> srcs(qu.n_cosets);
        for (uint32_t j = 0; j < qu.n_cosets; j++) srcs[j] = (const char*)sig.xrecv + (size_t)j * col_bytes;
        PK(zk_fr_interleave_dev(ctx, srcs.data(), qu.n_cosets, n, h_ext));
        for (auto e : cols) mem.give_back(e);
        return ZK_OK;
    }
    // ---- 7. divide, back to coefficients, commit the pieces ---------------------------------------------------------------------------------------------------------
    int quotient_pieces() {
        pieces.resize(n_pieces);
        if (by_cosets) {
            PK(mem.take(pieces, col_bytes));
            PK(zk_cosets_to_pieces_dev(ctx, numer.data(), n_pieces, k, ek, pieces.data()));
            for (auto e : numer) mem.give_back(e);
        } else {
            PK(zk_divide_by_vanishing_poly_dev(ctx, h_ext, k, ek));
            PK(zk_extended_to_coeff_dev(ctx, h_ext, k, ek));
            for (uint32_t i = 0; i < n_pieces; i++) pieces[i] = (char*)h_ext + (size_t)i * col_bytes;
        }
        if (low_cosets) {                                                 // h = (the high part's pieces) + (the low part's two pieces)
            std::vector<void*> lowp(low_cosets);
            PK(mem.take(lowp, col_bytes));
            PK(zk_cosets_to_pieces_dev(ctx, numer_low.data(), low_cosets, k, ek, lowp.data()));
            const Fe ones[2] = {one, one};
            for (uint32_t i = 0; i < low_cosets; i++) {
                const void* two[2] = {pieces[i], lowp[i]};
                PK(zk_fr_lincomb_dev(ctx, two, ones, 2, n, pieces[i]));
            }
            for (auto e : lowp) mem.give_back(e);
            mem.give_back(numer_low[0]);
        }
        return commit(pk->srs_g, pieces);
    }
    // ---- 8. x; evaluations ------------------------------------------------------------------------------------------------------------------------------------------------
    // Every query is listed once, in the transcript's order — advice (per circuit), fixed, random, sigma, permutation (per circuit), lookups (per circuit), h — with its place
    // in halo2's multi-open order as `open` = (section, place in it): per circuit c its advice (4c), permutation x / x_next (4c + 1), permutation x_last from the last set
    // down (4c + 2), lookup queries in lookup::Evaluated::open order (4c + 3); then fixed, sigma, h, the random polynomial once (4m ..).  multi_open sorts by it.
    int evaluations() {
        x = squeeze_noted(tr);
        Fe xn = x;
        for (uint32_t i = 0; i < k; i++) xn = Fr::sqr(xn);
        Fe omega;
        {
            const uint64_t rl[4] = BN254_FR_ROOT_OF_UNITY_M;
            for (int i = 0; i < 8; i++) omega.v[i] = (uint32_t)(rl[i >> 1] >> (32 * (i & 1)));
            for (uint32_t i = k; i < 28; i++) omega = Fr::sqr(omega);
        }
        const Fe omega_inv = Fr::inv(omega);
        auto rot = [&](int32_t r) { return Fr::mul(x, r >= 0 ? fe_pow_u64(omega, (uint64_t)r) : fe_pow_u64(omega_inv, (uint64_t)(-(int64_t)r))); };
        PK(mem.take(h_poly, col_bytes));
        {
            std::vector<Fe> pw(n_pieces, Fr::one());
            for (uint32_t i = 1; i < n_pieces; i++) pw[i] = Fr::mul(pw[i - 1], xn);
            PK(zk_fr_lincomb_dev(ctx, (const void* const*)pieces.data(), packed(pw).data(), n_pieces, n, h_poly));
        }
        const Fe x_last = rot(-(int32_t)(bf + 1)), x_next = rot(1), x_prev = rot(-1);
        auto add = [&](const void* poly, const Fe& point, uint64_t section, uint64_t place) { q.push_back({poly, point, Fr::zero(), section << 32 | place}); };
        const uint64_t once = 4 * (uint64_t)m;
        for (uint32_t c = 0; c < m; c++)
            for (uint32_t i = 0; i < pk->n_advice_queries; i++) add(adv[(size_t)c * A + pk->advice_queries[2 * i]].coef, rot((int32_t)pk->advice_queries[2 * i + 1]), 4 * c, 0);
        for (uint32_t i = 0; i < pk->n_fixed_queries; i++) add(pk->fixed_polys[pk->fixed_queries[2 * i]], rot((int32_t)pk->fixed_queries[2 * i + 1]), once, 0);
        add(random_poly, x, once + 3, 0);
        for (uint32_t j = 0; j < pk->n_perm_columns; j++) add(pk->sigma_polys[j], x, once + 1, 0);
        for (size_t cs = 0; cs < mS; cs++) {
            const uint64_t c = cs / n_sets, s = cs % n_sets;
            add(zs[cs].coef, x, 4 * c + 1, 0);
            add(zs[cs].coef, x_next, 4 * c + 1, 0);
            if (s + 1 < n_sets) add(zs[cs].coef, x_last, 4 * c + 2, n_sets - s);
        }
        for (size_t cl = 0; cl < mL; cl++) {
            const uint64_t c = cl / L, l = cl % L;
            add(lzs[cl].coef, x, 4 * c + 3, 5 * l); add(lzs[cl].coef, x_next, 4 * c + 3, 5 * l + 4);
            add(pin[cl].coef, x, 4 * c + 3, 5 * l + 1); add(pin[cl].coef, x_prev, 4 * c + 3, 5 * l + 3);
            add(ptab[cl].coef, x, 4 * c + 3, 5 * l + 2);
        }
        add(h_poly, x, once + 2, 0);
        std::vector<const void*> polys;
        std::vector<Fe> pts;
        for (const Query& e : q) { polys.push_back(e.poly); pts.push_back(e.point); }
        std::vector<uint64_t> ev(q.size() * 4);
        PK(zk_eval_polynomial_batch_dev(ctx, polys.data(), q.size(), n, packed(pts).data(), ev.data()));
        for (size_t i = 0; i < q.size(); i++) q[i].eval = load32(&ev[4 * i]);
        for (size_t i = 0; i + 1 < q.size(); i++) tr.write_scalar(q[i].eval);            // h's evaluation is the verifier's to derive
        return ZK_OK;
    }
    // ---- 9. ProverSHPLONK or ProverGWC (the context's setting): queries in the multi-open order --------------------------------------------------------------------------
    int multi_open() {
        std::stable_sort(q.begin(), q.end(), [](const Query& a, const Query& b) { return a.open < b.open; });
        if (multiopen == ZK_MULTIOPEN_GWC) return gwc_create_proof(ctx, mem, tr, q, n, [this](const std::vector<void*>& polys) { return commit(pk->srs_g, polys); });
        return shplonk_create_proof(ctx, mem, tr, q, n, [this](void* poly) { return commit(pk->srs_g, {poly}); });
    }
    // A commitment to the zero polynomial is the identity, which no transcript can absorb (Transcript::bad_point; halo2's common_point: "cannot write points at infinity
    // to the transcript").  The proof stops at the end of the phase that committed it and says which one: no byte is returned, so where inside the phase does not matter.
    int refused(const char* phase) {
        if (!tr.bad_point) return ZK_OK;
        return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof: a commitment of the %s phase is the point at infinity (the committed column is zero on every row): "
                                        "cannot write points at infinity to the transcript", phase);
    }
    // the phases in halo2's order; the laps are the nine intervals of zk_plonk_last_phase_ms
    int run() {
        PK(validate_and_plan());
        PK(instance_columns());  clk.lap(0);
        PK(advice_columns());    PK(refused("advice"));                  clk.lap(1);
        PK(lookups());           PK(refused("lookup permutation"));      clk.lap(2);
        PK(grand_products());    PK(refused("grand product"));           clk.lap(3);
        PK(random_polynomial()); PK(refused("random polynomial"));       clk.lap(4);
        PK(quotient());          clk.lap(5);
        PK(quotient_pieces());   PK(refused("quotient h(X)"));           clk.lap(6);
        PK(evaluations());       clk.lap(7);
        PK(multi_open());        PK(refused("multi-open"));              clk.lap(8);
        draws.finish();
        *proof_len = tr.out.size();
        if (!proof_out || proof_cap < tr.out.size()) return ZK_ERR_LIMIT;
        memcpy(proof_out, tr.out.data(), tr.out.size());
        return ZK_OK;
    }
};
}  // namespace

static int create_proof_entry(zk_ctx* ctx, const zk_plonk_pk_desc* pk, uint32_t m, const void* const* advice, int advice_on_device, const void* const* instances,
                              const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len, const PhaseSpec* ph = nullptr) {
    if (!ctx || !pk) return ZK_ERR_ARG;
    InFlight counted;
    Arena xmem(ctx);                                                   // (before the proof's own arena: a failing proof has returned everything else when the poisoned block travels)
    ShardSignal sig;
    sig.xmem = &xmem;
    int rc;
    try { Proof proof{ctx, pk, m, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len, sig, ph}; rc = proof.run(); }
    catch (...) { rc = abi_exception(ctx, "zk_plonk_create_proof"); }   // (here rather than at the barrier below: the other ranks of a sharded proof are told first)
    if (rc != ZK_OK && rc != ZK_ERR_COMM && sig.armed && sig.next < sig.sizes.size()) {
        std::string why = zk_last_error(ctx) ? zk_last_error(ctx) : "";
        if (zk_dev_upload(ctx, sig.xsend, POISON, 32) == ZK_OK && zk_dev_sync(ctx) == ZK_OK)
            (void)pk->allgather(pk->allgather_user, sig.xsend, sig.xrecv, sig.sizes[sig.next]);
        pk_fail(ctx, rc, "%s [rank %u of a sharded proof: failure signalled to the other ranks in exchange %zu]", why.c_str(), pk->shard_rank, sig.next);
    }
    return rc;
}

extern "C" int zk_plonk_create_proof(zk_ctx* ctx, const zk_plonk_pk_desc* pk, const void* const* advice, int advice_on_device, const void* const* instances,
                                     const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len) ZK_ABI_TRY {
    return create_proof_entry(ctx, pk, 1, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len);
} ZK_ABI_CATCH(ctx)

// halo2's create_proof over a slice of circuits: one proof, one vanishing argument, one SHPLONK opening for all of them (m = 1: zk_plonk_create_proof)
extern "C" int zk_plonk_create_proof_multi(zk_ctx* ctx, const zk_plonk_pk_desc* pk, uint32_t n_circuits, const void* const* advice, int advice_on_device,
                                           const void* const* instances, const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user,
                                           void* proof_out, size_t proof_cap, size_t* proof_len) ZK_ABI_TRY {
    if (!ctx || !pk) return ZK_ERR_ARG;
    if (!n_circuits) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_create_proof_multi: n_circuits = 0");
    return create_proof_entry(ctx, pk, n_circuits, advice, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len);
} ZK_ABI_CATCH(ctx)

// zk_plonk_prove_phased (pk.hip) with the key's descriptor and phase lists: the barrier is the caller's
int zk::create_proof_phased(zk_ctx* ctx, const zk_plonk_pk_desc* pk, const PhaseSpec* ph, uint32_t n_circuits, int advice_on_device, const void* const* instances,
                            const uint32_t* instance_lens, zk_rng_fn rng, void* rng_user, void* proof_out, size_t proof_cap, size_t* proof_len) {
    if (!ctx || !pk || !ph) return ZK_ERR_ARG;
    if (!n_circuits) return pk_fail(ctx, ZK_ERR_ARG, "zk_plonk_prove_phased: n_circuits = 0");
    if (pk->n_advice && !ph->advice_out) return ZK_ERR_ARG;
    return create_proof_entry(ctx, pk, n_circuits, ph->advice_out, advice_on_device, instances, instance_lens, rng, rng_user, proof_out, proof_cap, proof_len, ph);
}

extern "C" int zk_plonk_last_challenges(void* out, size_t cap, size_t* n) ZK_ABI_TRY {
    if (!n) return ZK_ERR_ARG;
    const size_t count = g_squeezed.user.size() + g_squeezed.rest.size();
    *n = count;
    if (cap < count * 32 || (count && !out)) return ZK_ERR_LIMIT;
    size_t at = 0;
    for (const std::vector<Fe>* part : {&g_squeezed.user, &g_squeezed.rest})
        for (const Fe& c : *part) { const u256 canon = Fr::from_mont(c); memcpy((char*)out + 32 * at++, canon.v, 32); }
    return ZK_OK;
} ZK_ABI_CATCH(nullptr)

extern "C" int zk_plonk_last_phase_ms(double out[9]) ZK_ABI_TRY {
    if (!out) return ZK_ERR_ARG;
    for (int i = 0; i < 9; i++) out[i] = g_phase_ms[i];
    return ZK_OK;
} ZK_ABI_CATCH(nullptr)
extern "C" int zk_plonk_trim(zk_ctx* ctx) ZK_ABI_TRY {
    if (!ctx) return ZK_ERR_ARG;
    std::shared_ptr<Pool> p;
    {
        std::lock_guard<std::mutex> lk(g_pools_mu);
        auto it = g_pools.find(ctx);
        if (it == g_pools.end()) return ZK_OK;
        p = it->second;
        g_pools.erase(it);
    }
    std::map<size_t, std::vector<void*>> idle;
    { std::lock_guard<std::mutex> lk(p->mu); p->retired = true; idle.swap(p->free_); }      // a proof still running on this context keeps its Arena's reference: its buffers are freed as it returns them
    for (auto& kv : idle) for (void* d : kv.second) (void)zk_dev_free(ctx, d);
    zk_internal_trim_helper(ctx);                                      // the side lane's context: its transform workspaces, twiddle and coset tables (rebuilt at the next lone proof)
    return ZK_OK;
} ZK_ABI_CATCH(ctx)
