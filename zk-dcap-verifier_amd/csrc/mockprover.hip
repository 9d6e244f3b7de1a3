// MockProver::verify on the device — halo2_proofs src/dev.rs, the witness check the reference runs before it proves
// (`MockProver::run(k, &circuit, vec![]).unwrap().assert_satisfied()`, circuits/src/sgx_dcap_verifier.rs:790-794).  The specification is
// zk-dcap-verifier_amd/plonk/dev.py's MockProver.verify: the same failures, in the same order (include/zkmi355.h, zk_mock_prover_verify).
//
// One implementation serves both entry points.  zk_mock_prover_open builds a MockSession - everything that depends on the circuit alone - and files it
// under a handle; zk_mock_prover_check runs mp_check on it.  zk_mock_prover_verify(_phased) validates with the same mp_validate, builds a MockSession on its stack
// with the same mp_build, runs the same mp_check on it and lets it go.  They differ in two choices, named in MockPlan and fixed when the session is built: how the
// copy pass reads the mapping (edges reduced once, or the dense planes) and whether fixed-only lookup tables are sorted once for the session.
//
// Four passes over the rows, each a HIP kernel:
//   1. copies (first: a mapping out of range is an argument error): dense plan, one gather-compare over the n_perm_columns x 2^k copy mapping (values fully reduced);
//      edge plan, one compare per cell the mapping moves.  Mismatches compacted.
//   2. gates, detection: the Evaluator blob's custom gates alone, compiled at extended_k = k (quotient_program_load_gates), fold every gate polynomial of a row
//      in a random r - Horner, as evaluate_h folds them in y - on the existing interpreter; rows < u whose value is non-zero are compacted into an ascending list.
//      A failing row folds to zero only if r is a root of the non-zero polynomial sum_i g_i(row) X^(E-1-i): probability at most (E - 1) / |Fr| <= E / |Fr| per
//      row, E = the number of gate polynomials.
//   3. gates, attribution: the same program on the listed rows only, one bit per polynomial (quotient_run's row-list mode; the zero test runs on each fully
//      reduced value, so it is exact) - failing rows x polynomials of work, whatever 2^k is, and exact counts when every row fails.
//   4. lookups: input and table tuples theta-compressed by the blobs' own expression programs (as the prover compresses them), theta random; the rows < u of
//      every distinct table blob sorted (bitonic network, full 256-bit order), every input row < u binary-searched, misses compacted.  Two different tuples of m
//      expressions compress to the same value with probability at most (m - 1) / |Fr| - the bound halo2's lookup argument itself rests on.
// Compaction (mp_compact): a 64-bit __ballot per wave and its popcount, a count per workgroup, one scan over the workgroups and a scatter - positions follow the
// element order, no arrival-order atomics, so every list is deterministic.  The records and the counts are assembled on the host from the lists.
#include "ctx.h"
#include "quotient.h"
#include <algorithm>
#include <atomic>
#include <list>
#include <random>
#include <string>

namespace zk {
int quotient_program_load(zk_ctx* ctx, const void* blob, size_t len, uint64_t* prog);
int quotient_program_release(zk_ctx* ctx, uint64_t prog);

namespace {
constexpr uint32_t MP_T = 256, MP_E = 8, MP_TILE = MP_T * MP_E, MP_WAVES = MP_T / 64;   // compaction: a workgroup owns MP_TILE consecutive flags
constexpr uint32_t MP_LOCAL = 2 * MP_T;                                                  // bitonic steps in LDS: values per workgroup

// 64-bit ballot of the calling lane's wave (gfx950: wave64).  The emulator has no waves: there the same mask is assembled through LDS.
__device__ inline uint64_t mp_ballot(bool p, uint32_t* lds) {
#ifdef ZK_EMU
    const uint32_t tid = threadIdx.x;
    lds[tid] = p ? 1u : 0u;
    __syncthreads();
    uint64_t m = 0;
    for (uint32_t l = 0; l < 64; l++) if (lds[(tid & ~63u) + l]) m |= 1ull << l;
    __syncthreads();
    return m;
#else
    (void)lds;
    return __ballot(p);
#endif
}

ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_count_kernel(const uint8_t* flags, uint64_t count, uint32_t* tile_counts) {
    __shared__ uint32_t bl[MP_T];
    __shared__ uint32_t wc[MP_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * MP_TILE;
    uint32_t mine = 0;
    for (uint32_t e = 0; e < MP_E; e++) {
        const uint64_t i = base + (uint64_t)e * MP_T + tid;
        mine += (uint32_t)__builtin_popcountll(mp_ballot(i < count && flags[i], bl));
    }
    if (lane == 0) wc[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < MP_WAVES; w++) s += wc[w];
        tile_counts[blockIdx.x] = s;
    }
}
// exclusive scan of the n_tiles counts in place (one workgroup), the total at counts[n_tiles]
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_scan_kernel(uint32_t* counts, uint32_t n_tiles) {
    __shared__ uint32_t s[MP_T];
    const uint32_t tid = threadIdx.x, per = (n_tiles + MP_T - 1) / MP_T;
    const uint32_t lo = tid * per < n_tiles ? tid * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += counts[i];
    s[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < MP_T; d <<= 1) {
        const uint32_t v = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    uint32_t run = s[tid] - sum;
    for (uint32_t i = lo; i < hi; i++) { const uint32_t c = counts[i]; counts[i] = run; run += c; }
    if (tid == MP_T - 1) counts[n_tiles] = s[MP_T - 1];
}
// flagged index i -> out[its rank among the flagged]: tile offset + earlier rounds of the tile + earlier waves of the round + earlier lanes of the wave
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_scatter_kernel(const uint8_t* flags, uint64_t count, const uint32_t* tile_offsets, uint32_t* out) {
    __shared__ uint32_t bl[MP_T];
    __shared__ uint32_t wc[MP_E][MP_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * MP_TILE;
    uint64_t masks[MP_E];
    for (uint32_t e = 0; e < MP_E; e++) {
        const uint64_t i = base + (uint64_t)e * MP_T + tid;
        masks[e] = mp_ballot(i < count && flags[i], bl);
        if (lane == 0) wc[e][wave] = (uint32_t)__builtin_popcountll(masks[e]);
    }
    __syncthreads();
    uint32_t pos = tile_offsets[blockIdx.x];
    for (uint32_t e = 0; e < MP_E; e++) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; w++) before += wc[e][w];
        if ((masks[e] >> lane) & 1ull)
            out[pos + before + (uint32_t)__builtin_popcountll(masks[e] & ((1ull << lane) - 1ull))] = (uint32_t)(base + (uint64_t)e * MP_T + tid);
        for (uint32_t w = 0; w < MP_WAVES; w++) pos += wc[e][w];
    }
}

// gate values of the rows < u -> flags (the interpreter's output is fully reduced)
ZK_KERNEL void mp_nonzero_kernel(const void* vals, uint32_t u, uint8_t* flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < u) flags[i] = Fr::is_zero(load_u256(vals, i)) ? 0 : 1;
}

ZK_HD bool mp_less(const u256& a, const u256& b) {
    for (int w = 7; w >= 0; w--)
        if (a.v[w] != b.v[w]) return a.v[w] < b.v[w];
    return false;
}
// the rows < u of a compressed table column, padded to n = 2^k with all-ones (above every reduced value: the network sorts powers of two)
ZK_KERNEL void mp_table_init_kernel(const void* src, uint32_t u, uint32_t n, void* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u256 v;
    if (i < u) v = load_u256(src, i);
    else for (int w = 0; w < 8; w++) v.v[w] = 0xffffffffu;
    store_u256(dst, i, v);
}
// one compare-exchange step of the bitonic network over n values: stage `size` (ascending where index & size == 0), partner distance `dist` >= MP_LOCAL
ZK_KERNEL void mp_bitonic_step_kernel(void* v, uint32_t n, uint32_t size, uint32_t dist) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n / 2) return;
    const uint32_t lo = ((t & ~(dist - 1u)) << 1) | (t & (dist - 1u)), hi = lo | dist;
    const u256 a = load_u256(v, lo), b = load_u256(v, hi);
    if (mp_less(b, a) == ((lo & size) == 0)) { store_u256(v, lo, b); store_u256(v, hi, a); }
}
// the steps of stages size_lo .. size_hi whose partner distance is below 2 * blockDim.x, on tiles of 2 * blockDim.x values in LDS
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_bitonic_local_kernel(void* v, uint32_t size_lo, uint32_t size_hi) {
    __shared__ uint4 s[2 * MP_LOCAL];
    const uint32_t tid = threadIdx.x, T = blockDim.x, base = blockIdx.x * 2 * T;
    const uint4* g = reinterpret_cast<const uint4*>(v) + 2 * (size_t)base;
    for (uint32_t j = tid; j < 4 * T; j += T) s[j] = g[j];
    __syncthreads();
    for (uint32_t size = size_lo; size <= size_hi; size <<= 1) {
        for (uint32_t dist = size / 2 < T ? size / 2 : T; dist > 0; dist >>= 1) {
            const uint32_t lo = ((tid & ~(dist - 1u)) << 1) | (tid & (dist - 1u)), hi = lo | dist;
            u256 a, b;
            const uint4 a0 = s[2 * lo], a1 = s[2 * lo + 1], b0 = s[2 * hi], b1 = s[2 * hi + 1];
            a.v[0] = a0.x; a.v[1] = a0.y; a.v[2] = a0.z; a.v[3] = a0.w; a.v[4] = a1.x; a.v[5] = a1.y; a.v[6] = a1.z; a.v[7] = a1.w;
            b.v[0] = b0.x; b.v[1] = b0.y; b.v[2] = b0.z; b.v[3] = b0.w; b.v[4] = b1.x; b.v[5] = b1.y; b.v[6] = b1.z; b.v[7] = b1.w;
            if (mp_less(b, a) == (((base + lo) & size) == 0)) { s[2 * lo] = b0; s[2 * lo + 1] = b1; s[2 * hi] = a0; s[2 * hi + 1] = a1; }
            __syncthreads();
        }
    }
    uint4* o = reinterpret_cast<uint4*>(v) + 2 * (size_t)base;
    for (uint32_t j = tid; j < 4 * T; j += T) o[j] = s[j];
}
// flags[r] = input row r < u has no equal among the n = 2^k sorted table values (lower bound by halving)
ZK_KERNEL void mp_search_kernel(const void* in, const void* sorted, uint32_t k, uint32_t u, uint8_t* flags) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= u) return;
    const u256 x = load_u256(in, r);
    uint32_t pos = 0;
    for (uint32_t b = (1u << k) >> 1; b; b >>= 1)
        if (mp_less(load_u256(sorted, pos + b - 1), x)) pos += b;
    flags[r] = Fr::eq(load_u256(sorted, pos), x) ? 0 : 1;
}
// flags[j * n + row] = cell (j, row) differs from the cell the copy mapping sends it to; an entry outside the mapping's range sets *bad and is not read
ZK_KERNEL void mp_copy_kernel(const void* const* cols, const uint32_t* map_c, const uint32_t* map_r, uint32_t n_cols, uint32_t k, uint8_t* flags, uint32_t* bad) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ((uint64_t)n_cols << k)) return;
    const uint32_t j = (uint32_t)(e >> k), row = (uint32_t)e & ((1u << k) - 1u), cj = map_c[e], rj = map_r[e];
    uint8_t f = 0;
    if (cj >= n_cols || rj >= (1u << k)) atomicOr(bad, 1u);
    else if (cj != j || rj != row) f = Fr::eq(Fr::normalize(load_u256(cols[j], row)), Fr::normalize(load_u256(cols[cj], rj))) ? 0 : 1;
    flags[e] = f;
}

// ---- the copy pass of the edge plan (MockPlan::copy_edges): only the cells the mapping moves can fail, so they are listed once per circuit ----
// 256 threads per workgroup, at most tune mock_edge_wgs workgroups, the rest a grid stride (as the keygen kernels of pk.hip).
// flags[e] = the mapping sends cell e = j * 2^k + row to another cell; an entry outside the mapping's range sets *bad and is not flagged
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_edge_flag_kernel(const uint32_t* map_c, const uint32_t* map_r, uint32_t n_cols, uint32_t k, uint8_t* flags, uint32_t* bad) {
    const uint64_t cells = (uint64_t)n_cols << k, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += stride) {
        const uint32_t cj = map_c[e], rj = map_r[e];
        uint8_t f = 0;
        if (cj >= n_cols || rj >= (1u << k)) atomicOr(bad, 1u);
        else f = (((uint64_t)cj << k) | rj) != e ? 1 : 0;
        flags[e] = f;
    }
}
// edges[i] = (cell, image) of the i-th moved cell, both as column * 2^k + row (the mapping has fewer than 2^32 cells)
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_edge_gather_kernel(const uint32_t* moved, uint32_t n_edges, const uint32_t* map_c, const uint32_t* map_r, uint32_t k, uint2* edges) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_edges; i += stride) {
        const uint32_t c = moved[i];
        edges[i] = make_uint2(c, (map_c[c] << k) | map_r[c]);
    }
}
// flags[i] = the two cells of edge i differ (values fully reduced, as mp_copy_kernel compares them)
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_copy_edges_kernel(const void* const* cols, const uint2* edges, uint32_t n_edges, uint32_t k, uint8_t* flags) {
    const uint32_t stride = gridDim.x * blockDim.x, mask = (1u << k) - 1u;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_edges; i += stride) {
        const uint2 e = edges[i];
        flags[i] = Fr::eq(Fr::normalize(load_u256(cols[e.x >> k], e.x & mask)), Fr::normalize(load_u256(cols[e.y >> k], e.y & mask))) ? 0 : 1;
    }
}
// out[i] = edges[picked[i]]: the (cell, image) pairs of the failing edges a caller takes records of
ZK_KERNEL void ZK_LAUNCH_BOUNDS(256) mp_edge_pick_kernel(const uint32_t* picked, uint32_t count, const uint2* edges, uint2* out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = edges[picked[i]];
}

struct MpMem {                                   // the temporaries of zk_mock_prover_open's edge reduction (the mapping planes, their flags and counters), returned to the device when it ends (error returns included)
    std::list<DevTmp> held;
    void* get(size_t bytes) {
        held.emplace_back();
        if (hipMalloc(&held.back().p, bytes ? bytes : 32) != hipSuccess) { held.back().p = nullptr; return nullptr; }
        return held.back().p;
    }
};

int mp_oom(zk_ctx* ctx, const char* fn) { return ctx->fail(ZK_ERR_HIP, "%s: device allocation failed", fn); }

// flags[0 .. count) -> the ascending list of the flagged indices and its length.  `cnt` holds one counter per tile of `count` and one more; the list grows with the
// number of flagged indices and is kept
int mp_compact(zk_ctx* ctx, const char* fn, const uint8_t* d_flags, uint64_t count, uint32_t* cnt, DevBuf& list, uint32_t* total) {
    const uint32_t tiles = (uint32_t)((count + MP_TILE - 1) / MP_TILE);
    *total = 0;
    if (!tiles) return ZK_OK;
    ZK_LAUNCH(mp_count_kernel, tiles, MP_T, 0, ctx->stream, d_flags, count, cnt);
    ZK_CHECK_LAUNCH();
    ZK_LAUNCH(mp_scan_kernel, 1, MP_T, 0, ctx->stream, cnt, tiles);
    ZK_CHECK_LAUNCH();
    ZK_HIP(hipMemcpyAsync(total, cnt + tiles, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    if (!*total) return ZK_OK;
    if (list.ensure((size_t)*total * 4) != hipSuccess) return mp_oom(ctx, fn);
    ZK_LAUNCH(mp_scatter_kernel, tiles, MP_T, 0, ctx->stream, d_flags, count, (const uint32_t*)cnt, (uint32_t*)list.p);
    ZK_CHECK_LAUNCH();
    return ZK_OK;
}

// bitonic sort of n = 2^k values in place (ascending, full 256-bit order)
int mp_sort(zk_ctx* ctx, void* d_v, uint32_t k) {
    const uint32_t n = 1u << k, T = std::min<uint32_t>(MP_T, n / 2), L = 2 * T;
    ZK_LAUNCH(mp_bitonic_local_kernel, n / L, T, 0, ctx->stream, d_v, 2u, L);
    ZK_CHECK_LAUNCH();
    for (uint32_t size = 2 * L; size <= n; size <<= 1) {
        for (uint32_t dist = size / 2; dist >= L; dist >>= 1) {
            ZK_LAUNCH(mp_bitonic_step_kernel, (n / 2 + 255) / 256, 256, 0, ctx->stream, d_v, n, size, dist);
            ZK_CHECK_LAUNCH();
        }
        ZK_LAUNCH(mp_bitonic_local_kernel, n / L, T, 0, ctx->stream, d_v, size, size);
        ZK_CHECK_LAUNCH();
    }
    return ZK_OK;
}

u256 mp_random_nonzero(std::mt19937_64& g) {     // a uniform non-zero field element (Montgomery form or not: the same distribution)
    for (;;) {
        u256 x;
        for (int i = 0; i < 8; i += 2) { const uint64_t w = g(); x.v[i] = (uint32_t)w; x.v[i + 1] = (uint32_t)(w >> 32); }
        x.v[7] &= 0x3fffffffu;                                        // < 2^254 < 2p
        x = Fr::reduce_once(x);
        if (!Fr::is_zero(x)) return x;
    }
}

struct MpTimer {                                 // one pass under HIP events (zk_timing_enable): "mock_open"; "mock_copies" or "mock_copy_edges", "mock_gates", "mock_gate_rows", "mock_lookups"
    EvTimer t;
    MpTimer(zk_ctx* ctx, const char* label) : t(ctx, label) {}
    void done() { t.stop(); t.resolve(); }
};

}  // namespace

// The two places where the entry points differ, fixed when a session is built (mp_build); everything else below is common to them.
struct MockPlan {
    // copies.  true: the mapping is reduced once to the list of the cells it moves, a check compares one pair per edge (mp_copy_edges_kernel, timer "mock_copy_edges")
    // and takes the other cell of a record from the packed edge (mp_edge_pick_kernel).  false: the two planes stay as they are, a check uploads them and compares every
    // cell (mp_copy_kernel, timer "mock_copies", the range check included) and takes the other cell of a record from the caller's planes.
    bool copy_edges;
    // lookup tables.  true: a table that reads fixed columns and constants only is compressed with a theta of the session and sorted once, when the session is built.
    // false: no session theta is drawn; every table is compressed with the check's theta and sorted in the check.
    bool resident_tables;
};
constexpr MockPlan MP_ONE_SHOT{false, false};    // zk_mock_prover_verify(_phased): the circuit is seen once, so nothing is worth reducing or keeping
constexpr MockPlan MP_SESSION{true, true};       // zk_mock_prover_open / _check

// Everything that depends on the circuit alone: the fixed columns, the copy mapping (as edges or as planes), the compiled programs, the sorted resident tables and every
// workspace of a check.  zk_mock_prover_open files one under a handle; zk_mock_prover_verify(_phased) builds one on its stack, checks its one witness and lets it go.
struct MockSession {
    zk_ctx* ctx;
    MockPlan plan = MP_SESSION;
    uint32_t k = 0, n = 0, u = 0, F = 0, A = 0, I = 0, L = 0, M = 0, n_challenges = 0, n_polys = 0, words = 0, n_edges = 0, n_programs = 0;
    uint64_t cells = 0;
    size_t bytes = 0;                                 // device memory owned
    std::vector<void*> owned;
    std::vector<uint64_t> progs;                      // program handles of ctx this session loaded
    std::vector<uint32_t> perm_cols;
    std::vector<const void*> fx;                      // fixed columns (owned, or borrowed with values_on_device)
    std::vector<void*> inst, adv_stage;               // instance columns (refilled per check); staging for host advice (allocated by the first such check)
    void *zero_col = nullptr, *work = nullptr, *d_cp = nullptr;
    uint2* edges = nullptr;                           // plan.copy_edges
    const uint32_t *map_c = nullptr, *map_r = nullptr;   // !plan.copy_edges: the caller's planes (HOST, borrowed: such a session does not outlive the call) ...
    uint32_t *d_mc = nullptr, *d_mr = nullptr, *d_bad = nullptr;   // ... their place on the device, and the range check's flag
    uint8_t* flags = nullptr;                         // max(copy pairs, u, L * u) flags: the passes of a check use it one after the other
    uint32_t* tile_counts = nullptr;
    DevBuf copy_list, gate_list, lookup_list, gate_bits, picked;   // sized by the number of failures: grow and are kept
    uint64_t gate_prog = 0;
    struct Table { uint64_t prog; bool resident; void* sorted; };
    std::vector<Table> tables;                        // distinct table blobs, in the order of their first lookup
    std::vector<uint64_t> input_prog;                 // per lookup
    std::vector<uint32_t> table_of;                   // per lookup: index into tables
    const u256 one = Fr::one();
    u256 theta;                                       // plan.resident_tables: of the resident tables; never leaves the library
    std::mt19937_64 rng;

    explicit MockSession(zk_ctx* c) : ctx(c) {}
    MockSession(const MockSession&) = delete;
    MockSession& operator=(const MockSession&) = delete;
    void* get(size_t b) {
        void* p = nullptr;
        if (hipMalloc(&p, b ? b : 32) != hipSuccess) return nullptr;
        owned.push_back(p);
        bytes += b ? b : 32;
        return p;
    }
    ~MockSession() {
        (void)hipSetDevice(ctx->device);
        for (void* p : owned) (void)hipFree(p);
        for (DevBuf* b : {&copy_list, &gate_list, &lookup_list, &gate_bits, &picked}) b->release();
        for (uint64_t h : progs) (void)quotient_program_release(ctx, h);
    }
};

namespace {
std::atomic<uint64_t> g_mock_session_id{1};
enum class MpChallenges { Refused, Given, Evaluator };   // what mp_validate asks of the challenge count a blob declares: none (zk_mock_prover_verify); the caller's (_verify_phased); the evaluator blob's (_open)

uint32_t mp_edge_grid(zk_ctx* ctx, uint64_t count) {
    const uint64_t want = (count + MP_T - 1) / MP_T, cap = ctx->tune.mock_edge_wgs > 0 ? (uint64_t)ctx->tune.mock_edge_wgs : 1;
    return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}
// a compiled lookup program that reads fixed columns and constants only: no advice, no instance, no l_* column, no challenge, no power of X.  Read from the micro-ops
// the executors run (quotient.h); whatever this reader does not recognise makes the table per-check, which is always correct.
bool mp_reads_fixed_only(const QuotProgram& P) {
    if (P.uses_xpow || P.part_hi || P.part_lo) return false;
    for (const uint4& ins : P.code)
        for (uint32_t src : {ins.y, ins.z, ins.w}) {
            const uint32_t kind = src >> 28, pay = src & 0x0fffffffu;
            if (kind == K_COL) { const uint32_t c = pay >> 8; if (c < P.col_fixed || c >= P.col_fixed + P.n_fixed) return false; }
            else if (kind == K_CONST) { if (pay >= P.c_chal && pay < P.c_chal + P.n_challenges) return false; }
            else if (kind != K_SLOT && kind != K_ACC && kind != K_NONE) return false;
        }
    return true;
}
MockSession* mp_session(zk_ctx* ctx, uint64_t mp, const char* fn) {
    auto it = ctx->mock_sessions.find(mp);
    if (it == ctx->mock_sessions.end()) { (void)ctx->fail(ZK_ERR_ARG, "%s: unknown handle %llu (closed, or opened on another context)", fn, (unsigned long long)mp); return nullptr; }
    return it->second.get();
}

// the witness of a one-shot call, which its descriptor carries, in the form a check takes
zk_mock_witness mp_witness_of(const zk_mock_desc* d, const void* challenges, uint32_t n_challenges) {
    zk_mock_witness w;
    ZK_STRUCT_INIT(w);
    w.advice_values = d->advice_values; w.instances = d->instances; w.instance_lens = d->instance_lens; w.values_on_device = d->values_on_device;
    w.challenges = challenges; w.n_challenges = n_challenges;
    return w;
}
int mp_witness_args(zk_ctx* ctx, const char* fn, uint32_t A, uint32_t I, uint32_t n, const zk_mock_witness& w) {
    if (A && !w.advice_values) return ctx->fail(ZK_ERR_ARG, "%s: missing advice column array", fn);
    for (uint32_t i = 0; i < A; i++) if (!w.advice_values[i]) return ctx->fail(ZK_ERR_ARG, "%s: advice column %u is NULL", fn, i);
    for (uint32_t c = 0; c < I; c++) {
        const uint32_t len = w.instance_lens ? w.instance_lens[c] : 0;
        if (len > n || (len && (!w.instances || !w.instances[c]))) return ctx->fail(ZK_ERR_ARG, "%s: instance column %u: %u values", fn, c, len);
    }
    return ZK_OK;
}

// A zk_mock_desc, checked before any work for the entry point `fn` (the prefix of every message).  `witness`: advice_values, instances and instance_lens are part of
// the descriptor (the one-shot calls) or ignored (zk_mock_prover_open).  *n_challenges: in with MpChallenges::Given, out with MpChallenges::Evaluator.
int mp_validate(zk_ctx* ctx, const zk_mock_desc* d, const char* fn, MpChallenges rule, uint32_t* n_challenges, bool witness) {
    if (!d) return ctx->fail(ZK_ERR_ARG, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(zk_mock_desc))
        return ctx->fail(ZK_ERR_ARG, "%s: zk_mock_desc.struct_size %u, expected %zu (ABI version %u)", fn, d->struct_size, sizeof(zk_mock_desc), ZK_ABI_VERSION);
    const uint32_t k = d->k, F = d->n_fixed, A = d->n_advice, I = d->n_instance, L = d->n_lookups, M = d->n_perm_columns;
    if (k < 2 || k > 26 || (uint64_t)d->blinding_factors + 1 >= (1ull << k)) return ctx->fail(ZK_ERR_ARG, "%s: k = %u with %u blinding factors", fn, k, d->blinding_factors);
    const uint32_t n = 1u << k, u = n - d->blinding_factors - 1;
    if ((F && !d->fixed_values) || (L && (!d->lookup_input_zkq1 || !d->lookup_input_zkq1_len || !d->lookup_table_zkq1 || !d->lookup_table_zkq1_len)) ||
        (M && (!d->perm_columns || !d->perm_map_column || !d->perm_map_row)) || !d->evaluator_zkq1)
        return ctx->fail(ZK_ERR_ARG, "%s: missing column / program / mapping array", fn);
    for (uint32_t i = 0; i < F; i++) if (!d->fixed_values[i]) return ctx->fail(ZK_ERR_ARG, "%s: fixed column %u is NULL", fn, i);
    if (witness) {
        const int rc = mp_witness_args(ctx, fn, A, I, n, mp_witness_of(d, nullptr, 0));
        if (rc) return rc;
    }
    for (uint32_t j = 0; j < M; j++) {
        const uint32_t ty = d->perm_columns[2 * j], ix = d->perm_columns[2 * j + 1];
        if (ty > 2 || ix >= (ty == 0 ? A : ty == 1 ? F : I)) return ctx->fail(ZK_ERR_ARG, "%s: permutation column %u = (%u, %u) out of range", fn, j, ty, ix);
    }
    if (((uint64_t)M << k) >= (1ull << 32) || (uint64_t)L * u >= (1ull << 32)) return ctx->fail(ZK_ERR_LIMIT, "%s: more than 2^32 cells to check in one pass", fn);
    // every program's header: the column counts are what the column tables are built from
    auto header = [&](const void* blob, size_t len, bool evaluator, const char* what, uint32_t i) -> int {
        if (!blob || len < 48 || (len & 3)) return ctx->fail(ZK_ERR_ARG, "%s: bad %s blob %u", fn, what, i);
        uint32_t w[7];
        memcpy(w, blob, sizeof w);
        if (w[0] != 0x31514B5Au) return ctx->fail(ZK_ERR_PROGRAM, "%s: %s blob %u: bad magic", fn, what, i);
        switch (rule) {
        case MpChallenges::Refused:
            if (w[6]) return ctx->fail(ZK_ERR_PROGRAM, "%s: %s blob %u declares %u challenges (their values go to zk_mock_prover_verify_phased)", fn, what, i, w[6]);
            break;
        case MpChallenges::Given:
            if (w[6] != *n_challenges) return ctx->fail(ZK_ERR_ARG, "zk_mock_prover_verify_phased: %s blob %u declares %u challenges, the caller passed %u", what, i, w[6], *n_challenges);
            break;
        case MpChallenges::Evaluator:                                 // the evaluator's count is the circuit's, and every blob must declare the same
            if (evaluator) *n_challenges = w[6];
            if (w[6] != *n_challenges) return ctx->fail(ZK_ERR_ARG, "%s: %s blob %u declares %u challenges, the evaluator %u", fn, what, i, w[6], *n_challenges);
            if (w[6] > ZK_MAX_CHALLENGES) return ctx->fail(ZK_ERR_LIMIT, "%s: %u challenges, the quotient interpreter's constant bank is sized for %u", fn, w[6], ZK_MAX_CHALLENGES);
            break;
        }
        if (w[1] != k || (!evaluator && w[2] != k)) return ctx->fail(ZK_ERR_ARG, "%s: %s blob %u is for k = %u / extended_k = %u, not k = %u", fn, what, i, w[1], w[2], k);
        if (w[3] != F || w[4] != A || w[5] != I)
            return ctx->fail(ZK_ERR_ARG, "%s: %s blob %u has %u / %u / %u fixed / advice / instance columns, the descriptor %u / %u / %u", fn, what, i, w[3], w[4], w[5], F, A, I);
        return ZK_OK;
    };
    int rc = header(d->evaluator_zkq1, d->evaluator_zkq1_len, true, "evaluator", 0);
    for (uint32_t l = 0; l < L && !rc; l++) {
        rc = header(d->lookup_input_zkq1[l], d->lookup_input_zkq1_len[l], false, "lookup input", l);
        if (!rc) rc = header(d->lookup_table_zkq1[l], d->lookup_table_zkq1_len[l], false, "lookup table", l);
    }
    return rc;
}

// the arguments of every program a session runs: its fixed columns, the zero column for the l_* slots the programs never read, beta = gamma = 1, the work column as output
zk_quotient_args mp_args(const MockSession& S, const void* const* advice, const void* const* instance, const void* challenges, const u256* theta, const u256* y) {
    zk_quotient_args qa;
    ZK_STRUCT_INIT(qa);
    qa.fixed = S.fx.data(); qa.advice = advice; qa.instance = instance;
    qa.l0 = qa.l_last = qa.l_active_row = S.zero_col;
    qa.challenges = challenges; qa.beta = &S.one; qa.gamma = &S.one; qa.theta = theta; qa.y = y;
    qa.out = S.work;
    return qa;
}
// one table: its program compresses the tuples (with qa's theta) into the work column, the rows < u are padded to 2^k and sorted into tb.sorted
int mp_table_sort(zk_ctx* ctx, const MockSession& S, const zk_quotient_args& qa, const MockSession::Table& tb) {
    const int rc = quotient_run(ctx, tb.prog, &qa, QuotRoute{});
    if (rc) return rc;
    ZK_LAUNCH(mp_table_init_kernel, (S.n + 255) / 256, 256, 0, ctx->stream, (const void*)S.work, S.u, S.n, tb.sorted);
    ZK_CHECK_LAUNCH();
    return mp_sort(ctx, tb.sorted, S.k);
}

// the circuit of a validated descriptor into S, by `plan`; an error return leaves what S holds so far to its destructor
int mp_build(zk_ctx* ctx, const zk_mock_desc* d, const char* fn, MockPlan plan, uint32_t n_challenges, MockSession& S) {
    const uint32_t k = d->k, F = d->n_fixed, A = d->n_advice, I = d->n_instance, L = d->n_lookups, M = d->n_perm_columns;
    const uint32_t n = 1u << k, u = n - d->blinding_factors - 1;
    const size_t col_bytes = (size_t)32 << k;
    S.plan = plan; S.k = k; S.n = n; S.u = u; S.F = F; S.A = A; S.I = I; S.L = L; S.M = M; S.n_challenges = n_challenges;
    S.cells = (uint64_t)M << k;
    if (M) S.perm_cols.assign(d->perm_columns, d->perm_columns + 2 * (size_t)M);
    std::random_device rd;
    S.rng.seed(((uint64_t)rd() << 32) ^ rd());
    if (plan.resident_tables) S.theta = mp_random_nonzero(S.rng);
    hipStream_t st = ctx->stream;
    int rc;
    // ---- fixed columns, the instance columns a check refills, the zero column, the work column ------------------------------------------------------------------
    S.fx.resize(F);
    for (uint32_t i = 0; i < F; i++) {
        if (d->values_on_device) { S.fx[i] = d->fixed_values[i]; continue; }
        void* p = S.get(col_bytes);
        if (!p) return mp_oom(ctx, fn);
        ZK_HIP(hipMemcpyAsync(p, d->fixed_values[i], col_bytes, hipMemcpyHostToDevice, st));
        S.fx[i] = p;
    }
    S.inst.resize(I);
    for (uint32_t c = 0; c < I; c++) if (!(S.inst[c] = S.get(col_bytes))) return mp_oom(ctx, fn);
    S.zero_col = S.get(col_bytes);
    S.work = S.get(col_bytes);
    if (!S.zero_col || !S.work) return mp_oom(ctx, fn);
    ZK_HIP(hipMemsetAsync(S.zero_col, 0, col_bytes, st));
    ZK_HIP(hipStreamSynchronize(st));                                 // (the caller's fixed columns are on the device)

    // ---- the copy mapping -------------------------------------------------------------------------------------------------------------------------------------------
    const size_t cells = (size_t)S.cells;
    if (M && plan.copy_edges) {                                       // planes up, range check + flag, compact (cell order), gather the pairs; the planes go when `mem` does
        MpMem mem;
        uint32_t* d_mc = (uint32_t*)mem.get(cells * 4);
        uint32_t* d_mr = (uint32_t*)mem.get(cells * 4);
        uint8_t* flags = (uint8_t*)mem.get(cells);
        uint32_t* cnt = (uint32_t*)mem.get(((cells + MP_TILE - 1) / MP_TILE + 1) * 4);
        uint32_t* d_bad = (uint32_t*)mem.get(4);
        if (!d_mc || !d_mr || !flags || !cnt || !d_bad) return mp_oom(ctx, fn);
        ZK_HIP(hipMemcpyAsync(d_mc, d->perm_map_column, cells * 4, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_mr, d->perm_map_row, cells * 4, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemsetAsync(d_bad, 0, 4, st));
        ZK_LAUNCH(mp_edge_flag_kernel, mp_edge_grid(ctx, cells), MP_T, 0, st, (const uint32_t*)d_mc, (const uint32_t*)d_mr, M, k, flags, d_bad);
        ZK_CHECK_LAUNCH();
        uint32_t bad = 0;
        ZK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        if (bad) return ctx->fail(ZK_ERR_ARG, "%s: a copy-mapping entry is out of range (column >= %u or row >= 2^%u)", fn, M, k);
        rc = mp_compact(ctx, fn, flags, cells, cnt, S.copy_list, &S.n_edges);   // (the moved cells pass through the buffer of the checks' copy list)
        if (rc) return rc;
        if (S.n_edges) {
            S.edges = (uint2*)S.get((size_t)S.n_edges * sizeof(uint2));
            if (!S.edges) return mp_oom(ctx, fn);
            ZK_LAUNCH(mp_edge_gather_kernel, mp_edge_grid(ctx, S.n_edges), MP_T, 0, st, (const uint32_t*)S.copy_list.p, S.n_edges, (const uint32_t*)d_mc, (const uint32_t*)d_mr, k, S.edges);
            ZK_CHECK_LAUNCH();
            ZK_HIP(hipStreamSynchronize(st));
        }
        S.copy_list.release();
    } else if (M) {                                                   // the planes as they are: the check uploads and range-checks them
        S.map_c = d->perm_map_column; S.map_r = d->perm_map_row;
        S.d_mc = (uint32_t*)S.get(cells * 4);
        S.d_mr = (uint32_t*)S.get(cells * 4);
        S.d_bad = (uint32_t*)S.get(4);
        if (!S.d_mc || !S.d_mr || !S.d_bad) return mp_oom(ctx, fn);
    }
    if (M && !(S.d_cp = S.get((size_t)M * sizeof(void*)))) return mp_oom(ctx, fn);

    // ---- programs: the gates, and one per distinct lookup blob -----------------------------------------------------------------------------------------------
    rc = quotient_program_load_gates(ctx, d->evaluator_zkq1, d->evaluator_zkq1_len, &S.gate_prog, &S.n_polys);
    if (rc) return rc;
    if (S.gate_prog) { S.progs.push_back(S.gate_prog); S.n_programs++; }
    S.words = (S.n_polys + 31) / 32;
    std::map<std::string, uint64_t> loaded;                           // blob -> program
    auto load = [&](const void* blob, size_t len, uint64_t* h) -> int {
        const std::string key((const char*)blob, len);
        auto it = loaded.find(key);
        if (it != loaded.end()) { *h = it->second; return ZK_OK; }
        int rc_ = quotient_program_load(ctx, blob, len, h);
        if (rc_) return rc_;
        S.progs.push_back(*h);
        S.n_programs++;
        loaded.emplace(key, *h);
        return ZK_OK;
    };
    std::map<uint64_t, uint32_t> table_index;                         // table program -> index into S.tables
    S.input_prog.resize(L);
    S.table_of.resize(L);
    for (uint32_t l = 0; l < L; l++) {
        uint64_t tp = 0;
        rc = load(d->lookup_input_zkq1[l], d->lookup_input_zkq1_len[l], &S.input_prog[l]);
        if (!rc) rc = load(d->lookup_table_zkq1[l], d->lookup_table_zkq1_len[l], &tp);
        if (rc) return rc;
        auto it = table_index.find(tp);
        if (it == table_index.end()) {
            void* sorted = S.get(col_bytes);
            if (!sorted) return mp_oom(ctx, fn);
            it = table_index.emplace(tp, (uint32_t)S.tables.size()).first;
            S.tables.push_back(MockSession::Table{tp, plan.resident_tables && mp_reads_fixed_only(*ctx->programs.at(tp)), sorted});
        }
        S.table_of[l] = it->second;
    }
    // ---- resident tables: compressed with the session's theta and sorted once ------------------------------------------------------------------------------------
    if (plan.resident_tables) {
        std::vector<const void*> ad(A, S.zero_col), in(I, S.zero_col);     // (a resident program reads neither)
        std::vector<u256> no_challenges(std::max<uint32_t>(n_challenges, 1), Fr::zero());
        const zk_quotient_args qa = mp_args(S, ad.data(), in.data(), no_challenges.data(), &S.theta, &S.one);
        for (auto& tb : S.tables) {
            if (!tb.resident) continue;
            rc = mp_table_sort(ctx, S, qa, tb);
            if (rc) return rc;
        }
    }
    // ---- the workspaces of a check ----------------------------------------------------------------------------------------------------------------------------
    const uint64_t max_flags = std::max<uint64_t>(std::max<uint64_t>(plan.copy_edges ? S.n_edges : S.cells, u), (uint64_t)L * u);
    S.flags = (uint8_t*)S.get(max_flags);
    S.tile_counts = (uint32_t*)S.get(((max_flags + MP_TILE - 1) / MP_TILE + 1) * 4);
    if (!S.flags || !S.tile_counts) return mp_oom(ctx, fn);
    ZK_HIP(hipStreamSynchronize(st));
    return ZK_OK;
}

// the witness on the device: instances checked, to Montgomery form and into the session's columns; advice as given (values_on_device) or staged.  ad: the advice columns to read
int mp_intake(zk_ctx* ctx, MockSession& S, const char* fn, const zk_mock_witness& w, std::vector<const void*>& ad) {
    const size_t col_bytes = (size_t)32 << S.k;
    hipStream_t st = ctx->stream;
    const int rc = mp_witness_args(ctx, fn, S.A, S.I, S.n, w);
    if (rc) return rc;
    std::vector<u256> host_col;
    for (uint32_t c = 0; c < S.I; c++) {
        const uint32_t len = w.instance_lens ? w.instance_lens[c] : 0;
        host_col.assign(S.n, Fr::zero());
        for (uint32_t i = 0; i < len; i++) {
            u256 v;
            memcpy(&v, (const char*)w.instances[c] + 32 * (size_t)i, 32);
            if (!Fr::eq(Fr::reduce_once(v), v)) return ctx->fail(ZK_ERR_ARG, "%s: instance %u of column %u is not canonical", fn, i, c);
            host_col[i] = Fr::to_mont(v);
        }
        ZK_HIP(hipMemcpyAsync(S.inst[c], host_col.data(), col_bytes, hipMemcpyHostToDevice, st));
        ZK_HIP(hipStreamSynchronize(st));                             // (host_col is refilled for the next column)
    }
    ad.assign(w.advice_values, w.advice_values + S.A);
    if (w.values_on_device) return ZK_OK;
    while (S.adv_stage.size() < S.A) {
        void* p = S.get(col_bytes);
        if (!p) return mp_oom(ctx, fn);
        S.adv_stage.push_back(p);
    }
    for (uint32_t i = 0; i < S.A; i++) {
        ZK_HIP(hipMemcpyAsync(S.adv_stage[i], w.advice_values[i], col_bytes, hipMemcpyHostToDevice, st));
        ad[i] = S.adv_stage[i];
    }
    ZK_HIP(hipStreamSynchronize(st));                                 // (the caller's columns are not read after the call, whatever passes the circuit has)
    return ZK_OK;
}

// One witness against the circuit of S: the records of zk_mock_prover_verify (include/zkmi355.h), for either entry point.  Copies first: a mapping out of range is an
// argument error, found before the other passes run.
int mp_check(zk_ctx* ctx, MockSession& S, const char* fn, const zk_mock_witness& w, zk_mock_failure* out, size_t cap, uint64_t counts[3], size_t* n_written) {
    const uint32_t k = S.k, n = S.n, u = S.u, L = S.L, M = S.M, blk = 256;
    hipStream_t st = ctx->stream;
    std::vector<const void*> ad, in(S.inst.begin(), S.inst.end());
    int rc = mp_intake(ctx, S, fn, w, ad);
    if (rc) return rc;
    const u256 r = mp_random_nonzero(S.rng), theta = mp_random_nonzero(S.rng);
    zk_quotient_args qa = mp_args(S, ad.data(), in.data(), w.n_challenges ? w.challenges : (const void*)&S.one, &theta, &r);

    // ---- copies: one thread per edge, or per cell of the mapping; the failing ones compacted in cell order -----------------------------------------------------------
    const uint64_t n_pairs = S.plan.copy_edges ? S.n_edges : S.cells;
    uint32_t n_copy = 0;
    if (n_pairs) {
        MpTimer t(ctx, S.plan.copy_edges ? "mock_copy_edges" : "mock_copies");
        std::vector<const void*> cp(M);
        for (uint32_t j = 0; j < M; j++) {
            const uint32_t ty = S.perm_cols[2 * j], ix = S.perm_cols[2 * j + 1];
            cp[j] = ty == 0 ? ad[ix] : ty == 1 ? S.fx[ix] : in[ix];
        }
        ZK_HIP(hipMemcpyAsync(S.d_cp, cp.data(), (size_t)M * sizeof(void*), hipMemcpyHostToDevice, st));
        if (S.plan.copy_edges) {
            ZK_LAUNCH(mp_copy_edges_kernel, mp_edge_grid(ctx, S.n_edges), MP_T, 0, st, (const void* const*)S.d_cp, (const uint2*)S.edges, S.n_edges, k, S.flags);
            ZK_CHECK_LAUNCH();
        } else {
            ZK_HIP(hipMemcpyAsync(S.d_mc, S.map_c, (size_t)S.cells * 4, hipMemcpyHostToDevice, st));
            ZK_HIP(hipMemcpyAsync(S.d_mr, S.map_r, (size_t)S.cells * 4, hipMemcpyHostToDevice, st));
            ZK_HIP(hipMemsetAsync(S.d_bad, 0, 4, st));
            ZK_LAUNCH(mp_copy_kernel, (uint32_t)((S.cells + blk - 1) / blk), blk, 0, st, (const void* const*)S.d_cp, (const uint32_t*)S.d_mc, (const uint32_t*)S.d_mr, M, k, S.flags, S.d_bad);
            ZK_CHECK_LAUNCH();
            uint32_t bad = 0;
            ZK_HIP(hipMemcpyAsync(&bad, S.d_bad, 4, hipMemcpyDeviceToHost, st));
            ZK_HIP(hipStreamSynchronize(st));
            if (bad) return ctx->fail(ZK_ERR_ARG, "%s: a copy-mapping entry is out of range (column >= %u or row >= 2^%u)", fn, M, k);
        }
        rc = mp_compact(ctx, fn, S.flags, n_pairs, S.tile_counts, S.copy_list, &n_copy);
        if (rc) return rc;
        t.done();
    }

    // ---- gates: detection over every row, attribution on the failing rows ---------------------------------------------------------------------------------------------
    const uint32_t n_polys = S.n_polys, words = S.words;
    uint32_t n_rows = 0;
    std::vector<uint32_t> rows, bits;
    if (n_polys) {
        {
            MpTimer t(ctx, "mock_gates");
            rc = quotient_run(ctx, S.gate_prog, &qa, QuotRoute{});
            if (rc) return rc;
            ZK_LAUNCH(mp_nonzero_kernel, (u + blk - 1) / blk, blk, 0, st, (const void*)S.work, u, S.flags);
            ZK_CHECK_LAUNCH();
            rc = mp_compact(ctx, fn, S.flags, u, S.tile_counts, S.gate_list, &n_rows);
            if (rc) return rc;
            t.done();
        }
        if (n_rows) {
            MpTimer t(ctx, "mock_gate_rows");
            if (S.gate_bits.ensure((size_t)n_rows * words * 4) != hipSuccess) return mp_oom(ctx, fn);
            const QuotRowList rl{(const uint32_t*)S.gate_list.p, n_rows, (uint32_t*)S.gate_bits.p, words};
            QuotRoute route;
            route.rows = &rl;
            rc = quotient_run(ctx, S.gate_prog, &qa, route);
            if (rc) return rc;
            rows.resize(n_rows);
            bits.resize((size_t)n_rows * words);
            ZK_HIP(hipMemcpyAsync(rows.data(), S.gate_list.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
            ZK_HIP(hipMemcpyAsync(bits.data(), S.gate_bits.p, bits.size() * 4, hipMemcpyDeviceToHost, st));
            ZK_HIP(hipStreamSynchronize(st));
            t.done();
        }
    }

    // ---- lookups: compress, sort each table this check has to sort once (before its first lookup), search every input ------------------------------------------------
    uint32_t n_lookup = 0;
    if (L) {
        MpTimer t(ctx, "mock_lookups");
        std::vector<bool> sorted(S.tables.size(), false);
        for (uint32_t l = 0; l < L; l++) {
            const MockSession::Table& tb = S.tables[S.table_of[l]];
            // THE THETA RULE, which no test can see (the records are the same for every theta short of a collision): a table sorted in this check is compressed with the
            // theta drawn for this check - never with the session's, which earlier answers depend on - and every input is compressed with ITS TABLE's theta.
            qa.theta = tb.resident ? &S.theta : &theta;
            if (!tb.resident && !sorted[S.table_of[l]]) {
                rc = mp_table_sort(ctx, S, qa, tb);
                if (rc) return rc;
                sorted[S.table_of[l]] = true;
            }
            rc = quotient_run(ctx, S.input_prog[l], &qa, QuotRoute{});
            if (rc) return rc;
            ZK_LAUNCH(mp_search_kernel, (u + blk - 1) / blk, blk, 0, st, (const void*)S.work, (const void*)tb.sorted, k, u, S.flags + (size_t)l * u);
            ZK_CHECK_LAUNCH();
        }
        rc = mp_compact(ctx, fn, S.flags, (uint64_t)L * u, S.tile_counts, S.lookup_list, &n_lookup);
        if (rc) return rc;
        t.done();
    }

    // ---- records: gates by (row, polynomial), lookups by (lookup, row), copies by (column, row); the first `cap` of them -------------------------------------------------
    uint64_t n_gate = 0;
    for (uint32_t wd : bits) n_gate += (uint64_t)__builtin_popcount(wd);
    counts[0] = n_gate; counts[1] = n_lookup; counts[2] = n_copy;
    size_t at = 0;
    for (uint32_t i = 0; i < n_rows && at < cap; i++)
        for (uint32_t p = 0; p < n_polys && at < cap; p++)
            if ((bits[(size_t)i * words + p / 32] >> (p & 31)) & 1u) out[at++] = zk_mock_failure{0, p, rows[i], 0, 0};
    std::vector<uint32_t> idx;
    const size_t take_l = std::min<size_t>(cap - at, n_lookup);
    if (take_l) {
        idx.resize(take_l);
        ZK_HIP(hipMemcpyAsync(idx.data(), S.lookup_list.p, take_l * 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        for (uint32_t e : idx) out[at++] = zk_mock_failure{1, e / u, e % u, 0, 0};
    }
    const size_t take_c = std::min<size_t>(cap - at, n_copy);
    if (take_c && S.plan.copy_edges) {                                // the list holds edge indices: the two cells come from the packed edge
        if (S.picked.ensure(take_c * sizeof(uint2)) != hipSuccess) return mp_oom(ctx, fn);
        ZK_LAUNCH(mp_edge_pick_kernel, mp_edge_grid(ctx, take_c), MP_T, 0, st, (const uint32_t*)S.copy_list.p, (uint32_t)take_c, (const uint2*)S.edges, (uint2*)S.picked.p);
        ZK_CHECK_LAUNCH();
        std::vector<uint2> pairs(take_c);
        ZK_HIP(hipMemcpyAsync(pairs.data(), S.picked.p, take_c * sizeof(uint2), hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        for (const uint2& e : pairs) out[at++] = zk_mock_failure{2, e.x >> k, e.x & (n - 1), e.y >> k, e.y & (n - 1)};
    } else if (take_c) {                                              // the list holds cell indices: the other cell comes from the caller's planes
        idx.resize(take_c);
        ZK_HIP(hipMemcpyAsync(idx.data(), S.copy_list.p, take_c * 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        for (uint32_t e : idx) out[at++] = zk_mock_failure{2, e >> k, e & (n - 1), S.map_c[e], S.map_r[e]};
    }
    if (n_written) *n_written = at;
    return ZK_OK;
}
}  // namespace

void release_mock_sessions(zk_ctx* ctx) { ctx->mock_sessions.clear(); }

// zk_mock_prover_verify, and with `phased` zk_mock_prover_verify_phased (challenges / n_challenges: the values of the circuit's user challenges, Montgomery, fed to every
// program as they are): a session by the one-shot plan that is filed nowhere, gets no handle and ends with the call, on every return
int mock_prover_verify(zk_ctx* ctx, const zk_mock_desc* d, zk_mock_failure* out, size_t cap, uint64_t counts[3], size_t* n_written, const void* challenges,
                       uint32_t n_challenges, bool phased) {
    const char* fn = "zk_mock_prover_verify";
    if (!counts || (cap && !out)) return ctx->fail(ZK_ERR_ARG, "%s: null counts / output", fn);
    int rc = mp_validate(ctx, d, fn, phased ? MpChallenges::Given : MpChallenges::Refused, &n_challenges, true);
    if (rc) return rc;
    MockSession S(ctx);
    rc = mp_build(ctx, d, fn, MP_ONE_SHOT, n_challenges, S);
    if (rc) return rc;
    return mp_check(ctx, S, fn, mp_witness_of(d, challenges, n_challenges), out, cap, counts, n_written);
}

// ---- the session: zk_mock_prover_open / _check / _info / _close (include/zkmi355.h) -----------------------------------------------------------------------------
int mock_prover_open(zk_ctx* ctx, const zk_mock_desc* d, uint64_t* mp) {
    const char* fn = "zk_mock_prover_open";
    if (!d || !mp) return ctx->fail(ZK_ERR_ARG, "%s: null descriptor / handle pointer", fn);
    uint32_t n_challenges = 0;
    int rc = mp_validate(ctx, d, fn, MpChallenges::Evaluator, &n_challenges, false);
    if (rc) return rc;
    MpTimer timer(ctx, "mock_open");
    auto S = std::make_shared<MockSession>(ctx);                      // an error return frees what the session holds so far
    rc = mp_build(ctx, d, fn, MP_SESSION, n_challenges, *S);
    if (rc) return rc;
    timer.done();
    const uint64_t id = (0x4d50ull << 48) | g_mock_session_id.fetch_add(1);
    ctx->mock_sessions[id] = S;
    *mp = id;
    return ZK_OK;
}

int mock_prover_info(zk_ctx* ctx, uint64_t mp, zk_mock_info* info) {
    if (!info) return ctx->fail(ZK_ERR_ARG, "zk_mock_prover_info: null output");
    if (info->struct_size != sizeof(zk_mock_info))
        return ctx->fail(ZK_ERR_ARG, "zk_mock_prover_info: zk_mock_info.struct_size %u, expected %zu (ABI version %u)", info->struct_size, sizeof(zk_mock_info), ZK_ABI_VERSION);
    const MockSession* S = mp_session(ctx, mp, "zk_mock_prover_info");
    if (!S) return ZK_ERR_ARG;
    info->n_tables = (uint32_t)S->tables.size();
    info->n_resident_tables = 0;
    for (auto& t : S->tables) info->n_resident_tables += t.resident ? 1 : 0;
    info->n_programs = S->n_programs;
    info->n_edges = S->n_edges;
    info->n_cells = S->cells;
    info->device_bytes = S->bytes + S->copy_list.cap + S->gate_list.cap + S->lookup_list.cap + S->gate_bits.cap + S->picked.cap;
    return ZK_OK;
}

int mock_prover_close(zk_ctx* ctx, uint64_t mp) {
    if (!mp_session(ctx, mp, "zk_mock_prover_close")) return ZK_ERR_ARG;
    (void)hipStreamSynchronize(ctx->stream);
    ctx->mock_sessions.erase(mp);
    return ZK_OK;
}

int mock_prover_check(zk_ctx* ctx, uint64_t mp, const zk_mock_witness* w, zk_mock_failure* out, size_t cap, uint64_t counts[3], size_t* n_written) {
    const char* fn = "zk_mock_prover_check";
    if (!w) return ctx->fail(ZK_ERR_ARG, "%s: null witness", fn);
    if (w->struct_size != sizeof(zk_mock_witness))
        return ctx->fail(ZK_ERR_ARG, "%s: zk_mock_witness.struct_size %u, expected %zu (ABI version %u)", fn, w->struct_size, sizeof(zk_mock_witness), ZK_ABI_VERSION);
    if (!counts || (cap && !out)) return ctx->fail(ZK_ERR_ARG, "%s: null counts / output", fn);
    MockSession* S = mp_session(ctx, mp, fn);
    if (!S) return ZK_ERR_ARG;
    if (w->n_challenges != S->n_challenges) return ctx->fail(ZK_ERR_ARG, "%s: the circuit's blobs declare %u challenges, the caller passed %u", fn, S->n_challenges, w->n_challenges);
    if (w->n_challenges && !w->challenges) return ctx->fail(ZK_ERR_ARG, "%s: %u challenges and a null array", fn, w->n_challenges);
    return mp_check(ctx, *S, fn, *w, out, cap, counts, n_written);
}

}  // namespace zk
