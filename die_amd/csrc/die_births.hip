// Dynamics.agents_born: the second half of _agent_lifecycle (core/env.py:256-261 is a TODO in the reference; the rules are
// DESIGN.md §6's).  After a step's deaths, parent j — the j-th slot, in slot order, that is alive with agent_food > born_threshold —
// breeds into free slot j — the j-th dead slot below n — for j < min(#parents, #free).  A deterministic compaction: three launches
// for one world or R replicas (blockIdx.y), kernel boundaries the only synchronisation, no atomics, no workgroup waits on another.
//   k_births_count  every workgroup counts the parents and the free slots of its contiguous range of slots (ballot + popcount)
//   k_births_rank   every workgroup sums the counts of the workgroups before it, ranks its slots (ballot + mbcnt inside a wave, LDS
//                   across waves) and writes the two compact lists: parents from the front of one array of `stride` words, free
//                   slots from its back (the two sets are disjoint: they never meet)
//   k_births_spawn  thread j < min writes the child into free_of_rank[j], halves parent_of_rank[j] and draws the displacement;
//                   one thread adds the number born to the step result's count
// tests/births_model.py is the numpy twin.
//
// The record (die_births_record / _batch; tests/heredity_model.py `record`): one more launch, only for a caller that asks who was
// born to whom.  The workspace still holds the two lists and the totals after the pass, both lists ascending in slot id, so
//   k_births_record every slot s < agent_stride looks itself up among the first `born` parents and the first `born` free slots (two
//                   binary searches) and writes parent_of[s] and child_of[s], -1 where it is neither — a gather, every word one writer
#include "die_common.h"
#include "die_rng.h"

#define BIRTH_BLOCK 256
#define BIRTH_WAVES (BIRTH_BLOCK / DIE_WAVE)
#define BIRTH_MAX_GROUPS 512      // workgroups per replica at most: the rank pass's sum over the workgroups before it stays short

struct BirthArgs {
    uint32_t* x;
    uint32_t* y;
    uint8_t* alive;
    float* agent_food;
    die_step_result* results;     // results[r].num_alive += born_r, or NULL
    uint32_t* ws;                 // replica r: ws + r * ws_stride words: [2 * BIRTH_MAX_GROUPS counts | 2 totals, 2 unused | stride list words]
    int64_t ws_stride;
    int64_t agent_stride;
    float threshold;
    int boundary;
    int64_t q;                    // round(born_spread * 2^32)
    uint32_t step;
    int64_t n[DIE_MAX_REPLICAS];
    uint64_t seed[DIE_MAX_REPLICAS];
};

#define BIRTH_WS_HEAD (2 * BIRTH_MAX_GROUPS + 4)

// the contiguous range of slots workgroup `blockIdx.x` covers in a world of n slots: whole chunks of BIRTH_BLOCK
__device__ __forceinline__ void birth_range(int64_t n, int64_t& lo, int64_t& hi) {
    const int64_t chunks = (n + BIRTH_BLOCK - 1) / BIRTH_BLOCK;
    const int64_t per = (chunks + gridDim.x - 1) / gridDim.x;
    lo = (int64_t)blockIdx.x * per * BIRTH_BLOCK;
    hi = lo + per * BIRTH_BLOCK;
    if (hi > n) hi = n;
    if (lo > n) lo = n;
}

__device__ __forceinline__ void birth_flags(const BirthArgs& a, int64_t base, int64_t i, int64_t hi, bool& parent, bool& freed) {
    parent = freed = false;
    if (i < hi) {
        const bool al = a.alive[base + i] != 0;
        parent = al && a.agent_food[base + i] > a.threshold;
        freed = !al;
    }
}

__device__ __forceinline__ uint32_t birth_lane_rank(unsigned long long mask) {      // set bits below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(BIRTH_BLOCK) void k_births_count(BirthArgs a) {
    __shared__ uint32_t sp[BIRTH_WAVES], sf[BIRTH_WAVES];
    const int r = blockIdx.y;
    const int64_t base = a.agent_stride * r;
    int64_t lo, hi;
    birth_range(a.n[r], lo, hi);
    uint32_t np = 0, nf = 0;                                   // wave-uniform
    for (int64_t c = lo; c < hi; c += BIRTH_BLOCK) {
        bool p, f;
        birth_flags(a, base, c + threadIdx.x, hi, p, f);
        np += (uint32_t)__popcll(__ballot(p));
        nf += (uint32_t)__popcll(__ballot(f));
    }
    const int lane = threadIdx.x & (DIE_WAVE - 1), wv = threadIdx.x / DIE_WAVE;
    if (lane == 0) { sp[wv] = np; sf[wv] = nf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tp = 0, tf = 0;
        for (int w = 0; w < BIRTH_WAVES; ++w) { tp += sp[w]; tf += sf[w]; }
        uint32_t* cnt = a.ws + a.ws_stride * r;
        cnt[2 * blockIdx.x] = tp;
        cnt[2 * blockIdx.x + 1] = tf;
    }
}

__global__ __launch_bounds__(BIRTH_BLOCK) void k_births_rank(BirthArgs a) {
    __shared__ uint32_t sp[BIRTH_WAVES], sf[BIRTH_WAVES];
    __shared__ uint32_t red[4][BIRTH_WAVES];
    const int r = blockIdx.y;
    const int64_t base = a.agent_stride * r;
    uint32_t* ws = a.ws + a.ws_stride * r;
    uint32_t* list = ws + BIRTH_WS_HEAD;
    const int lane = threadIdx.x & (DIE_WAVE - 1), wv = threadIdx.x / DIE_WAVE;
    // the counts of the workgroups before this one, and of all of them (integer sums: any order)
    uint32_t bp = 0, bf = 0, tp = 0, tf = 0;
    for (int g = threadIdx.x; g < (int)gridDim.x; g += BIRTH_BLOCK) {
        const uint32_t cp = ws[2 * g], cf = ws[2 * g + 1];
        tp += cp; tf += cf;
        if (g < (int)blockIdx.x) { bp += cp; bf += cf; }
    }
#pragma unroll
    for (int o = DIE_WAVE / 2; o > 0; o >>= 1) {
        bp += __shfl_down(bp, o, DIE_WAVE); bf += __shfl_down(bf, o, DIE_WAVE);
        tp += __shfl_down(tp, o, DIE_WAVE); tf += __shfl_down(tf, o, DIE_WAVE);
    }
    if (lane == 0) { red[0][wv] = bp; red[1][wv] = bf; red[2][wv] = tp; red[3][wv] = tf; }
    __syncthreads();
    bp = bf = tp = tf = 0;
    for (int w = 0; w < BIRTH_WAVES; ++w) { bp += red[0][w]; bf += red[1][w]; tp += red[2][w]; tf += red[3][w]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[2 * BIRTH_MAX_GROUPS] = tp; ws[2 * BIRTH_MAX_GROUPS + 1] = tf; }
    int64_t lo, hi;
    birth_range(a.n[r], lo, hi);
    const int64_t last = a.agent_stride - 1;                   // free_of_rank[j] lives at list[last - j]
    for (int64_t c = lo; c < hi; c += BIRTH_BLOCK) {
        bool p, f;
        const int64_t i = c + threadIdx.x;
        birth_flags(a, base, i, hi, p, f);
        const unsigned long long mp = __ballot(p), mf = __ballot(f);
        __syncthreads();                                       // the previous chunk's reads of sp / sf are done
        if (lane == 0) { sp[wv] = (uint32_t)__popcll(mp); sf[wv] = (uint32_t)__popcll(mf); }
        __syncthreads();
        uint32_t op = 0, of = 0, cp = 0, cf = 0;
        for (int w = 0; w < BIRTH_WAVES; ++w) {
            if (w < wv) { op += sp[w]; of += sf[w]; }
            cp += sp[w]; cf += sf[w];
        }
        if (p) list[bp + op + birth_lane_rank(mp)] = (uint32_t)i;
        if (f) list[last - (int64_t)(bf + of + birth_lane_rank(mf))] = (uint32_t)i;
        bp += cp; bf += cf;
    }
}

__global__ __launch_bounds__(BIRTH_BLOCK) void k_births_spawn(BirthArgs a) {
    const int r = blockIdx.y;
    const int64_t base = a.agent_stride * r;
    const uint32_t* ws = a.ws + a.ws_stride * r;
    const uint32_t* list = ws + BIRTH_WS_HEAD;
    const uint32_t np = ws[2 * BIRTH_MAX_GROUPS], nf = ws[2 * BIRTH_MAX_GROUPS + 1];
    const int64_t born = np < nf ? np : nf;
    const int64_t last = a.agent_stride - 1;
    const int64_t stride = (int64_t)gridDim.x * BIRTH_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * BIRTH_BLOCK + threadIdx.x; j < born; j += stride) {
        const int64_t p = list[j], f = list[last - j];
        const float food = a.agent_food[base + p];
        const float child = 0.5f * food;                       // exact; so is the difference: a pair conserves food to the bit
        const float keep = food - child;
        const die_u32x4 w = die_draw(a.seed[r], a.step, (uint64_t)p, DIE_STREAM_BIRTH);
        const int64_t ox = ((int64_t)(int32_t)w.v[0] * a.q) >> 31, oy = ((int64_t)(int32_t)w.v[1] * a.q) >> 31;
        uint32_t X = a.x[base + p], Y = a.y[base + p];
        if (a.boundary == DIE_BOUNDARY_WRAP) {                 // the move's own boundary code (die_env.hip move_claim_one)
            X += (uint32_t)ox;
            Y += (uint32_t)oy;
        } else {
            const int64_t px = (int64_t)X + ox, py = (int64_t)Y + oy;
            X = (uint32_t)(px < 0 ? 0 : (px > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : px));
            Y = (uint32_t)(py < 0 ? 0 : (py > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : py));
        }
        a.agent_food[base + p] = keep;
        a.x[base + f] = X; a.y[base + f] = Y; a.alive[base + f] = 1; a.agent_food[base + f] = child;
    }
    if (a.results && blockIdx.x == 0 && threadIdx.x == 0 && born > 0) a.results[r].num_alive += born;
}

static int64_t births_ws_words(int64_t agent_stride) {
    return (BIRTH_WS_HEAD + agent_stride + 63) & ~(int64_t)63;             // 256-byte multiples per replica
}

extern "C" int64_t die_births_workspace_bytes(int32_t replicas, int64_t agent_stride) {
    if (replicas < 1 || replicas > DIE_MAX_REPLICAS || agent_stride < 1 || agent_stride > (int64_t)DIE_OWNER_SLOT_MASK) return -1;
    return (int64_t)replicas * births_ws_words(agent_stride) * (int64_t)sizeof(uint32_t);
}

// every check, then the three launches
static int births_launch(const die_agents* a, const die_batch* b, const die_births* p, const uint64_t* seeds, die_step_result* results,
                         void* ws, int64_t ws_bytes, void* stream, const char* who) {
    DIE_REQUIRE(a && b && p && seeds && ws, "%s: null argument", who);
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas", who, DIE_MAX_REPLICAS);
    const int64_t need = die_births_workspace_bytes(b->replicas, b->agent_stride);
    DIE_REQUIRE(need > 0, "%s: bad agent stride %lld", who, (long long)b->agent_stride);
    DIE_REQUIRE(ws_bytes >= need, "%s: workspace too small (%lld < %lld: die_births_workspace_bytes)", who, (long long)ws_bytes, (long long)need);
    DIE_REQUIRE(a->x && a->y && a->alive && a->agent_food, "%s: bad agents", who);
    DIE_REQUIRE(((uintptr_t)ws & 3u) == 0, "%s: the workspace must be 4-byte aligned", who);
    if (a->slot) {
        die_set_error("%s: births match by storage order, which must be slot order (slot must be NULL: no re-sorted arrays)", who);
        return DIE_ERR_UNSUPPORTED;
    }
    if (p->boundary != DIE_BOUNDARY_WRAP && p->boundary != DIE_BOUNDARY_LIMIT) {
        die_set_error("%s: boundary %d is not representable in Q0.32", who, p->boundary);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(p->born_spread >= 0.0 && p->born_spread <= 0.5, "%s: born_spread %g outside [0, 0.5]", who, p->born_spread);
    DIE_REQUIRE(p->born_threshold == p->born_threshold, "%s: born_threshold is NaN", who);
    BirthArgs k{};
    k.x = a->x; k.y = a->y; k.alive = a->alive; k.agent_food = a->agent_food;
    k.results = results;
    k.ws = (uint32_t*)ws; k.ws_stride = births_ws_words(b->agent_stride); k.agent_stride = b->agent_stride;
    k.threshold = p->born_threshold; k.boundary = p->boundary; k.step = p->world_step;
    k.q = (int64_t)llrint(p->born_spread * 4294967296.0);
    int64_t nmax = 0;
    for (int r = 0; r < b->replicas; ++r) {
        DIE_REQUIRE(b->n[r] >= 1 && b->n[r] <= b->agent_stride, "%s: replica %d has %lld agents (stride %lld)", who, r, (long long)b->n[r],
                    (long long)b->agent_stride);
        k.n[r] = b->n[r];
        k.seed[r] = seeds[r];
        if (b->n[r] > nmax) nmax = b->n[r];
    }
    const int64_t chunks = (nmax + BIRTH_BLOCK - 1) / BIRTH_BLOCK;
    const dim3 grid((unsigned)(chunks < BIRTH_MAX_GROUPS ? chunks : BIRTH_MAX_GROUPS), (unsigned)b->replicas);
    const int64_t half = (nmax / 2 + BIRTH_BLOCK - 1) / BIRTH_BLOCK;       // parents and free slots are disjoint: at most n / 2 pairs
    const dim3 sgrid((unsigned)(half < 1 ? 1 : (half < 4096 ? half : 4096)), (unsigned)b->replicas);
    hipStream_t s = (hipStream_t)stream;
    k_births_count<<<grid, BIRTH_BLOCK, 0, s>>>(k);
    DIE_CHECK_LAUNCH(who);
    k_births_rank<<<grid, BIRTH_BLOCK, 0, s>>>(k);
    DIE_CHECK_LAUNCH(who);
    k_births_spawn<<<sgrid, BIRTH_BLOCK, 0, s>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_agent_births(const die_agents* a, const die_births* p, uint64_t world_seed, die_step_result* result, void* ws,
                                int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(a && p && ws, "die_agent_births: null argument");
    DIE_REQUIRE(a->N >= 1 && a->N <= (int64_t)DIE_OWNER_SLOT_MASK, "die_agent_births: %lld slots (1..%u)", (long long)a->N, DIE_OWNER_SLOT_MASK);
    die_batch b{};
    b.replicas = 1; b.agent_stride = a->N; b.n[0] = a->N;
    return births_launch(a, &b, p, &world_seed, result, ws, ws_bytes, stream, "die_agent_births");
}

extern "C" int die_agent_births_batch(const die_agents* a, const die_batch* b, const die_births* p, const uint64_t* world_seeds,
                                      die_step_result* results, void* ws, int64_t ws_bytes, void* stream) {
    return births_launch(a, b, p, world_seeds, results, ws, ws_bytes, stream, "die_agent_births_batch");
}

// ---- the record of the pass that just ran ------------------------------------------------------------------------------
#define BIRTH_RECORD_MAX_GROUPS 256   // workgroups per replica at most; a thread walks its slots one grid apart

struct BirthRecordArgs {
    const uint32_t* ws;           // as BirthArgs.ws, after the pass
    int64_t ws_stride, agent_stride;
    int32_t *parent_of, *child_of;                // replica r's agent_stride words r * agent_stride on
    int64_t n[DIE_MAX_REPLICAS];
};

// rank of `s` in the ascending list key(0) < key(1) < ... < key(born - 1), or -1
template <typename Key> __device__ __forceinline__ int64_t birth_find(int64_t born, uint32_t s, Key key) {
    int64_t lo = 0, hi = born;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key(mid) < s) lo = mid + 1; else hi = mid;
    }
    return lo < born && key(lo) == s ? lo : -1;
}

__global__ __launch_bounds__(BIRTH_BLOCK) void k_births_record(BirthRecordArgs a) {
    const int r = blockIdx.y;
    const int64_t base = a.agent_stride * r, n = a.n[r];
    const uint32_t* ws = a.ws + a.ws_stride * r;
    const uint32_t* list = ws + BIRTH_WS_HEAD;
    const uint32_t np = ws[2 * BIRTH_MAX_GROUPS], nf = ws[2 * BIRTH_MAX_GROUPS + 1];
    int64_t born = np < nf ? np : nf;
    if (born > n / 2) born = n / 2;                            // (what a pass leaves never exceeds it: no index leaves the lists)
    const int64_t last = a.agent_stride - 1;
    const int64_t stride = (int64_t)gridDim.x * BIRTH_BLOCK;
    for (int64_t s = (int64_t)blockIdx.x * BIRTH_BLOCK + threadIdx.x; s < a.agent_stride; s += stride) {
        int32_t parent = -1, child = -1;
        if (s < n) {
            const int64_t jp = birth_find(born, (uint32_t)s, [&](int64_t j) { return list[j]; });
            const int64_t jf = jp >= 0 ? -1 : birth_find(born, (uint32_t)s, [&](int64_t j) { return list[last - j]; });
            if (jp >= 0 && (int64_t)list[last - jp] < n) child = (int32_t)list[last - jp];
            if (jf >= 0 && (int64_t)list[jf] < n) parent = (int32_t)list[jf];
        }
        a.parent_of[base + s] = parent;
        a.child_of[base + s] = child;
    }
}

static int births_record_launch(const die_batch* b, const void* ws, int64_t ws_bytes, int32_t* parent_of, int32_t* child_of, void* stream,
                                const char* who) {
    DIE_REQUIRE(b && ws && parent_of && child_of, "%s: null argument", who);
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas", who, DIE_MAX_REPLICAS);
    const int64_t need = die_births_workspace_bytes(b->replicas, b->agent_stride);
    DIE_REQUIRE(need > 0, "%s: bad agent stride %lld", who, (long long)b->agent_stride);
    DIE_REQUIRE(ws_bytes >= need, "%s: workspace too small (%lld < %lld: die_births_workspace_bytes)", who, (long long)ws_bytes, (long long)need);
    DIE_REQUIRE(((uintptr_t)ws & 3u) == 0, "%s: the workspace must be 4-byte aligned", who);
    const int64_t out_bytes = (int64_t)b->replicas * b->agent_stride * 4;
    DIE_REQUIRE(!die_ranges_overlap(parent_of, out_bytes, child_of, out_bytes), "%s: parent_of overlaps child_of", who);
    DIE_REQUIRE(!die_ranges_overlap(parent_of, out_bytes, ws, need) && !die_ranges_overlap(child_of, out_bytes, ws, need),
                "%s: an output overlaps the workspace", who);
    BirthRecordArgs k{};
    k.ws = (const uint32_t*)ws; k.ws_stride = births_ws_words(b->agent_stride); k.agent_stride = b->agent_stride;
    k.parent_of = parent_of; k.child_of = child_of;
    for (int r = 0; r < b->replicas; ++r) {
        DIE_REQUIRE(b->n[r] >= 1 && b->n[r] <= b->agent_stride, "%s: replica %d has %lld agents (stride %lld)", who, r, (long long)b->n[r],
                    (long long)b->agent_stride);
        k.n[r] = b->n[r];
    }
    const int64_t chunks = (b->agent_stride + BIRTH_BLOCK - 1) / BIRTH_BLOCK;
    const dim3 grid((unsigned)(chunks < BIRTH_RECORD_MAX_GROUPS ? chunks : BIRTH_RECORD_MAX_GROUPS), (unsigned)b->replicas);
    k_births_record<<<grid, BIRTH_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_births_record(int64_t n_slots, const void* ws, int64_t ws_bytes, int32_t* parent_of, int32_t* child_of, void* stream) {
    DIE_REQUIRE(n_slots >= 1 && n_slots <= (int64_t)DIE_OWNER_SLOT_MASK, "die_births_record: %lld slots (1..%u)", (long long)n_slots,
                DIE_OWNER_SLOT_MASK);
    die_batch b{};
    b.replicas = 1; b.agent_stride = n_slots; b.n[0] = n_slots;
    return births_record_launch(&b, ws, ws_bytes, parent_of, child_of, stream, "die_births_record");
}

extern "C" int die_births_record_batch(const die_batch* b, const void* ws, int64_t ws_bytes, int32_t* parent_of, int32_t* child_of,
                                       void* stream) {
    return births_record_launch(b, ws, ws_bytes, parent_of, child_of, stream, "die_births_record_batch");
}
