// Heredity (gfx950): what a newborn receives from its parent — NeuralAutomataAgent(memory_inherit='blank' | 'copy',
// memory_mutation=a) under Dynamics(agents_born=True).  DESIGN.md §6; no reference counterpart (core/env.py:256-261 is a TODO).
// Runs after a birth pass, on its record (die_births.hip die_births_record: parent_of / child_of by slot id) and on the memory as
// this step's read-out left it — an (M, N) fp32 array by SLOT ID, rows row_stride apart; (R, M, agent_stride) for a batch.
//
//   k_memory_inherit           one thread per slot s of replica blockIdx.y; a slot with p = parent_of[s] >= 0 is a child:
//                                blank          mem[m][s] = +0
//                                copy, a == 0   mem[m][s] = mem[m][p] as a 32-bit word (negative zero, denormals, NaN payloads keep
//                                               their bits)
//                                copy, a > 0    mem[m][s] = fadd_rn(mem[m][p], fmul_rn(a, u)), u = (float)(int32)word * 2^-31 in
//                                               [-1, 1], word = word (m & 3) of die_draw(world seed, world step, p | (m >> 2) << 32,
//                                               DIE_STREAM_HEREDITY): the births' key and step on a stream of its own, one Philox
//                                               block per four channels.  Two separately rounded operations, never one fma.
//                              Every other slot is left alone.  Parents and children are disjoint sets and a parent has one child a
//                              pass, so the update is race-free in place: no word is read by one thread and written by another.
//   k_memory_inherit_backward  the adjoint, out of place, one thread per slot: a parent (c = child_of[s] >= 0) gets g[m][s] +
//                              g[m][c] (copy; one fp32 add) or g[m][s] (blank), a child +0, every other slot g[m][s] as a 32-bit
//                              word.  A gather in plain loads and stores: the additive noise has unit Jacobian, `a` does not appear.
// A record word that names a slot outside the replica (never written by die_births_record) reads as -1: nothing out of bounds.
// tests/heredity_model.py is the numpy twin.
//
// Roofline: latency.  A population of 10 x 1095 slots at M = 2 reads 44 KB of record and touches at most 88 KB of memory: the launch
// is the cost, as for the memory read-out next to it (LABBOOK §45).
#include "die_common.h"
#include "die_rng.h"

#define HEREDITY_MAX_GROUPS 256   // workgroups per replica at most; a thread walks its slots one grid apart

struct InheritArgs {
    const int32_t *parent_of, *child_of;     // replica r's words r * agent_stride on
    uint32_t* mem;                           // row m of replica r at mem + r * mem_rep + m * mem_row
    const uint32_t* grad;                    // (backward) the incoming gradient, laid out as mem; `mem` is then the output
    int64_t agent_stride, mem_row, mem_rep;
    int M, mode;
    float a;
    uint32_t step;
    int64_t n[DIE_MAX_REPLICAS];
    uint64_t seed[DIE_MAX_REPLICAS];
};

__device__ __forceinline__ int64_t inherit_link(const int32_t* link, int64_t i, int64_t n) {
    const int64_t v = link[i];
    return v >= 0 && v < n ? v : -1;
}

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_inherit(InheritArgs k) {
    const int r = blockIdx.y;
    const int64_t n = k.n[r], base = k.agent_stride * r;
    uint32_t* mem = k.mem + k.mem_rep * r;
    const int64_t stride = (int64_t)gridDim.x * DIE_BLOCK;
    for (int64_t s = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; s < n; s += stride) {
        const int64_t p = inherit_link(k.parent_of, base + s, n);
        if (p < 0 || p == s) continue;
        die_u32x4 w = {};
        for (int m = 0; m < k.M; ++m) {
            uint32_t* row = mem + k.mem_row * m;
            if (k.mode == DIE_INHERIT_BLANK) { row[s] = 0u; continue; }
            if (!(k.a > 0.f)) { row[s] = row[p]; continue; }
            if ((m & 3) == 0) w = die_draw(k.seed[r], k.step, (uint64_t)p | ((uint64_t)(m >> 2) << 32), DIE_STREAM_HEREDITY);
            const float u = (float)(int32_t)die_dropout_pick(w, (uint32_t)m) * 4.656612873077392578125e-10f;       // 2^-31: exact
            row[s] = __float_as_uint(__fadd_rn(__uint_as_float(row[p]), __fmul_rn(k.a, u)));
        }
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_inherit_backward(InheritArgs k) {
    const int r = blockIdx.y;
    const int64_t n = k.n[r], base = k.agent_stride * r;
    const uint32_t* g = k.grad + k.mem_rep * r;
    uint32_t* out = k.mem + k.mem_rep * r;
    const int64_t stride = (int64_t)gridDim.x * DIE_BLOCK;
    for (int64_t s = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; s < k.agent_stride; s += stride) {
        const bool inside = s < n;                               // (a replica's padding slots pass their gradient through)
        const int64_t p = inside ? inherit_link(k.parent_of, base + s, n) : -1;
        const int64_t c = inside ? inherit_link(k.child_of, base + s, n) : -1;
        for (int m = 0; m < k.M; ++m) {
            const uint32_t* row = g + k.mem_row * m;
            uint32_t v = row[s];
            if (p >= 0) v = 0u;
            else if (c >= 0 && k.mode == DIE_INHERIT_COPY) v = __float_as_uint(__fadd_rn(__uint_as_float(v), __uint_as_float(row[c])));
            out[k.mem_row * m + s] = v;
        }
    }
}

// ---- every check, then the one launch --------------------------------------------------------------------------------------
static int inherit_check(int32_t mode, int32_t M, const die_batch* b, int64_t row_stride, const int32_t* parent_of, const int32_t* child_of,
                         const float* mem, const float* grad, const char* who) {
    DIE_REQUIRE(mode == DIE_INHERIT_BLANK || mode == DIE_INHERIT_COPY, "%s: mode %d is neither DIE_INHERIT_BLANK nor DIE_INHERIT_COPY", who, mode);
    DIE_REQUIRE(M >= 1 && M <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who, M, DIE_MEMORY_MAX_CHANNELS);
    const int rc = die_batch_check(b, -1, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(row_stride >= b->agent_stride, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride,
                (long long)b->agent_stride);
    const int64_t R = b->replicas;
    const int64_t mem_bytes = ((R * M - 1) * row_stride + b->agent_stride) * 4, link_bytes = R * b->agent_stride * 4;
    DIE_REQUIRE(!die_ranges_overlap(mem, mem_bytes, parent_of, link_bytes) && !die_ranges_overlap(mem, mem_bytes, child_of, link_bytes),
                "%s: the %s overlaps the record", who, grad ? "output" : "memory");
    DIE_REQUIRE(!die_ranges_overlap(mem, mem_bytes, grad, mem_bytes), "%s: the output overlaps the incoming gradient", who);
    return DIE_OK;
}

static int inherit_launch(bool backward, int32_t mode, int32_t M, float a, const die_batch* b, int64_t row_stride, const int32_t* parent_of,
                          const int32_t* child_of, float* mem, const float* grad, const uint64_t* seeds, uint32_t step, void* stream,
                          const char* who) {
    InheritArgs k{};
    k.parent_of = parent_of; k.child_of = child_of; k.mem = (uint32_t*)mem; k.grad = (const uint32_t*)grad;
    k.agent_stride = b->agent_stride; k.mem_row = row_stride; k.mem_rep = (int64_t)M * row_stride;
    k.M = M; k.mode = mode; k.a = a; k.step = step;
    const int64_t nmax = die_replica_counts(k.n, b->n, b->replicas);
    for (int r = 0; r < b->replicas; ++r) k.seed[r] = seeds ? seeds[r] : 0;
    const int64_t slots = backward ? b->agent_stride : nmax;
    if (slots == 0) return DIE_OK;                           // no slot anywhere: nothing to write
    const int64_t chunks = (slots + DIE_BLOCK - 1) / DIE_BLOCK;
    const dim3 grid((unsigned)(chunks < HEREDITY_MAX_GROUPS ? chunks : HEREDITY_MAX_GROUPS), (unsigned)b->replicas);
    if (backward) k_memory_inherit_backward<<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    else k_memory_inherit<<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

static int inherit_forward(int32_t mode, float a, int32_t M, const die_batch* b, int64_t row_stride, const int32_t* parent_of, float* mem,
                           const uint64_t* seeds, uint32_t step, void* stream, const char* who) {
    DIE_REQUIRE(b && parent_of && mem && seeds, "%s: null argument", who);
    const int rc = inherit_check(mode, M, b, row_stride, parent_of, nullptr, mem, nullptr, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(a >= 0.f && a <= 3.4028234663852886e38f, "%s: mutation %g is not a finite number >= 0", who, (double)a);
    DIE_REQUIRE(mode == DIE_INHERIT_COPY || a == 0.f, "%s: a mutation (%g) needs DIE_INHERIT_COPY", who, (double)a);
    return inherit_launch(false, mode, M, a, b, row_stride, parent_of, nullptr, mem, nullptr, seeds, step, stream, who);
}

static int inherit_backward(int32_t mode, int32_t M, const die_batch* b, int64_t row_stride, const int32_t* parent_of, const int32_t* child_of,
                            const float* grad, float* out, void* stream, const char* who) {
    DIE_REQUIRE(b && parent_of && child_of && grad && out, "%s: null argument", who);
    const int rc = inherit_check(mode, M, b, row_stride, parent_of, child_of, out, grad, who);
    if (rc != DIE_OK) return rc;
    return inherit_launch(true, mode, M, 0.f, b, row_stride, parent_of, child_of, out, grad, nullptr, 0u, stream, who);
}

static int inherit_one(int64_t n_slots, die_batch* b, const char* who) {
    DIE_REQUIRE(n_slots >= 1 && n_slots <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: %lld slots outside 1..%lld", who, (long long)n_slots,
                (long long)DIE_OWNER_SLOT_MASK - 1);
    b->replicas = 1; b->agent_stride = n_slots; b->n[0] = n_slots;
    return DIE_OK;
}

extern "C" int die_memory_inherit(int32_t mode, float mutation, int32_t memory_channels, int64_t n_slots, const int32_t* parent_of,
                                  float* memory, int64_t row_stride, uint64_t world_seed, uint32_t world_step, void* stream) {
    const char* who = "die_memory_inherit";
    die_batch b{};
    const int rc = inherit_one(n_slots, &b, who);
    if (rc != DIE_OK) return rc;
    return inherit_forward(mode, mutation, memory_channels, &b, row_stride, parent_of, memory, &world_seed, world_step, stream, who);
}

extern "C" int die_memory_inherit_batch(int32_t mode, float mutation, int32_t memory_channels, const die_batch* b, const int32_t* parent_of,
                                        float* memory, const uint64_t* world_seeds, uint32_t world_step, void* stream) {
    const char* who = "die_memory_inherit_batch";
    DIE_REQUIRE(b, "%s: null argument", who);
    return inherit_forward(mode, mutation, memory_channels, b, b->agent_stride, parent_of, memory, world_seeds, world_step, stream, who);
}

extern "C" int die_memory_inherit_backward(int32_t mode, int32_t memory_channels, int64_t n_slots, const int32_t* parent_of,
                                           const int32_t* child_of, const float* grad, float* grad_memory, int64_t row_stride, void* stream) {
    const char* who = "die_memory_inherit_backward";
    die_batch b{};
    const int rc = inherit_one(n_slots, &b, who);
    if (rc != DIE_OK) return rc;
    return inherit_backward(mode, memory_channels, &b, row_stride, parent_of, child_of, grad, grad_memory, stream, who);
}

extern "C" int die_memory_inherit_backward_batch(int32_t mode, int32_t memory_channels, const die_batch* b, const int32_t* parent_of,
                                                 const int32_t* child_of, const float* grad, float* grad_memory, void* stream) {
    const char* who = "die_memory_inherit_backward_batch";
    DIE_REQUIRE(b, "%s: null argument", who);
    return inherit_backward(mode, memory_channels, b, b->agent_stride, parent_of, child_of, grad, grad_memory, stream, who);
}
