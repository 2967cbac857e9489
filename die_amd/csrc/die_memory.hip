// The memory channels of a NeuralAutomataAgent (gfx950): NeuralAutomataAgent(memory_channels=M), 1 <= M <= 8 — M values every
// agent carries from one forward to the next (no reference counterpart: core/agent/learning.py "TODO: need joint
// channels info for the system").  The memory is an (M, N) fp32 array indexed by SLOT ID, so it follows an agent through every
// re-sort of the storage.
//
//   k_memory_planes  the expand: one pass over the cells of replica blockIdx.y.  Reads the standing plane die_stock.hip builds
//                    (the claim plane's word: who stands on the cell at `epoch`, highest slot id of the alive ones) and writes M
//                    fp32 planes, P_j[c] = occupied(c) ? mem[j][winner(c)] : +0 — EVERY cell of every plane, so nobody clears
//                    them.  The word's payload (the stock) is ignored.  A thread owns 4 consecutive cells where the planes allow
//                    (32 bytes of words in, M 16-byte stores out: the wide layer's store width), one cell otherwise; the gather
//                    from the memory happens at occupied cells only.  The values travel as 32-bit words: negative zero,
//                    denormals and NaN payloads keep their bits.  A winner id past the memory's row (a plane built from other
//                    agents) reads as empty instead of reading out of bounds.
//   k_gather_memory  the read-out: one thread per stored slot n < n[r] of replica blockIdx.y, mem[j][id] = alive ?
//                    S_j[cell of the slot] : +0 with id = slot ? slot[n] : n.  No coefficient, no atomics: slot ids are distinct,
//                    so every word of the memory has one writer.  Dead slots are zeroed (a slot's next occupant starts blank);
//                    a replica's padding slots n >= n[r] are neither read nor written.
//
// Roofline: latency.  At 10 x 96^2 worlds the expand moves 8 + 4 M bytes per cell (92 160 cells: 1.5 MB at M = 2) and the
// read-out a few thousand words; both are far below what the memory system notices, and the launch itself is the cost — as
// for the stock build (LABBOOK §31: 3.6 us).
#include "die_common.h"
#include "die_nca.h"

struct MemPlanesArgs {
    const unsigned long long* standing;      // replica r's plane standing_rep words on
    const uint32_t* mem;                     // row j of replica r at mem + r * mem_rep + j * mem_row
    uint32_t* planes;                        // plane j of replica r at planes + j * plane_j + r * plane_rep
    int64_t cells, standing_rep, mem_row, mem_rep, plane_j, plane_rep;
    int M, epoch, vec;
    int64_t n[DIE_MAX_REPLICAS];             // slots a winner id may name (the width of a memory row that is read)
};

__device__ __forceinline__ int64_t mem_winner(unsigned long long word, int epoch, int64_t n) {
    if (!die_claim_occupied(word, epoch)) return -1;
    const int64_t id = (int64_t)((uint32_t)(word >> 32) & DIE_OWNER_SLOT_MASK) - 1;
    return id < n ? id : -1;
}

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_planes(MemPlanesArgs a) {
    const int r = blockIdx.y;
    const unsigned long long* standing = a.standing + a.standing_rep * r;
    const uint32_t* mem = a.mem + a.mem_rep * r;
    uint32_t* planes = a.planes + a.plane_rep * r;
    const int64_t n = a.n[r];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.vec) {
        const int64_t c = t * 4;
        if (c >= a.cells) return;                            // (cells % 4 == 0: a thread's 4 cells are all inside)
        const ulonglong2 w01 = *(const ulonglong2*)(standing + c), w23 = *(const ulonglong2*)(standing + c + 2);
        const int64_t id[4] = {mem_winner(w01.x, a.epoch, n), mem_winner(w01.y, a.epoch, n), mem_winner(w23.x, a.epoch, n),
                               mem_winner(w23.y, a.epoch, n)};
        for (int j = 0; j < a.M; ++j) {
            const uint32_t* row = mem + a.mem_row * j;
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = id[q] >= 0 ? row[id[q]] : 0u;
            *(uint4*)(planes + a.plane_j * j + c) = make_uint4(v[0], v[1], v[2], v[3]);
        }
    } else {
        if (t >= a.cells) return;
        const int64_t id = mem_winner(standing[t], a.epoch, n);
        for (int j = 0; j < a.M; ++j) planes[a.plane_j * j + t] = id >= 0 ? mem[a.mem_row * j + id] : 0u;
    }
}

struct MemGatherArgs {
    const uint32_t *x, *y, *slot;
    const uint8_t* alive;
    const uint32_t* planes;                  // S_j of replica r at planes + r * plane_rep + j * plane_j
    uint32_t* mem;                           // row j of replica r at mem + r * mem_rep + j * mem_row
    int64_t agent_stride, plane_j, plane_rep, mem_row, mem_rep;
    int W, H, M;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_memory(MemGatherArgs a) {
    const int r = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.n[r]) return;
    const int64_t i = a.agent_stride * r + n;
    const int64_t id = a.slot ? (int64_t)a.slot[i] : n;
    if (id >= a.n[r]) return;                                // (slot ids are 0 .. n - 1: never past the row)
    const bool alive = a.alive[i] != 0;
    const int64_t c = alive ? (int64_t)die_cell_u(a.x[i], a.W) * a.H + die_cell_u(a.y[i], a.H) : 0;      // (always inside the plane)
    const uint32_t* planes = a.planes + a.plane_rep * r + c;
    uint32_t* mem = a.mem + a.mem_rep * r + id;
    for (int j = 0; j < a.M; ++j) mem[a.mem_row * j] = alive ? planes[a.plane_j * j] : 0u;
}

// ---- the launches alone: every argument has been checked by the caller (the entry points below, die_env.hip's fused step) ----
int die_memory_planes_launch(int32_t W, int32_t H, int32_t replicas, const int64_t* n, const unsigned long long* standing,
                             int64_t standing_rep, int32_t epoch, int32_t M, const float* mem, int64_t mem_row, int64_t mem_rep,
                             float* planes, int64_t plane_j, int64_t plane_rep, void* stream, const char* who) {
    MemPlanesArgs k;
    k.standing = standing; k.mem = (const uint32_t*)mem; k.planes = (uint32_t*)planes;
    k.cells = (int64_t)W * H; k.standing_rep = standing_rep; k.mem_row = mem_row; k.mem_rep = mem_rep;
    k.plane_j = plane_j; k.plane_rep = plane_rep; k.M = M; k.epoch = epoch;
    // 16-byte accesses: whole groups of 4 cells, and every plane of every replica starting on a 16-byte boundary
    k.vec = (H & 3) == 0 && (plane_j & 3) == 0 && (plane_rep & 3) == 0 && ((uintptr_t)planes & 15) == 0 && (standing_rep & 1) == 0 &&
            ((uintptr_t)standing & 15) == 0;
    die_replica_counts(k.n, n, replicas);
    const int64_t units = k.vec ? k.cells / 4 : k.cells, g = (units + DIE_BLOCK - 1) / DIE_BLOCK;
    DIE_REQUIRE(g <= 0x7FFFFFFF, "%s: field too large (%lld cells)", who, (long long)k.cells);
    k_memory_planes<<<dim3((unsigned)g, (unsigned)replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

int die_gather_memory_launch(const die_medium* m, const die_agents* a, int32_t replicas, const int64_t* n, int64_t agent_stride, int32_t M,
                             const float* planes, int64_t plane_j, int64_t plane_rep, float* mem, int64_t mem_row, int64_t mem_rep,
                             void* stream, const char* who) {
    MemGatherArgs k;
    k.x = a->x; k.y = a->y; k.slot = a->slot; k.alive = a->alive;
    k.planes = (const uint32_t*)planes; k.mem = (uint32_t*)mem;
    k.agent_stride = agent_stride; k.plane_j = plane_j; k.plane_rep = plane_rep; k.mem_row = mem_row; k.mem_rep = mem_rep;
    k.W = m->W; k.H = m->H; k.M = M;
    const int64_t nmax = die_replica_counts(k.n, n, replicas);
    if (nmax == 0) return DIE_OK;                            // no slot anywhere: nothing to write
    k_gather_memory<<<dim3((unsigned)((nmax + DIE_BLOCK - 1) / DIE_BLOCK), (unsigned)replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the stand-alone entry points: every argument checked before anything is launched ---------------------------------
static int memory_world_check(const die_medium* m, int32_t M, const char* who) {
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium has no memory planes (periodic single-tile planes only)", who);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(M >= 1 && M <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who, M, DIE_MEMORY_MAX_CHANNELS);
    return DIE_OK;
}

extern "C" int die_memory_planes(const die_medium* m, const unsigned long long* standing, int32_t epoch, int32_t memory_channels,
                                 const float* memory, int64_t row_stride, int64_t n_slots, float* planes, int64_t plane_stride,
                                 void* stream) {
    const char* who = "die_memory_planes";
    DIE_REQUIRE(m && standing && memory && planes, "%s: null argument", who);
    const int rc = memory_world_check(m, memory_channels, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    DIE_REQUIRE(epoch >= 1 && epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, epoch, DIE_OWNER_EPOCH_MAX);
    DIE_REQUIRE(n_slots >= 0 && n_slots <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: %lld slots outside 0..%lld", who, (long long)n_slots,
                (long long)DIE_OWNER_SLOT_MASK - 1);
    DIE_REQUIRE(row_stride >= n_slots && row_stride >= 1, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride,
                (long long)n_slots);
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    const int64_t out_bytes = ((int64_t)(memory_channels - 1) * plane_stride + cells) * 4;
    DIE_REQUIRE(!die_ranges_overlap(planes, out_bytes, standing, cells * 8), "%s: the output planes overlap the standing plane", who);
    DIE_REQUIRE(!die_ranges_overlap(planes, out_bytes, memory, ((int64_t)(memory_channels - 1) * row_stride + n_slots) * 4),
                "%s: the output planes overlap the memory", who);
    return die_memory_planes_launch(m->W, m->H, 1, &n_slots, standing, 0, epoch, memory_channels, memory, row_stride, 0, planes, plane_stride,
                                    0, stream, who);
}

extern "C" int die_memory_planes_batch(const die_medium* m, const die_batch* b, const unsigned long long* standing, int32_t epoch,
                                       int32_t memory_channels, const float* memory, int64_t row_stride, float* planes, void* stream) {
    const char* who = "die_memory_planes_batch";
    DIE_REQUIRE(m && b && standing && memory && planes, "%s: null argument", who);
    int rc = memory_world_check(m, memory_channels, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    DIE_REQUIRE(epoch >= 1 && epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, epoch, DIE_OWNER_EPOCH_MAX);
    rc = die_batch_check(b, cells, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(row_stride >= b->agent_stride, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride,
                (long long)b->agent_stride);
    const int64_t R = b->replicas, M = memory_channels;
    const int64_t out_bytes = ((M * R - 1) * b->plane_stride + cells) * 4;
    DIE_REQUIRE(!die_ranges_overlap(planes, out_bytes, standing, ((R - 1) * b->plane_stride + cells) * 8), "%s: the output planes overlap the "
                "standing planes", who);
    DIE_REQUIRE(!die_ranges_overlap(planes, out_bytes, memory, R * M * row_stride * 4), "%s: the output planes overlap the memory", who);
    return die_memory_planes_launch(m->W, m->H, b->replicas, b->n, standing, b->plane_stride, epoch, memory_channels, memory, row_stride,
                                    M * row_stride, planes, R * b->plane_stride, b->plane_stride, stream, who);
}

static int gather_check(const die_medium* m, const die_agents* a, int32_t M, const float* planes, const float* memory, const char* who) {
    DIE_REQUIRE(m && a && planes && memory, "%s: null argument", who);
    DIE_REQUIRE(a->x && a->y && a->alive, "%s: null agent array", who);
    return memory_world_check(m, M, who);
}

extern "C" int die_gather_memory(const die_medium* m, const die_agents* agents, int32_t memory_channels, const float* planes,
                                 int64_t plane_stride, float* memory, int64_t row_stride, void* stream) {
    const char* who = "die_gather_memory";
    const int rc = gather_check(m, agents, memory_channels, planes, memory, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H, N = agents->N;
    DIE_REQUIRE(N >= 0 && N <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: %lld slots outside 0..%lld", who, (long long)N,
                (long long)DIE_OWNER_SLOT_MASK - 1);
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    DIE_REQUIRE(row_stride >= N && row_stride >= 1, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride, (long long)N);
    DIE_REQUIRE(!die_ranges_overlap(memory, ((int64_t)(memory_channels - 1) * row_stride + N) * 4, planes,
                             ((int64_t)(memory_channels - 1) * plane_stride + cells) * 4), "%s: the memory overlaps the planes", who);
    return die_gather_memory_launch(m, agents, 1, &N, 0, memory_channels, planes, plane_stride, 0, memory, row_stride, 0, stream, who);
}

extern "C" int die_gather_memory_batch(const die_medium* m, const die_agents* agents, const die_batch* b, int32_t memory_channels,
                                       const float* planes, int64_t plane_stride, int64_t replica_stride, float* memory, int64_t row_stride,
                                       void* stream) {
    const char* who = "die_gather_memory_batch";
    DIE_REQUIRE(b, "%s: null argument", who);
    int rc = gather_check(m, agents, memory_channels, planes, memory, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(!agents->slot, "%s: replicas hold their agents in slot order (no slot array)", who);
    const int64_t cells = (int64_t)m->W * m->H, R = b->replicas, M = memory_channels;
    rc = die_batch_check(b, cells, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    DIE_REQUIRE(replica_stride >= (M - 1) * plane_stride + cells, "%s: replica_stride %lld smaller than a replica's %lld planes", who,
                (long long)replica_stride, (long long)M);
    DIE_REQUIRE(row_stride >= b->agent_stride, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride,
                (long long)b->agent_stride);
    DIE_REQUIRE(!die_ranges_overlap(memory, R * M * row_stride * 4, planes, ((R - 1) * replica_stride + (M - 1) * plane_stride + cells) * 4),
                "%s: the memory overlaps the planes", who);
    return die_gather_memory_launch(m, agents, b->replicas, b->n, b->agent_stride, memory_channels, planes, plane_stride, replica_stride,
                                    memory, row_stride, M * row_stride, stream, who);
}
