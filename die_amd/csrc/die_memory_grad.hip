// The adjoints of a NeuralAutomataAgent's memory channels (gfx950): what backpropagation through time needs of die_memory.hip
// (NeuralAutomataAgent.recurrent_action, die_amd.functional.memory_record / memory_planes / gather_memory).
//
//   k_memory_cells            the record: one thread per stored entry n < N.  With id = slot ? slot[n] : n it writes
//                             cell[id] = the entry's cell (ix * H + iy, die_cell_u) for an alive slot, -1 for a dead one, and
//                             win[id] = that cell where the standing word there, at `epoch`, names id + 1, else -1 — dead
//                             slots and the losers of a shared cell.  die_deposit_cells' idea on the sense side: with the two
//                             arrays in hand both adjoints below are index-only and never look at the world again, so a graph
//                             survives every step, re-sort and reset.
//   k_memory_planes_backward  the expand's adjoint, a pure gather: one thread per slot id, grad_memory[j][id] = win[id] inside
//                             the plane ? grad_planes[j][win[id]] : +0.  Every word of the M rows is written once; the values
//                             travel as 32-bit words; plain loads and stores, the same bits on every run.  (Only a cell's
//                             winner was read by the expand, so only the winner gets the cell's gradient.)
//   k_gather_memory_backward  the read-out's adjoint, a scatter: the M planes are cleared on the stream, then one thread per slot
//                             id adds grad_memory[j][id] to grad_planes[j][cell[id]] where cell[id] is inside the plane — fp32
//                             atomic adds, die_gather_scale_backward's method; a zero term is skipped.  Every alive slot of a
//                             shared cell read the cell, so every one of them adds.
//
//
// The batched twins (BatchedNeuralAutomataAgent.recurrent_action; die_amd.functional.memory_record_batch / memory_planes_batch /
// gather_memory_batch): k_memory_cells_batch, k_memory_planes_backward_batch and k_gather_memory_backward_batch run the SAME three
// device bodies for replica blockIdx.y of a die_batch — one launch each for all R replicas, replica r's slots r * agent_stride
// on, its planes a replica stride on.  The record's padding slots n >= n[r] are written -1 in both arrays, so the two adjoints
// never look at n[] again: a -1 gathers +0 and scatters nothing.
//
// Roofline: latency, as die_memory.hip's own note says of the forward pair: a few thousand words move, the launch is the cost.
// The batched twins move R times as many words — at 16 x 96^2 worlds and M = 2 still under a megabyte — and stay launch-latency
// bound: what they buy is one launch where R stood.
#include "die_common.h"

struct MemCellsArgs {
    const uint32_t *x, *y, *slot;
    const uint8_t* alive;
    const unsigned long long* standing;
    int32_t *cell, *win;
    int64_t N;
    int W, H, epoch;
};

// stored entry n < a.N: its two words of the record
__device__ __forceinline__ void memory_cells_one(const MemCellsArgs& a, int64_t n) {
    const int64_t id = a.slot ? (int64_t)a.slot[n] : n;
    if (id >= a.N) return;                                   // (slot ids are 0 .. N - 1: never past the arrays)
    const bool alive = a.alive[n] != 0;
    const int c = die_cell_u(a.x[n], a.W) * a.H + die_cell_u(a.y[n], a.H);       // < W * H <= 2^31 - 1 (checked on the host)
    const bool won = alive && (uint32_t)(a.standing[c] >> 32) == die_owner_word(a.epoch, id);
    a.cell[id] = alive ? c : -1;
    a.win[id] = won ? c : -1;
}

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_cells(MemCellsArgs a) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n < a.N) memory_cells_one(a, n);
}

// replica blockIdx.y: its slots and its rows of the record `agents` words on, its standing plane `rep_plane` words on; the
// padding slots n[r] .. agents - 1 get -1 twice
struct MemCellsBatchArgs : MemCellsArgs {
    int64_t rep_plane, agents;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_cells_batch(MemCellsBatchArgs b) {
    const int r = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= b.agents) return;
    const int64_t pa = b.agents * r;
    MemCellsArgs a = b;
    a.x += pa; a.y += pa; a.alive += pa; a.cell += pa; a.win += pa;
    a.standing += b.rep_plane * r;
    a.N = b.n[r];
    if (n < a.N) memory_cells_one(a, n);
    else { a.cell[n] = -1; a.win[n] = -1; }
}

struct MemIndexArgs {
    const int32_t* index;                    // win (the expand's adjoint) or cell (the read-out's), by slot id
    const uint32_t* src;                     // what is read: row j / plane j at src + j * src_stride
    uint32_t* dst;                           // what is written: row j / plane j at dst + j * dst_stride
    int64_t n_slots, src_stride, dst_stride;
    uint32_t cells;
    int M;
};

// slot id < a.n_slots: its M words of the gather
__device__ __forceinline__ void memory_planes_backward_one(const MemIndexArgs& a, int64_t id) {
    const uint32_t c = (uint32_t)a.index[id];                // (-1 is 2^32 - 1: outside, as every index from W * H on)
    const bool in = c < a.cells;
    for (int j = 0; j < a.M; ++j) a.dst[a.dst_stride * j + id] = in ? a.src[a.src_stride * j + c] : 0u;
}

// slot id < a.n_slots: its M terms of the scatter
__device__ __forceinline__ void gather_memory_backward_one(const MemIndexArgs& a, int64_t id) {
    const uint32_t c = (uint32_t)a.index[id];
    if (c >= a.cells) return;
    for (int j = 0; j < a.M; ++j) {
        const float v = __uint_as_float(a.src[a.src_stride * j + id]);
        if (v != 0.f) atomicAdd((float*)a.dst + a.dst_stride * j + c, v);        // (a zero term changes no sum)
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_planes_backward(MemIndexArgs a) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n_slots) memory_planes_backward_one(a, id);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_memory_backward(MemIndexArgs a) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n_slots) gather_memory_backward_one(a, id);
}

// replica blockIdx.y: its row of the record n_slots words on (n_slots = the batch's agent_stride), what it reads `rep_src` and
// what it writes `rep_dst` words on
struct MemIndexBatchArgs : MemIndexArgs {
    int64_t rep_src, rep_dst;
};

__device__ __forceinline__ MemIndexArgs memory_index_replica(const MemIndexBatchArgs& b, int r) {
    MemIndexArgs a = b;
    a.index += b.n_slots * r; a.src += b.rep_src * r; a.dst += b.rep_dst * r;
    return a;
}

__global__ __launch_bounds__(DIE_BLOCK) void k_memory_planes_backward_batch(MemIndexBatchArgs b) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < b.n_slots) memory_planes_backward_one(memory_index_replica(b, blockIdx.y), id);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_memory_backward_batch(MemIndexBatchArgs b) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < b.n_slots) gather_memory_backward_one(memory_index_replica(b, blockIdx.y), id);
}

// ---- the entry points: every argument checked before anything is launched -------------------------------------------------
static int index_check(int32_t W, int32_t H, int32_t M, int64_t n_slots, int64_t row_stride, int64_t plane_stride, const char* who) {
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE(M >= 1 && M <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who, M, DIE_MEMORY_MAX_CHANNELS);
    const int64_t cells = (int64_t)W * H;
    DIE_REQUIRE(cells <= (int64_t)INT32_MAX, "%s: %dx%d cells do not fit the int32 cell index", who, W, H);
    DIE_REQUIRE(n_slots >= 0 && n_slots <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: %lld slots outside 0..%lld", who, (long long)n_slots,
                (long long)DIE_OWNER_SLOT_MASK - 1);
    DIE_REQUIRE(row_stride >= n_slots && row_stride >= 1, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride,
                (long long)n_slots);
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    return DIE_OK;
}

extern "C" int die_memory_cells(const die_medium* m, const die_agents* agents, const unsigned long long* standing, int32_t epoch,
                                int32_t* cell_out, int32_t* win_out, void* stream) {
    const char* who = "die_memory_cells";
    DIE_REQUIRE(m && agents && standing && cell_out && win_out, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium has no standing plane (periodic single-tile planes only)", who);
        return DIE_ERR_UNSUPPORTED;
    }
    const int64_t cells = (int64_t)m->W * m->H, N = agents->N;
    DIE_REQUIRE(cells <= (int64_t)INT32_MAX, "%s: %dx%d cells do not fit the int32 cell index", who, m->W, m->H);
    DIE_REQUIRE(epoch >= 1 && epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, epoch, DIE_OWNER_EPOCH_MAX);
    DIE_REQUIRE(N >= 0 && N <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: %lld slots outside 0..%lld", who, (long long)N,
                (long long)DIE_OWNER_SLOT_MASK - 1);
    DIE_REQUIRE(N == 0 || (agents->x && agents->y && agents->alive), "%s: null agent array", who);
    int32_t* const outs[2] = {cell_out, win_out};
    DIE_REQUIRE(!die_ranges_overlap(cell_out, N * 4, win_out, N * 4), "%s: the two records overlap", who);
    for (int q = 0; q < 2 && N > 0; ++q) {
        DIE_REQUIRE(!die_ranges_overlap(outs[q], N * 4, standing, cells * 8), "%s: a record overlaps the standing plane", who);
        DIE_REQUIRE(!die_ranges_overlap(outs[q], N * 4, agents->x, N * 4) && !die_ranges_overlap(outs[q], N * 4, agents->y, N * 4) &&
                    !die_ranges_overlap(outs[q], N * 4, agents->alive, N) && !die_ranges_overlap(outs[q], N * 4, agents->slot, N * 4),
                    "%s: a record overlaps the agent arrays", who);
    }
    if (N == 0) return DIE_OK;                               // no stored entry: nothing to write
    MemCellsArgs k;
    k.x = agents->x; k.y = agents->y; k.slot = agents->slot; k.alive = agents->alive;
    k.standing = standing; k.cell = cell_out; k.win = win_out; k.N = N; k.W = m->W; k.H = m->H; k.epoch = epoch;
    k_memory_cells<<<(unsigned)((N + DIE_BLOCK - 1) / DIE_BLOCK), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_memory_planes_backward(int32_t W, int32_t H, int32_t memory_channels, int64_t n_slots, const int32_t* win,
                                          const float* grad_planes, int64_t plane_stride, float* grad_memory, int64_t row_stride,
                                          void* stream) {
    const char* who = "die_memory_planes_backward";
    DIE_REQUIRE(win && grad_planes && grad_memory, "%s: null argument", who);
    const int rc = index_check(W, H, memory_channels, n_slots, row_stride, plane_stride, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)W * H, M = memory_channels;
    const int64_t out_bytes = ((M - 1) * row_stride + n_slots) * 4;
    DIE_REQUIRE(!die_ranges_overlap(grad_memory, out_bytes, win, n_slots * 4), "%s: the memory gradient overlaps the record", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_memory, out_bytes, grad_planes, ((M - 1) * plane_stride + cells) * 4),
                "%s: the memory gradient overlaps the planes' gradient", who);
    if (n_slots == 0) return DIE_OK;                         // no slot: nothing to write
    MemIndexArgs k;
    k.index = win; k.src = (const uint32_t*)grad_planes; k.dst = (uint32_t*)grad_memory;
    k.n_slots = n_slots; k.src_stride = plane_stride; k.dst_stride = row_stride; k.cells = (uint32_t)cells; k.M = memory_channels;
    k_memory_planes_backward<<<(unsigned)((n_slots + DIE_BLOCK - 1) / DIE_BLOCK), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_gather_memory_backward(int32_t W, int32_t H, int32_t memory_channels, int64_t n_slots, const int32_t* cell,
                                          const float* grad_memory, int64_t row_stride, float* grad_planes, int64_t plane_stride,
                                          void* stream) {
    const char* who = "die_gather_memory_backward";
    DIE_REQUIRE(cell && grad_memory && grad_planes, "%s: null argument", who);
    const int rc = index_check(W, H, memory_channels, n_slots, row_stride, plane_stride, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)W * H, M = memory_channels;
    const int64_t out_bytes = ((M - 1) * plane_stride + cells) * 4;
    DIE_REQUIRE(!die_ranges_overlap(grad_planes, out_bytes, cell, n_slots * 4), "%s: the planes' gradient overlaps the record", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_planes, out_bytes, grad_memory, ((M - 1) * row_stride + n_slots) * 4),
                "%s: the planes' gradient overlaps the memory gradient", who);
    for (int j = 0; j < memory_channels; ++j) {              // the cells of every plane; the words between two planes are left alone
        if (hipMemsetAsync(grad_planes + plane_stride * j, 0, (size_t)cells * sizeof(float), (hipStream_t)stream) != hipSuccess) {
            die_set_error("%s: clearing plane %d failed", who, j);
            return DIE_ERR_HIP;
        }
    }
    if (n_slots == 0) return DIE_OK;                         // no slot: the cleared planes are the answer
    MemIndexArgs k;
    k.index = cell; k.src = (const uint32_t*)grad_memory; k.dst = (uint32_t*)grad_planes;
    k.n_slots = n_slots; k.src_stride = row_stride; k.dst_stride = plane_stride; k.cells = (uint32_t)cells; k.M = memory_channels;
    k_gather_memory_backward<<<(unsigned)((n_slots + DIE_BLOCK - 1) / DIE_BLOCK), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the batched entry points (the replica in blockIdx.y): every argument checked before anything is launched -------------
extern "C" int die_memory_cells_batch(const die_medium* m, const die_agents* agents, const die_batch* b, const unsigned long long* standing,
                                      int32_t epoch, int32_t* cell_out, int32_t* win_out, void* stream) {
    const char* who = "die_memory_cells_batch";
    DIE_REQUIRE(m && agents && b && standing && cell_out && win_out, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium has no standing plane (periodic single-tile planes only)", who);
        return DIE_ERR_UNSUPPORTED;
    }
    const int64_t cells = (int64_t)m->W * m->H;
    DIE_REQUIRE(cells <= (int64_t)INT32_MAX, "%s: %dx%d cells do not fit the int32 cell index", who, m->W, m->H);
    DIE_REQUIRE(epoch >= 1 && epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, epoch, DIE_OWNER_EPOCH_MAX);
    const int rc = die_batch_check(b, -1, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(b->plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)b->plane_stride,
                (long long)cells);
    DIE_REQUIRE(agents->x && agents->y && agents->alive, "%s: null agent array", who);
    DIE_REQUIRE(!agents->slot, "%s: replicas hold their agents in slot order (no slot array)", who);
    const int64_t R = b->replicas, slots = R * b->agent_stride;
    int32_t* const outs[2] = {cell_out, win_out};
    DIE_REQUIRE(!die_ranges_overlap(cell_out, slots * 4, win_out, slots * 4), "%s: the two records overlap", who);
    for (int q = 0; q < 2; ++q) {
        DIE_REQUIRE(!die_ranges_overlap(outs[q], slots * 4, standing, ((R - 1) * b->plane_stride + cells) * 8), "%s: a record overlaps the standing "
                    "planes", who);
        DIE_REQUIRE(!die_ranges_overlap(outs[q], slots * 4, agents->x, slots * 4) && !die_ranges_overlap(outs[q], slots * 4, agents->y, slots * 4) &&
                    !die_ranges_overlap(outs[q], slots * 4, agents->alive, slots), "%s: a record overlaps the agent arrays", who);
    }
    MemCellsBatchArgs k;
    k.x = agents->x; k.y = agents->y; k.slot = nullptr; k.alive = agents->alive;
    k.standing = standing; k.cell = cell_out; k.win = win_out; k.N = 0; k.W = m->W; k.H = m->H; k.epoch = epoch;
    k.rep_plane = b->plane_stride; k.agents = b->agent_stride;
    die_replica_counts(k.n, b->n, b->replicas);
    k_memory_cells_batch<<<dim3((unsigned)((b->agent_stride + DIE_BLOCK - 1) / DIE_BLOCK), (unsigned)R), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// what the two batched index calls check alike, in the stand-alone calls' order
static int index_batch_check(int32_t W, int32_t H, int32_t M, const die_batch* b, int64_t row_stride, int64_t plane_stride,
                             int64_t replica_stride, const char* who) {
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE(M >= 1 && M <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who, M, DIE_MEMORY_MAX_CHANNELS);
    const int64_t cells = (int64_t)W * H;
    DIE_REQUIRE(cells <= (int64_t)INT32_MAX, "%s: %dx%d cells do not fit the int32 cell index", who, W, H);
    const int rc = die_batch_check(b, -1, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(row_stride >= b->agent_stride, "%s: row_stride %lld smaller than a row (%lld slots)", who, (long long)row_stride,
                (long long)b->agent_stride);
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    // replica-major ([R][M] planes: a sense gradient, a grad_in) or plane-major ([M][R]: die_memory_planes_batch's layout): either
    // way no two of the R * M planes share a word
    DIE_REQUIRE(replica_stride >= cells && (replica_stride >= (int64_t)(M - 1) * plane_stride + cells ||
                                            plane_stride >= (int64_t)(b->replicas - 1) * replica_stride + cells),
                "%s: replica_stride %lld with plane_stride %lld: the %d x %d planes would share words", who, (long long)replica_stride,
                (long long)plane_stride, b->replicas, M);
    return DIE_OK;
}

static MemIndexBatchArgs index_batch_args(int32_t W, int32_t H, int32_t M, const die_batch* b, const int32_t* index) {
    MemIndexBatchArgs k;
    k.index = index; k.n_slots = b->agent_stride; k.cells = (uint32_t)((int64_t)W * H); k.M = M;
    return k;
}

extern "C" int die_memory_planes_backward_batch(int32_t W, int32_t H, int32_t memory_channels, const die_batch* b, const int32_t* win,
                                                const float* grad_planes, int64_t plane_stride, int64_t replica_stride, float* grad_memory,
                                                int64_t row_stride, void* stream) {
    const char* who = "die_memory_planes_backward_batch";
    DIE_REQUIRE(b && win && grad_planes && grad_memory, "%s: null argument", who);
    const int rc = index_batch_check(W, H, memory_channels, b, row_stride, plane_stride, replica_stride, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)W * H, M = memory_channels, R = b->replicas, S = b->agent_stride;
    const int64_t out_bytes = ((R * M - 1) * row_stride + S) * 4;
    DIE_REQUIRE(!die_ranges_overlap(grad_memory, out_bytes, win, R * S * 4), "%s: the memory gradient overlaps the record", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_memory, out_bytes, grad_planes, ((R - 1) * replica_stride + (M - 1) * plane_stride + cells) * 4),
                "%s: the memory gradient overlaps the planes' gradient", who);
    MemIndexBatchArgs k = index_batch_args(W, H, memory_channels, b, win);
    k.src = (const uint32_t*)grad_planes; k.src_stride = plane_stride; k.rep_src = replica_stride;
    k.dst = (uint32_t*)grad_memory; k.dst_stride = row_stride; k.rep_dst = M * row_stride;
    k_memory_planes_backward_batch<<<dim3((unsigned)((S + DIE_BLOCK - 1) / DIE_BLOCK), (unsigned)R), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_gather_memory_backward_batch(int32_t W, int32_t H, int32_t memory_channels, const die_batch* b, const int32_t* cell,
                                                const float* grad_memory, int64_t row_stride, float* grad_planes, int64_t plane_stride,
                                                int64_t replica_stride, void* stream) {
    const char* who = "die_gather_memory_backward_batch";
    DIE_REQUIRE(b && cell && grad_memory && grad_planes, "%s: null argument", who);
    const int rc = index_batch_check(W, H, memory_channels, b, row_stride, plane_stride, replica_stride, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)W * H, M = memory_channels, R = b->replicas, S = b->agent_stride;
    const int64_t out_bytes = ((R - 1) * replica_stride + (M - 1) * plane_stride + cells) * 4;
    DIE_REQUIRE(!die_ranges_overlap(grad_planes, out_bytes, cell, R * S * 4), "%s: the planes' gradient overlaps the record", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_planes, out_bytes, grad_memory, ((R * M - 1) * row_stride + S) * 4),
                "%s: the planes' gradient overlaps the memory gradient", who);
    // the cells of every plane of every replica; the words between two planes and between two replicas are left alone: one
    // strided clear over the replicas where a replica's planes are dense, one per plane otherwise
    const bool dense = plane_stride == cells && replica_stride >= M * cells;
    for (int j = 0; j < (dense ? 1 : memory_channels); ++j) {
        if (hipMemset2DAsync(grad_planes + plane_stride * j, (size_t)replica_stride * sizeof(float), 0,
                             (size_t)(dense ? M : 1) * cells * sizeof(float), (size_t)R, (hipStream_t)stream) != hipSuccess) {
            die_set_error("%s: clearing plane %d failed", who, j);
            return DIE_ERR_HIP;
        }
    }
    MemIndexBatchArgs k = index_batch_args(W, H, memory_channels, b, cell);
    k.src = (const uint32_t*)grad_memory; k.src_stride = row_stride; k.rep_src = M * row_stride;
    k.dst = (uint32_t*)grad_planes; k.dst_stride = plane_stride; k.rep_dst = replica_stride;
    k_gather_memory_backward_batch<<<dim3((unsigned)((S + DIE_BLOCK - 1) / DIE_BLOCK), (unsigned)R), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}
