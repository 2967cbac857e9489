// The adjoint of Env.step's chem path (gfx950) — what Env.differentiable_step records and backpropagates.
//
// Of one step only this path carries an agent's parameters into the next step's observation:
//   chem' = (1 − decay) · G(chem + D),   D[cell] = deposit[n] where slot n won the cell (core/env.py:204-215, :136-145),
// G the separable periodic gaussian of k_diffuse / k_diffuse_rows (die_env.hip).  Positions are piecewise constant in the parameters
// (nearest-cell lookup), so food, the claim plane and the cells themselves have a zero gradient and nothing is approximated.
//
//   k_deposit_cells   who deposited where: entry n gets its cell ix · H + iy if it is alive and the claim word of that cell carries
//                     (epoch, slot + 1) — the winner k_resolve / the fused sweep added to chem — else −1.  Coordinates and claim
//                     words are read exactly as the step reads them (die_cell_u; the high word of the 64-bit claim).  One launch,
//                     coalesced reads of the arrays, one 8-byte read per entry of the claim plane (random unless the arrays are
//                     sorted: served by the L2, like the step's own claim pass), one coalesced 4-byte store.
//   die_env_step_backward
//       field part    grad_chem = (1 − decay) · Gᵀ(grad_chem_next).  On the torus with symmetric taps Gᵀ = G: the circulant of a
//                     symmetric kernel is a symmetric matrix, along both axes, and the two axis passes commute.  So the adjoint IS
//                     the forward sweep: die_diffuse_decay on the gradient plane — gaussian_taps, the row sweep where H % 4 == 0 and
//                     radius ≤ 4, the LDS-tiled kernel elsewhere.  No second gaussian exists in this library
//                     (tests/test_gpu_field_step_grad.py proves the identity ⟨step(c, d), g⟩ = ⟨c, grad_chem⟩ + ⟨d, grad_deposit⟩).
//       k_gather_cells   grad_deposit[n] = cells[n] ≥ 0 ? grad_chem[cells[n]] : 0, after the sweep on the same stream.  A gather:
//                     plain vector loads and stores, no atomics, every output written once by one thread.  Consecutive entries are
//                     grid neighbours only after sort_agents; otherwise the 4-byte reads are random over a plane that fits the L2
//                     up to 1024² and the Infinity Cache beyond.  Four entries per thread are in flight before the first is used.
//                     An index at or beyond W · H is treated like −1 (0 is stored): a bad cell never leaves the plane.
//
//   die_deposit_cells_batch / die_env_step_backward_batch   the same for every replica of a die_batch in one launch each (replica in
//                     blockIdx.y; the field part is die_diffuse_rows_batch of die_env.hip: the row sweep with the replica in gridDim.z,
//                     or one launch per gaussian radius under per-replica Dynamics).  Replica r is the stand-alone call, bit for bit.
//
// Roofline: both kernels move 4 to 20 bytes per entry and compute nothing; they are bound by the launch on every world this
// path is meant for (LABBOOK §20).
#include "die_common.h"

struct DepositCellsArgs {
    int W, H, epoch;
    int64_t N;
    const unsigned long long* owner;
    const uint32_t* x;
    const uint32_t* y;
    const uint8_t* alive;
    const uint32_t* slot;      // reference slot ids (NULL = identity)
    int32_t* cells;
};

__global__ __launch_bounds__(DIE_BLOCK) void k_deposit_cells(DepositCellsArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) {
        const int c = die_cell_u(a.x[n], a.W) * a.H + die_cell_u(a.y[n], a.H);       // < W · H ≤ 2^31 − 1 (checked on the host)
        const uint32_t sid = a.slot ? a.slot[n] : (uint32_t)n;
        const bool won = a.alive[n] != 0 && (uint32_t)(a.owner[c] >> 32) == die_owner_word(a.epoch, (int64_t)sid);
        a.cells[n] = won ? c : -1;
    }
}

#define GATHER_PER_THREAD 4

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_cells(const float* __restrict__ plane, uint32_t n_cells, const int32_t* __restrict__ cells,
                                                            int64_t N, float* __restrict__ out) {
    // a workgroup takes GATHER_PER_THREAD consecutive runs of DIE_BLOCK entries: every load and store of a wave is one
    // contiguous 256-byte run, and a thread's four gathers are issued before the first one is consumed
    const int64_t stride = (int64_t)gridDim.x * DIE_BLOCK * GATHER_PER_THREAD;
    for (int64_t base = (int64_t)blockIdx.x * DIE_BLOCK * GATHER_PER_THREAD + threadIdx.x; base < N; base += stride) {
        int32_t c[GATHER_PER_THREAD];
        float v[GATHER_PER_THREAD];
#pragma unroll
        for (int q = 0; q < GATHER_PER_THREAD; ++q) {
            const int64_t n = base + (int64_t)q * DIE_BLOCK;
            c[q] = n < N ? cells[n] : -1;
        }
#pragma unroll
        for (int q = 0; q < GATHER_PER_THREAD; ++q) v[q] = (uint32_t)c[q] < n_cells ? plane[(uint32_t)c[q]] : 0.f;   // (−1 is 2^32 − 1: out)
#pragma unroll
        for (int q = 0; q < GATHER_PER_THREAD; ++q) {
            const int64_t n = base + (int64_t)q * DIE_BLOCK;
            if (n < N) out[n] = v[q];
        }
    }
}

extern "C" int die_deposit_cells(const die_medium* m, const die_agents* ag, int32_t* cells_out, void* stream) {
    const char* who = "die_deposit_cells";
    DIE_REQUIRE(m && ag && cells_out, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    DIE_REQUIRE(m->epoch >= 1 && m->epoch <= DIE_OWNER_EPOCH_MAX, "%s: bad epoch %d", who, m->epoch);
    DIE_REQUIRE(m->owner, "%s: null claim plane", who);
    DIE_REQUIRE(ag->N >= 0 && ag->N <= (int64_t)DIE_OWNER_SLOT_MASK, "%s: bad slot count %lld", who, (long long)ag->N);
    DIE_REQUIRE(ag->N == 0 || (ag->x && ag->y && ag->alive), "%s: bad arrays", who);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium (one tile of a %dx%d world) is not supported", who, m->gW, m->gH);
        return DIE_ERR_UNSUPPORTED;
    }
    if ((int64_t)m->W * m->H > (int64_t)INT32_MAX) {
        die_set_error("%s: %dx%d cells do not fit the int32 cell index", who, m->W, m->H);
        return DIE_ERR_UNSUPPORTED;
    }
    if (ag->N == 0) return DIE_OK;
    DepositCellsArgs a;
    a.W = m->W; a.H = m->H; a.epoch = m->epoch; a.N = ag->N;
    a.owner = (const unsigned long long*)m->owner;
    a.x = (const uint32_t*)ag->x; a.y = (const uint32_t*)ag->y; a.alive = (const uint8_t*)ag->alive; a.slot = (const uint32_t*)ag->slot;
    a.cells = cells_out;
    const int64_t g = (ag->N + DIE_BLOCK - 1) / DIE_BLOCK;
    k_deposit_cells<<<(int)(g < 8192 ? g : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_env_step_backward(int32_t W, int32_t H, const float* grad_chem_next, float sigma, float decay, int64_t N,
                                     const int32_t* cells, float* grad_chem, float* grad_deposit, void* stream) {
    const char* who = "die_env_step_backward";
    DIE_REQUIRE(grad_chem_next && grad_chem, "%s: null argument", who);
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE(grad_chem != grad_chem_next, "%s: in-place grad_chem (it may not alias grad_chem_next)", who);
    DIE_REQUIRE(sigma > 0.f, "%s: sigma must be positive", who);      // (NaN fails too)
    DIE_REQUIRE(decay == decay, "%s: decay is not a number", who);
    DIE_REQUIRE(N >= 0, "%s: bad entry count %lld", who, (long long)N);
    const bool gather = N > 0 && grad_deposit;
    DIE_REQUIRE(!gather || cells, "%s: null cells", who);
    DIE_REQUIRE(!gather || ((const void*)grad_deposit != (const void*)grad_chem && (const void*)grad_deposit != (const void*)grad_chem_next &&
                            (const void*)grad_deposit != (const void*)cells),
                "%s: in-place grad_deposit", who);
    const int64_t n_cells = (int64_t)W * H;
    if (n_cells > (int64_t)INT32_MAX) {
        die_set_error("%s: %dx%d cells do not fit the int32 cell index", who, W, H);
        return DIE_ERR_UNSUPPORTED;
    }
    const int R = die_gaussian_radius(sigma);                   // gaussian_taps' radius: refused here, before any launch
    DIE_REQUIRE(R >= 1, "%s: sigma %g gives an empty kernel", who, (double)sigma);
    if (R > 8) {
        die_set_error("%s: sigma %g needs radius %d > 8", who, (double)sigma, R);
        return DIE_ERR_UNSUPPORTED;
    }
    // Gᵀ = G: the forward's own sweep on the gradient plane (see the header comment)
    const int rc = die_diffuse_decay(grad_chem_next, grad_chem, W, H, DIE_F32, sigma, decay, stream);
    if (rc != DIE_OK) return rc;
    if (!gather) return DIE_OK;
    const int64_t per_block = (int64_t)DIE_BLOCK * GATHER_PER_THREAD;
    const int64_t g = (N + per_block - 1) / per_block;
    k_gather_cells<<<(int)(g < 8192 ? g : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(grad_chem, (uint32_t)n_cells, cells, N, grad_deposit);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the same for every replica of a die_batch (BatchedEnv.differentiable_step) ------------------------------------------------
// Replica in blockIdx.y; batched agents are in slot order, so entry n's slot id is n.  Both kernels write a replica's whole
// agent_stride row: the padding from n[r] on gets −1 (cells) and 0 (gradient), so a (R, Nmax) tensor needs no clearing.
struct BatchCellsArgs {
    int W, H, epoch;
    int64_t plane_stride, agent_stride;
    const unsigned long long* owner;
    const uint32_t* x;
    const uint32_t* y;
    const uint8_t* alive;
    int32_t* cells;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_deposit_cells_batch(BatchCellsArgs a) {
    const int r = blockIdx.y;
    const int64_t pa = a.agent_stride * r, Nr = a.n[r];
    const unsigned long long* owner = a.owner + a.plane_stride * r;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.agent_stride; n += stride) {
        int32_t out = -1;
        if (n < Nr) {
            const int c = die_cell_u(a.x[pa + n], a.W) * a.H + die_cell_u(a.y[pa + n], a.H);   // < W · H ≤ 2^31 − 1 (checked on the host)
            const bool won = a.alive[pa + n] != 0 && (uint32_t)(owner[c] >> 32) == die_owner_word(a.epoch, n);
            out = won ? c : -1;
        }
        a.cells[pa + n] = out;
    }
}

struct BatchGatherArgs {
    const float* plane;
    const int32_t* cells;
    float* out;
    uint32_t n_cells;
    int64_t plane_stride, agent_stride;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_cells_batch(BatchGatherArgs a) {
    // k_gather_cells for replica blockIdx.y: runs of DIE_BLOCK entries, a thread's four gathers issued before the first is consumed
    const int r = blockIdx.y;
    const float* __restrict__ plane = a.plane + a.plane_stride * r;
    const int32_t* __restrict__ cells = a.cells + a.agent_stride * r;
    float* __restrict__ out = a.out + a.agent_stride * r;
    const int64_t Nr = a.n[r];
    const int64_t stride = (int64_t)gridDim.x * DIE_BLOCK * GATHER_PER_THREAD;
    for (int64_t base = (int64_t)blockIdx.x * DIE_BLOCK * GATHER_PER_THREAD + threadIdx.x; base < a.agent_stride; base += stride) {
        int32_t c[GATHER_PER_THREAD];
        float v[GATHER_PER_THREAD];
#pragma unroll
        for (int q = 0; q < GATHER_PER_THREAD; ++q) {
            const int64_t n = base + (int64_t)q * DIE_BLOCK;
            c[q] = n < Nr ? cells[n] : -1;                                              // (the padding: 0 is stored)
        }
#pragma unroll
        for (int q = 0; q < GATHER_PER_THREAD; ++q) v[q] = (uint32_t)c[q] < a.n_cells ? plane[(uint32_t)c[q]] : 0.f;   // (−1 is 2^32 − 1: out)
#pragma unroll
        for (int q = 0; q < GATHER_PER_THREAD; ++q) {
            const int64_t n = base + (int64_t)q * DIE_BLOCK;
            if (n < a.agent_stride) out[n] = v[q];
        }
    }
}

// the batch's own checks of both calls: 1..DIE_MAX_REPLICAS replicas, planes at least a replica apart
static int batch_planes_check(const die_batch* b, int32_t W, int32_t H, const char* who) {
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas", who, DIE_MAX_REPLICAS);
    DIE_REQUIRE(b->plane_stride >= (int64_t)W * H, "%s: strides smaller than a replica (plane_stride %lld < %dx%d cells)", who,
                (long long)b->plane_stride, W, H);
    return DIE_OK;
}

// … and, where the per-agent arrays are read: rows of agent_stride entries holding 0..agent_stride agents each
static int batch_agents_check(const die_batch* b, const char* who) {
    DIE_REQUIRE(b->agent_stride >= 1 && b->agent_stride <= (int64_t)DIE_OWNER_SLOT_MASK, "%s: bad agent stride %lld", who,
                (long long)b->agent_stride);
    for (int r = 0; r < b->replicas; ++r)
        DIE_REQUIRE(b->n[r] >= 0 && b->n[r] <= b->agent_stride, "%s: replica %d has %lld agents", who, r, (long long)b->n[r]);
    return DIE_OK;
}

extern "C" int die_deposit_cells_batch(const die_medium* m, const die_agents* ag, const die_batch* b, int32_t* cells_out, void* stream) {
    const char* who = "die_deposit_cells_batch";
    DIE_REQUIRE(m && ag && b && cells_out, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    DIE_REQUIRE(m->epoch >= 1 && m->epoch <= DIE_OWNER_EPOCH_MAX, "%s: bad epoch %d", who, m->epoch);
    DIE_REQUIRE(m->owner, "%s: null claim plane", who);
    DIE_REQUIRE(ag->x && ag->y && ag->alive, "%s: bad arrays", who);
    DIE_REQUIRE(!ag->slot, "%s: batched agents are in slot order (a->slot must be NULL)", who);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium (one tile of a %dx%d world) is not supported", who, m->gW, m->gH);
        return DIE_ERR_UNSUPPORTED;
    }
    if ((int64_t)m->W * m->H > (int64_t)INT32_MAX) {
        die_set_error("%s: %dx%d cells do not fit the int32 cell index", who, m->W, m->H);
        return DIE_ERR_UNSUPPORTED;
    }
    int rc = batch_planes_check(b, m->W, m->H, who);
    if (rc != DIE_OK) return rc;
    rc = batch_agents_check(b, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(ag->N >= 0 && ag->N <= b->agent_stride, "%s: strides smaller than a replica (agent_stride %lld < %lld slots)", who,
                (long long)b->agent_stride, (long long)ag->N);
    BatchCellsArgs a;
    a.W = m->W; a.H = m->H; a.epoch = m->epoch; a.plane_stride = b->plane_stride; a.agent_stride = b->agent_stride;
    a.owner = (const unsigned long long*)m->owner;
    a.x = (const uint32_t*)ag->x; a.y = (const uint32_t*)ag->y; a.alive = (const uint8_t*)ag->alive;
    a.cells = cells_out;
    die_replica_counts(a.n, b->n, b->replicas);
    const int64_t g = (b->agent_stride + DIE_BLOCK - 1) / DIE_BLOCK;
    k_deposit_cells_batch<<<dim3((unsigned)(g < 8192 ? g : 8192), (unsigned)b->replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_env_step_backward_batch(int32_t W, int32_t H, const die_batch* b, const float* grad_chem_next, float sigma, float decay,
                                           const die_dynamics_row* rows, const die_dynamics_row* rows_host, const int32_t* cells,
                                           float* grad_chem, float* grad_deposit, void* stream) {
    const char* who = "die_env_step_backward_batch";
    DIE_REQUIRE(b && grad_chem_next && grad_chem, "%s: null argument", who);
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    int rc = batch_planes_check(b, W, H, who);
    if (rc != DIE_OK) return rc;
    const int64_t n_cells = (int64_t)W * H;
    if (n_cells > (int64_t)INT32_MAX) {
        die_set_error("%s: %dx%d cells do not fit the int32 cell index", who, W, H);
        return DIE_ERR_UNSUPPORTED;
    }
    // buffers of the whole batch: the planes' [0, (R − 1) · plane_stride + W · H), the per-agent rows' [0, R · agent_stride)
    const int64_t plane_span = ((int64_t)(b->replicas - 1) * b->plane_stride + n_cells) * 4;
    auto overlap = [](const void* p, int64_t np, const void* q, int64_t nq) {
        return (const char*)p < (const char*)q + nq && (const char*)q < (const char*)p + np;
    };
    DIE_REQUIRE(!overlap(grad_chem, plane_span, grad_chem_next, plane_span), "%s: in-place grad_chem (it may not alias grad_chem_next)", who);
    DIE_REQUIRE(!rows == !rows_host, "%s: one dynamics table without the other (rows and rows_host go together)", who);
    if (H % 4 != 0) {
        die_set_error("%s: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4 (H = %d)", who, H);
        return DIE_ERR_UNSUPPORTED;
    }
    if (rows) {
        for (int r = 0; r < b->replicas; ++r)
            if (rows_host[r].radius < 1 || rows_host[r].radius > 4) {
                die_set_error("%s: row %d has radius %d, outside 1..4", who, r, rows_host[r].radius);
                return DIE_ERR_UNSUPPORTED;
            }
    } else {
        DIE_REQUIRE(sigma > 0.f, "%s: sigma must be positive", who);      // (NaN fails too)
        DIE_REQUIRE(decay == decay, "%s: decay is not a number", who);
        const int R = die_gaussian_radius(sigma);
        if (R < 1 || R > 4) {
            die_set_error("%s: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4 (sigma %g gives radius %d)", who,
                          (double)sigma, R);
            return DIE_ERR_UNSUPPORTED;
        }
    }
    // the sweep loads and stores four cells of a row at once
    DIE_REQUIRE(b->plane_stride % 4 == 0 && ((uintptr_t)grad_chem_next & 15) == 0 && ((uintptr_t)grad_chem & 15) == 0,
                "%s: the planes must be 16-byte aligned (plane_stride %lld a multiple of 4)", who, (long long)b->plane_stride);
    if (grad_deposit) {
        DIE_REQUIRE(cells, "%s: null cells", who);
        rc = batch_agents_check(b, who);
        if (rc != DIE_OK) return rc;
        const int64_t agent_span = (int64_t)b->replicas * b->agent_stride * 4;
        DIE_REQUIRE(!overlap(grad_deposit, agent_span, grad_chem, plane_span) && !overlap(grad_deposit, agent_span, grad_chem_next, plane_span) &&
                        !overlap(grad_deposit, agent_span, cells, agent_span),
                    "%s: in-place grad_deposit", who);
    }
    // Gᵀ = G: the forward's own sweep on the gradient planes (see the header comment)
    rc = die_diffuse_rows_batch(grad_chem_next, grad_chem, W, H, b->replicas, b->plane_stride, sigma, decay, rows, rows_host, stream, who);
    if (rc != DIE_OK || !grad_deposit) return rc;
    BatchGatherArgs a;
    a.plane = grad_chem; a.cells = cells; a.out = grad_deposit; a.n_cells = (uint32_t)n_cells;
    a.plane_stride = b->plane_stride; a.agent_stride = b->agent_stride;
    die_replica_counts(a.n, b->n, b->replicas);
    const int64_t per_block = (int64_t)DIE_BLOCK * GATHER_PER_THREAD;
    const int64_t g = (b->agent_stride + per_block - 1) / per_block;
    k_gather_cells_batch<<<dim3((unsigned)(g < 8192 ? g : 8192), (unsigned)b->replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}
