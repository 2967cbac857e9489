// The 'agent_food' observation channel of a NeuralAutomataAgent (gfx950): a plane that holds, on every cell, the stock of the
// agent standing there (no reference counterpart: core/agent/evo.py "agents should have access to their own
// resource stock").
//
//   k_stock_plane   one thread per slot of replica blockIdx.y.  An alive slot issues ONE 64-bit atomicMax of
//                   die_claim(epoch, slot id, float bits of agent_food) on its cell — the claim plane's own word with the stock in
//                   place of the deposit (die_env.hip: "an atomicMax on the slot id").  Where several alive agents share a cell the
//                   highest slot id wins, whatever order the arrays are stored in (slot ? slot[n] : n) and whatever order the
//                   waves run in: integer max, no float atomics, the same bits on every run.  Dead slots and a replica's padding
//                   slots n >= n[r] write nothing.
//
// The conv loaders read such a plane as DIE_PLANE_STOCK (die_nca.h nca_load): occupied at the call's epoch ? the payload : 0.
// The build does NOT clear: it needs a plane that is zero or holds only tags of earlier epochs of the same 1..31 cycle (an older
// tag loses every atomicMax against the build's and reads as empty afterwards).  The owners of the planes see to that:
// NeuralAutomataAgent and BatchedEnv zero a plane whose last build was not at a smaller epoch, and the batched step clears the
// stock planes with the claim planes on the epoch wrap.
//
// Roofline: latency.  One launch of N threads, 13 bytes read and one 8-byte atomic per alive slot: at 10 x 96^2 worlds a few
// thousand atomics, far below anything the memory system notices; the launch itself is the cost.
#include "die_common.h"
#include "die_nca.h"

struct StockArgs {
    const uint32_t *x, *y, *slot;
    const uint8_t* alive;
    const float* agent_food;
    unsigned long long* plane;
    int W, H, epoch;
    int64_t agent_stride, plane_stride;      // replica r's slots / plane start r strides on
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_stock_plane(StockArgs a) {
    const int r = blockIdx.y;
    const int64_t nr = a.n[r], base = a.agent_stride * r;
    unsigned long long* plane = a.plane + a.plane_stride * r;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < nr; n += stride) {
        const int64_t i = base + n;
        if (!a.alive[i]) continue;
        const int64_t c = (int64_t)die_cell_u(a.x[i], a.W) * a.H + die_cell_u(a.y[i], a.H);      // (always inside the plane)
        atomicMax(&plane[c], die_claim(a.epoch, a.slot ? (int64_t)a.slot[i] : n, a.agent_food[i]));
    }
}

// the launch alone: every argument has been checked by the caller (the entry points below, the batched steps of die_env.hip)
int die_stock_launch(const die_medium* m, const die_agents* a, int32_t replicas, const int64_t* n, int64_t agent_stride,
                     int64_t plane_stride, int32_t epoch, unsigned long long* planes, void* stream, const char* who) {
    StockArgs k;
    k.x = a->x; k.y = a->y; k.slot = a->slot; k.alive = a->alive; k.agent_food = a->agent_food;
    k.plane = planes; k.W = m->W; k.H = m->H; k.epoch = epoch;
    k.agent_stride = agent_stride; k.plane_stride = plane_stride;
    const int64_t nmax = die_replica_counts(k.n, n, replicas);
    if (nmax == 0) return DIE_OK;                        // no slot anywhere: the planes stay as they are
    const int64_t g = (nmax + DIE_BLOCK - 1) / DIE_BLOCK;
    k_stock_plane<<<dim3((unsigned)(g < 8192 ? g : 8192), (unsigned)replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

static int stock_check(const die_medium* m, const die_agents* a, int32_t epoch, const unsigned long long* planes, const char* who) {
    DIE_REQUIRE(m && a && planes, "%s: null argument", who);
    DIE_REQUIRE(a->x && a->y && a->alive && a->agent_food, "%s: null agent array", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium has no stock plane (periodic single-tile planes only)", who);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(epoch >= 1 && epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, epoch, DIE_OWNER_EPOCH_MAX);
    return DIE_OK;
}

extern "C" int die_stock_plane(const die_medium* m, const die_agents* agents, int32_t epoch, unsigned long long* plane, void* stream) {
    const char* who = "die_stock_plane";
    const int rc = stock_check(m, agents, epoch, plane, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(agents->N >= 0 && agents->N <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: %lld slots outside 0..%lld", who, (long long)agents->N,
                (long long)DIE_OWNER_SLOT_MASK - 1);
    return die_stock_launch(m, agents, 1, &agents->N, 0, 0, epoch, plane, stream, who);
}

extern "C" int die_stock_plane_batch(const die_medium* m, const die_agents* agents, const die_batch* b, int32_t epoch,
                                     unsigned long long* planes, void* stream) {
    const char* who = "die_stock_plane_batch";
    DIE_REQUIRE(b, "%s: null argument", who);
    int rc = stock_check(m, agents, epoch, planes, who);
    if (rc != DIE_OK) return rc;
    rc = die_batch_check(b, (int64_t)m->W * m->H, who);
    if (rc != DIE_OK) return rc;
    return die_stock_launch(m, agents, b->replicas, b->n, b->agent_stride, b->plane_stride, epoch, planes, stream, who);
}
