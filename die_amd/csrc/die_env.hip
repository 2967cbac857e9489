// Env.step kernels (gfx950) — core/env.py:101-131.
//
//   k_move_claim   _agent_move (:163-172) + ownership claim for _agent_deposit_and_layout (:204-215)
//                  + _agent_feed (:220-243) for alive slots (their own cell is occupied by definition)
//   k_resolve      winner of each occupied cell writes chem += deposit and food -= rate·food;
//                  dead slots finish their feed (they consume iff somebody alive owns their cell);
//                  _agent_lifecycle (:245-261) when agents_die; alive count
//   k_reduce       fixed-order sum of the per-block partials → die_step_result (deterministic)
//   k_diffuse      _medium_diffuse_decay (:136-145): separable gaussian, periodic, × (1 − decay)
//   k_lifecycle_batch  k_resolve's dead-slot + lifecycle work for R replicas (blockIdx.y) when agents_die: dead-slot feed from the
//                  claim pass's stash (consumed and action cost), starved slots zeroed, alive count per replica
//   k_nca_move_claim_batch  a NeuralAutomataAgent population (die_nca_env_step_batch): every agent reads its action out of
//                  its candidate's last conv planes (die_gather_scale's product, in registers), then k_move_claim's work
//   k_action_move_claim_batch  the caller's own actions (die_env_step_batch): three coalesced loads per slot instead of a forward, then
//                  k_move_claim's work — BatchedEnv.step_action, the step under BatchedEnv.differentiable_step
//
// Why two agent passes: every slot on a cell must read the food value from BEFORE the step's
// consumption (co-located agents each get the full amount, :224-225), so all reads of `food`
// (pass 1) are separated from the single write per occupied cell (pass 2) by a kernel boundary.
// "Last writer wins" of the fancy-index assignment at :211 is an atomicMax on the slot id.
#include "die_forward.h"
#include "die_nca.h"

#define DIE_MAX_PARTIALS 8192
// workgroup size of the per-agent step kernels (claim pass, dead-slot pass).  Swept on MI355X at 2.5 M agents, step time in
// µs: 192: 211.5, 256: 206.6, 320: 199.9, 384: 203.4, 448: 204.5, 512: 202.8, 640: 208.0, 768: 201.8 — 5 waves per
// workgroup it is (one agent per thread under the 8192-workgroup cap, and 20 instead of 24 waves per CU: the kernel
// is bound by L1 misses in flight, fewer waves thrash the L1 less).
#define DIE_STEP_BLOCK 320

struct StepArgs {
    die_geo g;
    int epoch;
    int do_move, do_claim;     // die_agent_move / die_agent_claim_feed run one half each
    int tile_w, tile_h, tiles_y;
    int32_t* tile_of;
    int64_t N;
    unsigned long long* owner;
    void* food;
    void* chem;
    uint32_t* x;
    uint32_t* y;
    const uint32_t* slot;  // reference slot ids (NULL = identity)
    uint8_t* alive;
    float* agent_food;
    const float* dx;
    const float* dy;
    const float* dep;
    float rate_feed, w_dep, w_dist;
    int boundary, cost, food_infinite, agents_die, has_dead;
    int skip_scatter;      // fused step: the winner's chem/food writes are done by k_diffuse_rows
    float* stash;          // N floats, only when has_dead
    float* stash_cost;     // batched lifecycle: the dead slots' action_cost next to `stash` (their actions stay in registers)
    long long* part_gain;  // gridDim.x fixed-point sums (die_fix)
    long long* part_alive; // gridDim.x
};

__device__ __forceinline__ float action_cost(const StepArgs& a, float dx, float dy, float dep) {
    // linear_action_cost (core/env.py:29-35) or zero_cost (:38-39)
    return a.cost == DIE_COST_LINEAR ? a.w_dep * fabsf(dep) + a.w_dist * die_sqrt1(dx * dx + dy * dy) : 0.f;
}

__device__ __forceinline__ void block_sum_store(long long g, long long c, long long* pg, long long* pc) {
    __shared__ long long sg[DIE_STEP_BLOCK / DIE_WAVE];
    __shared__ long long sc[DIE_STEP_BLOCK / DIE_WAVE];
    g = die_wave_sum(g);
    c = die_wave_sum(c);
    const int lane = threadIdx.x & (DIE_WAVE - 1), wv = threadIdx.x / DIE_WAVE;
    if (lane == 0) { sg[wv] = g; sc[wv] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tg = 0;
        long long tc = 0;
        for (int i = 0; i < DIE_STEP_BLOCK / DIE_WAVE; ++i) { tg += sg[i]; tc += sc[i]; }
        if (pg) pg[blockIdx.x] = tg;
        if (pc) pc[blockIdx.x] = tc;
    }
}

// One slot of _agent_move + claim + _agent_feed (alive slots); returns its `gained` (0 for dead slots).
template <typename T, bool EXT = true>
__device__ __forceinline__ float move_claim_one(const StepArgs& a, const int64_t n, uint32_t X, uint32_t Y, const float dx,
                                                const float dy, const float dep, const uint32_t sid, long long& owned_alive) {
    const T* food = (const T*)a.food;
    const die_geo g = a.g;
    if (a.do_move) {
        if (a.boundary == DIE_BOUNDARY_WRAP) {            // (xy + dxdy) % 1.
            X += (uint32_t)die_q32(dx);
            Y += (uint32_t)die_q32(dy);
        } else {                                          // clip(0, 1); 1.0 is held as 2^32 − 1
            int64_t px = (int64_t)X + die_q32(dx), py = (int64_t)Y + die_q32(dy);
            X = (uint32_t)(px < 0 ? 0 : (px > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : px));
            Y = (uint32_t)(py < 0 ? 0 : (py > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : py));
        }
        a.x[n] = X;
        a.y[n] = Y;
    }
    const int cx = die_cell((int64_t)X, g.gW), cy = die_cell((int64_t)Y, g.gH);
    if (a.tile_of) a.tile_of[n] = (cx / a.tile_w) * a.tiles_y + cy / a.tile_h;
    if (!a.do_claim) return 0.f;
    const int64_t c = die_local(g, cx, cy);
    const float consumed = a.rate_feed * die_ld(food, c);
    if (a.alive[n]) {
        // Claim: one 64-bit atomicMax (a plain store + a repair pass was measured: 70 + 38 µs against 105 µs, no gain)
        atomicMax(&a.owner[c], die_claim(a.epoch, (int64_t)sid, dep));
        const float gained = consumed - action_cost(a, dx, dy, dep);
        a.agent_food[n] += gained;
        if (EXT) {                                     // ghost-agent tiles (compiled out of the single-tile kernel)
            if (!die_owned(g, cx, cy)) return 0.f;     // a ghost: the rank that owns this cell accounts for it
            ++owned_alive;
        }
        return gained;
    }
    if (a.has_dead) {
        a.stash[n] = consumed;
        if (a.stash_cost) a.stash_cost[n] = action_cost(a, dx, dy, dep);   // the same ops k_resolve performs on the stored action
    }
    return 0.f;
}

template <typename T>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_move_claim(StepArgs a) {
    long long gsum = 0;
    long long cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) {
        const uint32_t sid = a.slot ? a.slot[n] : (uint32_t)n;
        gsum += die_fix(move_claim_one<T>(a, n, a.x[n], a.y[n], a.dx[n], a.dy[n], a.do_claim ? a.dep[n] : 0.f, sid, cnt));
    }
    if (a.do_claim) block_sum_store(gsum, cnt, a.part_gain, a.part_alive);
}

// Agent.forward fused with the first half of Env.step: the action stays in registers between the two
// (it is still written out for the caller, but never read back), x / y / slot are loaded once.
template <typename T, int KIND, bool EXT>
__device__ __forceinline__ void forward_move_claim_body(FwdArgs& f, StepArgs& a) {
    long long gsum = 0;
    long long cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // (giving every XCD a contiguous eighth of the sorted array instead of round-robin workgroups: 178 µs vs 122 µs)
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) {
        const uint32_t sid = a.slot ? a.slot[n] : (uint32_t)n;
        const uint32_t X = a.x[n], Y = a.y[n];
        const FwdOut o = die_forward_agent<T, KIND, EXT>(f, X, Y, die_heading_ld(f.heading_hi, f.heading_lo, n), sid, n);
        die_heading_st(f.heading_hi, f.heading_lo, n, o.heading);
        if (f.dx) { f.dx[n] = o.dx; f.dy[n] = o.dy; f.dep[n] = o.dep; }
        gsum += die_fix(move_claim_one<T, EXT>(a, n, X, Y, o.dx, o.dy, o.dep, sid, cnt));
    }
    if (a.do_claim) block_sum_store(gsum, cnt, a.part_gain, a.part_alive);
}

// Agent.forward fused with the first half of Env.step: the action stays in registers between the two
// (it is still written out for the caller, but never read back), x / y / slot are loaded once.
// LEAN: the host has checked that the agent has no momentum, no noise, a normalised gradient and no graph-replay step
// word (PhysarumAgent's defaults) — spelled out for the compiler, those paths of the shared forward code and the scalar
// registers that feed them drop out of the kernel (die_pic.hip: −30 % vector instructions, −4 % time).
__device__ __forceinline__ void fwd_args_lean(FwdArgs& f) {
    f.pgx = nullptr; f.pgy = nullptr; f.step_base = nullptr;
    f.inertia = 0.f; f.noise_scale = 0.f; f.normalized = 1;
}
static bool fwd_is_lean(const die_gradient_agent* g) {
    return g->kind == DIE_AGENT_PHYSARUM && g->inertia == 0.f && g->noise_scale == 0.f && g->normalized_grad && !g->prev_gx && !g->prev_gy &&
           !g->step_base;
}

template <typename T, int KIND, bool EXT = true, bool LEAN = false>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_forward_move_claim(FwdArgs f, StepArgs a) {
    if (LEAN) fwd_args_lean(f);
    forward_move_claim_body<T, KIND, EXT>(f, a);
}

// R replicas of one world shape in one launch (blockIdx.y = replica): every array of replica r lies `r` strides behind
// replica 0's, the Philox key is seed + r·seed_stride, its agent count n[r] — otherwise the kernel above.
struct BatchArgs {
    int64_t cells, agents;          // strides: cells per plane, agent slots per replica
    uint64_t seed_stride;
    int64_t n[DIE_MAX_REPLICAS];
};

// replica r's alive-count partials and dead-slot stash.  Without dead slots the claim pass writes the count partials; with
// them the lifecycle pass (k_lifecycle_batch) does, and the claim pass stashes each dead slot's `consumed` and action cost in
// replica r's [consumed | cost] pair of agent_stride floats (a.stash: replica 0's, behind the partials of every replica)
__device__ __forceinline__ void batch_stash(StepArgs& a, const BatchArgs& b, int r) {
    a.part_alive = a.has_dead ? nullptr : a.part_gain + 2 * DIE_MAX_PARTIALS;
    if (a.has_dead) {
        a.stash += 2 * b.agents * r;
        a.stash_cost = a.stash + b.agents;
    }
}

// Per-replica Dynamics (die_*_env_step_batch_rows): the batched claim kernels take the device table of die_dynamics_row as an
// optional last argument (`ROWS...`: nothing, or `const die_dynamics_row*`).  Given, replica r's row is fetched once per
// workgroup ahead of the loop — uniform and read-only, so scalar loads, as k_physarum_move_claim_batch reads its table —
// into the by-value StepArgs, so the loop body is the instruction stream of the shared-Dynamics kernel; not given, the kernel is
// the shared-Dynamics kernel itself.  (The claim pass reads rate_feed only; k_lifecycle_batch reads neither, so it takes no row.)
__device__ __forceinline__ void dynamics_row_args(StepArgs&, int) {}
__device__ __forceinline__ void dynamics_row_args(StepArgs& a, const int r, const die_dynamics_row* __restrict__ rows) {
    const die_dynamics_row row = rows[r];
    a.rate_feed = row.rate_feed; a.food_infinite = row.food_infinite;
}

// replica r's arrays, agent count, Philox key and workspace partials
template <typename T>
__device__ __forceinline__ void batch_replica_args(FwdArgs& f, StepArgs& a, const BatchArgs& b, const int r) {
    const int64_t pc = b.cells * r, pa = b.agents * r;
    f.chem = (const T*)f.chem + pc; f.food = (const T*)f.food + pc;
    f.x += pa; f.y += pa; f.heading_hi += pa; f.heading_lo += pa;
    if (f.slot) f.slot += pa;
    if (f.dx) { f.dx += pa; f.dy += pa; f.dep += pa; }
    f.N = b.n[r]; f.seed += b.seed_stride * (uint64_t)r;
    a.owner += pc; a.food = (T*)a.food + pc; a.chem = (T*)a.chem + pc;
    a.x += pa; a.y += pa; a.alive += pa; a.agent_food += pa;
    if (a.slot) a.slot += pa;
    a.N = b.n[r];
    a.part_gain += (int64_t)DIE_MAX_PARTIALS * 3 * r;               // replica r's own workspace partials
    batch_stash(a, b, r);
}

template <typename T, int KIND, bool LEAN = false, typename... ROWS>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_forward_move_claim_batch(FwdArgs f, StepArgs a, BatchArgs b, ROWS... rows) {
    if (LEAN) fwd_args_lean(f);
    const int r = blockIdx.y;
    dynamics_row_args(a, r, rows...);
    batch_replica_args<T>(f, a, b, r);
    forward_move_claim_body<T, KIND, false>(f, a);
    // every slot is alive: the sweep's reduction reads the count here (with dead slots, k_lifecycle_batch counts them)
    if (!a.has_dead && blockIdx.x == 0 && threadIdx.x == 0) a.part_alive[0] = a.N;
}

// A PhysarumAgent population (die_physarum_env_step_batch): the kernel above, replica r stepping with row r of the table in
// place of the shared scale / deposit / sense_offset / angles / tolerance and the constants derived from them.  The row is
// uniform over the workgroup and read-only: one 64-byte scalar load into the by-value FwdArgs, ahead of the loop, so the
// loop reads the same scalar registers it reads in the shared-parameter kernel.
template <typename T, bool LEAN, typename... ROWS>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_physarum_move_claim_batch(FwdArgs f, StepArgs a, BatchArgs b,
                                                                              const die_physarum_row* __restrict__ table, ROWS... rows) {
    if (LEAN) fwd_args_lean(f);
    const int r = blockIdx.y;
    const die_physarum_row row = table[r];
    f.scale = row.scale; f.deposit = row.deposit; f.sense_offset = row.sense_offset;
    f.turn_rad = row.turn_radians; f.sense_rad = row.sense_radians; f.rtol = row.turn_tolerance;
    f.x_turn = row.x_turn; f.atol = row.atol; f.c_turn = row.c_turn; f.c_sense = row.c_sense;
    dynamics_row_args(a, r, rows...);
    batch_replica_args<T>(f, a, b, r);
    forward_move_claim_body<T, DIE_AGENT_PHYSARUM, false>(f, a);
    if (!a.has_dead && blockIdx.x == 0 && threadIdx.x == 0) a.part_alive[0] = a.N;
}

// NeuralAutomataAgent population (die_nca_env_step_batch): replica r's agents read their action out of the last layer's
// planes of candidate r — die_gather_scale's product, kept in registers — then k_forward_move_claim_batch's step half.
struct NcaReadArgs {
    const float* sense;            // replica 0's (dx, dy, deposit) planes, `cells` apart; replica r's `rep` further
    int64_t cells, rep;
    float coef[3];
    float* act[3];                 // replica 0's action arrays (agent_stride apart), or NULL
};

template <typename T, typename... ROWS>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_nca_move_claim_batch(NcaReadArgs q, StepArgs a, BatchArgs b, ROWS... rows) {
    const int r = blockIdx.y;
    dynamics_row_args(a, r, rows...);
    const int64_t pc = b.cells * r, pa = b.agents * r;
    a.owner += pc; a.food = (T*)a.food + pc; a.chem = (T*)a.chem + pc;
    a.x += pa; a.y += pa; a.alive += pa; a.agent_food += pa;
    a.N = b.n[r];
    a.part_gain += (int64_t)DIE_MAX_PARTIALS * 3 * r;
    batch_stash(a, b, r);
    const float* s0 = q.sense + q.rep * r;
    const float* s1 = s0 + q.cells;
    const float* s2 = s1 + q.cells;
    long long gsum = 0;
    long long cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) {
        const uint32_t X = a.x[n], Y = a.y[n];
        const int64_t c = die_local(a.g, die_cell((int64_t)X, a.g.gW), die_cell((int64_t)Y, a.g.gH));
        const float dx = s0[c] * q.coef[0];
        const float dy = s1[c] * q.coef[1];
        const float dep = s2[c] * q.coef[2];
        if (q.act[0]) { q.act[0][pa + n] = dx; q.act[1][pa + n] = dy; q.act[2][pa + n] = dep; }
        gsum += die_fix(move_claim_one<T, false>(a, n, X, Y, dx, dy, dep, (uint32_t)n, cnt));
    }
    block_sum_store(gsum, cnt, a.part_gain, a.part_alive);
    if (!a.has_dead && blockIdx.x == 0 && threadIdx.x == 0) a.part_alive[0] = a.N;  // every slot is alive (as k_forward_move_claim_batch)
}

// The caller's own actions (die_env_step_batch): k_nca_move_claim_batch with the three plane gathers replaced by three coalesced
// loads of replica r's slot n (StepArgs' dx / dy / dep are replica 0's arrays, `agents` apart).  Agents in slot order.
template <typename T, typename... ROWS>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_action_move_claim_batch(StepArgs a, BatchArgs b, ROWS... rows) {
    const int r = blockIdx.y;
    dynamics_row_args(a, r, rows...);
    const int64_t pc = b.cells * r, pa = b.agents * r;
    a.owner += pc; a.food = (T*)a.food + pc; a.chem = (T*)a.chem + pc;
    a.x += pa; a.y += pa; a.alive += pa; a.agent_food += pa;
    a.N = b.n[r];
    a.part_gain += (int64_t)DIE_MAX_PARTIALS * 3 * r;
    batch_stash(a, b, r);
    long long gsum = 0;
    long long cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) {
        const uint32_t X = a.x[n], Y = a.y[n];
        const float dx = a.dx[pa + n];
        const float dy = a.dy[pa + n];
        const float dep = a.dep[pa + n];
        gsum += die_fix(move_claim_one<T, false>(a, n, X, Y, dx, dy, dep, (uint32_t)n, cnt));
    }
    block_sum_store(gsum, cnt, a.part_gain, a.part_alive);
    if (!a.has_dead && blockIdx.x == 0 && threadIdx.x == 0) a.part_alive[0] = a.N;  // every slot is alive (as k_forward_move_claim_batch)
}

template <typename T>
__device__ __forceinline__ void resolve_body(const StepArgs& a) {
    T* food = (T*)a.food;
    T* chem = (T*)a.chem;
    long long gsum = 0;
    long long alive_cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) {
        const uint32_t X = a.x[n], Y = a.y[n];
        const int cx = die_cell((int64_t)X, a.g.gW), cy = die_cell((int64_t)Y, a.g.gH);
        const int64_t c = die_local(a.g, cx, cy);
        const bool owned = die_owned(a.g, cx, cy);
        bool alive = a.alive[n] != 0;
        if (alive && !a.skip_scatter) {
            if ((uint32_t)(a.owner[c] >> 32) == die_owner_word(a.epoch, a.slot ? (int64_t)a.slot[n] : n)) {       // highest alive slot on the cell
                die_st(chem, c, die_ld(chem, c) + a.dep[n]);
                if (!a.food_infinite) {
                    const float f = die_ld(food, c);
                    die_st(food, c, f - a.rate_feed * f);
                }
            }
        } else if (!alive && a.has_dead) {
            const float consumed = die_claim_occupied(a.owner[c], a.epoch) ? a.stash[n] : 0.f;
            const float gained = consumed - (a.stash_cost ? a.stash_cost[n] : action_cost(a, a.dx[n], a.dy[n], a.dep[n]));
            a.agent_food[n] += gained;
            if (owned) gsum += die_fix(gained);
        }
        if (a.agents_die && !(a.agent_food[n] > 1e-4f)) {         // where(have_food, 0): every channel
            a.x[n] = 0; a.y[n] = 0; a.alive[n] = 0; a.agent_food[n] = 0.f;
            alive = false;
        }
        alive_cnt += (alive && owned) ? 1 : 0;
    }
    block_sum_store(gsum, alive_cnt, a.part_gain, a.part_alive);
}

template <typename T>
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_resolve(StepArgs a) { resolve_body<T>(a); }

// die_agent_dead_slots of R replicas in one launch (blockIdx.y = replica, the claim pass's x-grid): dead slots finish their
// feed from the claim pass's stash, _agent_lifecycle, alive count.  Replica r's dead-slot gains go to its second partial array,
// its counts to the third (the batched sweep's reduction sums both gain arrays).  No plane is written (skip_scatter).
__global__ __launch_bounds__(DIE_STEP_BLOCK) void k_lifecycle_batch(StepArgs a, BatchArgs b) {
    const int r = blockIdx.y;
    const int64_t pa = b.agents * r;
    a.owner += b.cells * r;
    a.x += pa; a.y += pa; a.alive += pa; a.agent_food += pa;
    a.N = b.n[r];
    a.part_gain += (int64_t)DIE_MAX_PARTIALS * 3 * r;
    batch_stash(a, b, r);
    a.part_gain += DIE_MAX_PARTIALS;
    a.part_alive = a.part_gain + DIE_MAX_PARTIALS;
    resolve_body<float>(a);          // (skip_scatter: the planes' dtype is never touched)
}

__global__ __launch_bounds__(1024) void k_reduce(const long long* pa, int na, const long long* pb, int nb,
                                                  const long long* pc, int nc, die_step_result* out,
                                                  long long alive_const) {
    // one block; integer sums (fixed-point gains, counts): exact in any order
    __shared__ long long sg[1024];
    __shared__ long long sc[1024];
    long long g = 0;
    long long c = 0;
    for (int i = threadIdx.x; i < na; i += 1024) g += pa[i];
    for (int i = threadIdx.x; i < nb; i += 1024) g += pb[i];
    for (int i = threadIdx.x; i < nc; i += 1024) c += pc[i];
    sg[threadIdx.x] = g;
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sg[threadIdx.x] += sg[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {         // (`out` may be pinned host memory a sync=True caller polls: die_common.h die_store_result_*)
        die_store_result_f64(&out->reward, (double)sg[0] / DIE_FIX_ONE);
        die_store_result_i64((long long*)&out->num_alive, alive_const >= 0 ? alive_const : sc[0]);
    }
}

// ---- diffusion --------------------------------------------------------------------------
// What the two kernels share with die_signal.hip's twins is die_diffuse.h (argument structs, edge rules, 16-byte accessors) and the
// two sweeps' text, die_diffuse_tile.inc / die_diffuse_rows.inc; here a cell is read as the plane holds it.
// ---- row-marching diffusion, optionally fused with deposit + feeding -----------------------
// One wave owns a strip of 248 columns (62 lanes × 4 contiguous cells; lanes 0 and 63 only load
// the 4-column halo to the left / right) and marches down DIF_ROWS rows.  Per row a lane loads its
// 4 cells with one 16-byte access, keeps the last 2R+1 rows in registers (x pass = axis 0 first,
// as scipy does), and gets the y-pass neighbours from the adjacent lanes with wave shuffles — no
// LDS, no barrier.  FUSED: the same sweep reads the 64-bit claim of every cell it loads and adds the
// winner's deposit before filtering (core/env.py:211) and, for the cells it owns, performs the
// feeding update food −= rate·food on occupied cells (:222-228): the per-cell scatter of the step
// becomes two coalesced streams.
#define DIF_ROWS 16     // rows per wave: 16 → ≈17 waves per CU at 4096² (32: 87 µs, 16: 75 µs, 8: 86 µs for the fused sweep)
#define DIF_WCOLS 248          // output columns per wave
#define DIF_BLOCK 128          // waves are independent (no LDS, no barrier): small workgroups balance better

#include "die_diffuse.h"

// LDS-tiled separable gaussian on the torus: the (TX+2R)×(TY+2R) input tile is staged once,
// filtered along x (axis 0, as scipy does first) into a second LDS plane, then along y.
template <typename T, int R>
__global__ __launch_bounds__(DIE_BLOCK) void k_diffuse(DiffuseArgs a) {
#define DIF_LOAD(src, i) die_ld(src, i)
#include "die_diffuse_tile.inc"
#undef DIF_LOAD
}

template <typename T, int R, int FUSED, bool WRAP, typename... TABLE>
__global__ __launch_bounds__(DIF_BLOCK) void k_diffuse_rows(RowsArgs a, TABLE... table) {
    static_assert(R >= 1 && R <= 4, "one halo lane of 4 columns per side");
    const unsigned z = rows_replica(a, R, table...);        // the replica of a batch this workgroup sweeps
    if (sizeof...(TABLE) > 0 || gridDim.z > 1) {            // replica z of a batch: same shape, arrays one stride apart
        const int64_t pc = a.rep_cells * z;
        a.src = (const T*)a.src + pc; a.dst = (T*)a.dst + pc;
        if (FUSED == 1) a.claim += pc;
        if (FUSED) a.food = (T*)a.food + pc;
        if (a.result) {
            a.part_gain += (int64_t)DIE_MAX_PARTIALS * 3 * z;
            if (a.part_gain2) a.part_gain2 += (int64_t)DIE_MAX_PARTIALS * 3 * z;
            if (a.part_alive) a.part_alive += (int64_t)DIE_MAX_PARTIALS * 3 * z;
            a.result += z;
        }
    }
    const int row0 = FUSED && a.result ? 1 : 0;             // grid rows ahead of the field's
    if (row0 && blockIdx.y == 0) {
        // an extra row of workgroups ahead of the field: (0, 0) reduces, the others have nothing to do.  (Doing it as a
        // prologue of a field workgroup made the whole sweep 10 µs longer: all its workgroups are resident at once, so
        // the kernel ends when its slowest workgroup does.)  The FIRST row since round 5: the reduction depends on the claim
        // pass only, and dispatched first it hands the step's result to an Env(sync=True) caller (pinned host memory) while
        // the field is still being swept — the caller's next launches are queued before this kernel ends (die_pic.hip's field
        // kernel does the same).
        if (blockIdx.x != 0) return;
        __shared__ long long s_g[DIF_BLOCK];
        // 8 loads in flight per thread: this workgroup must not outlast the sweep (one load at a time it took ≈ 45 µs per
        // array, and with the second array of ghost tiles it made the whole launch 100 µs instead of 71)
        auto strided_sum = [&](const long long* p) {
            long long t = 0;
            for (int base = threadIdx.x; base < a.n_part; base += DIF_BLOCK * 8) {
                long long v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { const int i = base + q * DIF_BLOCK; v[q] = i < a.n_part ? p[i] : 0; }
#pragma unroll
                for (int q = 0; q < 8; ++q) t += v[q];
            }
            return t;
        };
        long long g = strided_sum(a.part_gain);                    // fixed point: any order
        if (FUSED == 1 && a.part_gain2) g += strided_sum(a.part_gain2);      // (batched replicas only)
        s_g[threadIdx.x] = g;
        __syncthreads();
        for (int o = DIF_BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s_g[threadIdx.x] += s_g[threadIdx.x + o];
            __syncthreads();
        }
        long long cnt = 0;
        if (a.part_alive) {                                    // integer sum: any order
            __shared__ long long s_c[DIF_BLOCK];
            cnt = strided_sum(a.part_alive);
            s_c[threadIdx.x] = cnt;
            __syncthreads();
            for (int o = DIF_BLOCK / 2; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) s_c[threadIdx.x] += s_c[threadIdx.x + o];
                __syncthreads();
            }
            cnt = s_c[0];
        }
        if (threadIdx.x == 0) {
            die_store_result_f64(&a.result->reward, (double)s_g[0] / DIE_FIX_ONE);
            die_store_result_i64((long long*)&a.result->num_alive, a.part_alive ? cnt : a.alive_const);
        }
        return;
    }
#define DIF_EMIT(off, v)
#include "die_diffuse_rows.inc"
#undef DIF_EMIT
}

// A wave marches down its rows one dependent load at a time (one row of prefetch): on a large field the other waves of
// the CU hide that, on a small one the chain IS the kernel (256²: 20 iterations ≈ 21 µs).  Fewer rows per wave there:
// more, shorter waves (each re-reads 2R halo rows, which costs nothing when the field fits the L2).  Same bits.
static int rows_per_wave(int W, int H, int replicas) {
    const int64_t cells = (int64_t)W * H * replicas;
    return cells >= (1ll << 23) ? DIF_ROWS : cells >= (1ll << 21) ? 8 : cells >= (1ll << 19) ? 4 : 2;
}

template <typename T, int FUSED, bool WRAP = true>
static int launch_rows(RowsArgs a, int R, hipStream_t s, int replicas = 1) {
    const int strips = (a.H + DIF_WCOLS - 1) / DIF_WCOLS;
    constexpr int WPB = DIF_BLOCK / DIE_WAVE;
    a.rpw = rows_per_wave(a.W, a.H, replicas);
    dim3 grid((strips + WPB - 1) / WPB, (a.W + a.rpw - 1) / a.rpw + (FUSED && a.result ? 1 : 0), replicas);
    switch (R) {
        case 1: k_diffuse_rows<T, 1, FUSED, WRAP><<<grid, DIF_BLOCK, 0, s>>>(a); break;
        case 2: k_diffuse_rows<T, 2, FUSED, WRAP><<<grid, DIF_BLOCK, 0, s>>>(a); break;
        case 3: k_diffuse_rows<T, 3, FUSED, WRAP><<<grid, DIF_BLOCK, 0, s>>>(a); break;
        case 4: k_diffuse_rows<T, 4, FUSED, WRAP><<<grid, DIF_BLOCK, 0, s>>>(a); break;
        default: return DIE_ERR_UNSUPPORTED;
    }
    return DIE_OK;
}

int die_rows_per_wave(int W, int H, int planes) { return rows_per_wave(W, H, planes); }      // (die_signal.hip's launch of the same sweep)

static int gaussian_taps(float sigma, double* w) {
    // scipy.ndimage._gaussian_kernel1d: radius int(4σ + .5), exp(−x²/2σ²) normalised
    const int R = die_gaussian_radius(sigma);
    double sum = 0.0;
    for (int k = -R; k <= R && R <= DIF_MAXR; ++k) { w[k + R] = exp(-0.5 / ((double)sigma * (double)sigma) * k * k); sum += w[k + R]; }
    for (int k = 0; k <= 2 * R && R <= DIF_MAXR; ++k) w[k] /= sum;
    return R;
}

int die_gaussian_taps(float sigma, double* w) { return gaussian_taps(sigma, w); }      // (die_pic.hip)

template <typename T>
static int launch_diffuse(const DiffuseArgs& a, int R, hipStream_t s) {
    dim3 grid((a.H + DIF_TY - 1) / DIF_TY, (a.W + DIF_TX - 1) / DIF_TX);
    switch (R) {
        case 1: k_diffuse<T, 1><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 2: k_diffuse<T, 2><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 3: k_diffuse<T, 3><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 4: k_diffuse<T, 4><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 5: k_diffuse<T, 5><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 6: k_diffuse<T, 6><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 7: k_diffuse<T, 7><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 8: k_diffuse<T, 8><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        default: die_set_error("die_diffuse_decay: radius %d not supported (sigma too large)", R); return DIE_ERR_UNSUPPORTED;
    }
    return DIE_OK;
}

static int diffuse_decay_mode(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype, float sigma, float decay,
                              int32_t mode, void* stream) {
    DIE_REQUIRE(src && dst && src != dst, "die_diffuse_decay: src/dst must be distinct non-null planes");
    DIE_REQUIRE(W >= 1 && H >= 1, "die_diffuse_decay: bad size %dx%d", W, H);
    DIE_REQUIRE(sigma > 0.f, "die_diffuse_decay: sigma must be positive");
    DIE_REQUIRE(dtype == DIE_F32 || dtype == DIE_F16, "die_diffuse_decay: bad dtype %d", dtype);
    // scipy.ndimage._gaussian_kernel1d: radius int(4σ + .5), exp(−x²/2σ²) normalised
    const int R = die_gaussian_radius(sigma);
    DIE_REQUIRE(R >= 1, "die_diffuse_decay: sigma %g gives an empty kernel", (double)sigma);
    if (R > DIF_MAXR) {
        die_set_error("die_diffuse_decay: sigma %g needs radius %d > %d", (double)sigma, R, DIF_MAXR);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(mode >= DIE_DIFFUSE_WRAP && mode <= DIE_DIFFUSE_CONSTANT, "die_diffuse_decay: bad boundary mode %d", mode);
    if (mode == DIE_DIFFUSE_WRAP && rows_kernel_applies(W, H, R)) {
        RowsArgs ra;
        double wd[2 * DIF_MAXR + 1];
        gaussian_taps(sigma, wd);
        ra.src = src; ra.dst = dst; ra.claim = nullptr; ra.dep = nullptr; ra.food = nullptr; ra.W = W; ra.H = H; ra.epoch = 0; ra.halo = 0; ra.rep_cells = 0;
        ra.wrapx = ra.wrapy = 1; ra.part_gain = nullptr; ra.part_gain2 = nullptr; ra.part_alive = nullptr; ra.n_part = 0; ra.result = nullptr; ra.alive_const = 0;
        ra.food_infinite = 1; ra.keep = (float)(1.0 - (double)decay); ra.rate_feed = 0.f;
        for (int k = 0; k <= 2 * R; ++k) ra.w[k] = (float)wd[k];
        int rc2 = dtype == DIE_F32 ? launch_rows<float, 0>(ra, R, (hipStream_t)stream)
                                   : launch_rows<__half, 0>(ra, R, (hipStream_t)stream);
        if (rc2 != DIE_OK) return rc2;
        DIE_CHECK_LAUNCH("die_diffuse_decay");
        return DIE_OK;
    }
    DiffuseArgs a;
    a.src = src; a.dst = dst; a.W = W; a.H = H; a.mode = mode;
    a.keep = (float)(1.0 - (double)decay);
    double w[2 * DIF_MAXR + 1], sum = 0.0;
    for (int k = -R; k <= R; ++k) { w[k + R] = exp(-0.5 / ((double)sigma * (double)sigma) * k * k); sum += w[k + R]; }
    for (int k = 0; k <= 2 * R; ++k) a.w[k] = (float)(w[k] / sum);
    int rc = dtype == DIE_F32 ? launch_diffuse<float>(a, R, (hipStream_t)stream)
                              : launch_diffuse<__half>(a, R, (hipStream_t)stream);
    if (rc != DIE_OK) return rc;
    DIE_CHECK_LAUNCH("die_diffuse_decay");
    return DIE_OK;
}

extern "C" int die_diffuse_decay(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype, float sigma,
                                 float decay, void* stream) {
    return diffuse_decay_mode(src, dst, W, H, dtype, sigma, decay, DIE_DIFFUSE_WRAP, stream);
}

extern "C" int die_diffuse_decay_mode(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype, float sigma,
                                      float decay, int32_t mode, void* stream) {
    return diffuse_decay_mode(src, dst, W, H, dtype, sigma, decay, mode, stream);
}

// ---- step driver ----------------------------------------------------------------------
static int step_grid(int64_t N) {
    int64_t g = (N + DIE_STEP_BLOCK - 1) / DIE_STEP_BLOCK;
#define DIE_STEP_GRID_CAP 8192
    const int64_t cap = DIE_STEP_GRID_CAP;   // ≤ DIE_MAX_PARTIALS partial sums for k_reduce (8192 measured 3 % faster than 2048)
    return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}

// workspace layout: [part_gain_a | part_gain_b | part_alive | scan scratch (die_init) | stash (N floats)]
static const int64_t WS_PARTS = (int64_t)DIE_MAX_PARTIALS * 8 * 3;

extern "C" int64_t die_workspace_bytes(int32_t W, int32_t H, int64_t N) {
    if (W < 1 || H < 1 || N < 0) return -1;
    int64_t b = WS_PARTS + die_ws_scan_bytes(W, H) + N * (int64_t)sizeof(float);
    return (b + 255) & ~(int64_t)255;
}

static int fill_args(StepArgs& k, const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                     void* ws, int64_t ws_bytes, const char* who) {
    DIE_REQUIRE(m && a && d && ws, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1 && a->N > 0, "%s: bad sizes", who);
    DIE_REQUIRE((int64_t)a->N <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: too many slots for the ownership word", who);
    DIE_REQUIRE(m->epoch >= 1 && m->epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, m->epoch,
                DIE_OWNER_EPOCH_MAX);
    DIE_REQUIRE(m->owner && m->food && m->chem && a->x && a->y && a->alive && a->agent_food, "%s: null device pointer", who);
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad field dtype %d", who, m->dtype);
    DIE_REQUIRE(ws_bytes >= die_workspace_bytes(m->W, m->H, a->N), "%s: workspace too small (%lld < %lld)", who,
                (long long)ws_bytes, (long long)die_workspace_bytes(m->W, m->H, a->N));
    if (d->boundary != DIE_BOUNDARY_WRAP && d->boundary != DIE_BOUNDARY_LIMIT) {
        die_set_error("%s: boundary %d (pass-through) leaves [0,1) and is not representable in Q0.32", who, d->boundary);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(d->cost == DIE_COST_LINEAR || d->cost == DIE_COST_ZERO, "%s: bad cost operator %d", who, d->cost);
    if (act) {
        DIE_REQUIRE(act->N == a->N && act->dx && act->dy && act->deposit, "%s: bad action array", who);
        k.dx = act->dx; k.dy = act->dy; k.dep = act->deposit;
    } else {
        k.dx = k.dy = k.dep = nullptr;
    }
    k.g = die_geo_of(m); k.epoch = m->epoch; k.N = a->N;
    k.do_move = 1; k.do_claim = 1; k.tile_w = k.tile_h = k.tiles_y = 1; k.tile_of = nullptr;
    k.owner = (unsigned long long*)m->owner; k.food = m->food; k.chem = m->chem;
    k.x = a->x; k.y = a->y; k.slot = a->slot; k.alive = a->alive; k.agent_food = a->agent_food;
    k.rate_feed = d->rate_feed; k.w_dep = d->cost_w_deposit; k.w_dist = d->cost_w_dist;
    k.boundary = d->boundary; k.cost = d->cost; k.food_infinite = d->food_infinite; k.agents_die = d->agents_die;
    k.has_dead = d->has_dead_slots || d->agents_die;
    k.skip_scatter = 0;
    char* w = (char*)ws;
    k.part_gain = nullptr;
    // ghost-agent tiles: num_alive is the number of alive slots on OWNED cells, counted by the claim pass
    k.part_alive = k.g.own_x1 > 0 ? (long long*)ws + 2 * DIE_MAX_PARTIALS : nullptr;
    k.stash = (float*)(w + WS_PARTS + die_ws_scan_bytes(m->W, m->H));
    k.stash_cost = nullptr;
    return DIE_OK;
}

extern "C" int die_agent_move_claim(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                    void* ws, int64_t ws_bytes, void* stream) {
    StepArgs k;
    int rc = fill_args(k, m, a, act, d, ws, ws_bytes, "die_agent_move_claim");
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(act, "die_agent_move_claim: null action");
    k.part_gain = (long long*)ws;
    const int grid = step_grid(a->N);
    if (m->dtype == DIE_F32) k_move_claim<float><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    else k_move_claim<__half><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH("die_agent_move_claim");
    return DIE_OK;
}

extern "C" int die_agent_move(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                              int32_t tile_w, int32_t tile_h, int32_t tiles_y, int32_t* tile_of, void* stream) {
    DIE_REQUIRE(m && a && act && d && tile_of, "die_agent_move: null argument");
    DIE_REQUIRE(tile_w >= 1 && tile_h >= 1 && tiles_y >= 1, "die_agent_move: bad tile shape");
    DIE_REQUIRE(a->N > 0 && act->N == a->N && a->x && a->y && act->dx && act->dy, "die_agent_move: bad arrays");
    if (d->boundary != DIE_BOUNDARY_WRAP && d->boundary != DIE_BOUNDARY_LIMIT) {
        die_set_error("die_agent_move: boundary %d is not representable in Q0.32", d->boundary);
        return DIE_ERR_UNSUPPORTED;
    }
    StepArgs k = {};
    k.g = die_geo_of(m); k.N = a->N; k.x = a->x; k.y = a->y; k.dx = act->dx; k.dy = act->dy;
    k.boundary = d->boundary; k.do_move = 1; k.do_claim = 0;
    k.tile_w = tile_w; k.tile_h = tile_h; k.tiles_y = tiles_y; k.tile_of = tile_of;
    k_move_claim<float><<<step_grid(a->N), DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH("die_agent_move");
    return DIE_OK;
}

extern "C" int die_forward_move(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                const die_dynamics* d, int32_t tile_w, int32_t tile_h, int32_t tiles_y, int32_t* tile_of,
                                void* stream) {
    DIE_REQUIRE(m && a && g && act && d && tile_of, "die_forward_move: null argument");
    DIE_REQUIRE(tile_w >= 1 && tile_h >= 1 && tiles_y >= 1, "die_forward_move: bad tile shape");
    if (d->boundary != DIE_BOUNDARY_WRAP && d->boundary != DIE_BOUNDARY_LIMIT) {
        die_set_error("die_forward_move: boundary %d is not representable in Q0.32", d->boundary);
        return DIE_ERR_UNSUPPORTED;
    }
    FwdArgs f;
    int rc = die_fill_fwd_args(f, m, a, g, act, "die_forward_move");
    if (rc != DIE_OK) return rc;
    StepArgs k = {};
    k.g = die_geo_of(m); k.N = a->N; k.x = a->x; k.y = a->y; k.slot = a->slot;
    k.boundary = d->boundary; k.do_move = 1; k.do_claim = 0;
    k.tile_w = tile_w; k.tile_h = tile_h; k.tiles_y = tiles_y; k.tile_of = tile_of;
    const int grid = step_grid(a->N);
    hipStream_t s = (hipStream_t)stream;
    if (m->dtype == DIE_F32) {
        if (g->kind == DIE_AGENT_PHYSARUM) k_forward_move_claim<float, DIE_AGENT_PHYSARUM><<<grid, DIE_STEP_BLOCK, 0, s>>>(f, k);
        else k_forward_move_claim<float, DIE_AGENT_GRADIENT><<<grid, DIE_STEP_BLOCK, 0, s>>>(f, k);
    } else {
        if (g->kind == DIE_AGENT_PHYSARUM) k_forward_move_claim<__half, DIE_AGENT_PHYSARUM><<<grid, DIE_STEP_BLOCK, 0, s>>>(f, k);
        else k_forward_move_claim<__half, DIE_AGENT_GRADIENT><<<grid, DIE_STEP_BLOCK, 0, s>>>(f, k);
    }
    DIE_CHECK_LAUNCH("die_forward_move");
    return DIE_OK;
}

extern "C" int die_agent_claim_feed(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                    void* ws, int64_t ws_bytes, void* stream) {
    StepArgs k;
    int rc = fill_args(k, m, a, act, d, ws, ws_bytes, "die_agent_claim_feed");
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(act, "die_agent_claim_feed: null action");
    k.do_move = 0;
    k.part_gain = (long long*)ws;
    const int grid = step_grid(a->N);
    if (m->dtype == DIE_F32) k_move_claim<float><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    else k_move_claim<__half><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH("die_agent_claim_feed");
    return DIE_OK;
}

extern "C" int die_diffuse_decay_tile(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype, float sigma,
                                      float decay, void* stream) {
    DIE_REQUIRE(src && dst && src != dst, "die_diffuse_decay_tile: src/dst must be distinct non-null planes");
    DIE_REQUIRE(dtype == DIE_F32 || dtype == DIE_F16, "die_diffuse_decay_tile: bad dtype %d", dtype);
    DIE_REQUIRE(sigma > 0.f, "die_diffuse_decay_tile: sigma must be positive");
    const int R = die_gaussian_radius(sigma);
    if (!(R >= 1 && R <= 4 && H % 4 == 0 && H >= 8 && W >= 2 * R + 1)) {
        die_set_error("die_diffuse_decay_tile: needs H %% 4 == 0, H >= 8, radius 1..4 (W=%d H=%d sigma=%g)", W, H, (double)sigma);
        return DIE_ERR_UNSUPPORTED;
    }
    RowsArgs ra;
    double wd[2 * DIF_MAXR + 1];
    gaussian_taps(sigma, wd);
    ra.src = src; ra.dst = dst; ra.claim = nullptr; ra.dep = nullptr; ra.food = nullptr; ra.W = W; ra.H = H; ra.epoch = 0; ra.halo = 0; ra.rep_cells = 0;
    ra.wrapx = ra.wrapy = 0; ra.part_gain = nullptr; ra.part_gain2 = nullptr; ra.part_alive = nullptr; ra.n_part = 0; ra.result = nullptr; ra.alive_const = 0;
    ra.food_infinite = 1; ra.keep = (float)(1.0 - (double)decay); ra.rate_feed = 0.f;
    for (int k = 0; k <= 2 * R; ++k) ra.w[k] = (float)wd[k];
    int rc = dtype == DIE_F32 ? launch_rows<float, 0, false>(ra, R, (hipStream_t)stream)
                              : launch_rows<__half, 0, false>(ra, R, (hipStream_t)stream);
    if (rc != DIE_OK) return rc;
    DIE_CHECK_LAUNCH("die_diffuse_decay_tile");
    return DIE_OK;
}

extern "C" int die_agent_resolve(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                 void* ws, int64_t ws_bytes, void* stream) {
    StepArgs k;
    int rc = fill_args(k, m, a, act, d, ws, ws_bytes, "die_agent_resolve");
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(act, "die_agent_resolve: null action");
    k.part_gain = (long long*)ws + DIE_MAX_PARTIALS;
    k.part_alive = (long long*)ws + 2 * DIE_MAX_PARTIALS;
    const int grid = step_grid(a->N);
    if (m->dtype == DIE_F32) k_resolve<float><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    else k_resolve<__half><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH("die_agent_resolve");
    return DIE_OK;
}

extern "C" int die_step_reduce_ex(const die_agents* a, die_step_result* result, void* ws, int64_t ws_bytes,
                                  int32_t with_second_pass, int64_t alive_const, void* stream) {
    DIE_REQUIRE(a && result && ws, "die_step_reduce_ex: null argument");
    DIE_REQUIRE(ws_bytes >= WS_PARTS, "die_step_reduce_ex: workspace too small");
    const int g = step_grid(a->N);
    // with_second_pass: 0 = claim-pass gains, num_alive = alive_const; 1 = + the dead-slot pass's gains and its
    // alive count; 2 = claim-pass gains and the claim pass's count of owned alive slots (ghost-agent tiles);
    // 3 = both passes' gains, num_alive = alive_const (reference-compatible lifecycle: the count is frozen)
    const bool both = with_second_pass == 1 || with_second_pass == 3;
    k_reduce<<<1, 1024, 0, (hipStream_t)stream>>>((const long long*)ws, g, (const long long*)ws + DIE_MAX_PARTIALS, both ? g : 0,
                                                  (const long long*)ws + 2 * DIE_MAX_PARTIALS,
                                                  (with_second_pass == 1 || with_second_pass == 2) ? g : 0, result,
                                                  (with_second_pass == 1 || with_second_pass == 2) ? -1 : alive_const);
    DIE_CHECK_LAUNCH("die_step_reduce_ex");
    return DIE_OK;
}

// _agent_lifecycle (core/env.py:245-250) alone: where(agent_food > 1e-4, agents, 0) on every channel
__global__ __launch_bounds__(DIE_BLOCK) void k_lifecycle(int64_t N, uint32_t* x, uint32_t* y, uint8_t* alive, float* agent_food) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride)
        if (!(agent_food[n] > 1e-4f)) { x[n] = 0; y[n] = 0; alive[n] = 0; agent_food[n] = 0.f; }
}

extern "C" int die_agents_lifecycle(const die_agents* a, void* stream) {
    DIE_REQUIRE(a && a->N > 0 && a->x && a->y && a->alive && a->agent_food, "die_agents_lifecycle: bad agents");
    int64_t g = (a->N + DIE_BLOCK - 1) / DIE_BLOCK;
    k_lifecycle<<<(int)(g < 8192 ? g : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(a->N, a->x, a->y, a->alive, a->agent_food);
    DIE_CHECK_LAUNCH("die_agents_lifecycle");
    return DIE_OK;
}

extern "C" int die_step_reduce(const die_agents* a, const die_dynamics* d, die_step_result* result, void* ws,
                               int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(a && d && result && ws, "die_step_reduce: null argument");
    DIE_REQUIRE(ws_bytes >= WS_PARTS, "die_step_reduce: workspace too small");
    const int g = step_grid(a->N);
    k_reduce<<<1, 1024, 0, (hipStream_t)stream>>>((const long long*)ws, g, (const long long*)ws + DIE_MAX_PARTIALS, g,
                                                       (const long long*)ws + 2 * DIE_MAX_PARTIALS, g,
                                                       result, -1);
    DIE_CHECK_LAUNCH("die_step_reduce");
    return DIE_OK;
}

static int deposit_feed_diffuse(const die_medium* m, const die_dynamics* d, int halo, bool tile, void* stream, const char* who,
                                const long long* part_gain = nullptr, int n_part = 0, die_step_result* result = nullptr,
                                long long alive_const = 0, const long long* part_alive = nullptr, const float* dep_plane = nullptr);
extern "C" int die_agent_dead_slots(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                    void* ws, int64_t ws_bytes, void* stream);

static bool fused_step_applies(const die_medium* m, const die_dynamics* d) {
    const int R = die_gaussian_radius(d->diffuse_sigma);
    return m->gW <= 0 && d->diffuse_mode == DIE_DIFFUSE_WRAP && rows_kernel_applies(m->W, m->H, R) && R >= 1 && !d->staged;
}

bool fused_step_shape_ok(const die_medium* m, const die_dynamics* d) { return fused_step_applies(m, d); }      // (die_pic.hip)

// everything of die_env_step after the claims are in place (fused path)
static int env_step_tail(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                         die_step_result* result, void* ws, int64_t ws_bytes, void* stream) {
    // deposits and feeding ride on the diffusion sweep; the per-agent second pass is only needed for
    // dead slots / lifecycle (it then skips the winner's scatter)
    const bool second_pass = d->has_dead_slots || d->agents_die;
    if (second_pass) {
        int rc = die_agent_dead_slots(m, a, act, d, ws, ws_bytes, stream);
        if (rc != DIE_OK) return rc;
    }
    const int g = step_grid(a->N);
    if (!second_pass)                                       // an extra workgroup of the sweep does the reduction (same summation order)
        return deposit_feed_diffuse(m, d, 0, false, stream, "die_env_step(diffuse+deposit+feed+reduce)", (const long long*)ws, g,
                                    result, a->N);
    k_reduce<<<1, 1024, 0, (hipStream_t)stream>>>((const long long*)ws, g, (const long long*)ws + DIE_MAX_PARTIALS,
                                                  g, (const long long*)ws + 2 * DIE_MAX_PARTIALS, g, result, -1);
    DIE_CHECK_LAUNCH("die_env_step(reduce)");
    return deposit_feed_diffuse(m, d, 0, false, stream, "die_env_step(diffuse+deposit+feed)");
}

extern "C" int die_env_step(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                            die_step_result* result, void* ws, int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(m && a && act && d && result, "die_env_step: null argument");
    DIE_REQUIRE(m->chem_next && m->chem_next != m->chem, "die_env_step: chem_next must be a second plane");
    int rc = die_agent_move_claim(m, a, act, d, ws, ws_bytes, stream);
    if (rc != DIE_OK) return rc;
    if (fused_step_applies(m, d)) return env_step_tail(m, a, act, d, result, ws, ws_bytes, stream);
    rc = die_agent_resolve(m, a, act, d, ws, ws_bytes, stream);
    if (rc != DIE_OK) return rc;
    rc = die_step_reduce(a, d, result, ws, ws_bytes, stream);
    if (rc != DIE_OK) return rc;
    if (m->gW > 0) {
        die_set_error("die_env_step: a decomposed tile needs halo exchange and migration between the stages; "
                      "drive die_agent_move / die_agent_claim_feed / die_medium_deposit_feed_diffuse_tile instead");
        return DIE_ERR_UNSUPPORTED;
    }
    return diffuse_decay_mode(m->chem, m->chem_next, m->W, m->H, m->dtype, d->diffuse_sigma, d->rate_decay_chem, d->diffuse_mode,
                              stream);
}

static int forward_move_claim(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                              const die_dynamics* d, void* ws, int64_t ws_bytes, void* stream, bool tile_ok, const char* who) {
    DIE_REQUIRE(m && a && g && act && d, "%s: null argument", who);
    if (!tile_ok && !fused_step_applies(m, d)) {   // first half of the fused step: refuse before touching anything
        die_set_error("%s: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4", who);
        return DIE_ERR_UNSUPPORTED;
    }
    FwdArgs f;
    int rc = die_fill_fwd_args(f, m, a, g, act, who);
    if (rc != DIE_OK) return rc;
    StepArgs k;
    rc = fill_args(k, m, a, act, d, ws, ws_bytes, who);
    if (rc != DIE_OK) return rc;
    k.part_gain = (long long*)ws;
    const int grid = step_grid(a->N);
    hipStream_t s = (hipStream_t)stream;
    // the sense-mask and ownership tests are compiled out of the plain single-tile kernel (they cost ≈ 5 % there)
    const bool ext = f.mask != nullptr || k.g.own_x1 > 0;
#define DIE_FMC(T, KIND, LEAN) do { if (ext) k_forward_move_claim<T, KIND, true, LEAN><<<grid, DIE_STEP_BLOCK, 0, s>>>(f, k); \
                                    else k_forward_move_claim<T, KIND, false, LEAN><<<grid, DIE_STEP_BLOCK, 0, s>>>(f, k); } while (0)
    const bool lean = fwd_is_lean(g);
    if (m->dtype == DIE_F32) {
        if (g->kind != DIE_AGENT_PHYSARUM) DIE_FMC(float, DIE_AGENT_GRADIENT, false);
        else if (lean) DIE_FMC(float, DIE_AGENT_PHYSARUM, true);
        else DIE_FMC(float, DIE_AGENT_PHYSARUM, false);
    } else {
        if (g->kind != DIE_AGENT_PHYSARUM) DIE_FMC(__half, DIE_AGENT_GRADIENT, false);
        else if (lean) DIE_FMC(__half, DIE_AGENT_PHYSARUM, true);
        else DIE_FMC(__half, DIE_AGENT_PHYSARUM, false);
    }
#undef DIE_FMC
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_forward_move_claim(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                      const die_dynamics* d, void* ws, int64_t ws_bytes, void* stream) {
    return forward_move_claim(m, a, g, act, d, ws, ws_bytes, stream, false, "die_forward_move_claim");
}

extern "C" int die_forward_move_claim_tile(const die_medium* m, const die_agents* a, die_gradient_agent* g,
                                           const die_action* act, const die_dynamics* d, void* ws, int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(m && m->gW > 0, "die_forward_move_claim_tile: the planes must be a tile of a decomposed world");
    return forward_move_claim(m, a, g, act, d, ws, ws_bytes, stream, true, "die_forward_move_claim_tile");
}

extern "C" int die_env_step_finish(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                   die_step_result* result, void* ws, int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(m && a && act && d && result && ws, "die_env_step_finish: null argument");
    if (!fused_step_applies(m, d)) {
        die_set_error("die_env_step_finish: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4");
        return DIE_ERR_UNSUPPORTED;
    }
    return env_step_tail(m, a, act, d, result, ws, ws_bytes, stream);
}

extern "C" int die_forward_env_step(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                    const die_dynamics* d, die_step_result* result, void* ws, int64_t ws_bytes,
                                    void* stream) {
    DIE_REQUIRE(m && a && g && act && d && result, "die_forward_env_step: null argument");
    DIE_REQUIRE(m->chem_next && m->chem_next != m->chem, "die_forward_env_step: chem_next must be a second plane");
    if (!fused_step_applies(m, d)) {
        die_set_error("die_forward_env_step: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4");
        return DIE_ERR_UNSUPPORTED;
    }
    int rc = die_forward_move_claim(m, a, g, act, d, ws, ws_bytes, stream);
    if (rc != DIE_OK) return rc;
    return env_step_tail(m, a, act, d, result, ws, ws_bytes, stream);
}

extern "C" int64_t die_batch_workspace_bytes(int32_t replicas) {
    return replicas >= 1 && replicas <= DIE_MAX_REPLICAS ? (int64_t)replicas * WS_PARTS : -1;
}

// with dead slots (agents_die / has_dead_slots): the partials of every replica, then per replica a [consumed | cost] stash
// of agent_stride floats each (k_lifecycle_batch)
extern "C" int64_t die_batch_lifecycle_workspace_bytes(int32_t replicas, int64_t agent_stride) {
    if (replicas < 1 || replicas > DIE_MAX_REPLICAS || agent_stride < 1 || agent_stride > (int64_t)DIE_OWNER_SLOT_MASK) return -1;
    const int64_t b = (int64_t)replicas * WS_PARTS + (int64_t)replicas * 2 * agent_stride * (int64_t)sizeof(float);
    return (b + 255) & ~(int64_t)255;
}

// the workspace checks of both batched entry points (before anything else is read)
static int batch_ws_check(const die_dynamics* d, const die_batch* b, int64_t ws_bytes, const char* who) {
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas", who, DIE_MAX_REPLICAS);
    DIE_REQUIRE(ws_bytes >= die_batch_workspace_bytes(b->replicas), "%s: workspace too small", who);
    if (d->agents_die || d->has_dead_slots) {
        const int64_t need = die_batch_lifecycle_workspace_bytes(b->replicas, b->agent_stride);
        DIE_REQUIRE(need > 0, "%s: bad agent stride %lld", who, (long long)b->agent_stride);
        DIE_REQUIRE(ws_bytes >= need, "%s: workspace too small for dead slots (%lld < %lld: die_batch_lifecycle_workspace_bytes)", who,
                    (long long)ws_bytes, (long long)need);
    }
    return DIE_OK;
}

// what the claim launch of a batched step and the launches after it take
struct BatchLaunch {
    StepArgs k;
    BatchArgs ba;
    dim3 grid;                                          // the claim pass's, kept by the lifecycle pass; grid.x partials per replica
    hipStream_t s;
};

// the step half's arguments of every replica and the claim pass's grid, checked before any launch
static int batch_step_args(BatchLaunch& L, const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                           const die_batch* b, void* ws, void* stream, const char* who) {
    StepArgs& k = L.k;
    BatchArgs& ba = L.ba;
    // fill_args checks the per-replica workspace of the single-world step; here only the partial arrays are used
    DIE_REQUIRE(m->epoch >= 1 && m->epoch <= DIE_OWNER_EPOCH_MAX && m->owner && a->alive && a->agent_food, "%s: bad medium / agents", who);
    if (d->boundary != DIE_BOUNDARY_WRAP && d->boundary != DIE_BOUNDARY_LIMIT) {
        die_set_error("%s: boundary %d is not representable in Q0.32", who, d->boundary);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(d->cost == DIE_COST_LINEAR || d->cost == DIE_COST_ZERO, "%s: bad cost operator %d", who, d->cost);
    k = StepArgs{};
    k.g = die_geo_of(m); k.epoch = m->epoch; k.N = a->N; k.do_move = 1; k.do_claim = 1; k.tile_w = k.tile_h = k.tiles_y = 1;
    k.owner = (unsigned long long*)m->owner; k.food = m->food; k.chem = m->chem;
    k.x = a->x; k.y = a->y; k.slot = a->slot; k.alive = a->alive; k.agent_food = a->agent_food;
    k.dx = act ? act->dx : nullptr; k.dy = act ? act->dy : nullptr; k.dep = act ? act->deposit : nullptr;
    k.rate_feed = d->rate_feed; k.w_dep = d->cost_w_deposit; k.w_dist = d->cost_w_dist;
    k.boundary = d->boundary; k.cost = d->cost; k.food_infinite = d->food_infinite;
    k.agents_die = d->agents_die; k.has_dead = d->has_dead_slots || d->agents_die;
    k.skip_scatter = 1;                                 // (k_lifecycle_batch: the sweep writes the planes)
    k.part_gain = (long long*)ws;
    k.stash = k.has_dead ? (float*)((char*)ws + (int64_t)b->replicas * WS_PARTS) : nullptr;   // batch_stash offsets it per replica
    ba.cells = b->plane_stride; ba.agents = b->agent_stride; ba.seed_stride = b->seed_stride;
    int64_t nmax = 0;
    for (int r = 0; r < DIE_MAX_REPLICAS; ++r) {
        ba.n[r] = r < b->replicas ? b->n[r] : 0;
        DIE_REQUIRE(r >= b->replicas || (b->n[r] >= 1 && b->n[r] <= b->agent_stride), "%s: replica %d has %lld agents", who, r, (long long)b->n[r]);
        if (ba.n[r] > nmax) nmax = ba.n[r];
    }
    L.grid = dim3(step_grid(nmax), b->replicas);
    L.s = (hipStream_t)stream;
    return DIE_OK;
}

// Per-replica Dynamics: launch_rows' grid for the `grp.n` replicas of radius R (the rows-per-wave choice is the whole batch's, so
// a batch of one radius is launched in the shared-Dynamics sweep's shape)
// FUSED = 0: the plain sweep of those replicas (the step's adjoint, die_diffuse_rows_batch), no reduction row ahead of the field's
template <typename T, int FUSED = 1>
static void launch_rows_table(RowsArgs a, int R, const RowsTable& grp, int replicas, hipStream_t s) {
    const int strips = (a.H + DIF_WCOLS - 1) / DIF_WCOLS;
    constexpr int WPB = DIF_BLOCK / DIE_WAVE;
    a.rpw = rows_per_wave(a.W, a.H, replicas);
    dim3 grid((strips + WPB - 1) / WPB, (a.W + a.rpw - 1) / a.rpw + (FUSED ? 1 : 0), grp.n);
    switch (R) {
        case 1: k_diffuse_rows<T, 1, FUSED, true, RowsTable><<<grid, DIF_BLOCK, 0, s>>>(a, grp); break;
        case 2: k_diffuse_rows<T, 2, FUSED, true, RowsTable><<<grid, DIF_BLOCK, 0, s>>>(a, grp); break;
        case 3: k_diffuse_rows<T, 3, FUSED, true, RowsTable><<<grid, DIF_BLOCK, 0, s>>>(a, grp); break;
        default: k_diffuse_rows<T, 4, FUSED, true, RowsTable><<<grid, DIF_BLOCK, 0, s>>>(a, grp); break;
    }
}

// the replicas of radius R among rows_host, as the by-value index list of a sweep launch
static RowsTable rows_group(const die_dynamics_row* rows, const die_dynamics_row* rows_host, int replicas, int R) {
    RowsTable grp;
    grp.rows = rows;
    grp.n = 0;
    for (int r = 0; r < DIE_MAX_REPLICAS; ++r) grp.idx[r] = 0;
    for (int r = 0; r < replicas; ++r)
        if (rows_host[r].radius == R) grp.idx[grp.n++] = (uint8_t)r;
    return grp;
}

// the sweep of a batch with per-replica rows: one launch per radius present among rows_host (checked to lie in 1..4)
static int batch_sweep_rows(const die_medium* m, const RowsArgs& ra, const die_batch* b, hipStream_t s, const char* who,
                            const die_dynamics_row* rows, const die_dynamics_row* rows_host) {
    for (int R = 1; R <= 4; ++R) {
        const RowsTable grp = rows_group(rows, rows_host, b->replicas, R);
        if (!grp.n) continue;
        if (m->dtype == DIE_F32) launch_rows_table<float>(ra, R, grp, b->replicas, s);
        else launch_rows_table<__half>(ra, R, grp, b->replicas, s);
        DIE_CHECK_LAUNCH(who);
    }
    return DIE_OK;
}

// (1 - decay) * G(src) of `replicas` fp32 planes `plane_stride` cells apart, without deposits or feeding (die_env_grad.hip:
// die_env_step_backward_batch, whose checks precede this: H % 4 == 0, every radius in 1..4).  rows NULL: one launch, the taps and
// `keep` of (sigma, decay) exactly as diffuse_decay_mode builds them, the kernel die_diffuse_decay launches with the replica in
// gridDim.z.  Else replica r under rows[r]'s taps and keep: one launch per radius present, as batch_sweep_rows.
int die_diffuse_rows_batch(const float* src, float* dst, int32_t W, int32_t H, int32_t replicas, int64_t plane_stride, float sigma,
                           float decay, const die_dynamics_row* rows, const die_dynamics_row* rows_host, void* stream, const char* who) {
    RowsArgs ra;
    ra.src = src; ra.dst = dst; ra.claim = nullptr; ra.dep = nullptr; ra.food = nullptr; ra.W = W; ra.H = H; ra.epoch = 0; ra.halo = 0;
    ra.rep_cells = plane_stride;
    ra.wrapx = ra.wrapy = 1; ra.part_gain = nullptr; ra.part_gain2 = nullptr; ra.part_alive = nullptr; ra.n_part = 0; ra.result = nullptr; ra.alive_const = 0;
    ra.food_infinite = 1; ra.keep = 0.f; ra.rate_feed = 0.f;
    for (int k = 0; k <= 2 * 4; ++k) ra.w[k] = 0.f;
    hipStream_t s = (hipStream_t)stream;
    if (rows) {
        for (int R = 1; R <= 4; ++R) {
            const RowsTable grp = rows_group(rows, rows_host, replicas, R);
            if (!grp.n) continue;
            launch_rows_table<float, 0>(ra, R, grp, replicas, s);
            DIE_CHECK_LAUNCH(who);
        }
        return DIE_OK;
    }
    double wd[2 * DIF_MAXR + 1];
    const int R = gaussian_taps(sigma, wd);
    ra.keep = (float)(1.0 - (double)decay);
    for (int k = 0; k <= 2 * R; ++k) ra.w[k] = (float)wd[k];
    const int rc = launch_rows<float, 0>(ra, R, s, replicas);
    if (rc != DIE_OK) return rc;
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// both tables of a *_rows entry point (with_rows), after the parent's own checks
static int batch_rows_check(bool with_rows, const die_batch* b, const die_dynamics_row* rows, const die_dynamics_row* rows_host,
                            const char* who) {
    if (!with_rows) return DIE_OK;
    DIE_REQUIRE(rows, "%s: null dynamics rows (rows == NULL)", who);
    DIE_REQUIRE(rows_host, "%s: null host copy of the dynamics rows (rows_host == NULL)", who);
    for (int r = 0; r < b->replicas; ++r)
        DIE_REQUIRE(rows_host[r].radius >= 1 && rows_host[r].radius <= 4, "%s: row %d has radius %d, outside 1..4", who, r, rows_host[r].radius);
    return DIE_OK;
}

extern "C" int die_dynamics_rows(const die_dynamics* d, int32_t n, int32_t W, int32_t H, die_dynamics_row* rows_host) {
    const char* who = "die_dynamics_rows";
    DIE_REQUIRE(d && rows_host, "%s: null argument", who);
    DIE_REQUIRE(n >= 1 && n <= DIE_MAX_REPLICAS, "%s: %d rows, 1..%d expected", who, n, DIE_MAX_REPLICAS);
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    for (int r = 0; r < n; ++r) {
        const int R = die_gaussian_radius(d[r].diffuse_sigma);
        if (!(d[r].diffuse_sigma > 0.f) || R < 1 || !rows_kernel_applies(W, H, R)) {       // fused_step_applies, per row
            die_set_error("%s: row %d: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4 (W=%d H=%d sigma=%g radius %d)", who,
                          r, W, H, (double)d[r].diffuse_sigma, R);
            return DIE_ERR_UNSUPPORTED;
        }
        DIE_REQUIRE(d[r].diffuse_mode == DIE_DIFFUSE_WRAP, "%s: row %d: diffuse_mode %d: only WRAP is batched", who, r, d[r].diffuse_mode);
        DIE_REQUIRE(!d[r].staged, "%s: row %d: staged steps are not batched", who, r);
        DIE_REQUIRE(d[r].boundary == d[0].boundary, "%s: row %d disagrees with row 0 in boundary (%d != %d)", who, r, d[r].boundary, d[0].boundary);
        DIE_REQUIRE(d[r].cost == d[0].cost, "%s: row %d disagrees with row 0 in cost (%d != %d)", who, r, d[r].cost, d[0].cost);
        DIE_REQUIRE(d[r].cost_w_deposit == d[0].cost_w_deposit && d[r].cost_w_dist == d[0].cost_w_dist,
                    "%s: row %d disagrees with row 0 in the cost weights", who, r);
        DIE_REQUIRE(!d[r].agents_die == !d[0].agents_die, "%s: row %d disagrees with row 0 in agents_die", who, r);
        DIE_REQUIRE(!d[r].has_dead_slots == !d[0].has_dead_slots, "%s: row %d disagrees with row 0 in has_dead_slots", who, r);
    }
    for (int r = 0; r < n; ++r) {
        die_dynamics_row row = {};
        double wd[2 * DIF_MAXR + 1];
        row.radius = gaussian_taps(d[r].diffuse_sigma, wd);
        row.rate_feed = d[r].rate_feed;
        row.keep = (float)(1.0 - (double)d[r].rate_decay_chem);
        row.food_infinite = d[r].food_infinite ? 1 : 0;
        for (int k = 0; k <= 2 * row.radius; ++k) row.w[k] = (float)wd[k];
        rows_host[r] = row;
    }
    return DIE_OK;
}

// what every fused sweep takes from the medium and the dynamics (R: the gaussian radius of d->diffuse_sigma); the caller sets the
// rest: dep, halo, rep_cells, the wrap flags, the partials and the result
static RowsArgs rows_args_of(const die_medium* m, const die_dynamics* d, int R) {
    RowsArgs ra;
    double wd[2 * DIF_MAXR + 1];
    gaussian_taps(d->diffuse_sigma, wd);
    ra.src = m->chem; ra.dst = m->chem_next; ra.claim = (const unsigned long long*)m->owner; ra.food = m->food;
    ra.W = m->W; ra.H = m->H; ra.epoch = m->epoch; ra.food_infinite = d->food_infinite;
    ra.keep = (float)(1.0 - (double)d->rate_decay_chem); ra.rate_feed = d->rate_feed;
    for (int k = 0; k <= 2 * R; ++k) ra.w[k] = (float)wd[k];
    return ra;
}

// the field sweep of every replica in one launch (gridDim.z), each with its own reduction workgroup over the n_part partials
// (and, with dead slots, over the lifecycle pass's n_part partial gains too)
static int batch_sweep(const die_medium* m, const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws, int n_part,
                       hipStream_t s, const char* who, const die_dynamics_row* rows = nullptr, const die_dynamics_row* rows_host = nullptr) {
    const int R = die_gaussian_radius(d->diffuse_sigma);
    RowsArgs ra = rows_args_of(m, d, R);
    ra.dep = nullptr; ra.halo = 0; ra.rep_cells = b->plane_stride;
    ra.wrapx = ra.wrapy = 1;
    ra.part_gain = (const long long*)ws; ra.part_alive = (const long long*)ws + 2 * DIE_MAX_PARTIALS; ra.n_part = n_part;
    ra.part_gain2 = d->agents_die || d->has_dead_slots ? (const long long*)ws + DIE_MAX_PARTIALS : nullptr;
    ra.result = results; ra.alive_const = 0;
    if (rows) return batch_sweep_rows(m, ra, b, s, who, rows, rows_host);
    const int rc = m->dtype == DIE_F32 ? launch_rows<float, 1, true>(ra, R, s, b->replicas) : launch_rows<__half, 1, true>(ra, R, s, b->replicas);
    if (rc != DIE_OK) return rc;
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the three batched steps (a PhysarumAgent, a PhysarumAgent population, a NeuralAutomataAgent population) ----
// Each body is its own checks, batch_world_check, more of its own checks, batch_step_args (+ batch_rows_check), its claim launch
// and batch_step_tail.  The shared checks sit between each entry point's own ones, where they have always been made: when two
// arguments are wrong, the message that wins does not depend on which step was asked for.

// the workspace, the planes and the sizes of every replica.  The NCA step says two of these in its own words (its agents are in
// slot order, its food and chem planes are read by the conv launches) and checks the dtype and the positions it reads itself
static int batch_world_check(const die_medium* m, const die_agents* a, const die_dynamics* d, const die_batch* b, int64_t ws_bytes,
                             bool nca, const char* who) {
    const int rc = batch_ws_check(d, b, ws_bytes, who);
    if (rc != DIE_OK) return rc;
    if (nca) {
        DIE_REQUIRE(m->gW <= 0 && !m->sense_mask && !d->staged && !a->slot,
                    "%s: periodic single-tile replicas in slot order (no sense mask)", who);
        DIE_REQUIRE(m->food && m->chem && m->chem_next && m->chem_next != m->chem, "%s: null plane, or chem_next not a second plane", who);
        DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad field dtype %d", who, m->dtype);
        DIE_REQUIRE(a->x && a->y, "%s: null agent arrays", who);
    } else {
        DIE_REQUIRE(m->gW <= 0 && !m->sense_mask && !d->staged, "%s: periodic single-tile replicas (no sense mask)", who);
        DIE_REQUIRE(m->chem_next && m->chem_next != m->chem, "%s: chem_next must be a second plane", who);
    }
    DIE_REQUIRE(b->plane_stride >= (int64_t)m->W * m->H && b->agent_stride >= a->N, "%s: strides smaller than a replica", who);
    if (!fused_step_applies(m, d)) {
        die_set_error("%s: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4", who);
        return DIE_ERR_UNSUPPORTED;
    }
    return DIE_OK;
}

// after the claim launch: its status, then with dead slots the dead-slot pass + _agent_lifecycle of every replica in one launch
// on the claim pass's grid, then the field sweep
static int batch_step_tail(const BatchLaunch& L, const die_medium* m, const die_dynamics* d, const die_batch* b, die_step_result* results,
                           void* ws, const die_dynamics_row* rows, const die_dynamics_row* rows_host, const char* who) {
    DIE_CHECK_LAUNCH(who);
    if (L.k.has_dead) {
        k_lifecycle_batch<<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(L.k, L.ba);
        DIE_CHECK_LAUNCH(who);
    }
    return batch_sweep(m, d, b, results, ws, (int)L.grid.x, L.s, who, rows, rows_host);
}

// die_forward_env_step_batch (with_rows false) and die_forward_env_step_batch_rows: one body
static int forward_env_step_batch(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                  const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws, int64_t ws_bytes,
                                  bool with_rows, const die_dynamics_row* rows, const die_dynamics_row* rows_host, void* stream,
                                  const char* who) {
    DIE_REQUIRE(m && a && g && d && b && results && ws, "%s: null argument", who);
    int rc = batch_world_check(m, a, d, b, ws_bytes, false, who);
    if (rc != DIE_OK) return rc;
    FwdArgs f;
    rc = die_fill_fwd_args(f, m, a, g, act, who);
    if (rc != DIE_OK) return rc;
    BatchLaunch L;
    rc = batch_step_args(L, m, a, act, d, b, ws, stream, who);
    if (rc != DIE_OK) return rc;
    rc = batch_rows_check(with_rows, b, rows, rows_host, who);
    if (rc != DIE_OK) return rc;
#define DIE_FMCB(T, KIND, LEAN) do { \
        if (with_rows) k_forward_move_claim_batch<T, KIND, LEAN, const die_dynamics_row*><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(f, L.k, L.ba, rows); \
        else k_forward_move_claim_batch<T, KIND, LEAN><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(f, L.k, L.ba); } while (0)
    if (m->dtype == DIE_F32) {
        if (g->kind != DIE_AGENT_PHYSARUM) DIE_FMCB(float, DIE_AGENT_GRADIENT, false);
        else if (fwd_is_lean(g)) DIE_FMCB(float, DIE_AGENT_PHYSARUM, true);
        else DIE_FMCB(float, DIE_AGENT_PHYSARUM, false);
    } else {
        if (g->kind != DIE_AGENT_PHYSARUM) DIE_FMCB(__half, DIE_AGENT_GRADIENT, false);
        else if (fwd_is_lean(g)) DIE_FMCB(__half, DIE_AGENT_PHYSARUM, true);
        else DIE_FMCB(__half, DIE_AGENT_PHYSARUM, false);
    }
#undef DIE_FMCB
    return batch_step_tail(L, m, d, b, results, ws, rows, rows_host, who);
}

extern "C" int die_forward_env_step_batch(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                          const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                          int64_t ws_bytes, void* stream) {
    return forward_env_step_batch(m, a, g, act, d, b, results, ws, ws_bytes, false, nullptr, nullptr, stream, "die_forward_env_step_batch");
}

extern "C" int die_forward_env_step_batch_rows(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                               const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                               int64_t ws_bytes, const die_dynamics_row* rows, const die_dynamics_row* rows_host,
                                               void* stream) {
    return forward_env_step_batch(m, a, g, act, d, b, results, ws, ws_bytes, true, rows, rows_host, stream,
                                  "die_forward_env_step_batch_rows");
}

// die_physarum_env_step_batch (with_rows false) and die_physarum_env_step_batch_rows: one body
static int physarum_env_step_batch(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_physarum_row* table,
                                   const die_action* act, const die_dynamics* d, const die_batch* b, die_step_result* results,
                                   void* ws, int64_t ws_bytes, bool with_rows, const die_dynamics_row* rows,
                                   const die_dynamics_row* rows_host, void* stream, const char* who) {
    DIE_REQUIRE(m && a && g && d && b && results && ws, "%s: null argument", who);
    DIE_REQUIRE(table, "%s: null parameter table", who);
    int rc = batch_world_check(m, a, d, b, ws_bytes, false, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(g->kind == DIE_AGENT_PHYSARUM, "%s: kind %d: a population of PhysarumAgents", who, g->kind);
    DIE_REQUIRE(g->inertia == 0.f && g->noise_scale == 0.f && !g->prev_gx && !g->prev_gy && !g->step_base,
                "%s: no inertia, noise, prev_g* or step_base (they are state or constants of one agent, not of a population)", who);
    FwdArgs f;
    rc = die_fill_fwd_args(f, m, a, g, act, who);
    if (rc != DIE_OK) return rc;
    BatchLaunch L;
    rc = batch_step_args(L, m, a, act, d, b, ws, stream, who);
    if (rc != DIE_OK) return rc;
    rc = batch_rows_check(with_rows, b, rows, rows_host, who);
    if (rc != DIE_OK) return rc;
#define DIE_PMCB(T, LEAN) do { \
        if (with_rows) k_physarum_move_claim_batch<T, LEAN, const die_dynamics_row*><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(f, L.k, L.ba, table, rows); \
        else k_physarum_move_claim_batch<T, LEAN><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(f, L.k, L.ba, table); } while (0)
    if (m->dtype == DIE_F32) {
        if (fwd_is_lean(g)) DIE_PMCB(float, true);
        else DIE_PMCB(float, false);
    } else {
        if (fwd_is_lean(g)) DIE_PMCB(__half, true);
        else DIE_PMCB(__half, false);
    }
#undef DIE_PMCB
    return batch_step_tail(L, m, d, b, results, ws, rows, rows_host, who);
}

extern "C" int die_physarum_env_step_batch(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_physarum_row* table,
                                           const die_action* act, const die_dynamics* d, const die_batch* b, die_step_result* results,
                                           void* ws, int64_t ws_bytes, void* stream) {
    return physarum_env_step_batch(m, a, g, table, act, d, b, results, ws, ws_bytes, false, nullptr, nullptr, stream,
                                   "die_physarum_env_step_batch");
}

extern "C" int die_physarum_env_step_batch_rows(const die_medium* m, const die_agents* a, die_gradient_agent* g,
                                                const die_physarum_row* table, const die_action* act, const die_dynamics* d,
                                                const die_batch* b, die_step_result* results, void* ws, int64_t ws_bytes,
                                                const die_dynamics_row* rows, const die_dynamics_row* rows_host, void* stream) {
    return physarum_env_step_batch(m, a, g, table, act, d, b, results, ws, ws_bytes, true, rows, rows_host, stream,
                                   "die_physarum_env_step_batch_rows");
}

// die_env_step_batch (with_rows false) and die_env_step_batch_rows: one body.  No forward: the claim pass reads the caller's actions
static int env_step_batch(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d, const die_batch* b,
                          die_step_result* results, void* ws, int64_t ws_bytes, bool with_rows, const die_dynamics_row* rows,
                          const die_dynamics_row* rows_host, void* stream, const char* who) {
    DIE_REQUIRE(m && a && act && d && b && results && ws, "%s: null argument", who);
    int rc = batch_world_check(m, a, d, b, ws_bytes, false, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(act->dx && act->dy && act->deposit, "%s: null action arrays", who);
    DIE_REQUIRE(m->food && m->chem && a->x && a->y && !a->slot, "%s: null plane or agent array, or agents not in slot order", who);
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad field dtype %d", who, m->dtype);
    BatchLaunch L;
    rc = batch_step_args(L, m, a, act, d, b, ws, stream, who);
    if (rc != DIE_OK) return rc;
    rc = batch_rows_check(with_rows, b, rows, rows_host, who);
    if (rc != DIE_OK) return rc;
    if (with_rows) {
        if (m->dtype == DIE_F32) k_action_move_claim_batch<float, const die_dynamics_row*><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(L.k, L.ba, rows);
        else k_action_move_claim_batch<__half, const die_dynamics_row*><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(L.k, L.ba, rows);
    } else {
        if (m->dtype == DIE_F32) k_action_move_claim_batch<float><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(L.k, L.ba);
        else k_action_move_claim_batch<__half><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(L.k, L.ba);
    }
    return batch_step_tail(L, m, d, b, results, ws, rows, rows_host, who);
}

extern "C" int die_env_step_batch(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                  const die_batch* b, die_step_result* results, void* ws, int64_t ws_bytes, void* stream) {
    return env_step_batch(m, a, act, d, b, results, ws, ws_bytes, false, nullptr, nullptr, stream, "die_env_step_batch");
}

extern "C" int die_env_step_batch_rows(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                       const die_batch* b, die_step_result* results, void* ws, int64_t ws_bytes,
                                       const die_dynamics_row* rows, const die_dynamics_row* rows_host, void* stream) {
    return env_step_batch(m, a, act, d, b, results, ws, ws_bytes, true, rows, rows_host, stream, "die_env_step_batch_rows");
}

// die_nca_wide_env_step_batch_memory's own arguments (die_memory.hip: the agents' memory channels)
struct MemoryStep {
    int M;                       // memory channels, 1..DIE_MEMORY_MAX_CHANNELS
    float* mem;                  // (R, M, agent_stride)
    float* planes;               // plane j of replica r at (j * R + r) * plane_stride
    bool with_stock;             // layer 0 also reads the standing planes as its stock channel
};

// die_nca_wide_env_step_batch_signal's own arguments (die_signal.hip: the field the agents write and read)
struct SignalStep {
    int K;                       // signal channels, 1..DIE_SIGNAL_MAX_CHANNELS
    const float* field_in;       // plane k of replica r at (k * R + r) * plane_stride: layer 0 reads them, the update reads them again
    float* field_out;            // … and writes these, laid out alike
    float deposit, sigma, decay;
    bool with_stock;             // layer 0 also reads the standing planes as its stock channel (with or without memory)
};

// die_nca_env_step_batch (drop null) and die_nca_env_step_batch_dropout: one body; the mask only changes the last conv launch.
// `wide` (die_nca_wide_env_step_batch): the stack's check and its sensing are die_nca_wide.hip's, which hand back the same
// (sense pointer, replica stride); everything after the sensing is shared.
// `stock` (die_nca_env_step_batch_stock / die_nca_wide_env_step_batch_stock; null: the call without it): the R stock planes of
// die_stock.hip.  Layer 0 then reads one plane more; after every check the planes are built at sense_epoch (one launch more,
// L + 3 in all), layer 0 reads them as its last input, and on the epoch wrap they are cleared with the claim planes.
// `ms` (die_nca_wide_env_step_batch_memory; wide stacks only, `stock` then holds the standing planes whether or not layer 0 reads
// them): after the build the memory is expanded into its planes, layer 0 reads them after the field's, the last layer gives
// 3 + M planes and the planes 3.. are read out into the memory before the claim launch moves anything: L + 5 launches.
// `ss` (die_nca_wide_env_step_batch_signal; wide stacks only, `stock` the standing planes, `ms` null for M = 0): layer 0 reads the
// K field planes after chem, the last layer gives 3 + K + M planes — the memory read-out then starts at plane 3 + K — and after
// the read-outs ONE launch updates the field from the planes 3 .. 3 + K - 1 at the standing planes' cells: L + 4, L + 6 with memory.
static int nca_env_step_batch(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                              const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws, int64_t ws_bytes,
                              const die_nca_dropout* drop, void* stream, const char* who, bool with_rows = false,
                              const die_dynamics_row* rows = nullptr, const die_dynamics_row* rows_host = nullptr, bool wide = false,
                              unsigned long long* stock = nullptr, const MemoryStep* ms = nullptr, const SignalStep* ss = nullptr) {
    DIE_REQUIRE(m && a && nca && d && b && results && ws, "%s: null argument", who);
    int rc = batch_world_check(m, a, d, b, ws_bytes, true, who);
    if (rc != DIE_OK) return rc;
    const bool sense_stock = stock && (ss ? ss->with_stock : !ms || ms->with_stock);
    rc = die_nca_stack_check(wide ? DIE_NCA_WIDE : DIE_NCA_NARROW, nca, m->W, m->H, b->replicas, who, true, sense_stock, ms ? ms->M : 0,
                             ss ? ss->K : 0);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(nca->sense_epoch >= 1 && nca->sense_epoch <= DIE_OWNER_EPOCH_MAX && m->epoch == nca->sense_epoch % DIE_OWNER_EPOCH_MAX + 1,
                "%s: claims at epoch %d cannot follow sensing at epoch %d", who, m->epoch, nca->sense_epoch);
    DIE_REQUIRE(!act || (act->dx && act->dy && act->deposit), "%s: bad action arrays", who);
    BatchLaunch L;
    rc = batch_step_args(L, m, a, act, d, b, ws, stream, who);
    if (rc != DIE_OK) return rc;
    DropWords dw;
    if (drop) {
        rc = die_dropout_words(drop, &dw, who);
        if (rc != DIE_OK) return rc;
    }
    rc = batch_rows_check(with_rows, b, rows, rows_host, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    if (ss) {                                                         // the field's own rules, after the parent's and before any launch
        rc = die_signal_check(m, ss->K, nca->sense_epoch, ss->deposit, ss->sigma, ss->decay, who);
        if (rc != DIE_OK) return rc;
        const int64_t planes = (int64_t)b->replicas * b->plane_stride;
        rc = die_signal_overlap_check(ss->field_in, ss->field_out, (((int64_t)ss->K * b->replicas - 1) * b->plane_stride + cells) * 4, nca->scratch,
                                      nca->scratch_bytes, stock, ((int64_t)(b->replicas - 1) * b->plane_stride + cells) * 8, who);
        if (rc != DIE_OK) return rc;
        DIE_REQUIRE(!ms || !die_ranges_overlap(ss->field_out, ss->K * planes * 4, ms->planes, ms->M * planes * 4),
                    "%s: field_out overlaps the memory planes", who);
    }
    NcaReadArgs q;
    if (stock) {                                                      // every replica's stocks as they are now, tagged sense_epoch
        rc = die_stock_launch(m, a, b->replicas, b->n, b->agent_stride, b->plane_stride, nca->sense_epoch, stock, stream, who);
        if (rc != DIE_OK) return rc;
    }
    if (ms) {                                                         // the memory of whoever stands on a cell, as planes
        rc = die_memory_planes_launch(m->W, m->H, b->replicas, b->n, stock, b->plane_stride, nca->sense_epoch, ms->M, ms->mem, b->agent_stride,
                                      (int64_t)ms->M * b->agent_stride, ms->planes, (int64_t)b->replicas * b->plane_stride, b->plane_stride,
                                      stream, who);
        if (rc != DIE_OK) return rc;
    }
    // reads the claim plane at sense_epoch …
    rc = wide ? die_nca_wide_sense_batch(m, b, nca, &q.sense, &q.rep, drop ? &dw : nullptr, stream, sense_stock ? stock : nullptr,
                                         ms ? ms->planes : nullptr, ms ? ms->M : 0, ss ? ss->field_in : nullptr, ss ? ss->K : 0)
              : die_nca_sense_batch(m, b, nca, &q.sense, &q.rep, drop ? &dw : nullptr, stream, stock);
    if (rc != DIE_OK) return rc;
    if (ms) {                                                         // planes 3.. at the cells the agents stand on NOW: before the claim launch moves anything
        rc = die_gather_memory_launch(m, a, b->replicas, b->n, b->agent_stride, ms->M, q.sense + (3 + (ss ? ss->K : 0)) * (int64_t)m->W * m->H,
                                      (int64_t)m->W * m->H, q.rep, ms->mem, b->agent_stride, (int64_t)ms->M * b->agent_stride, stream, who);
        if (rc != DIE_OK) return rc;
    }
    if (ss) {                                                         // planes 3 .. 3 + K - 1 at the standing planes' cells, into the second buffer
        rc = die_signal_launch(m->W, m->H, b->replicas, ss->K, stock, b->plane_stride, nca->sense_epoch, q.sense + 3 * cells, cells, q.rep,
                               ss->field_in, ss->field_out, b->plane_stride, ss->deposit, ss->sigma, ss->decay, stream, who);
        if (rc != DIE_OK) return rc;
    }
    if (nca->sense_epoch == DIE_OWNER_EPOCH_MAX) {                    // … which is cleared before the tag 1 claims
        const int64_t words = (int64_t)(b->replicas - 1) * b->plane_stride + (int64_t)m->W * m->H;
        if (hipMemsetAsync(m->owner, 0, (size_t)words * sizeof(unsigned long long), L.s) != hipSuccess) {
            die_set_error("%s: clearing the claim planes failed", who);
            return DIE_ERR_HIP;
        }
        // (the stock planes start their 1..31 cycle over with them: the next build is tagged 1)
        if (stock && hipMemsetAsync(stock, 0, (size_t)words * sizeof(unsigned long long), L.s) != hipSuccess) {
            die_set_error("%s: clearing the stock planes failed", who);
            return DIE_ERR_HIP;
        }
    }
    q.cells = (int64_t)m->W * m->H;
    for (int c = 0; c < 3; ++c) q.coef[c] = nca->coef[c];
    q.act[0] = act ? act->dx : nullptr; q.act[1] = act ? act->dy : nullptr; q.act[2] = act ? act->deposit : nullptr;
    if (with_rows) {
        if (m->dtype == DIE_F32) k_nca_move_claim_batch<float, const die_dynamics_row*><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(q, L.k, L.ba, rows);
        else k_nca_move_claim_batch<__half, const die_dynamics_row*><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(q, L.k, L.ba, rows);
    } else {
        if (m->dtype == DIE_F32) k_nca_move_claim_batch<float><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(q, L.k, L.ba);
        else k_nca_move_claim_batch<__half><<<L.grid, DIE_STEP_BLOCK, 0, L.s>>>(q, L.k, L.ba);
    }
    return batch_step_tail(L, m, d, b, results, ws, rows, rows_host, who);
}

extern "C" int die_nca_env_step_batch_rows(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                           const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                           int64_t ws_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                           const die_dynamics_row* rows_host, void* stream) {
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, "die_nca_env_step_batch_rows", true, rows, rows_host);
}

extern "C" int die_nca_wide_env_step_batch(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                           const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                           int64_t ws_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                           const die_dynamics_row* rows_host, void* stream) {
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, "die_nca_wide_env_step_batch", rows || rows_host,
                              rows, rows_host, true);
}

// stock null: the parent call itself, under its own name
extern "C" int die_nca_env_step_batch_stock(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                            const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                            int64_t ws_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                            const die_dynamics_row* rows_host, unsigned long long* stock, void* stream) {
    if (!stock) return die_nca_env_step_batch_rows(m, a, nca, act, d, b, results, ws, ws_bytes, drop, rows, rows_host, stream);
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, "die_nca_env_step_batch_stock", rows || rows_host, rows,
                              rows_host, false, stock);
}

extern "C" int die_nca_wide_env_step_batch_stock(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                                 const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                                 int64_t ws_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                                 const die_dynamics_row* rows_host, unsigned long long* stock, void* stream) {
    if (!stock) return die_nca_wide_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, rows, rows_host, stream);
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, "die_nca_wide_env_step_batch_stock",
                              rows || rows_host, rows, rows_host, true, stock);
}

extern "C" int die_nca_wide_env_step_batch_memory(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                                  const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                                  int64_t ws_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                                  const die_dynamics_row* rows_host, unsigned long long* standing, int32_t memory_channels,
                                                  float* memory, float* memory_planes, int32_t with_stock, void* stream) {
    const char* who = "die_nca_wide_env_step_batch_memory";
    DIE_REQUIRE(standing && memory && memory_planes, "%s: null standing planes, memory or memory planes", who);
    DIE_REQUIRE(memory_channels >= 1 && memory_channels <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who, memory_channels,
                DIE_MEMORY_MAX_CHANNELS);
    DIE_REQUIRE(with_stock == 0 || with_stock == 1, "%s: with_stock is 0 or 1", who);
    const MemoryStep ms = {memory_channels, memory, memory_planes, with_stock == 1};
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, who, rows || rows_host, rows, rows_host, true, standing,
                              &ms);
}

// the memory variant's arguments (memory_channels = 0 with null memory pointers: none) and the signal field's
extern "C" int die_nca_wide_env_step_batch_signal(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                                  const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                                  int64_t ws_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                                  const die_dynamics_row* rows_host, unsigned long long* standing, int32_t memory_channels,
                                                  float* memory, float* memory_planes, int32_t with_stock, int32_t signal_channels,
                                                  const float* field_in, float* field_out, float deposit, float sigma, float decay,
                                                  void* stream) {
    const char* who = "die_nca_wide_env_step_batch_signal";
    DIE_REQUIRE(standing && field_in && field_out, "%s: null standing planes or signal field", who);
    DIE_REQUIRE(memory_channels >= 0 && memory_channels <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 0..%d", who, memory_channels,
                DIE_MEMORY_MAX_CHANNELS);
    DIE_REQUIRE(memory_channels ? memory && memory_planes : !memory && !memory_planes, "%s: %d memory channels need both the memory and its "
                "planes, none needs neither", who, memory_channels);
    DIE_REQUIRE(with_stock == 0 || with_stock == 1, "%s: with_stock is 0 or 1", who);
    DIE_REQUIRE(signal_channels >= 1 && signal_channels <= DIE_SIGNAL_MAX_CHANNELS, "%s: %d signal channels outside 1..%d", who, signal_channels,
                DIE_SIGNAL_MAX_CHANNELS);
    const MemoryStep ms = {memory_channels, memory, memory_planes, with_stock == 1};
    const SignalStep ss = {signal_channels, field_in, field_out, deposit, sigma, decay, with_stock == 1};
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, who, rows || rows_host, rows, rows_host, true, standing,
                              memory_channels ? &ms : nullptr, &ss);
}

extern "C" int die_nca_env_step_batch(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                      const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                      int64_t ws_bytes, void* stream) {
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, nullptr, stream, "die_nca_env_step_batch");
}

extern "C" int die_nca_env_step_batch_dropout(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                              const die_dynamics* d, const die_batch* b, die_step_result* results, void* ws,
                                              int64_t ws_bytes, const die_nca_dropout* drop, void* stream) {
    return nca_env_step_batch(m, a, nca, act, d, b, results, ws, ws_bytes, drop, stream, "die_nca_env_step_batch_dropout");
}

static int deposit_feed_diffuse(const die_medium* m, const die_dynamics* d, int halo, bool tile, void* stream,
                                const char* who, const long long* part_gain, int n_part, die_step_result* result,
                                long long alive_const, const long long* part_alive, const float* dep_plane) {
    DIE_REQUIRE(m && d, "%s: null argument", who);
    DIE_REQUIRE((m->owner || dep_plane) && m->food && m->chem && m->chem_next && m->chem_next != m->chem, "%s: null or aliased plane", who);
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad dtype %d", who, m->dtype);
    DIE_REQUIRE(dep_plane || (m->epoch >= 1 && m->epoch <= DIE_OWNER_EPOCH_MAX), "%s: bad epoch %d", who, m->epoch);
    const int R = die_gaussian_radius(d->diffuse_sigma);
    if (!(rows_kernel_applies(m->W, m->H, R) && R >= 1 && (!tile || (m->H >= 8 && m->W >= 2 * R + 1 && halo >= 0)))) {
        die_set_error("%s: needs H %% 4 == 0 and radius 1..4 (W=%d H=%d sigma=%g halo=%d)", who, m->W, m->H,
                      (double)d->diffuse_sigma, halo);
        return DIE_ERR_UNSUPPORTED;
    }
    RowsArgs ra = rows_args_of(m, d, R);
    ra.dep = dep_plane; ra.halo = halo; ra.rep_cells = 0;
    ra.wrapx = tile && m->gW > 0 && m->W == m->gW; ra.wrapy = tile && m->gW > 0 && m->H == m->gH;
    ra.part_gain = part_gain; ra.part_gain2 = nullptr; ra.part_alive = part_alive; ra.n_part = n_part; ra.result = result; ra.alive_const = alive_const;
    int rc;
    if (dep_plane) {
        DIE_REQUIRE(!tile, "%s: the deposit-plane sweep is for periodic single-tile planes", who);
        rc = m->dtype == DIE_F32 ? launch_rows<float, 2, true>(ra, R, (hipStream_t)stream)
                                 : launch_rows<__half, 2, true>(ra, R, (hipStream_t)stream);
    }
    else if (tile) rc = m->dtype == DIE_F32 ? launch_rows<float, 1, false>(ra, R, (hipStream_t)stream)
                                            : launch_rows<__half, 1, false>(ra, R, (hipStream_t)stream);
    else rc = m->dtype == DIE_F32 ? launch_rows<float, 1, true>(ra, R, (hipStream_t)stream)
                                  : launch_rows<__half, 1, true>(ra, R, (hipStream_t)stream);
    if (rc != DIE_OK) return rc;
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// the field half of the tile-binned step (die_pic.hip): the sweep reads the winners' deposits from a float plane
int die_sweep_dep_plane(const die_medium* m, const die_dynamics* d, const float* dep_plane, const long long* part_gain, int n_part,
                        die_step_result* result, long long alive_const, void* stream) {
    DIE_REQUIRE(dep_plane, "die_pic_step: null deposit plane");
    if (!fused_step_applies(m, d)) {
        die_set_error("die_pic_step: only for periodic planes with H %% 4 == 0 and gaussian radius 1..4");
        return DIE_ERR_UNSUPPORTED;
    }
    return deposit_feed_diffuse(m, d, 0, false, stream, "die_pic_step(diffuse+deposit+feed+reduce)", part_gain, n_part, result,
                                alive_const, nullptr, dep_plane);
}

extern "C" int die_medium_deposit_feed_diffuse(const die_medium* m, const die_dynamics* d, void* stream) {
    DIE_REQUIRE(m && m->gW <= 0, "die_medium_deposit_feed_diffuse: periodic single-tile planes only "
                                 "(decomposed tiles: die_medium_deposit_feed_diffuse_tile)");
    return deposit_feed_diffuse(m, d, 0, false, stream, "die_medium_deposit_feed_diffuse");
}

extern "C" int die_medium_deposit_feed_diffuse_tile(const die_medium* m, const die_dynamics* d, int32_t halo, void* stream) {
    return deposit_feed_diffuse(m, d, halo, true, stream, "die_medium_deposit_feed_diffuse_tile");
}

extern "C" int die_tile_sweep_reduce(const die_medium* m, const die_agents* a, const die_dynamics* d, int32_t halo,
                                     die_step_result* result, void* ws, int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(m && a && d && result && ws, "die_tile_sweep_reduce: null argument");
    DIE_REQUIRE(ws_bytes >= WS_PARTS, "die_tile_sweep_reduce: workspace too small");
    DIE_REQUIRE(!(d->has_dead_slots || d->agents_die), "die_tile_sweep_reduce: a dead-slot pass needs die_step_reduce_ex");
    const bool counted = m->gW > 0 && m->own_x1 > 0;       // ghost tiles: the claim pass counted the owned alive slots
    return deposit_feed_diffuse(m, d, halo, true, stream, "die_tile_sweep_reduce", (const long long*)ws, step_grid(a->N), result,
                                a->N, counted ? (const long long*)ws + 2 * DIE_MAX_PARTIALS : nullptr);
}

extern "C" int die_agent_dead_slots(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                                    void* ws, int64_t ws_bytes, void* stream) {
    StepArgs k;
    int rc = fill_args(k, m, a, act, d, ws, ws_bytes, "die_agent_dead_slots");
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(act, "die_agent_dead_slots: null action");
    k.part_gain = (long long*)ws + DIE_MAX_PARTIALS;
    k.part_alive = (long long*)ws + 2 * DIE_MAX_PARTIALS;
    k.skip_scatter = 1;
    const int grid = step_grid(a->N);
    if (m->dtype == DIE_F32) k_resolve<float><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    else k_resolve<__half><<<grid, DIE_STEP_BLOCK, 0, (hipStream_t)stream>>>(k);
    DIE_CHECK_LAUNCH("die_agent_dead_slots");
    return DIE_OK;
}

// ---- self-check of die_wave_sum_i64_dpp (die_common.h): one total per wave of 64 values --------------------------------
__global__ __launch_bounds__(DIE_BLOCK) void k_wave_sum_i64_check(const long long* in, int64_t n_waves, long long* out) {
    const int64_t w = (int64_t)blockIdx.x * (DIE_BLOCK / DIE_WAVE) + threadIdx.x / DIE_WAVE;
    if (w >= n_waves) return;                                   // (wave-uniform: the waves that go on are whole)
    const int lane = threadIdx.x & (DIE_WAVE - 1);
    const long long t = die_wave_sum_i64_dpp(in[w * DIE_WAVE + lane]);
    if (lane == 0) out[w] = t;
}

extern "C" int die_wave_sum_i64_check(const void* in, int64_t n_waves, void* out, void* stream) {
    DIE_REQUIRE(in && out, "die_wave_sum_i64_check: null array");
    DIE_REQUIRE(n_waves >= 1 && n_waves <= (1 << 20), "die_wave_sum_i64_check: n_waves %lld outside [1, 2^20]", (long long)n_waves);
    k_wave_sum_i64_check<<<die_grid_for(n_waves * DIE_WAVE), DIE_BLOCK, 0, (hipStream_t)stream>>>((const long long*)in, n_waves, (long long*)out);
    DIE_CHECK_LAUNCH("die_wave_sum_i64_check");
    return DIE_OK;
}

// ---- error plumbing ---------------------------------------------------------------------
static thread_local char g_err[512] = "";

void die_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* die_last_error(void) { return g_err; }
extern "C" int die_abi_version(void) { return DIE_ABI_VERSION; }
