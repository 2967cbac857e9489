/* die_hip.h — C ABI of libdie_hip.so: the MI355X (gfx950) implementation of the grid-update
 * hot path of gkirgizov/die (Env.step field dynamics + Agent.forward + data_init allocation).
 *
 * The reference has no FFI: the boundary it offers is the Python class API of core/env.py,
 * core/agent/ (all modules) and core/data_init.py.  The host side of this project
 * (the die_amd package) keeps those classes and calls the entry points below through ctypes; each
 * entry point names the reference function(s) it replaces.  Paths are relative to the
 * reference checkout.
 *
 * Conventions
 *   - plain C, no exceptions; every call returns DIE_OK (0) or a negative die_status and
 *     leaves a message for die_last_error() (thread-local).
 *   - all pointers in the structs are DEVICE pointers (HBM) owned by the caller; the library
 *     allocates nothing and keeps no state.  `stream` is a hipStream_t (NULL = default
 *     stream); every call only enqueues work on it and returns without synchronising.
 *   - field planes are W×H row-major, element (ix, iy) at ix*H + iy — the (channel, x, y)
 *     layout of core/data_init.py:95-112 with one plane per channel.
 *   - agent coordinates are Q0.32 fixed point: x = X / 2^32 in [0, 1).  The nearest-cell
 *     lookup of core/utils.py:39-54 is then exact integer arithmetic,
 *     cell = clamp((X*(W-1) + 2^31) >> 32, 0, W-1), and the `% 1.` wrap of
 *     core/env.py:155 is the natural 32-bit overflow.
 *   - the 'agents' medium channel (core/base_types.py:32) is held as a 64-bit claim per cell:
 *     high word (epoch << 27) | (slot + 1) of the highest-index alive agent standing on the
 *     cell in step `epoch`, low word the fp32 bits of that agent's deposit.  A cell is occupied
 *     iff claim >> 59 == current epoch (epoch in 1..31, the caller zeroes the plane when it
 *     wraps: once in 31 steps; 27 bits hold up to 134 M world slots).  One 64-bit atomicMax per agent: highest slot wins == the "last writer wins" of
 *     core/env.py:211, and the winner's deposit reaches the diffusion sweep without a second
 *     per-agent pass.
 */
#ifndef DIE_HIP_H
#define DIE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIE_ABI_VERSION 24

typedef enum die_status {
    DIE_OK = 0,
    DIE_ERR_ARG = -1,         /* null pointer, bad size, unsupported enum value */
    DIE_ERR_HIP = -2,         /* a HIP runtime call or kernel launch failed */
    DIE_ERR_UNSUPPORTED = -3  /* valid in the reference, not implemented on device */
} die_status;

typedef enum die_dtype { DIE_F32 = 0, DIE_F16 = 1 } die_dtype;

/* core/env.py:24-26 BoundaryCondition; anything else passes coordinates through (:158-161) */
typedef enum die_boundary { DIE_BOUNDARY_WRAP = 0, DIE_BOUNDARY_LIMIT = 1, DIE_BOUNDARY_NONE = 2 } die_boundary;

/* core/env.py:29-39 action-cost operators available on device */
typedef enum die_cost { DIE_COST_LINEAR = 0, DIE_COST_ZERO = 1 } die_cost;

/* core/agent/gradient.py: which forward() a call computes */
typedef enum die_agent_kind { DIE_AGENT_GRADIENT = 0, DIE_AGENT_PHYSARUM = 1 } die_agent_kind;

#define DIE_OWNER_EPOCH_SHIFT 27
#define DIE_OWNER_EPOCH_MAX 31
#define DIE_OWNER_SLOT_MASK 0x07FFFFFFu

/* The (3, W, H) medium of core/env.py:75-79 / core/base_types.py:32. */
typedef struct die_medium {
    int32_t W, H;
    int32_t dtype;       /* die_dtype of food / chem / chem_next */
    int32_t epoch;       /* current ownership epoch, 1..DIE_OWNER_EPOCH_MAX */
    uint64_t* owner;     /* 'agents' channel, W*H claim words (see header comment) */
    void* food;          /* 'env_food', W*H */
    void* chem;          /* 'chem1', W*H, current */
    void* chem_next;     /* W*H, receives the diffused plane; the caller swaps after die_env_step */
    /* Domain decomposition.  gW == 0: the planes ARE the periodic W×H world.
     * gW > 0: the planes are one rank's tile of a gW×gH world, halo included: local element
     * (i, j) is global cell (ox + i, oy + j); agent coordinates stay global; nothing wraps
     * inside the tile (the halo is filled by the caller's exchange). */
    int32_t gW, gH;
    int32_t ox, oy;
    /* Ghost-agent decomposition: a rank also steps copies of its neighbours' agents that stand in
     * its halo, so reward / num_alive must only count the agents standing on the cells this rank accounts for:
     * local rows [own_x0, own_x1) × columns [own_y0, own_y1).  own_x1 == 0: every cell counts.
     * An axis with W == gW (one rank along it) has no halo and is periodic inside the tile. */
    int32_t own_x0, own_y0, own_x1, own_y1;
    /* Dynamics.apply_sense_mask (core/env.py:276-295): W*H bytes from die_sense_mask; the forward kernels read the
     * chem / food of a cell with mask 0 as 0.  NULL: everything is visible. */
    const uint8_t* sense_mask;
} die_medium;

/* The (4, N) agent array of core/data_init.py:114-150, structure of arrays. */
typedef struct die_agents {
    int64_t N;           /* slots (alive or not) */
    uint32_t* x;         /* Q0.32 */
    uint32_t* y;         /* Q0.32 */
    uint8_t* alive;      /* 1 / 0 */
    float* agent_food;
    uint32_t* slot;      /* reference slot id of each array entry, or NULL = identity.  The arrays may be
                            held in any order (die_agents_sort keeps them spatially sorted); Philox
                            counters and ownership words always use the slot id, so results do not
                            depend on the order. */
} die_agents;

/* The (3, N) action array of core/data_init.py:152-157. */
typedef struct die_action {
    int64_t N;
    float* dx;
    float* dy;
    float* deposit;
} die_action;

/* core/env.py:42-61 Dynamics, the fields the device path honours. */
/* scipy.ndimage boundary modes as skimage.filters.gaussian passes them through (core/env.py:140-143) */
typedef enum die_diffuse_mode { DIE_DIFFUSE_WRAP = 0, DIE_DIFFUSE_NEAREST = 1, DIE_DIFFUSE_REFLECT = 2, DIE_DIFFUSE_MIRROR = 3,
                                DIE_DIFFUSE_CONSTANT = 4 } die_diffuse_mode;

typedef struct die_dynamics {
    float rate_feed;
    float rate_decay_chem;
    float diffuse_sigma;
    int32_t boundary;        /* die_boundary */
    int32_t cost;            /* die_cost */
    float cost_w_deposit;    /* 0.02 (core/env.py:29) */
    float cost_w_dist;       /* 0.01 */
    int32_t food_infinite;
    int32_t agents_die;
    int32_t has_dead_slots;  /* 0: caller guarantees every slot is alive (skips the dead-slot feed pass) */
    int32_t diffuse_mode;    /* die_diffuse_mode (Dynamics.diffuse_mode, core/env.py:49,142); only WRAP takes the fused sweep */
    int32_t staged;          /* 1: die_env_step runs its stages one kernel each (move/claim, resolve, reduce, diffuse) even where
                                the fused field sweep applies — same bits, for cross-checks (tests) */
} die_dynamics;

/* core/agent/gradient.py:19-28,139-151 constructor arguments + per-agent state. */
typedef struct die_gradient_agent {
    int32_t kind;            /* die_agent_kind */
    int32_t normalized_grad;
    float scale;
    float deposit;
    float inertia;
    float sense_offset;
    float noise_scale;
    float grad_clip;         /* < 0: None */
    /* The heading and the turn decision are float64, like the reference's (core/agent/gradient.py:168-208): the decision
     * `abs(dir_delta) > sense_radians` is an exact tie whenever a probe sits on the symmetry axis of a deposit, and which way
     * it falls is decided by the low bits of the heading — fp32 headings resolved ~0.1 % of agents differently per step. */
    double turn_radians;     /* physarum only: np.radians(turn_angle) */
    double sense_radians;
    double turn_tolerance;
    uint32_t* heading_hi;    /* N + N words: _direction_rads as float64, high and low halves in two arrays (state, read and */
    uint32_t* heading_lo;    /* written) — two 4-byte arrays travel through the sort / migration machinery like any other */
    float* prev_gx;          /* N, _prev_grad[0]; may be NULL when inertia == 0 */
    float* prev_gy;          /* N */
    const int8_t* turn_sign; /* N entries ±1 (indexed by SLOT id) replacing the random turn, or NULL → Philox(seed, step, slot) */
    uint64_t seed;
    uint32_t step;           /* forward-call counter, the Philox step word */
    uint32_t reserved2;
    const uint32_t* step_base; /* device word added to `step`, or NULL: lets a captured hipGraph of many steps be replayed
                                  (the launch arguments are frozen, the counter is not) */
} die_gradient_agent;

/* Device-resident result of one die_env_step (read it back after synchronising). */
typedef struct die_step_result {
    double reward;           /* sum of `gained` over every slot (core/env.py:119-120), accumulated in 32.32 fixed point:
                                identical bits whatever the order of the agent arrays or the decomposition */
    int64_t num_alive;       /* core/env.py:263-265 */
} die_step_result;

int die_abi_version(void);
const char* die_last_error(void);

/* Bytes of scratch die_env_step / die_init_agents need for this problem size. */
int64_t die_workspace_bytes(int32_t W, int32_t H, int64_t N);

/* ---- Agent.forward ------------------------------------------------------------------
 * GradientAgent.forward / PhysarumAgent.forward (core/agent/gradient.py:96-124, 168-219):
 * one forward probe of the normalised np.gradient of chem1 (4 taps around the probe cell,
 * :55-76), discrete turn, momentum, deposit; writes the action and updates agent state.
 * Every slot acts, alive or not, as in the reference. */
int die_gradient_forward(const die_medium* m, const die_agents* a, die_gradient_agent* g,
                         die_action* out, void* stream);

/* GradientAgent.render (core/agent/gradient.py:126-135): rgb_out (W, H, 3) fp32 = 0.5 * (stack(gx, gy, 0) + 1) of the
 * normalised, clipped np.gradient field of the chem plane (_get_gradient, :55-71). */
int die_gradient_render(const void* chem, int32_t W, int32_t H, int32_t dtype, int32_t normalized, float grad_clip,
                        float* rgb_out, void* stream);

/* BrownianAgent.forward (core/agent/static.py:40-50): (b-a)*u.round(3)+a per channel, × alive. */
int die_brownian_forward(const die_agents* a, float move_scale, float deposit_scale,
                         uint64_t seed, uint32_t step, die_action* out, void* stream);

/* ConstAgent.forward (core/agent/static.py:20-27). */
int die_const_forward(int64_t N, float dx, float dy, float deposit, die_action* out, void* stream);

/* ---- Env.step -------------------------------------------------------------------------
 * core/env.py:101-131 in one call: _agent_move (:163-172), _agent_deposit_and_layout
 * (:204-215), _agent_feed (:220-243), _agent_lifecycle (:245-261, agents_die only),
 * _medium_diffuse_decay (:136-145) and the reward / num_agents reductions (:117-126).
 * `m->epoch` must already be the new step's epoch.  On return (stream order) the diffused
 * plane is in m->chem_next.  `result` is a device pointer. */
int die_env_step(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                 die_step_result* result, void* workspace, int64_t workspace_bytes, void* stream);

/* Agent.forward + Env.step in one call for the common loop `env.step(agent.forward(obs))`
 * (examples/minimal_run.py:24-25): GradientAgent/PhysarumAgent.forward is fused with the move /
 * claim / feeding pass, so the action is written to `act` for the caller but never read back and
 * the agent coordinates are loaded once.  Same results as die_gradient_forward followed by
 * die_env_step.  DIE_ERR_UNSUPPORTED when the fused field sweep does not apply (decomposed tile,
 * H % 4 != 0, gaussian radius > 4): call the two separately then. */
int die_forward_env_step(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                         const die_dynamics* d, die_step_result* result, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* R replicas of one world shape stepped in ONE launch pair (BASELINE configs[4]: batched env replicas; small grids are
 * launch-bound one at a time).  `m`, `a`, `g`, `act` describe replica 0; every array of replica r starts r strides further
 * (planes: plane_stride elements, per-agent arrays: agent_stride elements; results[r]); replica r holds n[r] agent slots
 * and draws from Philox key g->seed + r * seed_stride — so replica r computes exactly what a stand-alone world with
 * that seed computes.  `act` may be NULL (no action written).  Same restrictions as die_forward_env_step, and no sense mask.
 *   d->agents_die (or d->has_dead_slots): one more launch between the claims and the sweep — die_agent_dead_slots of every
 * replica (dead slots finish their feed, _agent_lifecycle zeroes the starved slots, num_alive counts the alive ones), so
 * replica r's result words are die_forward_env_step's.  The claim pass stashes each dead slot's `consumed` and action cost
 * (its action stays in registers); the workspace must then hold die_batch_lifecycle_workspace_bytes(replicas,
 * agent_stride) bytes (−1: bad arguments), else the call is refused before any launch.  Without dead slots nothing changes. */
#define DIE_MAX_REPLICAS 64
typedef struct die_batch {
    int32_t replicas;
    int32_t reserved;
    int64_t plane_stride;
    int64_t agent_stride;
    uint64_t seed_stride;
    int64_t n[DIE_MAX_REPLICAS];
} die_batch;
int64_t die_batch_workspace_bytes(int32_t replicas);
int64_t die_batch_lifecycle_workspace_bytes(int32_t replicas, int64_t agent_stride);
int die_forward_env_step_batch(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                               const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* ---- PhysarumAgent populations: per-replica parameters ----------------------------------------------------------------
 * A device table of one kernel-ready row per replica: what a stand-alone PhysarumAgent of those constructor arguments hands
 * the kernels (die_gradient_agent's scale, deposit, sense_offset, turn_radians, sense_radians, turn_tolerance) and the
 * constants die_forward_env_step derives from them on the host (the np.isclose thresholds of _choose_turn and their cosines).
 * kind, normalized_grad, grad_clip, inertia = 0 and noise_scale = 0 stay shared: they choose the kernel instantiation.
 * 64 bytes, so that a workgroup fetches its replica's row with one scalar load. */
typedef struct die_physarum_row {
    float scale, deposit, sense_offset;
    float c_turn, c_sense;   /* cos(x_turn), cos(sense_radians); 2 / -2 where the angle is outside [0, pi) */
    float reserved;
    double turn_radians, sense_radians, turn_tolerance;
    double x_turn;           /* largest |x| np.isclose(0, x, rtol=1e-2, atol=turn_radians * turn_tolerance) accepts */
    double atol;             /* turn_radians * turn_tolerance */
} die_physarum_row;

/* Column order of a parameter row: scale, deposit, sense_offset, turn_angle, sense_angle (degrees), turn_tolerance. */
#define DIE_PHYSARUM_PARAMS 6
#define DIE_PHYSARUM_NATURAL 0
#define DIE_PHYSARUM_UNIT 1
typedef struct die_parameter_space {
    float lo[DIE_PHYSARUM_PARAMS];
    float hi[DIE_PHYSARUM_PARAMS];
} die_parameter_space;

/* One launch: (replicas, 6) fp32 `rows` -> `table` (replicas rows) and `values` (replicas, 6) fp32, the decoded values.
 *   DIE_PHYSARUM_NATURAL: a row holds the values themselves (`space` is ignored and may be NULL).
 *   DIE_PHYSARUM_UNIT: a row holds search coordinates u; value j = lo[j] + (hi[j] - lo[j]) * clamp(u[j], 0, 1) in fp32, each
 *     operation rounded by itself (a NaN coordinate reads as 0).  `space` is copied at the call; lo <= hi, both finite, and
 *     both ends of every decoded range must be values a PhysarumAgent accepts (scale, sense_offset, turn_tolerance >= 0,
 *     0 < turn_angle <= 180, 0 <= sense_angle <= 180), so that every decoded row is.
 * Degrees become radians as (double)v * (pi / 180) (Python's math.radians); x_turn is found by the bisection
 * die_forward_env_step runs on the host, the cosines by the device's float64 cos rounded to fp32. */
int die_physarum_decode_batch(const float* rows, int32_t replicas, int32_t mode, const die_parameter_space* space,
                              die_physarum_row* table, float* values, void* stream);

/* The same launch for a population with episodes: (candidates, 6) `rows` -> `table` of candidates * episodes rows, row c * E + e
 * being candidate c's (the E replicas that evaluate a candidate step with the same values), and `values` (candidates, 6).
 * candidates * episodes <= DIE_MAX_REPLICAS; episodes = 1 is die_physarum_decode_batch. */
int die_physarum_decode_episodes(const float* rows, int32_t candidates, int32_t episodes, int32_t mode,
                                 const die_parameter_space* space, die_physarum_row* table, float* values, void* stream);

/* die_init_heading of every replica in one launch: replica r covers n[r] slots r * agent_stride behind heading_hi / _lo,
 * draws from key seed + r * seed_stride and discretises with table[r].turn_radians. */
int die_physarum_heading_batch(uint32_t* heading_hi, uint32_t* heading_lo, const die_batch* b, const die_physarum_row* table,
                               uint64_t seed, void* stream);

/* die_forward_env_step_batch with the table: replica r steps with table[r] in place of g's scale, deposit, sense_offset,
 * turn_radians, sense_radians and turn_tolerance (which are ignored).  g->kind must be DIE_AGENT_PHYSARUM, with no
 * inertia, noise, prev_g* or step_base.  Otherwise the same call: same refusals before any launch, same dead-slot pass,
 * fp16 planes, `act` may be NULL. */
int die_physarum_env_step_batch(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_physarum_row* table,
                                const die_action* act, const die_dynamics* d, const die_batch* b, die_step_result* results,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* First kernel of die_forward_env_step alone (forward + move + claim + feeding of alive slots). */
int die_forward_move_claim(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                           const die_dynamics* d, void* workspace, int64_t workspace_bytes, void* stream);

/* Everything of die_forward_env_step / die_env_step after the claims are in place (dead-slot pass if
 * needed, reduction, fused field sweep) — lets a caller put work that only touches the agent arrays
 * (die_agents_sort) on another stream, next to the sweep. */
int die_env_step_finish(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                        die_step_result* result, void* workspace, int64_t workspace_bytes, void* stream);

/* The same kernel on a tile of a decomposed world (claims may land in the halo; the caller merges them
 * across ranks and runs die_medium_deposit_feed_diffuse_tile). */
int die_forward_move_claim_tile(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                const die_dynamics* d, void* workspace, int64_t workspace_bytes, void* stream);

/* The stages of die_env_step, individually (tests and custom update cycles such as
 * examples/simple_agents.py:16-30 `_manual_step`). */
int die_agent_move_claim(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                         void* workspace, int64_t workspace_bytes, void* stream);
int die_agent_resolve(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                      void* workspace, int64_t workspace_bytes, void* stream);
int die_step_reduce(const die_agents* a, const die_dynamics* d, die_step_result* result,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* The field half of a step in ONE sweep (what die_env_step runs after die_agent_move_claim when
 * H % 4 == 0 and the gaussian radius is <= 4): every cell's claim is read, the winner's deposit
 * added (core/env.py:211), occupied cells fed (food -= rate*food, :222-228), and the result
 * diffused and decayed (:136-145) into m->chem_next.  Replaces die_agent_resolve's per-agent
 * scatter + die_diffuse_decay; DIE_ERR_UNSUPPORTED for other shapes (use those two instead). */
int die_medium_deposit_feed_diffuse(const die_medium* m, const die_dynamics* d, void* stream);
/* Same sweep on a halo-padded tile of a decomposed world (no wrap; chem AND claims of the halo
 * must have been exchanged): deposits are applied everywhere, feeding only to the cells at
 * least `halo` away from the array border, the outer `radius` ring of chem_next is unspecified. */
int die_medium_deposit_feed_diffuse_tile(const die_medium* m, const die_dynamics* d, int32_t halo, void* stream);
/* die_medium_deposit_feed_diffuse_tile + die_step_reduce_ex in one launch (no dead-slot pass): an extra workgroup of
 * the sweep sums the claim pass's partials in k_reduce's order (ghost tiles: and its counts of owned alive slots). */
int die_tile_sweep_reduce(const die_medium* medium, const die_agents* agents, const die_dynamics* dynamics, int32_t halo,
                          die_step_result* result, void* ws, int64_t ws_bytes, void* stream);
/* The part of die_agent_resolve that does not touch the field: dead slots finish their feed,
 * lifecycle (agents_die), alive count — for callers that let the field sweep do the scatter. */
int die_agent_dead_slots(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* Decomposed step, first half: positions only (core/env.py:163-172).  tile_of[n] receives the
 * index tile_x * tiles_y + tile_y of the interior tile (tile_w × tile_h cells each) the agent now
 * stands on, so the caller can migrate it before die_agent_claim_feed. */
int die_agent_move(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                   int32_t tile_w, int32_t tile_h, int32_t tiles_y, int32_t* tile_of, void* stream);
/* die_gradient_forward fused with die_agent_move (decomposed worlds; the action is written to `act`). */
int die_forward_move(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                     const die_dynamics* d, int32_t tile_w, int32_t tile_h, int32_t tiles_y, int32_t* tile_of, void* stream);
/* die_step_reduce when the caller knows whether the dead-slot pass ran: without it only the
 * move/claim partials are summed and num_alive = alive_const (with_second_pass: 0 claim pass only; 1 both passes and the
 * dead-slot pass's alive count; 2 ghost tiles; 3 both passes' gains with num_alive = alive_const). */
int die_step_reduce_ex(const die_agents* a, die_step_result* result, void* workspace, int64_t workspace_bytes,
                       int32_t with_second_pass, int64_t alive_const, void* stream);
/* _agent_lifecycle (core/env.py:245-250) on its own: every channel of the slots with agent_food <= 1e-4 becomes 0.  Used by
 * the reference-compatible agents_die mode (die_amd/env.py Env._step_compat), whose claim / feeding lookups run on a frozen
 * copy of the agent array — the reference's stale AgentIndexer (core/env.py:249 vs core/utils.py:22). */
int die_agents_lifecycle(const die_agents* a, void* stream);

/* ---- Dynamics.agents_born (no reference counterpart: core/env.py:256-261 is a TODO) ------------------------
 * The birth half of _agent_lifecycle, run after a step's deaths.  A PARENT is a slot that is alive with agent_food >
 * born_threshold (fp32 compare); a FREE slot is a dead slot below n.  Both are ranked by slot index; parent j breeds into free
 * slot j for j < min(#parents, #free): the child is alive with 0.5f * agent_food, the parent keeps agent_food - child (both
 * exact), and the child stands at the parent's position displaced by (ox, oy) = ((int64)(int32)w.x * q) >> 31, likewise w.y,
 * w = Philox(key world_seed, counter (parent slot, world_step, stream 11)), q = round(born_spread * 2^32) — applied with the
 * move's boundary code (wrapping add / clamp to [0, 2^32 - 1]).  Only the agent arrays are written; `result` (may be NULL)
 * gets the number born added to num_alive.  Three launches, no atomics, the same bits on every run.  The arrays must be in
 * slot order (a->slot == NULL).  The workspace holds die_births_workspace_bytes(replicas, agent_stride) bytes (-1: bad
 * sizes); every refusal happens before any launch. */
typedef struct die_births {
    float born_threshold;
    int32_t boundary;        /* die_boundary: WRAP or LIMIT */
    double born_spread;      /* unit coordinates, 0 .. 0.5 */
    uint32_t world_step;     /* steps since construction / reset */
    uint32_t reserved;
} die_births;
int64_t die_births_workspace_bytes(int32_t replicas, int64_t agent_stride);
int die_agent_births(const die_agents* a, const die_births* p, uint64_t world_seed, die_step_result* result, void* workspace,
                     int64_t workspace_bytes, void* stream);
/* The same pass on every replica of a die_batch in the same three launches: `a` describes replica 0, replica r's arrays start
 * r * b->agent_stride elements further and hold b->n[r] slots; world_seeds is a HOST array of b->replicas keys, read during the
 * call; results[r] (may be NULL) gets replica r's number born.  Replica r ends exactly as die_agent_births on it alone. */
int die_agent_births_batch(const die_agents* a, const die_batch* b, const die_births* p, const uint64_t* world_seeds,
                           die_step_result* results, void* workspace, int64_t workspace_bytes, void* stream);
/* ---- The record of a birth pass, and heredity (die_births.hip, die_heredity.hip) ------------------------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 *
 * die_births_record — who was born to whom in the pass that JUST ran on this workspace (die_agent_births with n_slots slots;
 * nothing may have written the workspace since): parent_of[s] = the parent's slot if s was born in the pass, else -1; child_of[s]
 * = the child's slot if s bred in the pass, else -1; both n_slots int32 words.  One launch, a gather (every slot looks itself up
 * in the pass's two ascending lists), launched only for a caller that asks.  Checked before the launch: null pointers, n_slots
 * outside 1..DIE_OWNER_SLOT_MASK, a workspace smaller than die_births_workspace_bytes(1, n_slots) or not 4-byte aligned, outputs
 * that overlap each other or the workspace. */
int die_births_record(int64_t n_slots, const void* workspace, int64_t workspace_bytes, int32_t* parent_of, int32_t* child_of,
                      void* stream);
/* The same for the pass die_agent_births_batch ran: ONE launch for all replicas (the replica in blockIdx.y), replica r's words
 * r * b->agent_stride on; the slots b->n[r] <= s < b->agent_stride are -1 in both arrays.  Checked as the pass checks its batch. */
int die_births_record_batch(const die_batch* b, const void* workspace, int64_t workspace_bytes, int32_t* parent_of, int32_t* child_of,
                            void* stream);

/* die_memory_inherit — what a newborn's memory channels hold (NeuralAutomataAgent(memory_inherit=..., memory_mutation=a)), applied
 * IN PLACE to the (memory_channels, n_slots) fp32 memory by slot id (row m at memory + m * row_stride) after a birth pass and
 * after the step's read-out.  For every slot s with p = parent_of[s] >= 0 and every channel m:
 *   DIE_INHERIT_BLANK                memory[m][s] = +0.0f
 *   DIE_INHERIT_COPY, mutation == 0  memory[m][s] = memory[m][p], moved as a 32-bit word
 *   DIE_INHERIT_COPY, mutation  > 0  memory[m][s] = fadd_rn(memory[m][p], fmul_rn(mutation, u)), u = (float)(int32)word * 2^-31,
 *       word = word (m & 3) of Philox4x32-10(counter = (p, m >> 2, world_step, DIE_STREAM_HEREDITY = 12), key = world_seed) — the
 *       births' key and step on their own stream; two separately rounded fp32 operations.
 * Every other word is left alone (the parent keeps its memory).  One launch; parents and children are disjoint, so no word is
 * read by one thread and written by another.  A record word outside 0..n_slots - 1 reads as -1.  Checked before the launch: null
 * pointers, an unknown mode, memory_channels outside 1..DIE_MEMORY_MAX_CHANNELS, n_slots outside 1..DIE_OWNER_SLOT_MASK - 1,
 * row_stride < n_slots, a mutation that is negative or not finite, a mutation > 0 with DIE_INHERIT_BLANK, a memory that overlaps
 * the record. */
#define DIE_INHERIT_BLANK 0
#define DIE_INHERIT_COPY 1
int die_memory_inherit(int32_t mode, float mutation, int32_t memory_channels, int64_t n_slots, const int32_t* parent_of, float* memory,
                       int64_t row_stride, uint64_t world_seed, uint32_t world_step, void* stream);
/* Every replica in ONE launch: memory the dense (R, memory_channels, b->agent_stride) array, parent_of (R, b->agent_stride) as
 * die_births_record_batch writes it, world_seeds a HOST array of b->replicas keys read during the call (the births' own). */
int die_memory_inherit_batch(int32_t mode, float mutation, int32_t memory_channels, const die_batch* b, const int32_t* parent_of,
                             float* memory, const uint64_t* world_seeds, uint32_t world_step, void* stream);
/* The adjoint, out of place, one launch, plain loads and stores (a parent has at most one child a pass: no atomics).  With the
 * incoming gradient `grad` laid out as the memory, for every slot s and channel m:
 *   child_of[s] >= 0 (a parent)   grad_memory[m][s] = grad[m][s] + grad[m][child_of[s]] (COPY: one fp32 add) or grad[m][s] (BLANK)
 *   parent_of[s] >= 0 (a child)   +0.0f
 *   neither                       grad[m][s], moved as a 32-bit word
 * The mutation has unit Jacobian and does not appear.  Checked as die_memory_inherit, and: null child_of / grad / grad_memory, an
 * output that overlaps the incoming gradient or the record.  The batched twin also passes a replica's padding slots through. */
int die_memory_inherit_backward(int32_t mode, int32_t memory_channels, int64_t n_slots, const int32_t* parent_of, const int32_t* child_of,
                                const float* grad, float* grad_memory, int64_t row_stride, void* stream);
int die_memory_inherit_backward_batch(int32_t mode, int32_t memory_channels, const die_batch* b, const int32_t* parent_of,
                                      const int32_t* child_of, const float* grad, float* grad_memory, void* stream);
/* Decomposed step, second half: claim + feeding of die_agent_move_claim without the move. */
int die_agent_claim_feed(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* gaussian × (1 − decay) on a halo-padded tile: no wrap; exact for cells at least `radius` away
 * from the array border, the outer ring of dst is unspecified. */
int die_diffuse_decay_tile(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype,
                           float sigma, float decay, void* stream);
/* gaussian(sigma, mode='wrap') × (1 − decay): src → dst, W×H planes of `dtype`. */
int die_diffuse_decay(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype,
                      float sigma, float decay, void* stream);
/* … with any of scipy's boundary modes (LDS-tiled kernel; 'wrap' with H % 4 == 0 and radius <= 4 takes the row sweep) */
int die_diffuse_decay_mode(const void* src, void* dst, int32_t W, int32_t H, int32_t dtype, float sigma, float decay,
                           int32_t mode, void* stream);

/* ---- DataInitializer (core/data_init.py:92-253, core/env.py:74-86) ------------------- */
typedef struct die_food_spec {
    int32_t n_waves;             /* sinusoid mix (<= 8 waves), used when perlin_octaves == 0 */
    float scale;
    int32_t perlin_octaves;      /* > 0: with_food_perlin (:228-231): 2-D gradient noise of that many lattice cells per unit */
    float threshold;             /*      length, .round(3), values outside [0, threshold] masked to 0 (Env: 8, 1.0) */
    double fx[8], fy[8], phase[8], amp[8];
} die_food_spec;

/* with_agents(ratio) + with_food(...) + zero chem: fills owner (epoch 1), food, chem. */
int die_init_medium(const die_medium* m, double agent_ratio, uint64_t seed, const die_food_spec* food,
                    void* stream);
/* agents_from_medium (:133-150): occupied cells in row-major order → slots [0, K); slots
 * >= K are zeroed.  K is written to *num_alive_dev (device int64).  Fails at run time
 * (K clipped, flag in num_alive_dev[1]) when K > a->N. */
int die_init_agents(const die_medium* m, const die_agents* a, uint64_t seed, int64_t* num_alive_dev,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* The worlds of every replica of a die_batch at once (BatchedEnv.reset(seed=...)): replica r ends exactly as
 * die_init_medium(m_r, agent_ratio, seed + r * world_stride, food) followed by die_init_agents(m_r, a_r of b->n[r] slots, same
 * seed) would leave it — owner at epoch 1, food, the current chem plane (m->chem), x / y / alive / agent_food with the tail
 * zeroed.  `m` and `a` describe replica 0 (a whole world: gW <= 0); replica r starts b->plane_stride / b->agent_stride
 * elements further.  counts_dev[2r] receives min(K_r, n[r]) (the slots filled); counts_dev[2r + 1] gets 1 OR-ed in when K_r >
 * n[r] (the agents are then clipped as die_init_agents clips them) and is never cleared here.  Five launches whatever the
 * number of replicas, no allocation, no synchronisation (capturable).  A wave-mix spec (perlin_octaves == 0) is drawn from
 * one seed on the host, so it is refused with world_stride != 0.  The workspace must hold
 * die_init_batch_workspace_bytes(W, H, replicas) bytes (-1: bad sizes). */
int64_t die_init_batch_workspace_bytes(int32_t W, int32_t H, int32_t replicas);
int die_init_batch(const die_medium* m, const die_agents* a, const die_batch* b, double agent_ratio, uint64_t seed,
                   uint64_t world_stride, const die_food_spec* food, int64_t* counts_dev, void* workspace, int64_t workspace_bytes,
                   void* stream);
/* The same call with the world of every replica given: replica r is seeded from seeds[r] (BatchedEnv.reset(seeds=...); the E
 * worlds of every candidate of a population with episodes).  `seeds` is a HOST array of n_seeds values, read during the call
 * and passed to the kernels by value; n_seeds must be b->replicas (1..DIE_MAX_REPLICAS).  Any values, repeats included, no
 * arithmetic pattern.  Otherwise die_init_batch's contract: same five launches, same counts_dev words, same workspace; a
 * wave-mix spec is refused unless every seed is the same. */
int die_init_batch_seeds(const die_medium* m, const die_agents* a, const die_batch* b, double agent_ratio, const uint64_t* seeds,
                         int32_t n_seeds, const die_food_spec* food, int64_t* counts_dev, void* workspace, int64_t workspace_bytes,
                         void* stream);
/* GradientAgent/PhysarumAgent.__init__ state (:42-43,163): heading from N(0,.4) noise,
 * discretised to the turn lattice when turn_radians > 0; stored as the float64 of its fp32 rounding. */
int die_init_heading(uint32_t* heading_hi, uint32_t* heading_lo, float* prev_gx, float* prev_gy, int64_t N, double turn_radians,
                     uint64_t seed, void* stream);

/* DataInitializer's builder steps (core/data_init.py:171-253) on plain fp32 device arrays: one channel per call.
 *   DIE_FIELD_CONST   with_const (:214-216): dst = a
 *   DIE_FIELD_NOISE   with_noise / get_random (:168-169,218-220): (b - a) * random_sample().round(3) + a, the uniform being
 *                     word `word` (0..3) of Philox(seed, step, element)
 *   DIE_FIELD_AGENTS  with_agents (:222-226): ceil(_mask(random_sample().round(3), mask_above = b)), the random stream of
 *                     die_init_medium at the same `step` (0 there)
 *   DIE_FIELD_PERLIN  with_food_perlin / with_chem (:228-236): _mask(perlin.round(3), mask_above = b) on the W x H labels,
 *                     octaves = a (see die_food_spec), lattice seed `seed + step` */
typedef enum die_field_op { DIE_FIELD_CONST = 0, DIE_FIELD_NOISE = 1, DIE_FIELD_AGENTS = 2, DIE_FIELD_PERLIN = 3 } die_field_op;
int die_field_fill(float* dst, int64_t n, int32_t op, int32_t W, int32_t H, double a, double b, uint64_t seed, uint32_t step,
                   uint32_t word, void* stream);
/* build (:238-246): channels x mask -> the medium (occupied cells flagged for die_init_agents; chem / food converted to
 * the field dtype).  A NULL channel is zeros, a NULL mask is the scalar. */
int die_medium_from_fields(const die_medium* m, const float* agents, const float* food, const float* chem, const float* mask,
                           float mask_scalar, void* stream);

/* Env._medium_resource_dynamics (core/env.py:147-150) with the flow operator of WaveSequence.get_flow_operator
 * (core/data_init.py:29-38): food <- scale * z(x, y, t) + (1 - decay) * food, z = WaveSequence.__getitem__(t)
 * (core/data_init.py:71-89) evaluated at the world cell of every local element; float64 arithmetic. */
int die_food_flow_wave(const die_medium* medium, double t, double scale, double decay, void* stream);
/* The same with PerlinNoiseSequence.__getitem__(t) (core/data_init.py:55-69) as the field: round(noise((x, y, t)), 3), `noise` =
 * 3-D gradient noise at (x, y, t) * octaves on the linspace(0, 1, n) labels, lattice gradients from Philox(seed, point). */
int die_food_flow_perlin(const die_medium* medium, double t, int32_t octaves, double scale, double decay, uint64_t seed, void* stream);
/* One of the two flows above on every replica of a die_batch, in one launch: `m` describes replica 0 (a whole world: gW <= 0,
 * at least 2x2, H % 4 == 0), replica r's food plane starts r * b->plane_stride elements further.  Every replica sees the
 * same field (same t; for Perlin the same octaves and seed), evaluated once per cell, so replica r ends exactly as
 * die_food_flow_wave / die_food_flow_perlin on its plane alone would leave it.  `octaves` is read for DIE_FLOW_PERLIN only. */
#define DIE_FLOW_WAVE   1
#define DIE_FLOW_PERLIN 2
int die_food_flow_batch(const die_medium* m, const die_batch* b, int32_t kind, double t, double scale, double decay,
                        int32_t octaves, uint64_t seed, void* stream);

/* Env._get_sense_mask (core/env.py:276-290): mask = ceil(round(gaussian(agents channel, sigma, mode 'nearest',
 * truncate 4), decimals)) as W*H bytes (the reference uses sigma 2.0, 3 decimals); float64 accumulation, axis 0
 * then axis 1 as scipy does.  tmp: W*H doubles of device scratch.  Periodic single-tile planes only. */
int die_sense_mask(const die_medium* medium, float sigma, int32_t decimals, uint8_t* mask_out, double* tmp, void* stream);

/* EnvRenderer.render (core/render.py:76-110) on the device, one sweep: rgb_out (W, H, 3) float32 = (agents,
 * env_food, chem1); trace <- trace * trace_decay + agents (FieldTrace.update, :29-30) and rgba_out (W, H, 4) =
 * lut[index(trace)] with matplotlib's Colormap.__call__ index rule, lut = (lut_n + 3, 4) float32 (colours, under,
 * over, bad); rgb8_out (W, H, 3) uint8 = clip(rgb, 0, 1) * 255.  Any output may be NULL (trace may be NULL when
 * rgba_out is). */
int die_render_frames(const die_medium* medium, float* trace, float trace_decay, const float* lut, int32_t lut_n,
                      float* rgb_out, float* rgba_out, uint8_t* rgb8_out, void* stream);

/* ---- spatial re-ordering of the agent arrays (no reference counterpart; see die_sort.hip) ----
 * Writes `in` permuted into `out` (different arrays, out->slot required) so that array
 * neighbours are grid neighbours: counting sort by the (ix/16, iy/32) bucket of each agent's cell
 * (the order inside a bucket is free).  DIE_ERR_ARG for m->W or m->H < 1, like die_sort_workspace_bytes' -1.
 * Up to 4 further per-slot float arrays (agent-object state such as headings) are permuted
 * alongside.  Results of forward/step are independent of the order. */
int64_t die_sort_workspace_bytes(int32_t W, int32_t H, int64_t N);
int die_agents_sort(const die_medium* m, const die_agents* in, const die_agents* out, int32_t n_extra,
                    const float* const* extra_in, float* const* extra_out, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- tile-binned step (die_pic.hip; no reference counterpart for the data structure) --------------------------------
 * The fast path of `env.step(agent.forward(obs))` (examples/minimal_run.py:24-25) for worlds in which every slot is alive
 * and an agent moves less than a tile per step: the agent arrays are kept in EXACT tile order (tiles of 2^tile_xs ×
 * 2^tile_ys cells; 64×64, 32×128, 32×64 and 16×32 are compiled in), "last writer wins" of core/env.py:211 is resolved in LDS
 * and the field sweep reads a 4-byte deposit plane — no claim plane, no global atomics on cells.  Same bits as
 * die_forward_env_step.  A layout = the per-agent arrays plus per-tile words: segment offset / size, number of stayers
 * (agents of the segment that stand on the tile; the rest have walked onto a neighbouring tile), arrivals.  The step reads
 * layout[from] and writes layout[1 - from]; the caller alternates.  The 'agents' channel (m->owner) is NOT maintained by this
 * path: die_agents_mark_owner rebuilds it on demand. */
typedef struct die_pic_layout {
    uint32_t* x;             /* N, Q0.32 */
    uint32_t* y;
    float* agent_food;       /* N */
    uint32_t* slot;          /* N, reference slot ids (always materialised) */
    uint32_t* heading_hi;    /* N, the agent object's _direction_rads (float64 halves, die_gradient_agent) in this order */
    uint32_t* heading_lo;
    uint32_t *off, *n, *s, *inc;   /* die_pic_tiles() words each */
} die_pic_layout;

typedef struct die_pic {
    int32_t tile_xs, tile_ys;    /* log2 of the tile shape */
    int64_t N;                   /* agents = slots, all alive */
    die_pic_layout layout[2];
    float* dep;                  /* N floats of scratch */
    float* dep_plane;            /* three-launch form only (may be NULL when rim is given and the step qualifies), W*H: per cell the deposit of the highest slot standing
                                    on it, or 0xFFFFFFFF */
    void* part_gain;             /* 2 * die_pic_tiles() 64-bit words: reward partials per tile, then (tiles of a decomposed world:
                                    die_medium.gW > 0) the owned agents per tile; also the binning scratch */
    uint32_t* error;             /* device word, 0 = fine; sticky bits after a step: 1 segment bookkeeping broken, 2 an agent moved
                                    further than a tile.  Never cleared by the library */
    int32_t k1_threads;          /* tuning: workgroup size of the agent kernel (multiple of 64, <= 512); 0 = default */
    int32_t stages;              /* 0 = the whole step; else a bit mask of the launches to run (per-kernel timing: bench.py):
                                    1 agent kernel (ONE issue per step: it adds to layout[1 - from].inc), 2 claim resolution +
                                    next offsets, 4 field sweep (two-launch form: the sweep is part of the kernel of bit 2) */
    /* two-launch form (rim != NULL): the agent kernel also lists, per tile, the agents of the tile's new segment that matter
     * to ANOTHER tile's field — those that walked off the tile and those that stand within the gaussian radius of a border —
     * and ONE kernel per tile reads the lists of the 9 tiles around it (fixed places: requested with the first loads),
     * resolves the claims of its tile + rim in LDS, adds the winners' deposits, diffuses, decays and feeds: no deposit
     * plane, one launch less.  A list that overflows costs time (that tile's segment is then scanned), never correctness. */
    void* rim;                   /* die_pic_tiles() * die_pic_rim_cap() records of 16 bytes (x, y, slot, deposit bits), or NULL: three
                                    launches (claim resolution writes dep_plane, die_env.hip's sweep reads it) */
    uint8_t* rim_code;           /* die_pic_tiles() * die_pic_rim_cap() bytes: where each listed agent stands (see die_pic.hip) */
    uint32_t* rim_cnt;           /* die_pic_tiles() words */
    int64_t* status_out;         /* two-launch form, may be NULL: the step copies *error here next to writing `result` — a caller that
                                    places it behind its die_step_result reads reward, num_alive and the error word in ONE copy (both
                                    may be device-visible pinned host memory: one thread writes the three words with system-scope atomic stores, so their visibility does not wait for the kernel's end) */
    /* PhysarumAgent's random turn (core/agent/gradient.py:183) on this path: one bit per slot id from a table the library
     * fills, one Philox block per 128 slots (same bits as the stand-alone forward evaluates per agent: csrc/die_rng.h
     * die_turn_word).  The field kernel of a step fills it for (g->seed, g->step + 1); a caller that steps with the same
     * seed and consecutive g->step sets turn_ready = 1 from the second step on, else the step fills the table first. */
    uint32_t* turn_bits;         /* 4 * ceil(turn_slots / 128) words */
    int64_t turn_slots;          /* slot ids are < turn_slots (>= N; a decomposed world: the world's slot count) */
    int32_t turn_ready;          /* the table already holds the bits of (g->seed, g->step) */
    /* ORDER TABLE of the two-launch form's workgroups (ABI 23; may be NULL: workgroup id -> tile by XCD bands of columns, as before).
     * order[j * (tiles / 8) + k] = the tile the k-th workgroup of XCD j takes (linear workgroup id = 8 k + j): a permutation of band j's
     * tiles, written by the library (k_pic_order: crowded tiles first, band order among equals) from the populations of the layout a
     * step reads — when order_ready == 0 and every 32nd step (g->step % 32 == 0).  Only WHICH workgroup takes a tile changes, never a
     * result.  Late in a run, when the agents have aggregated (tiles of 3 000 agents beside tiles of 100), the crowded tiles — and the
     * tiles whose rim lists overflow — no longer make up a launch's tail: 166 -> 144 us per step at world step 3 000 of the benchmark
     * world (round 6).  Used when tiles-per-row % 8 == 0, tiles <= 65 536, an undivided world, all tiles in one launch; ignored otherwise.
     * The caller allocates die_pic_tiles() 16-bit words (4-byte aligned) and sets order_ready = 1 once a step has run with them (the
     * table stays a valid permutation across re-binning: it is only stale then).
     *   Below the crowd threshold the table keeps band order except for every band's share of the launch's last, partial round of agent-kernel
     * workgroups: those last places take the band's LIGHTEST tiles, in band order among themselves (the tail form; see k_pic_order).  The
     * round is measured in `slots`, the workgroups the device holds at once (CUs x resident workgroups of the agent kernel launched), which
     * the library asks of the runtime; no tail is shaped when tiles % slots is 0 or above 7/8 of slots.
     *   order_ready is a word of flags — 0 and 1 mean what they meant before: DIE_PIC_ORDER_READY as above; DIE_PIC_ORDER_NO_TAIL keeps band
     * order below the crowd threshold; a value s > 0 in the bits from DIE_PIC_ORDER_SLOTS_SHIFT up takes the place of the runtime's `slots`
     * (tests: a partial last round on a small world). */
#define DIE_PIC_ORDER_READY 1
#define DIE_PIC_ORDER_NO_TAIL 2
#define DIE_PIC_ORDER_SLOTS_SHIFT 8
    int32_t order_ready;
    uint16_t* order;
    /* ONE launch (stages = 1 or 2) over a subset of the tiles: sub_mode 0 all tiles; 1 only the rectangle [sub_tx0, sub_tx0 +
     * sub_ntx) x [sub_ty0, sub_ty0 + sub_nty) of tiles; 2 all tiles but that rectangle — and, for stages = 2, the workgroups that
     * complete a step (next offsets, reward, turn bits).  A decomposed rank steps the tiles that need nothing from its neighbours
     * while its ghost refresh's messages are in flight, the others once they have arrived (die_amd/dist.py).  The caller issues
     * every tile exactly once per stage; two-launch form only. */
    int32_t sub_mode, sub_tx0, sub_ty0, sub_ntx, sub_nty;
    int32_t halo_fresh;          /* decomposed tiles, the step behind die_pic_ghost_inplace: the agent kernel takes no arrivals on tiles
                                    outside the owned cells (die_medium.own_*) */
    /* The reference's default slot layout on this path (core/data_init.py:143-144: max_agents = W*H slots, most of which never
     * lived): the tiles' segments hold the n_alive alive agents, entries [0, n_alive) of the arrays, the dead slots lie behind them,
     * entries [n_alive, N), where die_pic_bin puts them.  A dead slot acts, moves, burns and "consumes" like the reference's
     * (core/env.py:163-172, 224-243) — from the occupancy map `occ` (one BYTE per cell: the cells alive agents stand on in this
     * step; scratch, W*H bytes) — and never claims, deposits or marks a cell.  0 (or N): every slot is alive.
     * Two-launch form, single-tile worlds. */
    int64_t n_alive;
    void* occ;
    /* GradientAgent with momentum on this path (core/agent/gradient.py:82-91: inertia and / or noise; normalised gradient).
     * prev_grad[l][0 / 1]: _prev_grad's x / y component in the order of layout[l] (N floats each) — the step reads layout[from]'s
     * and writes layout[1 - from]'s, die_pic_bin carries them from g's arrays into layout[into]'s; all NULL when inertia = 0
     * (noise alone keeps no state).  The step length the tiles must hold is |scale| * die_pic_step_bound(inertia, noise_scale). */
    float* prev_grad[2][2];
} die_pic;

/* entries per tile of die_pic.rim for a tile shape, or -1 if the shape is not compiled in */
int64_t die_pic_rim_cap(int32_t tile_xs, int32_t tile_ys);
/* 1 if die_pic_forward_env_step takes the two-launch form for these parameters when rim lists are given (world_max = the longer
 * axis of the WORLD in cells), 0 if it takes three launches (then dep_plane must exist and status_out is not written), -1 for a
 * tile shape that is not compiled in.  The library's own rule: callers need not restate it. */
/* Largest |component| of the vector a GradientAgent's action is `scale` times, per axis, for a normalised gradient: 1 without
 * momentum; with it the fixed point of |u'| <= (1 - inertia) + inertia |u| + noise_scale * 2.67 (2.67 = the largest value of the
 * library's 0.4-sigma Box-Muller normals, which also bounds the initial _prev_grad), i.e.
 * max(2.67, 1 + 2.67 noise_scale / (1 - inertia)); inertia = 0: 1 + 2.67 noise_scale.  +inf for inertia >= 1.  Callers pass
 * scale * bound where the rules below ask for `scale`. */
float die_pic_step_bound(float inertia, float noise_scale);
int32_t die_pic_two_launch(int32_t world_max, int32_t tile_xs, int32_t tile_ys, float scale, float diffuse_sigma, int32_t diffuse_mode);
/* number of tiles (words per per-tile array), or -1 if the shape is not compiled in */
int64_t die_pic_tiles(int32_t W, int32_t H, int32_t tile_xs, int32_t tile_ys);
/* Bin agents held in any order (die_agents; `heading` in the same order) into layout[into]; both layouts' per-tile words
 * are initialised.  DIE_ERR_UNSUPPORTED unless the world splits into at least 3×3 whole tiles. */
int die_pic_bin(const die_medium* m, const die_agents* a, const uint32_t* heading_hi, const uint32_t* heading_lo, const die_pic* p,
                int32_t into, void* stream);
/* … and a GradientAgent's _prev_grad (core/agent/gradient.py:42,89), same order, into p->prev_grad[into] (both NULL: die_pic_bin) */
int die_pic_bin_momentum(const die_medium* m, const die_agents* a, const uint32_t* heading_hi, const uint32_t* heading_lo,
                         const float* prev_gx, const float* prev_gy, const die_pic* p, int32_t into, void* stream);
/* GradientAgent/PhysarumAgent.forward (core/agent/gradient.py:96-124) + Env.step (core/env.py:101-131) on binned agents:
 * two launches when p->rim is given and floor(|scale| * (max(W, H) - 1)) + 2 + gaussian radius <= tile (forward + move + feeding +
 * re-binning + rim lists; per-tile claim resolution + deposit + diffusion + feeding + next offsets + reward), else three
 * (forward + move + feeding + re-binning; LDS claim resolution + next offsets; field sweep + reward).  Same bits.  The
 * agent state (g->heading_* are ignored: layout[from].heading_*) moves with the agents; `act` receives the action in the order
 * of layout[from].  Requires: every slot alive, no agents_die / sense mask, normalised gradient without inertia or noise
 * and |scale| * (max(W, H) - 1) <= tile - 1 (else DIE_ERR_UNSUPPORTED / DIE_ERR_ARG: use die_forward_env_step).
 * The planes may be a tile of a decomposed world (die_medium.gW > 0; two-launch form only): agents are binned by the plane
 * cell that holds their world cell (nearest edge for agents beyond the planes), the planes are treated as periodic — what
 * that brings in across their outer edge stays in the outermost cells of the halo, which a ghost-agent decomposition
 * discards —, probes clamp at the WORLD's edge, and reward / num_alive count the agents on cells the rank owns (own_*).  Per axis
 * the planes must either span the world or leave 2 * (probe margin) + 2 cells of it uncovered (the taps around an agent are
 * mapped from one mapping of its own cell; else DIE_ERR_UNSUPPORTED). */
int die_pic_forward_env_step(const die_medium* m, const die_pic* p, int32_t from, die_gradient_agent* g, const die_action* act,
                             const die_dynamics* d, die_step_result* result, void* stream);
/* n_steps x die_pic_forward_env_step(act = NULL) without the host in between — `for i in range(n): obs, ... = env.step(agent.forward(obs))`
 * (examples/minimal_run.py:23-25) for a caller that reads nothing back on the way: step i reads layout[(from + i) & 1] and writes the
 * other one, reads the chem plane step i - 1 wrote (m->chem and m->chem_next exchange roles every step: after an odd n_steps the
 * current plane is m->chem_next), draws from (g->seed, g->step + i), and leaves its result in results[i].  p->stages = 0, no
 * subset of the tiles; p->turn_ready as for the first step.  Same launches, same bits as n_steps separate calls. */
int die_pic_run(const die_medium* m, const die_pic* p, int32_t from, const die_gradient_agent* g, const die_dynamics* d,
                int32_t n_steps, die_step_result* results, void* stream);
/* Steps the calling thread's last die_pic_run had enqueued when it returned: n_steps on success; on an error the number of
 * whole steps already in the stream (arguments are checked by every step, so a failure behind the first one means a failed
 * launch) — the caller adopts the state those steps reach (layout (from + done) & 1, the chem plane roles exchanged `done`
 * times, step counter + done) before it reports the error.  ABI 22. */
int32_t die_pic_run_completed(void);
/* The agent kernel of die_pic_forward_env_step has SPECIALISED instantiations — tile shape, margins, workgroup size, boundary, cost
 * operator and rim as compile-time constants: fp32 planes with 64x64 tiles and fp16 planes with 32x128 tiles, a PhysarumAgent probing
 * up to 10 cells ahead and walking less than 2 cells per step, 512 threads, periodic boundary, linear cost, gaussian radius 2, the
 * staged two-launch form over all tiles of an undivided world — which a call that matches one of them takes; every other call takes the
 * generic instantiation.  Same bits either way.  die_pic_k1_generic(1) makes every call of this process take the generic one (A/B
 * measurements, tests), (0) lifts that, (-1) goes by the environment: DIE_PIC_K1_GENERIC=1, read once at the next step.
 * die_pic_k1_specialised_launches(): launches of a specialised instantiation by this process so far.
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24. */
void die_pic_k1_generic(int32_t force);
int64_t die_pic_k1_specialised_launches(void);
/* Self-check of the wave reduction the agent kernel's epilogue uses (die_wave_sum_i64_dpp: a 64-bit integer sum over a whole wave by
 * data-parallel-primitive moves, no LDS): in = n_waves x 64 int64 on the device, out[w] = the sum of in[64 w .. 64 w + 63] modulo 2^64.
 * 1 <= n_waves <= 2^20.  Added within ABI 24 like the two above: a new symbol only. */
int die_wave_sum_i64_check(const void* in, int64_t n_waves, void* out, void* stream);
/* `act` of die_pic_forward_env_step may be NULL: the action then stays in registers.  For a normalised PhysarumAgent it can
 * still be produced afterwards — until the next step overwrites p->dep — from what the step left in layout[lay] (the layout it
 * WROTE): (dx, dy) = scale * polar2xy(1, heading'), deposit = p->dep; same bits as the action the step would have stored, in
 * the order of layout[lay] (core/agent/gradient.py:110-124: the action PhysarumAgent.forward returns). */
int die_pic_action_physarum(const die_pic* p, int32_t lay, const die_gradient_agent* g, const die_action* act, void* stream);

/* ---- Ghost refresh by tiles (die_amd/dist.py DistEnv._refresh_ghosts_tiles; no reference counterpart) ----
 * For a rank of a ghost-agent decomposition whose agents are held in a tile-binned layout (layout[from], as a step or
 * die_pic_bin left it) over planes whose halo is whole tiles deep (die_medium.own_* on tile borders).  An agent is owned iff it
 * stands on an interior tile, so a refresh never looks at every agent:
 *   die_pic_ghost_pack   for every side, tile by tile of its band (tile rectangle [tx0, tx0+ntx) x [ty0, ty0+nty) of the
 *                        interior, row-major): the agents standing on the tile — its stayers and the neighbouring tiles'
 *                        leavers that landed on it — go to send_rec (six streams of `cap` words each: x | y | agent_food |
 *                        slot | heading_hi | heading_lo, the tiles' agents one tile after the other), their number to
 *                        send_counts[tile];
 *   (the caller exchanges the messages: what a neighbour packed for its side -d arrives as recv_* of side d)
 *   die_pic_ghost_merge  layout[1 - from] := tile by tile, the agents standing on an interior tile / the agents that arrived
 *                        for a halo tile (rectangle [hx0, hx0+ntx) x [hy0, hy0+nty), same shape as the band); every agent a
 *                        stayer, both layouts' per-tile words equal — the state die_pic_bin leaves.  Halo tiles no side
 *                        fills become empty.  At most `capacity` array entries are written.
 * summary (device, DIE_PIC_GHOST_SUMMARY_WORDS int64; cleared by die_pic_ghost_pack): [0] agents after the refresh, [1] of
 * them owned, [2 + k] agents sent to side k, [10 + k] agents arrived from side k, [18] flags (DIE_PIC_GHOST_*): the caller
 * reads it once, after die_pic_ghost_merge, and must not use the new layout if a flag is set. */
#define DIE_PIC_GHOST_SUMMARY_WORDS 19
#define DIE_PIC_GHOST_BAD_COUNT 1      /* a tile holds another number of agents than its per-tile words say */
#define DIE_PIC_GHOST_SEND_CAP 2       /* a band holds more agents than `cap` */
#define DIE_PIC_GHOST_BAD_RECV 4       /* a received count is impossible */
#define DIE_PIC_GHOST_CAPACITY 8       /* the agents do not fit `capacity` */
typedef struct die_pic_side {
    int32_t tx0, ty0, ntx, nty;        /* band (tiles of the planes) */
    int32_t hx0, hy0;                  /* halo block filled by the message arriving from this side's neighbour */
    int64_t cap;                       /* agents a message holds */
    uint32_t* send_counts;             /* ntx * nty */
    uint32_t* send_rec;                /* 6 * cap */
    const uint32_t* recv_counts;
    const uint32_t* recv_rec;
} die_pic_side;
int die_pic_ghost_pack(const die_medium* m, const die_pic* p, int32_t from, int32_t n_sides, const die_pic_side* sides,
                       int64_t* summary, void* stream);
int die_pic_ghost_merge(const die_medium* m, const die_pic* p, int32_t from, int32_t n_sides, const die_pic_side* sides,
                        int64_t capacity, int64_t* summary, void* stream);
/* The same in two halves, for a refresh whose messages travel while the next step runs on the tiles that need nothing from a
 * neighbour: phase 1 = the interior tiles' segments (they come first in the new layout: their offsets depend on nothing that
 * arrives; summary[1] = their total), phase 2 = the halo tiles' segments behind them, from the received counts; phase 0 = both
 * (die_pic_ghost_merge).  Phase 1 before phase 2, die_pic_ghost_pack before both. */
int die_pic_ghost_merge_phase(const die_medium* m, const die_pic* p, int32_t from, int32_t n_sides, const die_pic_side* sides,
                              int64_t capacity, int64_t* summary, int32_t phase, void* stream);
/* The refresh IN PLACE, for a step that follows at once and reads layout[from] (not layout[1 - from], as after die_pic_ghost_merge):
 * the interior tiles' segments stay where the step before left them — stayers, then leavers, as the agent kernel reads them
 * anyway — and nothing of them is copied.  phase 1: the places of the interior tiles' segments in the layout the coming step WRITES
 * (layout[1 - from].off / .n; summary[1]); phase 2, once the messages are here: the halo tiles' places behind them (summary[0],
 * arrived counts), and in layout[from] every halo tile gets a NEW segment behind everything the arrays hold — what arrived for it as
 * stayers, then those of its old leavers that stand on an interior tile (a ghost that walked into the interior is owned now) — and
 * its three words.  The coming step must run its agent kernel on the halo tiles with die_pic.halo_fresh = 1 (they take no arrivals:
 * an interior tile's leaver that stands on a halo tile is the stale copy of an agent that arrived with the message).  Entries beyond
 * the old end of the arrays are used: at most die_pic_tiles() words of `tail` scratch, `capacity` array entries. */
int die_pic_ghost_inplace(const die_medium* m, const die_pic* p, int32_t from, int32_t n_sides, const die_pic_side* sides,
                          int64_t capacity, int64_t* summary, int32_t phase, uint32_t* tail, void* stream);
/* Rebuild the 'agents' channel from the agent arrays: atomicMax of (m->epoch, slot) claims (deposit bits 0) for every
 * alive agent.  The caller advances m->epoch (or zeroes the plane) first. */
int die_agents_mark_owner(const die_medium* m, const die_agents* a, void* stream);

/* ---- NeuralAutomataAgent sensing (core/agent/evo.py:45-118,150-174; die_nca.hip) -----------------------------------
 * One layer of ConvolutionModel: a bias-free Conv2d with 'same' circular padding over (channel, x, y) planes,
 *   out[o, x, y] = sum_i sum_a sum_b w[o, i, a, b] * in[i, (x + a - r) mod W, (y + b - r) mod H],  r = k / 2,
 * k odd (1, 3, 5, 7), at most 4 channels in and out, weights (cout, cin, k, k) fp32 in device memory; the last layer of the
 * stack applies tanh (:97-99).  Input planes may be the medium's own: fp32 / fp16 fields, or the 'agents' channel read
 * from the claim plane (occupied cells are 1.0; `epoch` = die_medium.epoch).  Outputs are fp32 planes, never an input. */
/* DIE_PLANE_STOCK (die_stock.hip, below): a uint64 plane of die_stock_plane, read as
 * occupied at `epoch` ? the payload (the standing agent's agent_food) : 0.  The FORWARD layer calls take it (die_conv2d,
 * die_conv2d_circular, die_conv2d_dropout, die_conv2d_wide) as their LAST input plane, in[cin - 1] — the stock channel is the
 * observation's last (one stock plane a layer) —; at any other position kind 3 is refused as a plane of no kind, as it always
 * was, and the adjoint calls refuse it everywhere. */
typedef enum die_plane_kind { DIE_PLANE_F32 = 0, DIE_PLANE_F16 = 1, DIE_PLANE_AGENTS = 2, DIE_PLANE_STOCK = 3 } die_plane_kind;
typedef struct die_conv_plane {
    const void* data;
    int32_t kind;            /* die_plane_kind */
    int32_t reserved;
} die_conv_plane;
int die_conv2d_circular(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                        float* const* out, int32_t k, const float* weights, int32_t apply_tanh, void* stream);
/* The same layer with any `boundary` of ConvolutionModel (core/agent/evo.py:51,86 → torch.nn.Conv2d padding_mode). */
typedef enum die_pad_mode { DIE_PAD_CIRCULAR = 0, DIE_PAD_ZEROS = 1, DIE_PAD_REFLECT = 2, DIE_PAD_REPLICATE = 3 } die_pad_mode;
int die_conv2d(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
               float* const* out, int32_t k, const float* weights, int32_t apply_tanh, int32_t padding_mode, void* stream);
/* NeuralAutomataAgent.forward's per-agent read-out (core/agent/evo.py:161-170, core/utils.py:56-65): for EVERY slot
 * action[c, n] = planes[c][cell(x_n), cell(y_n)] * coefs[c], c = dx, dy, deposit1. */
int die_gather_scale(const die_medium* m, const die_agents* a, const float* const* planes, const float* coefs,
                     const die_action* out, void* stream);

/* ---- A population of NeuralAutomataAgents on batched replicas (die_amd/batch.py BatchedNeuralAutomataAgent) ----------
 * Replica r of a die_batch (same layout, same restrictions as die_forward_env_step_batch) is stepped by candidate r's
 * ConvolutionModel: one launch per layer (k_conv_circular with the replica in blockIdx.z: same tile, same summation order,
 * same tanh as die_conv2d), then one launch that reads every agent's action out of its replica's last planes
 * (die_gather_scale's product) and moves / claims / feeds it, then die_forward_env_step_batch's field sweep.  Replica r
 * computes exactly what die_conv2d per layer + die_gather_scale + die_env_step compute for that world alone.
 *   Epochs: the first layer reads the claim plane at `sense_epoch` (the epoch before this step's), the claims are made at
 * m->epoch, which must be sense_epoch + 1, or 1 after DIE_OWNER_EPOCH_MAX — then the claim planes of every replica are
 * cleared between the sensing and the claims (what Env.step's next_epoch does).
 *   Scratch: [set][replica][4][W][H] fp32 planes, set = layer % 2 (one set for a one-layer stack); the last layer's
 * (dx, dy, deposit) planes of replica r stay in set (n_layers − 1) % 2 until the next call.  `act` may be NULL. */
#define DIE_NCA_MAX_LAYERS 8
typedef struct die_nca_layer {
    int32_t k;                   /* odd, 1..7 */
    int32_t cin, cout;           /* 1..4; layer 0 reads 2 + with_agent_channel planes (one more in the *_stock calls), the last gives 3 */
    int32_t reserved;
    const float* weights;        /* device fp32: replica r's (cout, cin, k, k) block starts at weights + r * weight_stride
                                  * (with die_nca_batch.episodes = E > 1: at weights + (r / E) * weight_stride) */
    int64_t weight_stride;       /* elements, >= cout * cin * k * k (e.g. the row length of an (R, P) parameter matrix) */
} die_nca_layer;
typedef struct die_nca_batch {
    int32_t n_layers;            /* 1..DIE_NCA_MAX_LAYERS */
    int32_t padding_mode;        /* die_pad_mode of every layer */
    int32_t with_agent_channel;  /* 1: layer 0 reads (agents, food, chem); 0: (food, chem) */
    int32_t sense_epoch;
    const die_nca_layer* layers;
    float coef[3];               /* action = plane * coef: scale, scale, deposit */
    int32_t episodes;            /* E: replica r = c * E + e is candidate c on its e-th world and reads weight block r / E of every
                                  * layer (weights + (r / E) * weight_stride); must divide b->replicas.  0 (the former
                                  * `reserved`) reads as 1: a block per replica */
    float* scratch;
    int64_t scratch_bytes;
} die_nca_batch;
int64_t die_nca_batch_scratch_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers);
int die_nca_env_step_batch(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                           const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ---- Seeded agent dropout (core/agent/evo.py:98-118: ConvolutionModel's inverted-dropout mask over cells; die_nca.hip) -------
 * New entry points only: no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The reference draws its mask from torch's unseeded generator; here it is a pure function of (key, forward call, cell).  For
 * key s, forward-call counter t and cell c = ix * H + iy of a (W, H) plane:
 *   word(c) = word (c & 3) of Philox4x32-10(counter = (lo32(c >> 2), hi32(c >> 2), t, DIE_STREAM_DROPOUT = 10), key = s): one block
 *   per four consecutive cells; the cell is dropped iff (uint64)word(c) < thr, thr = (uint64)ceil(p * 2^32) in float64; a kept
 *   cell is multiplied by keep = (float)(1 / (1 - p)).  p = 1 drops every cell (thr = 2^32).  One mask per plane, shared by the
 *   layer's output channels: out = tanh(acc) * (0 or keep), one fp32 multiply — the reference's `sense_transform *= dropout_mask`.
 * 0 < p <= 1; any other p (NaN included) is DIE_ERR_ARG, and `reserved` must be 0.  Replica r of a batch is masked with key
 * seed + r * seed_stride (mod 2^64): stride 0 gives every replica the same mask.  Nothing is stored for the mask: the last
 * layer's launch evaluates it in its epilogue (one Philox block per thread where H % 4 == 0), so the planes the layer writes —
 * what die_gather_scale, the batched read-out and render() read — hold the masked values.  All arguments are checked before
 * anything is launched. */
typedef struct die_nca_dropout {
    double p;
    uint64_t seed;
    uint64_t seed_stride;
    uint32_t step;               /* t: the forward-call counter */
    uint32_t reserved;
} die_nca_dropout;
/* die_conv2d with the mask of (drop->seed, drop->step) on its outputs (seed_stride unused); drop NULL: die_conv2d itself. */
int die_conv2d_dropout(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                       float* const* out, int32_t k, const float* weights, int32_t apply_tanh, int32_t padding_mode,
                       const die_nca_dropout* drop, void* stream);
/* die_nca_env_step_batch whose last layer is masked, replica r with key drop->seed + r * drop->seed_stride; everything else in
 * the step is die_nca_env_step_batch's.  drop NULL: die_nca_env_step_batch itself. */
int die_nca_env_step_batch_dropout(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                   const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                   int64_t workspace_bytes, const die_nca_dropout* drop, void* stream);
/* The mask planes themselves: out[r * plane_stride + c] = 0 or keep for every cell c of every replica r < replicas
 * (1..DIE_MAX_REPLICAS; plane_stride >= W * H elements).  One launch. */
int die_dropout_mask(int32_t W, int32_t H, const die_nca_dropout* drop, int32_t replicas, int64_t plane_stride, float* out,
                     void* stream);

/* ---- Per-replica Dynamics on batched replicas (die_env.hip, die_init.hip; BatchedEnv(dynamics=[...])) ---------------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The replicas of a die_batch may live under different environment constants: rate_feed, rate_decay_chem, diffuse_sigma and
 * food_infinite of replica r come from row r of a device table, everything else (boundary, cost and its weights, agents_die,
 * has_dead_slots) stays shared in the die_dynamics of the call.  Replica r then computes, bit for bit, what a stand-alone world
 * under its own Dynamics computes.
 *   A row is one replica's constants as the kernels consume them.  64 bytes, so that a workgroup fetches its replica's row with
 * one scalar load (as die_physarum_row). */
typedef struct die_dynamics_row {
    float rate_feed;
    float keep;              /* (float)(1.0 - (double)rate_decay_chem): what the shared-Dynamics sweep multiplies by */
    int32_t food_infinite;
    int32_t radius;          /* (int)(4 * sigma + 0.5): 1..4 */
    float w[9];              /* the 2 * radius + 1 gaussian taps, (float) of the library's float64 taps; the rest 0 */
    float reserved[3];       /* 0 */
} die_dynamics_row;

/* n HOST rows from n die_dynamics for W x H replicas, with the taps the shared-Dynamics sweep computes for that sigma.  Nothing is
 * written unless every row is accepted.  Refused: n outside 1..DIE_MAX_REPLICAS; a radius outside 1..4 or H % 4 != 0
 * (DIE_ERR_UNSUPPORTED: the fused sweep does not apply); a diffuse_mode other than WRAP or staged != 0; a row that differs from
 * row 0 in boundary, cost, the two cost weights, agents_die or has_dead_slots. */
int die_dynamics_rows(const die_dynamics* d, int32_t n, int32_t W, int32_t H, die_dynamics_row* rows_host);

/* The three batched steps with the table: `rows` is a DEVICE array of b->replicas rows, `rows_host` the host rows it was uploaded
 * from (die_dynamics_rows' output; only the radii are read, to group the sweep's launches).  Replica r claims and feeds with
 * rows[r].rate_feed and is swept with rows[r]'s taps, keep, rate_feed and food_infinite; `d` supplies what does not vary (its own
 * rate_feed, rate_decay_chem, diffuse_sigma and food_infinite must still describe a valid world: they are checked as the parent
 * call checks them, and otherwise unused).  Each entry runs its parent's checks in the parent's order, then requires both tables.
 * The field sweep is launched once per distinct radius present (4 launches at most), each launch covering its replicas through a
 * by-value list of replica indices and running the kernel instantiation a stand-alone world of that radius takes; every replica
 * keeps its own reduction workgroup and result words.  With one radius the launch count is the parent's.
 * die_nca_env_step_batch_rows takes a nullable `drop`: NULL is die_nca_env_step_batch, else die_nca_env_step_batch_dropout. */
int die_forward_env_step_batch_rows(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_action* act,
                                    const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                    int64_t workspace_bytes, const die_dynamics_row* rows, const die_dynamics_row* rows_host,
                                    void* stream);
int die_physarum_env_step_batch_rows(const die_medium* m, const die_agents* a, die_gradient_agent* g, const die_physarum_row* table,
                                     const die_action* act, const die_dynamics* d, const die_batch* b, die_step_result* results,
                                     void* workspace, int64_t workspace_bytes, const die_dynamics_row* rows,
                                     const die_dynamics_row* rows_host, void* stream);
int die_nca_env_step_batch_rows(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                int64_t workspace_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                const die_dynamics_row* rows_host, void* stream);

/* ---- Batched replicas stepped with the caller's actions (die_env.hip; BatchedEnv.step_action) -------------------------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * die_env_step for R replicas: no agent forward runs, the claim pass reads `act` (required).  `m`, `a`, `act` describe replica 0;
 * replica r's three action arrays start r * b->agent_stride elements further (the layout the other batched steps write `act` in)
 * and only their first b->n[r] entries are read.  Replica r computes bit for bit what die_env_step computes on that world alone
 * with those actions: one claim launch (replica in blockIdx.y), with dead slots (d->agents_die / d->has_dead_slots) the dead-slot +
 * lifecycle launch, then the field sweep(s) of the other batched steps; the same workspace as they take.  Agents are in slot
 * order (a->slot NULL).  m->epoch is the epoch the claims are made at: the caller advances it, and clears the claim planes when
 * it wraps to 1.  Refused before any launch, in this order: a null argument (act included), the batched steps' world checks
 * (1..DIE_MAX_REPLICAS replicas, workspace, no decomposed medium or sense mask, chem_next a second plane, strides of at least a
 * replica, H % 4 == 0 and a gaussian radius of 1..4: DIE_ERR_UNSUPPORTED), a null action array, plane or agent array, the
 * step's own arguments (epoch, boundary, cost, n[r] in 1..agent_stride) and, for _rows, either table missing or a radius
 * outside 1..4. */
int die_env_step_batch(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d, const die_batch* b,
                       die_step_result* results, void* workspace, int64_t workspace_bytes, void* stream);
int die_env_step_batch_rows(const die_medium* m, const die_agents* a, const die_action* act, const die_dynamics* d,
                            const die_batch* b, die_step_result* results, void* workspace, int64_t workspace_bytes,
                            const die_dynamics_row* rows, const die_dynamics_row* rows_host, void* stream);

/* ---- The adjoint of the NeuralAutomataAgent sensing (die_nca_grad.hip; NeuralAutomataAgent.differentiable_sense / _action) -----
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The forward is z_l = conv_l(z_{l-1}) (die_conv2d per layer, z_0 = the medium's planes), s = tanh(z_L) * mask (the last layer's
 * launch), action[c, n] = s[c, cell_n] * coef[c] (die_gather_scale).  These calls give d loss / d weights of every layer from
 * d loss / d action; every argument is checked on the host before anything is launched. */

/* The read-out's adjoint: the three fp32 (m->W, m->H) planes are cleared (on `stream`), then
 *   grad_planes[c][cell_n] += grad_action[c][n] * coefs[c]   for EVERY slot n < a->N,
 * with die_gather_scale's indexing; grad_action's dx, dy, deposit arrays are the gradient's three rows.  fp32 atomic adds: where
 * several slots with a non-zero gradient stand on one cell the order of their sum is not fixed; the result is bit-reproducible
 * run to run whenever no two slots with a non-zero gradient share a cell (alive agents never do). */
int die_gather_scale_backward(const die_medium* m, const die_agents* a, const die_action* grad_action, const float* coefs,
                              float* const* grad_planes, void* stream);

/* Bytes of die_conv2d_backward's workspace: one partial row of cout * cin * k * k floats per 16 x 64 tile,
 *   ceil(W / 16) * ceil(H / 64) * cout * cin * k * k * 4;   -1 for a shape die_conv2d_backward refuses. */
int64_t die_conv2d_backward_workspace_bytes(int32_t W, int32_t H, int32_t cin, int32_t cout, int32_t k);

/* One layer's adjoint, two launches.  `in` / `epoch`: the layer's input planes as die_conv2d read them; `grad_out`: cout fp32
 * planes, the gradient at the layer's outputs; `weights`: (cout, cin, k, k).
 *   grad_weights[o, i, a, b] = sum_{x, y} g[o, x, y] * in[i, pad(x + a - r), pad(y + b - r)]   (cout * cin * k * k fp32, overwritten)
 *   grad_in[i, x, y] = sum_{o, a, b} weights[o, i, a, b] * g[o, pad'(x - a + r), pad'(y - b + r)]   (cin fp32 planes, overwritten;
 *       NULL: not wanted — the first layer's input is the medium.  pad': 'circular' wraps, 'zeros' drops what falls outside)
 * where g = grad_out, or, for the layer that carried the tanh, g = grad_out * mask * (1 - t * t): `fwd_out` are then that
 * layer's cout forward output planes t = tanh(z) WITHOUT the dropout mask (die_conv2d's, not die_conv2d_dropout's), and `drop`,
 * if the forward was masked, the die_nca_dropout it was masked with (the mask is recomputed, 0 or keep per cell; nothing is
 * divided by keep).  fwd_out NULL: no tanh in this layer (drop must then be NULL).
 *   The weight gradient uses no float atomics: the first launch writes one partial row per tile into `workspace`
 * (die_conv2d_backward_workspace_bytes), the second sums the rows in tile-index order in float64 and stores fp32 — the same
 * inputs give the same bits on every run.  k in {1, 3, 5, 7}, 1..4 channels; padding_mode DIE_PAD_CIRCULAR or DIE_PAD_ZEROS
 * (DIE_PAD_REFLECT / DIE_PAD_REPLICATE: DIE_ERR_UNSUPPORTED).  grad_in may be none of the call's other planes. */
int die_conv2d_backward(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                        const float* const* grad_out, int32_t k, const float* weights, float* grad_weights,
                        float* const* grad_in, const float* const* fwd_out, const die_nca_dropout* drop,
                        int32_t padding_mode, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The same adjoint for every replica of a die_batch (BatchedNeuralAutomataAgent.differentiable_sense / _action) ----------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * `m` / `a` describe replica 0 and `b` the strides, as in die_nca_env_step_batch (b->n[r] may be 0 here); the die_nca_batch's
 * `scratch` is not used by these calls and may be NULL.  Replica r computes, bit for bit, what the stand-alone calls above compute
 * on its world; the replica rides in blockIdx.z (conv) or blockIdx.y (read-out), so the launch counts do not depend on R.  Every
 * argument is checked on the host before anything is launched.
 *
 * die_nca_sense_batch_store: the L conv launches of die_nca_env_step_batch (replica r reads weight block r / E, the first layer
 * the claim plane at nca->sense_epoch), layer l's output of every replica kept in `store`, [L][R][4][W][H] fp32
 * (die_nca_sense_batch_store_bytes; -1 for a refused shape), instead of the ping-pong scratch.  With `drop` the last layer is
 * launched twice: unmasked into `store` (tanh(z), what the adjoint reads) and masked with key seed + r * seed_stride into `masked`,
 * [R][4][W][H] (required then, unused otherwise).  Nothing is stepped, claimed or moved. */
int64_t die_nca_sense_batch_store_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers);
int die_nca_sense_batch_store(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store, int64_t store_bytes,
                              float* masked, const die_nca_dropout* drop, void* stream);

/* The read-out of every replica, one launch: `sense` = replica 0's (dx, dy, deposit) planes, W * H elements apart, replica r's
 * sense_stride elements further (>= 3 * W * H);
 *   out[c][r * agent_stride + n] = sense_r[c][cell_n] * coefs[c] for n < b->n[r]   (die_gather_scale's indexing and product),
 *   out[c][r * agent_stride + n] = 0                              for b->n[r] <= n < agent_stride.   (out->N is not read.) */
int die_gather_scale_batch(const die_medium* m, const die_agents* a, const die_batch* b, const float* sense, int64_t sense_stride,
                           const float* coefs, const die_action* out, void* stream);

/* Its adjoint: the span grad_sense[0 .. (R - 1) * sense_stride + 3 * W * H) is cleared (on `stream`), then, one launch,
 *   grad_sense[r * sense_stride + c * W * H + cell_n] += grad_action[c][r * agent_stride + n] * coefs[c]   for n < b->n[r]
 * (the padding slots are not read).  fp32 atomic adds, as die_gather_scale_backward: bit-reproducible run to run whenever no two
 * slots of a replica with a non-zero gradient share a cell. */
int die_gather_scale_backward_batch(const die_medium* m, const die_agents* a, const die_batch* b, const die_action* grad_action,
                                    const float* coefs, float* grad_sense, int64_t sense_stride, void* stream);

/* The conv stack's adjoint, 2 launches per layer from the last.  `m`: replica 0's first-layer input planes as
 * die_nca_sense_batch_store read them (b->plane_stride apart); `store`: what that call wrote; `grad_sense`: the gradient at the
 * sense planes (3 planes W * H apart per replica, sense_stride between replicas); `drop`: the die_nca_dropout the forward was
 * masked with, or NULL.  Per layer, k_conv_backward with the replica in blockIdx.z — die_conv2d_backward's kernel body: replica r
 * stages weight block r / E, recomputes its own mask key and writes its partial rows to workspace[r][tile][cout * cin * k * k] —
 * then one thread per (candidate c, weight j) adds the partial rows of the candidate's E replicas in float64, episode e = 0 .. E - 1
 * outermost and tile index ascending inside, and stores fp32 at
 *   grad[c * grad_stride + offset_l + j],   offset_l = sum over the layers before l of cout * cin * k * k
 * (the row layout of parameters_to_vector; grad_stride >= the row's length).  No float atomics: the same inputs give the same bits
 * on every run; for E = 1 row r is die_conv2d_backward's gradient of replica r, bit for bit; for E > 1 row c is the float64 sum
 * over its E worlds, rounded once.  The gradient at the inputs of layers >= 2 travels through the workspace.
 *   Workspace (die_nca_backward_batch_workspace_bytes; -1 for a refused shape):
 *   (R * ceil(W / 16) * ceil(H / 64) * 4 * 4 * 7 * 7  +  min(n_layers - 1, 2) * R * 4 * W * H) * 4 bytes.
 * DIE_PAD_REFLECT / DIE_PAD_REPLICATE: DIE_ERR_UNSUPPORTED. */
int64_t die_nca_backward_batch_workspace_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers);
int die_nca_backward_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                           const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                           const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The adjoint of Env.step's chem path (die_env_grad.hip; Env.differentiable_step / Env.differentiable_chem) -----------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * One step maps (chem, deposit) to chem' = (1 - decay) * G(chem + D), D[cell] = deposit[n] where entry n won the cell; positions,
 * food and the claim plane are piecewise constant in an agent's parameters and carry no gradient.  Stand-alone worlds, fp32
 * planes, the periodic ('wrap') gaussian.  Every argument is checked on the host before anything is launched. */

/* Who deposited where.  Called right after die_env_step (or one of its equivalents), with the step's m->epoch and the post-move
 * coordinates; for array entry n with slot id s (a->slot[n], a->slot NULL: s = n)
 *   cells_out[n] = ix * m->H + iy   if a->alive[n] and the claim word of cell (ix, iy) carries (m->epoch, s + 1),
 *   cells_out[n] = -1               otherwise (dead slots; the losers of a shared cell),
 * with ix, iy and the claim word read as the step's kernels read them.  One launch; a->N int32 words are written, a->N == 0
 * launches nothing.  A slot that the step's lifecycle (agents_die) zeroed is dead by now and gets -1.  DIE_ERR_UNSUPPORTED for a
 * decomposed medium (m->gW > 0) and for more than 2^31 - 1 cells. */
int die_deposit_cells(const die_medium* m, const die_agents* a, int32_t* cells_out, void* stream);

/* The step's adjoint:
 *   grad_chem = (1 - decay) * G^T(grad_chem_next)                    (W x H fp32, overwritten)
 *   grad_deposit[n] = cells[n] >= 0 ? grad_chem[cells[n]] : 0        (N fp32, overwritten; cells as die_deposit_cells wrote them)
 * On the torus with symmetric taps G^T = G, so the field part is die_diffuse_decay itself on the gradient plane — the forward's
 * taps and kernels (the row sweep where H % 4 == 0 and the radius is at most 4, the LDS-tiled kernel elsewhere); there is no
 * second gaussian.  grad_deposit is a gather in plain loads and stores after the sweep: no atomics, every output written once,
 * the same bits on every run; an index at or beyond W * H counts as negative.  grad_chem may not alias grad_chem_next, nor
 * grad_deposit any other argument.  N == 0 or grad_deposit == NULL: the field part only (cells is not read).  sigma as
 * die_diffuse_decay takes it (radius int(4 sigma + .5) in 1..8, else DIE_ERR_ARG / DIE_ERR_UNSUPPORTED). */
int die_env_step_backward(int32_t W, int32_t H, const float* grad_chem_next, float sigma, float decay, int64_t N,
                          const int32_t* cells, float* grad_chem, float* grad_deposit, void* stream);

/* ---- The same adjoint for the replicas of a die_batch (die_env_grad.hip, die_nca_grad.hip; BatchedEnv.differentiable_step) -------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * Replica r of every call below computes, bit for bit, what its stand-alone twin above computes on that world alone. */

/* die_deposit_cells for every replica in one launch (replica in blockIdx.y).  `m`, `a` describe replica 0, the claim planes
 * b->plane_stride and the agent arrays b->agent_stride apart; batched agents are in slot order (a->slot must be NULL), so entry
 * n's slot id is n.  cells_out[r * agent_stride + n] = ix * m->H + iy (the cell within replica r's plane) under die_deposit_cells'
 * rule for n < b->n[r], -1 otherwise; the padding b->n[r] <= n < agent_stride is written -1, so all replicas * agent_stride words
 * are written.  Refused as die_deposit_cells refuses, and: replicas outside 1..DIE_MAX_REPLICAS, plane_stride < W * H,
 * agent_stride < a->N, a b->n[r] outside 0..agent_stride. */
int die_deposit_cells_batch(const die_medium* m, const die_agents* a, const die_batch* b, int32_t* cells_out, void* stream);

/* die_env_step_backward for every replica: grad_chem_next and grad_chem are b->replicas fp32 planes b->plane_stride apart (16-byte
 * aligned, plane_stride a multiple of 4), cells and grad_deposit rows of b->agent_stride entries.
 *   rows == NULL (and rows_host == NULL): one sweep launch for all replicas with the taps and (1 - decay) of (sigma, decay), built as
 *     die_diffuse_decay builds them.  Otherwise both tables of a die_*_env_step_batch_rows call: replica r is swept with rows[r]'s
 *     taps and keep, one launch per radius present; sigma and decay are ignored.
 *   Then one gather launch: grad_deposit[r * agent_stride + n] = cells[...] in [0, W * H) ? grad_chem_r[cells[...]] : 0 for
 *     n < b->n[r], and 0 for the padding up to agent_stride.  grad_deposit == NULL: the field part only (cells, agent_stride and n[]
 *     are not read).
 * No atomics, every output written once.  Refused before any launch: a null plane or batch, replicas outside 1..DIE_MAX_REPLICAS,
 * plane_stride < W * H, buffers that overlap (grad_chem with grad_chem_next; grad_deposit with either or with cells), one table
 * without the other, H % 4 != 0 or a radius outside 1..4 (DIE_ERR_UNSUPPORTED: a batched world always has the row sweep),
 * misaligned planes, and with grad_deposit null cells or a b->n[r] outside 0..agent_stride. */
int die_env_step_backward_batch(int32_t W, int32_t H, const die_batch* b, const float* grad_chem_next, float sigma, float decay,
                                const die_dynamics_row* rows, const die_dynamics_row* rows_host, const int32_t* cells,
                                float* grad_chem, float* grad_deposit, void* stream);

/* die_nca_backward_batch whose layer-0 launch also writes the gradient at the first layer's cin input planes (the kernel's has_gin
 * path, as for the layers above it): replica r's planes start at grad_in + r * grad_in_stride, W * H apart, in the layer's channel
 * order ([agents,] food, chem).  The weight gradient is bit for bit die_nca_backward_batch's; replica r's input gradient is bit for
 * bit die_conv2d_backward's grad_in on that world.  grad_in_stride >= cin * W * H; where H % 4 == 0 grad_in is 16-byte aligned and
 * grad_in_stride a multiple of 4; grad_in may overlap none of the call's other buffers. */
int die_nca_backward_batch_inputs(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                  const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                  const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                  int64_t grad_in_stride, void* stream);

/* ---- Wide NeuralAutomataAgent stacks: hidden channels and activations (die_nca_wide.hip; ConvolutionModel(hidden_channels=C,
 * hidden_activation=...)) -----------------------------------------------------------------------------------------------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.  die_conv2d,
 * die_nca_env_step_batch and their kin keep their 1..4 channels, their kernels and their refusals; a stack whose layers are
 * obs -> C -> ... -> C -> 3 with an activation after every layer takes the three entry points below for every layer.
 *   A layer is die_conv2d's cross-correlation with 1..32 channels in and out and k = 1, 3 or 5 (32 * 32 * 49 weights would not fit
 * LDS next to a tile), evaluated as an implicit GEMM on the fp32-input matrix instruction (v_mfma_f32_16x16x4_f32: exact fp32,
 * bit for bit a k-ordered fmaf chain).  Each output is summed over (chunk of 4 input channels, a, b, channel in the chunk) in
 * that order by one kernel body, which both calls launch: replica r of the batched step is the stand-alone call, bit for bit. */
typedef enum die_nca_activation { DIE_NCA_ACT_NONE = 0, DIE_NCA_ACT_TANH = 1, DIE_NCA_ACT_RELU = 2 } die_nca_activation;
/* One layer: out[o] = act(conv(in))[o] (* the dropout mask of `drop`, which may be NULL: as die_conv2d_dropout, after the
 * activation) for o < cout, output plane o at out + o * out_stride (out_stride >= W * H elements; nothing else is written).
 * `in`: cin planes as die_conv2d reads them (fp32 / fp16 fields, the claim plane at `epoch`); `weights`: (cout, cin, k, k) fp32 on
 * the device; `activation`: a die_nca_activation; `padding_mode`: a die_pad_mode.  Every argument is checked before anything is
 * launched, and all of these are DIE_ERR_ARG: W or H < 1, cin or cout outside 1..32, k other than 1, 3, 5, 'reflect' padding of a
 * field no larger than k / 2, an unknown activation or padding mode, a null pointer, an input plane that is not one of the four
 * kinds, out_stride below a plane, an input plane that overlaps the output planes (in-place), a bad `drop` (die_nca_dropout's
 * rules).  Where H % 4 == 0, `out` is 16-byte aligned and out_stride a multiple of 4, the stores are 16 bytes wide. */
int die_conv2d_wide(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout, float* out,
                    int64_t out_stride, int32_t k, const float* weights, int32_t activation, int32_t padding_mode,
                    const die_nca_dropout* drop, void* stream);
/* Bytes of die_conv2d_wide_backward's workspace: one partial row of cout * cin * k * k floats per 16 x 64 tile,
 *   ceil(W / 16) * ceil(H / 64) * cout * cin * k * k * 4;   -1 for a shape die_conv2d_wide_backward refuses. */
int64_t die_conv2d_wide_backward_workspace_bytes(int32_t W, int32_t H, int32_t cin, int32_t cout, int32_t k);
/* The adjoint of one die_conv2d_wide layer (die_nca_wide_grad.hip; added within ABI 24: new symbols only).  The forward returned
 * y = act(conv(in, weights)) (* the mask of `drop`); given the gradient at y (`grad_out`, plane o at grad_out + o * grad_out_stride)
 * and the layer's UNMASKED output t = act(z) (`fwd_out`, plane o at fwd_out + o * fwd_out_stride; NULL only with DIE_NCA_ACT_NONE
 * and no drop), the gradient at z is g_z = grad_out * mask * act'(t) — act'(t) = 1 - t^2 for tanh, (t > 0 ? 1 : 0) for relu, 1 for
 * none; the mask recomputed from its key, never divided out — formed while the kernels stage their operands, and
 *   grad_weights[o, i, a, b] = sum_xy g_z[o, x, y] * in[i, pad(x + a - r), pad(y + b - r)]        (cout, cin, k, k) fp32,
 *   grad_in[i, x, y] = sum_o sum_a sum_b weights[o, i, a, b] * g_z[o, pad'(x - a + r), pad'(y - b + r)]   (nullable; plane i at
 *                      grad_in + i * grad_in_stride),
 * both on v_mfma_f32_16x16x4_f32.  At most three launches: the weight-gradient kernel writes one partial row per tile into the
 * workspace (every element once, no float atomics), the input-gradient kernel runs when grad_in is given, and the fold sums the
 * rows in tile-index order in float64 (die_conv2d_backward's) — the same inputs give the same bits on every run.  Shapes as
 * die_conv2d_wide: 1..32 channels, k = 1, 3, 5; `in` as die_conv2d_wide reads it.  Every argument is checked before anything is
 * launched: DIE_PAD_REFLECT / DIE_PAD_REPLICATE are DIE_ERR_UNSUPPORTED; DIE_ERR_ARG for a bad size, channel count, kernel size,
 * activation or padding mode, a null pointer, a NULL fwd_out where it is needed, a stride below a plane, grad_weights == weights,
 * grad_in overlapping any other buffer of the call, a workspace below die_conv2d_wide_backward_workspace_bytes, a bad `drop`, and,
 * where H % 4 == 0 (16-byte stores), a grad_in that is not 16-byte aligned or a grad_in_stride that is no multiple of 4. */
int die_conv2d_wide_backward(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                             const float* grad_out, int64_t grad_out_stride, const float* fwd_out, int64_t fwd_out_stride,
                             int32_t k, const float* weights, int32_t activation, int32_t padding_mode,
                             const die_nca_dropout* drop, float* grad_weights, float* grad_in, int64_t grad_in_stride,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* Bytes of a batched wide stack's scratch, [set][replica][max_channels][W][H] fp32 with set = layer % 2 (one set for a single
 * layer) and max_channels the largest cout of the stack:
 *   (n_layers >= 2 ? 2 : 1) * replicas * max_channels * W * H * 4;
 * -1 for W or H < 1, replicas outside 1..DIE_MAX_REPLICAS, n_layers outside 1..DIE_NCA_MAX_LAYERS, max_channels outside 1..32. */
int64_t die_nca_wide_batch_scratch_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers, int32_t max_channels);
/* die_nca_env_step_batch_rows for a wide stack: the same step (the same read-out and claim launch, lifecycle launch, sweeps
 * and epoch-wrap clear) behind L launches of the wide layer kernel with the replica in blockIdx.z.  `nca` is a die_nca_batch
 * whose layers may have 1..32 channels and k = 1, 3, 5, and whose die_nca_layer.reserved is READ, as the layer's
 * die_nca_activation: any of the three for a hidden layer, DIE_NCA_ACT_TANH for the last (the other entry points ignore that
 * word, as they always have).  nca->scratch holds die_nca_wide_batch_scratch_bytes(W, H, replicas, n_layers, largest cout)
 * bytes; the last layer's (dx, dy, deposit) planes of replica r stay at set (n_layers - 1) % 2, replica stride
 * largest cout * W * H, until the next call.  `drop` (nullable): the last layer is masked as in die_nca_env_step_batch_dropout.
 * `rows` and `rows_host` (nullable, both or neither): per-replica Dynamics as in die_nca_env_step_batch_rows.  `act` may be NULL.
 * Checked before anything is launched, in die_nca_env_step_batch's order with the wide limits in place of the narrow ones. */
int die_nca_wide_env_step_batch(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                int64_t workspace_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                const die_dynamics_row* rows_host, void* stream);

/* ---- The stock channel: agents sense their own agent_food (die_stock.hip; NeuralAutomataAgent(with_stock_channel=True)) ------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * A stock plane is a W * H plane of uint64 words in the claim plane's format, the stock in place of the deposit:
 *   word = ((epoch << DIE_OWNER_EPOCH_SHIFT | slot id + 1) << 32) | float bits of agent_food.
 * die_stock_plane takes the agents as they are and, for every ALIVE slot in ascending slot id, sets the word of the cell it
 * stands on (the nearest label, as every cell lookup here): where several alive agents share a cell the highest slot id wins
 * (numpy's last writer, the deposit claim's rule), dead slots contribute nothing, negative and denormal stocks keep their bits.
 * One launch, one thread per slot, one 64-bit atomicMax per alive slot with slot id `agents->slot ? slot[n] : n`: no float
 * atomics, the result does not depend on the storage order and is the same on every run.
 *   The call does NOT clear.  `plane` must be zero, or hold only words tagged with earlier epochs of the same 1..31 cycle (they
 * lose against this build's words and read as empty afterwards); a word of the same or a later epoch would survive and read as
 * an agent that is not there.  Whoever owns the plane zeroes it when the epoch does not grow (NeuralAutomataAgent, BatchedEnv).
 *   A layer call reads the plane as DIE_PLANE_STOCK with the call's one `epoch`: occupied ? payload : 0.f, fp32 whatever the field
 * dtype.
 * Checked before the launch: a null pointer (m, agents, plane, or one of x, y, alive, agent_food), W or H < 1, a decomposed
 * medium (m->gW > 0: DIE_ERR_UNSUPPORTED), epoch outside 1..DIE_OWNER_EPOCH_MAX, more slots than a claim word can name. */
int die_stock_plane(const die_medium* m, const die_agents* agents, int32_t epoch, unsigned long long* plane, void* stream);
/* R planes in ONE launch (the replica in blockIdx.y): replica r's slots start at r * b->agent_stride, its plane at
 * planes + r * b->plane_stride; the padding slots n >= b->n[r] are skipped.  Checked as die_stock_plane, and: a null batch,
 * replicas outside 1..DIE_MAX_REPLICAS, plane_stride below a plane, agent_stride < 1, n[r] outside 0..agent_stride. */
int die_stock_plane_batch(const die_medium* m, const die_agents* agents, const die_batch* b, int32_t epoch,
                          unsigned long long* planes, void* stream);
/* die_nca_env_step_batch_rows / die_nca_wide_env_step_batch for a population that senses its stock.  `stock`: R stock planes,
 * b->plane_stride apart.  stock == NULL: the parent call itself.  Otherwise, in order: the parent's checks in the parent's order
 * with layer 0 reading 2 + with_agent_channel + 1 planes (`drop` nullable; `rows` and `rows_host` nullable, both or neither, for
 * the narrow stack as well); the stock build at nca->sense_epoch from the agents as the call finds them; the parent's launches
 * with the stock plane as layer 0's LAST input: L + 3 launches per step.  Where the parent clears the claim planes (sense_epoch ==
 * DIE_OWNER_EPOCH_MAX) the stock planes are cleared with them.  The planes must satisfy die_stock_plane's rule on entry:
 * consecutive calls on the same planes do by themselves; after anything else the caller zeroes them.  A narrow stack stays
 * within 4 channels (4 -> 4 hidden layers; the scratch holds 4 planes per replica already). */
int die_nca_env_step_batch_stock(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                 const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                 int64_t workspace_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                 const die_dynamics_row* rows_host, unsigned long long* stock, void* stream);
int die_nca_wide_env_step_batch_stock(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                      const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                      int64_t workspace_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                      const die_dynamics_row* rows_host, unsigned long long* stock, void* stream);

/* ---- Memory channels: agents carry M values between forwards (die_memory.hip; NeuralAutomataAgent(memory_channels=M)) ------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The memory is an (M, N) fp32 array indexed by SLOT ID (agents->slot ? slot[n] : n), row j at memory + j * row_stride.  One
 * forward: a standing plane (die_stock_plane's words at `epoch`: who stands on each cell, the highest slot id of
 * the alive ones; the payload is ignored) is expanded into M fp32 observation planes, the wide stack runs with them as plain
 * DIE_PLANE_F32 inputs and gives 3 + M planes, and the planes 3.. are read out at the agents' cells into the memory.
 *
 * die_memory_planes — the expand, one launch: P_j[c] = occupied(c at epoch) ? memory[j][winner(c)] : +0.0f for every cell c and
 * j < memory_channels, plane j at planes + j * plane_stride.  EVERY cell of every plane is written (nobody clears them); the
 * words between two planes (plane_stride > W * H) are left alone; the values are moved as 32-bit words (negative zero, denormals
 * and negative values keep their bits); a winner id >= n_slots reads as empty.  16-byte stores where H % 4 == 0 and the planes
 * and strides are 16-byte aligned.  Checked before the launch (DIE_ERR_ARG): a null pointer, W or H < 1, memory_channels outside
 * 1..DIE_MEMORY_MAX_CHANNELS, epoch outside 1..DIE_OWNER_EPOCH_MAX, n_slots outside 0..DIE_OWNER_SLOT_MASK - 1, row_stride <
 * max(n_slots, 1), plane_stride < W * H, output planes that overlap the standing plane or the memory; a decomposed medium
 * (m->gW > 0) is DIE_ERR_UNSUPPORTED.  Of `m` only W, H and gW are read. */
#define DIE_MEMORY_MAX_CHANNELS 8
int die_memory_planes(const die_medium* m, const unsigned long long* standing, int32_t epoch, int32_t memory_channels,
                      const float* memory, int64_t row_stride, int64_t n_slots, float* planes, int64_t plane_stride, void* stream);
/* R replicas in ONE launch (the replica in blockIdx.y).  Replica r: standing plane at standing + r * b->plane_stride, memory
 * rows at memory + (r * memory_channels + j) * row_stride with b->n[r] slots, output plane j at planes + (j * R + r) *
 * b->plane_stride — the layout in which a batched layer launch reads plane j of every replica b->plane_stride apart.  Checked as
 * die_memory_planes, and: a null batch, replicas outside 1..DIE_MAX_REPLICAS, b->plane_stride < W * H, agent_stride < 1, n[r]
 * outside 0..agent_stride, row_stride < agent_stride. */
int die_memory_planes_batch(const die_medium* m, const die_batch* b, const unsigned long long* standing, int32_t epoch,
                            int32_t memory_channels, const float* memory, int64_t row_stride, float* planes, void* stream);
/* die_gather_memory — the read-out, one launch, one thread per stored slot n < agents->N, no atomics (slot ids are distinct):
 *   memory[j][id] = alive[n] ? planes_j[cell of slot n] : +0.0f,  id = agents->slot ? slot[n] : n,  j < memory_channels,
 * plane j at planes + j * plane_stride (the stack's planes 3..: no coefficient).  Dead slots are zeroed; an id >= agents->N is
 * skipped.  Checked before the launch (DIE_ERR_ARG): a null pointer (m, agents, planes, memory, or one of x, y, alive), W or H
 * < 1, memory_channels outside 1..DIE_MEMORY_MAX_CHANNELS, N outside 0..DIE_OWNER_SLOT_MASK - 1, plane_stride < W * H,
 * row_stride < max(N, 1), a memory that overlaps the planes; a decomposed medium is DIE_ERR_UNSUPPORTED. */
int die_gather_memory(const die_medium* m, const die_agents* agents, int32_t memory_channels, const float* planes,
                      int64_t plane_stride, float* memory, int64_t row_stride, void* stream);
/* R replicas in ONE launch (blockIdx.y): replica r's slots start at r * b->agent_stride (slot order: agents->slot must be NULL),
 * its planes at planes + r * replica_stride + j * plane_stride, its memory rows at memory + (r * memory_channels + j) *
 * row_stride.  The padding slots n >= b->n[r] are neither read nor written.  Checked as die_gather_memory, and: a null batch, a
 * slot array, replicas outside 1..DIE_MAX_REPLICAS, b->plane_stride or plane_stride < W * H, replica_stride below a replica's
 * planes, agent_stride < 1, n[r] outside 0..agent_stride, row_stride < agent_stride. */
int die_gather_memory_batch(const die_medium* m, const die_agents* agents, const die_batch* b, int32_t memory_channels,
                            const float* planes, int64_t plane_stride, int64_t replica_stride, float* memory, int64_t row_stride,
                            void* stream);
/* die_nca_wide_env_step_batch_stock for a population whose agents carry memory.  Its arguments, and: `standing`, R uint64
 * planes b->plane_stride apart (the stock planes' rule: zero, or words of earlier epochs of the cycle); memory_channels = M in
 * 1..DIE_MEMORY_MAX_CHANNELS; `memory`, the dense (R, M, b->agent_stride) array; `memory_planes`, R * M fp32 planes laid out as
 * die_memory_planes_batch writes them; with_stock (0 / 1): layer 0 also reads the standing planes as DIE_PLANE_STOCK, its last
 * input.  In order: the parent's checks in the parent's order, with layer 0 reading 2 + with_agent_channel + M + with_stock
 * planes ([agents], food, chem, memory_0 .. memory_{M-1}, [stock]) and the last layer giving 3 + M; the standing build at
 * nca->sense_epoch (die_stock_plane_batch's launch: with_stock = 0 simply ignores the payload); the expand; the L wide layer
 * launches (the last layer's tanh and mask on all 3 + M planes); the memory read-out of planes 3.. — before anything moves —;
 * the parent's read-out-and-claim launch on planes 0..2, lifecycle and sweeps: L + 5 launches.  On the epoch wrap the standing
 * planes are cleared with the claim planes.  Also refused (DIE_ERR_ARG): a null standing / memory / memory_planes, M out of
 * range, with_stock not 0 or 1. */
int die_nca_wide_env_step_batch_memory(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                       const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                       int64_t workspace_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                       const die_dynamics_row* rows_host, unsigned long long* standing, int32_t memory_channels,
                                       float* memory, float* memory_planes, int32_t with_stock, void* stream);

/* ---- Signal channels: a field the agents write and read (die_signal.hip; NeuralAutomataAgent(signal_channels=K)) -----------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The field is K fp32 planes, whatever the medium's dtype.  One forward: the wide stack reads them as plain
 * DIE_PLANE_F32 inputs (after chem, before the memory planes) and gives 3 + K + M planes; the planes 3 .. 3 + K - 1 are the
 * emissions, and the field is updated from them at the occupied cells of a standing plane (die_stock_plane's words at `epoch`:
 * alive slots only; the payload is ignored, so agents sharing a cell emit once).
 *
 * die_signal_step — the update, one launch for all K planes:
 *   E_k[c] = occupied(c at epoch) ? deposit * emission_k[c] : +0.0f          (one fp32 multiply)
 *   field_out_k = (1 - decay) * gaussian(field_in_k + E_k, sigma, mode 'wrap', truncate 4)
 * in fp32: one fp32 add, then exactly die_diffuse_decay's arithmetic (the same device bodies with another loader).  Emission plane
 * k at emission_planes + k * plane_stride, field plane k at field_in / field_out + k * field_stride.  EVERY cell of every output
 * plane is written (nobody clears them); the words between two planes are left alone.  The row-marching kernel with 16-byte
 * accesses runs where H % 4 == 0, the radius is at most 4 and every pointer and stride is 16-byte aligned; the LDS-tiled one
 * elsewhere.  Checked before the launch (DIE_ERR_ARG): a null pointer, W or H < 1, signal_channels outside
 * 1..DIE_SIGNAL_MAX_CHANNELS, epoch outside 1..DIE_OWNER_EPOCH_MAX, a sigma whose radius int(4 sigma + .5) lies outside 1..8, decay
 * outside [0, 1], a deposit that is not finite, plane_stride or field_stride < W * H, a field_out that overlaps field_in, the emission
 * planes or the standing plane; a decomposed medium (m->gW > 0) is DIE_ERR_UNSUPPORTED.  Of `m` only W, H and gW are read. */
#define DIE_SIGNAL_MAX_CHANNELS 8
int die_signal_step(const die_medium* m, const unsigned long long* standing, int32_t epoch, int32_t signal_channels,
                    const float* emission_planes, int64_t plane_stride, const float* field_in, float* field_out, int64_t field_stride,
                    float deposit, float sigma, float decay, void* stream);
/* All K planes of all R replicas in ONE launch (plane k of replica r is blockIdx.z = k * R + r).  Replica r: standing plane at
 * standing + r * b->plane_stride, emission plane k at emission_planes + r * replica_stride + k * plane_stride (a stack's scratch),
 * field plane k at field_in / field_out + (k * R + r) * b->plane_stride — the layout in which a batched layer launch reads plane k
 * of every replica b->plane_stride apart.  Checked as die_signal_step, and: a null batch, replicas outside 1..DIE_MAX_REPLICAS,
 * b->plane_stride < W * H, agent_stride < 1, n[r] outside 0..agent_stride, replica_stride below a replica's K planes. */
int die_signal_step_batch(const die_medium* m, const die_batch* b, const unsigned long long* standing, int32_t epoch,
                          int32_t signal_channels, const float* emission_planes, int64_t plane_stride, int64_t replica_stride,
                          const float* field_in, float* field_out, float deposit, float sigma, float decay, void* stream);
/* die_nca_wide_env_step_batch_memory for a population whose agents also write a signal field.  Its arguments — memory_channels = 0
 * with null memory and memory_planes is allowed: no memory — and: signal_channels = K in 1..DIE_SIGNAL_MAX_CHANNELS; field_in and
 * field_out, K * R fp32 planes each, laid out as die_signal_step_batch reads them; the three constants.  In order: the parent's
 * checks in the parent's order, with layer 0 reading 2 + with_agent_channel + K + M + with_stock planes ([agents], food, chem,
 * signal_0 .., memory_0 .., [stock]) and the last layer giving 3 + K + M; die_signal_step's checks; the standing build; the expand if
 * M > 0; the L wide layer launches; the memory read-out of planes 3 + K .. if M > 0; the signal step on planes 3 .. 3 + K - 1; the
 * parent's claim, lifecycle and sweeps: L + 4 launches, L + 6 with memory.  The caller swaps field_in and field_out afterwards. */
int die_nca_wide_env_step_batch_signal(const die_medium* m, const die_agents* a, const die_nca_batch* nca, const die_action* act,
                                       const die_dynamics* d, const die_batch* b, die_step_result* results, void* workspace,
                                       int64_t workspace_bytes, const die_nca_dropout* drop, const die_dynamics_row* rows,
                                       const die_dynamics_row* rows_host, unsigned long long* standing, int32_t memory_channels,
                                       float* memory, float* memory_planes, int32_t with_stock, int32_t signal_channels,
                                       const float* field_in, float* field_out, float deposit, float sigma, float decay, void* stream);

/* ---- The signal channels' adjoint: backpropagation through the field for a stand-alone agent (die_signal_grad.hip) ----------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * die_signal_step is F' = (1 - decay) * G(F + occ * deposit * S) with G the periodic symmetric gaussian; on the torus G^T = G, so
 *   grad_F = (1 - decay) * G(grad_F')                 the forward's own sweep on the gradient planes
 *   grad_S_k[c] = occ[c] ? deposit * grad_F_k[c] : +0.0f     (one fp32 multiply of the value about to be stored)
 *
 * die_signal_cells — the record of one forward, taken after the standing plane is built (die_stock_plane at `epoch`): one launch,
 *   occupied_out[c] = (standing[c] is occupied at epoch) ? 1 : 0     for all m->W * m->H cells, one byte each.
 * EVERY byte is written (16-byte stores where both planes are 16-byte aligned, single bytes elsewhere and on the tail); nothing
 * beyond W * H is touched.  A graph that keeps this plane survives the next standing build, every step, re-sort and reset of the
 * field; it costs 1 byte per cell where a copy of the standing plane costs 8.  Checked before the launch (DIE_ERR_ARG): a null
 * pointer, W or H < 1, epoch outside 1..DIE_OWNER_EPOCH_MAX, an output that overlaps the standing plane; a decomposed medium
 * (m->gW > 0) is DIE_ERR_UNSUPPORTED.  Of `m` only W, H and gW are read.
 *
 * die_signal_step_backward — one launch for all K planes: the forward's sweep on grad_field_next (plane k at k * field_stride);
 * at the store the value o goes to grad_field + k * field_stride and occupied[c] ? deposit * o : +0.0f to grad_emission +
 * k * plane_stride.  Either output may be null (its store is skipped; the other gets the same bits), not both: the first link of
 * a chain, whose incoming field is a constant, needs the emission gradient alone.  grad_field is bit for bit what die_signal_step
 * writes for the field grad_field_next where nobody stands.  EVERY cell of every output plane is written; the words between two
 * planes are left alone; the inputs are only read.  The row-marching kernel runs where H % 4 == 0, the radius is at most 4, every
 * float pointer and stride is 16-byte aligned and `occupied` 4-byte aligned (a lane reads the mask of its 4 cells as one word);
 * the LDS-tiled one elsewhere.  Checked before the launch (DIE_ERR_ARG): a null occupied or grad_field_next, both outputs null, W
 * or H < 1, signal_channels outside 1..DIE_SIGNAL_MAX_CHANNELS, a sigma whose radius lies outside 1..8, decay outside [0, 1], a
 * deposit that is not finite, field_stride < W * H, plane_stride < W * H with a grad_emission, an output that overlaps an input or
 * the other output. */
int die_signal_cells(const die_medium* m, const unsigned long long* standing, int32_t epoch, uint8_t* occupied_out, void* stream);
int die_signal_step_backward(int32_t W, int32_t H, const uint8_t* occupied, int32_t signal_channels, const float* grad_field_next,
                             int64_t field_stride, float* grad_field, float* grad_emission, int64_t plane_stride, float deposit,
                             float sigma, float decay, void* stream);

/* ---- The memory channels' adjoints: backpropagation through time for a stand-alone agent (die_memory_grad.hip) -------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * All records and memories are indexed by SLOT ID (agents->slot ? slot[n] : n), as die_gather_memory indexes the memory, so
 * what a graph keeps survives every re-sort of the storage.
 *
 * die_memory_cells — the record of one forward, taken after the standing plane is built (die_stock_plane at `epoch`) and before
 * anything moves; one launch, one thread per stored entry, two int32 arrays of agents->N words:
 *   cell_out[id] = ix * m->H + iy (die_cell_u of the entry's coordinates) for an alive slot, -1 for a dead one;
 *   win_out[id]  = that cell where the standing word there, at `epoch`, names id + 1, else -1 (dead slots and the losers of a
 *                  shared cell).
 * An id >= agents->N is skipped; N == 0 launches nothing.  Checked before the launch (DIE_ERR_ARG): a null pointer (m, agents,
 * standing, an output, or one of x, y, alive while N > 0), W or H < 1, more than 2^31 - 1 cells, epoch outside
 * 1..DIE_OWNER_EPOCH_MAX, N outside 0..DIE_OWNER_SLOT_MASK - 1, an output that overlaps the other one, the standing plane or an
 * agent array; a decomposed medium (m->gW > 0) is DIE_ERR_UNSUPPORTED.  Of `m` only W, H and gW are read. */
int die_memory_cells(const die_medium* m, const die_agents* agents, const unsigned long long* standing, int32_t epoch,
                     int32_t* cell_out, int32_t* win_out, void* stream);
/* die_memory_planes_backward — die_memory_planes' adjoint, one launch, a pure gather in plain loads and stores:
 *   grad_memory[j][id] = 0 <= win[id] < W * H ? grad_planes[j][win[id]] : +0.0f     for every id < n_slots and j < memory_channels
 * (row j at grad_memory + j * row_stride, plane j at grad_planes + j * plane_stride; `win` as die_memory_cells wrote it).  Every
 * word of the M rows is written exactly once, the values are moved as 32-bit words, no atomics: the same bits on every run.
 * n_slots == 0 launches nothing.  Checked before the launch (DIE_ERR_ARG): a null pointer, W or H < 1, more than 2^31 - 1 cells,
 * memory_channels outside 1..DIE_MEMORY_MAX_CHANNELS, n_slots outside 0..DIE_OWNER_SLOT_MASK - 1, row_stride < max(n_slots, 1),
 * plane_stride < W * H, a grad_memory that overlaps `win` or grad_planes. */
int die_memory_planes_backward(int32_t W, int32_t H, int32_t memory_channels, int64_t n_slots, const int32_t* win,
                               const float* grad_planes, int64_t plane_stride, float* grad_memory, int64_t row_stride, void* stream);
/* die_gather_memory_backward — die_gather_memory's adjoint: the W * H cells of each of the M planes are cleared on `stream` (the
 * words between two planes are left alone), then one launch adds
 *   grad_planes[j][cell[id]] += grad_memory[j][id]     for every id < n_slots with 0 <= cell[id] < W * H and j < memory_channels
 * (`cell` as die_memory_cells wrote it; a zero term is skipped).  fp32 atomic adds, as die_gather_scale_backward: the result is
 * bit-reproducible run to run whenever no cell holds more than two alive slots with a non-zero gradient (two addends commute,
 * three need not).  n_slots == 0 clears the planes and launches nothing.  Checked before anything is cleared (DIE_ERR_ARG): as
 * die_memory_planes_backward, with grad_planes the output that may overlap neither `cell` nor grad_memory. */
int die_gather_memory_backward(int32_t W, int32_t H, int32_t memory_channels, int64_t n_slots, const int32_t* cell,
                               const float* grad_memory, int64_t row_stride, float* grad_planes, int64_t plane_stride, void* stream);

/* ---- The wide stack's adjoint for every replica of a die_batch (BatchedNeuralAutomataAgent.forward_device) -----------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The wide twins of die_nca_sense_batch_store / die_nca_backward_batch_inputs: `m` describes replica 0 and `b` the strides,
 * nca->scratch is not used and may be NULL, die_nca_layer.reserved is READ as the layer's activation (as
 * die_nca_wide_env_step_batch reads it), the replica rides in blockIdx.z and replica r reads weight block r / E.
 *
 * die_nca_wide_sense_batch_store: die_nca_wide_env_step_batch's L launches of the wide layer kernel, layer l's unmasked output
 * act(z) of every replica kept in `store`, [L][R][Cmax][W][H] fp32 with Cmax the largest cout of the stack
 * (die_nca_wide_sense_batch_store_bytes = n_layers * replicas * max_channels * W * H * 4; -1 for a refused shape).  With `drop`
 * the last layer is launched twice: unmasked into `store` and masked with key seed + r * seed_stride into `masked`,
 * [R][Cmax][W][H] (required then, unused otherwise).  Nothing is stepped, claimed or moved. */
int64_t die_nca_wide_sense_batch_store_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers, int32_t max_channels);
int die_nca_wide_sense_batch_store(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store, int64_t store_bytes,
                                   float* masked, const die_nca_dropout* drop, void* stream);

/* The stack's adjoint.  `m`: replica 0's first-layer planes as die_nca_wide_sense_batch_store read them (fp32, fp16 or the
 * claim plane at nca->sense_epoch, b->plane_stride apart); `store`: what that call wrote; `grad_sense`: the gradient at the sense
 * planes (3 planes W * H apart per replica, sense_stride between replicas); `drop`: the die_nca_dropout the forward was masked
 * with, or NULL.  Per layer, from the last to the first: die_conv2d_wide_backward's weight-gradient kernel with gridDim.z = R
 * (replica r writes its partial rows at workspace rows (r * tiles + tile)), its input-gradient kernel (layers >= 1 into a
 * ping-pong pair of [R][Cmax][W][H] sets in the workspace; layer 0 only when `grad_in` is given: replica r's cin_0 planes at
 * grad_in + r * grad_in_stride, in channel order ([agents,] food, chem)), and the fold: one thread per (candidate c, weight j)
 * adds the candidate's E * tiles partial rows in ascending order in float64 and stores fp32 at
 *   grad[c * grad_stride + offset_l + j]   (the row layout of parameters_to_vector; grad_stride >= the row's length).
 * 3 L - 1 launches, 3 L with grad_in.  One kernel body serves this call and die_conv2d_wide_backward: for E = 1 row r is that
 * call's gradient on replica r's world, bit for bit; for E > 1 row c is the float64 sum over its E worlds, rounded once.  No float
 * atomics: the same inputs give the same bits on every run.
 *   Workspace (die_nca_wide_backward_batch_workspace_bytes; -1 for any stack or shape the call refuses), in floats:
 *   R * ceil(W / 16) * ceil(H / 64) * max_l(cout_l * cin_l * k_l^2)  +  min(L - 1, 2) * R * Cmax * W * H;
 * 16-byte aligned where H % 4 == 0 and L >= 2 (the planes come first in it).
 * Every argument is checked on the host before anything is launched, in die_nca_backward_batch's order with the wide limits.
 * DIE_PAD_REFLECT / DIE_PAD_REPLICATE: DIE_ERR_UNSUPPORTED.  DIE_ERR_ARG: null arguments, replicas outside
 * 1..DIE_MAX_REPLICAS, episodes not dividing R, a layer outside 1..32 channels or k not in {1, 3, 5}, a last layer that is not 3
 * planes of tanh, an unknown activation, sense_epoch out of range, strides below their minimum, `grad` equal to a layer's
 * weights, a short workspace, a bad `drop`, a grad_in that is not 16-byte aligned or whose stride is not a multiple of 4 where
 * H % 4 == 0, and grad_in overlapping any other buffer of the call. */
int64_t die_nca_wide_backward_batch_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca);
int die_nca_wide_backward_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                int64_t grad_in_stride, void* stream);

/* ---- Batched BPTT: the memory channels' adjoints for every replica of a die_batch (BatchedNeuralAutomataAgent.recurrent_action) --
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The batched twins of die_memory_cells / die_memory_planes_backward / die_gather_memory_backward: ONE launch each for all R
 * replicas, the replica in blockIdx.y (as die_memory_planes_batch / die_gather_memory_batch), the device bodies those of the
 * stand-alone kernels.  Records are [R][b->agent_stride] int32, replica r's row at r * b->agent_stride; memories and their
 * gradients are dense (R, M, row) arrays, row j of replica r at (r * memory_channels + j) * row_stride; planes are plane j of
 * replica r at r * replica_stride + j * plane_stride.
 *
 * die_memory_cells_batch — the record of every replica.  Replica r's slots start at r * b->agent_stride (slot order:
 * agents->slot must be NULL), its standing plane (die_stock_plane_batch at `epoch`) at standing + r * b->plane_stride.  For n <
 * b->n[r] the two words are die_memory_cells' of replica r; the padding slots n >= b->n[r] are written -1 in both arrays, so
 * the two adjoints never need n[] again.  Checked before the launch as die_memory_cells, and: a null batch, a slot array,
 * replicas outside 1..DIE_MAX_REPLICAS, agent_stride outside 1..DIE_OWNER_SLOT_MASK - 1, n[r] outside 0..agent_stride,
 * b->plane_stride < W * H. */
int die_memory_cells_batch(const die_medium* m, const die_agents* agents, const die_batch* b, const unsigned long long* standing,
                           int32_t epoch, int32_t* cell_out, int32_t* win_out, void* stream);
/* die_memory_planes_backward_batch — the expand's adjoint, a gather:
 *   grad_memory[r][j][id] = 0 <= win[r][id] < W * H ? grad_planes_r,j[win[r][id]] : +0.0f     for every id < b->agent_stride.
 * Every word of every row, padding included, is written exactly once; the values move as 32-bit words; no atomics.  With
 * `cell` for an index the same call is the read-out's forward through the record.  Checked as die_memory_planes_backward, and:
 * the die_batch as above, row_stride < agent_stride, and strides under which two of the R * M planes would share words: the
 * planes may lie replica-major (replica_stride >= (M - 1) * plane_stride + W * H: a sense gradient, a grad_in) or plane-major
 * (plane_stride >= (R - 1) * replica_stride + W * H: die_memory_planes_batch's layout). */
int die_memory_planes_backward_batch(int32_t W, int32_t H, int32_t memory_channels, const die_batch* b, const int32_t* win,
                                     const float* grad_planes, int64_t plane_stride, int64_t replica_stride, float* grad_memory,
                                     int64_t row_stride, void* stream);
/* die_gather_memory_backward_batch — the read-out's adjoint: the W * H cells of each of the R * M planes are cleared on `stream`
 * (the words between two planes and between two replicas are left alone), then ONE launch adds
 *   grad_planes_r,j[cell[r][id]] += grad_memory[r][j][id]     wherever 0 <= cell[r][id] < W * H; a zero term is skipped.
 * fp32 atomic adds, the stand-alone method: replica r has die_gather_memory_backward's bits wherever no cell holds more than two
 * alive slots with a non-zero gradient.  Checked before anything is cleared, as die_memory_planes_backward_batch with grad_planes
 * the output. */
int die_gather_memory_backward_batch(int32_t W, int32_t H, int32_t memory_channels, const die_batch* b, const int32_t* cell,
                                     const float* grad_memory, int64_t row_stride, float* grad_planes, int64_t plane_stride,
                                     int64_t replica_stride, void* stream);
/* die_nca_wide_sense_batch_store for a population whose agents carry memory: layer 0 reads ([agents,] food, chem, memory_0 ..
 * memory_{M-1}), `mem_planes` laid out as die_memory_planes_batch writes them (plane j of replica r at (j * R + r) *
 * b->plane_stride), and the last layer gives 3 + M planes; the tanh and the mask fall on all of them.  Checked as the parent, in
 * its order, with those channel counts, and: null mem_planes, memory_channels outside 1..DIE_MEMORY_MAX_CHANNELS, memory planes
 * that overlap the store or the masked planes. */
int die_nca_wide_sense_batch_store_memory(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store,
                                          int64_t store_bytes, float* masked, const die_nca_dropout* drop, const float* mem_planes,
                                          int32_t memory_channels, void* stream);
/* die_nca_wide_backward_batch for such a stack: grad_sense holds 3 + M planes per replica, layer 0's inputs include the memory
 * planes, and `grad_in`, when given, holds replica r's 2 + with_agent_channel + M planes in channel order — the caller takes the
 * chem plane for the env's chem node and the M memory planes for die_memory_planes_backward_batch.  The same two adjoint kernels
 * and the same float64 fold: 3 L - 1 launches, 3 L with grad_in; for E = 1 row r is bit for bit the stand-alone per-layer
 * die_conv2d_wide_backward gradients of replica r.  A population whose incoming memory has a graph always passes grad_in; with
 * neither that nor a chem node, NULL skips the kernel.  Checked as the parent, in its order; the byte query gives -1 for a
 * refused shape (the parent's query and call keep refusing a 3 + M stack). */
int64_t die_nca_wide_backward_batch_memory_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca,
                                                           int32_t memory_channels);
int die_nca_wide_backward_batch_memory(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                       const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                       const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                       int64_t grad_in_stride, const float* mem_planes, int32_t memory_channels, void* stream);

/* ---- Batched BPTT through the signal channels (BatchedNeuralAutomataAgent.signalling_action; die_signal_grad.hip) -------------
 * Added within ABI 24: new symbols only, no existing struct or call changes, so DIE_ABI_VERSION stays 24.
 * The batched twins of die_signal_cells / die_signal_step_backward and the signal-aware forms of the two calls above.
 *
 * die_signal_cells_batch — the record of all R replicas in ONE launch, the replica in blockIdx.y (as the batched memory
 * kernels), the device body that of die_signal_cells.  Replica r's standing plane (die_stock_plane_batch at `epoch`) at standing +
 * r * b->plane_stride, its byte plane at occupied_out + r * occupied_stride.  EVERY byte of every plane is written; the bytes
 * between two planes and beyond the last are left alone.  16-byte stores where both base pointers are 16-byte aligned,
 * b->plane_stride is even and occupied_stride % 16 == 0; single bytes elsewhere and on the tail.  Checked before the launch, in
 * order: die_signal_cells' checks (a null pointer, the batch included; W or H < 1; a decomposed medium: DIE_ERR_UNSUPPORTED; the
 * epoch), die_signal_step_batch's die_batch checks (replicas outside 1..DIE_MAX_REPLICAS, b->plane_stride < W * H, agent_stride
 * < 1, n[r] outside 0..agent_stride), occupied_stride < W * H, an output that overlaps the standing planes. */
int die_signal_cells_batch(const die_medium* m, const die_batch* b, const unsigned long long* standing, int32_t epoch,
                           uint8_t* occupied_out, int64_t occupied_stride, void* stream);
/* die_signal_step_backward_batch — die_signal_step_backward for all K * R planes in ONE launch (plane k of replica r is
 * blockIdx.z = k * R + r, the kernels those of the stand-alone call: with one replica it is that call).  Gradient plane k of
 * replica r at grad_field_next / grad_field + (k * R + r) * b->plane_stride (die_signal_step_batch's field layout); replica r's
 * mask at occupied + r * occupied_stride; its emission gradient's plane k at grad_emission + r * replica_stride + k *
 * plane_stride — replica-major (replica_stride >= (K - 1) * plane_stride + W * H: plane 3 of an (R, 3 + K + M, W, H)
 * sense-gradient buffer, whose other planes are left alone) or plane-major (plane_stride >= (R - 1) * replica_stride + W * H).
 * Either output may be null (its store is skipped, the other gets the same bits), not both.  EVERY cell of every output plane
 * is written, nothing between them; the inputs are only read.  The row-marching kernel runs where H % 4 == 0, the radius is at
 * most 4, every float pointer and stride is 16-byte aligned and `occupied` and occupied_stride 4-byte aligned; the LDS-tiled one
 * elsewhere.  Checked before the launch (DIE_ERR_ARG), in order: die_signal_step_backward's checks (a null b, occupied or
 * grad_field_next; both outputs null; size, K and the three constants), the die_batch checks above, occupied_stride < W * H, with
 * a grad_emission plane_stride < W * H and strides under which two of its K * R planes would share words, then every overlap
 * between an output and an input, the masks or the other output, each taken over its whole K * R span. */
int die_signal_step_backward_batch(int32_t W, int32_t H, const die_batch* b, const uint8_t* occupied, int64_t occupied_stride,
                                   int32_t signal_channels, const float* grad_field_next, float* grad_field, float* grad_emission,
                                   int64_t plane_stride, int64_t replica_stride, float deposit, float sigma, float decay, void* stream);
/* die_nca_wide_sense_batch_store_memory for a population whose agents also write a signal field: layer 0 reads ([agents,] food,
 * chem, signal_0 .., memory_0 ..), `signal_planes` laid out as die_signal_step_batch reads the field (plane k of replica r at
 * (k * R + r) * b->plane_stride), and the last layer gives 3 + K + M planes; the tanh and the mask fall on all of them.
 * memory_channels = 0 with null mem_planes is allowed: no memory.  The parent's L launches (L + 1 with a mask).  Checked as the
 * parent, in its order, with those channel counts, and: null signal_planes, memory_channels outside 0..DIE_MEMORY_MAX_CHANNELS or
 * not 0 exactly where mem_planes is null, signal_channels outside 1..DIE_SIGNAL_MAX_CHANNELS, memory or signal planes that
 * overlap the store or the masked planes. */
int die_nca_wide_sense_batch_store_signal(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store,
                                          int64_t store_bytes, float* masked, const die_nca_dropout* drop, const float* mem_planes,
                                          int32_t memory_channels, const float* signal_planes, int32_t signal_channels, void* stream);
/* die_nca_wide_backward_batch_memory for such a stack — the one host body and the same two adjoint kernels and float64 fold,
 * given the signal planes as further layer-0 inputs: grad_sense holds 3 + K + M planes per replica, and `grad_in`, when given,
 * replica r's 2 + with_agent_channel + K + M planes in channel order — the caller takes the chem plane for the env's chem node,
 * the K signal planes for the incoming field and the M memory planes for die_memory_planes_backward_batch.  3 L - 1 launches,
 * 3 L with grad_in.  Checked as the parent, in its order (memory_channels = 0 with null mem_planes allowed, signal_planes
 * required, grad_in against the signal planes too); the byte query gives -1 for a refused shape.  The two older entry points
 * keep refusing a stack with signal planes. */
int64_t die_nca_wide_backward_batch_signal_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca,
                                                           int32_t memory_channels, int32_t signal_channels);
int die_nca_wide_backward_batch_signal(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                       const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                       const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                       int64_t grad_in_stride, const float* mem_planes, int32_t memory_channels,
                                       const float* signal_planes, int32_t signal_channels, void* stream);

/* die_food_flow_batch on the replicas whose bit is set in replica_mask (bit r = replica r); the others' planes are not touched.
 * One launch: a row of workgroups per replica, those of unset replicas exit at once.  A full mask leaves exactly what
 * die_food_flow_batch leaves; an empty mask launches nothing.  Bits at or above b->replicas must be 0. */
int die_food_flow_batch_masked(const die_medium* m, const die_batch* b, int32_t kind, double t, double scale, double decay,
                               int32_t octaves, uint64_t seed, uint64_t replica_mask, void* stream);

/* ---- PGPE search over an (R, P) parameter matrix (die_search.hip; die_amd/search.py PGPE) ------------------------------
 * The training half of the reference's examples/learning_agents.py (evotorch's PGPE with symmetric sampling and centred
 * ranks).  R = replicas (even, 2..DIE_MAX_REPLICAS), n = R / 2 directions, P = parameters; the matrix is row-major fp32
 * (the `parameters` of a BatchedNeuralAutomataAgent).  All arithmetic is float64; the state lives in the caller's device
 * buffers below.  Neither call reads anything back to the host.
 *   sample: z(i, p) = sqrt(-2 ln u1) cos(2 pi u2), u1 = (w0 + 1) / 2^32, u2 = w1 / 2^32 from the first two words of
 *     Philox(counter = (i P + p, generation, DIE_STREAM_SEARCH), key = seed); eps = stdev[p] z; row 2i = fl32(center + eps),
 *     row 2i + 1 = fl32(center - eps).  One launch.
 *   update: f_r = sum over t ascending of terms[t stride_t + r stride_r] (the (T, R, 2) die_step_result words of T batched
 *     steps: stride_t = 2R, stride_r = 2); centred ranks u_r = k / (R - 1) - 0.5 (ascending, ties by replica index); the
 *     evaluated noise e(i, p) = row_2i[p] - center[p]; g_mu = (1/n) sum_i e (u_2i - u_2i+1) / 2,
 *     g_sigma = (1/n) sum_i ((u_2i + u_2i+1) / 2) (e^2 - sigma^2) / sigma; the centre takes a ClipUp or Adam ascent step on
 *     g_mu, sigma + stdev_lr g_sigma is clamped to [sigma (1 - d), sigma (1 + d)] and then to [stdev_min, stdev_max];
 *     pop_best = the row of the highest f (lowest index on ties), best = the best row ever (replaced on a strictly greater f);
 *     history row `generation` = (mean, max, min, median of f, |g_mu|, mean of the new sigma).  Three launches (Adam) or four
 *     (ClipUp); the two norms are fixed-tree reductions (no float atomics): the same bits on every run. */
#define DIE_PGPE_CLIPUP 0
#define DIE_PGPE_ADAM 1
#define DIE_PGPE_MAX_BLOCKS 256
#define DIE_PGPE_WORK_DOUBLES(P) (4 * DIE_PGPE_MAX_BLOCKS + (int64_t)(P))
typedef struct die_pgpe {
    int32_t replicas;            /* R: even, 2..DIE_MAX_REPLICAS */
    int32_t optimizer;           /* DIE_PGPE_CLIPUP / DIE_PGPE_ADAM */
    int64_t num_params;          /* P >= 1 */
    uint64_t seed;               /* Philox key of the sampling */
    double center_lr;            /* ClipUp step size alpha / Adam lr, > 0 */
    double stdev_lr;             /* > 0 */
    double max_speed, momentum;  /* ClipUp: > 0, [0, 1) */
    double beta1, beta2, eps;    /* Adam: [0, 1), [0, 1), > 0 */
    double stdev_max_change;     /* d; negative: no relative clamp */
    double stdev_min, stdev_max; /* absolute clamp (-inf / +inf: none) */
    float* center;               /* [P] */
    float* stdev;                /* [P] */
    float* opt_a;                /* [P] ClipUp velocity / Adam first moment */
    float* opt_b;                /* [P] Adam second moment (ClipUp: unused, may be NULL) */
    float* pop_best;             /* [P] */
    float* best;                 /* [P] */
    double* fitness;             /* [R] f of the last update */
    double* evals;               /* [2]: pop_best's f, best's f (set best's to -inf before the first update) */
    double* history;             /* [history_rows][6] */
    int64_t history_rows;        /* update needs generation < history_rows */
    double* work;                /* DIE_PGPE_WORK_DOUBLES(P) float64 scratch */
} die_pgpe;
int die_pgpe_sample(const die_pgpe* s, float* params, int64_t generation, void* stream);
int die_pgpe_update(const die_pgpe* s, const float* params, const double* terms, int64_t T, int64_t stride_t, int64_t stride_r,
                    int64_t generation, void* stream);
/* Episodes: candidate c of the C = s->replicas rows was evaluated on E = episodes worlds, replica c E + e its e-th, so `terms`
 * holds C E replicas (C E <= DIE_MAX_REPLICAS).  One more launch ahead of die_pgpe_update's (one wave, no atomics):
 *   F_r = sum over t ascending of terms[t stride_t + r stride_r], r < C E  ->  episode_fitness[r]   ((C, E) row-major doubles);
 *   f_c = (((0 + F_{cE}) + F_{cE+1}) + ... + F_{cE+E-1}) / E               ->  folded[c]            (C doubles).
 * Then exactly die_pgpe_update(s, params, folded, T = 1, 1, 1, generation): ranks, gradients, pop_best, best and the history
 * row are those of f_c.  Both buffers are the caller's device memory. */
int die_pgpe_update_episodes(const die_pgpe* s, const float* params, const double* terms, int64_t T, int64_t stride_t,
                             int64_t stride_r, int32_t episodes, double* episode_fitness, double* folded, int64_t generation,
                             void* stream);

/* ---- separable CMA-ES over an (R, P) parameter matrix (die_cmaes.hip; die_amd/search.py CMAES) -------------------------
 * The other searcher of the reference's examples/learning_agents.py (evotorch's CMAES(separable=True)): a diagonal
 * covariance, cumulative step-size control, rank-one and rank-mu updates, optional active (negative) weights.
 * lambda = R (2..DIE_MAX_REPLICAS, odd allowed), d = P, g = generation.  The state is float64 in the caller's device
 * buffers; sigma is a device scalar, double-buffered by parity: generation g reads sigma[g & 1], its update writes
 * sigma[(g + 1) & 1].  Neither call reads anything back to the host.
 *   sample: z(i, p) = sqrt(-2 ln u1) cos(2 pi u2), u1 = (w0 + 1) / 2^32, u2 = w1 / 2^32 from the first two words of
 *     Philox(counter = (i d + p, g, DIE_STREAM_CMAES), key = seed); row i = fl32(m_p + (sigma sqrt(C_p)) z(i, p)).  Not
 *     symmetric.  One launch.
 *   constants (the caller's, computed once on the host in float64 and stored below; die_amd/search.py cmaes_constants):
 *     w'_k = ln((lambda + 1) / 2) - ln k, k = 1..lambda; mu = floor(lambda / 2); w_k = w'_k / sum_{j<=mu} w'_j for k <= mu,
 *     mu_eff = 1 / sum_{k<=mu} w_k^2; mu_eff- = (sum w'-)^2 / sum (w'-)^2 over the k > mu (w'_k <= 0);
 *     c_sigma = r_sigma (mu_eff + 2) / (d + mu_eff + 5); d_sigma = r_damp (1 + 2 max(0, sqrt((mu_eff - 1) / (d + 1)) - 1) + c_sigma);
 *     c_c = r_c (1 + 1/d + mu_eff/d) / (sqrt(d) + 1/d + 2 mu_eff/d); c_1 = r_1 / (d + 2 sqrt(d) + mu_eff/d);
 *     c_mu = r_mu min(1 - c_1, (0.25 + mu_eff + 1/mu_eff - 2) / (d + 4 sqrt(d) + mu_eff/2));
 *     chi_d = sqrt(d) (1 - 1/(4d) + 1/(21 d^2)); for k > mu (active) w_k = w'_k min(a_mu, a_mueff, a_posdef) / sum |w'-| with
 *     a_mu = 1 + c_1/c_mu, a_mueff = 1 + 2 mu_eff- / (mu_eff + 2), a_posdef = (1 - c_1 - c_mu) / (d c_mu); not active: 0.
 *   update: f_r = sum over t ascending of terms[t stride_t + r stride_r] (the (T, R, 2) die_step_result words: stride_t = 2R,
 *     stride_r = 2); ranks k = 1..lambda by descending f, ties to the lower replica index; z_i is regenerated from the counter
 *     of generation g (nothing of sample is stored), y_i = sqrt(C_p) z_i.  In this order:
 *       y_w = sum_{k<=mu} w_k y_{k:lambda}, z_w likewise (summed best first);   m <- m + (c_m sigma) y_w;
 *       p_sigma <- (1 - c_sigma) p_sigma + sqrt(c_sigma (2 - c_sigma) mu_eff) z_w;
 *       h_sigma = [|p_sigma| / sqrt(1 - (1 - c_sigma)^(2(g + 1))) < (1.4 + 2/(d + 1)) chi_d];
 *       p_c <- (1 - c_c) p_c + h_sigma sqrt(c_c (2 - c_c) mu_eff) y_w;
 *       C_p <- (1 + c_1 (1 - h_sigma) c_c (2 - c_c) - c_1 - c_mu sum_k w_k) C_p + c_1 p_c,p^2 + c_mu sum_k w°_k y_{k:lambda,p}^2,
 *         w°_k = w_k (w_k >= 0), w_k d / |z_{k:lambda}|^2 (w_k < 0), y with the old C, summed best first;
 *       sigma <- sigma exp((c_sigma / d_sigma) (|p_sigma| / chi_d - 1)), or with csa_squared
 *       sigma <- sigma exp((c_sigma / (2 d_sigma)) (|p_sigma|^2 / d - 1)).
 *     pop_best = the row of rank 1, best = the best row ever (replaced on a strictly greater f); history row g = (mean, max,
 *     min, median of f, the new sigma, the mean over p of the new sigma sqrt(C_p)).  Four launches (rank, mean and paths,
 *     covariance and sigma, statistics); |p_sigma|^2 and the lambda |z_i|^2 are fixed-tree reductions (no float atomics):
 *     the same bits on every run.  `params` is the matrix the same generation's sample filled, read only for the two rows. */
#define DIE_CMAES_MAX_BLOCKS 256
#define DIE_CMAES_WORK_DOUBLES(R, P) ((4 + (int64_t)(R)) * DIE_CMAES_MAX_BLOCKS + (int64_t)(P))
typedef struct die_cmaes {
    int32_t replicas;                  /* lambda: 2..DIE_MAX_REPLICAS */
    int32_t csa_squared;               /* 0: sigma from |p_sigma| / chi_d; 1: from |p_sigma|^2 / d */
    int64_t num_params;                /* d >= 1 */
    uint64_t seed;                     /* Philox key of the sampling */
    double c_m;                        /* > 0 */
    double c_sigma, d_sigma;           /* (0, 1], > 0 */
    double c_c, c_1, c_mu;             /* (0, 1], >= 0, >= 0 with c_1 + c_mu <= 1 */
    double mu_eff, chi_d;              /* >= 1, > 0 */
    double weights[DIE_MAX_REPLICAS];  /* w_k of rank k + 1 (best first); w_1 > 0; entries lambda.. unused */
    double* center;                    /* m [d] */
    double* C;                         /* [d] diagonal covariance */
    double* p_sigma;                   /* [d] */
    double* p_c;                       /* [d] */
    double* sigma;                     /* [2] by generation parity */
    float* pop_best;                   /* [d] */
    float* best;                       /* [d] */
    double* fitness;                   /* [R] f of the last update */
    double* evals;                     /* [2]: pop_best's f, best's f (set best's to -inf before the first update) */
    double* history;                   /* [history_rows][6] */
    int64_t history_rows;              /* update needs generation < history_rows */
    double* work;                      /* DIE_CMAES_WORK_DOUBLES(R, P) float64 scratch */
} die_cmaes;
int die_cmaes_sample(const die_cmaes* s, float* params, int64_t generation, void* stream);
int die_cmaes_update(const die_cmaes* s, const float* params, const double* terms, int64_t T, int64_t stride_t, int64_t stride_r,
                     int64_t generation, void* stream);
/* die_pgpe_update_episodes' fold (lambda candidates x `episodes` replicas), then die_cmaes_update on the folded f_c. */
int die_cmaes_update_episodes(const die_cmaes* s, const float* params, const double* terms, int64_t T, int64_t stride_t,
                              int64_t stride_r, int32_t episodes, double* episode_fitness, double* folded, int64_t generation,
                              void* stream);

/* ---- message packing for decomposed worlds (die_amd/dist.py; no reference counterpart) ----------
 * A block [r0, r1) x [c0, c1) of a row-major plane (pitch in elements, 2/4/8-byte elements) copied
 * to / from byte offset buf_offset of one contiguous message buffer; up to 16 blocks per launch. */
typedef struct die_rect {
    void* plane;
    int32_t pitch, r0, r1, c0, c1, elem_bytes;
    int64_t buf_offset;
} die_rect;
int die_rects_pack(const die_rect* rects, int32_t n, void* buf, void* stream);
int die_rects_unpack(const die_rect* rects, int32_t n, const void* buf, void* stream);
/* buffer → plane with plane = max(plane, buffer) on unsigned 64-bit words: merges the claims a
 * neighbour's stray agents made on this rank's cells (guard-band decomposition). */
int die_rects_unpack_max(const die_rect* rects, int32_t n, const void* buf, void* stream);
/* Agent records: word (k, j) of the (n, count) int32 matrix is element idx[j] of array k (4-byte
 * arrays bit-copied, 1-byte arrays widened): migration packs leavers and writes arrivals with one
 * launch each. */
int die_records_gather(void* const* arrays, const int32_t* elem_bytes, int32_t n, const int64_t* idx, int64_t count,
                       int32_t* records_out, void* stream);
int die_records_scatter(void* const* arrays, const int32_t* elem_bytes, int32_t n, const int64_t* idx, int64_t count,
                        const int32_t* records_in, void* stream);

/* ---- Ghost-agent refresh (die_amd/dist.py DistEnv._refresh_ghosts; no reference counterpart) ----
 * die_ghost_plan classifies every local agent of a ghost-agent tile (die_medium.own_* set): agents standing on an
 * interior cell are owned; of those, the ones within the halo depth (own_x0 / own_y0 cells) of side
 * (dirs[2k], dirs[2k+1]) ∈ {-1,0,1}² are listed in lists[k] — their copies become that neighbour's ghosts; every
 * other agent (a ghost, or an agent that walked out) is listed in lists[n_dirs] (holes).  Lists hold ascending
 * 32-bit array indices (deterministic: count per block, scan, fill), at most caps[k] entries each;
 * totals[0..n_dirs) = full list lengths (may exceed caps: the caller checks), totals[n_dirs] = holes,
 * totals[n_dirs + 1] = owned agents.  ws: die_ghost_workspace_bytes(N) bytes of device memory. */
int64_t die_ghost_workspace_bytes(int64_t N);
int die_ghost_plan(const die_medium* medium, const die_agents* agents, int32_t n_dirs, const int8_t* dirs,
                   int32_t* const* lists, const int64_t* caps, int64_t* totals, void* ws, int64_t ws_bytes, void* stream);
/* die_records_gather with the count on the device: packs min(*count_dev, cap) records of the 32-bit index list into
 * the (n, cap) matrix of a message and writes the true count to header_out (may be NULL). */
int die_records_gather_dev(void* const* arrays, const int32_t* elem_bytes, int32_t n, const int32_t* idx,
                           const int64_t* count_dev, int64_t cap, int32_t* records_out, int64_t* header_out, void* stream);
/* die_records_scatter for a 32-bit index list and a record matrix with row pitch `pitch` >= count. */
int die_records_scatter_at(void* const* arrays, const int32_t* elem_bytes, int32_t n, const int32_t* idx, int64_t count,
                           int64_t pitch, const int32_t* records_in, void* stream);
/* The refresh without the host in the middle.  Message k of a buffer = [int64 count at hdr_off[k]] [(n_arrays, caps[k])
 * int32 record matrix at rec_off[k]] (field blocks follow: die_rects_pack).  die_ghost_pack fills every side's records
 * and header from the plan's lists / totals in ONE launch.  die_ghost_apply consumes a received buffer: arrival j (sides
 * in order) overwrites holes[j], or is appended behind n_local once the holes are used up; with fewer arrivals than
 * holes the kept entries of the cut tail move into the remaining holes (plan_ws = the workspace die_ghost_plan wrote
 * its membership words to).  `capacity` = entries each array holds: an arrival that would land at or beyond it is dropped,
 * never written (n_new_out[0] still reports the unclamped count, so the caller sees the overflow).  All counts are read on the device; n_new_out (3 + 2 * n_dirs words) receives what the host
 * wants afterwards: [new number of local agents, holes, owned, sent per side…, arrived per side… (raw headers)]. */
int die_ghost_pack(void* const* arrays, const int32_t* elem_bytes, int32_t n_arrays, int32_t n_dirs, int32_t* const* lists,
                   const int64_t* totals, const int64_t* caps, const int64_t* hdr_off, const int64_t* rec_off, void* send_buf,
                   void* stream);
int die_ghost_apply(void* const* arrays, const int32_t* elem_bytes, int32_t n_arrays, int32_t n_dirs, const int64_t* totals,
                    const int64_t* caps, const int64_t* hdr_off, const int64_t* rec_off, const void* recv_buf,
                    const int32_t* holes, const void* plan_ws, int64_t n_local, int64_t capacity, int64_t* n_new_out, void* stream);

/* A plain streaming copy of `bytes` (a multiple of 16; both buffers 16-byte aligned) device bytes, 16 bytes per lane: what bench.py
 * measures as this GPU's streaming ceiling (roofline.stream_ceiling_gbs), beside the 8 TB/s peak.  No reference counterpart. */
int die_stream_copy(const void* src, void* dst, int64_t bytes, void* stream);

/* Device-visible address of pinned host memory on `device` (-1: the current one), through the HIP runtime this library is linked
 * against (hipHostGetDevicePointer).  Env(sync=True) lets the step's last kernel write its three result words there. */
int die_host_device_pointer(void* host, int32_t device, void** dev_out);

#ifdef __cplusplus
}
#endif
#endif /* DIE_HIP_H */
