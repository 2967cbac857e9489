// PhysarumAgent populations (gfx950): the parameter rows of R candidates -> the table of kernel-ready rows that
// k_physarum_move_claim_batch (die_env.hip) and k_init_heading_batch (die_init.hip) read, one row per replica.
//
//   k_physarum_decode  one thread per replica: the six values (natural, or lo + (hi - lo)·clamp(u, 0, 1) in fp32), degrees to
//                      radians, and what die_fill_fwd_args (die_agents.hip) derives on the host for a stand-alone agent:
//                      atol = turn·rtol, x_turn (die_isclose_bound, the function the host runs), cos(x_turn),
//                      cos(sense).  With episodes E > 1 (die_physarum_decode_episodes) replica r decodes row r / E — the E
//                      replicas of a candidate get the same table row — and the first of them writes the candidate's values.
// One wave, a few hundred float64 operations: the launch is its whole cost.  tests/physarum_pop_model.py is its numpy twin.
#include "die_common.h"
#include <math.h>

namespace {

struct DecodeArgs {
    int R, unit;
    int E;                       // episodes: replica r decodes row r / E (1: a row per replica)
    die_parameter_space s;
};

__global__ __launch_bounds__(DIE_WAVE) void k_physarum_decode(DecodeArgs a, const float* __restrict__ rows, die_physarum_row* table,
                                                              float* values) {
    const int r = threadIdx.x;
    if (r >= a.R) return;
    const int c = r / a.E;
    const bool first = r == c * a.E;
    float v[DIE_PHYSARUM_PARAMS];
    for (int j = 0; j < DIE_PHYSARUM_PARAMS; ++j) {
        const float u = rows[c * DIE_PHYSARUM_PARAMS + j];
        if (a.unit) {
            // (one operation per statement: -ffp-contract=on must not fuse the product into the sum — the model rounds each)
            const float c = fminf(fmaxf(u, 0.f), 1.f);        // (fmaxf(NaN, 0) = 0)
            const float span = a.s.hi[j] - a.s.lo[j];
            const float t = span * c;
            v[j] = a.s.lo[j] + t;
        } else {
            v[j] = u;
        }
        if (first) values[c * DIE_PHYSARUM_PARAMS + j] = v[j];
    }
    const double deg = 3.141592653589793 / 180.0;             // math.radians' constant
    die_physarum_row o;
    o.scale = v[0]; o.deposit = v[1]; o.sense_offset = v[2];
    o.turn_radians = (double)v[3] * deg;
    o.sense_radians = (double)v[4] * deg;
    o.turn_tolerance = (double)v[5];
    o.atol = o.turn_radians * o.turn_tolerance;
    o.x_turn = die_isclose_bound(o.atol, 1e-2);
    const double pi = 3.141592653589793;
    o.c_turn = o.x_turn < 0.0 ? 2.f : (o.x_turn >= pi ? -2.f : (float)cos(o.x_turn));
    o.c_sense = o.sense_radians < 0.0 ? 2.f : (o.sense_radians >= pi ? -2.f : (float)cos(o.sense_radians));
    o.reserved = 0.f;
    table[r] = o;
}

}  // namespace

static_assert(sizeof(die_physarum_row) == 64, "die_physarum_row: one 64-byte scalar load");

static int decode_rows(const char* who, const float* rows, int32_t replicas, int32_t episodes, int32_t mode,
                       const die_parameter_space* space, die_physarum_row* table, float* values, void* stream) {
    DIE_REQUIRE(mode == DIE_PHYSARUM_NATURAL || mode == DIE_PHYSARUM_UNIT, "%s: mode %d: natural (0) or unit (1)", who, mode);
    DecodeArgs a{};
    a.R = replicas; a.E = episodes; a.unit = mode == DIE_PHYSARUM_UNIT;
    if (a.unit) {
        DIE_REQUIRE(space, "%s: unit mode needs a parameter space", who);
        a.s = *space;
        for (int j = 0; j < DIE_PHYSARUM_PARAMS; ++j) {
            const float lo = space->lo[j], hi = space->hi[j];
            DIE_REQUIRE(isfinite(lo) && isfinite(hi) && lo <= hi, "%s: column %d: bounds (%g, %g) must be finite with lo <= hi", who, j,
                        (double)lo, (double)hi);
            volatile float span = hi - lo;                        // the decoded value at u = 1, as the kernel rounds it
            volatile float top = lo + span;
            const float vmax = top;
            const bool angle = j == 3 || j == 4;
            DIE_REQUIRE(j == 1 || lo >= 0.f, "%s: column %d: lower bound %g is negative", who, j, (double)lo);
            DIE_REQUIRE(j != 3 || lo > 0.f, "%s: column 3: turn_angle must be positive (lower bound %g)", who, (double)lo);
            DIE_REQUIRE(!angle || vmax <= 180.f, "%s: column %d: an angle beyond 180 degrees (upper bound %g)", who, j, (double)hi);
        }
    }
    k_physarum_decode<<<1, DIE_WAVE, 0, (hipStream_t)stream>>>(a, rows, table, values);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_physarum_decode_batch(const float* rows, int32_t replicas, int32_t mode, const die_parameter_space* space,
                                         die_physarum_row* table, float* values, void* stream) {
    const char* who = "die_physarum_decode_batch";
    DIE_REQUIRE(rows && table && values, "%s: null rows, table or values", who);
    DIE_REQUIRE(replicas >= 1 && replicas <= DIE_MAX_REPLICAS, "%s: replicas %d: in 1..%d", who, replicas, DIE_MAX_REPLICAS);
    return decode_rows(who, rows, replicas, 1, mode, space, table, values, stream);
}

extern "C" int die_physarum_decode_episodes(const float* rows, int32_t candidates, int32_t episodes, int32_t mode,
                                            const die_parameter_space* space, die_physarum_row* table, float* values, void* stream) {
    const char* who = "die_physarum_decode_episodes";
    DIE_REQUIRE(rows && table && values, "%s: null rows, table or values", who);
    DIE_REQUIRE(episodes >= 1, "%s: episodes %d: at least 1", who, episodes);
    DIE_REQUIRE(candidates >= 1 && (int64_t)candidates * episodes <= DIE_MAX_REPLICAS, "%s: %d candidates x %d episodes: 1..%d replicas", who,
                candidates, episodes, DIE_MAX_REPLICAS);
    return decode_rows(who, rows, candidates * episodes, episodes, mode, space, table, values, stream);
}
