// DataInitializer on device (gfx950) — core/data_init.py:92-253 as used by Env._init_data
// (core/env.py:74-86) and the agent constructors (core/agent/gradient.py:42-43,163).
//
//   k_init_medium   with_agents(ratio) (:222-226) + synthetic with_food (:228-231) + zero chem
//   k_count / k_scan_blocks / k_scatter
//                   agents_from_medium (:133-150): stream compaction of the occupied cells in
//                   row-major order into slots [0, K) — three passes, 4096 cells per workgroup
//   k_init_heading  _get_some_noise → get_radians → discretize
// Every computation is one device body (init_cell, count_tile, scan_blocks, scatter_tile, zero_tail, init_heading_one, flow_wave_z /
// flow_perlin_z / flow_mix) that the stand-alone kernel and its batched twin (replica in blockIdx.y) both call.
#include "die_common.h"
#include "die_rng.h"

#define SCAN_ITEMS 16
#define SCAN_TILE (DIE_BLOCK * SCAN_ITEMS)

struct FoodArgs {
    int n_waves;
    float scale;
    int perlin_octaves;        // > 0: Perlin food, _mask(perlin(x·octaves, y·octaves).round(3), mask_above=threshold) (:228-231)
    float threshold;
    double fx[8], fy[8], phase[8], amp[8];
};

// _mask (core/data_init.py:181-185) of a value already rounded to 3 decimals
__device__ __forceinline__ double mask_range(double v, double below, double above) { return (below <= v && v <= above) ? v : 0.0; }

// food value of world cell (ix, iy): with_food_perlin (:228-231) on the linspace(0, 1, n) labels, or the sinusoid mix
__device__ __forceinline__ float init_food_value(const die_geo& g, const FoodArgs& fa, uint64_t seed, int ix, int iy) {
    if (fa.perlin_octaves > 0) {
        const double x = g.gW > 1 ? (double)ix / (double)(g.gW - 1) : 0.0, y = g.gH > 1 ? (double)iy / (double)(g.gH - 1) : 0.0;
        const double p = rint(die_perlin2(seed, x * fa.perlin_octaves, y * fa.perlin_octaves) * 1000.0) / 1000.0;
        return (float)mask_range(p, 0.0, (double)fa.threshold);
    }
    const double x = (double)ix / g.gW, y = (double)iy / g.gH;
    double s = 0.0;
    for (int k = 0; k < fa.n_waves; ++k)
        s += fa.amp[k] * sin(6.283185307179586476925 * (fa.fx[k] * x + fa.fy[k] * y) + fa.phase[k]);
    s = 2.0 * (double)fa.scale * s;
    s = s < 0.0 ? 0.0 : (s > (double)fa.scale ? (double)fa.scale : s);
    return (float)(rint(s * 1000.0) / 1000.0);   // .round(3) (:196)
}

// world cell (ix, iy) of element c of the planes of `g`: a decomposed tile's halo wraps around the world (a whole world: ix = c / H,
// iy = c % H, which TILE = false states without the division by the world size)
template <bool TILE>
__device__ __forceinline__ void world_cell(const die_geo& g, int64_t c, int& ix, int& iy) {
    const int lx = (int)(c / g.H), ly = (int)(c - (int64_t)lx * g.H);
    ix = lx; iy = ly;
    if (TILE) {
        ix = (lx + g.ox) % g.gW; iy = (ly + g.oy) % g.gH;
        ix = ix < 0 ? ix + g.gW : ix;
        iy = iy < 0 ? iy + g.gH : iy;
    }
}

// element c of the three planes of `g` under `seed`: the occupancy flag, the food value, zero chem
template <bool TILE, typename T>
__device__ __forceinline__ void init_cell(const die_geo& g, uint64_t* owner, T* food, T* chem, double ratio, uint64_t seed,
                                          const FoodArgs& fa, int64_t c) {
    int ix, iy;
    world_cell<TILE>(g, c, ix, iy);
    // ceil(u·[0 ≤ u ≤ ratio]) with u = random_sample().round(3): occupied iff 0 < u ≤ ratio
    const uint64_t gc = (uint64_t)ix * (uint64_t)g.gH + (uint64_t)iy;
    const int r = die_round3_units(die_draw(seed, 0, gc, DIE_STREAM_INIT_AGENTS).v[0]);
    const double u = r / 1000.0;
    owner[c] = (r > 0 && u <= ratio) ? 1ull : 0ull;    // provisional flag; scatter_tile writes the claim word
    die_st(food, c, init_food_value(g, fa, seed, ix, iy));
    die_st(chem, c, 0.f);
}

template <typename T>
__global__ __launch_bounds__(DIE_BLOCK) void k_init_medium(die_geo g, uint64_t* owner, T* food, T* chem, double ratio,
                                                           uint64_t seed, FoodArgs fa) {
    const int64_t C = (int64_t)g.W * g.H;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += stride) init_cell<true>(g, owner, food, chem, ratio, seed, fa, c);
}

// the occupied cells of scan tile blockIdx.x → block_sum[blockIdx.x]
__device__ __forceinline__ void count_tile(const uint64_t* flag, int64_t C, int32_t* block_sum) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) cnt += (base + i < C && flag[base + i] != 0) ? 1 : 0;
    __shared__ int s[DIE_BLOCK];
    s[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = DIE_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sum[blockIdx.x] = s[0];
}

// one workgroup: exclusive scan of nb block sums → block_off (int64); total[0] = min(K, capacity); total[1], the overflow word
// (more agents than slots), is assigned 0 / 1, or with STICKY only ever set (|= 1 on overflow, never cleared here)
template <bool STICKY>
__device__ __forceinline__ void scan_blocks(const int32_t* block_sum, int nb, int64_t* block_off, int64_t* total, int64_t capacity) {
    __shared__ long long s[DIE_BLOCK];
    const int per = (nb + DIE_BLOCK - 1) / DIE_BLOCK;
    const int lo = threadIdx.x * per, hi = min(lo + per, nb);
    long long t = 0;
    for (int i = lo; i < hi; ++i) t += block_sum[i];
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < DIE_BLOCK; ++i) { long long v = s[i]; s[i] = run; run += v; }
        total[0] = run < capacity ? run : capacity;
        if (STICKY) { if (run > capacity) total[1] |= 1; }
        else total[1] = run > capacity ? 1 : 0;
    }
    __syncthreads();
    long long run = s[threadIdx.x];
    for (int i = lo; i < hi; ++i) { block_off[i] = run; run += block_sum[i]; }
}

// the occupied cells of scan tile blockIdx.x, in row-major order, into slots block_off[blockIdx.x] … (below N: the rest are clipped)
// (the geometry by value: through a reference the compiler converts W − 1 and gH − 1 to double once per cell, not once)
template <bool TILE>
__device__ __forceinline__ void scatter_tile(const die_geo g, uint64_t* owner, const int64_t* block_off, int64_t N, uint32_t* x,
                                             uint32_t* y, uint8_t* alive, float* agent_food, uint64_t seed) {
    const int H = g.H, W = g.gW;             // labels are world coordinates: linspace(0, 1, gW)
    const int64_t C = (int64_t)g.W * g.H;
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int flags = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < C && owner[base + i] != 0) { flags |= 1 << i; ++cnt; }
    __shared__ int s[DIE_BLOCK];
    s[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 1; o < DIE_BLOCK; o <<= 1) {          // Hillis–Steele inclusive scan
        int v = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    int64_t k = block_off[blockIdx.x] + (s[threadIdx.x] - cnt);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const int64_t c = base + i;
        if (c >= C) break;
        if (flags & (1 << i)) {
            if (k < N) {
                const int lx = (int)(c / H), ly = (int)(c - (int64_t)lx * H);
                const int ix = TILE ? lx + g.ox : lx, iy = TILE ? ly + g.oy : ly;
                // x = linspace(0, 1, W)[ix] in Q0.32; the last label 1.0 is held as 2^32 − 1
                const double qx = W > 1 ? (double)ix / (double)(W - 1) * 4294967296.0 : 0.0;
                const double qy = g.gH > 1 ? (double)iy / (double)(g.gH - 1) * 4294967296.0 : 0.0;
                const long long X = __double2ll_rn(qx), Y = __double2ll_rn(qy);
                x[k] = (uint32_t)(X > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : X);
                y[k] = (uint32_t)(Y > 0xFFFFFFFFLL ? 0xFFFFFFFFLL : Y);
                alive[k] = 1;
                // get_random(K, 0.1, 1.0) = 0.9·u.round(3) + 0.1 (:140, :168-169)
                const int r = die_round3_units(die_draw(seed, 0, (uint64_t)k, DIE_STREAM_INIT_AGENT_FOOD).v[0]);
                agent_food[k] = (float)(0.9 * (r / 1000.0) + 0.1);
                owner[c] = die_claim(1, k, 0.f);
            } else {
                owner[c] = 0;
            }
            ++k;
        }
    }
}

// slots K … N − 1: nobody.  (The caller's thread index and grid stride come as arguments: blockDim read in a device function
// compiles to the form that allows a partial last workgroup, one more load at the head of the kernel.)
__device__ __forceinline__ void zero_tail(int64_t K, int64_t N, int64_t thread, int64_t stride, uint32_t* x, uint32_t* y, uint8_t* alive,
                                          float* agent_food) {
    for (int64_t n = K + thread; n < N; n += stride) {
        x[n] = 0; y[n] = 0; alive[n] = 0; agent_food[n] = 0.f;
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_count(const uint64_t* flag, int64_t C, int32_t* block_sum) { count_tile(flag, C, block_sum); }

__global__ __launch_bounds__(DIE_BLOCK) void k_scan_blocks(const int32_t* block_sum, int nb, int64_t* block_off,
                                                            int64_t* total, int64_t capacity) {
    scan_blocks<false>(block_sum, nb, block_off, total, capacity);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_scatter(die_geo g, uint64_t* owner, const int64_t* block_off, int64_t N,
                                                       uint32_t* x, uint32_t* y, uint8_t* alive, float* agent_food,
                                                       uint64_t seed) {
    scatter_tile<true>(g, owner, block_off, N, x, y, alive, agent_food, seed);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_zero_tail(const int64_t* total, int64_t N, uint32_t* x, uint32_t* y,
                                                         uint8_t* alive, float* agent_food) {
    zero_tail(total[0], N, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, x, y, alive, agent_food);
}

// slot n's heading under `seed`: the float64 state (hi, lo words) and the Box–Muller pair (gx, gy) behind it
__device__ __forceinline__ void init_heading_one(uint64_t seed, int64_t n, double turn, uint32_t* hi, uint32_t* lo, float* pgx, float* pgy) {
    const die_u32x4 r = die_draw(seed, 0, (uint64_t)n, DIE_STREAM_INIT_HEADING);
    // Box–Muller pair: its polar angle is 2π·u2, wrapped to (−π, π] like np.angle
    const double u1 = ((double)r.v[0] + 1.0) * (1.0 / 4294967296.0);
    const double u2 = (double)r.v[1] * (1.0 / 4294967296.0);
    const double rad = 0.4 * sqrt(-2.0 * log(u1));
    const double gx = rad * cos(6.283185307179586476925 * u2), gy = rad * sin(6.283185307179586476925 * u2);
    double ang = atan2(gy, gx);
    if (turn > 0.0) ang = floor(ang / turn) * turn;      // discretize (core/utils.py:183-184)
    const double h = (double)(float)ang;                 // float64 state holding the fp32 rounding of the lattice angle
    *hi = (uint32_t)__double2hiint(h);
    *lo = (uint32_t)__double2loint(h);
    *pgx = (float)gx; *pgy = (float)gy;
}

__global__ __launch_bounds__(DIE_BLOCK) void k_init_heading(uint32_t* hhi, uint32_t* hlo, float* pgx, float* pgy, int64_t N, double turn,
                                                            uint64_t seed) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
        float gx, gy;
        init_heading_one(seed, n, turn, &hhi[n], &hlo[n], &gx, &gy);
        if (pgx) { pgx[n] = gx; pgy[n] = gy; }
    }
}

// k_init_heading of every replica of a PhysarumAgent population (blockIdx.y = replica): replica r's n[r] slots lie r agent
// strides further, its key is seed + r·seed_stride, its lattice the turn angle of its own table row
struct HeadingBatchArgs {
    int64_t agents;
    uint64_t seed, seed_stride;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_init_heading_batch(uint32_t* hhi, uint32_t* hlo, HeadingBatchArgs b,
                                                                  const die_physarum_row* __restrict__ table) {
    const int r = blockIdx.y;
    const int64_t N = b.n[r];
    const double turn = table[r].turn_radians;
    const uint64_t seed = b.seed + b.seed_stride * (uint64_t)r;
    hhi += b.agents * r; hlo += b.agents * r;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
        float gx, gy;                                    // (a population keeps no previous gradient: the pair is dropped)
        init_heading_one(seed, n, turn, &hhi[n], &hlo[n], &gx, &gy);
    }
}

static int init_grid(int64_t n) {
    int64_t g = (n + DIE_BLOCK - 1) / DIE_BLOCK;
    return (int)(g < 8192 ? (g > 0 ? g : 1) : 8192);
}

// the kernels' copy of a die_food_spec whose n_waves the caller has checked (both callers check it ahead of other arguments)
static int food_args_of(const char* who, const die_food_spec* food, FoodArgs* fa) {
    DIE_REQUIRE(food->perlin_octaves >= 0 && food->perlin_octaves < (1 << 19), "%s: bad perlin_octaves %d", who, food->perlin_octaves);
    fa->n_waves = food->n_waves;
    fa->scale = food->scale;
    fa->perlin_octaves = food->perlin_octaves;
    fa->threshold = food->threshold;
    for (int i = 0; i < 8; ++i) { fa->fx[i] = food->fx[i]; fa->fy[i] = food->fy[i]; fa->phase[i] = food->phase[i]; fa->amp[i] = food->amp[i]; }
    return DIE_OK;
}

int64_t die_ws_scan_bytes(int32_t W, int32_t H) {
    const int64_t nb = ((int64_t)W * H + SCAN_TILE - 1) / SCAN_TILE;
    return ((nb * 4 + 255) & ~(int64_t)255) + ((nb * 8 + 255) & ~(int64_t)255);
}

extern "C" int die_init_medium(const die_medium* m, double agent_ratio, uint64_t seed, const die_food_spec* food,
                               void* stream) {
    DIE_REQUIRE(m && food, "die_init_medium: null argument");
    DIE_REQUIRE(m->W >= 1 && m->H >= 1 && m->owner && m->food && m->chem, "die_init_medium: bad medium");
    DIE_REQUIRE(food->n_waves >= 0 && food->n_waves <= 8, "die_init_medium: n_waves %d outside 0..8", food->n_waves);
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "die_init_medium: bad dtype %d", m->dtype);
    FoodArgs fa;
    const int rc = food_args_of("die_init_medium", food, &fa);
    if (rc != DIE_OK) return rc;
    const int grid = init_grid((int64_t)m->W * m->H);
    if (m->dtype == DIE_F32)
        k_init_medium<float><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(die_geo_of(m), m->owner, (float*)m->food,
                                                                           (float*)m->chem, agent_ratio, seed, fa);
    else
        k_init_medium<__half><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(die_geo_of(m), m->owner, (__half*)m->food,
                                                                            (__half*)m->chem, agent_ratio, seed, fa);
    DIE_CHECK_LAUNCH("die_init_medium");
    return DIE_OK;
}

extern "C" int die_init_agents(const die_medium* m, const die_agents* a, uint64_t seed, int64_t* num_alive_dev, void* ws,
                               int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(m && a && num_alive_dev && ws, "die_init_agents: null argument");
    DIE_REQUIRE(m->W >= 1 && m->H >= 1 && m->owner, "die_init_agents: bad medium");
    DIE_REQUIRE(a->N > 0 && a->x && a->y && a->alive && a->agent_food, "die_init_agents: bad agents");
    DIE_REQUIRE(ws_bytes >= die_workspace_bytes(m->W, m->H, a->N), "die_init_agents: workspace too small");
    const int64_t C = (int64_t)m->W * m->H;
    const int64_t nb = (C + SCAN_TILE - 1) / SCAN_TILE;
    DIE_REQUIRE(nb < (1ll << 31), "die_init_agents: field too large");
    char* w = (char*)ws + (int64_t)8192 * 8 * 3;        // after the step partials (die_env.hip WS_PARTS)
    int32_t* block_sum = (int32_t*)w;
    int64_t* block_off = (int64_t*)(w + ((nb * 4 + 255) & ~(int64_t)255));
    hipStream_t s = (hipStream_t)stream;
    k_count<<<(int)nb, DIE_BLOCK, 0, s>>>(m->owner, C, block_sum);
    k_scan_blocks<<<1, DIE_BLOCK, 0, s>>>(block_sum, (int)nb, block_off, num_alive_dev, a->N);
    k_scatter<<<(int)nb, DIE_BLOCK, 0, s>>>(die_geo_of(m), m->owner, block_off, a->N, a->x, a->y, a->alive, a->agent_food, seed);
    k_zero_tail<<<init_grid(a->N), DIE_BLOCK, 0, s>>>(num_alive_dev, a->N, a->x, a->y, a->alive, a->agent_food);
    DIE_CHECK_LAUNCH("die_init_agents");
    return DIE_OK;
}

extern "C" int die_init_heading(uint32_t* heading_hi, uint32_t* heading_lo, float* prev_gx, float* prev_gy, int64_t N, double turn_radians,
                                uint64_t seed, void* stream) {
    DIE_REQUIRE(heading_hi && heading_lo && N > 0, "die_init_heading: bad arguments");
    DIE_REQUIRE((prev_gx == nullptr) == (prev_gy == nullptr), "die_init_heading: prev_gx/prev_gy must come together");
    k_init_heading<<<init_grid(N), DIE_BLOCK, 0, (hipStream_t)stream>>>(heading_hi, heading_lo, prev_gx, prev_gy, N, turn_radians,
                                                                          seed);
    DIE_CHECK_LAUNCH("die_init_heading");
    return DIE_OK;
}

extern "C" int die_physarum_heading_batch(uint32_t* heading_hi, uint32_t* heading_lo, const die_batch* b, const die_physarum_row* table,
                                          uint64_t seed, void* stream) {
    const char* who = "die_physarum_heading_batch";
    DIE_REQUIRE(heading_hi && heading_lo && b && table, "%s: null argument", who);
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas", who, DIE_MAX_REPLICAS);
    DIE_REQUIRE(b->agent_stride >= 1, "%s: bad agent stride %lld", who, (long long)b->agent_stride);
    HeadingBatchArgs k;
    k.agents = b->agent_stride; k.seed = seed; k.seed_stride = b->seed_stride;
    int64_t nmax = 0;
    for (int r = 0; r < DIE_MAX_REPLICAS; ++r) {
        k.n[r] = r < b->replicas ? b->n[r] : 0;
        DIE_REQUIRE(r >= b->replicas || (b->n[r] >= 1 && b->n[r] <= b->agent_stride), "%s: replica %d has %lld agents", who, r, (long long)b->n[r]);
        if (k.n[r] > nmax) nmax = k.n[r];
    }
    k_init_heading_batch<<<dim3(init_grid(nmax), b->replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(heading_hi, heading_lo, k, table);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the worlds of every replica of a die_batch (BatchedEnv.reset(seed=...) / reset(seeds=...)) ------------------------
// Replica r (blockIdx.y) is die_init_medium + die_init_agents of seed[r] on its own planes and agent arrays (die_init_batch:
// seed + r·world_stride, worked out on the host; die_init_batch_seeds: the caller's list, passed by value):
// the kernels below hand init_cell / count_tile / scan_blocks / scatter_tile / zero_tail the replica's pointers (a replica's
// plane is a whole world: no tile offsets).  The scan workspace of replica r is its own die_ws_scan_bytes slice.
struct InitBatchArgs {
    int64_t cells, agents;          // strides: cells per plane, agent slots per replica
    uint64_t seed[DIE_MAX_REPLICAS];    // the world of every replica
    int64_t ws_stride;              // bytes of scan workspace per replica
    int64_t nb;                     // scan tiles per plane
    int64_t n[DIE_MAX_REPLICAS];    // slots of every replica
};

// the block sums and the block offsets in replica r's slice of the scan workspace
__device__ __forceinline__ int32_t* ws_block_sum(char* ws, const InitBatchArgs& b, int r) { return (int32_t*)(ws + b.ws_stride * r); }
__device__ __forceinline__ int64_t* ws_block_off(char* ws, const InitBatchArgs& b, int r) {
    return (int64_t*)(ws + b.ws_stride * r + ((b.nb * 4 + 255) & ~(int64_t)255));
}

template <typename T>
__global__ __launch_bounds__(DIE_BLOCK) void k_init_medium_batch(die_geo g, uint64_t* owner, T* food, T* chem, double ratio,
                                                                 FoodArgs fa, InitBatchArgs b) {
    const int r = blockIdx.y;
    const uint64_t sr = b.seed[r];
    owner += b.cells * r; food += b.cells * r; chem += b.cells * r;
    const int64_t C = (int64_t)g.W * g.H;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += stride) init_cell<false>(g, owner, food, chem, ratio, sr, fa, c);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_count_batch(const uint64_t* flag, int64_t C, char* ws, InitBatchArgs b) {
    const int r = blockIdx.y;
    count_tile(flag + b.cells * r, C, ws_block_sum(ws, b, r));
}

// one workgroup per replica: counts[2r] = min(K_r, n[r]), counts[2r + 1] |= 1 when K_r > n[r] (never cleared here)
__global__ __launch_bounds__(DIE_BLOCK) void k_scan_blocks_batch(char* ws, int64_t* counts, InitBatchArgs b) {
    const int r = blockIdx.y;
    scan_blocks<true>(ws_block_sum(ws, b, r), (int)b.nb, ws_block_off(ws, b, r), counts + 2 * r, b.n[r]);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_scatter_batch(die_geo g, uint64_t* owner, const char* ws, uint32_t* x, uint32_t* y,
                                                             uint8_t* alive, float* agent_food, InitBatchArgs b) {
    const int r = blockIdx.y;
    const int64_t pa = b.agents * r;
    scatter_tile<false>(g, owner + b.cells * r, ws_block_off((char*)ws, b, r), b.n[r], x + pa, y + pa, alive + pa, agent_food + pa, b.seed[r]);   // (read only)
}

__global__ __launch_bounds__(DIE_BLOCK) void k_zero_tail_batch(const int64_t* counts, uint32_t* x, uint32_t* y, uint8_t* alive,
                                                               float* agent_food, InitBatchArgs b) {
    const int r = blockIdx.y;
    const int64_t pa = b.agents * r;
    zero_tail(counts[2 * r], b.n[r], (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, x + pa, y + pa, alive + pa,
              agent_food + pa);
}

extern "C" int64_t die_init_batch_workspace_bytes(int32_t W, int32_t H, int32_t replicas) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS) return -1;
    if (((int64_t)W * H + SCAN_TILE - 1) / SCAN_TILE >= (1ll << 31)) return -1;
    return (int64_t)replicas * die_ws_scan_bytes(W, H);
}

// both entry points: `seeds` is NULL for die_init_batch (seed + r·world_stride), else the n_seeds worlds of die_init_batch_seeds
static int init_batch(const char* who, const die_medium* m, const die_agents* a, const die_batch* b, double agent_ratio, uint64_t seed,
                      uint64_t world_stride, const uint64_t* seeds, int32_t n_seeds, const die_food_spec* food, int64_t* counts_dev,
                      void* ws, int64_t ws_bytes, void* stream) {
    DIE_REQUIRE(m && a && b && food && counts_dev && ws, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1 && m->owner && m->food && m->chem, "%s: bad medium", who);
    DIE_REQUIRE(m->gW <= 0, "%s: a replica's plane is a whole world, not a tile", who);
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad dtype %d", who, m->dtype);
    DIE_REQUIRE(a->N > 0 && a->x && a->y && a->alive && a->agent_food, "%s: bad agents", who);
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: %d replicas, 1..%d expected", who, b->replicas, DIE_MAX_REPLICAS);
    DIE_REQUIRE(b->plane_stride >= (int64_t)m->W * m->H && b->agent_stride >= a->N, "%s: strides smaller than a replica", who);
    DIE_REQUIRE(b->agent_stride <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: agent stride %lld too large for the ownership word", who,
                (long long)b->agent_stride);
    for (int r = 0; r < b->replicas; ++r)
        DIE_REQUIRE(b->n[r] >= 1 && b->n[r] <= b->agent_stride, "%s: replica %d has %lld slots, 1..%lld expected", who, r,
                    (long long)b->n[r], (long long)b->agent_stride);
    DIE_REQUIRE(food->n_waves >= 0 && food->n_waves <= 8, "%s: n_waves %d outside 0..8", who, food->n_waves);
    FoodArgs fa;
    const int rc = food_args_of(who, food, &fa);
    if (rc != DIE_OK) return rc;
    // the sinusoid mix is drawn from the seed on the host: one spec is the food of one seed only
    DIE_REQUIRE(food->perlin_octaves > 0 || world_stride == 0, "%s: a wave-mix food spec (perlin_octaves 0) with world_stride %llu: "
                "its waves belong to one seed", who, (unsigned long long)world_stride);
    if (seeds) {
        DIE_REQUIRE(n_seeds == b->replicas, "%s: %d seeds for %d replicas", who, n_seeds, b->replicas);
        for (int r = 1; r < n_seeds; ++r)
            DIE_REQUIRE(food->perlin_octaves > 0 || seeds[r] == seeds[0], "%s: a wave-mix food spec (perlin_octaves 0) with differing "
                        "seeds (replica %d): its waves belong to one seed", who, r);
    }
    const int64_t need = die_init_batch_workspace_bytes(m->W, m->H, b->replicas);
    DIE_REQUIRE(need > 0, "%s: field too large", who);
    DIE_REQUIRE(ws_bytes >= need, "%s: workspace too small (%lld < %lld: die_init_batch_workspace_bytes)", who, (long long)ws_bytes,
                (long long)need);
    const int64_t C = (int64_t)m->W * m->H;
    InitBatchArgs ib;
    ib.cells = b->plane_stride; ib.agents = b->agent_stride;
    for (int r = 0; r < DIE_MAX_REPLICAS; ++r)
        ib.seed[r] = r >= b->replicas ? 0 : seeds ? seeds[r] : seed + (uint64_t)r * world_stride;
    ib.ws_stride = die_ws_scan_bytes(m->W, m->H);
    ib.nb = (C + SCAN_TILE - 1) / SCAN_TILE;
    const int64_t nmax = die_replica_counts(ib.n, b->n, b->replicas);
    const die_geo g = die_geo_of(m);
    const hipStream_t s = (hipStream_t)stream;
    const int R = b->replicas;
    char* w = (char*)ws;
    const dim3 cells(init_grid(C), R), tiles((unsigned)ib.nb, R), slots(init_grid(nmax), R);
    if (m->dtype == DIE_F32)
        k_init_medium_batch<float><<<cells, DIE_BLOCK, 0, s>>>(g, m->owner, (float*)m->food, (float*)m->chem, agent_ratio, fa, ib);
    else
        k_init_medium_batch<__half><<<cells, DIE_BLOCK, 0, s>>>(g, m->owner, (__half*)m->food, (__half*)m->chem, agent_ratio, fa, ib);
    k_count_batch<<<tiles, DIE_BLOCK, 0, s>>>(m->owner, C, w, ib);
    k_scan_blocks_batch<<<dim3(1, R), DIE_BLOCK, 0, s>>>(w, counts_dev, ib);
    k_scatter_batch<<<tiles, DIE_BLOCK, 0, s>>>(g, m->owner, w, a->x, a->y, a->alive, a->agent_food, ib);
    k_zero_tail_batch<<<slots, DIE_BLOCK, 0, s>>>(counts_dev, a->x, a->y, a->alive, a->agent_food, ib);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_init_batch(const die_medium* m, const die_agents* a, const die_batch* b, double agent_ratio, uint64_t seed,
                              uint64_t world_stride, const die_food_spec* food, int64_t* counts_dev, void* ws, int64_t ws_bytes,
                              void* stream) {
    return init_batch("die_init_batch", m, a, b, agent_ratio, seed, world_stride, nullptr, 0, food, counts_dev, ws, ws_bytes, stream);
}

extern "C" int die_init_batch_seeds(const die_medium* m, const die_agents* a, const die_batch* b, double agent_ratio,
                                    const uint64_t* seeds, int32_t n_seeds, const die_food_spec* food, int64_t* counts_dev, void* ws,
                                    int64_t ws_bytes, void* stream) {
    const char* who = "die_init_batch_seeds";
    DIE_REQUIRE(seeds, "%s: null seed list", who);
    DIE_REQUIRE(n_seeds >= 1 && n_seeds <= DIE_MAX_REPLICAS, "%s: %d seeds, 1..%d expected (one per replica)", who, n_seeds,
                DIE_MAX_REPLICAS);
    return init_batch(who, m, a, b, agent_ratio, 0, 0, seeds, n_seeds, food, counts_dev, ws, ws_bytes, stream);
}

// ---- food flow: WaveSequence.get_flow_operator (core/data_init.py:29-38,71-89) --------------------------------
// food ← scale·z(x, y, t) + (1 − decay)·food with the reference's running-wave field z; x varies along the last
// axis and y along the first (core/utils.py:113-118 builds the grid from the reversed sizes).  float64 arithmetic,
// one rounding to the field dtype.  Tiles evaluate z at their world cells.
// (gi, gj): the world cell's index along the first (W) and the second (H) axis
__device__ __forceinline__ double flow_wave_z(int gi, int gj, int gW, int gH, double t) {
    const double pi = 3.141592653589793;
    // np.linspace(0, 1, n)[k] = k·(1/(n−1)); then (v − 0.5)·2
    const double x = ((double)gj * (1.0 / (double)(gH - 1)) - 0.5) * 2.0;
    const double y = ((double)gi * (1.0 / (double)(gW - 1)) - 0.5) * 2.0;
    const double r = sqrt(x * x + y * y);
    const double rwave = r + cos(pi * x) + sin(0.4 * pi * y);
    const double z_waves = cos(1.0 * pi * (rwave + t));
    const double z_islands = sin(pi * x * 3.0 + t) + cos(pi * y * 3.0 + t);
    return (1.0 - 0.25) * z_waves + 0.25 * z_islands;
}

// the update of one cell holding v, in every flow kernel: one expression, so one rounding
__device__ __forceinline__ float flow_mix(double scale, double z, double keep, float v) { return (float)(scale * z + keep * (double)v); }

template <typename T>
__global__ __launch_bounds__(DIE_BLOCK) void k_food_flow_wave(T* food, die_geo g, double t, double scale, double keep) {
    const int64_t total = (int64_t)g.W * g.H;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int gi, gj;
        world_cell<true>(g, i, gi, gj);
        die_st(food, i, flow_mix(scale, flow_wave_z(gi, gj, g.gW, g.gH, t), keep, die_ld(food, i)));
    }
}

extern "C" int die_food_flow_wave(const die_medium* m, double t, double scale, double decay, void* stream) {
    DIE_REQUIRE(m && m->food && m->W >= 1 && m->H >= 1, "die_food_flow_wave: bad medium");
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "die_food_flow_wave: bad field dtype %d", m->dtype);
    const die_geo g = die_geo_of(m);
    DIE_REQUIRE(g.gW >= 2 && g.gH >= 2, "die_food_flow_wave: the world must be at least 2x2");
    const int64_t total = (int64_t)m->W * m->H;
    const int grid = init_grid(total);
    if (m->dtype == DIE_F32) k_food_flow_wave<float><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>((float*)m->food, g, t, scale, 1.0 - decay);
    else k_food_flow_wave<__half><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>((__half*)m->food, g, t, scale, 1.0 - decay);
    DIE_CHECK_LAUNCH("die_food_flow_wave");
    return DIE_OK;
}


// PerlinNoiseSequence.__getitem__ (core/data_init.py:55-69) inside FieldSequence.get_flow_operator (:29-38):
// food ← scale · round(noise((x, y, t)), 3) + (1 − decay) · food with x, y the linspace(0, 1, n) labels of the world cell and
// `noise` the 3-D gradient noise at (x, y, t) · octaves.
// (flatten: die_perlin3 is inlined here; called, it costs 32 B of scratch per lane)
__device__ __forceinline__ __attribute__((flatten)) double flow_perlin_z(int gi, int gj, int gW, int gH, double t, double octaves, uint64_t seed) {
    const double x = (double)gi / (double)(gW - 1), y = (double)gj / (double)(gH - 1);
    return rint(die_perlin3(seed, x * octaves, y * octaves, t * octaves) * 1000.0) / 1000.0;
}

template <typename T>
__global__ __launch_bounds__(DIE_BLOCK) void k_food_flow_perlin(T* food, die_geo g, double t, double octaves, double scale, double keep, uint64_t seed) {
    const int64_t total = (int64_t)g.W * g.H;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int gi, gj;
        world_cell<true>(g, i, gi, gj);
        die_st(food, i, flow_mix(scale, flow_perlin_z(gi, gj, g.gW, g.gH, t, octaves, seed), keep, die_ld(food, i)));
    }
}

extern "C" int die_food_flow_perlin(const die_medium* m, double t, int32_t octaves, double scale, double decay, uint64_t seed, void* stream) {
    DIE_REQUIRE(m && m->food && m->W >= 1 && m->H >= 1, "die_food_flow_perlin: bad medium");
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "die_food_flow_perlin: bad field dtype %d", m->dtype);
    DIE_REQUIRE(octaves >= 1, "die_food_flow_perlin: octaves %d", octaves);
    const die_geo g = die_geo_of(m);
    DIE_REQUIRE(g.gW >= 2 && g.gH >= 2, "die_food_flow_perlin: the world must be at least 2x2");
    const int64_t total = (int64_t)m->W * m->H;
    const int grid = init_grid(total);
    if (m->dtype == DIE_F32) k_food_flow_perlin<float><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>((float*)m->food, g, t, (double)octaves, scale, 1.0 - decay, seed);
    else k_food_flow_perlin<__half><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>((__half*)m->food, g, t, (double)octaves, scale, 1.0 - decay, seed);
    DIE_CHECK_LAUNCH("die_food_flow_perlin");
    return DIE_OK;
}

// ---- food flow on the replicas of a die_batch ----------------------------------------------------------------------
// The field z(x, y, t) is the same for every replica (same world, same t, same seed); only the food planes differ.  One
// thread per cell evaluates z once and updates that cell in every plane, issuing a chunk's loads before its first store.
// (One cell per thread, not a 4-cell vector: at 96² that is 36 workgroups instead of 9 to share the float64 field; the
// planes themselves are small.)
// A replica's plane is a whole world: gW = W, gH = H, no offsets; the field is flow_wave_z / flow_perlin_z and the update
// flow_mix, as in k_food_flow_wave / k_food_flow_perlin.
// Loads in flight per thread.  Replicas past the last one of a chunk re-load the last plane (in bounds) and store nothing.
#define FLOW_BATCH_CHUNK 16

template <typename T, int KIND>
__global__ __launch_bounds__(DIE_BLOCK) void k_food_flow_batch(T* food, int W, int H, int R, int64_t plane_stride, double t, double scale,
                                                               double keep, double octaves, uint64_t seed) {
    const int64_t total = (int64_t)W * H;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int gi = (int)(i / H), gj = (int)(i - (int64_t)gi * H);
        const double z = KIND == DIE_FLOW_WAVE ? flow_wave_z(gi, gj, W, H, t) : flow_perlin_z(gi, gj, W, H, t, octaves, seed);
        for (int r0 = 0; r0 < R; r0 += FLOW_BATCH_CHUNK) {
            float v[FLOW_BATCH_CHUNK];
#pragma unroll
            for (int q = 0; q < FLOW_BATCH_CHUNK; ++q) v[q] = die_ld(food + (int64_t)min(r0 + q, R - 1) * plane_stride, i);
#pragma unroll
            for (int q = 0; q < FLOW_BATCH_CHUNK; ++q)
                if (r0 + q < R) die_st(food + (int64_t)(r0 + q) * plane_stride, i, flow_mix(scale, z, keep, v[q]));
        }
    }
}

template <typename T>
static void launch_food_flow_batch(int32_t kind, T* food, int W, int H, int R, int64_t plane_stride, double t, double scale, double keep,
                                   double octaves, uint64_t seed, hipStream_t s) {
    const int grid = init_grid((int64_t)W * H);
    if (kind == DIE_FLOW_WAVE) k_food_flow_batch<T, DIE_FLOW_WAVE><<<grid, DIE_BLOCK, 0, s>>>(food, W, H, R, plane_stride, t, scale, keep, octaves, seed);
    else k_food_flow_batch<T, DIE_FLOW_PERLIN><<<grid, DIE_BLOCK, 0, s>>>(food, W, H, R, plane_stride, t, scale, keep, octaves, seed);
}

// die_food_flow_batch_masked: the same update on the replicas whose bit is set.  A row of workgroups per replica (blockIdx.y);
// those of an unset replica exit at once, so a replica without a flow costs no memory traffic.  Each replica's workgroups
// evaluate the field themselves, by the functions k_food_flow_batch calls, so a full mask leaves its bits.
template <typename T, int KIND>
__global__ __launch_bounds__(DIE_BLOCK) void k_food_flow_batch_masked(T* food, int W, int H, int64_t plane_stride, double t, double scale,
                                                                      double keep, double octaves, uint64_t seed, uint64_t mask) {
    if (!((mask >> blockIdx.y) & 1ull)) return;
    food += (int64_t)blockIdx.y * plane_stride;
    const int64_t total = (int64_t)W * H;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int gi = (int)(i / H), gj = (int)(i - (int64_t)gi * H);
        const double z = KIND == DIE_FLOW_WAVE ? flow_wave_z(gi, gj, W, H, t) : flow_perlin_z(gi, gj, W, H, t, octaves, seed);
        die_st(food, i, flow_mix(scale, z, keep, die_ld(food, i)));
    }
}

template <typename T>
static void launch_food_flow_batch_masked(int32_t kind, T* food, int W, int H, int R, int64_t plane_stride, double t, double scale,
                                          double keep, double octaves, uint64_t seed, uint64_t mask, hipStream_t s) {
    const dim3 grid(init_grid((int64_t)W * H), R);
    if (kind == DIE_FLOW_WAVE) k_food_flow_batch_masked<T, DIE_FLOW_WAVE><<<grid, DIE_BLOCK, 0, s>>>(food, W, H, plane_stride, t, scale, keep, octaves, seed, mask);
    else k_food_flow_batch_masked<T, DIE_FLOW_PERLIN><<<grid, DIE_BLOCK, 0, s>>>(food, W, H, plane_stride, t, scale, keep, octaves, seed, mask);
}

static int food_flow_batch(const die_medium* m, const die_batch* b, int32_t kind, double t, double scale, double decay, int32_t octaves,
                           uint64_t seed, bool masked, uint64_t mask, void* stream, const char* who);

extern "C" int die_food_flow_batch(const die_medium* m, const die_batch* b, int32_t kind, double t, double scale, double decay,
                                   int32_t octaves, uint64_t seed, void* stream) {
    return food_flow_batch(m, b, kind, t, scale, decay, octaves, seed, false, 0, stream, "die_food_flow_batch");
}

extern "C" int die_food_flow_batch_masked(const die_medium* m, const die_batch* b, int32_t kind, double t, double scale, double decay,
                                          int32_t octaves, uint64_t seed, uint64_t replica_mask, void* stream) {
    return food_flow_batch(m, b, kind, t, scale, decay, octaves, seed, true, replica_mask, stream, "die_food_flow_batch_masked");
}

static int food_flow_batch(const die_medium* m, const die_batch* b, int32_t kind, double t, double scale, double decay, int32_t octaves,
                           uint64_t seed, bool masked, uint64_t mask, void* stream, const char* who) {
    DIE_REQUIRE(m && b && m->food, "%s: null argument", who);
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: %d replicas, 1..%d expected", who, b->replicas, DIE_MAX_REPLICAS);
    DIE_REQUIRE(kind == DIE_FLOW_WAVE || kind == DIE_FLOW_PERLIN, "%s: unknown flow kind %d", who, kind);
    DIE_REQUIRE(kind != DIE_FLOW_PERLIN || octaves >= 1, "%s: octaves %d", who, octaves);
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad field dtype %d", who, m->dtype);
    DIE_REQUIRE(m->gW <= 0, "%s: a replica's plane is a whole world, not a tile", who);
    DIE_REQUIRE(m->W >= 2 && m->H >= 2, "%s: the world must be at least 2x2, not %dx%d", who, m->W, m->H);
    // (the kernel does not need it, but no batched step exists for such planes: the step entries refuse them too)
    DIE_REQUIRE(m->H % 4 == 0, "%s: H %% 4 != 0 (H = %d): not a batched layout", who, m->H);
    DIE_REQUIRE(b->plane_stride >= (int64_t)m->W * m->H, "%s: plane_stride %lld smaller than a replica's %dx%d plane", who,
                (long long)b->plane_stride, m->W, m->H);
    const hipStream_t s = (hipStream_t)stream;
    if (masked) {
        DIE_REQUIRE(b->replicas == 64 || !(mask >> b->replicas), "%s: replica_mask %#llx has bits beyond the %d replicas", who,
                    (unsigned long long)mask, b->replicas);
        if (!mask) return DIE_OK;
        if (m->dtype == DIE_F32) launch_food_flow_batch_masked(kind, (float*)m->food, m->W, m->H, b->replicas, b->plane_stride, t, scale, 1.0 - decay, (double)octaves, seed, mask, s);
        else launch_food_flow_batch_masked(kind, (__half*)m->food, m->W, m->H, b->replicas, b->plane_stride, t, scale, 1.0 - decay, (double)octaves, seed, mask, s);
        DIE_CHECK_LAUNCH(who);
        return DIE_OK;
    }
    if (m->dtype == DIE_F32) launch_food_flow_batch(kind, (float*)m->food, m->W, m->H, b->replicas, b->plane_stride, t, scale, 1.0 - decay, (double)octaves, seed, s);
    else launch_food_flow_batch(kind, (__half*)m->food, m->W, m->H, b->replicas, b->plane_stride, t, scale, 1.0 - decay, (double)octaves, seed, s);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- DataInitializer builder steps on plain fp32 arrays (core/data_init.py:171-253) --------------------------------
// with_const (:214-216), with_noise / get_random (:168-169,218-220), with_agents (:222-226), with_food_perlin / with_chem
// (:228-236) fill one channel; build / build_agents (:238-253) multiply by the static mask and hand the channels over.
struct FieldOpArgs {
    float* dst;
    int64_t n;
    int op;                    // die_field_op
    int W, H;                  // perlin: the field shape (labels linspace(0, 1, W) × linspace(0, 1, H))
    double a, b;               // const: a; noise: range [a, b]; agents: ratio = b; perlin: threshold = b, octaves = a
    uint64_t seed;
    uint32_t step, word;
};

__global__ __launch_bounds__(DIE_BLOCK) void k_field_op(FieldOpArgs q) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q.n; i += stride) {
        double v = 0.0;
        if (q.op == DIE_FIELD_CONST) {
            v = q.a;
        } else if (q.op == DIE_FIELD_NOISE) {                 // (b − a)·random_sample().round(3) + a
            const int r = die_round3_units(die_draw(q.seed, q.step, (uint64_t)i, DIE_STREAM_BUILDER).v[q.word & 3u]);
            v = (q.b - q.a) * (r / 1000.0) + q.a;
        } else if (q.op == DIE_FIELD_AGENTS) {                // ceil(_mask(u, mask_above=ratio)): the stream of die_init_medium
            const int r = die_round3_units(die_draw(q.seed, q.step, (uint64_t)i, DIE_STREAM_INIT_AGENTS).v[0]);
            v = (r > 0 && r / 1000.0 <= q.b) ? 1.0 : 0.0;
        } else {                                              // DIE_FIELD_PERLIN
            const int ix = (int)(i / q.H), iy = (int)(i - (int64_t)ix * q.H);
            const double x = q.W > 1 ? (double)ix / (double)(q.W - 1) : 0.0, y = q.H > 1 ? (double)iy / (double)(q.H - 1) : 0.0;
            const double p = rint(die_perlin2(q.seed + q.step, x * q.a, y * q.a) * 1000.0) / 1000.0;
            v = mask_range(p, 0.0, q.b);
        }
        q.dst[i] = (float)v;
    }
}

extern "C" int die_field_fill(float* dst, int64_t n, int32_t op, int32_t W, int32_t H, double a, double b, uint64_t seed,
                              uint32_t step, uint32_t word, void* stream) {
    DIE_REQUIRE(dst && n > 0, "die_field_fill: bad array");
    DIE_REQUIRE(op >= DIE_FIELD_CONST && op <= DIE_FIELD_PERLIN, "die_field_fill: bad op %d", op);
    DIE_REQUIRE(op != DIE_FIELD_PERLIN || (W >= 1 && H >= 1 && (int64_t)W * H == n && a >= 1.0 && a < 524288.0), "die_field_fill: bad perlin shape");
    FieldOpArgs q;
    q.dst = dst; q.n = n; q.op = op; q.W = W; q.H = H; q.a = a; q.b = b; q.seed = seed; q.step = step; q.word = word;
    k_field_op<<<init_grid(n), DIE_BLOCK, 0, (hipStream_t)stream>>>(q);
    DIE_CHECK_LAUNCH("die_field_fill");
    return DIE_OK;
}

// build (:238-246): the three channels × mask into the medium's own representation (occupied cells get the
// provisional flag die_init_agents turns into claim words).  Any channel / the mask may be NULL (zeros / ones).
template <typename T>
__global__ __launch_bounds__(DIE_BLOCK) void k_medium_from_fields(int64_t C, uint64_t* owner, T* food, T* chem, const float* fa,
                                                                  const float* ff, const float* fc, const float* mask, float mask_scalar) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += stride) {
        const float mk = mask ? mask[c] : mask_scalar;
        owner[c] = (fa && fa[c] * mk > 0.f) ? 1ull : 0ull;
        die_st(food, c, ff ? ff[c] * mk : 0.f);
        die_st(chem, c, fc ? fc[c] * mk : 0.f);
    }
}

extern "C" int die_medium_from_fields(const die_medium* m, const float* agents, const float* food, const float* chem,
                                      const float* mask, float mask_scalar, void* stream) {
    DIE_REQUIRE(m && m->owner && m->food && m->chem && m->W >= 1 && m->H >= 1, "die_medium_from_fields: bad medium");
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "die_medium_from_fields: bad dtype %d", m->dtype);
    const int64_t C = (int64_t)m->W * m->H;
    if (m->dtype == DIE_F32)
        k_medium_from_fields<float><<<init_grid(C), DIE_BLOCK, 0, (hipStream_t)stream>>>(C, m->owner, (float*)m->food, (float*)m->chem,
                                                                                         agents, food, chem, mask, mask_scalar);
    else
        k_medium_from_fields<__half><<<init_grid(C), DIE_BLOCK, 0, (hipStream_t)stream>>>(C, m->owner, (__half*)m->food, (__half*)m->chem,
                                                                                          agents, food, chem, mask, mask_scalar);
    DIE_CHECK_LAUNCH("die_medium_from_fields");
    return DIE_OK;
}
