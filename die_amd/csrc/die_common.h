// Shared device/host helpers for libdie_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <math.h>
#include "../../include/die_hip.h"

#define DIE_WAVE 64
#define DIE_BLOCK 256

void die_set_error(const char* fmt, ...);

#define DIE_REQUIRE(cond, ...)                      \
    do {                                            \
        if (!(cond)) {                              \
            die_set_error(__VA_ARGS__);             \
            return DIE_ERR_ARG;                     \
        }                                           \
    } while (0)

// The three words of a step's result (reward, num_alive, status) may live in pinned HOST memory that the caller polls while the
// kernel that writes them is still running (Env(sync=True): include/die_hip.h die_host_device_pointer).  Written as system-scope
// atomic stores (write-through, `sc0 sc1`), so that their visibility to the host does not rest on the allocation being
// fine-grained / uncached or on the kernel's end; the host waits for each word's sentinel on its own, so no order between them is
// needed and no fence is issued (a release fence here would write back the XCD's whole L2 in the middle of the field kernel).
__device__ __forceinline__ void die_store_result_f64(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void die_store_result_i64(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

#define DIE_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            die_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return DIE_ERR_HIP;                                                       \
        }                                                                             \
    } while (0)

static inline int die_grid_for(int64_t n, int block = DIE_BLOCK) { return (int)((n + block - 1) / block); }

// scipy.ndimage._gaussian_kernel1d's radius int(4σ + .5).  Compared in double BEFORE the cast: the conversion of a value
// beyond int's range (sigma inf, 1e30) is undefined, and a caller's `R > max` refusal must not rest on what it happens to give.
// Saturates at INT32_MAX / INT32_MIN, NaN gives INT32_MIN (never a radius); every value in range converts as before.
static inline int die_gaussian_radius(float sigma) {
    const double r = 4.0 * (double)sigma + 0.5;
    if (r >= (double)INT32_MAX) return INT32_MAX;
    return r > (double)INT32_MIN ? (int)r : INT32_MIN;
}

// ---- host functions one .hip file defines and another calls (not exported; the NeuralAutomataAgent's are in die_nca.h, the
// tile-binned step's in die_forward.h).  Every such function is declared in exactly one header, which the defining file
// includes too: the compiler checks the definition against it.
// bytes of the scan scratch inside a step's workspace (die_init.hip; die_env.hip lays the workspace out)
int64_t die_ws_scan_bytes(int32_t W, int32_t H);
// (1 - decay) * G(src) of `replicas` fp32 planes, one (sigma, decay) or a row per replica (die_env.hip; die_env_grad.hip's adjoint)
int die_diffuse_rows_batch(const float* src, float* dst, int32_t W, int32_t H, int32_t replicas, int64_t plane_stride, float sigma,
                           float decay, const die_dynamics_row* rows, const die_dynamics_row* rows_host, void* stream, const char* who);

// ---- what the host side of several files asks alike: each stated here, once ------------------------------------------------
// do [p, p + p_bytes) and [q, q + q_bytes) share a byte?  (a null pointer is no range)
static inline bool die_ranges_overlap(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}
// a die_batch's n[0 .. replicas) as a kernel's n[DIE_MAX_REPLICAS], 0 past the last replica; returns the largest
static inline int64_t die_replica_counts(int64_t* dst, const int64_t* n, int32_t replicas) {
    int64_t nmax = 0;
    for (int r = 0; r < DIE_MAX_REPLICAS; ++r) {
        dst[r] = r < replicas ? n[r] : 0;
        if (dst[r] > nmax) nmax = dst[r];
    }
    return nmax;
}
// a die_batch's own fields, as the batched stock and memory calls require them (cells < 0: the call has no plane_stride rule of its
// own at this point).  die_nca_batch_shape_check and the steps of die_env.hip, die_init.hip and die_births.hip word theirs otherwise.
static inline int die_batch_check(const die_batch* b, int64_t cells, const char* who) {
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas (got %d)", who, DIE_MAX_REPLICAS, b->replicas);
    DIE_REQUIRE(cells < 0 || b->plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who,
                (long long)b->plane_stride, (long long)cells);
    DIE_REQUIRE(b->agent_stride >= 1 && b->agent_stride <= (int64_t)DIE_OWNER_SLOT_MASK - 1, "%s: agent_stride %lld outside 1..%lld", who,
                (long long)b->agent_stride, (long long)DIE_OWNER_SLOT_MASK - 1);
    for (int r = 0; r < b->replicas; ++r)
        DIE_REQUIRE(b->n[r] >= 0 && b->n[r] <= b->agent_stride, "%s: replica %d has %lld agents (0..%lld)", who, r, (long long)b->n[r],
                    (long long)b->agent_stride);
    return DIE_OK;
}

// A checked die_nca_dropout as the words a kernel reads (die_nca.hip die_dropout_words; die_rng.h defines the mask)
struct DropWords {
    uint64_t seed, seed_stride;  // replica z is masked with key seed + z · seed_stride (mod 2^64)
    uint64_t thr;                // a cell is dropped iff its word < thr = ceil(p · 2^32)
    uint32_t step;               // the forward-call counter
    float keep;                  // (float)(1 / (1 − p))
};

// ---- field element access (f32 / f16 planes) ---------------------------------------------
__device__ __forceinline__ float die_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float die_ld(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ void die_st(float* p, int64_t i, float v) { p[i] = v; }
// fp32 → fp16 of a value that has been ROUNDED TO fp32 first.  Without the barrier the compiler folds the arithmetic that
// produced `v` and the conversion into one mixed-precision instruction (v_fma_mixlo_f16: a single rounding straight to
// fp16) in some instantiations and not in others — the results then differ in the last fp16 bit whenever the fp32 value is
// an exact tie between two halves (found by tests/fuzz_cases.py fuzz_binned: f − 0.35·f on fp16 food).
__device__ __forceinline__ float die_round_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ __half die_f2h(float v) { return __float2half(die_round_f32(v)); }
__device__ __forceinline__ void die_st(__half* p, int64_t i, float v) { p[i] = die_f2h(v); }
// what a value becomes when it is stored in a plane of T and read back (the staged step stores chem + deposit before it
// diffuses; the fused sweeps keep the sum in registers and have to round it the same way to give the same bits)
template <typename T> __device__ __forceinline__ float die_as_stored(float v);
template <> __device__ __forceinline__ float die_as_stored<float>(float v) { return v; }
template <> __device__ __forceinline__ float die_as_stored<__half>(float v) { return __half2float(die_f2h(v)); }

// ---- Q0.32 fixed-point coordinates -------------------------------------------------------
// nearest label of linspace(0, 1, n) to X / 2^32, P may lie outside [0, 2^32) (probe offsets):
// clamp like pandas get_indexer(method='nearest') does (core/utils.py:39-54).
__device__ __forceinline__ int die_cell_u(uint32_t X, int n) {       // X in [0, 2^32): one 32×32→64 multiply-add, never clamps
    return (int)(((uint64_t)X * (uint32_t)(n - 1) + 0x80000000ull) >> 32);
}
__device__ __forceinline__ int die_cell(int64_t P, int n) {
    // (P·(n−1) + 2^31) >> 32 clamped to [0, n−1]: below 0 the quotient is ≤ 0, from 2^32 on it is ≥ n−1, so only the low
    // word needs the multiply (a zero-extended coordinate folds to die_cell_u at compile time)
    const int hi = (int)(P >> 32);
    const int c = die_cell_u((uint32_t)P, n);
    return hi == 0 ? c : (hi < 0 ? 0 : n - 1);
}

// nearest label to (X + off) / 2^32 for a coordinate X and a signed 32-bit offset (a probe): the 33-bit sum never
// materialises — a carry out of the 32-bit add (off >= 0) is "beyond the last label", a borrow (off < 0) "before the first"
__device__ __forceinline__ int die_cell_off(uint32_t X, int32_t off, int n) {
    const uint32_t lo = X + (uint32_t)off;
    const bool out = off >= 0 ? lo < X : lo > X;
    const int c = die_cell_u(lo, n);
    return out ? (off >= 0 ? n - 1 : 0) : c;
}

// square root to 1 ulp (v_sqrt_f32) instead of the correctly rounded library form (15 instructions).  Arguments below
// 2^-126 (denormals) count as 0: lengths that small are below the resolution of everything they are added to.
__device__ __forceinline__ float die_sqrt1(float v) { return __builtin_amdgcn_sqrtf(v); }

// float displacement (fraction of the unit square) → Q0.32 increment
// v·2^32 is exact in fp32 (a power-of-two scaling), so below 2^31 the nearest integer comes from the 32-bit convert;
// larger displacements take the float64 route.  Same value either way.
// the same for |v| < 0.5 (a guarantee of the caller: the tile-binned step bounds both the probe offset and the step length
// by a tile): no float64 fallback, no branch
__device__ __forceinline__ int64_t die_q32_small(float v) { return (int64_t)__float2int_rn(v * 4294967296.0f); }
__device__ __forceinline__ int64_t die_q32(float v) {
    const float t = v * 4294967296.0f;
    if (fabsf(t) < 2147483520.0f) return (int64_t)__float2int_rn(t);
    return (int64_t)__double2ll_rn((double)v * 4294967296.0);
}

__device__ __forceinline__ uint32_t die_owner_word(int epoch, int64_t slot) {
    return ((uint32_t)epoch << DIE_OWNER_EPOCH_SHIFT) | (uint32_t)(slot + 1);
}
__device__ __forceinline__ bool die_owner_occupied(uint32_t w, int epoch) {
    return (w >> DIE_OWNER_EPOCH_SHIFT) == (uint32_t)epoch;
}
// 64-bit claim: ownership word above the fp32 bits of the claimant's deposit
__device__ __forceinline__ unsigned long long die_claim(int epoch, int64_t slot, float deposit) {
    return ((unsigned long long)die_owner_word(epoch, slot) << 32) | (unsigned long long)__float_as_uint(deposit);
}
__device__ __forceinline__ bool die_claim_occupied(unsigned long long k, int epoch) {
    return (uint32_t)(k >> (32 + DIE_OWNER_EPOCH_SHIFT)) == (uint32_t)epoch;
}
__device__ __forceinline__ float die_claim_deposit(unsigned long long k) { return __uint_as_float((uint32_t)k); }

// The reward is accumulated in 32.32 fixed point: integer sums are associative, so reward does not depend on the order
// of the agent arrays, on the grid size or on the decomposition — bit for bit (a slot's gain is rounded to 2^-32 ≈
// 2.3e-10 once; the float64 sum it replaces differed by rounding noise between orders).
#define DIE_FIX_ONE 4294967296.0
__device__ __forceinline__ long long die_fix(float g) {
    const float t = g * 4294967296.0f;                       // exact (power-of-two scaling)
    if (fabsf(t) < 2147483520.0f) return (long long)__float2int_rn(t);
    return __double2ll_rn((double)g * DIE_FIX_ONE);
}

// np.isclose(0, x, rtol, atol): x <= atol + rtol·x as numpy evaluates it — the product rounded, then the sum (never one fma)
__host__ __device__ inline bool die_isclose_ok(double x, double atol, double rtol) {
#ifdef __HIP_DEVICE_COMPILE__
    const double m = __dmul_rn(rtol, x), s = __dadd_rn(atol, m);
#else
    volatile double m = rtol * x;
    volatile double s = atol + m;
#endif
    return x <= s;
}

// Largest x >= 0 that np.isclose(0, x, rtol, atol) accepts (core/agent/gradient.py:177-178).  The accepted set is an interval
// [0, X] (for rtol < 1 the right-hand side grows a hundred times slower than x), so X is found by bisection over the bit patterns
// of the non-negative doubles — a kernel then decides with ONE comparison per test, and the tie at the threshold falls exactly
// where numpy puts it.  Host (die_fill_fwd_args) and device (k_physarum_decode) run this one function.
__host__ __device__ inline double die_isclose_bound(double atol, double rtol) {
    if (!die_isclose_ok(0.0, atol, rtol)) return -1.0;
    if (!(rtol < 1.0)) return HUGE_VAL;
    const double top = 2.0 * atol / (1.0 - rtol) + 1e-300;
    if (die_isclose_ok(top, atol, rtol)) return HUGE_VAL;
    uint64_t lo = 0, hi;
    memcpy(&hi, &top, 8);
    while (hi - lo > 1) {                       // ok(lo), !ok(hi); the distance halves: 64 rounds at most
        const uint64_t mid = lo + (hi - lo) / 2;
        double x;
        memcpy(&x, &mid, 8);
        if (die_isclose_ok(x, atol, rtol)) lo = mid; else hi = mid;
    }
    double x;
    memcpy(&x, &lo, 8);
    return x;
}

// "no agent on this cell" in the deposit plane of the tile-binned step (a NaN no deposit can carry)
#define DIE_DEP_EMPTY 0xFFFFFFFFu

// ---- tile geometry (die_medium.gW/gH/ox/oy) ----------------------------------------------------
struct die_geo {
    int W, H;        // local plane dims (pitch = H)
    int gW, gH;      // world size used for coordinate → cell
    int ox, oy;      // global cell of local element (0, 0)
    int own_x0, own_y0, own_x1, own_y1;   // local cells this rank accounts for in reward / num_alive (x1 == 0: all)
};
static inline die_geo die_geo_of(const die_medium* m) {
    die_geo g;
    g.W = m->W; g.H = m->H;
    g.gW = m->gW > 0 ? m->gW : m->W; g.gH = m->gW > 0 ? m->gH : m->H;
    g.ox = m->gW > 0 ? m->ox : 0; g.oy = m->gW > 0 ? m->oy : 0;
    const bool own = m->gW > 0 && m->own_x1 > 0;
    g.own_x0 = own ? m->own_x0 : 0; g.own_y0 = own ? m->own_y0 : 0;
    g.own_x1 = own ? m->own_x1 : 0; g.own_y1 = own ? m->own_y1 : 0;
    return g;
}
// world cell → element of the local planes.  In a decomposed world the halo holds periodic images, so a
// cell on the far side of the world's seam maps into the halo (gx − ox modulo gW); then clamped: a slot can
// for one call sit outside the tile that holds it (zeroed by the lifecycle, about to migrate) and must never
// turn into an out-of-bounds access.  For periodic single-tile planes all of this is a no-op.
__device__ __forceinline__ int64_t die_local(const die_geo& g, int gx, int gy) {
    int lx = gx - g.ox, ly = gy - g.oy;
    lx = lx >= g.W ? lx - g.gW : (lx < 0 ? lx + g.gW : lx);      // beyond the planes: try the periodic image
    ly = ly >= g.H ? ly - g.gH : (ly < 0 ? ly + g.gH : ly);
    lx = lx < 0 ? 0 : (lx >= g.W ? g.W - 1 : lx);
    ly = ly < 0 ? 0 : (ly >= g.H ? g.H - 1 : ly);
    return (int64_t)lx * g.H + ly;
}

// world cell → row (or column) of the local planes for the TILE-BINNED kernels: the periodic image inside the planes or, for a
// cell the planes do not hold (an agent that walked out of a decomposed tile's halo), the NEAREST edge — an agent's local
// cell never jumps, so "an agent moves less than a tile per step" survives the plane's edge (die_local above tries one
// periodic image and clamps: fine for a lookup, but it sends the first row past the bottom edge to row 0).
// c in [0, gn), o = global cell of local element 0, n = local extent, gn = world extent
__device__ __forceinline__ int die_plane_coord(int c, int o, int n, int gn) {
    int l = c - o;
    l += l < 0 ? gn : 0;
    l -= l >= gn ? gn : 0;
    return l < n ? l : (l - n < gn - l ? n - 1 : 0);
}

// does this rank account for the agent standing on world cell (gx, gy)?  (ghost-agent decomposition)
__device__ __forceinline__ bool die_owned(const die_geo& g, int gx, int gy) {
    if (g.own_x1 == 0) return true;
    int lx = gx - g.ox, ly = gy - g.oy;
    lx = lx >= g.W ? lx - g.gW : (lx < 0 ? lx + g.gW : lx);
    ly = ly >= g.H ? ly - g.gH : (ly < 0 ? ly + g.gH : ly);
    return lx >= g.own_x0 && lx < g.own_x1 && ly >= g.own_y0 && ly < g.own_y1;
}

// ---- wave / block reductions -------------------------------------------------------------
__device__ __forceinline__ double die_wave_sum(double v) {
#pragma unroll
    for (int o = DIE_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, DIE_WAVE);
    return v;
}
__device__ __forceinline__ long long die_wave_sum(long long v) {
#pragma unroll
    for (int o = DIE_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, DIE_WAVE);
    return v;
}
// The same sum for a WHOLE wave (all 64 lanes active: the caller's control flow must be wave-uniform here), without LDS: the
// shuffle form above is six dependent pairs of ds_bpermute_b32, each an LDS round trip.  Data-parallel-primitive moves instead:
// an inclusive scan inside each row of 16 lanes (row_shr 1/2/4/8; a lane without a source adds 0), then lane 15 of rows 0 and 2
// into rows 1 and 3 (row_bcast:15, row mask 0xA) and lane 31 into rows 2 and 3 (row_bcast:31, row mask 0xC): lane 63 holds the
// total, which comes back wave-uniform (v_readlane).  Both halves of a lane's value move together and are added as 64 bits, so
// carries are exact at every step.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ long long die_dpp_i64(long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)v >> 32), CTRL, ROW_MASK, 0xF, false);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
}
__device__ __forceinline__ long long die_wave_sum_i64_dpp(long long v) {
    v += die_dpp_i64<0x111, 0xF>(v);      // row_shr:1
    v += die_dpp_i64<0x112, 0xF>(v);      // row_shr:2
    v += die_dpp_i64<0x114, 0xF>(v);      // row_shr:4
    v += die_dpp_i64<0x118, 0xF>(v);      // row_shr:8
    v += die_dpp_i64<0x142, 0xA>(v);      // row_bcast:15 → rows 1, 3
    v += die_dpp_i64<0x143, 0xC>(v);      // row_bcast:31 → rows 2, 3
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, DIE_WAVE - 1);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), DIE_WAVE - 1);
    return (long long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}

// Groups the active lanes of the wave by key (no memory traffic), then every group's first lane issues ONE atomicAdd of
// the group's size — all of a wave's atomics are in flight together — and the lanes get base + rank inside the group
// (lane order): a unique slot of the bucket's range when `counter` is a cursor.  RETURNING = false: histogram only.
template <bool RETURNING>
__device__ __forceinline__ uint32_t wave_grouped_add(uint32_t* counter, uint32_t key, bool active) {
    const int lane = threadIdx.x & (DIE_WAVE - 1);
    int my_lead = lane;
    uint32_t my_rank = 0, my_count = 0;
    bool todo = active;
    unsigned long long pending = __ballot(todo);
    while (pending) {
        const int lead = __ffsll((long long)pending) - 1;
        const uint32_t kk = __shfl(key, lead, DIE_WAVE);
        const bool match = todo && key == kk;
        const unsigned long long mask = __ballot(match);
        if (match) {
            my_lead = lead;
            my_rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (lane == lead) my_count = (uint32_t)__popcll(mask);
            todo = false;
        }
        pending &= ~mask;
    }
    uint32_t base = 0;
    if (active && lane == my_lead) {
        if (RETURNING) base = atomicAdd(&counter[key], my_count);
        else atomicAdd(&counter[key], my_count);
    }
    if (!RETURNING) return 0;
    base = __shfl(base, my_lead, DIE_WAVE);
    return base + my_rank;
}

