// What the separable gaussian's kernels share (gfx950): argument structs, edge rules, 16-byte accessors.  The two device bodies
// themselves — the LDS-tiled sweep and the row-marching one — are die_diffuse_tile.inc and die_diffuse_rows.inc,
// written once and included INSIDE each kernel that runs them, between the definitions of the one thing that differs: how a cell
// is loaded.  die_env.hip's k_diffuse / k_diffuse_rows read the plane as it is, die_signal.hip's kernels add the agents' emission
// first.  die_signal_grad.hip's kernels differ at the other end: they define DIF_STORE, what becomes of a finished output — left
// undefined it is the plain store, the statement every other kernel has always had.  Text, not a function: the compiler sees in k_diffuse / k_diffuse_rows the very tokens it always saw, so their code does
// not move when a twin is added (an inlined body function changed register allocation in every instantiation), and every twin sums
// in the same order.
#pragma once
#include "die_common.h"

#define DIF_TX 16      // tile rows (x, stride H)
#define DIF_TY 256     // tile columns (y, contiguous)
#define DIF_MAXR 8

struct DiffuseArgs {
    const void* src;
    void* dst;
    int W, H;
    float keep;                 // 1 − decay
    int mode;                   // die_diffuse_mode: what lies beyond the edges
    float w[2 * DIF_MAXR + 1];  // w[k + R], k = −R..R
};

__device__ __forceinline__ int wrap_idx(int v, int n) {
    v %= n;
    return v < 0 ? v + n : v;
}

// scipy.ndimage boundary modes (what skimage.filters.gaussian passes through, core/env.py:140-143): the index that
// stands in for v outside [0, n), or −1 for 'constant' (cval = 0)
__device__ __forceinline__ int edge_idx(int v, int n, int mode) {
    if (v >= 0 && v < n) return v;
    switch (mode) {
        case DIE_DIFFUSE_NEAREST: return v < 0 ? 0 : n - 1;
        case DIE_DIFFUSE_REFLECT: {                    // d c b a | a b c d | d c b a   (period 2n)
            int m = v % (2 * n);
            m = m < 0 ? m + 2 * n : m;
            return m < n ? m : 2 * n - 1 - m;
        }
        case DIE_DIFFUSE_MIRROR: {                     // d c b | a b c d | c b a       (period 2n − 2)
            if (n == 1) return 0;
            const int p = 2 * n - 2;
            int m = v % p;
            m = m < 0 ? m + p : m;
            return m < n ? m : p - m;
        }
        case DIE_DIFFUSE_CONSTANT: return -1;
        default: return wrap_idx(v, n);
    }
}

// ---- the row-marching sweep: one wave per strip of DIF_WCOLS columns, DIF_BLOCK threads a workgroup.  die_env.hip states the two
// numbers itself, with what they were measured against, ahead of this header (the premises of the mid-size tests are read from
// its text); a file that instantiates the sweep without it gets them here, and die_env.hip does not compile if the two disagree.
#ifdef DIF_WCOLS
static_assert(DIF_WCOLS == 248 && DIF_BLOCK == 128, "die_env.hip and die_diffuse.h state two different sweep shapes");
#else
#define DIF_WCOLS 248          // output columns per wave: 62 lanes of 4 cells, a halo lane on each side
#define DIF_BLOCK 128
#endif

struct RowsArgs {
    const void* src;
    void* dst;
    const unsigned long long* claim;   // FUSED == 1: the 64-bit claim plane
    const float* dep;                  // FUSED == 2: per cell the winner's deposit, or DIE_DEP_EMPTY (tile-binned step, die_pic.hip)
    void* food;                        // FUSED only
    int W, H, epoch, food_infinite;
    int64_t rep_cells;                 // batched replicas (gridDim.z > 1): plane stride in cells; partials / results stride per replica
    int halo;                          // tile mode: cells within `halo` of the array border belong to neighbours
    int rpw;                           // rows per wave (rows_per_wave): DIF_ROWS on large fields, fewer on small ones
    int wrapx, wrapy;                  // tile mode: this axis spans the whole world (one rank along it) and is periodic
    // k_reduce folded in: workgroup (0, 0) first sums the claim pass's `n_part` partial gains (a kernel boundary lies
    // between their producer and this sweep) in k_reduce's order and writes the step result — one launch less per step
    const long long* part_gain;
    const long long* part_gain2;       // NULL, or a second `n_part` partial gains (batched replicas' dead-slot pass)
    const long long* part_alive;       // NULL: num_alive = alive_const; else the sum of the claim pass's counts (ghost tiles)
    int n_part;
    die_step_result* result;
    long long alive_const;
    float keep, rate_feed;
    float w[2 * 4 + 1];
};

template <typename T> struct Vec4;
template <> struct Vec4<float> {
    static __device__ __forceinline__ void ld(const float* p, float v[4]) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    static __device__ __forceinline__ void st(float* p, const float v[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Vec4<__half> {
    static __device__ __forceinline__ void ld(const __half* p, float v[4]) {
        const uint2 t = *(const uint2*)p;
        const __half2 a = *(const __half2*)&t.x, b = *(const __half2*)&t.y;
        v[0] = __low2float(a); v[1] = __high2float(a); v[2] = __low2float(b); v[3] = __high2float(b);
    }
    static __device__ __forceinline__ void st(__half* p, const float v[4]) {
        const __half2 a = __halves2half2(die_f2h(v[0]), die_f2h(v[1])), b = __halves2half2(die_f2h(v[2]), die_f2h(v[3]));
        uint2 t; t.x = *(const uint32_t*)&a; t.y = *(const uint32_t*)&b;
        *(uint2*)p = t;
    }
};

// Per-replica Dynamics: the batched fused sweep of the replicas of ONE gaussian radius takes a table as an optional last argument
// (`TABLE...`: nothing, or a RowsTable).  Workgroup plane blockIdx.z then sweeps replica idx[blockIdx.z] with the taps, keep,
// rate_feed and food_infinite of that replica's row — scalar loads into the by-value RowsArgs ahead of the sweep, which
// is the instantiation (and so the arithmetic per cell) a stand-alone world of that sigma takes.  The index list travels by value;
// 64 rows would not fit the kernarg segment comfortably, hence the device table.
struct RowsTable {
    const die_dynamics_row* rows;
    int32_t n;
    uint8_t idx[DIE_MAX_REPLICAS];
};

__device__ __forceinline__ unsigned rows_replica(RowsArgs&, int) { return blockIdx.z; }
__device__ __forceinline__ unsigned rows_replica(RowsArgs& a, const int R, const RowsTable& t) {
    const unsigned z = t.idx[blockIdx.z];
    const die_dynamics_row row = t.rows[z];
    a.keep = row.keep; a.rate_feed = row.rate_feed; a.food_infinite = row.food_infinite;
    for (int k = 0; k <= 2 * R; ++k) a.w[k] = row.w[k];
    return z;
}

static bool rows_kernel_applies(int W, int H, int R) { return R <= 4 && H % 4 == 0 && H >= 4 && W >= 1; }
// RowsArgs.rpw for a launch that sweeps `planes` planes of W x H (die_env.hip's rows_per_wave, beside what it was measured with)
int die_rows_per_wave(int W, int H, int planes);
