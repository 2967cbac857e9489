// Device helpers shared by the population searchers (die_search.hip: PGPE, die_cmaes.hip: separable CMA-ES).
#pragma once
#include "die_common.h"
#include "die_rng.h"

// Sum of one double per thread of a 256-thread workgroup, the same bits in every thread: xor butterfly inside each wave
// (lane i and lane i ^ o add the same two values), then the four wave sums in a fixed order.
__device__ inline double pgpe_block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, DIE_WAVE);
    if ((threadIdx.x & (DIE_WAVE - 1)) == 0) lds[threadIdx.x / DIE_WAVE] = v;
    __syncthreads();
    const double t = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return t;
}

// the sum of the nb workgroup partials at work[off]: the same bits in every workgroup that asks
__device__ inline double pgpe_partials(const double* work, int64_t off, int nb, double* lds) {
    return pgpe_block_sum((int)threadIdx.x < nb ? work[off + threadIdx.x] : 0.0, lds);
}

// The cosine half of Box–Muller on the first two words of Philox(counter, generation, stream): oracle/rng.py
// normals2(seed, generation, n, stream, scale=1)[0][counter].
__device__ inline double die_search_normal(uint64_t seed, uint32_t generation, uint64_t counter, uint32_t stream) {
    const die_u32x4 r = die_draw(seed, generation, counter, stream);
    const double u1 = ((double)r.v[0] + 1.0) * (1.0 / 4294967296.0);      // (0, 1]
    const double u2 = (double)r.v[1] * (1.0 / 4294967296.0);              // [0, 1)
    const double rad = sqrt(-2.0 * log(u1));
    return rad * cos(6.283185307179586 * u2);
}

// Episodes (a candidate evaluated on E worlds, replica c E + e its e-th): every check of the fold, then its one launch —
// episode_fitness[c E + e] = F_{cE+e} (die_search_fitness of that replica), folded[c] = (((0 + F_{cE}) + F_{cE+1}) + …) / E.
// die_search.hip; shared by die_pgpe_update_episodes and die_cmaes_update_episodes.
int die_episode_fold_check(int32_t candidates, int32_t episodes, const double* episode_fitness, const double* folded, const char* who);
int die_episode_fold_launch(const double* terms, int64_t T, int64_t stride_t, int64_t stride_r, int32_t candidates, int32_t episodes,
                            double* episode_fitness, double* folded, void* stream, const char* who);

// f_r = sum over t ascending of q[t * st], q = terms + r * sr: eight loads in flight, then the adds in t order
__device__ inline double die_search_fitness(const double* q, int64_t T, int64_t st) {
    double s = 0.0, v[8];
    int64_t t = 0;
    for (; t + 8 <= T; t += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = q[(t + k) * st];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; t < T; ++t) s += q[t * st];
    return s;
}
