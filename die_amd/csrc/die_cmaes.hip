// Separable CMA-ES on the device (gfx950) — the second searcher of the reference's examples/learning_agents.py (evotorch's
// CMAES(separable=True): a diagonal covariance), over the (R, P) fp32 parameter matrix that BatchedNeuralAutomataAgent steps.
// include/die_hip.h states the arithmetic; tests/cmaes_model.py is its float64 numpy twin.
//
//   k_cmaes_sample  one thread per (replica i, parameter p): one Philox block, Box–Muller, row i.
//   k_cmaes_rank    one wave: replica r's fitness (a serial float64 sum over t), its rank (descending, ties to the lower
//                   index), the generation's statistics, whether pop_best beats best.
//   k_cmaes_paths   grid-stride over P: z and y of the mu best regenerated from their counters, y_w and z_w, the new mean and
//                   p_sigma, pop_best / best rows; per-workgroup partials of |p_sigma|^2 and, for every rank with a negative
//                   weight, of |z|^2.
//   k_cmaes_cov     every workgroup reduces those partials itself (same tree, same bits in all of them): h_sigma, the new
//                   sigma and the w°_k; then p_c and C over P (z regenerated once more), partials of sigma sqrt(C).
//   k_cmaes_stats   one workgroup: the history's mean stdev.
// Workgroups: min(ceil(P / 256), DIE_CMAES_MAX_BLOCKS), a function of P only, so every reduction has one fixed tree (the
// block sums of die_search.h).  No float atomics.  sigma is double-buffered by generation parity: every workgroup reads
// sigma[g & 1], k_cmaes_cov writes sigma[(g + 1) & 1], so no workgroup can see a sigma of the wrong generation.
//
// Roofline: R = 10, P = 162 for the reference's agent — the whole state is a few KB; these launches are latency, not
// bandwidth: what matters is that there are few of them and that none waits for the host.
#include "die_search.h"

namespace {

struct CmaesArgs {
    int R, mu, nb, csa_squared;
    int64_t P;
    uint64_t seed;
    double c_m, c_s, d_s, c_c, c_1, c_mu, mu_eff, chi;
    double ps_gain, pc_gain, c1cc, sum_w, h_thr;     // derived on the host: see cmaes_args
    double w[DIE_MAX_REPLICAS];
    double *m, *C, *ps, *pc, *sigma;
    float *pop_best, *best;
    double *fitness, *evals, *history, *work;
};

// work layout (doubles)
#define CMAES_W_ORDER 0                                  // [64] replica of rank k (best first)
#define CMAES_W_IMPROVED 64                              // 1: pop_best beats best
#define CMAES_W_PSQ (1 * DIE_CMAES_MAX_BLOCKS)           // [nb] partials of |p_sigma|^2
#define CMAES_W_SD (2 * DIE_CMAES_MAX_BLOCKS)            // [nb] partials of sigma' sqrt(C')
#define CMAES_W_ZSQ (4 * DIE_CMAES_MAX_BLOCKS)           // [R][DIE_CMAES_MAX_BLOCKS] partials of |z_{k:lambda}|^2
#define CMAES_W_YW(R) ((4 + (int64_t)(R)) * DIE_CMAES_MAX_BLOCKS)   // [P] y_w

__device__ inline double cmaes_z(const CmaesArgs& a, uint32_t generation, int i, int64_t p) {
    return die_search_normal(a.seed, generation, (uint64_t)i * (uint64_t)a.P + (uint64_t)p, DIE_STREAM_CMAES);
}

__global__ __launch_bounds__(DIE_BLOCK) void k_cmaes_sample(CmaesArgs a, float* params, uint32_t generation) {
    const int64_t total = (int64_t)a.R * a.P;
    const double sigma = a.sigma[generation & 1u];
    for (int64_t idx = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * DIE_BLOCK) {
        const int64_t p = idx % a.P;
        const double z = die_search_normal(a.seed, generation, (uint64_t)idx, DIE_STREAM_CMAES);
        // (one product per statement: -ffp-contract=on must not fuse these into FMAs — tests/cmaes_model.py rounds each)
        const double sd = sqrt(a.C[p]);
        const double t = sigma * sd;
        const double e = t * z;
        params[idx] = (float)(a.m[p] + e);
    }
}

__global__ __launch_bounds__(DIE_WAVE) void k_cmaes_rank(CmaesArgs a, const double* terms, int64_t T, int64_t st, int64_t sr,
                                                          int64_t generation) {
    __shared__ double f[DIE_MAX_REPLICAS], desc[DIE_MAX_REPLICAS];
    const int r = threadIdx.x, R = a.R;
    if (r < R) f[r] = die_search_fitness(terms + r * sr, T, st);
    __syncthreads();
    if (r < R) {
        int k = 0;
        for (int j = 0; j < R; ++j) k += (f[j] > f[r] || (f[j] == f[r] && j < r)) ? 1 : 0;
        a.work[CMAES_W_ORDER + k] = (double)r;
        a.fitness[r] = f[r];
        desc[k] = f[r];
    }
    __syncthreads();
    if (r == 0) {
        double sum = 0.0;
        for (int j = 0; j < R; ++j) sum += f[j];
        const double fb = desc[0], prev = a.evals[1];
        const bool improved = fb > prev;
        a.work[CMAES_W_IMPROVED] = improved ? 1.0 : 0.0;
        a.evals[0] = fb;
        if (improved) a.evals[1] = fb;
        double* h = a.history + generation * 6;
        h[0] = sum / (double)R;
        h[1] = desc[0];
        h[2] = desc[R - 1];
        h[3] = (R & 1) ? desc[R / 2] : (desc[R / 2] + desc[R / 2 - 1]) / 2.0;
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_cmaes_paths(CmaesArgs a, const float* params, uint32_t generation) {
    __shared__ double lds[4];
    __shared__ int order[DIE_MAX_REPLICAS];
    if ((int)threadIdx.x < a.R) order[threadIdx.x] = (int)a.work[CMAES_W_ORDER + threadIdx.x];
    __syncthreads();
    const bool improved = a.work[CMAES_W_IMPROVED] != 0.0;
    const int64_t b = order[0];
    const double step = a.c_m * a.sigma[generation & 1u];
    const double keep = 1.0 - a.c_s;
    double* yw_out = a.work + CMAES_W_YW(a.R);
    double psq = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; p < a.P; p += (int64_t)a.nb * DIE_BLOCK) {
        const double sd = sqrt(a.C[p]);
        double yw = 0.0, zw = 0.0;
        for (int k = 0; k < a.mu; ++k) {
            const double z = cmaes_z(a, generation, order[k], p);
            const double y = sd * z;
            const double ty = a.w[k] * y;
            yw += ty;
            const double tz = a.w[k] * z;
            zw += tz;
        }
        const double dm = step * yw;
        a.m[p] = a.m[p] + dm;
        const double ps0 = keep * a.ps[p];
        const double ps1 = a.ps_gain * zw;
        const double ps = ps0 + ps1;
        a.ps[p] = ps;
        yw_out[p] = yw;
        const double p2 = ps * ps;
        psq += p2;
        const float row = params[b * a.P + p];
        a.pop_best[p] = row;
        if (improved) a.best[p] = row;
    }
    psq = pgpe_block_sum(psq, lds);
    if (threadIdx.x == 0) a.work[CMAES_W_PSQ + blockIdx.x] = psq;
    for (int k = a.mu; k < a.R; ++k) {                  // |z|^2 of the ranks with a negative weight (active only)
        if (!(a.w[k] < 0.0)) continue;
        double s = 0.0;
        for (int64_t p = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; p < a.P; p += (int64_t)a.nb * DIE_BLOCK) {
            const double z = cmaes_z(a, generation, order[k], p);
            const double zz = z * z;
            s += zz;
        }
        s = pgpe_block_sum(s, lds);
        if (threadIdx.x == 0) a.work[CMAES_W_ZSQ + k * DIE_CMAES_MAX_BLOCKS + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_cmaes_cov(CmaesArgs a, int64_t generation) {
    __shared__ double lds[4];
    __shared__ double wo[DIE_MAX_REPLICAS];
    __shared__ int order[DIE_MAX_REPLICAS];
    if ((int)threadIdx.x < a.R) {
        order[threadIdx.x] = (int)a.work[CMAES_W_ORDER + threadIdx.x];
        wo[threadIdx.x] = a.w[threadIdx.x];
    }
    const double d = (double)a.P;
    const double psq = pgpe_partials(a.work, CMAES_W_PSQ, a.nb, lds);
    for (int k = a.mu; k < a.R; ++k) {
        if (!(a.w[k] < 0.0)) continue;
        const double zsq = pgpe_partials(a.work, CMAES_W_ZSQ + k * DIE_CMAES_MAX_BLOCKS, a.nb, lds);
        if (threadIdx.x == 0) {
            const double wd = a.w[k] * d;
            wo[k] = wd / zsq;
        }
    }
    __syncthreads();
    const double psn = sqrt(psq);
    const double keep = 1.0 - a.c_s;
    const double bias = sqrt(1.0 - pow(keep, 2.0 * (double)(generation + 1)));
    const double h = psn / bias < a.h_thr ? 1.0 : 0.0;
    const double sigma = a.sigma[generation & 1];
    double ex;
    if (a.csa_squared) {
        const double rate = a.c_s / (2.0 * a.d_s);
        ex = rate * (psq / d - 1.0);
    } else {
        const double rate = a.c_s / a.d_s;
        ex = rate * (psn / a.chi - 1.0);
    }
    const double sigma_new = sigma * exp(ex);
    const double a0 = 1.0 + (1.0 - h) * a.c1cc;
    const double a1 = a0 - a.c_1;
    const double coef = a1 - a.c_mu * a.sum_w;
    const double pc_gain = h * a.pc_gain;
    const double pc_keep = 1.0 - a.c_c;
    const uint32_t gen = (uint32_t)generation;
    const double* yw_in = a.work + CMAES_W_YW(a.R);
    double sds = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; p < a.P; p += (int64_t)a.nb * DIE_BLOCK) {
        const double pc0 = pc_keep * a.pc[p];
        const double pc1 = pc_gain * yw_in[p];
        const double pc = pc0 + pc1;
        const double c = a.C[p];
        const double sd = sqrt(c);
        double acc = 0.0;
        for (int k = 0; k < a.R; ++k) {
            if (wo[k] == 0.0) continue;
            const double z = cmaes_z(a, gen, order[k], p);
            const double y = sd * z;
            const double yy = y * y;
            const double t = wo[k] * yy;
            acc += t;
        }
        const double t0 = coef * c;
        const double pc2 = pc * pc;
        const double t1 = a.c_1 * pc2;
        const double t2 = a.c_mu * acc;
        const double cn = (t0 + t1) + t2;
        a.pc[p] = pc;
        a.C[p] = cn;
        const double s = sigma_new * sqrt(cn);
        sds += s;
    }
    sds = pgpe_block_sum(sds, lds);
    if (threadIdx.x == 0) {
        a.work[CMAES_W_SD + blockIdx.x] = sds;
        if (blockIdx.x == 0) {
            a.sigma[(generation + 1) & 1] = sigma_new;
            a.history[generation * 6 + 4] = sigma_new;
        }
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_cmaes_stats(CmaesArgs a, int64_t generation) {
    __shared__ double lds[4];
    const double sds = pgpe_partials(a.work, CMAES_W_SD, a.nb, lds);
    if (threadIdx.x == 0) a.history[generation * 6 + 5] = sds / (double)a.P;
}

// every refusal of both entry points, before any launch
int cmaes_args(CmaesArgs& a, const die_cmaes* s, int64_t generation, const char* who) {
    DIE_REQUIRE(s, "%s: null state", who);
    DIE_REQUIRE(s->replicas >= 2 && s->replicas <= DIE_MAX_REPLICAS, "%s: replicas %d: in 2..%d", who, s->replicas, DIE_MAX_REPLICAS);
    DIE_REQUIRE(s->num_params >= 1, "%s: num_params %lld: at least 1", who, (long long)s->num_params);
    DIE_REQUIRE(s->c_m > 0.0, "%s: c_m %g: must be positive", who, s->c_m);
    DIE_REQUIRE(s->c_sigma > 0.0 && s->c_sigma <= 1.0, "%s: c_sigma %g: in (0, 1]", who, s->c_sigma);
    DIE_REQUIRE(s->d_sigma > 0.0, "%s: d_sigma %g: must be positive", who, s->d_sigma);
    DIE_REQUIRE(s->c_c > 0.0 && s->c_c <= 1.0, "%s: c_c %g: in (0, 1]", who, s->c_c);
    DIE_REQUIRE(s->c_1 >= 0.0 && s->c_mu >= 0.0 && s->c_1 + s->c_mu <= 1.0, "%s: c_1 %g, c_mu %g: non-negative, sum at most 1", who,
                s->c_1, s->c_mu);
    DIE_REQUIRE(s->mu_eff >= 1.0, "%s: mu_eff %g: at least 1", who, s->mu_eff);
    DIE_REQUIRE(s->chi_d > 0.0, "%s: chi_d %g: must be positive", who, s->chi_d);
    DIE_REQUIRE(s->weights[0] > 0.0, "%s: weights[0] %g: must be positive", who, s->weights[0]);
    DIE_REQUIRE(s->center && s->C && s->p_sigma && s->p_c && s->sigma && s->pop_best && s->best && s->fitness && s->evals &&
                    s->history && s->work,
                "%s: null state buffer", who);
    DIE_REQUIRE(generation >= 0 && generation <= 0xFFFFFFFFll, "%s: generation %lld: in 0..2^32 - 1", who, (long long)generation);
    const int R = s->replicas;
    a.R = R;
    a.mu = R / 2;
    a.csa_squared = s->csa_squared != 0;
    a.P = s->num_params;
    const int64_t nb = (a.P + DIE_BLOCK - 1) / DIE_BLOCK;
    a.nb = (int)(nb < DIE_CMAES_MAX_BLOCKS ? nb : DIE_CMAES_MAX_BLOCKS);
    a.seed = s->seed;
    a.c_m = s->c_m; a.c_s = s->c_sigma; a.d_s = s->d_sigma; a.c_c = s->c_c; a.c_1 = s->c_1; a.c_mu = s->c_mu;
    a.mu_eff = s->mu_eff; a.chi = s->chi_d;
    a.ps_gain = sqrt(a.c_s * (2.0 - a.c_s) * a.mu_eff);
    a.pc_gain = sqrt(a.c_c * (2.0 - a.c_c) * a.mu_eff);
    a.c1cc = a.c_1 * a.c_c * (2.0 - a.c_c);
    a.sum_w = 0.0;
    for (int k = 0; k < DIE_MAX_REPLICAS; ++k) {
        a.w[k] = k < R ? s->weights[k] : 0.0;
        a.sum_w += a.w[k];
    }
    a.h_thr = (1.4 + 2.0 / ((double)a.P + 1.0)) * a.chi;
    a.m = s->center; a.C = s->C; a.ps = s->p_sigma; a.pc = s->p_c; a.sigma = s->sigma;
    a.pop_best = s->pop_best; a.best = s->best;
    a.fitness = s->fitness; a.evals = s->evals; a.history = s->history; a.work = s->work;
    return DIE_OK;
}

}  // namespace

extern "C" int die_cmaes_sample(const die_cmaes* s, float* params, int64_t generation, void* stream) {
    const char* who = "die_cmaes_sample";
    CmaesArgs a;
    const int rc = cmaes_args(a, s, generation, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(params, "%s: null parameter matrix", who);
    const int64_t total = (int64_t)a.R * a.P;
    const int64_t blocks = (total + DIE_BLOCK - 1) / DIE_BLOCK;
    k_cmaes_sample<<<(int)(blocks < 8192 ? blocks : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(a, params, (uint32_t)generation);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_cmaes_update(const die_cmaes* s, const float* params, const double* terms, int64_t T, int64_t stride_t,
                                int64_t stride_r, int64_t generation, void* stream) {
    const char* who = "die_cmaes_update";
    CmaesArgs a;
    const int rc = cmaes_args(a, s, generation, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(params && terms, "%s: null parameter matrix or terms", who);
    DIE_REQUIRE(T >= 1, "%s: T %lld: at least one term per replica", who, (long long)T);
    DIE_REQUIRE(stride_t > 0 && stride_r > 0, "%s: strides (%lld, %lld) must be positive", who, (long long)stride_t, (long long)stride_r);
    DIE_REQUIRE(generation < s->history_rows, "%s: generation %lld beyond the %lld history rows", who, (long long)generation,
                (long long)s->history_rows);
    hipStream_t st = (hipStream_t)stream;
    k_cmaes_rank<<<1, DIE_WAVE, 0, st>>>(a, terms, T, stride_t, stride_r, generation);
    DIE_CHECK_LAUNCH(who);
    k_cmaes_paths<<<a.nb, DIE_BLOCK, 0, st>>>(a, params, (uint32_t)generation);
    DIE_CHECK_LAUNCH(who);
    k_cmaes_cov<<<a.nb, DIE_BLOCK, 0, st>>>(a, generation);
    DIE_CHECK_LAUNCH(who);
    k_cmaes_stats<<<1, DIE_BLOCK, 0, st>>>(a, generation);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_cmaes_update_episodes(const die_cmaes* s, const float* params, const double* terms, int64_t T, int64_t stride_t,
                                         int64_t stride_r, int32_t episodes, double* episode_fitness, double* folded,
                                         int64_t generation, void* stream) {
    const char* who = "die_cmaes_update_episodes";
    CmaesArgs a;
    int rc = cmaes_args(a, s, generation, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(params && terms, "%s: null parameter matrix or terms", who);
    DIE_REQUIRE(T >= 1, "%s: T %lld: at least one term per replica", who, (long long)T);
    DIE_REQUIRE(stride_t > 0 && stride_r > 0, "%s: strides (%lld, %lld) must be positive", who, (long long)stride_t, (long long)stride_r);
    DIE_REQUIRE(generation < s->history_rows, "%s: generation %lld beyond the %lld history rows", who, (long long)generation,
                (long long)s->history_rows);
    rc = die_episode_fold_check(s->replicas, episodes, episode_fitness, folded, who);
    if (rc != DIE_OK) return rc;
    rc = die_episode_fold_launch(terms, T, stride_t, stride_r, s->replicas, episodes, episode_fitness, folded, stream, who);
    if (rc != DIE_OK) return rc;
    return die_cmaes_update(s, params, folded, 1, 1, 1, generation, stream);      // f_c is the candidate's one term
}
