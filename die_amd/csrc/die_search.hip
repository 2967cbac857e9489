// PGPE search on the device (gfx950) — the training half of the reference's examples/learning_agents.py (evotorch's PGPE:
// symmetric sampling, centred ranks, ClipUp or Adam on the centre), over the (R, P) fp32 parameter matrix that
// BatchedNeuralAutomataAgent steps.  include/die_hip.h states the arithmetic; tests/pgpe_model.py is its float64 numpy twin.
//
//   k_pgpe_sample   one thread per (direction i, parameter p): one Philox block, Box–Muller, rows 2i and 2i + 1.
//   k_pgpe_rank     one wave: replica r's fitness (a serial float64 sum over t), its centred rank, the generation's
//                   statistics, the index of pop_best and whether it beats best.
//   k_pgpe_grad     grid-stride over P: g_mu and g_sigma of p (serial sums over i), the new sigma, pop_best / best rows;
//                   per-workgroup partial sums of g_mu^2 and of the new sigma.
//   k_pgpe_step     every workgroup reduces the partials of g_mu^2 itself (same tree, same bits in all of them), then the
//                   Adam step, or ClipUp's velocity before the clip (and the partials of its square).
//   k_pgpe_clip     ClipUp only: every workgroup reduces |v|^2, clips, moves the centre.
//   k_episode_fold  one wave, ahead of k_pgpe_rank / k_cmaes_rank when a candidate is evaluated on E worlds: thread r sums
//                   replica r's terms (the per-episode fitness), thread c then averages candidate c's E sums in episode order.
//                   The rank kernel reads the C averages as one term each.
// Workgroups: min(ceil(P / 256), DIE_PGPE_MAX_BLOCKS), a function of P only, so every reduction has one fixed tree — a
// wave's xor butterfly, the four waves in order, the workgroups' partials by the same block sum.  No float atomics.
//
// Roofline: the update reads the R x P matrix once (R = 10, P = 162 for the reference's agent: a few KB) — these launches
// are latency, not bandwidth; what matters is that there are few of them and that none waits for the host.
#include "die_search.h"

namespace {

struct PgpeArgs {
    int R, n, nb;
    int64_t P;
    uint64_t seed;
    double center_lr, stdev_lr, max_speed, momentum, beta1, beta2, eps, dmax, smin, smax;
    float *center, *stdev, *opt_a, *opt_b, *pop_best, *best;
    double *fitness, *evals, *history, *work;
};

// work layout (doubles)
#define PGPE_W_U 0               // [64] centred ranks
#define PGPE_W_BEST 64           // index of pop_best
#define PGPE_W_IMPROVED 65       // 1: pop_best beats best
#define PGPE_W_GSQ 256           // [nb] partials of g_mu^2
#define PGPE_W_SIG 512           // [nb] partials of the new sigma
#define PGPE_W_VSQ 768           // [nb] partials of ClipUp's |v|^2
#define PGPE_W_G 1024            // [P] g_mu, then ClipUp's unclipped velocity

__global__ __launch_bounds__(DIE_BLOCK) void k_pgpe_sample(PgpeArgs a, float* params, uint32_t generation) {
    const int64_t total = (int64_t)a.n * a.P;
    for (int64_t idx = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * DIE_BLOCK) {
        const int64_t i = idx / a.P, p = idx - i * a.P;
        const double z = die_search_normal(a.seed, generation, (uint64_t)idx, DIE_STREAM_SEARCH);
        const double c = (double)a.center[p];
        const double e = (double)a.stdev[p] * z;
        params[2 * i * a.P + p] = (float)(c + e);
        params[(2 * i + 1) * a.P + p] = (float)(c - e);
    }
}

__global__ __launch_bounds__(DIE_WAVE) void k_pgpe_rank(PgpeArgs a, const double* terms, int64_t T, int64_t st, int64_t sr,
                                                        int64_t generation) {
    __shared__ double f[DIE_MAX_REPLICAS], sorted[DIE_MAX_REPLICAS];
    const int r = threadIdx.x, R = a.R;
    if (r < R) f[r] = die_search_fitness(terms + r * sr, T, st);
    __syncthreads();
    if (r < R) {
        int k = 0;
        for (int j = 0; j < R; ++j) k += (f[j] < f[r] || (f[j] == f[r] && j < r)) ? 1 : 0;
        a.work[PGPE_W_U + r] = (double)k / (double)(R - 1) - 0.5;
        a.fitness[r] = f[r];
        sorted[k] = f[r];
    }
    __syncthreads();
    if (r == 0) {
        double sum = 0.0;
        int b = 0;
        for (int j = 0; j < R; ++j) {
            sum += f[j];
            if (f[j] > f[b]) b = j;
        }
        const double fb = f[b], prev = a.evals[1];
        const bool improved = fb > prev;
        a.work[PGPE_W_BEST] = (double)b;
        a.work[PGPE_W_IMPROVED] = improved ? 1.0 : 0.0;
        a.evals[0] = fb;
        if (improved) a.evals[1] = fb;
        double* h = a.history + generation * 6;
        h[0] = sum / (double)R;
        h[1] = sorted[R - 1];
        h[2] = sorted[0];
        h[3] = (sorted[R / 2 - 1] + sorted[R / 2]) / 2.0;
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_pgpe_grad(PgpeArgs a, const float* params) {
    __shared__ double lds[4];
    const double* u = a.work + PGPE_W_U;
    const int64_t b = (int64_t)a.work[PGPE_W_BEST];
    const bool improved = a.work[PGPE_W_IMPROVED] != 0.0;
    const double n = (double)a.n;
    double gsq = 0.0, ssum = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; p < a.P; p += (int64_t)a.nb * DIE_BLOCK) {
        const double c = (double)a.center[p], s = (double)a.stdev[p];
        const double ss = s * s;
        double gm = 0.0, gs = 0.0;
        for (int i = 0; i < a.n; ++i) {
            const double e = (double)params[2 * i * a.P + p] - c;
            const double du = (u[2 * i] - u[2 * i + 1]) / 2.0, av = (u[2 * i] + u[2 * i + 1]) / 2.0;
            // (one product per statement: -ffp-contract=on must not fuse these into FMAs — tests/pgpe_model.py rounds each)
            const double tm = e * du;
            gm += tm;
            const double ee = e * e;
            const double q = (ee - ss) / s;
            const double tq = av * q;
            gs += tq;
        }
        gm /= n;
        gs /= n;
        const double step = a.stdev_lr * gs;
        double ns = s + step;
        if (a.dmax >= 0.0) ns = fmin(fmax(ns, s * (1.0 - a.dmax)), s * (1.0 + a.dmax));
        ns = fmin(fmax(ns, a.smin), a.smax);
        const float nsf = (float)ns;
        a.stdev[p] = nsf;
        a.work[PGPE_W_G + p] = gm;
        const double g2 = gm * gm;
        gsq += g2;
        ssum += (double)nsf;
        const float w = params[b * a.P + p];
        a.pop_best[p] = w;
        if (improved) a.best[p] = w;
    }
    gsq = pgpe_block_sum(gsq, lds);
    ssum = pgpe_block_sum(ssum, lds);
    if (threadIdx.x == 0) {
        a.work[PGPE_W_GSQ + blockIdx.x] = gsq;
        a.work[PGPE_W_SIG + blockIdx.x] = ssum;
    }
}

template <int OPT>
__global__ __launch_bounds__(DIE_BLOCK) void k_pgpe_step(PgpeArgs a, int64_t generation) {
    __shared__ double lds[4];
    const double norm = sqrt(pgpe_partials(a.work, PGPE_W_GSQ, a.nb, lds));
    double vsq = 0.0;
    double bc1 = 1.0, bc2s = 1.0;
    if (OPT == DIE_PGPE_ADAM) {
        const double t = (double)(generation + 1);
        bc1 = 1.0 - pow(a.beta1, t);
        bc2s = sqrt(1.0 - pow(a.beta2, t));
    }
    for (int64_t p = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; p < a.P; p += (int64_t)a.nb * DIE_BLOCK) {
        const double gm = a.work[PGPE_W_G + p];
        if (OPT == DIE_PGPE_CLIPUP) {
            const double gh = norm > 0.0 ? gm / norm : 0.0;
            const double mv = a.momentum * (double)a.opt_a[p];
            const double av = a.center_lr * gh;
            const double v = mv + av;
            a.work[PGPE_W_G + p] = v;
            const double v2 = v * v;
            vsq += v2;
        } else {                                                // torch.optim.Adam on the loss gradient -g_mu
            const double g = -gm;
            const double m0 = a.beta1 * (double)a.opt_a[p], m1 = (1.0 - a.beta1) * g;
            const double m = m0 + m1;
            const double gg = g * g;
            const double v0 = a.beta2 * (double)a.opt_b[p], v1 = (1.0 - a.beta2) * gg;
            const double v = v0 + v1;
            const double denom = sqrt(v) / bc2s + a.eps;
            const double stepsize = a.center_lr / bc1;
            const double upd = stepsize * (m / denom);
            a.center[p] = (float)((double)a.center[p] - upd);
            a.opt_a[p] = (float)m;
            a.opt_b[p] = (float)v;
        }
    }
    if (OPT == DIE_PGPE_CLIPUP) {
        vsq = pgpe_block_sum(vsq, lds);
        if (threadIdx.x == 0) a.work[PGPE_W_VSQ + blockIdx.x] = vsq;
    }
    if (blockIdx.x == 0) {
        const double ssum = pgpe_partials(a.work, PGPE_W_SIG, a.nb, lds);
        if (threadIdx.x == 0) {
            a.history[generation * 6 + 4] = norm;
            a.history[generation * 6 + 5] = ssum / (double)a.P;
        }
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_pgpe_clip(PgpeArgs a) {
    __shared__ double lds[4];
    const double vn = sqrt(pgpe_partials(a.work, PGPE_W_VSQ, a.nb, lds));
    const bool clip = vn > a.max_speed;
    for (int64_t p = (int64_t)blockIdx.x * DIE_BLOCK + threadIdx.x; p < a.P; p += (int64_t)a.nb * DIE_BLOCK) {
        double v = a.work[PGPE_W_G + p];
        if (clip) {
            const double vm = v * a.max_speed;
            v = vm / vn;
        }
        a.center[p] = (float)((double)a.center[p] + v);
        a.opt_a[p] = (float)v;
    }
}

__global__ __launch_bounds__(DIE_WAVE) void k_episode_fold(const double* terms, int64_t T, int64_t st, int64_t sr, int C, int E,
                                                           double* episode_fitness, double* folded) {
    __shared__ double F[DIE_MAX_REPLICAS];
    const int r = threadIdx.x;
    if (r < C * E) {
        const double f = die_search_fitness(terms + r * sr, T, st);
        F[r] = f;
        episode_fitness[r] = f;
    }
    __syncthreads();
    if (r < C) {
        double s = 0.0;
        for (int e = 0; e < E; ++e) s += F[r * E + e];
        folded[r] = s / (double)E;
    }
}

// every refusal of both entry points, before any launch
int pgpe_args(PgpeArgs& a, const die_pgpe* s, int64_t generation, const char* who) {
    DIE_REQUIRE(s, "%s: null state", who);
    DIE_REQUIRE(s->replicas >= 2 && s->replicas <= DIE_MAX_REPLICAS && s->replicas % 2 == 0,
                "%s: replicas %d: an even number in 2..%d (symmetric pairs)", who, s->replicas, DIE_MAX_REPLICAS);
    DIE_REQUIRE(s->num_params >= 1, "%s: num_params %lld: at least 1", who, (long long)s->num_params);
    DIE_REQUIRE(s->optimizer == DIE_PGPE_CLIPUP || s->optimizer == DIE_PGPE_ADAM, "%s: unknown optimizer %d", who, s->optimizer);
    DIE_REQUIRE(s->center_lr > 0.0, "%s: center_lr %g: must be positive", who, s->center_lr);
    DIE_REQUIRE(s->stdev_lr > 0.0, "%s: stdev_lr %g: must be positive", who, s->stdev_lr);
    if (s->optimizer == DIE_PGPE_CLIPUP) {
        DIE_REQUIRE(s->max_speed > 0.0, "%s: max_speed %g: must be positive", who, s->max_speed);
        DIE_REQUIRE(s->momentum >= 0.0 && s->momentum < 1.0, "%s: momentum %g: in [0, 1)", who, s->momentum);
    } else {
        DIE_REQUIRE(s->beta1 >= 0.0 && s->beta1 < 1.0 && s->beta2 >= 0.0 && s->beta2 < 1.0, "%s: Adam betas (%g, %g): in [0, 1)", who,
                    s->beta1, s->beta2);
        DIE_REQUIRE(s->eps > 0.0, "%s: Adam eps %g: must be positive", who, s->eps);
    }
    DIE_REQUIRE(!(s->stdev_min > s->stdev_max), "%s: stdev_min %g above stdev_max %g", who, s->stdev_min, s->stdev_max);
    DIE_REQUIRE(s->center && s->stdev && s->opt_a && s->pop_best && s->best && s->fitness && s->evals && s->history && s->work &&
                    (s->optimizer != DIE_PGPE_ADAM || s->opt_b),
                "%s: null state buffer", who);
    DIE_REQUIRE(generation >= 0 && generation <= 0xFFFFFFFFll, "%s: generation %lld: in 0..2^32 - 1", who, (long long)generation);
    a.R = s->replicas;
    a.n = s->replicas / 2;
    a.P = s->num_params;
    const int64_t nb = (a.P + DIE_BLOCK - 1) / DIE_BLOCK;
    a.nb = (int)(nb < DIE_PGPE_MAX_BLOCKS ? nb : DIE_PGPE_MAX_BLOCKS);
    a.seed = s->seed;
    a.center_lr = s->center_lr; a.stdev_lr = s->stdev_lr; a.max_speed = s->max_speed; a.momentum = s->momentum;
    a.beta1 = s->beta1; a.beta2 = s->beta2; a.eps = s->eps;
    a.dmax = s->stdev_max_change; a.smin = s->stdev_min; a.smax = s->stdev_max;
    a.center = s->center; a.stdev = s->stdev; a.opt_a = s->opt_a; a.opt_b = s->opt_b; a.pop_best = s->pop_best; a.best = s->best;
    a.fitness = s->fitness; a.evals = s->evals; a.history = s->history; a.work = s->work;
    return DIE_OK;
}

}  // namespace

int die_episode_fold_check(int32_t candidates, int32_t episodes, const double* episode_fitness, const double* folded, const char* who) {
    DIE_REQUIRE(episodes >= 1, "%s: episodes %d: at least 1", who, episodes);
    DIE_REQUIRE(candidates >= 1 && (int64_t)candidates * episodes <= DIE_MAX_REPLICAS, "%s: %d candidates x %d episodes: at most %d replicas",
                who, candidates, episodes, DIE_MAX_REPLICAS);
    DIE_REQUIRE(episode_fitness && folded, "%s: null episode_fitness or folded buffer", who);
    return DIE_OK;
}

int die_episode_fold_launch(const double* terms, int64_t T, int64_t stride_t, int64_t stride_r, int32_t candidates, int32_t episodes,
                            double* episode_fitness, double* folded, void* stream, const char* who) {
    static_assert(DIE_MAX_REPLICAS <= DIE_WAVE, "k_episode_fold: one thread per replica of one wave");
    k_episode_fold<<<1, DIE_WAVE, 0, (hipStream_t)stream>>>(terms, T, stride_t, stride_r, candidates, episodes, episode_fitness, folded);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_pgpe_sample(const die_pgpe* s, float* params, int64_t generation, void* stream) {
    const char* who = "die_pgpe_sample";
    PgpeArgs a;
    const int rc = pgpe_args(a, s, generation, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(params, "%s: null parameter matrix", who);
    const int64_t total = (int64_t)a.n * a.P;
    const int64_t blocks = (total + DIE_BLOCK - 1) / DIE_BLOCK;
    k_pgpe_sample<<<(int)(blocks < 8192 ? blocks : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(a, params, (uint32_t)generation);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_pgpe_update(const die_pgpe* s, const float* params, const double* terms, int64_t T, int64_t stride_t,
                               int64_t stride_r, int64_t generation, void* stream) {
    const char* who = "die_pgpe_update";
    PgpeArgs a;
    const int rc = pgpe_args(a, s, generation, who);
    if (rc != DIE_OK) return rc;
    DIE_REQUIRE(params && terms, "%s: null parameter matrix or terms", who);
    DIE_REQUIRE(T >= 1, "%s: T %lld: at least one term per replica", who, (long long)T);
    DIE_REQUIRE(stride_t > 0 && stride_r > 0, "%s: strides (%lld, %lld) must be positive", who, (long long)stride_t, (long long)stride_r);
    DIE_REQUIRE(generation < s->history_rows, "%s: generation %lld beyond the %lld history rows", who, (long long)generation,
                (long long)s->history_rows);
    hipStream_t st = (hipStream_t)stream;
    k_pgpe_rank<<<1, DIE_WAVE, 0, st>>>(a, terms, T, stride_t, stride_r, generation);
    DIE_CHECK_LAUNCH(who);
    k_pgpe_grad<<<a.nb, DIE_BLOCK, 0, st>>>(a, params);
    DIE_CHECK_LAUNCH(who);
    if (s->optimizer == DIE_PGPE_ADAM) {
        k_pgpe_step<DIE_PGPE_ADAM><<<a.nb, DIE_BLOCK, 0, st>>>(a, generation);
        DIE_CHECK_LAUNCH(who);
        return DIE_OK;
    }
    k_pgpe_step<DIE_PGPE_CLIPUP><<<a.nb, DIE_BLOCK, 0, st>>>(a, generation);
    DIE_CHECK_LAUNCH(who);
    k_pgpe_clip<<<a.nb, DIE_BLOCK, 0, st>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_pgpe_update_episodes(const die_pgpe* s, const float* params, const double* terms, int64_t T, int64_t stride_t,
                                        int64_t stride_r, int32_t episodes, double* episode_fitness, double* folded,
                                        int64_t generation, void* stream) {
    const char* who = "die_pgpe_update_episodes";
    PgpeArgs a;
    int rc = pgpe_args(a, s, generation, who);
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
    return die_pgpe_update(s, params, folded, 1, 1, 1, generation, stream);       // f_c is the candidate's one term
}
