// The adjoint of NeuralAutomataAgent's sensing (gfx950): what die_nca.hip computes forward,
//   z_l = conv_l(z_{l−1}) for l = 1..L (z_0: the medium's planes; nothing between the layers),   s = tanh(z_L) · mask,
//   action[c, n] = s[c, cell(x_n), cell(y_n)] · coef[c] for every slot n,
// differentiated with respect to the layers' weights — "backpropagation through agent indexing operation" (core/agent/evo.py:48).
//
//   k_gather_scale_backward   g_s[c, cell_n] += grad_action[c, n] · coef[c] into planes the entry point has zeroed: k_gather_scale's
//                     indexing (die_cell / die_local), one fp32 atomic add per non-zero term.  Several slots may stand on one cell
//                     (dead slots often do, alive agents never): the sum's order is then the arrival order.  The result is
//                     bit-reproducible run to run whenever no two slots with a non-zero gradient share a cell.
//   k_conv_backward   one layer, one launch: the forward's 16 × 64 tile.  A workgroup stages, for every channel, the input tile
//                     plus halo (nca_load semantics for the first layer: fp32 / fp16 fields, the 'agents' channel from the claim
//                     plane) and the tile plus halo of the gradient g_z arriving at the layer's outputs.  For the layer that
//                     carried the tanh, g_z = g_s · mask · (1 − t²) is formed while staging, from t = tanh(z_L) as the forward
//                     stored it UNMASKED and the mask recomputed from its key (die_rng.h: a pure function of key, step and
//                     cell) — no launch of its own, no division by keep.
//       weight gradient   grad_w[o, i, a, b] = Σ_{x, y} g_z[o, x, y] · in[i, pad(x + a − r), pad(y + b − r)].  A lane owns one column
//                     of the tile and keeps its 16 g_z of every output channel in registers; a wave takes the units (i, b) wave,
//                     wave + 4, …, reads the unit's input column (16 + 2r values, consecutive lanes on consecutive LDS words:
//                     no bank conflict) and forms, for every (o, a), 16 products down the column, then a butterfly sum over the
//                     64 lanes.  Lane 0 stores the term into the workgroup's partial row [cout · cin · k · k] — every element
//                     of the row is written once, by one wave.  NO float atomics.
//       input gradient    (layers ≥ 2 only; the first layer's input is the medium, no leaf) grad_in[i, x, y] = Σ_o Σ_a Σ_b
//                     w[o, i, a, b] · g_z[o, pad'(x − a + r), pad'(y − b + r)]: the correlation with the flipped kernel, where
//                     pad' is the padding's adjoint — 'circular' wraps, 'zeros' drops what falls outside.  Thread layout and
//                     stores are the forward's (4 consecutive y per thread, 16-byte stores where H % 4 == 0).
//   k_conv_backward_sum   the second launch: one thread per weight sums the partial rows in tile-index order (tile = row of tiles ·
//                     tiles per row + column), in float64, and stores fp32.  Fixed order, fixed tree: the same inputs give the
//                     same bits on every run.
//
//   die_nca_backward_batch / die_gather_scale_backward_batch   the same for every replica of a die_batch (a population's candidates):
//                     k_conv_backward<K, true> with the replica in blockIdx.z, k_conv_backward_sum_batch folding a candidate's E
//                     replicas in a fixed order, k_gather_scale_backward_batch with the replica in blockIdx.y.  Replica r is bit
//                     for bit the stand-alone computation on its world.
//
// Roofline: as the forward (die_nca.hip) — a 3→3 3×3 layer reads 9 planes and writes 3 per cell for 2 × 81 MAC: no MFMA.
#include <math.h>
#include <type_traits>
#include "die_common.h"
#include "die_rng.h"
#include "die_nca.h"

struct ConvBwdArgs {
    const void* in[NCA_MAXC];
    int kind[NCA_MAXC];          // die_conv_plane.kind
    const float* g[NCA_MAXC];    // gradient at the layer's outputs (before the tanh adjoint when t is given)
    const float* t[NCA_MAXC];    // the layer's forward outputs tanh(z), unmasked, or all null
    float* gin[NCA_MAXC];        // gradient at the layer's inputs, or all null
    const float* w;              // [cout][cin][k][k]
    float* part;                 // [tiles][cout · cin · k · k]
    int W, H, cin, cout, epoch, pad;
    int has_t, has_drop, has_gin;
    DropWords d;
};
// what a BATCH launch reads on top (die_nca_backward_batch; the stand-alone instantiations keep ConvBwdArgs as their whole argument):
// elements from replica r's planes / weights / partial rows to replica r + 1's
struct ConvBwdBatchArgs : ConvBwdArgs {
    int64_t rep_in, rep_g, rep_t, rep_gin, rep_w, rep_part;
    int episodes;                // replica r stages weight row r / episodes (1: a row per replica)
};

// BATCH: replica blockIdx.z of die_nca_backward_batch — its planes, its candidate's weights, its mask key (seed + z · seed_stride) and
// its block of partial rows; tile, staging, register layout, butterfly and the tanh / mask adjoint are this one body.
template <int K, bool BATCH = false>
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_backward(typename std::conditional<BATCH, ConvBwdBatchArgs, ConvBwdArgs>::type a) {
    constexpr int R = K / 2, LX = NCA_TX + 2 * R, LYV = NCA_TY + 2 * R, LY = LYV + 1;     // odd pitch, as the forward
    extern __shared__ __align__(16) float nca_grad_smem[];
    float* s_in = nca_grad_smem;                             // [cin][LX][LY]
    float* s_g = s_in + a.cin * LX * LY;                     // [cout][LX][LY]
    float* s_w = s_g + a.cout * LX * LY;                     // [cout][cin][K][K]
    const int x0 = blockIdx.y * NCA_TX, y0 = blockIdx.x * NCA_TY;
    const int nw = a.cout * a.cin * K * K;
    // replica z's offsets into the planes, weights and partial rows, and its mask key (BATCH only: every use below is the stand-alone
    // expression when BATCH is off, so those instantiations compile to the code they always had)
    [[maybe_unused]] int64_t o_in = 0, o_g = 0, o_t = 0, o_gin = 0, o_w = 0, o_part = 0;
    [[maybe_unused]] uint64_t key = 0;
    if constexpr (BATCH) {
        const int64_t z = (int64_t)blockIdx.z;
        o_in = z * a.rep_in; o_g = z * a.rep_g; o_t = z * a.rep_t; o_gin = z * a.rep_gin;
        o_w = (int64_t)((int)blockIdx.z / a.episodes) * a.rep_w;
        o_part = z * a.rep_part;
        key = a.d.seed + (uint64_t)blockIdx.z * a.d.seed_stride;
    }
    for (int i = threadIdx.x; i < nw; i += DIE_BLOCK) s_w[i] = BATCH ? a.w[o_w + i] : a.w[i];
    // every staged element stands for the virtual cell (x0 − R + li, y0 − R + lj), read through the padding: also past the field's
    // last row / column inside a partial tile, where the input gradient of the cells before the edge needs the wrapped values
    for (int i = threadIdx.x; i < LX * LYV; i += DIE_BLOCK) {
        const int li = i / LYV, lj = i - li * LYV;
        const int gx = nca_pad_index(x0 - R + li, a.W, a.pad), gy = nca_pad_index(y0 - R + lj, a.H, a.pad);
        const bool in_field = gx >= 0 && gy >= 0;
        const int64_t cell = in_field ? (int64_t)gx * a.H + gy : 0;
        for (int c = 0; c < a.cin; ++c) s_in[(c * LX + li) * LY + lj] = in_field ? nca_load(a.in[c], a.kind[c], BATCH ? o_in + cell : cell, a.epoch) : 0.f;
        float m = 1.f;
        if (a.has_drop && in_field) m = die_dropout_factor(die_dropout_word(BATCH ? key : a.d.seed, a.d.step, (uint64_t)cell), a.d.thr, a.d.keep);
        for (int o = 0; o < a.cout; ++o) {
            float v = 0.f;
            if (in_field) {
                v = a.g[o][BATCH ? o_g + cell : cell];
                if (a.has_t) {
                    const float t = a.t[o][BATCH ? o_t + cell : cell];
                    v = a.has_drop ? v * m * (1.f - t * t) : v * (1.f - t * t);
                }
            }
            s_g[(o * LX + li) * LY + lj] = v;
        }
    }
    __syncthreads();

    // ---- weight gradient: this tile's row of partial sums
    {
        const int lane = threadIdx.x & (DIE_WAVE - 1), wave = threadIdx.x / DIE_WAVE;
        const bool col_ok = y0 + lane < a.H;
        float greg[NCA_MAXC][NCA_TX];
#pragma unroll
        for (int o = 0; o < NCA_MAXC; ++o) {
#pragma unroll
            for (int r = 0; r < NCA_TX; ++r) {
                greg[o][r] = 0.f;
                if (o < a.cout && col_ok && x0 + r < a.W) greg[o][r] = s_g[(o * LX + r + R) * LY + lane + R];
            }
        }
        float* prow = (BATCH ? a.part + o_part : a.part) + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nw;
        for (int u = wave; u < a.cin * K; u += DIE_BLOCK / DIE_WAVE) {       // wave-uniform
            const int i = u / K, b = u - i * K;
            float col[LX];
#pragma unroll
            for (int r = 0; r < LX; ++r) col[r] = s_in[(i * LX + r) * LY + lane + b];
#pragma unroll
            for (int ka = 0; ka < K; ++ka) {
#pragma unroll
                for (int o = 0; o < NCA_MAXC; ++o) {
                    if (o < a.cout) {
                        float p = 0.f;
#pragma unroll
                        for (int r = 0; r < NCA_TX; ++r) p += greg[o][r] * col[r + ka];
#pragma unroll
                        for (int off = DIE_WAVE / 2; off > 0; off >>= 1) p += __shfl_xor(p, off, DIE_WAVE);
                        if (lane == 0) prow[((o * a.cin + i) * K + ka) * K + b] = p;
                    }
                }
            }
        }
    }
    if (!a.has_gin) return;

    // ---- input gradient: s_g row ti + a' is virtual x − R + a' = x − a + r for a = K − 1 − a'
    const int ti = threadIdx.x / (NCA_TY / 4), tj = (threadIdx.x % (NCA_TY / 4)) * 4;
    float acc[NCA_MAXC][4];
#pragma unroll
    for (int c = 0; c < NCA_MAXC; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.f;
    for (int o = 0; o < a.cout; ++o) {
#pragma unroll
        for (int ka = 0; ka < K; ++ka) {
            float row[4 + K - 1];
#pragma unroll
            for (int q = 0; q < 4 + K - 1; ++q) row[q] = s_g[(o * LX + ti + ka) * LY + tj + q];
#pragma unroll
            for (int c = 0; c < NCA_MAXC; ++c) {
                if (c < a.cin) {
#pragma unroll
                    for (int kb = 0; kb < K; ++kb) {
                        const float wv = s_w[((o * a.cin + c) * K + (K - 1 - ka)) * K + (K - 1 - kb)];
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[c][q] += wv * row[q + kb];
                    }
                }
            }
        }
    }
    const int gx = x0 + ti, gy = y0 + tj;
    if (gx >= a.W || gy >= a.H) return;
#pragma unroll
    for (int c = 0; c < NCA_MAXC; ++c) {
        if (c < a.cin) {
            float* dst = (BATCH ? a.gin[c] + o_gin : a.gin[c]) + (int64_t)gx * a.H + gy;
            if (gy + 3 < a.H && (a.H & 3) == 0) *(float4*)dst = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (gy + q < a.H) dst[q] = acc[c][q];
            }
        }
    }
}

// weight j: `rows` partial rows in ascending order, float64, rounded once
__device__ __forceinline__ void conv_backward_sum_one(const float* part, int64_t rows, int nw, int j, float* out) {
    double s = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < rows; ++t) s += (double)part[t * nw + j];
    out[j] = (float)s;
}

// one thread per weight: the tiles' partial rows in tile-index order
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_backward_sum(const float* part, int64_t tiles, int nw, float* out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nw) conv_backward_sum_one(part, tiles, nw, j, out);
}

// the same launch for die_conv2d_wide_backward's partial rows (die_nca_wide_grad.hip)
void die_conv_backward_fold(const float* part, int64_t tiles, int nw, float* out, hipStream_t s) {
    k_conv_backward_sum<<<die_grid_for(nw), DIE_BLOCK, 0, s>>>(part, tiles, nw, out);
}

// die_nca_backward_batch's: one thread per (candidate blockIdx.y, weight j).  The E replicas of candidate c hold their partial rows
// one behind the other ([replica][tile][nw], replica = c · E + e), so the fold "episode e = 0 … E − 1 outermost, tile index ascending
// inside" is ONE ascending walk over E · tiles rows — for E = 1 k_conv_backward_sum on replica c's rows.
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_backward_sum_batch(const float* part, int64_t rows, int nw, float* out, int64_t out_stride) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nw) conv_backward_sum_one(part + (int64_t)blockIdx.y * rows * nw, rows, nw, j, out + (int64_t)blockIdx.y * out_stride);
}

// the same launch for die_nca_wide_backward_batch's partial rows (die_nca_wide_grad.hip): candidate c's `rows` rows into out + c * out_stride
void die_conv_backward_fold_batch(const float* part, int64_t rows, int nw, int candidates, float* out, int64_t out_stride, hipStream_t s) {
    k_conv_backward_sum_batch<<<dim3((unsigned)die_grid_for(nw), (unsigned)candidates), DIE_BLOCK, 0, s>>>(part, rows, nw, out, out_stride);
}

static bool conv_shape_ok(int32_t W, int32_t H, int32_t cin, int32_t cout, int32_t k) {
    return W >= 1 && H >= 1 && cin >= 1 && cin <= NCA_MAXC && cout >= 1 && cout <= NCA_MAXC && (k == 1 || k == 3 || k == 5 || k == 7);
}

extern "C" int64_t die_conv2d_backward_workspace_bytes(int32_t W, int32_t H, int32_t cin, int32_t cout, int32_t k) {
    if (!conv_shape_ok(W, H, cin, cout, k)) return -1;
    return die_nca_tiles(W, H) * cout * cin * k * k * (int64_t)sizeof(float);
}

extern "C" int die_conv2d_backward(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                                   const float* const* grad_out, int32_t k, const float* weights, float* grad_weights,
                                   float* const* grad_in, const float* const* fwd_out, const die_nca_dropout* drop,
                                   int32_t padding_mode, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "die_conv2d_backward";
    DIE_REQUIRE(padding_mode >= DIE_PAD_CIRCULAR && padding_mode <= DIE_PAD_REPLICATE, "%s: bad padding mode %d", who, padding_mode);
    if (die_nca_pad_adjoint_check(padding_mode, who) != DIE_OK) return DIE_ERR_UNSUPPORTED;
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE(cin >= 1 && cin <= NCA_MAXC && cout >= 1 && cout <= NCA_MAXC, "%s: 1..%d channels (got %d -> %d)", who, NCA_MAXC, cin, cout);
    if (!(k == 1 || k == 3 || k == 5 || k == 7)) {
        die_set_error("%s: kernel size %d (odd sizes up to %d)", who, k, NCA_MAXK);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(in && grad_out && weights && grad_weights && workspace, "%s: null argument", who);
    DIE_REQUIRE(grad_weights != weights, "%s: grad_weights is the weights", who);
    DIE_REQUIRE(fwd_out || !drop, "%s: a dropout mask without the forward outputs it was applied to", who);
    const int64_t need = die_conv2d_backward_workspace_bytes(W, H, cin, cout, k);
    DIE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)workspace_bytes, (long long)need);
    ConvBwdArgs a = {};
    for (int c = 0; c < cin; ++c) {
        DIE_REQUIRE(in[c].data && in[c].kind >= DIE_PLANE_F32 && in[c].kind <= DIE_PLANE_AGENTS, "%s: bad input plane %d", who, c);
        a.in[c] = in[c].data; a.kind[c] = in[c].kind;
        if (grad_in) {
            DIE_REQUIRE(grad_in[c], "%s: null grad_in plane %d", who, c);
            a.gin[c] = grad_in[c];
        }
    }
    for (int o = 0; o < cout; ++o) {
        DIE_REQUIRE(grad_out[o], "%s: null gradient plane %d", who, o);
        a.g[o] = grad_out[o];
        if (fwd_out) {
            DIE_REQUIRE(fwd_out[o], "%s: null forward output plane %d", who, o);
            a.t[o] = fwd_out[o];
        }
    }
    if (grad_in) {
        for (int c = 0; c < cin; ++c) {
            bool alias = false;
            for (int q = 0; q < cin; ++q) alias |= (const void*)grad_in[c] == in[q].data || (q != c && grad_in[c] == grad_in[q]);
            for (int o = 0; o < cout; ++o) alias |= grad_in[c] == grad_out[o] || (fwd_out && grad_in[c] == fwd_out[o]);
            DIE_REQUIRE(!alias, "%s: in-place grad_in (plane %d is one of the call's other planes)", who, c);
        }
    }
    DropWords dw = {};
    if (drop) {
        const int rc = die_dropout_words(drop, &dw, who);
        if (rc != DIE_OK) return rc;
    }
    a.w = weights; a.part = (float*)workspace;
    a.W = W; a.H = H; a.cin = cin; a.cout = cout; a.epoch = epoch; a.pad = padding_mode;
    a.has_t = fwd_out != nullptr; a.has_drop = drop != nullptr; a.has_gin = grad_in != nullptr;
    a.d = dw;
    const int R = k / 2, nw = cout * cin * k * k;
    const size_t lds = ((size_t)(cin + cout) * (NCA_TX + 2 * R) * (NCA_TY + 2 * R + 1) + (size_t)nw) * sizeof(float);
    dim3 grid((H + NCA_TY - 1) / NCA_TY, (W + NCA_TX - 1) / NCA_TX);
    DIE_REQUIRE(grid.y <= 65535u, "%s: field too tall (%d rows of tiles)", who, (int)grid.y);
    hipStream_t s = (hipStream_t)stream;
    switch (k) {
        case 1: k_conv_backward<1><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        case 3: k_conv_backward<3><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        case 5: k_conv_backward<5><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        default: k_conv_backward<7><<<grid, DIE_BLOCK, lds, s>>>(a); break;
    }
    DIE_CHECK_LAUNCH(who);
    k_conv_backward_sum<<<die_grid_for(nw), DIE_BLOCK, 0, s>>>(a.part, die_nca_tiles(W, H), nw, grad_weights);
    DIE_CHECK_LAUNCH("die_conv2d_backward(sum)");
    return DIE_OK;
}

// ---- the read-out's adjoint --------------------------------------------------------------------------------------------
struct GatherBwdArgs {
    die_geo g;
    int64_t N;
    const uint32_t *x, *y;
    const float* grad[3];
    float coef[3];
    float* plane[3];
};

// slot n: its gradient times the coefficients, added to the three planes at its cell
__device__ __forceinline__ void gather_scale_backward_one(const GatherBwdArgs& a, int64_t n) {
    const int64_t c = die_local(a.g, die_cell((int64_t)a.x[n], a.g.gW), die_cell((int64_t)a.y[n], a.g.gH));
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float v = a.grad[q][n] * a.coef[q];
        if (v != 0.f) atomicAdd(&a.plane[q][c], v);          // (a zero term changes no sum: dead slots with no gradient cost nothing)
    }
}

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_scale_backward(GatherBwdArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) gather_scale_backward_one(a, n);
}

// die_gather_scale_backward_batch: replica blockIdx.y — its planes `rep_plane` elements on, its slots `agents` on, n[r] of them
struct GatherBwdBatchArgs : GatherBwdArgs {
    int64_t rep_plane, agents;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_scale_backward_batch(GatherBwdBatchArgs b) {
    const int r = blockIdx.y;
    const int64_t pa = b.agents * r;
    GatherBwdArgs a = b;
    a.N = b.n[r]; a.x += pa; a.y += pa;
#pragma unroll
    for (int q = 0; q < 3; ++q) { a.grad[q] += pa; a.plane[q] += b.rep_plane * r; }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) gather_scale_backward_one(a, n);
}

extern "C" int die_gather_scale_backward(const die_medium* m, const die_agents* ag, const die_action* grad_action, const float* coefs,
                                         float* const* grad_planes, void* stream) {
    const char* who = "die_gather_scale_backward";
    DIE_REQUIRE(m && ag && grad_action && coefs && grad_planes, "%s: null argument", who);
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    DIE_REQUIRE(ag->N > 0 && grad_action->N == ag->N && ag->x && ag->y && grad_action->dx && grad_action->dy && grad_action->deposit,
                "%s: bad arrays", who);
    GatherBwdArgs a;
    a.g = die_geo_of(m); a.N = ag->N; a.x = ag->x; a.y = ag->y;
    a.grad[0] = grad_action->dx; a.grad[1] = grad_action->dy; a.grad[2] = grad_action->deposit;
    for (int q = 0; q < 3; ++q) {
        DIE_REQUIRE(grad_planes[q], "%s: null plane %d", who, q);
        for (int p = 0; p < q; ++p) DIE_REQUIRE(grad_planes[p] != grad_planes[q], "%s: planes %d and %d are one", who, p, q);
        a.plane[q] = grad_planes[q]; a.coef[q] = coefs[q];
    }
    const size_t bytes = (size_t)m->W * m->H * sizeof(float);
    for (int q = 0; q < 3; ++q) {
        if (hipMemsetAsync(a.plane[q], 0, bytes, (hipStream_t)stream) != hipSuccess) {
            die_set_error("%s: clearing plane %d failed", who, q);
            return DIE_ERR_HIP;
        }
    }
    const int64_t g = (ag->N + DIE_BLOCK - 1) / DIE_BLOCK;
    k_gather_scale_backward<<<(int)(g < 8192 ? g : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_gather_scale_backward_batch(const die_medium* m, const die_agents* ag, const die_batch* b, const die_action* grad_action,
                                               const float* coefs, float* grad_sense, int64_t sense_stride, void* stream) {
    const char* who = "die_gather_scale_backward_batch";
    DIE_REQUIRE(m && ag && b && grad_action && coefs && grad_sense, "%s: null argument", who);
    int rc = die_nca_batch_shape_check(m, b, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    DIE_REQUIRE(sense_stride >= 3 * cells, "%s: sense_stride %lld below three planes", who, (long long)sense_stride);
    DIE_REQUIRE(ag->x && ag->y && grad_action->dx && grad_action->dy && grad_action->deposit, "%s: bad arrays", who);
    GatherBwdBatchArgs a;
    a.g = die_geo_of(m); a.N = 0; a.x = ag->x; a.y = ag->y;
    a.grad[0] = grad_action->dx; a.grad[1] = grad_action->dy; a.grad[2] = grad_action->deposit;
    for (int q = 0; q < 3; ++q) { a.plane[q] = grad_sense + q * cells; a.coef[q] = coefs[q]; }
    a.rep_plane = sense_stride; a.agents = b->agent_stride;
    int64_t nmax = die_replica_counts(a.n, b->n, b->replicas);
    if (nmax < 1) nmax = 1;
    // the 3 · R planes (and what lies between two replicas' planes where sense_stride leaves a gap)
    const size_t span = (size_t)((int64_t)(b->replicas - 1) * sense_stride + 3 * cells) * sizeof(float);
    if (hipMemsetAsync(grad_sense, 0, span, (hipStream_t)stream) != hipSuccess) {
        die_set_error("%s: clearing the planes failed", who);
        return DIE_ERR_HIP;
    }
    const int64_t g = (nmax + DIE_BLOCK - 1) / DIE_BLOCK;
    k_gather_scale_backward_batch<<<dim3((unsigned)(g < 8192 ? g : 8192), (unsigned)b->replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the conv stack's adjoint for every replica of a batch ---------------------------------------------------------------
// Workspace: [replica][tile][4 · 4 · 7 · 7] partial rows at most (a layer uses [replica][tile][cout · cin · k · k] of it), then
// min(layers − 1, 2) sets of [replica][4][W][H] planes for the gradient travelling down the stack (ping-pong).
static int64_t nca_backward_part_floats(int32_t W, int32_t H, int32_t replicas) {
    return (int64_t)replicas * die_nca_tiles(W, H) * NCA_MAXC * NCA_MAXC * NCA_MAXK * NCA_MAXK;
}

extern "C" int64_t die_nca_backward_batch_workspace_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS || n_layers < 1 || n_layers > DIE_NCA_MAX_LAYERS) return -1;
    if ((W + NCA_TX - 1) / NCA_TX > 65535) return -1;
    return (nca_backward_part_floats(W, H, replicas) + (int64_t)die_nca_gin_sets(n_layers) * replicas * NCA_MAXC * (int64_t)W * H) *
           (int64_t)sizeof(float);
}

// die_nca_backward_batch (grad_in null) and die_nca_backward_batch_inputs: one body.  grad_in: layer 0's launch also writes the
// gradient at its cin input planes (has_gin, as the layers above it do into the workspace), replica r's at grad_in + r * grad_in_stride
static int nca_backward_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                              const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                              const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                              int64_t grad_in_stride, void* stream, const char* who) {
    DIE_REQUIRE(m && b && nca && store && grad_sense && grad && workspace, "%s: null argument", who);
    int rc = die_nca_batch_shape_check(m, b, who);
    if (rc != DIE_OK) return rc;
    rc = die_nca_stack_check(DIE_NCA_NARROW, nca, m->W, m->H, b->replicas, who, false);
    if (rc == DIE_OK) rc = die_nca_pad_adjoint_check(nca->padding_mode, who);
    if (rc == DIE_OK) rc = die_nca_field_check(m, nca, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H, rep_planes = NCA_MAXC * cells;
    DIE_REQUIRE(sense_stride >= 3 * cells, "%s: sense_stride %lld below three planes", who, (long long)sense_stride);
    int64_t P = 0;
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        P += (int64_t)L.cout * L.cin * L.k * L.k;
        DIE_REQUIRE(grad != L.weights, "%s: grad is layer %d's weights", who, l);
    }
    DIE_REQUIRE(grad_stride >= P, "%s: grad_stride %lld below a row of %lld weights", who, (long long)grad_stride, (long long)P);
    const int64_t need = die_nca_backward_batch_workspace_bytes(m->W, m->H, b->replicas, nca->n_layers);
    DIE_REQUIRE(need > 0, "%s: field too tall", who);
    DIE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)workspace_bytes, (long long)need);
    if (grad_in) {
        const int64_t in_planes = (int64_t)nca->layers[0].cin * cells;
        DIE_REQUIRE(grad_in_stride >= in_planes, "%s: grad_in_stride %lld below the first layer's %d input planes", who,
                    (long long)grad_in_stride, nca->layers[0].cin);
        // the kernel stores four cells of a row at once where H % 4 == 0
        DIE_REQUIRE(m->H % 4 != 0 || (((uintptr_t)grad_in & 15) == 0 && grad_in_stride % 4 == 0),
                    "%s: grad_in must be 16-byte aligned and grad_in_stride a multiple of 4 where H %% 4 == 0", who);
        const char* lo = (const char*)grad_in;
        const char* hi = lo + ((int64_t)(b->replicas - 1) * grad_in_stride + in_planes) * (int64_t)sizeof(float);
        auto inside = [&](const void* q) { return q && (const char*)q >= lo && (const char*)q < hi; };
        const char* ws_hi = (const char*)workspace + need;
        DIE_REQUIRE(!inside(store) && !inside(grad_sense) && !inside(grad) && !inside(workspace) && !inside(m->owner) && !inside(m->food) &&
                        !inside(m->chem) && !((const char*)workspace <= lo && lo < ws_hi),
                    "%s: grad_in aliases another buffer of the call", who);
        for (int l = 0; l < nca->n_layers; ++l) DIE_REQUIRE(!inside(nca->layers[l].weights), "%s: grad_in aliases layer %d's weights", who, l);
    }
    DropWords dw = {};
    if (drop) {
        rc = die_dropout_words(drop, &dw, who);
        if (rc != DIE_OK) return rc;
    }
    const int E = nca->episodes > 1 ? nca->episodes : 1, R = b->replicas, L = nca->n_layers;
    const int64_t tiles = die_nca_tiles(m->W, m->H);
    float* part = (float*)workspace;
    float* gin_sets = part + nca_backward_part_floats(m->W, m->H, R);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((m->H + NCA_TY - 1) / NCA_TY, (m->W + NCA_TX - 1) / NCA_TX, R);
    int64_t off = P;
    const float* g = grad_sense;
    int64_t rep_g = sense_stride;
    for (int l = L - 1; l >= 0; --l) {
        const die_nca_layer& Ly = nca->layers[l];
        const int nw = Ly.cout * Ly.cin * Ly.k * Ly.k;
        off -= nw;
        ConvBwdBatchArgs a = {};
        if (l == 0) {
            die_nca_layer0_planes(m, b, nca, nullptr, 0, nullptr, a.in, a.kind, &a.rep_in);
        } else {
            for (int c = 0; c < Ly.cin; ++c) { a.in[c] = store + (int64_t)(l - 1) * R * rep_planes + c * cells; a.kind[c] = DIE_PLANE_F32; }
            a.rep_in = rep_planes;
        }
        float* gin = l > 0 ? gin_sets + (int64_t)((L - 1 - l) % 2) * R * rep_planes : grad_in;
        for (int c = 0; c < Ly.cin && gin; ++c) a.gin[c] = gin + c * cells;
        for (int o = 0; o < Ly.cout; ++o) {
            a.g[o] = g + o * cells;
            if (l == L - 1) a.t[o] = store + (int64_t)l * R * rep_planes + o * cells;
        }
        a.rep_g = rep_g; a.rep_t = rep_planes; a.rep_gin = l > 0 ? rep_planes : grad_in_stride;
        a.w = Ly.weights; a.rep_w = Ly.weight_stride; a.episodes = E;
        a.part = part; a.rep_part = tiles * nw;
        a.W = m->W; a.H = m->H; a.cin = Ly.cin; a.cout = Ly.cout; a.epoch = nca->sense_epoch; a.pad = nca->padding_mode;
        a.has_t = l == L - 1; a.has_drop = drop != nullptr && l == L - 1; a.has_gin = gin != nullptr;
        a.d = dw;
        const int Rk = Ly.k / 2;
        const size_t lds = ((size_t)(Ly.cin + Ly.cout) * (NCA_TX + 2 * Rk) * (NCA_TY + 2 * Rk + 1) + (size_t)nw) * sizeof(float);
        switch (Ly.k) {
            case 1: k_conv_backward<1, true><<<grid, DIE_BLOCK, lds, s>>>(a); break;
            case 3: k_conv_backward<3, true><<<grid, DIE_BLOCK, lds, s>>>(a); break;
            case 5: k_conv_backward<5, true><<<grid, DIE_BLOCK, lds, s>>>(a); break;
            default: k_conv_backward<7, true><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        }
        DIE_CHECK_LAUNCH(who);
        k_conv_backward_sum_batch<<<dim3((unsigned)die_grid_for(nw), (unsigned)(R / E)), DIE_BLOCK, 0, s>>>(part, (int64_t)E * tiles, nw, grad + off,
                                                                                                    grad_stride);
        DIE_CHECK_LAUNCH("die_nca_backward_batch(sum)");
        g = gin; rep_g = rep_planes;
    }
    return DIE_OK;
}

extern "C" int die_nca_backward_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                      const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                      const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream) {
    return nca_backward_batch(m, b, nca, store, grad_sense, sense_stride, grad, grad_stride, drop, workspace, workspace_bytes, nullptr, 0,
                              stream, "die_nca_backward_batch");
}

extern "C" int die_nca_backward_batch_inputs(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                             const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                             const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                             int64_t grad_in_stride, void* stream) {
    const char* who = "die_nca_backward_batch_inputs";
    DIE_REQUIRE(grad_in, "%s: null argument (grad_in)", who);
    return nca_backward_batch(m, b, nca, store, grad_sense, sense_stride, grad, grad_stride, drop, workspace, workspace_bytes, grad_in,
                              grad_in_stride, stream, who);
}
