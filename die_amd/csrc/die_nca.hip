// NeuralAutomataAgent sensing (gfx950) — core/agent/evo.py:45-118 (ConvolutionModel: a stack of bias-free Conv2d with
// 'same' padding — `boundary` = torch's padding_mode: 'circular' by default, 'zeros' / 'reflect' / 'replicate' —, one Tanh at the end) and :150-174 (forward: per-agent gather of the transformed medium at
// the agent's cell, core/utils.py:56-65, times the action coefficients).
//
//   k_conv_circular   one layer: out[o, x, y] = Σ_i Σ_a Σ_b w[o, i, a, b] · in[i, (x + a − r) mod W, (y + b − r) mod H]
//                     (torch's Conv2d is a cross-correlation; medium axes are (channel, x, y), so kernel rows run along
//                     x).  A workgroup stages the (16 + 2r) × (64 + 2r) input tile of every input channel in LDS and the
//                     layer's weights next to it; a thread produces 4 consecutive y of every output channel (16-byte
//                     stores).  The first layer reads the medium's own planes: fp32 / fp16 fields, and the 'agents'
//                     channel straight from the claim plane (occupied ⇔ epoch tag) — and, for an agent that senses its own
//                     stock, the stock plane of die_stock.hip (DIE_PLANE_STOCK: occupied ? payload : 0).  The last layer applies tanh.
//   k_gather_scale    action[c, n] = plane[c][cell(x_n), cell(y_n)] · coef[c] for EVERY slot (only_alive = False).
//                     k_gather_scale_batch (die_gather_scale_batch, replica in blockIdx.y) calls the same gather_scale_one.
//   die_nca_env_step_batch (a population of candidates on batched replicas) runs k_conv_circular<K, true>: the same body
//                     with the replica in blockIdx.z (its planes, weights and outputs one stride further each); the read-out
//                     and the step half are k_nca_move_claim_batch in die_env.hip.
//   DROP              (k_conv_circular<K, BATCH, true>, the last layer of a stack whose agent dropout is on: die_conv2d_dropout,
//                     die_nca_env_step_batch_dropout) multiplies the layer's outputs by the cells' dropout mask of die_rng.h in
//                     the epilogue — one mask per (W, H) plane, shared by the output channels; nothing is stored for it.
//   k_dropout_mask    the mask planes themselves (die_dropout_mask): 0 or keep per cell, for looking at and for the tests.
//   Host rules shared with die_nca_wide.hip and the two adjoint files (declared in die_nca.h, each defined once): here layer 0's input
//                     list (die_nca_layer0_planes), the read-out's die_batch (die_nca_batch_shape_check), the field's planes
//                     (die_nca_field_check), the paddings without an adjoint (die_nca_pad_adjoint_check) and the store calls' checks
//                     (die_nca_store_check); the stack's own rules, narrow and wide (die_nca_stack_check): die_nca_wide.hip.
//
// Roofline: HBM.  A 3→3 channel 3×3 layer is 81 MAC per cell against 24 bytes per cell (3 planes in, 3 out): 6.75 flop
// per byte, far below the ≈ 20 flop/byte at which fp32 vector math (157 TFLOP/s) meets 8 TB/s — no MFMA: the matrix
// cores would sit idle behind the same memory stream.
#include <math.h>
#include <type_traits>
#include "die_common.h"
#include "die_rng.h"
#include "die_nca.h"

struct ConvArgs {
    const void* in[NCA_MAXC];
    int kind[NCA_MAXC];          // die_conv_plane.kind
    float* out[NCA_MAXC];
    const float* w;              // [cout][cin][k][k]
    int W, H, cin, cout, k, epoch, apply_tanh;
    int pad;                     // die_pad_mode: how cells beyond the field are read ('same' padding of torch's Conv2d)
    int64_t rep_in, rep_w, rep_out;  // batch (gridDim.z = replicas): elements from replica r's planes / weights to r + 1's
    int episodes;                // batch: replica r reads weight row r / episodes (1: a row per replica)
};
// what a DROP launch reads on top (the other instantiations keep ConvArgs as their whole argument)
struct ConvDropArgs : ConvArgs { DropWords d; };

// (nca_pad_index — which cell stands in for one beyond the field — and nca_load — a first-layer plane's element — : die_nca.h)

// BATCH: replica blockIdx.z of die_nca_env_step_batch — its input planes, weights and output planes lie blockIdx.z strides
// on; everything else (tile, LDS, summation order, tanh) is this one body.  With episodes E > 1 (a candidate evaluated on E
// worlds) the E replicas of a candidate share one weight row: row r / E, uniform over the workgroup (one scalar division).
//
// DROP: the epilogue multiplies by the dropout mask.  A thread owns 4 consecutive y from a multiple of 4; with H % 4 == 0 their
// cells ix·H + iy … + 3 are one Philox block (one die_philox per thread, after the accumulation, before the stores); with any
// other H (stand-alone layers only) the words are evaluated cell by cell — the same mask either way.
template <int K, bool BATCH = false, bool DROP = false>
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_circular(typename std::conditional<DROP, ConvDropArgs, ConvArgs>::type a) {
    constexpr int R = K / 2, LX = NCA_TX + 2 * R, LY = NCA_TY + 2 * R + 1;     // odd pitch: conflict-free column walks
    extern __shared__ __align__(16) float nca_smem[];
    float* s_in = nca_smem;                                  // [cin][LX][LY]
    float* s_w = nca_smem + a.cin * LX * LY;                 // [cout][cin][K][K]
    const int x0 = blockIdx.y * NCA_TX, y0 = blockIdx.x * NCA_TY;
    const int64_t rep = BATCH ? (int64_t)blockIdx.z : 0;
    const int64_t row = (BATCH && a.episodes > 1) ? (int64_t)((int)blockIdx.z / a.episodes) : rep;
    const float* w = a.w + row * a.rep_w;
    const int nw = a.cout * a.cin * K * K;
    for (int i = threadIdx.x; i < nw; i += DIE_BLOCK) s_w[i] = w[i];
    constexpr int LYV = NCA_TY + 2 * R;
    for (int c = 0; c < a.cin; ++c) {
        for (int i = threadIdx.x; i < LX * LYV; i += DIE_BLOCK) {
            const int li = i / LYV, lj = i - li * LYV;
            // (rows / columns past the last tile's outputs wrap like a circular field whatever the mode: never used)
            const int vx = x0 - R + li, vy = y0 - R + lj;
            const int gx = nca_pad_index(vx < a.W + R ? vx : vx % a.W, a.W, a.pad), gy = nca_pad_index(vy < a.H + R ? vy : vy % a.H, a.H, a.pad);
            s_in[(c * LX + li) * LY + lj] = (gx < 0 || gy < 0) ? 0.f : nca_load(a.in[c], a.kind[c], rep * a.rep_in + (int64_t)gx * a.H + gy, a.epoch);
        }
    }
    __syncthreads();
    const int ti = threadIdx.x / (NCA_TY / 4), tj = (threadIdx.x % (NCA_TY / 4)) * 4;     // 16 rows × 16 column quads
    float acc[NCA_MAXC][4];
#pragma unroll
    for (int o = 0; o < NCA_MAXC; ++o) acc[o][0] = acc[o][1] = acc[o][2] = acc[o][3] = 0.f;
    for (int c = 0; c < a.cin; ++c) {
#pragma unroll
        for (int ka = 0; ka < K; ++ka) {
            float row[4 + K - 1];
#pragma unroll
            for (int q = 0; q < 4 + K - 1; ++q) row[q] = s_in[(c * LX + ti + ka) * LY + tj + q];
#pragma unroll
            for (int o = 0; o < NCA_MAXC; ++o) {
                if (o < a.cout) {
#pragma unroll
                    for (int kb = 0; kb < K; ++kb) {
                        const float wv = s_w[((o * a.cin + c) * K + ka) * K + kb];
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[o][q] += wv * row[q + kb];
                    }
                }
            }
        }
    }
    const int gx = x0 + ti, gy = y0 + tj;
    if (gx >= a.W) return;
    float mask[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (DROP) {
        if (gy >= a.H) return;
        const uint64_t key = a.d.seed + (uint64_t)blockIdx.z * a.d.seed_stride;
        const uint64_t cell = (uint64_t)gx * (uint64_t)a.H + (uint64_t)gy;
        if ((a.H & 3) == 0) {
            const die_u32x4 r = die_draw(key, a.d.step, cell >> 2, DIE_STREAM_DROPOUT);
#pragma unroll
            for (int q = 0; q < 4; ++q) mask[q] = die_dropout_factor(r.v[q], a.d.thr, a.d.keep);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (gy + q < a.H) mask[q] = die_dropout_factor(die_dropout_word(key, a.d.step, cell + q), a.d.thr, a.d.keep);
        }
    }
#pragma unroll
    for (int o = 0; o < NCA_MAXC; ++o) {
        if (o < a.cout) {
            float v[4] = {acc[o][0], acc[o][1], acc[o][2], acc[o][3]};
            if (a.apply_tanh) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tanhf(v[q]);
            }
            if constexpr (DROP) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] * mask[q];
            }
            float* dst = a.out[o] + rep * a.rep_out + (int64_t)gx * a.H + gy;
            if (gy + 3 < a.H && (a.H & 3) == 0) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (gy + q < a.H) dst[q] = v[q];
            }
        }
    }
}

// `drop` (checked: die_dropout_words): the layer's outputs times the dropout mask, the DROP instantiation
template <bool BATCH>
static void launch_conv(const ConvArgs& a, int replicas, hipStream_t s, const DropWords* drop = nullptr) {
    const int R = a.k / 2;
    const size_t lds = ((size_t)a.cin * (NCA_TX + 2 * R) * (NCA_TY + 2 * R + 1) + (size_t)a.cout * a.cin * a.k * a.k) * sizeof(float);
    dim3 grid((a.H + NCA_TY - 1) / NCA_TY, (a.W + NCA_TX - 1) / NCA_TX, replicas);
    if (drop) {
        ConvDropArgs da;
        static_cast<ConvArgs&>(da) = a;
        da.d = *drop;
        switch (a.k) {
            case 1: k_conv_circular<1, BATCH, true><<<grid, DIE_BLOCK, lds, s>>>(da); break;
            case 3: k_conv_circular<3, BATCH, true><<<grid, DIE_BLOCK, lds, s>>>(da); break;
            case 5: k_conv_circular<5, BATCH, true><<<grid, DIE_BLOCK, lds, s>>>(da); break;
            default: k_conv_circular<7, BATCH, true><<<grid, DIE_BLOCK, lds, s>>>(da); break;
        }
        return;
    }
    switch (a.k) {
        case 1: k_conv_circular<1, BATCH><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        case 3: k_conv_circular<3, BATCH><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        case 5: k_conv_circular<5, BATCH><<<grid, DIE_BLOCK, lds, s>>>(a); break;
        default: k_conv_circular<7, BATCH><<<grid, DIE_BLOCK, lds, s>>>(a); break;
    }
}

extern "C" int die_conv2d_circular(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                                   float* const* out, int32_t k, const float* weights, int32_t apply_tanh, void* stream) {
    return die_conv2d(W, H, cin, in, epoch, cout, out, k, weights, apply_tanh, DIE_PAD_CIRCULAR, stream);
}

// die_nca_dropout, checked, as the words the kernels read
int die_dropout_words(const die_nca_dropout* drop, DropWords* out, const char* who) {
    DIE_REQUIRE(drop, "%s: null dropout", who);
    DIE_REQUIRE(drop->p > 0.0 && drop->p <= 1.0, "%s: dropout p = %g: 0 < p <= 1 (p = 0 is the call without a mask)", who, drop->p);   // (NaN fails both)
    DIE_REQUIRE(drop->reserved == 0, "%s: die_nca_dropout.reserved must be 0", who);
    out->seed = drop->seed; out->seed_stride = drop->seed_stride; out->step = drop->step;
    out->thr = (uint64_t)ceil(drop->p * 4294967296.0);
    out->keep = (float)(1.0 / (1.0 - drop->p));            // (p = 1: inf, never read: every word is below thr = 2^32)
    return DIE_OK;
}

static int conv2d(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout, float* const* out, int32_t k,
                  const float* weights, int32_t apply_tanh, int32_t padding_mode, const die_nca_dropout* drop, void* stream) {
    DIE_REQUIRE(padding_mode >= DIE_PAD_CIRCULAR && padding_mode <= DIE_PAD_REPLICATE, "die_conv2d: bad padding mode %d", padding_mode);
    if (padding_mode == DIE_PAD_REFLECT && (k / 2 >= W || k / 2 >= H)) {      // (torch refuses it too)
        die_set_error("die_conv2d: 'reflect' padding of %d cells needs a field larger than that (%dx%d)", k / 2, W, H);
        return DIE_ERR_ARG;
    }
    DIE_REQUIRE(W >= 1 && H >= 1, "die_conv2d_circular: bad size %dx%d", W, H);
    DIE_REQUIRE(cin >= 1 && cin <= NCA_MAXC && cout >= 1 && cout <= NCA_MAXC, "die_conv2d_circular: 1..%d channels (got %d -> %d)",
                NCA_MAXC, cin, cout);
    if (!(k == 1 || k == 3 || k == 5 || k == 7)) {
        die_set_error("die_conv2d_circular: kernel size %d (odd sizes up to %d: 'same' padding of an even kernel is asymmetric)", k, NCA_MAXK);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(in && out && weights, "die_conv2d_circular: null argument");
    ConvArgs a;
    for (int c = 0; c < NCA_MAXC; ++c) {
        a.in[c] = c < cin ? in[c].data : nullptr;
        a.kind[c] = c < cin ? in[c].kind : 0;
        a.out[c] = c < cout ? out[c] : nullptr;
        // (a stock plane is the observation's LAST channel, DESIGN §6: kind 3 anywhere else is a plane of no kind, as it always was)
        DIE_REQUIRE(c >= cin || (in[c].data && in[c].kind >= DIE_PLANE_F32 && in[c].kind <= (c == cin - 1 ? DIE_PLANE_STOCK : DIE_PLANE_AGENTS)),
                    "die_conv2d_circular: bad input plane %d", c);
        DIE_REQUIRE(c >= cout || out[c], "die_conv2d_circular: null output plane %d", c);
        for (int q = 0; q < cout && c < cin; ++q) DIE_REQUIRE((const void*)out[q] != in[c].data, "die_conv2d_circular: in-place convolution");
    }
    a.w = weights; a.W = W; a.H = H; a.cin = cin; a.cout = cout; a.k = k; a.epoch = epoch; a.apply_tanh = apply_tanh; a.pad = padding_mode;
    a.rep_in = a.rep_w = a.rep_out = 0;
    a.episodes = 1;
    DropWords dw;
    if (drop) {
        const int rc = die_dropout_words(drop, &dw, "die_conv2d_dropout");
        if (rc != DIE_OK) return rc;
    }
    launch_conv<false>(a, 1, (hipStream_t)stream, drop ? &dw : nullptr);
    DIE_CHECK_LAUNCH("die_conv2d_circular");
    return DIE_OK;
}

extern "C" int die_conv2d(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                          float* const* out, int32_t k, const float* weights, int32_t apply_tanh, int32_t padding_mode, void* stream) {
    return conv2d(W, H, cin, in, epoch, cout, out, k, weights, apply_tanh, padding_mode, nullptr, stream);
}

extern "C" int die_conv2d_dropout(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                                  float* const* out, int32_t k, const float* weights, int32_t apply_tanh, int32_t padding_mode,
                                  const die_nca_dropout* drop, void* stream) {
    return conv2d(W, H, cin, in, epoch, cout, out, k, weights, apply_tanh, padding_mode, drop, stream);
}

// one thread per Philox block: cells 4i … 4i + 3 of replica blockIdx.y's plane
__global__ __launch_bounds__(DIE_BLOCK) void k_dropout_mask(DropWords d, int64_t cells, int64_t plane_stride, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * i >= cells) return;
    const die_u32x4 r = die_draw(d.seed + (uint64_t)blockIdx.y * d.seed_stride, d.step, (uint64_t)i, DIE_STREAM_DROPOUT);
    float* dst = out + (int64_t)blockIdx.y * plane_stride + 4 * i;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (4 * i + q < cells) dst[q] = die_dropout_factor(r.v[q], d.thr, d.keep);
}

extern "C" int die_dropout_mask(int32_t W, int32_t H, const die_nca_dropout* drop, int32_t replicas, int64_t plane_stride, float* out,
                                void* stream) {
    const char* who = "die_dropout_mask";
    DIE_REQUIRE(drop && out, "%s: null argument", who);
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE(replicas >= 1 && replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas (got %d)", who, DIE_MAX_REPLICAS, replicas);
    const int64_t cells = (int64_t)W * H;
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    DropWords dw;
    const int rc = die_dropout_words(drop, &dw, who);
    if (rc != DIE_OK) return rc;
    const int64_t blocks = ((cells + 3) / 4 + DIE_BLOCK - 1) / DIE_BLOCK;
    DIE_REQUIRE(blocks <= 0x7FFFFFFF, "%s: plane too large", who);
    k_dropout_mask<<<dim3((unsigned)blocks, (unsigned)replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(dw, cells, plane_stride, out);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

struct GatherArgs {
    die_geo g;
    int64_t N;
    const uint32_t *x, *y;
    const float* plane[3];
    float coef[3];
    float* out[3];
};

// slot n: the three planes at its cell, each times its coefficient
__device__ __forceinline__ void gather_scale_one(const GatherArgs& a, int64_t n) {
    const int64_t c = die_local(a.g, die_cell((int64_t)a.x[n], a.g.gW), die_cell((int64_t)a.y[n], a.g.gH));
#pragma unroll
    for (int q = 0; q < 3; ++q) a.out[q][n] = a.plane[q][c] * a.coef[q];
}

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_scale(GatherArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < a.N; n += stride) gather_scale_one(a, n);
}

// die_gather_scale_batch: replica blockIdx.y — its planes `rep_plane` elements on, its slots `agents` on; slots n[r] … agents − 1
// (the padding of a replica with fewer agents than the widest) read as 0
struct GatherBatchArgs : GatherArgs {
    int64_t rep_plane, agents;
    int64_t n[DIE_MAX_REPLICAS];
};

__global__ __launch_bounds__(DIE_BLOCK) void k_gather_scale_batch(GatherBatchArgs b) {
    const int r = blockIdx.y;
    const int64_t pa = b.agents * r, nr = b.n[r];
    GatherArgs a = b;
    a.x += pa; a.y += pa;
#pragma unroll
    for (int q = 0; q < 3; ++q) { a.plane[q] += b.rep_plane * r; a.out[q] += pa; }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < b.agents; n += stride) {
        if (n < nr) {
            gather_scale_one(a, n);
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) a.out[q][n] = 0.f;
        }
    }
}

extern "C" int die_gather_scale(const die_medium* m, const die_agents* ag, const float* const* planes, const float* coefs,
                                const die_action* out, void* stream) {
    DIE_REQUIRE(m && ag && planes && coefs && out, "die_gather_scale: null argument");
    DIE_REQUIRE(ag->N > 0 && out->N == ag->N && ag->x && ag->y && out->dx && out->dy && out->deposit, "die_gather_scale: bad arrays");
    GatherArgs a;
    a.g = die_geo_of(m); a.N = ag->N; a.x = ag->x; a.y = ag->y;
    for (int q = 0; q < 3; ++q) { a.plane[q] = planes[q]; a.coef[q] = coefs[q]; DIE_REQUIRE(planes[q], "die_gather_scale: null plane %d", q); }
    a.out[0] = out->dx; a.out[1] = out->dy; a.out[2] = out->deposit;
    int64_t g = (ag->N + DIE_BLOCK - 1) / DIE_BLOCK;
    k_gather_scale<<<(int)(g < 8192 ? g : 8192), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH("die_gather_scale");
    return DIE_OK;
}

// what the batched read-out and its adjoint require of a die_batch (die_nca_grad.hip uses it too)
int die_nca_batch_shape_check(const die_medium* m, const die_batch* b, const char* who) {
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    DIE_REQUIRE(b->replicas >= 1 && b->replicas <= DIE_MAX_REPLICAS, "%s: 1..%d replicas (got %d)", who, DIE_MAX_REPLICAS, b->replicas);
    DIE_REQUIRE(b->plane_stride >= (int64_t)m->W * m->H, "%s: plane_stride %lld smaller than a plane", who, (long long)b->plane_stride);
    DIE_REQUIRE(b->agent_stride >= 1, "%s: agent_stride %lld", who, (long long)b->agent_stride);
    for (int r = 0; r < b->replicas; ++r)
        DIE_REQUIRE(b->n[r] >= 0 && b->n[r] <= b->agent_stride, "%s: replica %d has %lld agents", who, r, (long long)b->n[r]);
    return DIE_OK;
}

extern "C" int die_gather_scale_batch(const die_medium* m, const die_agents* ag, const die_batch* b, const float* sense, int64_t sense_stride,
                                      const float* coefs, const die_action* out, void* stream) {
    const char* who = "die_gather_scale_batch";
    DIE_REQUIRE(m && ag && b && sense && coefs && out, "%s: null argument", who);
    int rc = die_nca_batch_shape_check(m, b, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    DIE_REQUIRE(sense_stride >= 3 * cells, "%s: sense_stride %lld below three planes", who, (long long)sense_stride);
    DIE_REQUIRE(ag->x && ag->y && out->dx && out->dy && out->deposit, "%s: bad arrays", who);
    GatherBatchArgs a;
    a.g = die_geo_of(m); a.N = b->agent_stride; a.x = ag->x; a.y = ag->y;
    for (int q = 0; q < 3; ++q) { a.plane[q] = sense + q * cells; a.coef[q] = coefs[q]; }
    a.out[0] = out->dx; a.out[1] = out->dy; a.out[2] = out->deposit;
    a.rep_plane = sense_stride; a.agents = b->agent_stride;
    die_replica_counts(a.n, b->n, b->replicas);
    const int64_t g = (b->agent_stride + DIE_BLOCK - 1) / DIE_BLOCK;
    k_gather_scale_batch<<<dim3((unsigned)(g < 8192 ? g : 8192), (unsigned)b->replicas), DIE_BLOCK, 0, (hipStream_t)stream>>>(a);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- die_nca_env_step_batch's sensing (the step itself: die_env.hip) --------------------------------------------------
// Scratch: [set][replica][NCA_MAXC][W][H] fp32, set = layer % 2 (one set for a single layer); the last layer's planes stay
// there until the next step (BatchedNeuralAutomataAgent.render).
extern "C" int64_t die_nca_batch_scratch_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS || n_layers < 1 || n_layers > DIE_NCA_MAX_LAYERS) return -1;
    return (int64_t)die_nca_pingpong_sets(n_layers) * replicas * NCA_MAXC * (int64_t)W * H * (int64_t)sizeof(float);
}

int die_nca_layer0_planes(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* mem_planes, int memory,
                          const unsigned long long* stock, const void* in[], int kind[], int64_t* rep_in, const float* signal_planes,
                          int signals) {
    const int fkind = m->dtype == DIE_F32 ? DIE_PLANE_F32 : DIE_PLANE_F16;
    int c = 0;
    if (nca->with_agent_channel) { in[c] = m->owner; kind[c++] = DIE_PLANE_AGENTS; }
    in[c] = m->food; kind[c++] = fkind;
    in[c] = m->chem; kind[c++] = fkind;
    // the signal field (die_signal.hip): plane k of replica r at (k * R + r) * plane_stride too, fp32 whatever the field's dtype
    for (int k = 0; signal_planes && k < signals; ++k) { in[c] = signal_planes + (int64_t)k * b->replicas * b->plane_stride; kind[c++] = DIE_PLANE_F32; }
    // plane j of replica r at (j * R + r) * plane_stride, as die_memory_planes_batch writes them: one plane_stride a replica
    for (int j = 0; mem_planes && j < memory; ++j) { in[c] = mem_planes + (int64_t)j * b->replicas * b->plane_stride; kind[c++] = DIE_PLANE_F32; }
    if (stock) { in[c] = stock; kind[c++] = DIE_PLANE_STOCK; }
    *rep_in = b->plane_stride;
    return c;
}

// the stack for every replica, one launch per layer.  Layer l writes `dst` + set(l) · R · rep planes: set(l) = l % 2 for the
// step's ping-pong scratch, l for caller-owned storage that keeps every layer.  `drop` (checked words, or null): the last layer's
// launch is the DROP one — into `masked` when given (the unmasked launch then runs as well and keeps its place), else in place of it.
// `stock` (or null): the R stock planes of die_stock.hip, built at sense_epoch — layer 0's last input (die_nca_layer0_planes).
static int sense_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* dst, bool pingpong, float* masked,
                       const float** sense, int64_t* rep, const DropWords* drop, void* stream, const unsigned long long* stock = nullptr) {
    const int64_t cells = (int64_t)m->W * m->H, rep_scratch = NCA_MAXC * cells;
    ConvArgs a = {};
    die_nca_layer0_planes(m, b, nca, nullptr, 0, stock, a.in, a.kind, &a.rep_in);
    a.W = m->W; a.H = m->H; a.epoch = nca->sense_epoch; a.pad = nca->padding_mode;
    a.episodes = nca->episodes > 1 ? nca->episodes : 1;
    float* out = nullptr;
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        out = dst + (pingpong ? l % die_nca_pingpong_sets(nca->n_layers) : l) * b->replicas * rep_scratch;
        for (int o = 0; o < NCA_MAXC; ++o) a.out[o] = o < L.cout ? out + o * cells : nullptr;
        a.w = L.weights; a.rep_w = L.weight_stride; a.rep_out = rep_scratch;
        a.cin = L.cin; a.cout = L.cout; a.k = L.k; a.apply_tanh = l == nca->n_layers - 1;
        launch_conv<true>(a, b->replicas, (hipStream_t)stream, a.apply_tanh && !masked ? drop : nullptr);
        DIE_CHECK_LAUNCH("die_nca_env_step_batch(conv)");
        if (a.apply_tanh && masked && drop) {
            for (int o = 0; o < L.cout; ++o) a.out[o] = masked + o * cells;
            launch_conv<true>(a, b->replicas, (hipStream_t)stream, drop);
            DIE_CHECK_LAUNCH("die_nca_sense_batch_store(masked)");
            out = masked;
        }
        for (int o = 0; o < NCA_MAXC; ++o) { a.in[o] = a.out[o]; a.kind[o] = DIE_PLANE_F32; }
        a.rep_in = rep_scratch;
    }
    *sense = out;
    *rep = rep_scratch;
    return DIE_OK;
}

// *sense = the last layer's planes of replica 0 in the step's scratch, replica r's *rep further
int die_nca_sense_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float** sense, int64_t* rep,
                        const DropWords* drop, void* stream, const unsigned long long* stock) {
    return sense_batch(m, b, nca, nca->scratch, true, nullptr, sense, rep, drop, stream, stock);
}

int die_nca_field_check(const die_medium* m, const die_nca_batch* nca, const char* who) {
    DIE_REQUIRE(m->dtype == DIE_F32 || m->dtype == DIE_F16, "%s: bad field dtype %d", who, m->dtype);
    DIE_REQUIRE(m->food && m->chem && (m->owner || !nca->with_agent_channel), "%s: null plane", who);
    DIE_REQUIRE(nca->sense_epoch >= 1 && nca->sense_epoch <= DIE_OWNER_EPOCH_MAX, "%s: sense_epoch %d", who, nca->sense_epoch);
    return DIE_OK;
}

int die_nca_pad_adjoint_check(int32_t padding_mode, const char* who) {
    if (padding_mode != DIE_PAD_REFLECT && padding_mode != DIE_PAD_REPLICATE) return DIE_OK;
    die_set_error("%s: the adjoint of 'reflect' / 'replicate' padding is not implemented ('circular' and 'zeros' are)", who);
    return DIE_ERR_UNSUPPORTED;
}

int die_nca_store_check(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store, die_nca_kind kind, const char* who,
                        int memory, int signals) {
    DIE_REQUIRE(m && b && nca && store, "%s: null argument", who);
    int rc = die_nca_batch_shape_check(m, b, who);
    if (rc != DIE_OK) return rc;
    rc = die_nca_stack_check(kind, nca, m->W, m->H, b->replicas, who, false, false, memory, signals);
    if (rc != DIE_OK) return rc;
    return die_nca_field_check(m, nca, who);
}

extern "C" int64_t die_nca_sense_batch_store_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS || n_layers < 1 || n_layers > DIE_NCA_MAX_LAYERS) return -1;
    return (int64_t)n_layers * replicas * NCA_MAXC * (int64_t)W * H * (int64_t)sizeof(float);
}

extern "C" int die_nca_sense_batch_store(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store, int64_t store_bytes,
                                         float* masked, const die_nca_dropout* drop, void* stream) {
    const char* who = "die_nca_sense_batch_store";
    int rc = die_nca_store_check(m, b, nca, store, DIE_NCA_NARROW, who);
    if (rc != DIE_OK) return rc;
    const int64_t need = die_nca_sense_batch_store_bytes(m->W, m->H, b->replicas, nca->n_layers);
    DIE_REQUIRE(store_bytes >= need, "%s: store too small (%lld < %lld)", who, (long long)store_bytes, (long long)need);
    DIE_REQUIRE((m->W + NCA_TX - 1) / NCA_TX <= 65535, "%s: field too tall", who);
    DropWords dw;
    if (drop) {
        DIE_REQUIRE(masked && masked != store, "%s: a dropout mask needs planes of its own for the masked values", who);
        rc = die_dropout_words(drop, &dw, who);
        if (rc != DIE_OK) return rc;
    }
    const float* sense;
    int64_t rep;
    return sense_batch(m, b, nca, store, false, drop ? masked : nullptr, &sense, &rep, drop ? &dw : nullptr, stream);
}
