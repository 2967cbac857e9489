// The adjoint of one wide NeuralAutomataAgent layer (gfx950): what die_nca_wide.hip's k_conv_wide computes forward,
//   y = act(conv(x, w)) (* the dropout mask), up to 32 channels in and out, kernel sizes 1, 3 and 5,
// differentiated with respect to the weights and, where asked, the inputs — both GEMMs on v_mfma_f32_16x16x4_f32
// (__builtin_amdgcn_mfma_f32_16x16x4f32), as the forward.  The gradient at the pre-activation,
//   g_z = g * mask * act'(t),   act'(t) = 1 - t^2 (tanh), t > 0 ? 1 : 0 (relu, torch's convention from the stored output), 1 (none),
// is formed while a kernel stages its operands, from the gradient g at the returned value, the layer's UNMASKED output
// t = act(z) and the mask recomputed from its key (die_rng.h) — no launch and no buffer of its own, no division by keep.
//
//   k_conv_wide_gin<K, NB>   grad_in[i, x, y] = sum_o sum_a sum_b w[o, i, a, b] * g_z[o, pad'(x - a + r), pad'(y - b + r)].  For
//                       'circular' and 'zeros' the padding's adjoint is the padding itself (also where the radius exceeds the
//                       field), so this IS the forward's implicit GEMM over the g_z planes with the weight read as
//                       w'[i][o][a][b] = w[o][i][k-1-a][k-1-b] and no activation: k_conv_wide's body — the 16 x 64 tile and its 4
//                       waves, chunks of 4 channels through LDS with the next chunk's global loads issued before this chunk's
//                       MFMAs, s_in with its channel stride of 16 mod 64 words, s_w with the output fastest, 16-byte stores
//                       where H % 4 == 0 — with g_z formed between the registers and LDS.  A second kernel, not a template
//                       parameter on k_conv_wide: the forward's instantiations stay the code they were.
//   k_conv_wide_gw<K, GO, GI>   grad_w[o, i, a, b] = sum_xy g_z[o, x, y] * in[i, pad(x + a - r), pad(y + b - r)]: per tile and tap
//                       a (cout x cells) . (cells x cin) GEMM with the tile's cells as the K dimension.  One MFMA covers 4
//                       consecutive y of one row: A = g_z[o = lane & 15][cell c0 + (lane >> 4)], B = in[i = lane & 15][that cell +
//                       tap], both 64 consecutive LDS words of planes staged [cell][16 channels], channel fastest (GO / GI = 1 or
//                       2 groups of 16 output / input channels; channels past cout / cin are zeros).  The k^2 taps are dealt to
//                       the 4 waves as w, w + 4, ... (at most 7 at k = 5), a wave keeps GO * GI accumulator blocks per tap (at most
//                       112 VGPRs) and the tile is walked in strips of SR rows, SR the largest of 4, 2, 1 whose g_z strip and
//                       input strip with halo fit 64 KB of LDS next to the tile's mask factors (4 KB, worked out once, so
//                       that the Philox key schedule is not live over the strips).  Cells of a partial tile past W or H are staged as
//                       g_z = 0; the input cells are read through nca_pad_index, the first layer's through nca_load.  An element
//                       of the tile's partial row [cout * cin * k * k] is summed over (strip, row, 4 cells, cell) in that order
//                       and written exactly once, by one lane.  NO float atomics.
//   the fold            die_nca_grad.hip's k_conv_backward_sum: one thread per weight adds the partial rows in tile-index order
//                       in float64 and stores fp32.  Fixed order, fixed tree: the same inputs give the same bits on every run.
//   die_nca_wide_backward_batch   the same for every replica of a die_batch (a population's candidates), a whole stack per call:
//                       both kernels with BATCH on and the replica in blockIdx.z — its planes, weight block r / E, mask key
//                       seed + r * seed_stride, partial rows (r * tiles + tile) and input gradient, the offsets scalars added to
//                       the pointers once — then k_conv_backward_sum_batch folding a candidate's E * tiles rows in ascending
//                       order.  One arithmetic body: for E = 1 replica r is die_conv2d_wide_backward on its world, bit for bit.
//                       The stand-alone instantiations (BATCH off) keep WideBwdArgs as their whole argument and the registers,
//                       LDS and occupancy they had.
//   die_nca_wide_backward_batch_memory   that call for a population whose agents carry memory (BatchedNeuralAutomataAgent.
//                       recurrent_action): the same host body and the same launches with 3 + M planes at the top of the stack and
//                       the R * M expanded memory planes (die_memory_planes_batch's layout) among layer 0's inputs; grad_in then
//                       holds replica r's 2 + with_agent_channel + M planes, the chem plane for the env's chem node, the last M for
//                       die_memory_planes_backward_batch.  Roofline: the parent's — the M planes widen layer 0's weight gradient
//                       and the last layer's two GEMMs by M of their C channels (5 -> 8 -> 5 instead of 3 -> 8 -> 3 at M = 2),
//                       inside the same 16-channel MFMA blocks up to M = 8; at 16 x 96^2 the weight-gradient kernel is the
//                       largest launch of a training step (LABBOOK §38).
//
// Roofline.  Both GEMMs are 2 C^2 k^2 flop per cell, the forward's count, against 12 C bytes (g, t and the inputs in; the input
// gradient out): a C -> C layer with C >= 16 at k >= 3 is compute-bound on the fp32 matrix rate (157 TFLOP/s, 64 flop per clock
// per SIMD) in either kernel.  The layers touching 3 channels stay HBM-bound and pay for the padding to 4 (a chunk) and 16 (a
// block): 3 -> 16's weight gradient issues 16 / 3 of the MFMAs its 3 input channels need.
#include <math.h>
#include <type_traits>
#include "die_common.h"
#include "die_rng.h"
#include "die_nca.h"

struct WideBwdArgs {
    const void* in[NCAW_MAXC];   // the layer's inputs
    int kind[NCAW_MAXC];         // die_conv_plane.kind
    const float* g;              // gradient at the returned value: plane o at g + o * g_stride
    const float* t;              // the unmasked forward output act(z), plane o at t + o * t_stride (read where act != none)
    int64_t g_stride, t_stride;
    const float* w;              // [cout][cin][k][k]
    float* gin;                  // gradient at the inputs: plane i at gin + i * gin_stride
    int64_t gin_stride;
    float* part;                 // [tiles][cout * cin * k * k]
    int W, H, cin, cout, epoch;
    int act;                     // die_nca_activation of the forward's epilogue
    int pad;                     // die_pad_mode: circular or zeros
    int vec;                     // 16-byte stores of grad_in: H % 4 == 0 (the entry point has checked the alignment)
    int drop;                    // 1: g_z carries the dropout mask of `d`
    DropWords d;
};
// what a BATCH launch reads on top (die_nca_wide_backward_batch; the stand-alone instantiations keep WideBwdArgs as their whole
// argument): elements from replica r's planes / gradients / outputs / weights / input gradients / partial rows to replica r + 1's
struct WideBwdBatchArgs : WideBwdArgs {
    int64_t rep_in, rep_g, rep_t, rep_w, rep_gin, rep_part;
    int episodes;                // replica r reads weight block r / episodes (1: a block per replica)
};
template <bool BATCH> using WideBwdArgsOf = typename std::conditional<BATCH, WideBwdBatchArgs, WideBwdArgs>::type;

// bytes per cell of a first-layer plane (die_conv_plane.kind): a replica's offset into it, in bytes
__device__ __forceinline__ int64_t ncaw_plane_bytes(int kind) { return kind == DIE_PLANE_F32 ? 4 : kind == DIE_PLANE_F16 ? 2 : 8; }

// g_z of one cell and channel: the gradient at the returned value through the mask and the activation
__device__ __forceinline__ float ncaw_gz(float g, float t, float mask, int act, int drop) {
    float v = g;
    if (drop) v = v * mask;
    if (act == DIE_NCA_ACT_TANH) v = v * (1.f - t * t);
    else if (act == DIE_NCA_ACT_RELU) v = t > 0.f ? v : 0.f;
    return v;
}

// ---- input gradient: k_conv_wide over the g_z planes with the flipped, transposed weight ---------------------------------
// BATCH (both kernels): replica blockIdx.z of die_nca_wide_backward_batch — its planes, its candidate's weights, its mask key
// (seed + z * seed_stride), its partial rows and its input gradient.  The offsets are scalars, added to the pointers once at the
// kernel's entry; with BATCH off every pointer below IS the argument's, so those instantiations compile to the code they always were.
template <int K, int NB, bool BATCH = false>
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_wide_gin(WideBwdArgsOf<BATCH> a) {
    constexpr int R = K / 2, LX = NCA_TX + 2 * R, LY = NCA_TY + 2 * R;
    constexpr int CS = (LX * LY - 16 + 63) / 64 * 64 + 16;         // channel stride: 16 mod 64 words
    constexpr int MB = 16;                                          // M-blocks per wave: 4 rows x 4 blocks of 16 y
    __shared__ __align__(16) float s_in[NCAW_CH * CS];
    __shared__ __align__(16) float s_w[K * K * NB * NCAW_CH * 16];
    const int x0 = blockIdx.y * NCA_TX, y0 = blockIdx.x * NCA_TY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lk = lane >> 4, ln = lane & 15;
    const bool has_t = a.act != DIE_NCA_ACT_NONE;
    uint64_t key = a.d.seed;
    [[maybe_unused]] int wrow = 0;                                  // the replica's weight block
    if constexpr (BATCH) {
        wrow = (int)blockIdx.z / a.episodes;
        key += (uint64_t)blockIdx.z * a.d.seed_stride;
    }

    ncaw_f32x4 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[m][nb] = ncaw_f32x4{0.f, 0.f, 0.f, 0.f};

    // the forward's staging plan: tile words i = tid, tid + 256, ... of every g_z plane and the weight words likewise, their
    // addresses worked out once — and the mask of every tile word, which no chunk changes
    constexpr int NI = (LX * LY + DIE_BLOCK - 1) / DIE_BLOCK, NWI = (K * K * NB * NCAW_CH * 16 + DIE_BLOCK - 1) / DIE_BLOCK;
    int64_t cell[NI];
    float mask[NI];
    int wbase[NWI];                                                // the word's offset in w for chunk 0 (0 for a zero word)
    unsigned live = 0, wlive = 0;
#pragma unroll
    for (int t = 0; t < NI; ++t) {
        const int i = threadIdx.x + t * DIE_BLOCK, li = i / LY, lj = i - li * LY;
        // (rows / columns past the last tile's outputs wrap like a circular field whatever the mode: never used)
        const int vx = x0 - R + li, vy = y0 - R + lj;
        const int gx = nca_pad_index(vx < a.W + R ? vx : vx % a.W, a.W, a.pad), gy = nca_pad_index(vy < a.H + R ? vy : vy % a.H, a.H, a.pad);
        const bool ok = i < LX * LY && gx >= 0 && gy >= 0;
        cell[t] = ok ? (int64_t)gx * a.H + gy : 0;
        live |= ok ? 1u << t : 0u;
        mask[t] = a.drop ? die_dropout_factor(die_dropout_word(key, a.d.step, (uint64_t)cell[t]), a.d.thr, a.d.keep) : 1.f;
    }
    // s_w[a][b][nb][c][i]: the word of output (input channel of the layer) i = nb * 16 + (word & 15), chunk channel c (an output
    // channel of the layer), tap (a, b) is w[c][i][k-1-a][k-1-b]
#pragma unroll
    for (int t = 0; t < NWI; ++t) {
        const int i = threadIdx.x + t * DIE_BLOCK, o = ((i >> 6) % NB) * 16 + (i & 15), tap = i / (64 * NB);
        const bool ok = i < K * K * NB * NCAW_CH * 16 && o < a.cin;
        wbase[t] = ok ? (((i >> 4) & 3) * a.cin + o) * (K * K) + (K * K - 1 - tap) : 0;
        wlive |= ok ? 1u << t : 0u;
    }
    float pre[NI][NCAW_CH], pret[NI][NCAW_CH], wpre[NWI];
    auto fetch = [&](int c0) {
        // the replica's bases: scalars from the arguments, worked out per chunk (a handful of scalar operations) so that no
        // pointer pair stays live over the MFMAs
        const float *gbase = a.g, *tbase = a.t, *w = a.w;
        if constexpr (BATCH) {
            gbase += (int64_t)blockIdx.z * a.rep_g; tbase += (int64_t)blockIdx.z * a.rep_t; w += (int64_t)wrow * a.rep_w;
        }
#pragma unroll
        for (int t = 0; t < NWI; ++t) {
            const int c = c0 + (((threadIdx.x + t * DIE_BLOCK) >> 4) & 3);
            wpre[t] = w[c < a.cout ? wbase[t] + c0 * a.cin * (K * K) : 0];
        }
#pragma unroll
        for (int j = 0; j < NCAW_CH; ++j) {
            const int c = c0 + j;                                   // (uniform)
            if (c >= a.cout) continue;
            const float* gp = gbase + (int64_t)c * a.g_stride;
#pragma unroll
            for (int t = 0; t < NI; ++t) pre[t][j] = gp[cell[t]];
            if (has_t) {
                const float* tp = tbase + (int64_t)c * a.t_stride;
#pragma unroll
                for (int t = 0; t < NI; ++t) pret[t][j] = tp[cell[t]];
            }
        }
    };
#pragma unroll
    for (int t = 0; t < NI; ++t)
#pragma unroll
        for (int j = 0; j < NCAW_CH; ++j) pre[t][j] = pret[t][j] = 0.f;
    fetch(0);
    for (int c0 = 0; c0 < a.cout; c0 += NCAW_CH) {
        if (c0) __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int t = 0; t < NWI; ++t) {
            const int i = threadIdx.x + t * DIE_BLOCK;
            const int c = c0 + ((i >> 4) & 3);
            if (i < K * K * NB * NCAW_CH * 16) s_w[i] = ((wlive >> t) & 1) && c < a.cout ? wpre[t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NI; ++t) {
            const int i = threadIdx.x + t * DIE_BLOCK;
            if (i < LX * LY) {
#pragma unroll
                for (int j = 0; j < NCAW_CH; ++j)
                    s_in[j * CS + i] = ((live >> t) & 1) && c0 + j < a.cout ? ncaw_gz(pre[t][j], pret[t][j], mask[t], a.act, a.drop) : 0.f;
            }
        }
        __syncthreads();
        if (c0 + NCAW_CH < a.cout) fetch(c0 + NCAW_CH);
#pragma unroll
        for (int ka = 0; ka < K; ++ka) {
#pragma unroll
            for (int kb = 0; kb < K; ++kb) {
                float bv[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) bv[nb] = s_w[((ka * K + kb) * NB + nb) * 64 + lane];
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    const float av = s_in[lk * CS + (wave * 4 + (m >> 2) + ka) * LY + (m & 3) * 16 + ln + kb];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nb], acc[m][nb], 0, 0, 0);
                }
            }
        }
    }

    float* ginbase = a.gin;                                         // (worked out here: not live over the chunks)
    if constexpr (BATCH) ginbase += (int64_t)blockIdx.z * a.rep_gin;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int gx = x0 + wave * 4 + (m >> 2), gy = y0 + (m & 3) * 16 + lk * 4;      // this lane's 4 cells: (gx, gy .. gy + 3)
        if (gx >= a.W || gy >= a.H) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int i = nb * 16 + ln;
            if (i >= a.cin) continue;
            float* dst = ginbase + (int64_t)i * a.gin_stride + (int64_t)gx * a.H + gy;
            if (a.vec) *(float4*)dst = make_float4(acc[m][nb][0], acc[m][nb][1], acc[m][nb][2], acc[m][nb][3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (gy + q < a.H) dst[q] = acc[m][nb][q];
            }
        }
    }
}

// ---- weight gradient: one partial row per tile ---------------------------------------------------------------------------
// rows per strip: the largest of 4, 2, 1 whose g_z strip [GO][SR][64][16] and input strip [GI][SR + 2r][64 + 2r][16] fit 64 KB
// next to the tile's 4 KB of mask factors
template <int K, int GO, int GI>
constexpr int ncaw_gw_strip() {
    constexpr int R = K / 2;
    for (int sr = 4; sr > 1; sr >>= 1)
        if (((GO * sr * NCA_TY + GI * (sr + 2 * R) * (NCA_TY + 2 * R)) * 16 + NCA_TX * NCA_TY) * 4 <= 65536) return sr;
    return 1;
}

template <int K, int GO, int GI, bool BATCH = false>
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_wide_gw(WideBwdArgsOf<BATCH> a) {
    constexpr int R = K / 2, SR = ncaw_gw_strip<K, GO, GI>(), LY = NCA_TY + 2 * R, XR = SR + 2 * R;
    constexpr int NT = (K * K + 3) / 4;                             // taps per wave: wave, wave + 4, ...
    constexpr int GCELLS = SR * NCA_TY, XCELLS = XR * LY;
    static_assert(((GO * GCELLS + GI * XCELLS) * 16 + NCA_TX * NCA_TY) * 4 <= 65536, "the strips do not fit LDS");
    static_assert(NCA_TX % SR == 0 && DIE_BLOCK % GCELLS == 0, "strips tile the rows, a strip's cells the workgroup");
    __shared__ __align__(16) float s_g[GO * GCELLS * 16];           // [group of 16 o][row][y][o]
    __shared__ __align__(16) float s_x[GI * XCELLS * 16];           // [group of 16 i][row + halo][y + halo][i]
    __shared__ float s_m[NCA_TX * NCA_TY];                          // the tile's mask factors (written and read with a mask only)
    const int x0 = blockIdx.y * NCA_TX, y0 = blockIdx.x * NCA_TY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lk = lane >> 4, ln = lane & 15;
    const bool has_t = a.act != DIE_NCA_ACT_NONE;
    const float *gbase = a.g, *tbase = a.t;
    uint64_t key = a.d.seed;
    [[maybe_unused]] int64_t o_in = 0;                              // replica z's offset into an input plane, in cells
    if constexpr (BATCH) {
        const int64_t z = (int64_t)blockIdx.z;
        gbase += z * a.rep_g; tbase += z * a.rep_t;
        o_in = z * a.rep_in;
        key += (uint64_t)blockIdx.z * a.d.seed_stride;
    }

    ncaw_f32x4 acc[NT][GO][GI];
    int toff[NT];                                                   // tap (ta, tb)'s offset in s_x, in cells
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int tap = wave + 4 * j, ta = tap / K, tb = tap - ta * K;
        toff[j] = ta * LY + tb;
#pragma unroll
        for (int og = 0; og < GO; ++og)
#pragma unroll
            for (int ig = 0; ig < GI; ++ig) acc[j][og][ig] = ncaw_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the mask of every cell of the tile, once (the Philox key schedule does not stay live over the strips)
    if (a.drop) {
#pragma unroll
        for (int n = 0; n < NCA_TX * NCA_TY / DIE_BLOCK; ++n) {
            const int i = threadIdx.x + n * DIE_BLOCK, gx = x0 + i / NCA_TY, gy = y0 + i % NCA_TY;
            const uint64_t cell = gx < a.W && gy < a.H ? (uint64_t)gx * (uint64_t)a.H + (uint64_t)gy : 0;
            s_m[i] = die_dropout_factor(die_dropout_word(key, a.d.step, cell), a.d.thr, a.d.keep);
        }
        __syncthreads();
    }

#pragma unroll 1
    for (int r0 = 0; r0 < NCA_TX && x0 + r0 < a.W; r0 += SR) {      // (a strip past the field holds g_z = 0 only)
        if (r0) __syncthreads();                                    // the previous strip has been read
        // g_z: a thread stages ONE cell of the strip, tid % GCELLS (consecutive lanes on consecutive y: a plane's loads coalesce),
        // for the quads of channels tid / GCELLS, that + 256 / GCELLS, ...: one 16-byte LDS store per quad
        {
            const int ci = threadIdx.x % GCELLS, gx = x0 + r0 + ci / NCA_TY, gy = y0 + ci % NCA_TY;
            const bool ok = gx < a.W && gy < a.H;
            const int64_t cell = ok ? (int64_t)gx * a.H + gy : 0;
            const float m = a.drop ? s_m[r0 * NCA_TY + ci] : 1.f;
#pragma unroll 1
            for (int q = threadIdx.x / GCELLS; q < 4 * GO; q += DIE_BLOCK / GCELLS) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = 4 * q + e;
                    v[e] = 0.f;
                    if (o < a.cout && ok) {
                        const float g = gbase[(int64_t)o * a.g_stride + cell];
                        const float t = has_t ? tbase[(int64_t)o * a.t_stride + cell] : 0.f;
                        v[e] = ncaw_gz(g, t, m, a.act, a.drop);
                    }
                }
                *(float4*)&s_g[((q >> 2) * GCELLS + ci) * 16 + (q & 3) * 4] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        // the inputs under the strip and its halo, through the padding (a cell past the field in a partial tile reads whatever
        // the padding gives: its g_z is 0)
#pragma unroll 1
        for (int cj = threadIdx.x; cj < XCELLS; cj += DIE_BLOCK) {
            const int li = cj / LY, lj = cj - li * LY;
            const int gx = nca_pad_index(x0 + r0 - R + li, a.W, a.pad), gy = nca_pad_index(y0 - R + lj, a.H, a.pad);
            const bool ok = gx >= 0 && gy >= 0;
            const int64_t cell = ok ? (int64_t)gx * a.H + gy : 0;
#pragma unroll 1
            for (int q = 0; q < 4 * GI; ++q) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = 4 * q + e;                        // (uniform: the plane's pointer and kind are scalar loads)
                    v[e] = 0.f;
                    if (c < a.cin) {
                        const void* p = a.in[c];
                        const int kind = a.kind[c];
                        if constexpr (BATCH) p = (const char*)p + o_in * ncaw_plane_bytes(kind);      // (scalar: once per plane)
                        if (ok) v[e] = nca_load(p, kind, cell, a.epoch);
                    }
                }
                *(float4*)&s_x[((q >> 2) * XCELLS + cj) * 16 + (q & 3) * 4] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        __syncthreads();
        // one K-step = 4 consecutive y of one row; lane (lk, ln) reads word lane of the step's 64 in either operand
        for (int s = 0; s < SR * (NCA_TY / 4); ++s) {
            const int gcell = (s >> 4) * NCA_TY + (s & 15) * 4 + lk, xcell = (s >> 4) * LY + (s & 15) * 4 + lk;
            float av[GO];
#pragma unroll
            for (int og = 0; og < GO; ++og) av[og] = s_g[(og * GCELLS + gcell) * 16 + ln];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (wave + 4 * j < K * K) {                         // (wave-uniform)
                    float bv[GI];
#pragma unroll
                    for (int ig = 0; ig < GI; ++ig) bv[ig] = s_x[(ig * XCELLS + xcell + toff[j]) * 16 + ln];
#pragma unroll
                    for (int og = 0; og < GO; ++og)
#pragma unroll
                        for (int ig = 0; ig < GI; ++ig)
                            acc[j][og][ig] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[og], bv[ig], acc[j][og][ig], 0, 0, 0);
                }
            }
        }
    }

    // accumulator block (og, ig) of tap (ta, tb): column lane & 15 = input channel, rows 4 (lane >> 4) + q = output channel
    const int nw = a.cout * a.cin * K * K;
    float* part = a.part;                                           // (worked out here: not live over the strips)
    if constexpr (BATCH) part += (int64_t)blockIdx.z * a.rep_part;
    float* prow = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nw;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int tap = wave + 4 * j;
        if (tap >= K * K) continue;
#pragma unroll
        for (int og = 0; og < GO; ++og) {
#pragma unroll
            for (int ig = 0; ig < GI; ++ig) {
                const int i = ig * 16 + ln;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int o = og * 16 + lk * 4 + q;
                    if (o < a.cout && i < a.cin) prow[(o * a.cin + i) * (K * K) + tap] = acc[j][og][ig][q];
                }
            }
        }
    }
}

// the two launches of one layer: gridDim.z = replicas for BATCH, 1 (and WideBwdArgs alone) otherwise
template <int K, bool BATCH>
static void launch_wide_backward(const WideBwdArgsOf<BATCH>& a, bool want_gin, int replicas, hipStream_t s) {
    dim3 grid((a.H + NCA_TY - 1) / NCA_TY, (a.W + NCA_TX - 1) / NCA_TX, replicas);
    const bool go2 = a.cout > 16, gi2 = a.cin > 16;
    if (go2 && gi2) k_conv_wide_gw<K, 2, 2, BATCH><<<grid, DIE_BLOCK, 0, s>>>(a);
    else if (go2) k_conv_wide_gw<K, 2, 1, BATCH><<<grid, DIE_BLOCK, 0, s>>>(a);
    else if (gi2) k_conv_wide_gw<K, 1, 2, BATCH><<<grid, DIE_BLOCK, 0, s>>>(a);
    else k_conv_wide_gw<K, 1, 1, BATCH><<<grid, DIE_BLOCK, 0, s>>>(a);
    if (!want_gin) return;
    if (gi2) k_conv_wide_gin<K, 2, BATCH><<<grid, DIE_BLOCK, 0, s>>>(a);
    else k_conv_wide_gin<K, 1, BATCH><<<grid, DIE_BLOCK, 0, s>>>(a);
}

static bool wide_shape_ok(int32_t W, int32_t H, int32_t cin, int32_t cout, int32_t k) {
    return W >= 1 && H >= 1 && (W + NCA_TX - 1) / NCA_TX <= 65535 && cin >= 1 && cin <= NCAW_MAXC && cout >= 1 && cout <= NCAW_MAXC &&
           (k == 1 || k == 3 || k == 5);
}

extern "C" int64_t die_conv2d_wide_backward_workspace_bytes(int32_t W, int32_t H, int32_t cin, int32_t cout, int32_t k) {
    if (!wide_shape_ok(W, H, cin, cout, k)) return -1;
    return die_nca_tiles(W, H) * cout * cin * k * k * (int64_t)sizeof(float);
}

extern "C" int die_conv2d_wide_backward(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout,
                                        const float* grad_out, int64_t grad_out_stride, const float* fwd_out, int64_t fwd_out_stride,
                                        int32_t k, const float* weights, int32_t activation, int32_t padding_mode,
                                        const die_nca_dropout* drop, float* grad_weights, float* grad_in, int64_t grad_in_stride,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "die_conv2d_wide_backward";
    DIE_REQUIRE(padding_mode >= DIE_PAD_CIRCULAR && padding_mode <= DIE_PAD_REPLICATE, "%s: bad padding mode %d", who, padding_mode);
    if (die_nca_pad_adjoint_check(padding_mode, who) != DIE_OK) return DIE_ERR_UNSUPPORTED;
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE((W + NCA_TX - 1) / NCA_TX <= 65535, "%s: field too tall", who);
    DIE_REQUIRE(cin >= 1 && cin <= NCAW_MAXC && cout >= 1 && cout <= NCAW_MAXC, "%s: 1..%d channels (got %d -> %d)", who, NCAW_MAXC, cin, cout);
    DIE_REQUIRE(k == 1 || k == 3 || k == 5, "%s: kernel size %d (1, 3 or 5)", who, k);
    DIE_REQUIRE(activation >= DIE_NCA_ACT_NONE && activation <= DIE_NCA_ACT_RELU, "%s: bad activation %d", who, activation);
    DIE_REQUIRE(in && grad_out && weights && grad_weights && workspace, "%s: null argument", who);
    DIE_REQUIRE(fwd_out || (activation == DIE_NCA_ACT_NONE && !drop), "%s: an activation or a dropout mask without the forward outputs "
                "it was applied to", who);
    DIE_REQUIRE(grad_weights != weights, "%s: grad_weights is the weights", who);
    const int64_t cells = (int64_t)W * H, nw = (int64_t)cout * cin * k * k;
    DIE_REQUIRE(grad_out_stride >= cells, "%s: grad_out_stride %lld smaller than a plane (%lld cells)", who, (long long)grad_out_stride,
                (long long)cells);
    DIE_REQUIRE(!fwd_out || fwd_out_stride >= cells, "%s: fwd_out_stride %lld smaller than a plane (%lld cells)", who,
                (long long)fwd_out_stride, (long long)cells);
    DIE_REQUIRE(!grad_in || grad_in_stride >= cells, "%s: grad_in_stride %lld smaller than a plane (%lld cells)", who,
                (long long)grad_in_stride, (long long)cells);
    const int64_t need = die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k);
    DIE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)workspace_bytes, (long long)need);
    WideBwdArgs a = {};
    const int64_t gin_bytes = ((int64_t)(cin - 1) * grad_in_stride + cells) * (int64_t)sizeof(float);
    auto overlaps = [&](const void* p, int64_t bytes) { return die_ranges_overlap(grad_in, gin_bytes, p, bytes); };
    for (int c = 0; c < cin; ++c) {
        DIE_REQUIRE(in[c].data && in[c].kind >= DIE_PLANE_F32 && in[c].kind <= DIE_PLANE_AGENTS, "%s: bad input plane %d", who, c);
        const int64_t bytes = cells * (in[c].kind == DIE_PLANE_F32 ? 4 : in[c].kind == DIE_PLANE_F16 ? 2 : 8);
        DIE_REQUIRE(!overlaps(in[c].data, bytes), "%s: grad_in aliases another buffer of the call (input plane %d)", who, c);
        a.in[c] = in[c].data; a.kind[c] = in[c].kind;
    }
    DIE_REQUIRE(!overlaps(grad_out, ((int64_t)(cout - 1) * grad_out_stride + cells) * 4) &&
                    !overlaps(fwd_out, ((int64_t)(cout - 1) * fwd_out_stride + cells) * 4) && !overlaps(weights, nw * 4) &&
                    !overlaps(grad_weights, nw * 4) && !overlaps(workspace, need),
                "%s: grad_in aliases another buffer of the call", who);
    // the kernel stores four cells of a row at once where H % 4 == 0
    DIE_REQUIRE(!grad_in || H % 4 != 0 || (((uintptr_t)grad_in & 15) == 0 && grad_in_stride % 4 == 0),
                "%s: grad_in must be 16-byte aligned and grad_in_stride a multiple of 4 where H %% 4 == 0", who);
    if (drop) {
        const int rc = die_dropout_words(drop, &a.d, who);
        if (rc != DIE_OK) return rc;
        a.drop = 1;
    }
    a.g = grad_out; a.g_stride = grad_out_stride; a.t = fwd_out; a.t_stride = fwd_out_stride;
    a.w = weights; a.gin = grad_in; a.gin_stride = grad_in_stride; a.part = (float*)workspace;
    a.W = W; a.H = H; a.cin = cin; a.cout = cout; a.epoch = epoch; a.act = activation; a.pad = padding_mode;
    a.vec = H % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    switch (k) {
        case 1: launch_wide_backward<1, false>(a, grad_in != nullptr, 1, s); break;
        case 3: launch_wide_backward<3, false>(a, grad_in != nullptr, 1, s); break;
        default: launch_wide_backward<5, false>(a, grad_in != nullptr, 1, s); break;
    }
    DIE_CHECK_LAUNCH(who);
    die_conv_backward_fold((const float*)workspace, die_nca_tiles(W, H), (int)nw, grad_weights, s);
    DIE_CHECK_LAUNCH("die_conv2d_wide_backward(sum)");
    return DIE_OK;
}

// ---- the wide stack's adjoint for every replica of a batch ---------------------------------------------------------------
// Workspace: min(layers - 1, 2) sets of [replica][Cmax][W][H] planes for the gradient travelling down the stack (ping-pong), Cmax
// the widest cout: the store's plane count — first, so that their 16-byte stores stay aligned whatever the rows' length — then
// [replica][tile][the largest cout * cin * k * k of the stack] partial rows (a layer uses [replica][tile][its own nw] of it).
static int64_t wide_bwd_max_weights(const die_nca_batch* nca) {
    int64_t mw = 0;
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        const int64_t nw = (int64_t)L.cout * L.cin * L.k * L.k;
        mw = nw > mw ? nw : mw;
    }
    return mw;
}

// the shapes the byte query answers for (the call itself checks everything again, with messages)
// (memory, signals: layer 0 reads that many planes more, the last layer gives 3 + signals + memory)
static bool wide_bwd_stack_ok(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca, int memory = 0, int signals = 0) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS || (W + NCA_TX - 1) / NCA_TX > 65535) return false;
    if (!nca || !nca->layers || nca->n_layers < 1 || nca->n_layers > DIE_NCA_MAX_LAYERS) return false;
    if (nca->with_agent_channel != 0 && nca->with_agent_channel != 1) return false;
    if (nca->padding_mode != DIE_PAD_CIRCULAR && nca->padding_mode != DIE_PAD_ZEROS) return false;
    if (nca->episodes < 0 || replicas % (nca->episodes > 1 ? nca->episodes : 1) != 0) return false;
    int cin = 2 + nca->with_agent_channel + signals + memory;
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        if (!wide_shape_ok(W, H, L.cin, L.cout, L.k) || L.cin != cin) return false;
        if (L.reserved < DIE_NCA_ACT_NONE || L.reserved > DIE_NCA_ACT_RELU) return false;
        if (l == nca->n_layers - 1 && L.reserved != DIE_NCA_ACT_TANH) return false;
        cin = L.cout;
    }
    return cin == 3 + signals + memory;
}

static int64_t wide_bwd_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca, int memory, int signals = 0) {
    if (!wide_bwd_stack_ok(W, H, replicas, nca, memory, signals)) return -1;
    return ((int64_t)replicas * die_nca_tiles(W, H) * wide_bwd_max_weights(nca) +
            (int64_t)die_nca_gin_sets(nca->n_layers) * replicas * die_nca_max_channels(nca) * (int64_t)W * H) * (int64_t)sizeof(float);
}

extern "C" int64_t die_nca_wide_backward_batch_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca) {
    return wide_bwd_workspace_bytes(W, H, replicas, nca, 0);
}

extern "C" int64_t die_nca_wide_backward_batch_memory_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca,
                                                                      int32_t memory_channels) {
    if (memory_channels < 1 || memory_channels > DIE_MEMORY_MAX_CHANNELS) return -1;
    return wide_bwd_workspace_bytes(W, H, replicas, nca, memory_channels);
}

extern "C" int64_t die_nca_wide_backward_batch_signal_workspace_bytes(int32_t W, int32_t H, int32_t replicas, const die_nca_batch* nca,
                                                                      int32_t memory_channels, int32_t signal_channels) {
    if (memory_channels < 0 || memory_channels > DIE_MEMORY_MAX_CHANNELS || signal_channels < 1 || signal_channels > DIE_SIGNAL_MAX_CHANNELS)
        return -1;
    return wide_bwd_workspace_bytes(W, H, replicas, nca, memory_channels, signal_channels);
}

// die_nca_wide_backward_batch (memory = 0, mem_planes null), die_nca_wide_backward_batch_memory and die_nca_wide_backward_batch_signal
// (signals > 0 with signal_planes): one body, the same launches
static int wide_backward_batch(const char* who, const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                               const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                               const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                               int64_t grad_in_stride, const float* mem_planes, int memory, void* stream,
                               const float* signal_planes = nullptr, int signals = 0) {
    int rc = die_nca_batch_shape_check(m, b, who);
    if (rc != DIE_OK) return rc;
    rc = die_nca_stack_check(DIE_NCA_WIDE, nca, m->W, m->H, b->replicas, who, false, false, memory, signals);
    if (rc == DIE_OK) rc = die_nca_pad_adjoint_check(nca->padding_mode, who);
    if (rc == DIE_OK) rc = die_nca_field_check(m, nca, who);
    if (rc != DIE_OK) return rc;
    const int Cmax = die_nca_max_channels(nca);
    const int64_t cells = (int64_t)m->W * m->H, rep_planes = Cmax * cells;
    const int n_sense = 3 + signals + memory;                // planes per replica at the top of the stack
    if (memory || signals) DIE_REQUIRE(sense_stride >= n_sense * cells, "%s: sense_stride %lld below %d planes", who, (long long)sense_stride, n_sense);
    else DIE_REQUIRE(sense_stride >= 3 * cells, "%s: sense_stride %lld below three planes", who, (long long)sense_stride);
    int64_t P = 0;
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        P += (int64_t)L.cout * L.cin * L.k * L.k;
        DIE_REQUIRE(grad != L.weights, "%s: grad is layer %d's weights", who, l);
    }
    DIE_REQUIRE(grad_stride >= P, "%s: grad_stride %lld below a row of %lld weights", who, (long long)grad_stride, (long long)P);
    const int64_t need = wide_bwd_workspace_bytes(m->W, m->H, b->replicas, nca, memory, signals);
    DIE_REQUIRE(need > 0, "%s: a shape the call does not take", who);
    DIE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)workspace_bytes, (long long)need);
    // the input-gradient kernel stores four cells of a row at once where H % 4 == 0, into the workspace's planes too
    DIE_REQUIRE(m->H % 4 != 0 || nca->n_layers < 2 || ((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned where H %% 4 == 0", who);
    const int E = nca->episodes > 1 ? nca->episodes : 1, R = b->replicas, L = nca->n_layers;
    if (grad_in) {
        const int64_t in_planes = (int64_t)nca->layers[0].cin * cells;
        DIE_REQUIRE(grad_in_stride >= in_planes, "%s: grad_in_stride %lld below the first layer's %d input planes", who,
                    (long long)grad_in_stride, nca->layers[0].cin);
        // the kernel stores four cells of a row at once where H % 4 == 0
        DIE_REQUIRE(m->H % 4 != 0 || (((uintptr_t)grad_in & 15) == 0 && grad_in_stride % 4 == 0),
                    "%s: grad_in must be 16-byte aligned and grad_in_stride a multiple of 4 where H %% 4 == 0", who);
        const int64_t gin_bytes = ((int64_t)(R - 1) * grad_in_stride + in_planes) * (int64_t)sizeof(float);
        auto overlaps = [&](const void* p, int64_t bytes) { return die_ranges_overlap(grad_in, gin_bytes, p, bytes); };
        const int64_t fbytes = ((int64_t)(R - 1) * b->plane_stride + cells) * (m->dtype == DIE_F32 ? 4 : 2);
        DIE_REQUIRE(!overlaps(store, (int64_t)L * R * rep_planes * 4) && !overlaps(grad_sense, ((int64_t)(R - 1) * sense_stride + n_sense * cells) * 4) &&
                        !overlaps(grad, ((int64_t)(R / E - 1) * grad_stride + P) * 4) && !overlaps(workspace, need) &&
                        !overlaps(m->owner, ((int64_t)(R - 1) * b->plane_stride + cells) * 8) && !overlaps(m->food, fbytes) &&
                        !overlaps(m->chem, fbytes) &&
                        !overlaps(mem_planes, (((int64_t)memory * R - 1) * b->plane_stride + cells) * 4) &&
                        !overlaps(signal_planes, (((int64_t)signals * R - 1) * b->plane_stride + cells) * 4),
                    "%s: grad_in aliases another buffer of the call", who);
        for (int l = 0; l < L; ++l) {
            const die_nca_layer& Ly = nca->layers[l];
            DIE_REQUIRE(!overlaps(Ly.weights, ((int64_t)(R / E - 1) * Ly.weight_stride + (int64_t)Ly.cout * Ly.cin * Ly.k * Ly.k) * 4),
                        "%s: grad_in aliases layer %d's weights", who, l);
        }
    }
    DropWords dw = {};
    if (drop) {
        rc = die_dropout_words(drop, &dw, who);
        if (rc != DIE_OK) return rc;
    }
    const int64_t tiles = die_nca_tiles(m->W, m->H);
    float* gin_sets = (float*)workspace;
    float* part = gin_sets + (int64_t)die_nca_gin_sets(L) * R * rep_planes;
    hipStream_t s = (hipStream_t)stream;
    int64_t off = P;
    const float* g = grad_sense;
    int64_t rep_g = sense_stride;
    for (int l = L - 1; l >= 0; --l) {
        const die_nca_layer& Ly = nca->layers[l];
        const int nw = Ly.cout * Ly.cin * Ly.k * Ly.k;
        off -= nw;
        WideBwdBatchArgs a = {};
        if (l == 0) {
            die_nca_layer0_planes(m, b, nca, mem_planes, memory, nullptr, a.in, a.kind, &a.rep_in, signal_planes, signals);
        } else {
            for (int c = 0; c < Ly.cin; ++c) { a.in[c] = store + (int64_t)(l - 1) * R * rep_planes + c * cells; a.kind[c] = DIE_PLANE_F32; }
            a.rep_in = rep_planes;
        }
        float* gin = l > 0 ? gin_sets + (int64_t)((L - 1 - l) % 2) * R * rep_planes : grad_in;
        a.g = g; a.g_stride = cells; a.rep_g = rep_g;
        a.t = store + (int64_t)l * R * rep_planes; a.t_stride = cells; a.rep_t = rep_planes;
        a.w = Ly.weights; a.rep_w = Ly.weight_stride; a.episodes = E;
        a.gin = gin; a.gin_stride = cells; a.rep_gin = l > 0 ? rep_planes : grad_in_stride;
        a.part = part; a.rep_part = tiles * nw;
        a.W = m->W; a.H = m->H; a.cin = Ly.cin; a.cout = Ly.cout; a.epoch = nca->sense_epoch; a.act = Ly.reserved; a.pad = nca->padding_mode;
        a.vec = m->H % 4 == 0;
        a.drop = drop != nullptr && l == L - 1;
        a.d = dw;
        switch (Ly.k) {
            case 1: launch_wide_backward<1, true>(a, gin != nullptr, R, s); break;
            case 3: launch_wide_backward<3, true>(a, gin != nullptr, R, s); break;
            default: launch_wide_backward<5, true>(a, gin != nullptr, R, s); break;
        }
        DIE_CHECK_LAUNCH(who);
        die_conv_backward_fold_batch(part, (int64_t)E * tiles, nw, R / E, grad + off, grad_stride, s);
        DIE_CHECK_LAUNCH("die_nca_wide_backward_batch(sum)");
        g = gin; rep_g = rep_planes;
    }
    return DIE_OK;
}

extern "C" int die_nca_wide_backward_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                           const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                           const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                           int64_t grad_in_stride, void* stream) {
    const char* who = "die_nca_wide_backward_batch";
    DIE_REQUIRE(m && b && nca && store && grad_sense && grad && workspace, "%s: null argument", who);
    return wide_backward_batch(who, m, b, nca, store, grad_sense, sense_stride, grad, grad_stride, drop, workspace, workspace_bytes, grad_in,
                               grad_in_stride, nullptr, 0, stream);
}

extern "C" int die_nca_wide_backward_batch_memory(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                                  const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                                  const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                                  int64_t grad_in_stride, const float* mem_planes, int32_t memory_channels, void* stream) {
    const char* who = "die_nca_wide_backward_batch_memory";
    DIE_REQUIRE(m && b && nca && store && grad_sense && grad && workspace && mem_planes, "%s: null argument", who);
    DIE_REQUIRE(memory_channels >= 1 && memory_channels <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who,
                memory_channels, DIE_MEMORY_MAX_CHANNELS);
    return wide_backward_batch(who, m, b, nca, store, grad_sense, sense_stride, grad, grad_stride, drop, workspace, workspace_bytes, grad_in,
                               grad_in_stride, mem_planes, memory_channels, stream);
}

extern "C" int die_nca_wide_backward_batch_signal(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store,
                                                  const float* grad_sense, int64_t sense_stride, float* grad, int64_t grad_stride,
                                                  const die_nca_dropout* drop, void* workspace, int64_t workspace_bytes, float* grad_in,
                                                  int64_t grad_in_stride, const float* mem_planes, int32_t memory_channels,
                                                  const float* signal_planes, int32_t signal_channels, void* stream) {
    const char* who = "die_nca_wide_backward_batch_signal";
    DIE_REQUIRE(m && b && nca && store && grad_sense && grad && workspace && signal_planes, "%s: null argument", who);
    DIE_REQUIRE(memory_channels >= 0 && memory_channels <= DIE_MEMORY_MAX_CHANNELS && (memory_channels > 0) == (mem_planes != nullptr),
                "%s: %d memory channels outside 0..%d, or not 0 exactly where the memory planes are null", who, memory_channels,
                DIE_MEMORY_MAX_CHANNELS);
    DIE_REQUIRE(signal_channels >= 1 && signal_channels <= DIE_SIGNAL_MAX_CHANNELS, "%s: %d signal channels outside 1..%d", who,
                signal_channels, DIE_SIGNAL_MAX_CHANNELS);
    return wide_backward_batch(who, m, b, nca, store, grad_sense, sense_stride, grad, grad_stride, drop, workspace, workspace_bytes, grad_in,
                               grad_in_stride, mem_planes, memory_channels, stream, signal_planes, signal_channels);
}
