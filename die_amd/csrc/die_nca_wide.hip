// NeuralAutomataAgent sensing for wide stacks (gfx950): ConvolutionModel(hidden_channels=C, hidden_activation=...), layers of up
// to 32 channels in and out, kernel sizes 1, 3 and 5, an activation after every layer (none / tanh / relu; the last layer's tanh
// and its dropout mask as in die_nca.hip).  The narrow kernels of die_nca.hip stay what they are; a stack with either argument
// set takes these entry points for every layer, also where it would fit the narrow ones.  What a valid stack is — narrow or wide, one
// walk over two sets of limits — is checked here (die_nca_stack_check); layer 0's input list, the field check and the store calls'
// checks are die_nca.hip's, the sizes derived from a stack die_nca.h's.
//
//   k_conv_wide<K, NB>  one layer as an implicit GEMM on v_mfma_f32_16x16x4_f32 (__builtin_amdgcn_mfma_f32_16x16x4f32):
//                       M = 16 consecutive y of one row x, N = 16 output channels (NB = 1 or 2 blocks of them, the weights of
//                       channels past cout are zeros), one K-step = 4 input channels at one tap (a, b).  A workgroup of 4 waves
//                       owns die_nca.hip's 16 x 64 output tile: wave w rows 4w .. 4w + 3, 4 M-blocks per row, so 16 * NB
//                       independent accumulator blocks per wave (the dependent-accumulator latency of 40 cycles against a
//                       32-cycle issue needs 2).  The input channels go through LDS in chunks of 4 (one K-step per tap), each
//                       with its slice of the weights:
//                         s_in[c][x][y]          (16 + 2r) x (64 + 2r) cells per channel, the channel stride padded to 16 mod 64
//                                                words: lane l reads s_in[l >> 4][x + a][y0 + (l & 15) + b], 4 x 16 consecutive
//                                                words in 4 different quarters of the banks;
//                         s_w[a][b][nb][c][o]    o fastest: lane l reads word l of its (a, b, nb) block.
//                       Channels past cin are staged as zeros, inputs and weights both.  A chunk travels global -> registers ->
//                       LDS, and chunk n + 1's global loads are issued before chunk n's MFMAs: with one workgroup per CU
//                       (about 290 VGPRs at NB = 2) nothing else would hide their latency.  The sum of one output runs over
//                       (chunk, a, b, channel in the chunk) in that order, and the MFMA is bit for bit the k-ordered fmaf chain,
//                       so the order is fixed by this one body.  The replica is blockIdx.z (0 for die_conv2d_wide), its weight
//                       row blockIdx.z / episodes: the batched launch IS the stand-alone launch one stride further.
//                       The accumulator layout (column = lane & 15 = channel, rows 4 (lane >> 4) + i = y) gives every lane 4
//                       consecutive y of one output plane: the VALU epilogue applies the activation, then die_rng.h's dropout
//                       mask (one Philox block per 4 cells where H % 4 == 0, cell by cell otherwise), then stores 16 bytes.
//
// Roofline.  A C -> C layer of kernel size k is 2 C^2 k^2 flop per cell against 8 C bytes (C planes in, C out, fp32):
// C k^2 / 4 flop per byte — 36 for 16 -> 16 at k = 3, 72 for 32 -> 32, past the ~ 20 flop/byte at which 157 TFLOP/s of fp32
// meet 8 TB/s: such a layer is compute-bound and its ceiling is the fp32 matrix rate (64 flop per clock per SIMD, the
// vector rate, with the VALU left free for the epilogue).  The first layer (3 -> C: 2 * 3 * C * 9 flop against 4 (3 + C) bytes,
// 11 flop/byte at C = 16) and the last (C -> 3) stay HBM-bound, and both pay for the padding to 4 channels / 16 outputs: the
// last layer of a 16-wide stack issues 16 / 3 of the MFMAs its outputs need.  LDS per workgroup at k = 5, NB = 2:
// 4 * 1360 * 4 = 21 760 bytes of tile + 25 * 2 * 64 * 4 = 12 800 bytes of weights, 34 560 of the 64 K.
#include <math.h>
#include "die_common.h"
#include "die_rng.h"
#include "die_nca.h"

struct WideArgs {
    const void* in[NCAW_MAXC];
    int kind[NCAW_MAXC];         // die_conv_plane.kind
    float* out;                  // output plane o at out + o * out_stride
    int64_t out_stride;
    const float* w;              // [cout][cin][k][k]
    int W, H, cin, cout, epoch;
    int act;                     // die_nca_activation of the epilogue
    int pad;                     // die_pad_mode
    int vec;                     // 16-byte stores: H % 4 == 0 and every output plane 16-byte aligned
    int drop;                    // 1: the epilogue multiplies by the dropout mask of `d`
    int episodes;                // replica r reads weight row r / episodes
    int64_t rep_in, rep_w, rep_out;  // elements from replica r's planes / weights / outputs to r + 1's (gridDim.z = replicas)
    DropWords d;
};

template <int K, int NB>
__global__ __launch_bounds__(DIE_BLOCK) void k_conv_wide(WideArgs a) {
    constexpr int R = K / 2, LX = NCA_TX + 2 * R, LY = NCA_TY + 2 * R;
    constexpr int CS = (LX * LY - 16 + 63) / 64 * 64 + 16;         // channel stride: 16 mod 64 words
    constexpr int MB = 16;                                          // M-blocks per wave: 4 rows x 4 blocks of 16 y
    __shared__ __align__(16) float s_in[NCAW_CH * CS];
    __shared__ __align__(16) float s_w[K * K * NB * NCAW_CH * 16];
    const int x0 = blockIdx.y * NCA_TX, y0 = blockIdx.x * NCA_TY;
    const int64_t rep = blockIdx.z;
    const int64_t row = a.episodes > 1 ? (int64_t)((int)blockIdx.z / a.episodes) : rep;
    const float* w = a.w + row * a.rep_w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lk = lane >> 4, ln = lane & 15;

    ncaw_f32x4 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[m][nb] = ncaw_f32x4{0.f, 0.f, 0.f, 0.f};

    // What a thread stages of every chunk is fixed: tile words i = tid, tid + 256, ... (word i of a channel's tile is cell
    // (i / LY, i % LY), so s_in's index is the channel's base + i) and weight words likewise; their global addresses are
    // worked out once.  A chunk goes global -> registers -> LDS, and the next chunk's loads are issued before this chunk's
    // MFMAs, so that their latency runs under the matrix work instead of in front of it.
    constexpr int NI = (LX * LY + DIE_BLOCK - 1) / DIE_BLOCK, NWI = (K * K * NB * NCAW_CH * 16 + DIE_BLOCK - 1) / DIE_BLOCK;
    int64_t cell[NI];                                              // (0 where the word reads as zero: `live` says which do not)
    int wbase[NWI];                                                // the word's offset in w for chunk 0 (0 for a zero word)
    unsigned live = 0, wlive = 0;                                  // bit t: word t is read from memory
#pragma unroll
    for (int t = 0; t < NI; ++t) {
        const int i = threadIdx.x + t * DIE_BLOCK, li = i / LY, lj = i - li * LY;
        // (rows / columns past the last tile's outputs wrap like a circular field whatever the mode: never used)
        const int vx = x0 - R + li, vy = y0 - R + lj;
        const int gx = nca_pad_index(vx < a.W + R ? vx : vx % a.W, a.W, a.pad), gy = nca_pad_index(vy < a.H + R ? vy : vy % a.H, a.H, a.pad);
        const bool ok = i < LX * LY && gx >= 0 && gy >= 0;
        cell[t] = rep * a.rep_in + (ok ? (int64_t)gx * a.H + gy : 0);
        live |= ok ? 1u << t : 0u;
    }
#pragma unroll
    for (int t = 0; t < NWI; ++t) {
        const int i = threadIdx.x + t * DIE_BLOCK, o = ((i >> 6) % NB) * 16 + (i & 15), tap = i / (64 * NB);
        const bool ok = i < K * K * NB * NCAW_CH * 16 && o < a.cout;
        wbase[t] = ok ? (o * a.cin + ((i >> 4) & 3)) * (K * K) + tap : 0;
        wlive |= ok ? 1u << t : 0u;
    }
    // The loads themselves are unconditional (a zero word reads cell 0 / weight 0 and is replaced when it is stored): a load
    // under a per-lane condition is a branch, and the loads of a chunk must all be in flight together.
    float pre[NI][NCAW_CH], wpre[NWI];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int t = 0; t < NWI; ++t) {
            const int c = c0 + (((threadIdx.x + t * DIE_BLOCK) >> 4) & 3);
            wpre[t] = w[c < a.cin ? wbase[t] + c0 * (K * K) : 0];
        }
#pragma unroll
        for (int j = 0; j < NCAW_CH; ++j) {
            const int c = c0 + j;                                   // (uniform: the plane's pointer and kind are scalar loads)
            if (c >= a.cin) continue;
            const void* p = a.in[c];
            const int kind = a.kind[c];
            if (kind == DIE_PLANE_F32) {
#pragma unroll
                for (int t = 0; t < NI; ++t) pre[t][j] = ((const float*)p)[cell[t]];
            } else {
#pragma unroll
                for (int t = 0; t < NI; ++t) pre[t][j] = nca_load(p, kind, cell[t], a.epoch);
            }
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < a.cin; c0 += NCAW_CH) {
        if (c0) __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int t = 0; t < NWI; ++t) {
            const int i = threadIdx.x + t * DIE_BLOCK;
            const int c = c0 + ((i >> 4) & 3);
            if (i < K * K * NB * NCAW_CH * 16) s_w[i] = ((wlive >> t) & 1) && c < a.cin ? wpre[t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NI; ++t) {
            const int i = threadIdx.x + t * DIE_BLOCK;
            if (i < LX * LY) {
#pragma unroll
                for (int j = 0; j < NCAW_CH; ++j) s_in[j * CS + i] = ((live >> t) & 1) && c0 + j < a.cin ? pre[t][j] : 0.f;
            }
        }
        __syncthreads();
        if (c0 + NCAW_CH < a.cin) fetch(c0 + NCAW_CH);
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

    const uint64_t key = a.d.seed + (uint64_t)blockIdx.z * a.d.seed_stride;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int gx = x0 + wave * 4 + (m >> 2), gy = y0 + (m & 3) * 16 + lk * 4;      // this lane's 4 cells: (gx, gy .. gy + 3)
        if (gx >= a.W || gy >= a.H) continue;
        float mask[4] = {1.f, 1.f, 1.f, 1.f};
        if (a.drop) {
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
        for (int nb = 0; nb < NB; ++nb) {
            const int o = nb * 16 + ln;
            if (o >= a.cout) continue;
            float v[4] = {acc[m][nb][0], acc[m][nb][1], acc[m][nb][2], acc[m][nb][3]};
            if (a.act == DIE_NCA_ACT_TANH) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tanhf(v[q]);
            } else if (a.act == DIE_NCA_ACT_RELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] > 0.f ? v[q] : 0.f;
            }
            if (a.drop) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] * mask[q];
            }
            float* dst = a.out + (int64_t)o * a.out_stride + rep * a.rep_out + (int64_t)gx * a.H + gy;
            if (a.vec) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (gy + q < a.H) dst[q] = v[q];
            }
        }
    }
}

static void launch_wide(const WideArgs& a, int k, int replicas, hipStream_t s) {
    dim3 grid((a.H + NCA_TY - 1) / NCA_TY, (a.W + NCA_TX - 1) / NCA_TX, replicas);
    const bool two = a.cout > 16;
    switch (k) {
        case 1: if (two) k_conv_wide<1, 2><<<grid, DIE_BLOCK, 0, s>>>(a); else k_conv_wide<1, 1><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        case 3: if (two) k_conv_wide<3, 2><<<grid, DIE_BLOCK, 0, s>>>(a); else k_conv_wide<3, 1><<<grid, DIE_BLOCK, 0, s>>>(a); break;
        default: if (two) k_conv_wide<5, 2><<<grid, DIE_BLOCK, 0, s>>>(a); else k_conv_wide<5, 1><<<grid, DIE_BLOCK, 0, s>>>(a); break;
    }
}

static bool wide_vec(const float* out, int64_t out_stride, int64_t rep_out, int H) {
    return (H & 3) == 0 && (out_stride & 3) == 0 && (rep_out & 3) == 0 && ((uintptr_t)out & 15) == 0;
}

extern "C" int die_conv2d_wide(int32_t W, int32_t H, int32_t cin, const die_conv_plane* in, int32_t epoch, int32_t cout, float* out,
                               int64_t out_stride, int32_t k, const float* weights, int32_t activation, int32_t padding_mode,
                               const die_nca_dropout* drop, void* stream) {
    const char* who = "die_conv2d_wide";
    DIE_REQUIRE(padding_mode >= DIE_PAD_CIRCULAR && padding_mode <= DIE_PAD_REPLICATE, "%s: bad padding mode %d", who, padding_mode);
    DIE_REQUIRE(W >= 1 && H >= 1, "%s: bad size %dx%d", who, W, H);
    DIE_REQUIRE((W + NCA_TX - 1) / NCA_TX <= 65535, "%s: field too tall", who);
    DIE_REQUIRE(cin >= 1 && cin <= NCAW_MAXC && cout >= 1 && cout <= NCAW_MAXC, "%s: 1..%d channels (got %d -> %d)", who, NCAW_MAXC, cin, cout);
    DIE_REQUIRE(k == 1 || k == 3 || k == 5, "%s: kernel size %d (1, 3 or 5)", who, k);
    DIE_REQUIRE(padding_mode != DIE_PAD_REFLECT || (k / 2 < W && k / 2 < H), "%s: 'reflect' padding of %d cells needs a field larger than "
                "that (%dx%d)", who, k / 2, W, H);
    DIE_REQUIRE(activation >= DIE_NCA_ACT_NONE && activation <= DIE_NCA_ACT_RELU, "%s: bad activation %d", who, activation);
    DIE_REQUIRE(in && out && weights, "%s: null argument", who);
    const int64_t cells = (int64_t)W * H;
    DIE_REQUIRE(out_stride >= cells, "%s: out_stride %lld smaller than a plane (%lld cells)", who, (long long)out_stride, (long long)cells);
    WideArgs a = {};
    const char *o0 = (const char*)out, *o1 = (const char*)(out + (int64_t)(cout - 1) * out_stride + cells);
    for (int c = 0; c < cin; ++c) {
        // (a stock plane is the observation's LAST channel, DESIGN §6: kind 3 anywhere else is a plane of no kind, as it always was)
        DIE_REQUIRE(in[c].data && in[c].kind >= DIE_PLANE_F32 && in[c].kind <= (c == cin - 1 ? DIE_PLANE_STOCK : DIE_PLANE_AGENTS),
                    "%s: bad input plane %d", who, c);
        const int64_t bytes = cells * (in[c].kind == DIE_PLANE_F32 ? 4 : in[c].kind == DIE_PLANE_F16 ? 2 : 8);
        const char* p = (const char*)in[c].data;
        DIE_REQUIRE(p + bytes <= o0 || p >= o1, "%s: in-place convolution (input plane %d lies in the output planes)", who, c);
        a.in[c] = in[c].data; a.kind[c] = in[c].kind;
    }
    if (drop) {
        const int rc = die_dropout_words(drop, &a.d, who);
        if (rc != DIE_OK) return rc;
        a.drop = 1;
    }
    a.out = out; a.out_stride = out_stride; a.w = weights;
    a.W = W; a.H = H; a.cin = cin; a.cout = cout; a.epoch = epoch; a.act = activation; a.pad = padding_mode;
    a.episodes = 1;
    a.vec = wide_vec(out, out_stride, 0, H);
    launch_wide(a, k, 1, (hipStream_t)stream);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- what a valid stack is, narrow (die_nca.hip's kernels) or wide: one walk, and the two kinds' limits -------------------------
struct NcaLimits {
    int max_channels, max_k;     // cout in 1..max_channels, k odd in 1..max_k
    const char* k_text;          // … as the refusal names them (a format: %d is max_k)
    bool activation;             // die_nca_layer.reserved is the layer's die_nca_activation (the last layer's: tanh)
};
static const NcaLimits nca_limits[2] = {{NCA_MAXC, NCA_MAXK, "odd sizes up to %d", false}, {NCAW_MAXC, 5, "1, 3 or 5", true}};

int die_nca_stack_check(die_nca_kind kind, const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who, bool scratch,
                        bool stock, int memory, int signals) {
    const bool wide = kind == DIE_NCA_WIDE;
    const NcaLimits& lim = nca_limits[kind];
    if (scratch) DIE_REQUIRE(nca && nca->layers && nca->scratch, "%s: null stack, layer list or scratch", who);
    else DIE_REQUIRE(nca && nca->layers, "%s: null stack or layer list", who);
    DIE_REQUIRE(nca->n_layers >= 1 && nca->n_layers <= DIE_NCA_MAX_LAYERS, "%s: 1..%d layers (got %d)", who, DIE_NCA_MAX_LAYERS, nca->n_layers);
    DIE_REQUIRE(nca->padding_mode >= DIE_PAD_CIRCULAR && nca->padding_mode <= DIE_PAD_REPLICATE, "%s: bad padding mode %d", who, nca->padding_mode);
    DIE_REQUIRE(nca->with_agent_channel == 0 || nca->with_agent_channel == 1, "%s: with_agent_channel is 0 or 1", who);
    DIE_REQUIRE(nca->episodes >= 0 && replicas % (nca->episodes > 1 ? nca->episodes : 1) == 0, "%s: episodes %d: at least 1 (0 reads as 1) "
                "and a divisor of the %d replicas", who, nca->episodes, replicas);
    DIE_REQUIRE(W >= 1 && H >= 1 && replicas >= 1 && replicas <= DIE_MAX_REPLICAS, "%s: bad size %dx%d or replicas %d outside 1..%d", who,
                W, H, replicas, DIE_MAX_REPLICAS);
    // the ping-pong planes: NCA_MAXC a replica for a narrow stack, asked for before its layers; the widest cout for a wide one, after
    auto scratch_check = [&](int channels) -> int {
        const int64_t need = (int64_t)die_nca_pingpong_sets(nca->n_layers) * replicas * channels * (int64_t)W * H * (int64_t)sizeof(float);
        DIE_REQUIRE(nca->scratch_bytes >= need, "%s: scratch too small (%lld < %lld)", who, (long long)nca->scratch_bytes, (long long)need);
        return DIE_OK;
    };
    if (wide) DIE_REQUIRE((W + NCA_TX - 1) / NCA_TX <= 65535, "%s: field too tall", who);
    else if (scratch && scratch_check(NCA_MAXC) != DIE_OK) return DIE_ERR_ARG;
    int cin = 2 + nca->with_agent_channel + signals + memory + (stock ? 1 : 0);
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        if (!(L.k >= 1 && L.k <= lim.max_k && (L.k & 1))) {
            char sizes[32];
            snprintf(sizes, sizeof(sizes), lim.k_text, lim.max_k);
            die_set_error("%s: layer %d: kernel size %d (%s)", who, l, L.k, sizes);
            return DIE_ERR_ARG;
        }
        DIE_REQUIRE(L.cin == cin && L.cout >= 1 && L.cout <= lim.max_channels, "%s: layer %d: %d -> %d channels (input has %d, at most %d out)",
                    who, l, L.cin, L.cout, cin, lim.max_channels);
        DIE_REQUIRE(!lim.activation || (L.reserved >= DIE_NCA_ACT_NONE && L.reserved <= DIE_NCA_ACT_RELU &&
                                        (l < nca->n_layers - 1 || L.reserved == DIE_NCA_ACT_TANH)),
                    "%s: layer %d: activation %d (0 none, 1 tanh, 2 relu; the last layer's is tanh)", who, l, L.reserved);
        DIE_REQUIRE(L.weights && L.weight_stride >= (int64_t)L.cout * L.cin * L.k * L.k, "%s: layer %d: null weights or stride below a "
                    "replica's block", who, l);
        DIE_REQUIRE(nca->padding_mode != DIE_PAD_REFLECT || (L.k / 2 < W && L.k / 2 < H), "%s: layer %d: 'reflect' padding of %d cells "
                    "needs a field larger than that (%dx%d)", who, l, L.k / 2, W, H);
        cin = L.cout;
    }
    if (signals) DIE_REQUIRE(cin == 3 + signals + memory, "%s: the last layer gives %d planes (dx, dy, deposit, %d signal and %d memory planes: %d)",
                             who, cin, signals, memory, 3 + signals + memory);
    else if (memory) DIE_REQUIRE(cin == 3 + memory, "%s: the last layer gives %d planes (dx, dy, deposit and %d memory planes: %d)", who, cin,
                            memory, 3 + memory);
    else DIE_REQUIRE(cin == 3, "%s: the last layer gives %d planes (dx, dy, deposit: 3)", who, cin);
    return wide && scratch ? scratch_check(die_nca_max_channels(nca)) : DIE_OK;
}

// ---- die_nca_wide_env_step_batch's sensing (the step itself: die_env.hip) ---------------------------------------------
// Scratch: [set][replica][max_channels][W][H] fp32, set = layer % 2 (one set for a single layer), max_channels the widest
// cout of the stack; the last layer's three planes stay there until the next step (BatchedNeuralAutomataAgent.render).
extern "C" int64_t die_nca_wide_batch_scratch_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers, int32_t max_channels) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS || n_layers < 1 || n_layers > DIE_NCA_MAX_LAYERS ||
        max_channels < 1 || max_channels > NCAW_MAXC) return -1;
    return (int64_t)die_nca_pingpong_sets(n_layers) * replicas * max_channels * (int64_t)W * H * (int64_t)sizeof(float);
}

// the stack for every replica, one launch per layer.  Layer l writes `dst` + set(l) * R * rep planes: set(l) = l % 2 for the
// step's ping-pong scratch, l for caller-owned storage that keeps every layer.  `drop` (checked words, or null): the last layer's
// launch is the masked one — into `masked` when given (the unmasked launch then runs as well and keeps its place), else in place
// of it.  *sense = the last layer's planes of replica 0, replica r's *rep further (what die_nca_sense_batch returns for a narrow
// stack: k_nca_move_claim_batch reads either)
// `stock`, `mem_planes` with `memory` (or null / 0): the stock planes built at sense_epoch and the memory planes, layer 0's inputs
// after the field's (die_nca.h die_nca_layer0_planes: the one list of them)
static int wide_sense_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* dst, bool pingpong, float* masked,
                            const float** sense, int64_t* rep, const DropWords* drop, void* stream, const unsigned long long* stock = nullptr,
                            const float* mem_planes = nullptr, int memory = 0, const float* signal_planes = nullptr, int signals = 0) {
    const int64_t cells = (int64_t)m->W * m->H, rep_scratch = die_nca_max_channels(nca) * cells;
    WideArgs a = {};
    die_nca_layer0_planes(m, b, nca, mem_planes, memory, stock, a.in, a.kind, &a.rep_in, signal_planes, signals);
    a.W = m->W; a.H = m->H; a.epoch = nca->sense_epoch; a.pad = nca->padding_mode;
    a.episodes = nca->episodes > 1 ? nca->episodes : 1;
    a.out_stride = cells; a.rep_out = rep_scratch;
    for (int l = 0; l < nca->n_layers; ++l) {
        const die_nca_layer& L = nca->layers[l];
        const bool last = l == nca->n_layers - 1;
        a.out = dst + (pingpong ? l % die_nca_pingpong_sets(nca->n_layers) : l) * b->replicas * rep_scratch;
        a.w = L.weights; a.rep_w = L.weight_stride;
        a.cin = L.cin; a.cout = L.cout; a.act = L.reserved;
        a.vec = wide_vec(a.out, a.out_stride, a.rep_out, a.H);
        a.drop = last && drop && !masked;
        if (last && drop) a.d = *drop;
        launch_wide(a, L.k, b->replicas, (hipStream_t)stream);
        DIE_CHECK_LAUNCH("die_nca_wide_env_step_batch(conv)");
        if (last && drop && masked) {
            a.out = masked;
            a.vec = wide_vec(a.out, a.out_stride, a.rep_out, a.H);
            a.drop = 1;
            launch_wide(a, L.k, b->replicas, (hipStream_t)stream);
            DIE_CHECK_LAUNCH("die_nca_wide_sense_batch_store(masked)");
        }
        for (int o = 0; o < L.cout; ++o) { a.in[o] = a.out + o * cells; a.kind[o] = DIE_PLANE_F32; }
        a.rep_in = rep_scratch;
    }
    *sense = a.out;
    *rep = rep_scratch;
    return DIE_OK;
}

int die_nca_wide_sense_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float** sense, int64_t* rep,
                             const DropWords* drop, void* stream, const unsigned long long* stock, const float* mem_planes, int memory,
                             const float* signal_planes, int signals) {
    return wide_sense_batch(m, b, nca, nca->scratch, true, nullptr, sense, rep, drop, stream, stock, mem_planes, memory, signal_planes, signals);
}

// ---- the same launches into storage that keeps every layer (the forward of die_nca_wide_backward_batch) -----------------
extern "C" int64_t die_nca_wide_sense_batch_store_bytes(int32_t W, int32_t H, int32_t replicas, int32_t n_layers, int32_t max_channels) {
    if (W < 1 || H < 1 || replicas < 1 || replicas > DIE_MAX_REPLICAS || n_layers < 1 || n_layers > DIE_NCA_MAX_LAYERS ||
        max_channels < 1 || max_channels > NCAW_MAXC || (W + NCA_TX - 1) / NCA_TX > 65535) return -1;
    return (int64_t)n_layers * replicas * max_channels * (int64_t)W * H * (int64_t)sizeof(float);
}

// Everything the three entry points below share once their own leading argument checks have passed: the stack's and the store's
// rules, the mask's, the overlap of the planes layer 0 reads (`memory` / `signals` of them, 0 with null planes: none) with what
// the launches write, and the launches.
static int wide_sense_batch_store(const char* who, const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store,
                                  int64_t store_bytes, float* masked, const die_nca_dropout* drop, const float* mem_planes, int memory,
                                  const float* signal_planes, int signals, void* stream) {
    int rc = die_nca_store_check(m, b, nca, store, DIE_NCA_WIDE, who, memory, signals);
    if (rc != DIE_OK) return rc;
    const int64_t need = die_nca_wide_sense_batch_store_bytes(m->W, m->H, b->replicas, nca->n_layers, die_nca_max_channels(nca));
    DIE_REQUIRE(store_bytes >= need, "%s: store too small (%lld < %lld)", who, (long long)store_bytes, (long long)need);
    DropWords dw;
    if (drop) {
        DIE_REQUIRE(masked && masked != store, "%s: a dropout mask needs planes of its own for the masked values", who);
        rc = die_dropout_words(drop, &dw, who);
        if (rc != DIE_OK) return rc;
    }
    // the memory and the signal planes are read by layer 0 while the store (and the masked planes) are written
    const int64_t cells = (int64_t)m->W * m->H, masked_bytes = (int64_t)b->replicas * die_nca_max_channels(nca) * cells * 4;
    auto planes_bytes = [&](int n) { return (((int64_t)n * b->replicas - 1) * b->plane_stride + cells) * 4; };
    auto overlaps = [&](const void* p, int64_t bytes) {
        return die_ranges_overlap(p, bytes, store, need) || (drop && die_ranges_overlap(p, bytes, masked, masked_bytes));
    };
    if (memory > 0)
        DIE_REQUIRE(!overlaps(mem_planes, planes_bytes(memory)), "%s: the memory planes overlap the store or the masked planes", who);
    if (signals > 0)
        DIE_REQUIRE(!overlaps(signal_planes, planes_bytes(signals)), "%s: the signal planes overlap the store or the masked planes", who);
    const float* sense;
    int64_t rep;
    return wide_sense_batch(m, b, nca, store, false, drop ? masked : nullptr, &sense, &rep, drop ? &dw : nullptr, stream, nullptr,
                            mem_planes, memory, signal_planes, signals);
}

extern "C" int die_nca_wide_sense_batch_store(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store,
                                              int64_t store_bytes, float* masked, const die_nca_dropout* drop, void* stream) {
    return wide_sense_batch_store("die_nca_wide_sense_batch_store", m, b, nca, store, store_bytes, masked, drop, nullptr, 0, nullptr, 0, stream);
}

// ---- the same for a population whose agents carry memory (the forward of die_nca_wide_backward_batch_memory) --------------
// Layer 0 reads ([agents,] food, chem, memory_0 .. memory_{M-1}), the last layer gives 3 + M planes; the tanh and the mask fall
// on all of them (k_conv_wide's epilogue knows no plane from another).  The launches are die_nca_wide_sense_batch_store's.
// Roofline: k_conv_wide's, above — the M planes are M more fp32 planes in and out of the first and the last layer (HBM-bound
// both, 4 bytes a cell and plane): the last layer's 3 + M outputs stay inside one 16-channel block up to M = 8, layer 0 stages
// ceil((3 + M) / 4) chunks of 4 input channels where it staged one.
extern "C" int die_nca_wide_sense_batch_store_memory(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store,
                                                     int64_t store_bytes, float* masked, const die_nca_dropout* drop, const float* mem_planes,
                                                     int32_t memory_channels, void* stream) {
    const char* who = "die_nca_wide_sense_batch_store_memory";
    DIE_REQUIRE(m && b && nca && store && mem_planes, "%s: null argument", who);
    DIE_REQUIRE(memory_channels >= 1 && memory_channels <= DIE_MEMORY_MAX_CHANNELS, "%s: %d memory channels outside 1..%d", who,
                memory_channels, DIE_MEMORY_MAX_CHANNELS);
    return wide_sense_batch_store(who, m, b, nca, store, store_bytes, masked, drop, mem_planes, memory_channels, nullptr, 0, stream);
}

// ---- the same for a population whose agents also write a signal field (the forward of die_nca_wide_backward_batch_signal) --------
// Layer 0 reads ([agents,] food, chem, signal_0 .., memory_0 ..), the last layer gives 3 + K + M planes; M = 0 with null mem_planes:
// no memory.  The launches are die_nca_wide_sense_batch_store's; the K planes cost what M more memory planes would (above).
extern "C" int die_nca_wide_sense_batch_store_signal(const die_medium* m, const die_batch* b, const die_nca_batch* nca, float* store,
                                                     int64_t store_bytes, float* masked, const die_nca_dropout* drop, const float* mem_planes,
                                                     int32_t memory_channels, const float* signal_planes, int32_t signal_channels,
                                                     void* stream) {
    const char* who = "die_nca_wide_sense_batch_store_signal";
    DIE_REQUIRE(m && b && nca && store && signal_planes, "%s: null argument", who);
    DIE_REQUIRE(memory_channels >= 0 && memory_channels <= DIE_MEMORY_MAX_CHANNELS && (memory_channels > 0) == (mem_planes != nullptr),
                "%s: %d memory channels outside 0..%d, or not 0 exactly where the memory planes are null", who, memory_channels,
                DIE_MEMORY_MAX_CHANNELS);
    DIE_REQUIRE(signal_channels >= 1 && signal_channels <= DIE_SIGNAL_MAX_CHANNELS, "%s: %d signal channels outside 1..%d", who,
                signal_channels, DIE_SIGNAL_MAX_CHANNELS);
    return wide_sense_batch_store(who, m, b, nca, store, store_bytes, masked, drop, mem_planes, memory_channels, signal_planes,
                                  signal_channels, stream);
}
