// The adjoint of the signal channels' update (gfx950) — what die_amd.functional.signal_step records and backpropagates
// (NeuralAutomataAgent.signalling_action).  The forward, die_signal.hip:
//
//     F' = (1 - decay) * G(F + occ ⊙ deposit * S)          G: the periodic symmetric gaussian of die_diffuse_rows.inc / _tile.inc
//
// On the torus Gᵀ = G (die_env_grad.hip argues it at its top, tests/test_gpu_field_step_grad.py proves it), so with g = grad_F':
//
//     grad_F      = (1 - decay) * G(g)                      the forward's own sweep on the gradient planes
//     grad_S_k[c] = occ[c] ? deposit * grad_F_k[c] : +0     a masked multiply of what the sweep is about to store
//
//   k_signal_cells          the record: occupied[c] = die_claim_occupied(standing[c], epoch) ? 1 : 0, one byte a cell.  A graph that
//                           keeps this plane survives the next standing build, every step, re-sort and reset_signals(); a T-step
//                           unroll holds 1 byte per cell and step instead of the standing plane's 8, and the backward sweep reads 1.
//                           16 cells per thread: 128 bytes of words in, one 16-byte store out; the tail and an unaligned plane go
//                           byte by byte.  Plain vector loads and stores.
//   k_signal_cells_batch    the same body for every replica of a die_batch in ONE launch, the replica in blockIdx.y (as the batched
//                           memory kernels): replica r's words b->plane_stride on, its bytes occupied_stride on.
//   k_signal_back_rows<R>   the row-marching sweep with the plane read as it is (an empty DIF_EMIT) and a DIF_STORE that writes the 4
//   k_signal_back_tile<R>   finished values o to grad_field and occ ? deposit * o : +0 to grad_emission (the LDS-tiled sweep: cell by
//                           cell, a plain DIF_LOAD).  Either output may be absent.  One launch for all K planes of all replicas,
//                           plane z = blockIdx.z being channel k = z / replicas of replica r = z % replicas as in die_signal.hip.
//
// Roofline: 4 + 1 bytes in and up to 8 out per cell and channel against the forward's 20 — below what the memory system notices on the
// worlds this path is for, where the launch is the cost; bandwidth-bound like the sweep it instantiates on large ones (LABBOOK §43).
#include <math.h>
#include "die_forward.h"
#include "die_nca.h"
#include "die_diffuse.h"

// ---- the record ------------------------------------------------------------------------------------------------------------------
#define CELLS_PER_THREAD 16

template <bool VEC>
__global__ __launch_bounds__(DIE_BLOCK) void k_signal_cells(const unsigned long long* __restrict__ standing, int64_t cells, int epoch,
                                                            uint8_t* __restrict__ out) {
    const int64_t groups = VEC ? cells / CELLS_PER_THREAD : 0;                  // whole 16-byte groups, then the tail byte by byte
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t g = t0; g < groups; g += stride) {
        const int64_t base = g * CELLS_PER_THREAD;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const ulonglong2 c01 = *(const ulonglong2*)(standing + base + 4 * q), c23 = *(const ulonglong2*)(standing + base + 4 * q + 2);
            w[q] = (die_claim_occupied(c01.x, epoch) ? 1u : 0u) | (die_claim_occupied(c01.y, epoch) ? 1u << 8 : 0u) |
                   (die_claim_occupied(c23.x, epoch) ? 1u << 16 : 0u) | (die_claim_occupied(c23.y, epoch) ? 1u << 24 : 0u);
        }
        *(uint4*)(out + base) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int64_t c = groups * CELLS_PER_THREAD + t0; c < cells; c += stride) out[c] = die_claim_occupied(standing[c], epoch) ? 1 : 0;
}

// the record of every replica: replica r = blockIdx.y, its standing plane standing_rep words on, its byte plane out_rep bytes on; from
// there k_signal_cells' statements (a kernel of its own: as a shared inlined body they moved k_signal_cells' registers)
template <bool VEC>
__global__ __launch_bounds__(DIE_BLOCK) void k_signal_cells_batch(const unsigned long long* __restrict__ standing, int64_t standing_rep,
                                                                  int64_t cells, int epoch, uint8_t* __restrict__ out, int64_t out_rep) {
    standing += standing_rep * blockIdx.y;
    out += out_rep * blockIdx.y;
    const int64_t groups = VEC ? cells / CELLS_PER_THREAD : 0;                  // whole 16-byte groups, then the tail byte by byte
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t g = t0; g < groups; g += stride) {
        const int64_t base = g * CELLS_PER_THREAD;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const ulonglong2 c01 = *(const ulonglong2*)(standing + base + 4 * q), c23 = *(const ulonglong2*)(standing + base + 4 * q + 2);
            w[q] = (die_claim_occupied(c01.x, epoch) ? 1u : 0u) | (die_claim_occupied(c01.y, epoch) ? 1u << 8 : 0u) |
                   (die_claim_occupied(c23.x, epoch) ? 1u << 16 : 0u) | (die_claim_occupied(c23.y, epoch) ? 1u << 24 : 0u);
        }
        *(uint4*)(out + base) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int64_t c = groups * CELLS_PER_THREAD + t0; c < cells; c += stride) out[c] = die_claim_occupied(standing[c], epoch) ? 1 : 0;
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------------
struct SignalBackArgs {
    const uint8_t* occupied;                 // replica r's mask plane occ_rep bytes on
    float* grad_emission;                    // null, or plane k of replica r at grad_emission + k * em_plane + r * em_rep
    int64_t occ_rep, em_plane, em_rep, field_stride;
    int replicas, has_field;                 // has_field 0: grad_field is absent
    float deposit;
};

// the one statement of grad_S: a multiply of its own (build.py's -ffp-contract=on fuses inside one expression only), then the mask
__device__ __forceinline__ float signal_back(float o, uint32_t occ, float deposit) {
    const float e = deposit * o;
    return occ ? e : 0.f;
}

// the mask and the emission gradient of the plane this workgroup sweeps: channel k = z / replicas of replica r = z % replicas
struct SignalBack {
    const uint8_t* occupied;
    float* grad_emission;
    bool has_field;
    float deposit;
    __device__ __forceinline__ SignalBack(const SignalBackArgs& s) {
        const int k = (int)blockIdx.z / s.replicas, r = (int)blockIdx.z - k * s.replicas;
        occupied = s.occupied + s.occ_rep * r;
        grad_emission = s.grad_emission ? s.grad_emission + s.em_plane * k + s.em_rep * r : nullptr;
        has_field = s.has_field != 0; deposit = s.deposit;
    }
    // 4 finished cells at plane offset `off` (a multiple of 4; 16-byte aligned planes, a 4-byte aligned mask): the lane's 4 mask bytes
    // are one 32-bit load
    __device__ __forceinline__ void store4(float* dst, int64_t off, const float* o) const {
        if (has_field) Vec4<float>::st(dst + off, o);
        if (grad_emission) {
            const uint32_t m = *(const uint32_t*)(occupied + off);
            const float e[4] = {signal_back(o[0], m & 0xffu, deposit), signal_back(o[1], m & 0xff00u, deposit),
                                signal_back(o[2], m & 0xff0000u, deposit), signal_back(o[3], m & 0xff000000u, deposit)};
            Vec4<float>::st(grad_emission + off, e);
        }
    }
    __device__ __forceinline__ void store(float* dst, int64_t i, float o) const {
        if (has_field) die_st(dst, i, o);
        if (grad_emission) grad_emission[i] = signal_back(o, occupied[i], deposit);
    }
};

template <int R>
__global__ __launch_bounds__(DIF_BLOCK) void k_signal_back_rows(RowsArgs a, SignalBackArgs s) {
    static_assert(R >= 1 && R <= 4, "one halo lane of 4 columns per side");
    using T = float;
    constexpr int FUSED = 0, row0 = 0;
    constexpr bool WRAP = true;
    const SignalBack back(s);
    const int64_t plane = a.rep_cells * blockIdx.z;
    a.src = (const float*)a.src + plane;
    if (s.has_field) a.dst = (float*)a.dst + plane;
#define DIF_EMIT(off, v)
#define DIF_STORE(dst, off, o) back.store4(dst, off, o);
#include "die_diffuse_rows.inc"
#undef DIF_STORE
#undef DIF_EMIT
}

template <int R>
__global__ __launch_bounds__(DIE_BLOCK) void k_signal_back_tile(DiffuseArgs a, SignalBackArgs s) {
    using T = float;
    const SignalBack back(s);
    const int64_t plane = s.field_stride * blockIdx.z;
    a.src = (const float*)a.src + plane;
    if (s.has_field) a.dst = (float*)a.dst + plane;
#define DIF_LOAD(src, i) die_ld(src, i)
#define DIF_STORE(dst, i, v) back.store(dst, i, v);
#include "die_diffuse_tile.inc"
#undef DIF_STORE
#undef DIF_LOAD
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- the launch alone: every argument has been checked by the caller ---------------------------------------------------------------
// gradient plane k of replica r at grad_next / grad_field + (k * replicas + r) * field_stride (the forward's field layout), replica
// r's mask plane occ_rep bytes on, its emission gradient's plane k at grad_emission + k * em_plane + r * em_rep
int die_signal_backward_launch(int32_t W, int32_t H, int32_t replicas, int32_t K, const uint8_t* occupied, int64_t occ_rep, const float* grad_next,
                               float* grad_field, int64_t field_stride, float* grad_emission, int64_t em_plane, int64_t em_rep, float deposit,
                               float sigma, float decay, void* stream, const char* who) {
    double wd[2 * DIF_MAXR + 1];
    const int R = die_gaussian_taps(sigma, wd);
    const float keep = (float)(1.0 - (double)decay);
    const int planes = K * replicas;
    hipStream_t s = (hipStream_t)stream;
    SignalBackArgs sa;
    sa.occupied = occupied; sa.grad_emission = grad_emission; sa.occ_rep = occ_rep; sa.em_plane = em_plane; sa.em_rep = em_rep;
    sa.field_stride = field_stride; sa.replicas = replicas; sa.has_field = grad_field != nullptr; sa.deposit = deposit;
    // 16-byte accesses: whole groups of 4 cells, every plane of every replica on a 16-byte boundary, the 4 mask bytes of a group one word
    const bool vec = rows_kernel_applies(W, H, R) && aligned16(grad_next) && aligned16(grad_field) && aligned16(grad_emission) &&
                     ((uintptr_t)occupied & 3) == 0 && (field_stride & 3) == 0 && (em_plane & 3) == 0 && (em_rep & 3) == 0 && (occ_rep & 3) == 0;
    if (vec) {
        RowsArgs ra;
        ra.src = grad_next; ra.dst = grad_field; ra.claim = nullptr; ra.dep = nullptr; ra.food = nullptr; ra.W = W; ra.H = H; ra.epoch = 0; ra.halo = 0;
        ra.rep_cells = field_stride;
        ra.wrapx = ra.wrapy = 1; ra.part_gain = nullptr; ra.part_gain2 = nullptr; ra.part_alive = nullptr; ra.n_part = 0; ra.result = nullptr;
        ra.alive_const = 0; ra.food_infinite = 1; ra.keep = keep; ra.rate_feed = 0.f;
        for (int k = 0; k <= 2 * 4; ++k) ra.w[k] = k <= 2 * R ? (float)wd[k] : 0.f;
        const int strips = (H + DIF_WCOLS - 1) / DIF_WCOLS;
        constexpr int WPB = DIF_BLOCK / DIE_WAVE;
        ra.rpw = die_rows_per_wave(W, H, planes);
        const int64_t gy = ((int64_t)W + ra.rpw - 1) / ra.rpw;
        DIE_REQUIRE(gy <= 65535, "%s: field too tall (%d rows)", who, W);
        const dim3 grid((strips + WPB - 1) / WPB, (unsigned)gy, planes);
        switch (R) {
            case 1: k_signal_back_rows<1><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
            case 2: k_signal_back_rows<2><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
            case 3: k_signal_back_rows<3><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
            default: k_signal_back_rows<4><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
        }
    } else {
        DiffuseArgs a;
        a.src = grad_next; a.dst = grad_field; a.W = W; a.H = H; a.mode = DIE_DIFFUSE_WRAP; a.keep = keep;
        for (int k = 0; k <= 2 * DIF_MAXR; ++k) a.w[k] = k <= 2 * R ? (float)wd[k] : 0.f;
        DIE_REQUIRE((W + DIF_TX - 1) / DIF_TX <= 65535, "%s: field too tall (%d rows)", who, W);
        const dim3 grid((H + DIF_TY - 1) / DIF_TY, (W + DIF_TX - 1) / DIF_TX, planes);
        switch (R) {
            case 1: k_signal_back_tile<1><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 2: k_signal_back_tile<2><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 3: k_signal_back_tile<3><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 4: k_signal_back_tile<4><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 5: k_signal_back_tile<5><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 6: k_signal_back_tile<6><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 7: k_signal_back_tile<7><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            default: k_signal_back_tile<8><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
        }
    }
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_signal_cells(const die_medium* m, const unsigned long long* standing, int32_t epoch, uint8_t* occupied_out, void* stream) {
    const char* who = "die_signal_cells";
    DIE_REQUIRE(m && standing && occupied_out, "%s: null argument", who);
    const int rc = die_signal_check(m, 1, epoch, 0.f, 0.5f, 0.f, who);          // (size, a decomposed medium, the epoch: die_signal_step's rules)
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    DIE_REQUIRE(!die_ranges_overlap(occupied_out, cells, standing, cells * 8), "%s: occupied_out overlaps the standing plane", who);
    const bool vec = aligned16(standing) && aligned16(occupied_out);
    const int64_t threads = vec ? (cells + CELLS_PER_THREAD - 1) / CELLS_PER_THREAD : cells;
    const int64_t g = (threads + DIE_BLOCK - 1) / DIE_BLOCK;
    const int grid = (int)(g < 8192 ? g : 8192);
    if (vec) k_signal_cells<true><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(standing, cells, epoch, occupied_out);
    else k_signal_cells<false><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(standing, cells, epoch, occupied_out);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_signal_cells_batch(const die_medium* m, const die_batch* b, const unsigned long long* standing, int32_t epoch,
                                      uint8_t* occupied_out, int64_t occupied_stride, void* stream) {
    const char* who = "die_signal_cells_batch";
    DIE_REQUIRE(m && b && standing && occupied_out, "%s: null argument", who);
    int rc = die_signal_check(m, 1, epoch, 0.f, 0.5f, 0.f, who);                // (size, a decomposed medium, the epoch: die_signal_cells' rules)
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H;
    rc = die_batch_check(b, cells, who);
    if (rc != DIE_OK) return rc;
    const int64_t R = b->replicas;
    DIE_REQUIRE(occupied_stride >= cells, "%s: occupied_stride %lld smaller than a plane (%lld cells)", who, (long long)occupied_stride,
                (long long)cells);
    DIE_REQUIRE(!die_ranges_overlap(occupied_out, (R - 1) * occupied_stride + cells, standing, ((R - 1) * b->plane_stride + cells) * 8),
                "%s: occupied_out overlaps the standing planes", who);
    // 16-byte accesses: every replica's words and bytes on a 16-byte boundary
    const bool vec = aligned16(standing) && aligned16(occupied_out) && (b->plane_stride & 1) == 0 && (occupied_stride & 15) == 0;
    const int64_t threads = vec ? (cells + CELLS_PER_THREAD - 1) / CELLS_PER_THREAD : cells;
    const int64_t g = (threads + DIE_BLOCK - 1) / DIE_BLOCK;
    const dim3 grid((unsigned)(g < 8192 ? g : 8192), (unsigned)R);
    if (vec) k_signal_cells_batch<true><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(standing, b->plane_stride, cells, epoch, occupied_out, occupied_stride);
    else k_signal_cells_batch<false><<<grid, DIE_BLOCK, 0, (hipStream_t)stream>>>(standing, b->plane_stride, cells, epoch, occupied_out, occupied_stride);
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

extern "C" int die_signal_step_backward(int32_t W, int32_t H, const uint8_t* occupied, int32_t signal_channels, const float* grad_field_next,
                                        int64_t field_stride, float* grad_field, float* grad_emission, int64_t plane_stride, float deposit,
                                        float sigma, float decay, void* stream) {
    const char* who = "die_signal_step_backward";
    DIE_REQUIRE(occupied && grad_field_next, "%s: null argument", who);
    DIE_REQUIRE(grad_field || grad_emission, "%s: null argument (grad_field and grad_emission are both absent)", who);
    die_medium m = {};
    m.W = W; m.H = H;
    const int rc = die_signal_check(&m, signal_channels, 1, deposit, sigma, decay, who);      // (the forward's rules for K and the constants)
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)W * H, K = signal_channels;
    DIE_REQUIRE(field_stride >= cells, "%s: field_stride %lld smaller than a plane (%lld cells)", who, (long long)field_stride, (long long)cells);
    DIE_REQUIRE(!grad_emission || plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride,
                (long long)cells);
    const int64_t field_bytes = ((K - 1) * field_stride + cells) * 4, em_bytes = ((K - 1) * plane_stride + cells) * 4;
    DIE_REQUIRE(!die_ranges_overlap(grad_field, field_bytes, grad_field_next, field_bytes), "%s: grad_field overlaps grad_field_next", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_field, field_bytes, occupied, cells), "%s: grad_field overlaps the occupancy plane", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_emission, em_bytes, grad_field_next, field_bytes), "%s: grad_emission overlaps grad_field_next", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_emission, em_bytes, occupied, cells), "%s: grad_emission overlaps the occupancy plane", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_emission, em_bytes, grad_field, field_bytes), "%s: grad_emission overlaps grad_field", who);
    return die_signal_backward_launch(W, H, 1, signal_channels, occupied, 0, grad_field_next, grad_field, field_stride, grad_emission,
                                      grad_emission ? plane_stride : 0, 0, deposit, sigma, decay, stream, who);
}

extern "C" int die_signal_step_backward_batch(int32_t W, int32_t H, const die_batch* b, const uint8_t* occupied, int64_t occupied_stride,
                                              int32_t signal_channels, const float* grad_field_next, float* grad_field, float* grad_emission,
                                              int64_t plane_stride, int64_t replica_stride, float deposit, float sigma, float decay,
                                              void* stream) {
    const char* who = "die_signal_step_backward_batch";
    DIE_REQUIRE(b && occupied && grad_field_next, "%s: null argument", who);
    DIE_REQUIRE(grad_field || grad_emission, "%s: null argument (grad_field and grad_emission are both absent)", who);
    die_medium m = {};
    m.W = W; m.H = H;
    int rc = die_signal_check(&m, signal_channels, 1, deposit, sigma, decay, who);            // (the forward's rules for K and the constants)
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)W * H, K = signal_channels;
    rc = die_batch_check(b, cells, who);
    if (rc != DIE_OK) return rc;
    const int64_t R = b->replicas;
    DIE_REQUIRE(occupied_stride >= cells, "%s: occupied_stride %lld smaller than a plane (%lld cells)", who, (long long)occupied_stride,
                (long long)cells);
    if (grad_emission) {
        DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
        // replica-major ([R][K] planes: a sense gradient at plane 3) or plane-major ([K][R]: the field's layout): either way no two
        // of the K * R planes share a word
        DIE_REQUIRE(replica_stride >= cells && (replica_stride >= (K - 1) * plane_stride + cells || plane_stride >= (R - 1) * replica_stride + cells),
                    "%s: replica_stride %lld with plane_stride %lld: the %d x %d planes would share words", who, (long long)replica_stride,
                    (long long)plane_stride, b->replicas, signal_channels);
    }
    // every range over the whole K * R span
    const int64_t field_bytes = ((K * R - 1) * b->plane_stride + cells) * 4, em_bytes = ((R - 1) * replica_stride + (K - 1) * plane_stride + cells) * 4,
                  occ_bytes = (R - 1) * occupied_stride + cells;
    DIE_REQUIRE(!die_ranges_overlap(grad_field, field_bytes, grad_field_next, field_bytes), "%s: grad_field overlaps grad_field_next", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_field, field_bytes, occupied, occ_bytes), "%s: grad_field overlaps the occupancy planes", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_emission, em_bytes, grad_field_next, field_bytes), "%s: grad_emission overlaps grad_field_next", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_emission, em_bytes, occupied, occ_bytes), "%s: grad_emission overlaps the occupancy planes", who);
    DIE_REQUIRE(!die_ranges_overlap(grad_emission, em_bytes, grad_field, field_bytes), "%s: grad_emission overlaps grad_field", who);
    return die_signal_backward_launch(W, H, b->replicas, signal_channels, occupied, occupied_stride, grad_field_next, grad_field, b->plane_stride,
                                      grad_emission, grad_emission ? plane_stride : 0, grad_emission ? replica_stride : 0, deposit, sigma, decay,
                                      stream, who);
}
