// The signal channels of a NeuralAutomataAgent (gfx950): NeuralAutomataAgent(signal_channels=K), 1 <= K <= 8 — a field of K fp32
// planes the agents write and read (the reference's notes: "abstracted actionable channels: let the medium have
// channels rgbc, and enable the Agent to sense 'rgb' and to act on 'g' and 'c'").  Where memory travels with an agent, a signal stays
// where it was written, diffuses, decays and is read by whoever comes by.  One update per forward:
//
//     E_k[c] = occupied(c) ? deposit * S_k[c] : +0.0f                      (one fp32 multiply; S_k: the last layer's plane 3 + k)
//     F_k   <- (1 - decay) * gaussian(F_k + E_k, sigma, wrap, truncate 4)   (one fp32 add, then die_diffuse_decay's arithmetic)
//
// `occupied` is the standing plane's word (die_stock.hip: alive slots only, tagged `epoch`; its payload is ignored), so agents
// sharing a cell emit once.  The result goes into a second buffer: EVERY cell of every output plane is written, nobody clears.
//
//   k_signal_rows<R>  the row-marching sweep of die_diffuse_rows.inc (the one die_diffuse_decay runs where H % 4 == 0 and R <= 4) with
//                     a loader that adds the emission to the 4 cells a lane has just read: 32 bytes of standing words and 16 of
//                     emission beside the 16 of field, all 16-byte accesses.  Taken where everything is 16-byte aligned.
//   k_signal_tile<R>  the LDS-tiled sweep of die_diffuse_tile.inc (R <= 8, any H, any alignment) with the same rule cell by cell.
// There is no second gaussian here: both sweeps are the text die_env.hip's k_diffuse_rows / k_diffuse include (die_diffuse.h says why
// text), so the field's update is die_diffuse_decay's arithmetic, tap for tap, with one fp32 add in front.
//
// Plane z = blockIdx.z of the launch is channel k = z / replicas of replica r = z % replicas: the field's planes lie (k * replicas +
// r) * field_stride apart — the layout in which a batched layer launch reads plane k of every replica one stride apart — so all K
// planes of all R replicas are ONE launch, and the stand-alone call is the batched one with one replica.
//
// Roofline: 4 * (2 reads + 1 write) bytes per cell and channel, plus 8 bytes of standing word per cell and channel (L2 hits from
// the second channel on).  At 10 x 96^2 worlds and K = 2 that is 184 320 cells * 20 bytes = 3.7 MB: far below what the memory system
// notices, the launch is the cost, as for die_memory.hip's kernels (measured, LABBOOK 41: 6.3 us a launch, between the 5 us of the
// claim launch and the 6.9 us of the chem sweep).  At large worlds the kernel is bandwidth-bound like the sweep it instantiates
// (1 x 2048^2, K = 2: 26.6 us against 20.8 us for die_diffuse_decay on the same two planes, both cache-resident).
#include <math.h>
#include "die_forward.h"
#include "die_nca.h"
#include "die_diffuse.h"

struct SignalArgs {
    const unsigned long long* standing;      // replica r's plane standing_rep words on
    const float* emission;                   // S_k of replica r at emission + k * em_plane + r * em_rep
    int64_t standing_rep, em_plane, em_rep, field_stride;
    int replicas, epoch;
    float deposit;
};

// the one statement of E: a multiply of its own (build.py's -ffp-contract=on fuses inside one expression only), then the add
__device__ __forceinline__ float signal_add(float f, unsigned long long word, float s, int epoch, float deposit) {
    const float e = die_claim_occupied(word, epoch) ? deposit * s : 0.f;
    return f + e;
}

// the standing words and the emission of the plane this workgroup updates: channel k = z / replicas of replica r = z % replicas
struct SignalEmit {
    const unsigned long long* standing;
    const float* emission;
    int epoch;
    float deposit;
    __device__ __forceinline__ SignalEmit(const SignalArgs& s) {
        const int k = (int)blockIdx.z / s.replicas, r = (int)blockIdx.z - k * s.replicas;
        standing = s.standing + s.standing_rep * r;
        emission = s.emission + s.em_plane * k + s.em_rep * r;
        epoch = s.epoch; deposit = s.deposit;
    }
    // 4 cells at plane offset `off` (a multiple of 4; 16-byte aligned planes): 32 bytes of words, 16 of emission
    __device__ __forceinline__ void add4(int64_t off, float* v) const {
        const ulonglong2 c01 = *(const ulonglong2*)(standing + off), c23 = *(const ulonglong2*)(standing + off + 2);
        const float4 s = *(const float4*)(emission + off);
        v[0] = signal_add(v[0], c01.x, s.x, epoch, deposit);
        v[1] = signal_add(v[1], c01.y, s.y, epoch, deposit);
        v[2] = signal_add(v[2], c23.x, s.z, epoch, deposit);
        v[3] = signal_add(v[3], c23.y, s.w, epoch, deposit);
    }
    __device__ __forceinline__ float add(float f, int64_t i) const { return signal_add(f, standing[i], emission[i], epoch, deposit); }
};

template <int R>
__global__ __launch_bounds__(DIF_BLOCK) void k_signal_rows(RowsArgs a, SignalArgs s) {
    static_assert(R >= 1 && R <= 4, "one halo lane of 4 columns per side");
    using T = float;
    constexpr int FUSED = 0, row0 = 0;
    constexpr bool WRAP = true;
    const SignalEmit emit(s);
    const int64_t plane = a.rep_cells * blockIdx.z;
    a.src = (const float*)a.src + plane;
    a.dst = (float*)a.dst + plane;
#define DIF_EMIT(off, v) emit.add4(off, v);
#include "die_diffuse_rows.inc"
#undef DIF_EMIT
}

template <int R>
__global__ __launch_bounds__(DIE_BLOCK) void k_signal_tile(DiffuseArgs a, SignalArgs s) {
    using T = float;
    const SignalEmit emit(s);
    const int64_t plane = s.field_stride * blockIdx.z;
    a.src = (const float*)a.src + plane;
    a.dst = (float*)a.dst + plane;
#define DIF_LOAD(src, i) emit.add(die_ld(src, i), i)
#include "die_diffuse_tile.inc"
#undef DIF_LOAD
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- the launch alone: every argument has been checked by the caller (the entry points below, die_env.hip's batched step) ----
// field plane k of replica r at field + (k * replicas + r) * field_stride (in and out alike), emission plane k of replica r at
// emission + k * em_plane + r * em_rep, replica r's standing plane standing_rep words on
int die_signal_launch(int32_t W, int32_t H, int32_t replicas, int32_t K, const unsigned long long* standing, int64_t standing_rep, int32_t epoch,
                      const float* emission, int64_t em_plane, int64_t em_rep, const float* field_in, float* field_out, int64_t field_stride,
                      float deposit, float sigma, float decay, void* stream, const char* who) {
    double wd[2 * DIF_MAXR + 1];
    const int R = die_gaussian_taps(sigma, wd);
    const float keep = (float)(1.0 - (double)decay);
    const int planes = K * replicas;
    hipStream_t s = (hipStream_t)stream;
    SignalArgs sa;
    sa.standing = standing; sa.emission = emission; sa.standing_rep = standing_rep; sa.em_plane = em_plane; sa.em_rep = em_rep;
    sa.field_stride = field_stride; sa.replicas = replicas; sa.epoch = epoch; sa.deposit = deposit;
    // 16-byte accesses: whole groups of 4 cells, every plane of every replica on a 16-byte boundary
    const bool vec = rows_kernel_applies(W, H, R) && aligned16(field_in) && aligned16(field_out) && aligned16(emission) && aligned16(standing) &&
                     (field_stride & 3) == 0 && (em_plane & 3) == 0 && (em_rep & 3) == 0 && (standing_rep & 1) == 0;
    if (vec) {
        RowsArgs ra;
        ra.src = field_in; ra.dst = field_out; ra.claim = nullptr; ra.dep = nullptr; ra.food = nullptr; ra.W = W; ra.H = H; ra.epoch = 0; ra.halo = 0;
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
            case 1: k_signal_rows<1><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
            case 2: k_signal_rows<2><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
            case 3: k_signal_rows<3><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
            default: k_signal_rows<4><<<grid, DIF_BLOCK, 0, s>>>(ra, sa); break;
        }
    } else {
        DiffuseArgs a;
        a.src = field_in; a.dst = field_out; a.W = W; a.H = H; a.mode = DIE_DIFFUSE_WRAP; a.keep = keep;
        for (int k = 0; k <= 2 * DIF_MAXR; ++k) a.w[k] = k <= 2 * R ? (float)wd[k] : 0.f;
        DIE_REQUIRE((W + DIF_TX - 1) / DIF_TX <= 65535, "%s: field too tall (%d rows)", who, W);
        const dim3 grid((H + DIF_TY - 1) / DIF_TY, (W + DIF_TX - 1) / DIF_TX, planes);
        switch (R) {
            case 1: k_signal_tile<1><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 2: k_signal_tile<2><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 3: k_signal_tile<3><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 4: k_signal_tile<4><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 5: k_signal_tile<5><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 6: k_signal_tile<6><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            case 7: k_signal_tile<7><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
            default: k_signal_tile<8><<<grid, DIE_BLOCK, 0, s>>>(a, sa); break;
        }
    }
    DIE_CHECK_LAUNCH(who);
    return DIE_OK;
}

// ---- the checks both entry points and the batched step make alike, before anything is launched -------------------------
// (m, K, epoch, the three constants: sigma's radius must lie in 1..DIF_MAXR, decay in [0, 1], deposit finite)
int die_signal_check(const die_medium* m, int32_t K, int32_t epoch, float deposit, float sigma, float decay, const char* who) {
    DIE_REQUIRE(m->W >= 1 && m->H >= 1, "%s: bad size %dx%d", who, m->W, m->H);
    if (m->gW > 0) {
        die_set_error("%s: a decomposed medium has no signal field (periodic single-tile planes only)", who);
        return DIE_ERR_UNSUPPORTED;
    }
    DIE_REQUIRE(K >= 1 && K <= DIE_SIGNAL_MAX_CHANNELS, "%s: %d signal channels outside 1..%d", who, K, DIE_SIGNAL_MAX_CHANNELS);
    DIE_REQUIRE(epoch >= 1 && epoch <= DIE_OWNER_EPOCH_MAX, "%s: epoch %d outside 1..%d", who, epoch, DIE_OWNER_EPOCH_MAX);
    DIE_REQUIRE(sigma > 0.f && sigma < 1e6f, "%s: sigma %g must be positive and finite", who, (double)sigma);
    const int R = die_gaussian_radius(sigma);
    DIE_REQUIRE(R >= 1 && R <= DIF_MAXR, "%s: sigma %g gives radius %d outside 1..%d", who, (double)sigma, R, DIF_MAXR);
    DIE_REQUIRE(decay >= 0.f && decay <= 1.f, "%s: decay %g outside [0, 1]", who, (double)decay);
    DIE_REQUIRE(isfinite(deposit), "%s: deposit %g is not finite", who, (double)deposit);
    return DIE_OK;
}

// field_out against everything the launch reads: the field's own input planes, the emission planes, the standing planes
int die_signal_overlap_check(const float* field_in, const float* field_out, int64_t field_bytes, const float* emission, int64_t em_bytes,
                             const unsigned long long* standing, int64_t standing_bytes, const char* who) {
    DIE_REQUIRE(!die_ranges_overlap(field_out, field_bytes, field_in, field_bytes), "%s: field_out overlaps field_in", who);
    DIE_REQUIRE(!die_ranges_overlap(field_out, field_bytes, emission, em_bytes), "%s: field_out overlaps the emission planes", who);
    DIE_REQUIRE(!die_ranges_overlap(field_out, field_bytes, standing, standing_bytes), "%s: field_out overlaps the standing plane", who);
    return DIE_OK;
}

extern "C" int die_signal_step(const die_medium* m, const unsigned long long* standing, int32_t epoch, int32_t signal_channels,
                               const float* emission_planes, int64_t plane_stride, const float* field_in, float* field_out,
                               int64_t field_stride, float deposit, float sigma, float decay, void* stream) {
    const char* who = "die_signal_step";
    DIE_REQUIRE(m && standing && emission_planes && field_in && field_out, "%s: null argument", who);
    int rc = die_signal_check(m, signal_channels, epoch, deposit, sigma, decay, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H, K = signal_channels;
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    DIE_REQUIRE(field_stride >= cells, "%s: field_stride %lld smaller than a plane (%lld cells)", who, (long long)field_stride, (long long)cells);
    rc = die_signal_overlap_check(field_in, field_out, ((K - 1) * field_stride + cells) * 4, emission_planes, ((K - 1) * plane_stride + cells) * 4,
                                  standing, cells * 8, who);
    if (rc != DIE_OK) return rc;
    return die_signal_launch(m->W, m->H, 1, signal_channels, standing, 0, epoch, emission_planes, plane_stride, 0, field_in, field_out,
                             field_stride, deposit, sigma, decay, stream, who);
}

extern "C" int die_signal_step_batch(const die_medium* m, const die_batch* b, const unsigned long long* standing, int32_t epoch,
                                     int32_t signal_channels, const float* emission_planes, int64_t plane_stride, int64_t replica_stride,
                                     const float* field_in, float* field_out, float deposit, float sigma, float decay, void* stream) {
    const char* who = "die_signal_step_batch";
    DIE_REQUIRE(m && b && standing && emission_planes && field_in && field_out, "%s: null argument", who);
    int rc = die_signal_check(m, signal_channels, epoch, deposit, sigma, decay, who);
    if (rc != DIE_OK) return rc;
    const int64_t cells = (int64_t)m->W * m->H, K = signal_channels;
    rc = die_batch_check(b, cells, who);
    if (rc != DIE_OK) return rc;
    const int64_t R = b->replicas;
    DIE_REQUIRE(plane_stride >= cells, "%s: plane_stride %lld smaller than a plane (%lld cells)", who, (long long)plane_stride, (long long)cells);
    DIE_REQUIRE(replica_stride >= (K - 1) * plane_stride + cells, "%s: replica_stride %lld smaller than a replica's %lld planes", who,
                (long long)replica_stride, (long long)K);
    rc = die_signal_overlap_check(field_in, field_out, ((K * R - 1) * b->plane_stride + cells) * 4, emission_planes,
                                  ((R - 1) * replica_stride + (K - 1) * plane_stride + cells) * 4, standing,
                                  ((R - 1) * b->plane_stride + cells) * 8, who);
    if (rc != DIE_OK) return rc;
    return die_signal_launch(m->W, m->H, b->replicas, signal_channels, standing, b->plane_stride, epoch, emission_planes, plane_stride,
                             replica_stride, field_in, field_out, b->plane_stride, deposit, sigma, decay, stream, who);
}
