// What the NeuralAutomataAgent files share.  Device side (die_nca.hip / die_nca_wide.hip: the forward; die_nca_grad.hip /
// die_nca_wide_grad.hip: its adjoint): the workgroup tile, the limits, how a cell beyond the field is read and how a first-layer plane
// is loaded.  Host side, each rule stated once: layer 0's input list (die_nca_layer0_planes), the field's planes (die_nca_field_check)
// and the paddings without an adjoint (die_nca_pad_adjoint_check) in die_nca.hip; what a valid stack is, narrow or wide
// (die_nca_stack_check), in die_nca_wide.hip; the sizes both directions derive from a stack (tiles, ping-pong sets, widest layer) here.
#pragma once
#include "die_common.h"

#define NCA_TX 16
#define NCA_TY 64
#define NCA_MAXC 4
#define NCA_MAXK 7

// the wide layer kernels (die_nca_wide.hip: the forward; die_nca_wide_grad.hip: its adjoint)
#define NCAW_MAXC 32             // channels in or out of one layer
#define NCAW_CH 4                // input channels per staged chunk: one MFMA K-step per tap
typedef float ncaw_f32x4 __attribute__((ext_vector_type(4)));

// index of the cell that stands in for coordinate v of an axis of n cells, or −1 for "reads as zero" (torch.nn.functional.pad:
// 'circular' wraps, 'zeros' pads with 0, 'reflect' mirrors WITHOUT repeating the edge cell, 'replicate' repeats it)
__device__ __forceinline__ int nca_pad_index(int v, int n, int mode) {
    if (v >= 0 && v < n) return v;
    if (mode == DIE_PAD_CIRCULAR) { v %= n; return v < 0 ? v + n : v; }
    if (mode == DIE_PAD_ZEROS) return -1;
    if (mode == DIE_PAD_REPLICATE) return v < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const int period = 2 * (n - 1);                  // 'reflect': … 2 1 | 0 1 2 … n−1 | n−2 n−3 …
    v %= period; v = v < 0 ? v + period : v;
    return v < n ? v : period - v;
}

__device__ __forceinline__ float nca_load(const void* p, int kind, int64_t i, int epoch) {
    if (kind == DIE_PLANE_F32) return ((const float*)p)[i];
    if (kind == DIE_PLANE_F16) return __half2float(((const __half*)p)[i]);
    const unsigned long long word = ((const unsigned long long*)p)[i];
    // DIE_PLANE_STOCK (die_stock.hip): the claim plane's word with the standing agent's stock as its payload
    if (kind == DIE_PLANE_STOCK) return die_claim_occupied(word, epoch) ? die_claim_deposit(word) : 0.f;
    return die_claim_occupied(word, epoch) ? 1.f : 0.f;
}

// die_nca_dropout, checked, as the words the kernels read (die_nca.hip)
int die_dropout_words(const die_nca_dropout* drop, DropWords* out, const char* who);

// ---- the host-side rules of a stack ----
// the forward's 16 x 64 tiles over a W x H field: a layer's partial rows, one per tile
static inline int64_t die_nca_tiles(int32_t W, int32_t H) { return (int64_t)((W + NCA_TX - 1) / NCA_TX) * ((H + NCA_TY - 1) / NCA_TY); }
// the step's scratch holds set = layer % 2 of the layers' outputs; the adjoint's workspace as many sets of the gradient going down
static inline int die_nca_pingpong_sets(int32_t n_layers) { return n_layers >= 2 ? 2 : 1; }
static inline int die_nca_gin_sets(int32_t n_layers) { return n_layers - 1 < 2 ? n_layers - 1 : 2; }
// the widest cout of a stack: the planes a replica has in a wide stack's scratch, store and workspace
static inline int die_nca_max_channels(const die_nca_batch* nca) {
    int mc = 1;
    for (int l = 0; l < nca->n_layers; ++l) mc = nca->layers[l].cout > mc ? nca->layers[l].cout : mc;
    return mc;
}
// Layer 0's input planes, in THE order: the agents plane if with_agent_channel, food, chem, then the `memory` planes of
// die_memory.hip (mem_planes null: none; plane j of replica 0 at mem_planes + j * replicas * plane_stride), then the stock plane of
// die_stock.hip (null: none).  Fills in[] / kind[] (a kernel argument's arrays) and returns the count; *rep_in: replica r's planes lie
// r * b->plane_stride elements on, every one of them.  The forward and the adjoint of both kinds read their list here.
// `signal_planes` with `signals` (die_signal.hip; null / 0: none): the signal field's planes, laid out as the memory planes are, read
// as plain fp32 planes AFTER chem and BEFORE the memory planes: [agents], food, chem, signal_0 .., memory_0 .., [stock].
int die_nca_layer0_planes(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* mem_planes, int memory,
                          const unsigned long long* stock, const void* in[], int kind[], int64_t* rep_in,
                          const float* signal_planes = nullptr, int signals = 0);
// every argument of a stack, before anything is launched, in the order its kind has always checked them (narrow: the scratch's size
// before the layers; wide: after them).  `scratch`: the step's ping-pong planes are required (the calls that keep every layer in
// caller-owned storage check their own); `stock`: layer 0 reads the stock plane as its last input; `memory`: layer 0 reads that many
// planes more and the last layer gives 3 + memory (die_nca_wide.hip, beside the wider kind's limits); `signals`: layer 0 reads that
// many planes more as well and the last layer gives 3 + signals + memory, the emissions ahead of the memory
enum die_nca_kind { DIE_NCA_NARROW = 0, DIE_NCA_WIDE = 1 };     // die_nca.hip's kernels / die_nca_wide.hip's
int die_nca_stack_check(die_nca_kind kind, const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who, bool scratch,
                        bool stock = false, int memory = 0, int signals = 0);
// the die_batch of the batched read-out, sensing and adjoint
int die_nca_batch_shape_check(const die_medium* m, const die_batch* b, const char* who);
// the field a stack senses: its dtype, its planes, sense_epoch
int die_nca_field_check(const die_medium* m, const die_nca_batch* nca, const char* who);
// 'reflect' and 'replicate' padding have no adjoint kernel: DIE_ERR_UNSUPPORTED
int die_nca_pad_adjoint_check(int32_t padding_mode, const char* who);
// what the *_sense_batch_store calls check alike, in their order: the arguments, the die_batch, the stack, the field
int die_nca_store_check(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store, die_nca_kind kind, const char* who,
                        int memory = 0, int signals = 0);

// ---- what the batched step (die_env.hip: nca_env_step_batch) calls after die_nca_stack_check, in its order ----
// every replica's stock plane at `epoch` (die_stock.hip)
int die_stock_launch(const die_medium* m, const die_agents* a, int32_t replicas, const int64_t* n, int64_t agent_stride,
                     int64_t plane_stride, int32_t epoch, unsigned long long* planes, void* stream, const char* who);
// the memory of whoever stands on a cell as planes, and the planes read back into the memory (die_memory.hip)
int die_memory_planes_launch(int32_t W, int32_t H, int32_t replicas, const int64_t* n, const unsigned long long* standing,
                             int64_t standing_rep, int32_t epoch, int32_t M, const float* mem, int64_t mem_row, int64_t mem_rep,
                             float* planes, int64_t plane_j, int64_t plane_rep, void* stream, const char* who);
int die_gather_memory_launch(const die_medium* m, const die_agents* a, int32_t replicas, const int64_t* n, int64_t agent_stride, int32_t M,
                             const float* planes, int64_t plane_j, int64_t plane_rep, float* mem, int64_t mem_row, int64_t mem_rep,
                             void* stream, const char* who);
// the stack into the step's scratch: *sense = the last layer's planes of replica 0, replica r's *rep further (die_nca.hip) …
int die_nca_sense_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float** sense, int64_t* rep,
                        const DropWords* drop, void* stream, const unsigned long long* stock);
// … and a wide one (die_nca_wide.hip; `stock`, `mem_planes` with `memory`: null / 0 without them)
int die_nca_wide_sense_batch(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float** sense, int64_t* rep,
                             const DropWords* drop, void* stream, const unsigned long long* stock, const float* mem_planes, int memory,
                             const float* signal_planes = nullptr, int signals = 0);
// the signal field's update (die_signal.hip): the checks its entry points and the batched step share, then the one launch for the K
// planes of every replica — field plane k of replica r at (k * replicas + r) * field_stride, in and out alike
int die_signal_check(const die_medium* m, int32_t K, int32_t epoch, float deposit, float sigma, float decay, const char* who);
int die_signal_overlap_check(const float* field_in, const float* field_out, int64_t field_bytes, const float* emission, int64_t em_bytes,
                             const unsigned long long* standing, int64_t standing_bytes, const char* who);
int die_signal_launch(int32_t W, int32_t H, int32_t replicas, int32_t K, const unsigned long long* standing, int64_t standing_rep, int32_t epoch,
                      const float* emission, int64_t em_plane, int64_t em_rep, const float* field_in, float* field_out, int64_t field_stride,
                      float deposit, float sigma, float decay, void* stream, const char* who);
// … and its adjoint's (die_signal_grad.hip): the same sweep on the gradient planes, laid out as the field's; replica r's occupancy bytes
// occ_rep on, its emission gradient's plane k at grad_emission + k * em_plane + r * em_rep; grad_field or grad_emission may be null
int die_signal_backward_launch(int32_t W, int32_t H, int32_t replicas, int32_t K, const uint8_t* occupied, int64_t occ_rep, const float* grad_next,
                               float* grad_field, int64_t field_stride, float* grad_emission, int64_t em_plane, int64_t em_rep, float deposit,
                               float sigma, float decay, void* stream, const char* who);

// k_conv_backward_sum on `tiles` partial rows of nw weights (die_nca_grad.hip), for the wide adjoint's rows as well
void die_conv_backward_fold(const float* part, int64_t tiles, int nw, float* out, hipStream_t s);
// k_conv_backward_sum_batch: candidate c's `rows` consecutive partial rows (its E replicas' tiles, [candidate][rows][nw]) in ascending
// order, float64, into out + c * out_stride — for the wide stack's batched adjoint
void die_conv_backward_fold_batch(const float* part, int64_t rows, int nw, int candidates, float* out, int64_t out_stride, hipStream_t s);
