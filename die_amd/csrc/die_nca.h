// What the NeuralAutomataAgent kernels share (die_nca.hip: the forward; die_nca_grad.hip: its adjoint): the workgroup tile, the
// limits, how a cell beyond the field is read and how a first-layer plane is loaded.
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

// a die_nca_batch without the step's scratch (the calls that keep every layer in caller-owned storage), and the die_batch
// of the batched read-out, sensing and adjoint: checked before anything is launched (die_nca.hip)
int die_nca_stack_check(const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who);
int die_nca_batch_shape_check(const die_medium* m, const die_batch* b, const char* who);
// the same for a wide stack (die_nca_wide.hip: 1..32 channels, k in 1, 3, 5, an activation per layer in die_nca_layer.reserved)
int die_nca_wide_stack_check(const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who);
// … whose layer 0 reads `memory` fp32 planes more and whose last layer gives 3 + memory (the *_memory store / backward pair)
int die_nca_wide_stack_check_memory(const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who, int memory);
// what die_nca_sense_batch_store and die_nca_wide_sense_batch_store check alike, in their order: the arguments, the die_batch, the
// stack (`wide`: die_nca_wide_stack_check), the field's dtype and planes, sense_epoch (die_nca.hip)
int die_nca_store_check(const die_medium* m, const die_batch* b, const die_nca_batch* nca, const float* store, bool wide, const char* who);

// ---- what the batched step (die_env.hip: nca_env_step_batch) calls, in its order ----
// the stack WITH the step's scratch (die_nca.hip; `stock`: layer 0 reads the stock plane as its last input) …
int die_nca_batch_check(const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who, bool stock);
// … and a wide one (die_nca_wide.hip; `memory`: layer 0 reads that many planes more, the last layer gives 3 + memory)
int die_nca_wide_batch_check(const die_nca_batch* nca, int32_t W, int32_t H, int32_t replicas, const char* who, bool stock, int memory);
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
                             const DropWords* drop, void* stream, const unsigned long long* stock, const float* mem_planes, int memory);

// k_conv_backward_sum on `tiles` partial rows of nw weights (die_nca_grad.hip), for the wide adjoint's rows as well
void die_conv_backward_fold(const float* part, int64_t tiles, int nw, float* out, hipStream_t s);
// k_conv_backward_sum_batch: candidate c's `rows` consecutive partial rows (its E replicas' tiles, [candidate][rows][nw]) in ascending
// order, float64, into out + c * out_stride — for the wide stack's batched adjoint
void die_conv_backward_fold_batch(const float* part, int64_t rows, int nw, int candidates, float* out, int64_t out_stride, hipStream_t s);
