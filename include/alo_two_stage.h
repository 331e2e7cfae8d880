/*
 * alo_two_stage.h — C ABI of the data-movement passes of two-stage Deformable-DETR for gfx950 (MI355X).
 *
 * Between the encoder and the decoder, the two-stage variant turns every token of the (B, S, C) encoder memory into a box
 * proposal, keeps the best K and makes them the decoder's queries (reference: alonet/deformable_detr/deformable_transformer.py
 * :130-177, :248-263).  The matrix products of that prologue run on the GEMM kernels of alo_hotpath.h; the three passes below (the first two also as one launch)
 * replace the element-wise torch chains around them (per-level meshgrid / divide / window test / log / two masked_fill pairs;
 * gather / sigmoid / divide / sin / cos / stack / flatten).
 *
 * Part of libalo_hotpath.so, under its one ABI number (alo_abi_version()), and bound to the conventions of alo_hotpath.h: device
 * pointers on the current HIP device, work enqueued on `stream` (a hipStream_t as void*), no allocation, no synchronisation,
 * ALO_OK or an alo_status_t with a message in alo_last_error(), argument errors detected before anything is enqueued.  Forward only.
 *
 * Limits: 1 <= B, 1 <= L <= 8 levels, every level non-empty, B * S < 2^31 tokens, B * K < 2^31.
 */
#ifndef ALO_TWO_STAGE_H
#define ALO_TWO_STAGE_H

#include "alo_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Box proposal of every token (gen_encoder_output_proposals, :145-171).
 *   mask_flatten       (B, S) uint8 / bool, non-zero on padding; S = sum of h_l * w_l
 *   level_shapes_host  HOST array of 2 * L ints: (h_0, w_0, h_1, w_1, ...); level l starts at token sum_{k<l} h_k * w_k
 *   proposals          (B, S, 4) float32, fully overwritten: log(p / (1 - p)) of p = ((x + 0.5) / valid_W, (y + 0.5) / valid_H,
 *                      0.05 * 2^l, 0.05 * 2^l) for a kept token, +inf in all four components otherwise
 *   keep               (B, S) uint8, fully overwritten: 1 where the token is not padding and 0.01 < p < 0.99 holds in all four
 *                      components, else 0
 * valid_W / valid_H of (image, level) are counted inside the kernel: un-padded tokens of the level's first row / first column.
 * The arithmetic is float32 with correctly rounded division, so `keep` equals the float32 torch formulation bit for bit;
 * valid_W = 0 or valid_H = 0 gives p = inf, which fails the window: every token of that level is dropped (+inf, no NaN).
 */
int alo_encoder_proposals(const unsigned char* mask_flatten, float* proposals, unsigned char* keep, int B, int L,
                          const int* level_shapes_host, void* stream);

/*
 * output_memory = keep ? memory : 0 (the two masked_fill passes of :173-175 in one).
 *   memory, out   (rows, C) in `dtype` (ALO_F32, ALO_BF16 or ALO_F16: bits are copied), 16-byte aligned, C * element size a multiple of 16 (C % 8 == 0
 *                 covers both types); `out` is fully overwritten and must not alias `memory`
 *   keep          (rows,) uint8
 * A dropped row is written as zeros without being read (NaN / inf there become 0); a kept row is copied bit for bit.
 */
int alo_mask_rows(const void* memory, const unsigned char* keep, void* out, long rows, int C, int dtype, void* stream);

/*
 * alo_encoder_proposals and alo_mask_rows in one launch: proposals, keep and out = keep ? memory : 0 for memory, out (B, S, C) in
 * `dtype`, under the conditions of both.  Same bits as the two calls; 0.026 against 0.029 ms at B = 8, S = 22 223, C = 256, bf16.
 */
int alo_encoder_proposals_masked(const unsigned char* mask_flatten, float* proposals, unsigned char* keep, const void* memory, void* out,
                                 int B, int L, const int* level_shapes_host, int C, int dtype, void* stream);

/*
 * Decoder queries from the selected proposals (:259-262 and get_proposal_pos_embed, :130-143).
 *   coords_unact      (B, S, 4) float32 (may hold +-inf)
 *   topk              (B, K) int64 token indices; an index outside [0, S) counts as a row of zeros (no trap, nothing read outside the tensor)
 *   dim_t             (64,) float32, 16-byte aligned: the frequency of each (sin, cos) pair, 10000^(k / 64) = 10000^(2 k / 128),
 *                     handed in so that kernel and torch formulation divide by the very same float32 values
 *   reference_points  (B, K, 4) float32: sigmoid of the gathered rows
 *   embed             (B, K, 512) in `dtype` (ALO_F32, ALO_BF16 or ALO_F16), 16-byte aligned: for component c and i in [0, 128),
 *                     embed[c * 128 + i] = sin(a) for even i, cos(a) for odd i, a = sigmoid(coord_c) * 2 pi / dim_t[floor(i / 2)].
 *                     Sigmoid and angle are evaluated in double and rounded once: near a zero crossing of sin / cos a float32
 *                     angle would be off by more than a bf16 / fp16 ulp of the result
 */
int alo_proposal_queries(const float* coords_unact, const long long* topk, const float* dim_t, float* reference_points, void* embed,
                         int B, int S, int K, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ALO_TWO_STAGE_H */
