/*
 * alo_encoder_block.h — C ABI of the fused row-local part of a Deformable-DETR encoder layer for gfx950 (MI355X).
 *
 * Between two multi-scale deformable attention launches everything an encoder layer does is local to a row of the (batch * S, 256)
 * token matrix (reference: alonet/deformable_detr/deformable_transformer.py:310-344, ops/modules/ms_deform_attn.py:111-137):
 *
 *     [ src   = LayerNorm1(attn_out @ Wo^T + bo + src) ]                      attention tail, optional
 *       src'  = LayerNorm2(relu(src @ W1^T + b1) @ W2^T + b2 + src)           feed-forward block
 *     [ value = masked_fill(src' @ Wv^T + bv, padding_mask, 0), head-major    the NEXT layer's three projections, optional
 *       offsets_logits = (src' + pos) @ Wq^T + bq ]
 *
 * alo_encoder_block runs that chain in one kernel over 64-row tiles held in LDS; every intermediate of the chain stays on the chip.
 * The rounding points (bf16 after each product and each LayerNorm, `src' + pos` taken on the rounded src') and the summation orders
 * are those of alo_linear_shortk, alo_add_layernorm, alo_ffn256 and alo_value_proj_head_major of alo_hotpath.h, so the results equal
 * the chain of those launches bit for bit.
 *
 * Part of libalo_hotpath.so, under its one ABI number (alo_abi_version()), and bound to the conventions of alo_hotpath.h: device
 * pointers on the current HIP device, 16-byte aligned, work enqueued on `stream` (a hipStream_t as void*), no allocation, no
 * synchronisation, ALO_OK or an alo_status_t with a message in alo_last_error(), argument errors detected before anything is
 * enqueued.  Forward only, bf16 only, d_model = 256, 8 heads of 32 channels.
 */
#ifndef ALO_ENCODER_BLOCK_H
#define ALO_ENCODER_BLOCK_H

#include "alo_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * All matrices are bf16; every *_packed weight is alo_pack_mfma_b of the row-major (N, K) weight; biases and LayerNorm parameters
 * are bf16 vectors.  Rows = batch * S.
 *   attention tail (all of attn_out, wo_packed, bo, norm1_w, norm1_b, or none of them):
 *     attn_out (rows, 256)   un-projected attention output;  wo_packed (256, 256), bo (256,);  norm1_w / norm1_b (256,), eps1
 *   feed-forward block (always):
 *     src (rows, 256)        the layer's input (the tail's residual; without a tail the FFN's input)
 *     w1_packed (F, 256), b1 (F,), w2_packed (256, F), b2 (256,), F % 256 == 0;  norm2_w / norm2_b (256,), eps2
 *     src_out (rows, 256)    fully overwritten; may not alias src
 *   next layer's projections (all of pos, wv_packed, bv, wq_packed, bq, value_hm, offsets_logits, or none of them):
 *     pos (rows, 256);  padding_mask (rows,) uint8, non-zero on padding, or NULL
 *     wv_packed (256, 256), bv (256,)  -> value_hm (batch, 8, S, 32), rows under the mask zeroed
 *     wq_packed (384, 256), bq (384,)  -> offsets_logits (rows, 384): [sampling_offsets; attention_weights] of (src' + pos)
 */
int alo_encoder_block(const void* attn_out, const void* wo_packed, const void* bo, const void* norm1_w, const void* norm1_b,
                      const void* src, const void* w1_packed, const void* b1, const void* w2_packed, const void* b2,
                      const void* norm2_w, const void* norm2_b, void* src_out, const void* pos, const void* padding_mask,
                      const void* wv_packed, const void* bv, const void* wq_packed, const void* bq, void* value_hm,
                      void* offsets_logits, int batch, int S, int F, float eps1, float eps2, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
