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
 * enqueued.  Forward only, bf16 only (ALO_BLOCK_ATTENTION: also fp16 and fp32), d_model = 256, 8 heads of 32 channels.
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
 *
 * The decoder's two row-local chains: a flag OR-ed into `dtype` above its low byte (dtype = ALO_BF16 | ALO_BLOCK_...; bf16 only).
 * A decoder layer is self-attention, chain A, the MSDA launch, chain B; with tgt the layer's input and pos its query_pos:
 *   ALO_BLOCK_NO_FFN (chain A):  src_out = LayerNorm1(attn_out @ Wo^T + bo + src),  offsets_logits = (src_out + pos) @ Wq^T + bq
 *     attn_out the un-projected self-attention output, src = tgt, norm1_* the decoder layer's norm2, wq_packed (384, 256), bq (384,),
 *     offsets_logits (rows, 384).  Required: attn_out, wo_packed, bo, norm1_w, norm1_b, src, src_out, pos, wq_packed, bq,
 *     offsets_logits.  Must be NULL: w1_packed, b1, w2_packed, b2, norm2_w, norm2_b, padding_mask, wv_packed, bv, value_hm.
 *   ALO_BLOCK_DECODER_NEXT (chain B):  x = LayerNorm1(attn_out @ Wo^T + bo + src),  src_out = LayerNorm2(ffn(x) + x),
 *     value_hm = src_out @ Wv^T + bv written ROW-major (rows, 256),  offsets_logits = (src_out + pos) @ Wq^T + bq over 512 columns
 *     attn_out the un-projected MSDA output, src = chain A's src_out, norm1_* / norm2_* the decoder layer's norm1 / norm3, wv_packed
 *     and wq_packed (512, 256) the NEXT layer's self-attention value and [q; k] input projections, offsets_logits (rows, 512).
 *     Every pointer is required except padding_mask, which must be NULL.
 * Both equal the alo_linear_shortk / alo_add_layernorm (with pos) / alo_ffn256 launches they stand in for bit for bit.  Rows are
 * worked on in tiles of 64, or of 32 while ceil(rows / 64) is below the device's compute unit count (few rows: more compute units get
 * work) or while the 64-row LDS frame does not fit (chain B with F > 4864; the 32-row frame fits up to F = 21760); a row's bits do
 * not depend on the tile height.  ALO_BLOCK_TILE_32 / ALO_BLOCK_TILE_64 (with one of the two flags above only) fix the height
 * instead; a fixed height whose frame does not fit is ALO_ERR_UNSUPPORTED.  Refused before anything is enqueued, the message
 * naming the flag or the argument: a bit above the low byte that is none of these (ALO_ERR_UNSUPPORTED), both chains or both
 * heights at once, a height without a chain, a pointer that is NULL or non-NULL against the lists above
 * (ALO_ERR_INVALID_ARGUMENT), a flag with another dtype than ALO_BF16 (ALO_ERR_UNSUPPORTED).  Without a flag the call is the
 * encoder's, as above.
 *
 * Dense multi-head attention with a key padding mask: the step between chain B's projections and chain A (or an out_proj), on the
 * same entry point because it consumes the one's outputs and produces the other's input.  bf16, fp16 or fp32.
 *   ALO_BLOCK_ATTENTION:  src_out = softmax(q k^T * eps1 + mask) v per head, 8 heads of 32 channels (head h: columns 32 h .. 32 h + 31)
 *     src      q (batch, S, .), S queries;   pos  k (batch, F, .), F keys (any positive S, F: self- and cross-attention).  Row pitch
 *              of q and k: 256 elements
 *     attn_out v (batch, F, 256);   padding_mask (batch, F) uint8 or NULL, non-zero = the key is ignored (key_padding_mask)
 *     src_out  out (batch, S, 256), fully overwritten: the un-projected attention output chain A and an out_proj take
 *     eps1     the softmax scale, > 0 (1 / sqrt(32) for the usual attention), applied to the product (in fp32; in fp64 for fp32
 *              operands), never to the 16-bit operands; eps2 must be 0
 *     Every other pointer must be NULL.
 *   ALO_BLOCK_PACKED_QK (with ALO_BLOCK_ATTENTION only): q and k are the two halves of chain B's (rows, 512) [q; k] matrix: row
 *     pitch 512 elements, pos == src + 256 elements, F == S.
 *   A key past F does not exist: its memory is not read.  A query all of whose keys are masked gets NaN in its 256 outputs (what
 *   nn.MultiheadAttention returns); other queries and images are unaffected.  The 16-bit flavours accumulate in fp32 and round the
 *   probabilities to the storage type before the second product; fp32 operands are widened to fp64 and both products, the
 *   exponentials and the sums run in fp64, so the fp32 result carries one rounding.
 *   Refused before anything is enqueued, the message naming the flag or the argument: ALO_BLOCK_PACKED_QK without
 *   ALO_BLOCK_ATTENTION, with F != S or with another pos; ALO_BLOCK_ATTENTION with a chain or tile flag; a wanted pointer that is
 *   NULL or another that is not; eps1 <= 0, eps2 != 0; non-positive sizes; pointers off a 16-byte boundary; src_out overlapping an
 *   input (ALO_ERR_INVALID_ARGUMENT); any other bit above the low byte, a dtype outside the three, a q, k, v or out of 2 GiB or
 *   more (ALO_ERR_UNSUPPORTED).
 */
#define ALO_BLOCK_NO_FFN 0x100
#define ALO_BLOCK_DECODER_NEXT 0x200
#define ALO_BLOCK_TILE_32 0x400
#define ALO_BLOCK_TILE_64 0x800
#define ALO_BLOCK_ATTENTION 0x2000
#define ALO_BLOCK_PACKED_QK 0x8000

int alo_encoder_block(const void* attn_out, const void* wo_packed, const void* bo, const void* norm1_w, const void* norm1_b,
                      const void* src, const void* w1_packed, const void* b1, const void* w2_packed, const void* b2,
                      const void* norm2_w, const void* norm2_b, void* src_out, const void* pos, const void* padding_mask,
                      const void* wv_packed, const void* bv, const void* wq_packed, const void* bq, void* value_hm,
                      void* offsets_logits, int batch, int S, int F, float eps1, float eps2, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
