/*
 * alo_corr_alt.h — C ABI of RAFT's memory-light correlation block ("AlternateCorrBlock") for gfx950 (MI355X).
 *
 * Replaces AlternateCorrBlock.__init__ / __call__ of the reference (alonet/raft/corr.py:63-91), whose lookup calls the
 * third-party alt_cuda_corr extension.  Instead of the O((HW)^2) all-pairs volume of alo_corr_build, only the feature maps are
 * kept; every lookup computes the (2r+2)^2 inner products under each query's window on the fly and interpolates them.
 * The result equals alo_corr_lookup on alo_corr_build's pyramid up to fp32 rounding (2x2 means commute with the inner product).
 *
 * Part of libalo_hotpath.so, under its one ABI number (alo_abi_version()), and bound to the conventions of alo_hotpath.h: device
 * pointers on the current HIP device, work enqueued on `stream` (a hipStream_t as void*), no allocation and no synchronisation,
 * ALO_OK or an alo_status_t with a message in alo_last_error(), argument errors detected before anything is enqueued.
 *
 * Limits (index arithmetic of the kernels): 1 <= B <= 65535, 1 <= C <= 65536, H * W <= 2^26, 1 <= num_levels <= 8,
 * 0 <= radius <= 7, and no pyramid level may be empty (alo_corr_level_shape: floor-halving per level).  Levels one pixel wide
 * or high are accepted.  Sizes past a limit give ALO_ERR_UNSUPPORTED.
 */
#ifndef ALO_CORR_ALT_H
#define ALO_CORR_ALT_H

#include <stddef.h>

#include "alo_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Flag, OR-ed into `num_levels` of alo_corr_alt_workspace_bytes and alo_corr_alt_lookup (the level count is the low byte): the
 * workspace carries a gradient region, and the lookup is the ADJOINT of a lookup with respect to both feature maps (below).  Any
 * other bit above the low byte is refused (ALO_ERR_UNSUPPORTED by the lookup, 0 bytes by the size query). */
#define ALO_CORR_ALT_GRAD 0x100

/* Bytes of the caller-owned workspace that alo_corr_alt_prepare fills and alo_corr_alt_lookup reads: fmap1 and every level of
 * fmap2 in channels-last layout, channels zero-padded to a multiple of 16 (Cp), every part rounded up to 256 bytes.  0 when the
 * sizes are outside the limits above.
 *
 * With num_levels | ALO_CORR_ALT_GRAD: those prepared parts PLUS the gradient region behind them, in this order, every part
 * rounded up to 256 bytes, all float32:
 *   num_levels planes of grad_fmap1, plane l = the contribution of level l: (B, H*W, Cp) channels-last, as the prepared fmap1;
 *                grad_fmap1 is the sum of the planes
 *   then for l = 0 .. num_levels-1 the gradient of fmap2's level l, SLICE-MAJOR: (Cp/16, B, h_l*w_l, 16); element
 *                [s][b][p][c] belongs to channel 16 s + c of pixel p (the bytes of the prepared level l, in another order)
 * Channels C..Cp-1 of the region stay as the caller left them plus zero. */
size_t alo_corr_alt_workspace_bytes(int B, int C, int H, int W, int num_levels);

/*
 * Relayout once per block (AlternateCorrBlock.__init__, corr.py:63-71).
 *   fmap1          (B, C, H, W) float32
 *   fmap2_levels   HOST array of num_levels DEVICE pointers: level l = fmap2 2x2-average-pooled l times (floor),
 *                  (B, C, h_l, w_l) float32 with (h_l, w_l) = alo_corr_level_shape(H, W, l)
 *   workspace      device memory of alo_corr_alt_workspace_bytes(...) bytes, 16-byte aligned; overwritten
 */
int alo_corr_alt_prepare(const float* fmap1, const float* const* fmap2_levels, void* workspace, size_t workspace_bytes,
                         int B, int C, int H, int W, int num_levels, void* stream);

/*
 * Windowed correlation lookup (AlternateCorrBlock.__call__, corr.py:73-91).
 *   workspace  as filled by alo_corr_alt_prepare with the same B, C, H, W, num_levels (read only)
 *   coords     (B, 2, H, W) float32 pixel coordinates (x, y) on level 0; level l uses coords / 2^l.  Zero padding outside the
 *              map; NaN, +-inf and |coord / 2^l| >= 1e6 read as all-zero windows
 *   out        (B, num_levels * (2r+1)^2, H, W) float32, fully overwritten.  Channel l*(2r+1)^2 + i*(2r+1) + j is the bilinear
 *              sample at (x/2^l + i - r, y/2^l + j - r) of <fmap1[b,:,query], fmap2_l[b,:,.]> / sqrt(C): the FIRST window
 *              axis offsets x (the layout of alo_corr_lookup)
 *
 * With num_levels | ALO_CORR_ALT_GRAD the call is the adjoint of that lookup with respect to fmap1 and every level of fmap2:
 *   workspace  of the FLAGGED size.  The prepared part is read.  The gradient region is ADDED TO: the call WRITES THROUGH THIS
 *              `const` POINTER.  The caller zeroes the region before the first of the lookups whose gradients are to be summed;
 *              calls that share a workspace must be ordered (one stream)
 *   coords     as above.  A query that reads as an all-zero window adds nothing
 *   out        is READ: grad_out, (B, num_levels * (2r+1)^2, H, W) float32
 * The checks are the unflagged call's, in its order, with the flagged workspace size.  grad_fmap1's planes are added to with plain
 * loads and stores (bitwise reproducible); the levels' gradients with float atomics, so their last bits depend on the run.
 */
int alo_corr_alt_lookup(const void* workspace, size_t workspace_bytes, const float* coords, float* out, int B, int C, int H,
                        int W, int radius, int num_levels, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ALO_CORR_ALT_H */
