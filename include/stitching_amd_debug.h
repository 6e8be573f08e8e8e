/* stitching_amd_debug.h — TEST HOOKS of libstitching_amd.so.  Not part of the drop-in surface (include/stitching_amd.h): nothing in
 * stitching/warper.py or stitching/blender.py has a counterpart for these, and the Python classes never call them.  They exist so that
 * tests can look at intermediate values the fused kernels never store.
 */
#ifndef STITCHING_AMD_DEBUG_H
#define STITCHING_AMD_DEBUG_H

#include "stitching_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fp32 backward map of a warp — what cv.PyRotationWarper(type, scale).buildMaps(size, K, R) hands to cv.remap in
 * stitching/warper.py:44-51 (RotationWarperBase::buildMaps: xmap, ymap = projector.mapBackward(u, v) for every pixel of the roi) — as
 * the DEVICE projector computes it: the warp kernels run up to the division x / z, y / z and store the two quotients instead of the
 * samples they select.  `which` = 1: the kernel stx_warp / stx_warp_batch would launch for this camera (the tuned kernel of the
 * spherical / cylindrical / plane / affine warpers: tabled trig, packed row pairs, shared-reciprocal division); 2: the generic
 * one-pixel-per-lane kernels (what the float remap modes run).  rect_xywh: NULL -> the warp roi (returned in out_xywh), else any
 * rectangle in warp coordinates.  Outputs: two f32x1 images of the rectangle's size.  The process-wide trig mode applies.
 * tests/test_gpu_maps.py compares them with the CPU checker's build_maps: 0 ULP. */
int stx_debug_warp_maps(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], int w, int h, int which,
                        const int rect_xywh[4], stx_buf** out_xmap_f32, stx_buf** out_ymap_f32, int out_xywh[4]);

/* Saturation distance of the feather blender's distance transform (stitching/blender.py:34-36 -> FeatherBlender::createWeightMap ->
 * distanceTransform(DIST_L1, 3): OpenCV's 16.16 fixed point clamps at INT_MAX >> 2 = 8192.0f).  The sharded feather blender sizes the
 * halo of its strips by it (stitching_amd/distributed.py: FEATHER_DIST_CAP); tests/test_host_logic.py ties the two together. */
int stx_debug_feather_dist_cap(void);

/* How many gather launches of the LAST blend() on this context took their images from the cover table of an adopted stx_mb_weights
 * handle instead of searching for them (stx_blend_use_weights; levels 0 .. bands - 3 of a multi-band blender with at most 64 images
 * whose regions are the ones the table was recorded over): 0 when the blender searched.  tests/test_gpu_cover_replay.py. */
int stx_debug_blend_replayed(stx_ctx* ctx, int* out_launches);

/* How many table kernels (warp_tables_kernel: one per launch batch of the typed projectors) the LAST batched warp call on this context
 * launched: 0 when every batch read the kept tables of a stx_warp_tables handle.  tests/test_gpu_warp_tables_kept.py. */
int stx_debug_warp_table_launches(stx_ctx* ctx, int* out_launches);

/* How many descriptor tables (StxMbImage arrays) the LAST blend() on this context copied to the device: 0 when an adopted blender found
 * its table, byte for byte, among the resident copies of its stx_mb_weights handle.  tests/test_gpu_blend_resident.py. */
int stx_debug_blend_uploads(stx_ctx* ctx, int* out_uploads);

/* 1 when the level-0 launch of the LAST multi-band blend() on this context stored the panorama mask, 0 when it did not: an adopted
 * blender over the output region its stx_mb_weights handle recorded the mask for hands out the handle's mask instead (also 0 after a
 * blend() of another kind).  tests/test_gpu_blend_resident.py. */
int stx_debug_blend_mask_stored(stx_ctx* ctx, int* out_stored);

/* Which kernels the seam masks of this context went through (stx_seam_mask_resize, stx_seam_mask_resize_batch, ..._batch_sub): the
 * profiler gives every path the one name "seam_mask_resize".  out_images = images launched so far, counted since the context was made,
 * through {the one-launch LDS kernel, the table-fed 4-pixel batch kernels, the single-image 4-pixel kernels, the per-pixel kernel}.
 * A caller reads it before and after a call and takes the difference.  tests/test_gpu_constructed_resizes.py. */
int stx_debug_seam_resize_paths(stx_ctx* ctx, int out_images[4]);

#ifdef __cplusplus
}
#endif
#endif /* STITCHING_AMD_DEBUG_H */
