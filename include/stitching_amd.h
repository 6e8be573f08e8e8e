/* stitching_amd.h — C ABI of the MI355X (gfx950) warp + blend back end.
 *
 * Drop-in boundary for ONE hot path of OpenStitching/stitching: what
 * stitching/warper.py and stitching/blender.py reach through cv2.  Each entry point
 * below names the reference call site it replaces (file:line in /root/reference) and the
 * OpenCV routine behind it.  Plain C types only: the library is loaded with ctypes
 * (stitching_amd/_lib.py); INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - every function returns STX_OK (0) or a negative STX_ERR_* code; stx_last_error()
 *     gives the thread-local message.  The Python shim raises StitchingError
 *     (reference: stitching/stitching_error.py:1-2).
 *   - one stx_ctx per (process, GPU); it owns one HIP stream and a caching device
 *     allocator.  Calls on one ctx must be serialised by the caller (the reference is
 *     single threaded: stitching/stitcher.py:247-254).  All work is enqueued on the ctx
 *     stream; only stx_buf_to_host, stx_warp_roi(s), stx_ctx_sync and stx_prof_* wait.
 *   - inputs are borrowed for the duration of the call; outputs are library-owned
 *     opaque handles released with stx_buf_free / stx_blend_destroy / stx_ctx_destroy.
 *   - images are row-major HWC exactly as numpy/cv2 hand them over: u8x3 BGR images,
 *     u8x1 masks, optionally s16x3 (what stitching/blender.py:41 produces with astype).
 *   - K and R are 3x3 row-major fp32 (the reference casts: stitching/warper.py:86,
 *     stitching/camera_estimator.py:25-26).
 */
#ifndef STITCHING_AMD_H
#define STITCHING_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STX_VERSION 100 /* 0.1.0 */

/* status codes */
#define STX_OK 0
#define STX_ERR_INVALID (-1)     /* bad argument (mirrors CV_Assert failures)        */
#define STX_ERR_HIP (-2)         /* HIP runtime error                                 */
#define STX_ERR_OOM (-3)         /* device allocation failed                          */
#define STX_ERR_STATE (-4)       /* call order violated (e.g. feed after finish)      */
#define STX_ERR_UNSUPPORTED (-5) /* valid in the reference, not implemented here      */

/* trig modes.  stitching/warper.py:44-51 builds a cv.PyRotationWarper per call; its projectors evaluate sinf / cosf with the
 * HOST's libm, so the warp coordinates of the reference depend on the machine it runs on.  The back end offers:
 *   STX_TRIG_EXACT       correctly rounded sinf / cosf (default; equals any libm wherever that libm is correctly rounded);
 *   STX_TRIG_GLIBC       sinf / cosf as glibc >= 2.28 computes them on an x86-64-v3 host (__sinf_fma / __cosf_fma): bit-identical to
 *                        that libm on every float argument (tests/test_glibc_trig.py);
 *   STX_TRIG_GLIBC_NOFMA the same routines without fused multiply-add (__sinf_sse2 / __cosf_sse2).
 * The mode is process-wide, like the libm it stands for: STITCHING_AMD_TRIG = exact | glibc | glibc-nofma at first use, or
 * stx_set_trig_mode.  atan2f / acosf / tanf / ... (forward maps: warp_roi) stay correctly rounded in every mode. */
#define STX_TRIG_EXACT 0
#define STX_TRIG_GLIBC 1
#define STX_TRIG_GLIBC_NOFMA 2
int stx_set_trig_mode(int mode);
int stx_get_trig_mode(void);

/* remap modes.  stitching/warper.py:46-51 calls cv.remap(INTER_LINEAR, BORDER_REFLECT) on fp32 maps.  OpenCV 4.x quantises the
 * position to 1/32 pixel and blends the four taps with Q15 table weights (remapBilinear); the reference pins opencv-python 5.0.0.93
 * (requirements.txt:1), whose build is not available here — if it interpolates in fp32 on the unquantised position, the bytes differ by
 * 1-2 LSB on about a sixth of the pixels (profiles/r02_oracle_sensitivity.md).  The back end offers both arithmetic models:
 *   STX_REMAP_Q15        the classic fixed-point scheme (default; the tuned kernels);
 *   STX_REMAP_FLOAT      fp32 bilinear on the unquantised position: a = x - floor(x), t = a (p01 - p00) + p00, u likewise on the lower
 *                        row, cvRound(b (u - t) + t), every step rounded to fp32 (multiply and add separate);
 *   STX_REMAP_FLOAT_FMA  the same with each multiply-add fused.
 * The float modes are a MODEL of that build (oracle/stx_oracle.cpp: bilinear_px_float), unverified against it like everything here
 * that restates OpenCV.  Since round 5 they run on the tuned batched kernel like the default: wavefronts whose samples all lie inside the
 * source blend in fp32 straight from the same two 12-byte windows per row (warp_fast_kernel<.., RM>, blend_float_to_lds), wavefronts that
 * touch a border go one pixel at a time (sample_float); 0.90 x the default's rate on config 2.  Only what the tuned kernel does not
 * take at all (sources beyond 32767 px or 2 GB, a nearest-neighbour source image) runs on the plain one-pixel-per-lane kernels, in any
 * mode.  Masks (INTER_NEAREST) are the same in every mode.
 * Process-wide: STITCHING_AMD_REMAP = q15 | float | float-fma at first use, or stx_set_remap_mode. */
#define STX_REMAP_Q15 0
#define STX_REMAP_FLOAT 1
#define STX_REMAP_FLOAT_FMA 2
int stx_set_remap_mode(int mode);
int stx_get_remap_mode(void);

/* pyrDown order of the fp32 weight pyramids.  stitching/blender.py:40-41 -> MultiBandBlender::feed -> pyrDown(CV_32F) per level.  The
 * 5-tap sums are integers for the image planes (any order gives the same bits) but fp32 for the weights, where OpenCV's scalar loop
 * and its SIMD code associate differently:
 *   scalar      row:  s2*6 + (s1+s3)*4 + s0 + s4                 column: the same expression
 *   SIMD        row:  s2*6 + ((s1+s3)*4 + (s0+s4))               column: (r1+r3+r2)*4 + (r0+r4+(r2+r2))
 * and a build with FMA contracts each multiply-add.  The vector code covers the outputs 1 .. 1 + ((width0-1)/L)*L of a row
 * (width0 = min((w-3)/2+1, dw), L = lanes per vector) and the first (dw/L)*L outputs of the column pass; the rest is the scalar loop.
 * With 0 / 255 masks the levels 1..3 are exact in every order; coarser levels, and grey masks from level 1 on, move by an ULP and the
 * panorama by at most 1 LSB at a few bytes (profiles/r02_oracle_sensitivity.md).
 *   STX_PYRDOWN_SCALAR (default: the tuned kernels)   STX_PYRDOWN_SIMD_V: column pass vectorised   STX_PYRDOWN_SIMD_HV: both
 *   | STX_PYRDOWN_FMA: fused multiply-adds in the vector code;   lanes = 4 (SSE / NEON), 8 (AVX2), 16 (AVX-512)
 * Like the float remap these are MODELS of OpenCV builds (the CPU checker holds the same ones), unverified here; any mode but the default
 * builds the pyramids with the plain one-sample-per-lane kernels.  Process-wide: STITCHING_AMD_PYRDOWN = scalar | simd-v | simd-hv |
 * simd-v-fma | simd-hv-fma, optionally ":lanes" (simd-hv:8), at first use, or stx_set_pyrdown_mode; read when a blender builds its pyramids. */
#define STX_PYRDOWN_SCALAR 0
#define STX_PYRDOWN_SIMD_V 1
#define STX_PYRDOWN_SIMD_HV 3
#define STX_PYRDOWN_FMA 4
int stx_set_pyrdown_mode(int mode, int lanes);
int stx_get_pyrdown_mode(int* out_lanes);

/* warper types: the names of Warper.WARP_TYPE_CHOICES (stitching/warper.py:10-27);
 * cv.PyRotationWarper(type, scale) string -> id in the Python shim */
#define STX_WARP_PLANE 0
#define STX_WARP_AFFINE 1
#define STX_WARP_CYLINDRICAL 2
#define STX_WARP_SPHERICAL 3
/* the other twelve names cv.PyRotationWarper accepts: generic RotationWarperBase<P> warpers (roi from every source
 * pixel, per-pixel projector), (a, b) fixed by the name as in PyRotationWarper's constructor */
#define STX_WARP_FISHEYE 4
#define STX_WARP_STEREOGRAPHIC 5
#define STX_WARP_COMPRESSED_PLANE_A2B1 6
#define STX_WARP_COMPRESSED_PLANE_A15B1 7
#define STX_WARP_COMPRESSED_PLANE_PORTRAIT_A2B1 8
#define STX_WARP_COMPRESSED_PLANE_PORTRAIT_A15B1 9
#define STX_WARP_PANINI_A2B1 10
#define STX_WARP_PANINI_A15B1 11
#define STX_WARP_PANINI_PORTRAIT_A2B1 12
#define STX_WARP_PANINI_PORTRAIT_A15B1 13
#define STX_WARP_MERCATOR 14
#define STX_WARP_TRANSVERSE_MERCATOR 15
#define STX_WARP_TYPE_COUNT 16

/* cv.INTER_* / cv.BORDER_* values used by stitching/warper.py:49-50,65-66 */
#define STX_INTER_NEAREST 0
#define STX_INTER_LINEAR 1
#define STX_BORDER_CONSTANT 0
#define STX_BORDER_REFLECT 2

/* blender kinds (stitching/blender.py:8-12) */
#define STX_BLEND_NO 0
#define STX_BLEND_FEATHER 1
#define STX_BLEND_MULTIBAND 2

/* element types of stx_buf */
#define STX_U8 0
#define STX_S16 1
#define STX_F32 2

typedef struct stx_ctx stx_ctx;
typedef struct stx_buf stx_buf;
typedef struct stx_blender stx_blender;
typedef struct stx_mb_weights stx_mb_weights;
typedef struct stx_warp_tables stx_warp_tables;

/* ---- library / context ------------------------------------------------------------ */
int stx_version(void);
const char* stx_last_error(void);
int stx_device_count(int* out_n);
int stx_ctx_create(int device, stx_ctx** out);
int stx_ctx_destroy(stx_ctx* ctx);
int stx_ctx_sync(stx_ctx* ctx);

/* ---- device images ------------------------------------------------------------------
 * Replaces the numpy.ndarray / cv.UMat values that cross the reference's cv2 boundary
 * (stitching/blender.py:41 cv.UMat(img.astype(np.int16))). */
int stx_buf_from_host(stx_ctx* ctx, const void* host, size_t host_stride_bytes, int w, int h, int channels, int elem,
                      stx_buf** out);
int stx_buf_alloc(stx_ctx* ctx, int w, int h, int channels, int elem, stx_buf** out);
/* page-locked host memory (for decoded frames / read-backs): stx_buf_from_host / stx_buf_to_host on such memory run at
 * PCIe rate instead of the pageable-copy rate (the cv.imread -> UMat staging in front of stitching/images.py:111) */
int stx_host_alloc(size_t bytes, void** out);
int stx_host_free(void* p);
int stx_buf_to_host(const stx_buf* buf, void* host, size_t host_stride_bytes);
/* asynchronous forms for page-locked host memory (stx_host_alloc): the copy is queued on the context's stream and the
 * call returns; the host memory must stay untouched (upload) / unread (read-back) until stx_ctx_sync(ctx).  With pageable
 * memory they behave like the synchronous calls.  Two contexts fed alternately keep both PCIe directions busy. */
int stx_buf_from_host_async(stx_ctx* ctx, const void* host, size_t host_stride_bytes, int w, int h, int channels, int elem,
                            stx_buf** out);
int stx_buf_to_host_async(const stx_buf* buf, void* host, size_t host_stride_bytes);
/* rectangular sub-view sharing the parent's memory (numpy slicing in stitching/cropper.py:150-151) */
int stx_buf_view(const stx_buf* buf, int x, int y, int w, int h, stx_buf** out);
/* Source validity masks: which pixels of a frame are picture (a lens' wedges, the corners of a circular fisheye image, a mount in view).
 * stx_buf_with_validity: a NEW handle onto the same pixels as img (a whole-image view) that carries mask — u8x1 of img's size, same
 *   context; the handle holds a reference on it, img itself is not changed and mask is never written.  Refused with STX_ERR_INVALID
 *   before anything is allocated: a null handle, img not u8x3, mask not u8x1, unequal sizes, different contexts, img already carrying a
 *   mask.  stx_buf_view of such a handle carries the matching view of the mask.
 * stx_buf_validity: a new handle on the attached mask, or *out = NULL when there is none.
 * Honoured by stx_warp_batch and stx_warp_image_and_mask where they write masks (see stx_warp_batch); every other entry point reads
 * the pixels and ignores the mask. */
int stx_buf_with_validity(const stx_buf* img, const stx_buf* mask_u8x1, stx_buf** out);
int stx_buf_validity(const stx_buf* buf, stx_buf** out);
/* info = {w, h, channels, elem, stride_bytes, device} */
int stx_buf_info(const stx_buf* buf, int64_t info[6]);
/* device address of the first pixel (for zero-copy consumers, e.g. RCCL strip exchange) */
int stx_buf_device_ptr(const stx_buf* buf, void** out);
int stx_buf_free(stx_buf* buf);

/* ---- Warper -------------------------------------------------------------------------
 * stx_warp_roi  <- stitching/warper.py:79-82  cv.PyRotationWarper(type, scale).warpRoi(size, K, R)
 *                  (RotationWarperBase::warpRoi / detectResultRoi[ByBorder],
 *                   SphericalWarper::detectResultRoi, PlaneWarper/AffineWarper::warpRoi)
 * out_xywh = (tl.x, tl.y, br.x-tl.x+1, br.y-tl.y+1). */
int stx_warp_roi(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], int w, int h,
                 int out_xywh[4]);
/* batched form of the loop in stitching/warper.py:70-77 (one device pass, one sync) */
int stx_warp_rois(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s, const int* sizes_wh,
                  int* out_xywh);
/* stx_warp <- stitching/warper.py:43-52 (interp=LINEAR, border=REFLECT, src u8x3) and
 *             stitching/warper.py:58-68 (interp=NEAREST, border=CONSTANT, src u8x1):
 *             cv.PyRotationWarper(type, scale).warp(src, K, R, interp, border)
 *             = RotationWarperBase::buildMaps + cv::remap, fused: maps are never stored.
 * out_tl receives the corner the reference discards (stitching/warper.py:45 `_`). */
int stx_warp(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], const stx_buf* src, int interp,
             int border, stx_buf** out, int out_tl[2]);
/* fused form of warper.py:43-52 + 58-68 for one camera: one pass computes the backward map
 * once and writes both the bilinear image and the nearest-neighbour 255-mask.
 * out_img / out_mask may each be NULL. */
int stx_warp_image_and_mask(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9],
                            const stx_buf* src, stx_buf** out_img, stx_buf** out_mask, int out_xywh[4]);
/* stx_warp_batch: batched form of the generator loops stitching/warper.py:39-41 (warp_images) and :54-56 (create_and_warp_masks) for n
 * cameras of one warper: ROIs in one device pass, then ONE table launch and ONE remap launch for all images (the per-image argument
 * blocks travel as kernel arguments: no upload, no host synchronisation).  out_imgs / out_masks are arrays of n handles; either may be
 * NULL, not both.  out_xywh (or NULL) receives the n rectangles warped: the ROIs, or rects_xywh echoed.  The options, each NULL / 0
 * where absent; what breaks a rule below is refused with STX_ERR_INVALID before the device is touched:
 *
 * rects_xywh: caller-given destination rectangles (x, y, w, h in warp coordinates, normally sub-rectangles of the ROIs of
 *   stx_warp_rois) instead of the ROIs: the pixels are exactly those of the full warp inside the rectangle.  For pipelines that know
 *   which part of a warped image the blender can see (seam masks: stitching/stitcher.py:124 cuts every image down to its seam cell AFTER
 *   warping all of it, :119-121).
 * gain_maps, gain_flags: the block gains of the exposure compensator in the same call: the loops stitching/stitcher.py:119-123 (warp final
 *   images, then compensator.apply on each) for the "gain_blocks" compensator.  gain_maps[i]: f32x1 (f32x3: channel_blocks) map of image
 *   i, laid over its WHOLE warped image (BlocksCompensator::apply) also when rects_xywh names a rectangle of it, which must then lie
 *   inside the ROI; gain_flags (or NULL) as in stx_block_gain_apply_batch.  The product happens in the warp kernel's epilogue when it can
 *   (tuned kernel, bounded f32x1 maps), else as a second pass: out_imgs equal stx_block_gain_apply_batch over the images of the call
 *   without gain_maps byte for byte either way.  Needs out_imgs.
 * flags & STX_WARP_FRESH_ROIS: one panorama's warps, its ROI pass included: stitching/stitcher.py:188 (warp_rois) + :119-123 in ONE call.
 *   The ROIs are computed by this call (never taken from the cache of earlier calls: a panorama pays for its own ROI pass) and returned in
 *   out_xywh; the host waits for them once, inside the call, by polling stamps the ROI kernel writes into pinned memory, and launches the
 *   warps right behind — the device idles for ~25 us at the head of a panorama instead of the ~145 us of stx_warp_rois + Python + a
 *   second call (profiles/r05_latency.md).  Results equal stx_warp_rois + the call without the flag byte for byte.  Needs out_xywh and no
 *   rects_xywh; other bits of flags are refused.
 * tables: for the panoramas of one rig.  The per-column / per-row tables of the typed projectors (plane, affine, cylindrical, spherical,
 *   mercator) follow from the cameras, the rectangles, the scale and the trig mode — never from the pixels — so a handle keeps them
 *   between calls.  *tables = NULL on the first call: a handle is made and filled; a call that fails leaves it NULL.  A later call with
 *   the handle compares everything the table kernel reads (projector type and family; per image the rectangle, scale, trig mode, t[0..1]
 *   and the products' factors k_rinv[1], [4], [7]) with the handle's record: equal -> no table kernel is launched and no table block
 *   allocated, the warp reads the kept tables; any difference -> the tables are rebuilt into the handle in stream order and the record
 *   updated.  The library decides, never the caller; the bytes are those of the calls without a handle either way.  The per-pixel
 *   projector families use no tables and leave the handle empty.  Kept tables belong to given rectangles: rects_xywh, or
 *   STX_WARP_FRESH_ROIS on the first panorama of a rig, whose ROIs become the rects_xywh of the later calls.  A handle belongs to the
 *   context that made it: another context's is refused.  stx_warp_tables_free gives the block back (stream-ordered: warps that read it
 *   may still be in flight).
 * validity: a source made by stx_buf_with_validity carries its own mask M, and the warped mask of that image is then
 *   remapNearest(M, xmap, ymap) with a constant 0 border — the source value at (saturate_cast<short>(cvRound(x)), ... (y)) where both
 *   indices are inside, 0 elsewhere, cvRound taken of the fp32 coordinate itself — instead of the warp of a 255-filled rectangle.  An
 *   image without a mask behaves as with a 255-filled one, and a batch may mix both.  The image bytes, the ROIs, out_xywh and the
 *   tables' record do not depend on the mask; a grey mask comes out grey, and the warped mask counts as binary (stx_buf_flags) when M
 *   does.  With gain_maps on top the gain runs as the second pass (equal bytes, see above).  M may be a view (its own pitch). */
#define STX_WARP_FRESH_ROIS 1
int stx_warp_batch(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s, const stx_buf* const* srcs,
                   const int* rects_xywh, const stx_buf* const* gain_maps_f32, const int* gain_flags, int flags, stx_buf** out_imgs,
                   stx_buf** out_masks, int* out_xywh, stx_warp_tables** tables);
int stx_warp_tables_free(stx_warp_tables* t);
/* stitching/warper.py:58-68 without allocating the 255-filled source (size only) */
int stx_warp_mask(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], int w, int h,
                  stx_buf** out_mask, int out_xywh[4]);

/* the widest image the feather blender takes (stx_blend_feed) */
#define STX_FEATHER_MAX_WIDTH 32768

/* ---- Blender ------------------------------------------------------------------------
 * stx_result_roi    <- stitching/blender.py:24    cv.detail.resultRoi(corners, sizes)
 * stx_blend_create  <- stitching/blender.py:27-38 Blender_createDefault(NO) | detail_MultiBandBlender()
 *                      + setNumBands | detail_FeatherBlender() + setSharpness, then .prepare(dst_sz)
 *                      (Blender/FeatherBlender/MultiBandBlender::prepare)
 * stx_blend_feed    <- stitching/blender.py:40-41 blender.feed(UMat(int16 img), mask, corner)
 *                      img: u8x3 (converted on load) or s16x3; mask u8x1.  DEFERRED for all three kinds: the blender
 *                      keeps a reference to img and mask and reads them in stx_blend_finish (one gather over the
 *                      panorama), so the two buffers must not be modified between feed and finish (OpenCV consumes
 *                      them inside feed).  Limit of the feather blender, checked before anything is allocated or
 *                      launched (STX_ERR_INVALID): an image of at most STX_FEATHER_MAX_WIDTH columns — the row pass of
 *                      its distance transform keeps a row in LDS, 2 bytes per column; the refused feed leaves the
 *                      blender as it was
 * stx_blend_finish  <- stitching/blender.py:43-48 blender.blend() + cv.convertScaleAbs(result)
 *                      returns the u8x3 panorama and the u8 mask; consumes the blender
 *                      (a second finish is STX_ERR_STATE; OpenCV releases dst_ in blend). */
int stx_result_roi(int n, const int* corners_xy, const int* sizes_wh, int out_xywh[4]);
int stx_blend_create(stx_ctx* ctx, int kind, int num_bands, float sharpness, const int roi_xywh[4],
                     stx_blender** out);
/* band count after MultiBandBlender::prepare's clamp (0 for the other kinds) */
int stx_blend_num_bands(const stx_blender* b, int* out_num_bands);
int stx_blend_feed(stx_blender* b, const stx_buf* img, const stx_buf* mask, int tlx, int tly);
int stx_blend_finish(stx_blender* b, stx_buf** out_pano_u8, stx_buf** out_mask_u8);
/* as stx_blend_finish, but also hands out the int16 result that blender.blend() returns
 * before convertScaleAbs (stitching/blender.py:46); any out pointer may be NULL.
 * THE RETURNED MASK IS READ-ONLY where weights are kept (stx_blend_keep_weights / stx_blend_use_weights below): the mask a blender marked
 * by stx_blend_keep_weights returns is also held by its handle, and a blender that adopted the handle returns THAT SAME buffer (one more
 * reference) instead of storing the same bytes again — the panoramas of a known rig may share one mask buffer from run to run.  Whoever
 * writes into it changes the mask of every later panorama of the rig.  The buffer is reference-counted like every stx_buf: it stays
 * valid after the handle, the blenders and the context's other users of it are gone, until its last stx_buf_free.  A caller that needs
 * a mask of its own copies it.  Blenders without a handle return a buffer of their own, as ever. */
int stx_blend_finish_ex(stx_blender* b, stx_buf** out_pano_u8, stx_buf** out_mask_u8, stx_buf** out_pano_s16);
int stx_blend_destroy(stx_blender* b);
/* Weight pyramids that outlive their blender: the panoramas of one rig ("video: same rig, new frames").  W_1..W_B of a fed image, their
 * occupancy maps included, depend on its mask and on the geometry of the feed — never on the pixels — so a second panorama with the
 * same masks at the same places need not build them again.
 * stx_blend_keep_weights: on a multi-band blender, after its feeds and before stx_blend_finish.  After a finish that succeeded the handle owns the
 *   wt[1..B] allocations and the occupancy arena of every image fed (they no longer die with the blender), holds a reference to every
 *   mask buffer AND TO THE PANORAMA MASK this finish returns (w x h bytes of the output region: 54 MB for eight 4000 x 3000 frames, next to
 *   the ~150 MB of weights; see stx_blend_finish_ex: read-only from here on), four small device copies of the blenders' descriptor table
 *   (stx_blend_use_weights) and records per image: mask buffer, 0/255 flag and the half-precision W_1 flag, size, corner, feed rectangle, border
 *   offsets, and the blender's band count and pyrDown mode.  Needs: only images fed on this blender (no received strips), u8 images,
 *   the batched pyramid kernels (STX_PYRDOWN_SCALAR), occupancy recording on, >= 1 band, weights of its own (not adopted ones).  Where
 *   that does not hold *out is NULL, the call returns STX_OK and the blender builds as ever.  A handle whose blender never finished
 *   stays empty and is never adopted.
 * stx_blend_use_weights: on a fresh blender after its feeds (no feed may follow).  *out_adopted = 1: every fed image matches the handle's
 *   record field for field (same order, same mask buffer, same geometry, bands, mode), the blender has taken the handle's weight and
 *   occupancy pointers in place of its own allocations and builds its pyramids without their weight half (no mask read, no weight
 *   read / sum / write, no occupancy note: the "mb_down0" / "mb_down" profiler entries carry the bytes of what then moves).
 *   Such a blender also (i) finds its descriptor table (per image: geometry and buffer addresses) among the handle's four resident device
 *   copies when the same addresses come round again — the context's allocator hands out the lowest free block of a size, so they do — and
 *   then uploads nothing, else overwrites the least recently used copy in stream order; (ii) returns the handle's panorama mask from
 *   stx_blend_finish[_ex] and stores none, when its output region is the one the mask was recorded over (no stx_blend_set_band in
 *   between) and its level-0 launch replays the recorded image search; otherwise it stores a mask of its own as ever.
 *   *out_adopted = 0: nothing was adopted — all images or none — and everything is built as ever.  The masks must hold what they held
 *   at the keep: the caller owns that promise.  Handle and blender live on ONE context, whose stream order makes the weights ready
 *   before their first reuse; a blender of another context is refused with STX_ERR_INVALID.
 * stx_mb_weights_free: gives the allocations back (stream-ordered: blenders that adopted the handle may still be in flight). */
int stx_blend_keep_weights(stx_blender* b, stx_mb_weights** out);
int stx_blend_use_weights(stx_blender* b, stx_mb_weights* w, int* out_adopted);
int stx_mb_weights_free(stx_mb_weights* w);

/* ---- "next" rows either side of the path -----------------------------------------------------
 * stx_gain_apply      <- stitching/exposure_error_compensator.py:43-45 compensator.apply(idx, corner, img, mask) for the
 *                        "gain" / "channel" compensators (GainCompensator::apply, ChannelsCompensator::apply =
 *                        cv::multiply(image, gain): fp32 product, cvRound, saturate to u8), in place on the warped image
 *                        between warp and feed (stitching/stitcher.py:123,219-221).  The block compensators
 *                        ("gain_blocks", "channel_blocks") are stx_block_gain_apply_batch below.
 * stx_timelapse_frame <- stitching/timelapser.py:36-52 timelapser.process(img, mask, corner) + getDst():
 *                        zero frame of the roi given to initialize(), the image pasted at its corner. */
int stx_gain_apply(stx_ctx* ctx, stx_buf* img_u8x3, const float gains_bgr[3]);
/* the reference's default compensator "gain_blocks": BlocksCompensator::apply = cv::resize(gain map, image size,
 * INTER_LINEAR) [fp32] + cv::multiply, fused (the full-size gain map is never stored); gain_map is f32x1, or f32x3 (BGR
 * maps, interleaved) for "channel_blocks" (BlocksChannelsCompensator).  For all n images of a panorama (the generator loop
 * stitching/stitcher.py:219-221): two launches per 16 images, gain maps resident on the device.  full_wh_xy0 (or NULL) = {full_w, full_h, x0, y0} per image: imgs[i] is the rectangle at (x0, y0) of a warped
 * image of size full_w x full_h (a seam-cell crop: stx_warp_batch with rects_xywh) and the gain map is laid over the FULL image, as
 * BlocksCompensator::apply does — the rectangle's bytes equal those of the whole image compensated and then cut.
 * flags (or NULL): STX_GAIN_MAP_BOUNDED per image — the caller has checked that every gain of the map is finite and below 2^31 / 255. */
#define STX_GAIN_MAP_BOUNDED 1
int stx_block_gain_apply_batch(stx_ctx* ctx, int n, stx_buf* const* imgs_u8x3, const stx_buf* const* gain_maps_f32,
                               const int* full_wh_xy0, const int* flags);
/* ---- exposure-gain estimation: ExposureCompensator::feed (stitching/exposure_error_compensator.py:39-41) ------------------------
 * kind: the cv.detail ids of the compensators that estimate (ExposureCompensator_GAIN, _GAIN_BLOCKS, _CHANNELS, _CHANNELS_BLOCKS).
 * The overlap statistics of every feed are one kernel launch over a table of unit pairs (whole images or blocks); the linear system
 * is assembled on the host and solved there by default (OpenCV's cv::solve(DECOMP_LU), eliminating only non-zero entries: the same bits
 * as the dense loop) or on the device (below: the same bits again).  Parity: a restatement of OpenCV 4.x from recollection; tests/numpy_exposure.py is the contract. */
#define STX_EXPOSURE_GAIN 1
#define STX_EXPOSURE_GAIN_BLOCKS 2
#define STX_EXPOSURE_CHANNELS 3
#define STX_EXPOSURE_CHANNELS_BLOCKS 4
/* stx_exposure_feed_ex (declared below, with its solver argument): the whole feed of n u8x3 images and their u8x1 masks (pixels count where both masks are 255) at corners_xy.  Gains go to
 * out_gains image after image: gain 1 value, channels 3 (BGR), gain_blocks bh x bw fp32 map values (filtered as getMatGains returns
 * them), channels_blocks bh x bw x 3, with bw = ceil(w / block_size), bh = ceil(h / block_size).  *inout_count: capacity of
 * out_gains in values; out_gains NULL: only writes the count needed (no GPU work).  The images are never modified.
 * The device statistics ms of out_info are HIP events over all feeds. */
/* The statistics of the first feed alone, per pair job: units (a, b) with a <= b, the count c of pixels both masks hold 255 in,
 * and the sums of norms over them ({sum_a, sum_b} for the gain kinds; {B, G, R of a, B, G, R of b} for the channel kinds: six
 * values per job either way).  out_ab NULL: only writes *inout_jobs (the pair enumeration runs, no GPU work). */
int stx_exposure_stats(stx_ctx* ctx, int kind, int n, const stx_buf* const* imgs_u8x3, const stx_buf* const* masks_u8,
                       const int* corners_xy, int block_size, long long* inout_jobs, int* out_ab, long long* out_c,
                       double* out_sums);
/* Host only (no context, no GPU): assembly + solve of GainCompensator::singleFeed from given statistics of m units.  npairs entries
 * (i, j) with i <= j; n_iij_iji = {N(i,j), I(i,j), I(j,i)} each; pairs not listed have N = 0.  skip[u] != 0: unit u overlaps no
 * other unit (gain 1).  out_gains: m values. */
int stx_exposure_solve(int m, int npairs, const int* pairs_ij, const double* n_iij_iji, const unsigned char* skip,
                       double* out_gains);
/* ---- the gain systems solved on the device -------------------------------------------------------------------------------------
 * cv::solve(DECOMP_LU) as a dense fp64 elimination in HIP, returning THE SAME BITS as the host solve above: partial pivoting by the
 * largest |a[j][i]| (the smallest row among equal magnitudes), alpha = a[j][i] * (-1 / a[i][i]), a[j][k] = a[j][k] + alpha * a[i][k]
 * as one rounded product and one rounded sum (no FMA), every element updated by the pivots in ascending order; a blocked right-looking
 * scheme (32 pivots per step: panel, row swaps + the panel's rows, trailing update) with the pivot indices on the device and no host
 * synchronisation before the end.  The back substitution is one dependent chain: the non-zeros of U and the transformed right side are
 * compacted on the device, copied back and substituted on the host in the host solve's order.  Inputs must be finite and hold no -0.
 * Limit: the dense matrix takes 8 n^2 bytes of device memory; more than 16384 unknowns (2 GiB) are refused with STX_ERR_INVALID —
 * there is no fall-back to the host.  A singular system fails with STX_ERR_INVALID, "exposure system is singular at row %d".
 * Which one to pick: the device from a few thousand unknowns on (DESIGN.md section 9 has the measured table); below, the host.
 *
 * The solver of a feed is a process-wide mode: STX_EXPOSURE_SOLVER_HOST (default) or _DEVICE; STITCHING_AMD_EXPOSURE_SOLVER
 * (host | device) sets the start-up value.  stx_exposure_feed_ex takes it per call (STX_EXPOSURE_SOLVER_DEFAULT: the mode). */
#define STX_EXPOSURE_SOLVER_DEFAULT (-1)
#define STX_EXPOSURE_SOLVER_HOST 0
#define STX_EXPOSURE_SOLVER_DEVICE 1
int stx_set_exposure_solver(int mode);
int stx_get_exposure_solver(void);
/* The feed, with the solver given.  out_info (or NULL): {units, pair jobs, device statistics ms, assembly + solve + filter ms
 * (wall clock: with the device solver it covers the device elimination and the host tail), the solver used, device elimination ms (HIP
 * events), compaction + copy + back substitution ms, non-zeros of U — the last three summed over the solves, 0 with the host solver}. */
int stx_exposure_feed_ex(stx_ctx* ctx, int kind, int n, const stx_buf* const* imgs_u8x3, const stx_buf* const* masks_u8,
                         const int* corners_xy, int block_size, int nr_feeds, int solver, double* out_gains, long long* inout_count,
                         double out_info[8]);
/* The twin of stx_exposure_solve: the same assembly, systems of more than 3 unknowns eliminated on ctx's device (up to 3: Cramer's rule
 * on the host, as there).  out_info (or NULL): {device elimination ms, compaction + copy + back substitution ms, non-zeros of U, 0}. */
int stx_exposure_solve_device(stx_ctx* ctx, int m, int npairs, const int* pairs_ij, const double* n_iij_iji, const unsigned char* skip,
                              double* out_gains, double out_info[4]);
/* The elimination alone, for tests and tools: A (n x n, row-major, host) x = b by the device LU for every n >= 1 -> x_out[n], the bits
 * of tests/numpy_exposure.py::lu_solve(A, b, skip_zeros=False).  out_info as stx_exposure_solve_device. */
int stx_lu_solve_device(stx_ctx* ctx, int n, const double* A_dense_host, const double* b_host, double* x_out, double out_info[4]);
/* ---- exposure-gain tracking on a known rig (tests/numpy_exposure_track.py is the contract) -----------------
 * The gains of ExposureCompensator::feed are estimated once, on the low-resolution pass.  A tracker measures, on the warped and
 * compensated images every panorama of a known rig makes anyway, how far the cameras have drifted since: integer sums over a lattice.
 * The lattice of stride s holds the panorama pixels (X, Y) with X mod s == 0 and Y mod s == 0 (floor-mod: corners are often
 * negative).  Image i is warped into rects_xywh[i]; V_i is 1 at the lattice points inside it where its warped mask is 255 (grey values
 * do not count); c_ii = sum(V_i).  A pair job is (a, b), a < b, whose rectangles intersect (also where the intersection holds no
 * lattice point), in lexicographic order.  Its statistics are eight 64-bit integers c, aB, aG, aR, bB, bG, bR, rej over the lattice
 * points of both rectangles with V_a & V_b: a sample whose six bytes all lie in 1 .. 254 adds 1 to c and its channels to the sums,
 * any other adds 1 to rej (a saturated product cannot be de-compensated).  Integer sums: the same bits whatever the order.
 * stx_exposure_track_create: one launch over the masks (u8x1, the rectangles' sizes; views with their own pitch are taken) makes the V
 *   grids, one byte per lattice point, kept by the handle; the masks are not kept.  One host wait (c_ii comes back).
 * stx_exposure_track_pairs: out_ab NULL and out_self_counts NULL: writes the number of pair jobs to *inout_count.  Else *inout_count is
 *   the capacity of out_ab in pairs; out_ab gets (a, b) per pair, out_self_counts c_ii per image (n values).
 * stx_exposure_track_measure: in the context's stream order — clears the accumulators of slot k mod 2 (k: measures so far), one
 *   launch (a 256-lane workgroup per tile of 32 x 32 lattice points of a pair; one 64-bit integer atomic add per value and workgroup),
 *   an asynchronous copy to page-locked host memory, an event.  No host wait.  imgs_u8x3[i]: the warped, compensated image of
 *   rectangle i (its size; views are taken); it must stay unwritten until the launch has run (stream order does that for the
 *   library's own calls).  At most two measures may be pending.
 * stx_exposure_track_collect: waits for the event of the OLDEST pending measure and copies its pairs x 8 values to out_stats (may
 *   be NULL without pairs).  STX_ERR_INVALID if none is pending.
 * stx_exposure_track_info: {pair jobs, tile jobs, bytes of the V grids, the statistics launch of the last collected measure in ms (HIP
 *   events), the wait of the last collect in ms (host clock), measures so far}.
 * Refused with STX_ERR_INVALID before anything is launched, the context stays usable: null handles or handles of another context,
 * images or masks whose size is not their rectangle's, wrong element types, a stride outside 1 .. STX_TRACK_STRIDE_MAX, n outside
 * 1 .. STX_TRACK_IMAGES_MAX, more than STX_TRACK_TILES_MAX tile jobs (take a larger stride). */
#define STX_TRACK_STRIDE_MAX 64
#define STX_TRACK_IMAGES_MAX 1024
#define STX_TRACK_TILES_MAX 65536
typedef struct stx_exposure_track stx_exposure_track;
int stx_exposure_track_create(stx_ctx* ctx, int n, const int* rects_xywh, const stx_buf* const* masks_u8, int stride,
                              stx_exposure_track** out);
int stx_exposure_track_pairs(stx_exposure_track* t, int* inout_count, int* out_ab, long long* out_self_counts);
int stx_exposure_track_measure(stx_exposure_track* t, const stx_buf* const* imgs_u8x3);
int stx_exposure_track_collect(stx_exposure_track* t, long long* out_stats);
int stx_exposure_track_info(stx_exposure_track* t, double out_info[6]);
int stx_exposure_track_free(stx_exposure_track* t);
/* outs[i] = a new f32 image, maps_f32[i] * factors in fp32 (one rounded product per value), for all n maps in one launch per 32: an
 * f32x1 map with planes == 1 gives f32x1 (factors[i]), with planes == 3 f32x3 (factors[3 i + c] per channel); an f32x3 map gives f32x3
 * (planes == 1: the one factor for all channels).  The factors travel in the kernel's arguments: no upload, no host wait.  Refused with
 * STX_ERR_INVALID before anything is launched: null handles, maps of another context, maps that are not f32x1 / f32x3, planes other
 * than 1 or 3, n outside 1 .. STX_TRACK_IMAGES_MAX.  A failing call hands nothing out. */
int stx_gain_maps_scale(stx_ctx* ctx, int n, const stx_buf* const* maps_f32, const float* factors, int planes, stx_buf** outs);
/* ---- seam finding: SeamFinder::find of the "voronoi" and "no" finders (stitching/seam_finder.py:33-35) -------------------------
 * kind: STX_SEAM_VORONOI (VoronoiSeamFinder: PairwiseSeamFinder::run over the overlapping pairs (i, j), i < j, in order; a gap of
 * 10 pixels around each overlap; dist1 < dist2 of the L1 distances (saturated at 8192) zeroes mask j there, anything else mask i) or
 * STX_SEAM_NO (NoSeamFinder: the masks unchanged).  Parity: a restatement of OpenCV 4.x from recollection;
 * tests/numpy_seams.py is the contract. */
#define STX_SEAM_NO 0
#define STX_SEAM_VORONOI 1
#define STX_SEAM_GAP 10
/* n u8x1 masks of images of sizes_wh = {w, h} per image at corners_xy; every mask must be its image's size.  masks_out[i]: new
 * buffers (the inputs are never written).  The pairs run level by level (stx_seam_schedule), two launches per level.
 * out_info (or NULL): {pairs, levels, device ms of the levels, device ms including the copy of the inputs} (HIP events). */
int stx_seam_find(stx_ctx* ctx, int kind, int n, const int* sizes_wh, const int* corners_xy, const stx_buf* const* masks_in,
                  stx_buf** masks_out, double out_info[4]);
/* Host only (no context, no GPU): the overlapping pairs in PairwiseSeamFinder::run's order, out_pairs = {i, j, roi x, y, w, h} each,
 * and the dependency level of each (0: depends on no earlier pair; else 1 + the highest level among the earlier pairs that share
 * an image with it where one's roi meets the other's roi +- STX_SEAM_GAP clipped to that image).  Running the levels in order, pairs
 * of one level in any order, gives the sequential result.  out_pairs NULL: only writes *inout_npairs. */
int stx_seam_schedule(int n, const int* sizes_wh, const int* corners_xy, int* inout_npairs, int* out_pairs, int* out_levels);
/* ---- colour-aware seams: the project's OWN finder, not OpenCV's DpSeamFinder ("dp_color" / "dp_colorgrad" stay cv2's) -------------
 * Pairwise, integer only, one dynamic programme per overlapping pair in PairwiseSeamFinder::run's order: the cost of a pixel both masks
 * hold is the squared BGR difference of the two images, the seam is the 8-connected path of least cost along the overlap (vertical or
 * horizontal by the images' centres), and it splits the pixels both masks hold between the two images.  tests/numpy_color_seams.py is the
 * contract, byte for byte.
 * images: n u8x3 images of sizes_wh (read only), masks_in: n u8x1 masks of the same sizes (never written), masks_out[i]: new buffers.
 * Limits, checked before anything is launched (STX_ERR_INVALID): a seam of at most STX_COLOR_SEAM_MAX_LENGTH pixels (u32 accumulators:
 * 16384 * 3 * 255^2 < 2^32), at most STX_COLOR_SEAM_MAX_CROSS pixels across it (two u32 accumulator rows of that many in LDS: 32 KiB).
 * The pairs run level by level (stx_seam_schedule), two launches per level.  out_info as stx_seam_find. */
#define STX_COLOR_SEAM_MAX_LENGTH 16384
#define STX_COLOR_SEAM_MAX_CROSS 4096
int stx_color_seam_find(stx_ctx* ctx, int n, const int* sizes_wh, const int* corners_xy, const stx_buf* const* images,
                        const stx_buf* const* masks_in, stx_buf** masks_out, double out_info[4]);
/* ---- cropping: Cropper.estimate_largest_interior_rectangle (stitching/cropper.py:91-106) -----------------------------------------
 * mask_u8x1: the panorama mask (views and pitched buffers allowed; nonzero means true), never copied to the host.
 * out_contours = {foreground components (8-connected), holes (4-connected background components of the zero-framed mask that do
 * not reach its frame)}: findContours' hierarchy is a single entry exactly when they are {1, 0}.  out_xywh: the largest rectangle of
 * true cells, ties broken by smallest y, then smallest x, then largest w; {0, 0, 0, 0} for a mask without true cells.  The rectangle
 * is computed whatever the counts are.  Exact integer arithmetic: the result does not depend on scheduling.  Parity: the reference's
 * lir(grid, contour) returns the same area; which of several equal-area rectangles it picks is unpinned;
 * tests/numpy_lir.py is the contract.  Six launches, one synchronisation at the end.  At most 2^31 - 2 pixels.
 * out_info (or NULL): {device ms of the launches} (HIP events). */
int stx_crop_lir(stx_ctx* ctx, const stx_buf* mask_u8x1, int out_xywh[4], int out_contours[2], double out_info[1]);
/* ---- feature detection: the project's OWN detector, not cv.ORB (FeatureDetector's "orb" / "sift" stay cv2's) ---------------------
 * Corner keypoints and 256-bit binary descriptors in the family of oriented FAST + rotated BRIEF, integer only: grey pyramid,
 * 9-of-16 segment-test score with 3 x 3 non-maximum suppression, a Harris-like integer response, the best quotas[l] corners of every
 * level by (response descending, y, x), orientation in 36 bins from the intensity centroid of a radius-15 disc, 256 comparisons of a
 * 5 x 5 binomial blur under the rotated pattern.  tests/numpy_features.py is the contract, byte for byte.
 * images: n u8x3 images of unequal sizes (read only; views allowed); masks: NULL, or n entries of which any may be NULL, else a u8x1
 * mask of its image's size (nonzero: keypoints allowed; never written).
 * The caller computes, in double precision as the contract states them, and hands in per image i: level_counts[i] <= nlevels kept
 * levels, their sizes level_wh[(i * STX_FEATURES_MAX_LEVELS + l) * 2] = {w, h} (level 0: the image's own; every side in 33 .. the
 * image's) and the quotas[i * STX_FEATURES_MAX_LEVELS + l] >= 0 (their sum at most nfeatures); once per process cxcy = {CX[36],
 * CY[36]} and patterns[36][256] = {px, py, qx, qy} (the rotated comparison pairs, every coordinate within +-13).
 * Results per image i, k = out_counts[i] <= nfeatures keypoints by level, then by that order: out_lxyb[(i * nfeatures + j) * 4] =
 * {level, x, y, bin}, out_R[i * nfeatures + j], out_desc[(i * nfeatures + j) * 32].  out_info (or NULL): {levels, candidates,
 * keypoints, 0} of the call.
 * The pyramid levels are stx_resize_linear_exact_batch's, one launch per level; the host waits once for the candidate counts.  The
 * candidate arena holds the most a level can produce (one per 2 x 2 cell of its interior): nothing is dropped, and the result does
 * not depend on scheduling.
 * Refused with STX_ERR_INVALID before anything is launched: an image side above STX_FEATURES_MAX_SIDE ((response, y, x) is one 64-bit
 * key), nlevels > STX_FEATURES_MAX_LEVELS, nfeatures > STX_FEATURES_MAX_FEATURES, a mask of another size, an image that is not u8x3. */
#define STX_FEATURES_MAX_SIDE 32767
#define STX_FEATURES_MAX_LEVELS 16
#define STX_FEATURES_MAX_FEATURES 65536
int stx_features_detect(stx_ctx* ctx, int n, const stx_buf* const* images, const stx_buf* const* masks, int nfeatures, int nlevels,
                        int fast_threshold, const int* level_counts, const int* level_wh, const int* quotas, const int* cxcy,
                        const signed char* patterns, int* out_counts, int* out_lxyb, long long* out_R, unsigned char* out_desc,
                        double out_info[4]);
/* ---- feature matching: the project's OWN matcher, not cv.detail.BestOf2NearestMatcher ("homography" / "affine" stay cv2's) ---------
 * Two-nearest-neighbour matching of 256-bit descriptors by Hamming distance with an integer ratio test (1024 d1 < ratio_T d2), the
 * union of both directions in OpenCV's order, and a homography RANSAC with a counter-based sampler and a division-free closed form in
 * IEEE fp64 without FMA.  tests/numpy_matches.py is the contract: every integer result and the bits of out_H.
 * Per image i (host memory, read only): desc[i], desc_shape[3 i] = {rows, columns, bytes per element} as the caller holds them, and
 * pts[i] = pts_rows[i] x {x, y} doubles, level-0 pixels relative to the image centre.  ratio_T = floor((1 - match_conf) 1024 + 0.5) in
 * 0 .. 1024; range_width < 0: every pair i < j, else those with j - i <= range_width; threshold_sq = ransac_threshold^2.
 * Results by pair ordinal k (the processed pairs i < j, row-major) with slot(k) = the sum of rows_i + rows_j over the pairs before it:
 * out_counts[k] = m matches; out_matches[3 (slot(k) + e)] = {query, train, distance} and out_mask[slot(k) + e] for e < m; out_pick[2 k]
 * = {inliers of the best hypothesis, its number, or 0 and -1 where m < 6}; out_H[9 k] = that hypothesis's H as computed (zeros where
 * m < 6).  The refit, the confidence and the mirrored entries are the caller's (float64 on the host).
 * out_info (or NULL): {pairs, matches, device ms of the four launches, device ms with the copies both ways} (HIP events).
 * One host wait, at the end.  Refused with STX_ERR_INVALID before anything is launched: more than STX_MATCH_MAX_FEATURES features in an
 * image, ransac_iters outside 1 .. STX_MATCH_MAX_ITERS, descriptors that are not rows x 32 of one byte, pts_rows[i] != rows. */
#define STX_MATCH_MAX_FEATURES 65536
#define STX_MATCH_MAX_ITERS 4096
int stx_match_features(stx_ctx* ctx, int n, const unsigned char* const* desc, const int* desc_shape, const double* const* pts,
                       const int* pts_rows, int ratio_T, int range_width, int ransac_iters, double threshold_sq, unsigned seed,
                       int* out_counts, int* out_matches, unsigned char* out_mask, int* out_pick, double* out_H, double out_info[4]);
/* stx_match_features with the geometric model of the RANSAC chosen: STX_MATCH_MODEL_HOMOGRAPHY is stx_match_features bit for bit (which
 * forwards here with it).  The affine models are for scans and flat tiles; pts are then level-0 pixels that are NOT centred, the frame
 * the affine warper applies a camera's R in.  _AFFINE_PARTIAL: a similarity (4 degrees of freedom) of 2 sampled matches; _AFFINE_FULL:
 * an affine map (6) of 3.  The sampler is the homography's restricted to the first 2 or 3 draws; the closed forms are division free
 * and homogeneous, out_H[9 k] = {h0 .. h5, +0.0, +0.0, h8} with h8 > 0 after the sign rule (h8 == 0, coincident or collinear sample
 * points: no inliers); inliers, best hypothesis and mask as for the homography.  tests/numpy_affine.py is the contract (DESIGN.md
 * section 18).  A model outside the three is refused with STX_ERR_INVALID before anything is launched. */
#define STX_MATCH_MODEL_HOMOGRAPHY 0
#define STX_MATCH_MODEL_AFFINE_PARTIAL 1
#define STX_MATCH_MODEL_AFFINE_FULL 2
int stx_match_features_model(stx_ctx* ctx, int n, const unsigned char* const* desc, const int* desc_shape, const double* const* pts,
                             const int* pts_rows, int ratio_T, int range_width, int ransac_iters, double threshold_sq, unsigned seed,
                             int model, int* out_counts, int* out_matches, unsigned char* out_mask, int* out_pick, double* out_H,
                             double out_info[4]);
/* ---- ray bundle adjustment: the project's OWN solver, not cv.detail.BundleAdjusterRay ("ray" stays cv2's) ----------------------------
 * The normal equations of CameraSolver's Levenberg-Marquardt steps.  An edge is a pair of cameras i < j with its inlier matches
 * (x, y) in image i and (u, v) in image j, level-0 pixels relative to the image centre.  A camera has 9 variants of 10 doubles
 * {f', H' = Rodrigues(r') diag(1 / f', 1 / f', 1) row-major}: its parameters, then + and - 1e-3 on each of the four (made by the caller).
 * Per match the residual sqrt(f_i' f_j') (ray_i - ray_j) of the unit rays H' (x, y, 1) / |.| and its 3 x 8 Jacobian by central
 * differences over the variants; per edge E = sum r.r, g[8] = sum J^T r and the upper triangle B[36] of sum J^T J, row-major.
 * tests/numpy_cameras.py is the contract, in the bits of all 45 sums: IEEE fp64 without FMA, 256 lanes that stride over the matches,
 * folded by v[l] += v[l + s] for s = 128 .. 1.
 * stx_ray_problem_create uploads the edges once: edge_cams[2 e] = {i, j}, offsets[n_edges + 1] ascending from 0, pts[4 offsets[n_edges]].
 * stx_ray_problem_eval: variants[n_cams * 90] -> out[45 e] = {E, g, B}; one launch, one host wait.  An edge without matches gives 45
 * zeros.  out_info (or NULL): {edges, matches, device ms of the launch, device ms with the copies both ways} (HIP events).
 * Refused with STX_ERR_INVALID before anything is allocated or launched: a camera index outside 0 .. STX_RAY_MAX_CAMERAS - 1 or more
 * than STX_RAY_MAX_CAMERAS cameras, an edge with i >= j, offsets that do not ascend, more than STX_RAY_MAX_MATCHES matches on an edge,
 * fewer cameras than the edges name, a variant that is not finite.  Free the problem before its context. */
#define STX_RAY_MAX_CAMERAS 1024
#define STX_RAY_MAX_MATCHES 131072 /* 2 x STX_MATCH_MAX_FEATURES: the union of both directions */
typedef struct stx_ray_problem stx_ray_problem;
int stx_ray_problem_create(stx_ctx* ctx, int n_edges, const int* edge_cams, const long long* offsets, const double* pts,
                           stx_ray_problem** out);
int stx_ray_problem_eval(stx_ray_problem* problem, int n_cams, const double* variants, double* out, double out_info[4]);
/* The normal equations of CameraSolver's affine-partial adjustment (model="affine"), on a problem made by stx_ray_problem_create from
 * points that are NOT centred.  A camera is the similarity T = [[a, -b, tx], [b, a, ty], [0, 0, 1]] from its image to the panorama
 * plane; it has 9 variants of 8 doubles {a, b, tx, ty, a', b', tx', ty'}, the map and its inverse: its parameters, then + and - 1e-3
 * on each of the four (made by the caller).  Per match P = T_i (x, y), Q = T_j^-1 P, the residual (u, v) - Q in image j's pixels and
 * its 2 x 8 Jacobian by central differences over the variants; per edge the same 45 sums in the same order of summation as
 * stx_ray_problem_eval.  Multiplies, adds and subtractions only.  tests/numpy_affine.py is the contract, in the bits of all 45 sums
 * (DESIGN.md section 18).  variants[n_cams * 72] -> out[45 e]; out_info and the refusals as stx_ray_problem_eval's. */
int stx_affine_problem_eval(stx_ray_problem* problem, int n_cams, const double* variants, double* out, double out_info[4]);
/* The normal equations of CameraSolver's reprojection adjustment (model="reproj"; the project's own, not cv.detail.BundleAdjusterReproj),
 * on a problem made by stx_ray_problem_create from centred points.  A camera has 7 parameters — focal f, the principal point's offset
 * (cx, cy) from the image centre, the aspect a, a Rodrigues vector — and 15 variants of 18 doubles {P = R K^-1, Q = K R^T, row-major},
 * K = [[f, 0, cx], [0, f a, cy], [0, 0, 1]]: its parameters, then + and - 1e-3 on each of the seven (made by the caller).  Per match
 * X = P_i (x, y, 1), Y = Q_j X, the residual (u - Y0 / Y2, v - Y1 / Y2) in image j's pixels (IEEE divide, no case of its own for
 * Y2 <= 0) and its 2 x 14 Jacobian by central differences over the variants; per edge E = sum r.r, g[14] = sum J^T r and the upper
 * triangle B[105] of sum J^T J, row-major, in the same order of summation as stx_ray_problem_eval.  tests/numpy_reproj.py is the
 * contract, in the bits of all 120 sums.  variants[n_cams * 270] -> out[120 e]; an edge without matches gives
 * 120 zeros; out_info and the refusals as stx_ray_problem_eval's. */
int stx_reproj_problem_eval(stx_ray_problem* problem, int n_cams, const double* variants, double* out, double out_info[4]);
int stx_ray_problem_free(stx_ray_problem* problem);
/* stx_resize_linear_exact <- stitching/images.py:122-124 cv.resize(img, size, interpolation=cv.INTER_LINEAR_EXACT) (u8x1 / u8x3:
 *                            the final-resolution resize of Images.resize, next row N3)
 * stx_seam_mask_resize    <- stitching/seam_finder.py:37-43 SeamFinder.resize: cv.dilate(seam_mask, None), cv.resize(...,
 *                            INTER_LINEAR_EXACT) to the size of the final warped mask, cv.bitwise_and with it (next row N2);
 *                            one fused kernel, the result is what Blender.feed receives (stitching/stitcher.py:124,127) */
int stx_resize_linear_exact(stx_ctx* ctx, const stx_buf* src_u8, int dst_w, int dst_h, stx_buf** out);
int stx_seam_mask_resize(stx_ctx* ctx, const stx_buf* seam_mask_u8x1, const stx_buf* final_mask_u8x1, stx_buf** out);
/* stx_resize_linear_exact for n images of unequal sizes (u8x1 and u8x3 mixed, views included) in one launch: the generator loop of
 * Images.resize (stitching/images.py:72-77, stitching/stitcher.py:167-168).  dst_wh = {w, h} per image; outs[i] is byte for byte what
 * stx_resize_linear_exact(srcs[i], w, h) returns.  n <= 0 is STX_ERR_INVALID; a failing call hands nothing out. */
/* Conservative shrink of source validity masks (u8x1) to the lower resolutions of a pipeline, one launch for the list.  Pixel (x, y) of
 * the dw x dh result is 255 iff EVERY source pixel in columns [x sw / dw, ((x + 1) sw + dw - 1) / dw) and the rows likewise (integer
 * divisions) is non-zero, else 0; dw == sw binarises.  Refused (STX_ERR_INVALID, nothing allocated): dw > sw or dh > sh, zero sizes,
 * inputs that are not u8x1, masks of another context.  The results are binary (stx_buf_flags). */
int stx_mask_shrink_batch(stx_ctx* ctx, int n, const stx_buf* const* masks_u8x1, const int* dst_wh, stx_buf** outs);
int stx_resize_linear_exact_batch(stx_ctx* ctx, int n, const stx_buf* const* srcs_u8, const int* dst_wh, stx_buf** outs);
/* the same for all n images of a panorama (the generator loop stitching/stitcher.py:223-225): one table upload, one dilate
 * and one resize launch per 16 images */
int stx_seam_mask_resize_batch(stx_ctx* ctx, int n, const stx_buf* const* seam_masks, const stx_buf* const* final_masks,
                               stx_buf** outs);
/* the same for rectangles of the final masks: final_masks[i] is the w x h rectangle at (x0, y0) of image i's warped mask of
 * size full_w x full_h; full_wh_xy0 = {full_w, full_h, x0, y0} per image (x0 a multiple of 4).  Output i equals that
 * rectangle of stx_seam_mask_resize_batch's output for the whole mask. */
int stx_seam_mask_resize_batch_sub(stx_ctx* ctx, int n, const stx_buf* const* seam_masks, const stx_buf* const* final_masks,
                                   const int* full_wh_xy0, stx_buf** outs);
int stx_timelapse_frame(stx_ctx* ctx, const stx_buf* img, int tlx, int tly, const int dst_roi_xywh[4], stx_buf** out_frame);

/* ---- device frame ingest: foreign device memory -> images of the library's own ----------------------------
 * No counterpart in the reference (its frames are host arrays).  A frame that was born on the device — a decoder's NV12 surface, an
 * upstream stage's RGB / BGRA, another framework's array — is COPIED or converted into a new image: the kernels rely on
 * STX_BUF_FRONT_PAD readable bytes in front of every image the library allocates, which foreign memory does not promise, so a foreign
 * pointer never becomes a stx_buf.  tests/numpy_ingest.py is the contract, byte for byte.
 *
 * format: STX_INGEST_RAW copies h rows of w * channels elements of `elem` (any image layout the library has, 1 .. 4 channels); the
 * others are u8: BGR / GRAY copy, RGB reverses the channels, BGRA / RGBA drop alpha (RGBA reverses as well), NV12 (plane[0] = Y: h x w,
 * plane[1] = interleaved U, V: ceil(h/2) rows of ceil(w/2) pairs) and I420 (plane[1] = U, plane[2] = V, ceil(h/2) x ceil(w/2) each) become
 * u8x3 BGR.  Pixel (x, y) takes the chroma sample (x >> 1, y >> 1); with C = Y - 16 (limited range) or Y (full), D = U - 128,
 * E = V - 128 and the 8-bit-fraction constants of `matrix` / `range`, in int32 with an arithmetic shift,
 *   R = clip8((yk C + rv E + 128) >> 8), G = clip8((yk C - gu D - gv E + 128) >> 8), B = clip8((yk C + bu D + 128) >> 8).
 * channels / elem describe plane[0]: 3 u8 for BGR / RGB, 4 u8 for BGRA / RGBA, 1 u8 for GRAY / NV12 / I420.  pitch: bytes per row.
 *
 * One call takes n frames of unequal sizes and formats and makes ONE launch.  Everything is checked before anything is allocated or
 * launched (STX_ERR_INVALID, the context stays usable): every plane must be device memory of the context's device
 * (hipPointerGetAttributes: host, pinned host, managed and other-device memory are refused) and lie, first byte to last, inside one
 * allocation (hipMemGetAddressRange); pitch >= row bytes; format agrees with channels / elem; 1 <= w, h <= STX_INGEST_MAX_SIDE.
 * has_stream != 0: the conversion is ordered after everything queued on producer_stream so far (an event recorded there, waited for by
 * the context's stream: no host wait; 1 as a handle means the legacy default stream — the null stream —, 2 the per-thread default stream); 0: the caller vouches that the
 * source is complete.  The call only queues work: the source must stay untouched until the context's stream has passed it
 * (stx_ctx_sync).  The results carry no "mask holds only 0 / 255" flag: nothing is known about a foreign mask. */
#define STX_INGEST_RAW 0
#define STX_INGEST_BGR 1
#define STX_INGEST_RGB 2
#define STX_INGEST_BGRA 3
#define STX_INGEST_RGBA 4
#define STX_INGEST_GRAY 5
#define STX_INGEST_NV12 6
#define STX_INGEST_I420 7
#define STX_INGEST_BT601 0
#define STX_INGEST_BT709 1
#define STX_INGEST_LIMITED 0
#define STX_INGEST_FULL 1
#define STX_INGEST_MAX_SIDE 32768
/* one foreign frame: up to three planes of device memory, pitches in bytes */
typedef struct { const void* plane[3]; long long pitch[3]; int w, h, channels, elem, format; } stx_foreign_frame;
int stx_ingest(stx_ctx* ctx, int n, const stx_foreign_frame* frames, int matrix, int range, void* producer_stream, int has_stream,
               stx_buf** out);

/* ---- device frame emit: images of the library's own -> NV12 / I420 / RGBA ... in the caller's surfaces ------
 * The mirror of stx_ingest, and like it without a counterpart in the reference.  tests/numpy_emit.py is the contract, byte for byte.
 *
 * An item is a source image `src` (a crop view included), a format (the STX_INGEST_* codes) and, optionally, an alpha image and a
 * target.  STX_INGEST_RAW copies any image layout; the others take u8: BGR / GRAY copy (u8x3 / u8x1), RGB reverses the channels,
 * BGRA / RGBA add a fourth byte — 255, or the byte of `alpha`, a u8x1 image of the source's size (the panorama mask) —, NV12
 * (plane[0] = Y: h x w, plane[1] = interleaved U, V: ceil(h/2) rows of ceil(w/2) pairs) and I420 (plane[1] = U, plane[2] = V) are made
 * from u8x3 BGR with the 16-bit-fraction constants of `matrix` / `range`, in int32 with an arithmetic shift:
 *   Y = clip8(((kyb B + kyg G + kyr R + 32768) >> 16) + yoff) per pixel,
 *   U = clip8(((kub SB + kug SG + kur SR + 131072) >> 18) + 128) per 2 x 2 block from the block's channel sums (coordinates clamped to
 *   the image: an odd last column or row is replicated), V likewise.
 *
 * has_target != 0: plane[] / pitch[] (bytes) name the caller's memory, written in place, and the item's three slots of `out` stay null.
 * has_target == 0: the planes are allocated and returned in out[3 i ..]: one image for the packed formats, Y (u8x1) and UV (u8x2) for
 * NV12, Y, U, V (u8x1) for I420; unused slots are null.  `out` holds 3 n slots.
 *
 * One call takes n items of unequal sizes and formats and makes ONE launch.  Everything is checked before anything is allocated or
 * launched (STX_ERR_INVALID with a message that names item and plane; the context stays usable): the source's layout agrees with the
 * format; alpha is u8x1 of the source's size and only given with BGRA / RGBA; 1 <= w, h <= STX_INGEST_MAX_SIDE; every target plane is
 * device memory of the context's device (host, pinned host, managed and other-device memory are refused) and lies, first byte to last,
 * inside one allocation; row bytes <= pitch <= 2^40; no target plane's byte range overlaps another target plane of the call, or any
 * source or alpha image of the call.  No byte outside the rows of a target plane is written.
 * has_stream != 0: the launch is ordered after everything queued on consumer_stream so far (the consumer may still be reading the
 * surface) and consumer_stream is ordered after the launch, both by events, without a host wait; 1 as a handle means the legacy
 * default stream, 2 the per-thread default stream.  0: the caller vouches that the targets are free, and syncs the context
 * (stx_ctx_sync) before it reads them. */
typedef struct {
    const stx_buf* src;
    const stx_buf* alpha; /* or null */
    int format, has_target;
    void* plane[3];
    long long pitch[3];
} stx_emit_item;
int stx_emit(stx_ctx* ctx, int n, const stx_emit_item* items, int matrix, int range, void* consumer_stream, int has_stream, stx_buf** out);

/* ---- lens rectification: distorted frames -> pinhole frames -------------------------------------------------
 * No counterpart in the reference (it assumes pinhole cameras; a caller of it runs cv2.remap on the host).  tests/numpy_rectify.py is
 * the contract, byte for byte; the device half of it is integer only.
 *
 * A lens map belongs to one camera: for a destination image dst_w x dst_h it holds, every STX_LENS_CELL destination pixels, the source
 * coordinate (sx, sy) of that pixel in Q6 (int32, |value| <= 2^21) — nx = (dst_w + 15) / 16 + 1 nodes per row, ny = (dst_h + 15) / 16 + 1
 * rows, node (i, j) at destination pixel (16 i, 16 j), the nodes past the right and bottom edge included; nodes_xy_q6 is ny x nx x 2.
 * stx_lens_map_create copies the nodes to device memory once and returns when the caller's array is free again.
 *
 * Destination pixel (x, y), ax = x & 15, ay = y & 15, nodes N00 N10 / N01 N11 of its cell, per coordinate, in int32:
 *   S = (16 - ay) ((16 - ax) N00 + ax N10) + ay ((16 - ax) N01 + ax N11);  q = (S + 256) >> 9 (arithmetic: Q5, floor);  i = q >> 5, f = q & 31
 *   out = (w00 p00 + w10 p10 + w01 p01 + w11 p11 + 512) >> 10 per channel, w00 = (32 - fx)(32 - fy), w10 = fx (32 - fy), ...
 * over the taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1).  A tap outside the source reads 0 (STX_RECTIFY_CONSTANT) or has
 * its indices clamped (STX_RECTIFY_REPLICATE).  The mask is 255 where all four taps lie inside the source, else 0.
 *
 * stx_rectify takes n sources (u8, 1 or 3 channels, crop views included) of unequal sizes with one map each and makes ONE launch.
 * out_imgs[i] is a new dst_w x dst_h image with the source's channels; with want_masks != 0 out_masks[i] is a new u8x1 mask (flagged as
 * holding only 0 and 255), else out_masks may be null.  Everything is checked before anything is allocated or launched
 * (STX_ERR_INVALID, the context stays usable): null handles, element type and channels, source size against the map's, sides in
 * 1 .. STX_RECTIFY_MAX_SIDE, the node counts against (dst_w, dst_h), node values within +- 2^21, a map of another context, a source that spans 2^31 bytes or has a pitch of 2^24 (a view of a very wide parent). */
#define STX_LENS_CELL 16
#define STX_RECTIFY_CONSTANT 0
#define STX_RECTIFY_REPLICATE 1
#define STX_RECTIFY_MAX_SIDE 16384
typedef struct stx_lens_map stx_lens_map;
int stx_lens_map_create(stx_ctx* ctx, int dst_w, int dst_h, int src_w, int src_h, int nx, int ny, const int* nodes_xy_q6, stx_lens_map** out);
int stx_lens_map_free(stx_lens_map* map);
int stx_rectify(stx_ctx* ctx, int n, const stx_buf* const* srcs, const stx_lens_map* const* maps, int border, int want_masks,
                stx_buf** out_imgs, stx_buf** out_masks);

/* ---- the warp through the lens: distorted frames -> warped images in ONE resampling ---------------------------
 * stx_rectify followed by stx_warp_batch resamples every frame twice.  stx_warp_lens_batch keeps the warp's own fp32 backward map — for
 * all 16 warper types, bit for bit what stx_warp_batch computes — and puts another sampler behind it: the map's 1/32-px position in the
 * RECTIFIED (pinhole) frame goes through the camera's lens map and four taps of the DISTORTED frame are blended.  tests/numpy_lens_warp.py
 * is the contract, byte for byte.  Per destination pixel with map value (x, y), integer only after the first step:
 *   sx = cvRound(32 x), sy = cvRound(32 y) (as remap; NaN and anything outside int32: INT_MIN);
 *   qx = clip(sx, 0, 32 (W - 1)), qy = clip(sy, 0, 32 (H - 1)), W x H the map's dst_w x dst_h: a replicate border in the pinhole frame;
 *   cell (qx >> 9, qy >> 9), nodes N00 N10 / N01 N11, ax = qx & 511, ay = qy & 511, per coordinate in int32:
 *     L0 = ((512 - ax) N00 + ax N10 + 256) >> 9, L1 likewise from N01, N11 (Q6);  q = ((512 - ay) L0 + ay L1 + 512) >> 10 (Q5, floor);
 *   i = q >> 5, f = q & 31; the taps (ix, iy) .. (ix + 1, iy + 1) at indices CLAMPED into the source, always;
 *   out = (w00 p00 + w10 p10 + w01 p01 + w11 p11 + 512) >> 10 per channel, the weights of stx_rectify.
 * |q / 32 - B| <= 1/32 px, B the exact bilinear interpolation of the unrounded node coordinates at (qx / 32, qy / 32).  With an identity
 * lens map the result is stx_warp_batch's image wherever that one's taps are not reflected ones.
 *
 * K, R and the rectangles belong to the rectified frame (the map's dst_w x dst_h); srcs[i] is the map's src_w x src_h distorted frame
 * (u8x3, crop views included).  Images only: warped masks do not depend on pixel values, stx_warp_batch (out_imgs null) over the
 * rectified sizes makes them.  rects_xywh null: the ROIs of stx_warp_rois over the rectified sizes; out_xywh (or null) receives the
 * rectangles used.  tables (or null) as in stx_warp_batch: a kept handle means no table kernel on later calls of the same rig; the
 * per-pixel projector families leave it empty.  More images than one launch takes go in groups.  The trig mode is honoured (it acts on
 * the map only).  Refused with STX_ERR_INVALID before anything is allocated or launched, the context stays usable: null handles, a
 * source that is not u8x3 or whose size is not the map's source size, a map, buffer or tables handle of another context, a source that
 * spans 2^31 bytes or has a pitch of 2^24, a rectangle with a non-positive side, a remap mode other than STX_REMAP_Q15 (the sampler has
 * one arithmetic). */
int stx_warp_lens_batch(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s, const stx_buf* const* srcs,
                        const stx_lens_map* const* maps, const int* rects_xywh, stx_buf** out_imgs, int* out_xywh, stx_warp_tables** tables);

/* ---- sharded multi-band blending: one process per GPU, one stx_blender per rank ------------------
 * No counterpart in the reference (it is single process, stitching/stitcher.py:247-254).  Every rank
 * prepares the same roi; rank g produces the columns [x0, x1) of the panorama (stx_blend_set_band).
 * An image fed on rank o whose 2^bands-aligned feed rectangle reaches another rank's columns is
 * exported there as a CONTRIBUTION: per pyramid level the products (short)(L*W) and the weights W
 * over a strip (stx_blend_export_contrib -> RCCL send/recv -> stx_blend_feed_contrib_ex).  Integer sums
 * are order independent and `order` (the global feed index) fixes the fp32 weight-sum order, so the
 * assembled panorama is bit-identical to the single-GPU result.  DESIGN.md §6. */
int stx_blend_set_band(stx_blender* b, int x0, int x1);
int stx_blend_feed_ex(stx_blender* b, const stx_buf* img, const stx_buf* mask, int tlx, int tly, int order);
/* strip rect (relative to the roi origin, level 0) and packed size of the contribution that an image
 * of size (img_w, img_h) at corner (tlx, tly) owes to the owner of columns [band_x0, band_x1);
 * w = 0 when it owes nothing.  Pure geometry: sender and receiver compute the same answer. */
int stx_blend_contrib_rect(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int band_x0, int band_x1,
                           int out_rect_xywh[4], size_t* out_bytes);
int stx_blend_export_contrib(stx_blender* b, int order, int band_x0, int band_x1, stx_buf** out_packed,
                             int out_rect_xywh[4]);
/* all the strips a rank owes in one call (n images / destination bands): same results, one kernel launch per kernel
 * instantiation instead of one per strip and level; out_packed[n], out_rects_xywh[4 n] */
int stx_blend_export_contribs(stx_blender* b, int n, const int* orders, const int* band_x0s, const int* band_x1s,
                              stx_buf** out_packed, int* out_rects_xywh);
/* build the pyramids of every image fed so far now (they are otherwise built at the first export / blend()):
 * a sharded rank calls it for its interior images while its strips are still in flight */
int stx_blend_build(stx_blender* b);
/* flags travel with a strip over the caller's control plane.  STX_CONTRIB_U8_BINARY: the strip was exported from
 * a u8 image whose mask holds only 0 / 255 (then its products are L or 0 and its weights 0.f or 1.f, and the
 * receiver may keep the packed 16-bit level-0 kernel).  stx_buf_flags reads it off an exported strip (or a mask:
 * the same bit says "only 0 / 255"). */
#define STX_CONTRIB_U8_BINARY 1
/* STX_STRIP_MASK_BITS (strips only): the mask rows of the flat buffer hold one bit per pixel instead of a byte (a 0 / 255 mask:
 * 3.125 instead of 4 bytes per pixel on the link); stx_strip_unpack / stx_blend_feed_strips expand them into a mask buffer. */
#define STX_STRIP_MASK_BITS 2
int stx_blend_feed_contrib_ex(stx_blender* b, int order, const int rect_xywh[4], const stx_buf* packed, int flags);
int stx_buf_flags(const stx_buf* buf, int* out_flags);

/* Rectangle {x0, x1, y0, y1} of an image that the panorama rectangle [band_x0, band_x1) x [band_y0, band_y1) (roi-relative)
 * depends on through the pyramids: stx_strip_rect's column range and the same range along y.  A pipeline that knows where an
 * image's fed mask is non-zero (its seam cell) needs no more of the image than this; all zeros: nothing. */
int stx_view_rect(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int band_x0, int band_x1, int band_y0, int band_y1,
                  int out_x0x1y0y1[4]);
/* image-strip form of the same exchange: the owner of an image ships the COLUMNS [x0, x1) of the warped
 * image and mask that another band depends on (4 bytes per pixel, no export pass) and the receiver feeds them with
 * stx_blend_feed_ex like an image of its own, at corner (tlx + x0, tly) and with the image's global `order`; its band
 * comes out bit-identical.  stx_strip_rect: pure geometry (x0 == x1: nothing owed), columns relative to the image;
 * stx_strip_pack: image rows then mask rows in one flat buffer (two 2-D device copies on the context stream);
 * stx_strip_unpack: the two views of a received flat buffer (flags: STX_CONTRIB_U8_BINARY when the mask is 0 / 255). */
int stx_strip_rect(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int band_x0, int band_x1, int out_x0x1[2],
                   size_t* out_bytes);
int stx_strip_pack(stx_ctx* ctx, const stx_buf* img, const stx_buf* mask, int x0, int x1, stx_buf** out_packed);
/* all strips a rank owes in one call (one copy kernel per 16 strips); x0 multiples of 8, whole image buffers (no views); flags: 0 or
 * STX_STRIP_MASK_BITS; stx_strip_bytes: size of the flat buffer of a w x h strip under these flags */
int stx_strip_pack_batch_ex(stx_ctx* ctx, int n, const stx_buf* const* imgs, const stx_buf* const* masks, const int* x0s, const int* x1s,
                            int flags, stx_buf** out_packed);
int stx_strip_bytes(int w, int h, int flags, size_t* out_bytes);
/* all received strips in one call: unpack + stx_blend_feed_ex(strip i at (tlxs[i], tlys[i]), orders[i]) */
int stx_blend_feed_strips(stx_blender* b, int n, const stx_buf* const* packed, const int* ws, const int* hs, const int* tlxs,
                          const int* tlys, const int* orders, int flags);
int stx_strip_unpack(const stx_buf* packed, int w, int h, int flags, stx_buf** out_img, stx_buf** out_mask);

/* ---- RCCL strip exchange over xGMI ---------------------------------------------------------------
 * One communicator per rank (one process per GPU).  An exchange issues every send / receive of one step as a
 * single RCCL group: it is ordered after the kernels that filled the send buffers and before the kernels that
 * read the receive buffers.  The unique id (128 bytes, from rank 0) travels over the caller's control plane. */
typedef struct stx_comm stx_comm;
int stx_comm_unique_id(unsigned char out[128]);
int stx_comm_create(stx_ctx* ctx, int nranks, int rank, const unsigned char id[128], stx_comm** out);
/* _begin_on issues the group on the communicator's own stream, ordered after everything queued so far on the stream
 * of context `on`; kernels queued on that stream between _begin_on and _end_on (warps and pyramids of images that
 * send nothing) overlap with the transfer; _end_on orders the context stream after the transfer.  The buffers must
 * stay alive until _end_on has been called.  `on`: the communicator's own context or another one of the same device:
 * one communicator serves several panoramas in flight on different streams; their exchanges are serialised on the
 * communicator's stream */
int stx_comm_exchange_begin_on(stx_comm* comm, stx_ctx* on, int n_ops, const int* peers, const int* is_send,
                               void* const* dev_ptrs, const size_t* bytes);
int stx_comm_exchange_end_on(stx_comm* comm, stx_ctx* on);
/* what librccl itself reports: {ncclCommCount, ncclCommUserRank, ncclGetVersion, device}; -1 where the loaded library lacks the call */
int stx_comm_info(const stx_comm* comm, int out_info[4]);
int stx_comm_destroy(stx_comm* comm);

/* ---- measurement hooks (bench.py) -----------------------------------------------------
 * When enabled, every kernel launch on the ctx stream is bracketed by HIP events recorded
 * on that stream; stx_prof_get reports per-kernel call count, summed duration and the
 * algorithmic bytes the launch sites declared. */
int stx_prof_enable(stx_ctx* ctx, int on);
int stx_prof_reset(stx_ctx* ctx);
int stx_prof_count(stx_ctx* ctx, int* out_n);
int stx_prof_get(stx_ctx* ctx, int index, char* name, int name_cap, int64_t* calls, double* total_ms,
                 double* algo_bytes);
/* elapsed device time between two marks recorded on the ctx stream */
int stx_mark(stx_ctx* ctx, int slot);
int stx_mark_elapsed_ms(stx_ctx* ctx, int slot_begin, int slot_end, double* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* STITCHING_AMD_H */
