// stx_resize_host.cpp — host side of cv::resize(INTER_LINEAR_EXACT) of images and seam masks.  Kernels: stx_resize.hip.  Compiled with
// -ffp-contract=off: the coefficient tables restate OpenCV's baseline (non-FMA) evaluation order.
#include <algorithm>
#include <cmath>

#include "stx_internal.h"

// interpolationLinear<ufixedpoint16>::getCoeffs of cv::resize(INTER_LINEAR_EXACT) [OCV-MEM]: all in double precision
// (softdouble upstream = IEEE double; this file is compiled with -ffp-contract=off)
static void linear_exact_table(int src_n, int dst_n, std::vector<int>& t)
{
    t.resize(2 * (size_t)dst_n);
    const double inv_scale = (double)dst_n / (double)src_n;
    const double scale = 1.0 / inv_scale;
    for (int v = 0; v < dst_n; v++) {
        const double fval = scale * ((double)v + 0.5) - 0.5;
        const int ival = (int)std::floor(fval);
        int ofs = 0, c1 = 0, interior = 0;
        if (ival >= 0 && src_n > 1) {
            if (ival < src_n - 1) { ofs = ival; c1 = (int)std::nearbyint((fval - (double)ival) * 256.0); interior = 1; }
            else ofs = src_n - 1;
        }
        t[2 * (size_t)v] = ofs;
        t[2 * (size_t)v + 1] = c1 | (interior << 16);
    }
}

static int resize_impl(stx_ctx* ctx, const stx_buf* src, int dw, int dh, bool dilate, const stx_buf* andmask, stx_buf** out)
{
    if (src->elem != STX_U8 || (src->c != 1 && src->c != 3)) return stx_fail(STX_ERR_UNSUPPORTED, "resize needs a u8x1 or u8x3 image");
    if (dw <= 0 || dh <= 0) return stx_fail(STX_ERR_INVALID, "resize to %dx%d", dw, dh);
    if (src->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "image lives on another device");
    std::vector<int> xt, yt;
    linear_exact_table(src->w, dw, xt);
    linear_exact_table(src->h, dh, yt);
    const size_t nx = xt.size();
    xt.resize((nx + 7) & ~(size_t)7, 0);  // entries in whole groups of 4 columns (the 4-pixel seam kernel reads 4 at once), 32-byte rows
    std::vector<int> both(xt);
    both.insert(both.end(), yt.begin(), yt.end());
    StxDevBlock d_tab;
    STX_TRY(upload_small(ctx, both.data(), both.size() * sizeof(int), &d_tab));
    StxBufRef dst;
    STX_TRY(stx_buf_new(ctx, dw, dh, src->c, STX_U8, &dst));
    STX_TRY(stx_launch_resize_exact(ctx, src, dst.get(), (const int*)d_tab.get(), (const int*)d_tab.get() + xt.size(), dilate, andmask));
    *out = dst.release();
    return STX_OK;
}

STX_EXPORT int stx_resize_linear_exact(stx_ctx* ctx, const stx_buf* src, int dst_w, int dst_h, stx_buf** out)
{
    if (!ctx || !src || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    return resize_impl(ctx, src, dst_w, dst_h, false, nullptr, out);
}

// Images.resize for a list of images: one descriptor upload through the pinned ring, one launch.  Everything is checked before anything
// is allocated or launched; a failing call hands nothing out.
STX_EXPORT int stx_resize_linear_exact_batch(stx_ctx* ctx, int n, const stx_buf* const* srcs, const int* dst_wh, stx_buf** outs)
{
    if (!ctx || !srcs || !dst_wh || !outs) return stx_fail(STX_ERR_INVALID, "null argument");
    if (n <= 0) return stx_fail(STX_ERR_INVALID, "resize of %d images", n);
    STX_TRY(stx_set_device(ctx));
    std::vector<StxResizeItem> items((size_t)n);
    long long tiles = 0;
    double bytes = 0.0;
    for (int i = 0; i < n; i++) {
        const stx_buf* src = srcs[i];
        if (!src) return stx_fail(STX_ERR_INVALID, "null argument");
        const int dw = dst_wh[2 * i], dh = dst_wh[2 * i + 1];
        if (src->elem != STX_U8 || (src->c != 1 && src->c != 3)) return stx_fail(STX_ERR_UNSUPPORTED, "resize needs a u8x1 or u8x3 image");
        if (dw <= 0 || dh <= 0) return stx_fail(STX_ERR_INVALID, "resize to %dx%d", dw, dh);
        if (src->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "image lives on another device");
        StxResizeItem& K = items[i];
        K = StxResizeItem{};
        K.src = src->ptr; K.sstride = (long long)src->stride; K.sw = src->w; K.sh = src->h; K.dw = dw; K.dh = dh; K.c = src->c;
        K.xscale = 1.0 / ((double)dw / (double)src->w); K.yscale = 1.0 / ((double)dh / (double)src->h);
        K.tiles_x = (dw + STX_RESIZE_TW - 1) / STX_RESIZE_TW;
        K.tile0 = (int)tiles;
        tiles += (long long)K.tiles_x * ((dh + STX_RESIZE_TH - 1) / STX_RESIZE_TH);
        if (tiles > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "resize batch of more than 2^31 destination tiles");
        bytes += (double)dw * dh * src->c * 5.0;  // four taps and the result
    }
    std::vector<StxBufRef> dsts((size_t)n);
    for (int i = 0; i < n; i++) {
        STX_TRY(stx_buf_new(ctx, items[i].dw, items[i].dh, items[i].c, STX_U8, &dsts[i]));
        items[i].dst = dsts[i]->ptr; items[i].dstride = (long long)dsts[i]->stride;
    }
    StxDevBlock d_items;
    STX_TRY(upload_small(ctx, items.data(), items.size() * sizeof(StxResizeItem), &d_items));
    STX_TRY(stx_launch_resize_exact_batch(ctx, (const StxResizeItem*)d_items.get(), n, (int)tiles, bytes));
    for (int i = 0; i < n; i++) outs[i] = dsts[i].release();
    return STX_OK;  // the descriptor block goes back here: stream-ordered reuse
}

// Source validity masks at the lower resolutions of a pipeline: one launch for the list, everything checked before anything is allocated
STX_EXPORT int stx_mask_shrink_batch(stx_ctx* ctx, int n, const stx_buf* const* masks, const int* dst_wh, stx_buf** outs)
{
    if (!ctx || !masks || !dst_wh || !outs) return stx_fail(STX_ERR_INVALID, "null argument");
    if (n <= 0) return stx_fail(STX_ERR_INVALID, "shrink of %d masks", n);
    STX_TRY(stx_set_device(ctx));
    std::vector<StxResizeItem> items((size_t)n);
    long long tiles = 0;
    double bytes = 0.0;
    for (int i = 0; i < n; i++) {
        const stx_buf* m = masks[i];
        if (!m) return stx_fail(STX_ERR_INVALID, "null argument");
        const int dw = dst_wh[2 * i], dh = dst_wh[2 * i + 1];
        if (m->elem != STX_U8 || m->c != 1) return stx_fail(STX_ERR_INVALID, "mask %d is not u8x1", i);
        if (m->ctx != ctx) return stx_fail(STX_ERR_INVALID, "mask %d belongs to another context", i);
        if (dw <= 0 || dh <= 0) return stx_fail(STX_ERR_INVALID, "mask %d: shrink to %dx%d", i, dw, dh);
        if (dw > m->w || dh > m->h) return stx_fail(STX_ERR_INVALID, "mask %d: %dx%d is larger than the mask's %dx%d (a shrink only)", i, dw, dh, m->w, m->h);
        StxResizeItem& K = items[i];
        K = StxResizeItem{};
        K.src = m->ptr; K.sstride = (long long)m->stride; K.sw = m->w; K.sh = m->h; K.dw = dw; K.dh = dh; K.c = 1;
        K.tiles_x = (dw + STX_RESIZE_TW - 1) / STX_RESIZE_TW;
        K.tile0 = (int)tiles;
        tiles += (long long)K.tiles_x * ((dh + STX_RESIZE_TH - 1) / STX_RESIZE_TH);
        if (tiles > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "shrink batch of more than 2^31 destination tiles");
        bytes += (double)m->w * m->h + (double)dw * dh;  // every source pixel once, every result once
    }
    std::vector<StxBufRef> dsts((size_t)n);
    for (int i = 0; i < n; i++) {
        STX_TRY(stx_buf_new(ctx, items[i].dw, items[i].dh, 1, STX_U8, &dsts[i]));
        dsts[i]->mask_binary = 1;
        items[i].dst = dsts[i]->ptr; items[i].dstride = (long long)dsts[i]->stride;
    }
    StxDevBlock d_items;
    STX_TRY(upload_small(ctx, items.data(), items.size() * sizeof(StxResizeItem), &d_items));
    STX_TRY(stx_launch_mask_shrink_batch(ctx, (const StxResizeItem*)d_items.get(), n, (int)tiles, bytes));
    for (int i = 0; i < n; i++) outs[i] = dsts[i].release();
    return STX_OK;  // the descriptor block goes back here: stream-ordered reuse
}

STX_EXPORT int stx_seam_mask_resize(stx_ctx* ctx, const stx_buf* seam_mask, const stx_buf* final_mask, stx_buf** out)
{
    if (!ctx || !seam_mask || !final_mask || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    if (seam_mask->c != 1 || seam_mask->elem != STX_U8 || final_mask->c != 1 || final_mask->elem != STX_U8)
        return stx_fail(STX_ERR_INVALID, "seam masks are u8x1");
    STX_TRY(stx_set_device(ctx));
    if (seam_mask->ctx->device == ctx->device && final_mask->ctx->device == ctx->device) {  // the one-launch form first
        StxBufRef d;
        STX_TRY(stx_buf_new(ctx, final_mask->w, final_mask->h, 1, STX_U8, &d));
        stx_buf* const dp = d.get();
        bool done = false;
        STX_TRY(stx_launch_seam_resize_lds(ctx, 1, &seam_mask, &final_mask, &dp, nullptr, &done));
        if (done) { *out = d.release(); return STX_OK; }
    }
    return resize_impl(ctx, seam_mask, final_mask->w, final_mask->h, true, final_mask, out);
}

// SeamFinder.resize for all images of a panorama: one table upload, one dilate launch and one resize launch per 16 images.
// Falls back to the per-image call when a buffer does not meet the 4-pixel kernel's alignment needs.
// sub: null -> final_masks[i] is the whole final mask; else {full_w, full_h, x0, y0} per image: final_masks[i] is the
// rectangle at (x0, y0) of a final mask of size full_w x full_h (the seam mask is enlarged to THAT size, only the
// rectangle is produced; x0 a multiple of 4)
static int seam_resize_batch_impl(stx_ctx* ctx, int n, const stx_buf* const* seam_masks, const stx_buf* const* final_masks,
                                  const int* sub, stx_buf** outs)
{
    if (!ctx || n < 0 || (n > 0 && (!seam_masks || !final_masks || !outs))) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    bool fast = true;
    for (int i = 0; i < n && sub; i++) {
        const int* q = sub + 4 * i;
        if (!final_masks[i] || q[2] < 0 || q[3] < 0 || (q[2] & 3) || q[2] + final_masks[i]->w > q[0] || q[3] + final_masks[i]->h > q[1])
            return stx_fail(STX_ERR_INVALID, "seam mask rectangle %d outside its final mask (or x0 not a multiple of 4)", i);
    }
    for (int i = 0; i < n; i++) {
        const stx_buf *s = seam_masks[i], *m = final_masks[i];
        if (!s || !m) return stx_fail(STX_ERR_INVALID, "null argument");
        if (s->c != 1 || s->elem != STX_U8 || m->c != 1 || m->elem != STX_U8) return stx_fail(STX_ERR_INVALID, "seam masks are u8x1");
        if (s->ctx->device != ctx->device || m->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "image lives on another device");
        fast = fast && ((uintptr_t)m->ptr & 3) == 0 && (m->stride & 3) == 0 && (size_t)((m->w + 3) & ~3) <= m->stride;
    }
    if (n == 0) return STX_OK;
    // final masks the 4-pixel kernel cannot read in place (a view that starts on an odd byte, a pitch that is not a multiple
    // of 4): whole masks go through the per-image call; rectangles (sub) are first copied into aligned buffers of their own
    std::vector<StxBufRef> aligned;  // released on every path below
    std::vector<const stx_buf*> fm(final_masks, final_masks + n);
    if (!fast && !sub) {
        std::vector<StxBufRef> made(n);
        for (int i = 0; i < n; i++) {
            const int rc1 = stx_seam_mask_resize(ctx, seam_masks[i], final_masks[i], &outs[i]);
            if (rc1 != STX_OK) {  // hand nothing out: `made` releases what the earlier iterations produced
                std::fill(outs, outs + i, nullptr);
                return rc1;
            }
            made[i].reset(outs[i]);
        }
        for (StxBufRef& m : made) m.release();
        return STX_OK;
    }
    if (!fast) {
        for (int i = 0; i < n; i++) {
            const stx_buf* m = final_masks[i];
            if (((uintptr_t)m->ptr & 3) == 0 && (m->stride & 3) == 0 && (size_t)((m->w + 3) & ~3) <= m->stride) continue;
            aligned.emplace_back();
            StxBufRef& c = aligned.back();
            STX_TRY(stx_buf_new(ctx, m->w, m->h, 1, STX_U8, &c));
            STX_HIP(hipMemcpy2DAsync(c->ptr, c->stride, m->ptr, m->stride, (size_t)m->w, (size_t)m->h, hipMemcpyDeviceToDevice, ctx->stream));
            c->mask_binary = m->mask_binary;
            fm[i] = c.get();
        }
    }
    final_masks = fm.data();
    {
        // the one-launch form: nothing to upload, no scratch (whole buffers of the library's own qualify; anything else: the tables below)
        std::vector<StxBufRef> d1(n);
        for (int i = 0; i < n; i++) STX_TRY(stx_buf_new(ctx, final_masks[i]->w, final_masks[i]->h, 1, STX_U8, &d1[i]));
        bool done = false;
        STX_TRY(stx_launch_seam_resize_lds(ctx, n, seam_masks, final_masks, stx_buf_ptrs(d1).data(), sub, &done));
        if (done) {
            for (int i = 0; i < n; i++) outs[i] = d1[i].release();
            return STX_OK;
        }
    }
    // tables of all images in one upload: per image xt (dw rounded up to 4 entries) then yt
    std::vector<int> all;
    std::vector<size_t> xoff(n), yoff(n);
    for (int i = 0; i < n; i++) {
        std::vector<int> xt, yt;
        linear_exact_table(seam_masks[i]->w, sub ? sub[4 * i] : final_masks[i]->w, xt);
        linear_exact_table(seam_masks[i]->h, sub ? sub[4 * i + 1] : final_masks[i]->h, yt);
        if (sub) {  // the rectangle's slice of the tables (2 ints per destination column / row)
            const int x0 = sub[4 * i + 2], y0 = sub[4 * i + 3];
            xt = std::vector<int>(xt.begin() + 2 * (size_t)x0, xt.begin() + 2 * (size_t)(x0 + final_masks[i]->w));
            yt = std::vector<int>(yt.begin() + 2 * (size_t)y0, yt.begin() + 2 * (size_t)(y0 + final_masks[i]->h));
        }
        xt.resize((xt.size() + 7) & ~(size_t)7, 0);
        xoff[i] = all.size();
        all.insert(all.end(), xt.begin(), xt.end());
        yoff[i] = all.size();
        all.insert(all.end(), yt.begin(), yt.end());
        all.resize((all.size() + 7) & ~(size_t)7, 0);  // keep every table 32-byte aligned
    }
    StxDevBlock d_tab;
    STX_TRY(upload_small(ctx, all.data(), all.size() * sizeof(int), &d_tab));
    std::vector<StxBufRef> dsts(n);
    std::vector<StxDevBlock> tmps(n);  // (declared after d_tab: returned to the allocator first)
    std::vector<uint8_t*> tptr(n);
    std::vector<size_t> tstride(n);
    std::vector<const int*> dx(n), dy(n);
    for (int i = 0; i < n; i++) {
        STX_TRY(stx_buf_new(ctx, final_masks[i]->w, final_masks[i]->h, 1, STX_U8, &dsts[i]));
        tstride[i] = ((size_t)seam_masks[i]->w + 63) & ~(size_t)63;
        STX_TRY(stx_dev_alloc(ctx, tstride[i] * seam_masks[i]->h, &tmps[i]));
        tptr[i] = (uint8_t*)tmps[i].get();
        dx[i] = (const int*)d_tab.get() + xoff[i];
        dy[i] = (const int*)d_tab.get() + yoff[i];
    }
    STX_TRY(stx_launch_seam_resize_batch(ctx, n, seam_masks, final_masks, stx_buf_ptrs(dsts).data(), dx.data(), dy.data(), tptr.data(), tstride.data()));
    for (int i = 0; i < n; i++) outs[i] = dsts[i].release();
    return STX_OK;  // the scratch blocks go back here: stream-ordered reuse
}

STX_EXPORT int stx_seam_mask_resize_batch(stx_ctx* ctx, int n, const stx_buf* const* seam_masks, const stx_buf* const* final_masks,
                                          stx_buf** outs)
{
    return seam_resize_batch_impl(ctx, n, seam_masks, final_masks, nullptr, outs);
}

STX_EXPORT int stx_seam_mask_resize_batch_sub(stx_ctx* ctx, int n, const stx_buf* const* seam_masks, const stx_buf* const* final_masks,
                                              const int* full_wh_xy0, stx_buf** outs)
{
    if (!full_wh_xy0 && n > 0) return stx_fail(STX_ERR_INVALID, "null argument");
    return seam_resize_batch_impl(ctx, n, seam_masks, final_masks, full_wh_xy0, outs);
}

// include/stitching_amd_debug.h: which kernels the seam masks of this context went through so far
STX_EXPORT int stx_debug_seam_resize_paths(stx_ctx* ctx, int out_images[4])
{
    if (!ctx || !out_images) return stx_fail(STX_ERR_INVALID, "null argument");
    std::copy(ctx->seam_resize_paths, ctx->seam_resize_paths + 4, out_images);
    return STX_OK;
}
