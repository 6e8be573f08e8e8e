// stx_gain_host.cpp — host side of the exposure gains multiplied into warped images between warp and feed: one gain per image or
// channel (stx_gain_apply) and block gain maps (stx_block_gain_apply_batch), with the coefficient tables of cv::resize(INTER_LINEAR).
// Kernels: stx_gain.hip.  Compiled with -ffp-contract=off: the tables restate OpenCV's baseline (non-FMA) evaluation order.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "stx_internal.h"

// "next" rows: exposure gain between warp and feed (N1)
STX_EXPORT int stx_gain_apply(stx_ctx* ctx, stx_buf* img, const float gains_bgr[3])
{
    if (!ctx || !img || !gains_bgr) return stx_fail(STX_ERR_INVALID, "null argument");
    if (img->elem != STX_U8 || img->c != 3) return stx_fail(STX_ERR_INVALID, "gain apply needs a u8x3 image");
    if (img->ctx != ctx) return stx_fail(STX_ERR_INVALID, "image belongs to another context");
    STX_TRY(stx_set_device(ctx));
    return stx_launch_gain_apply(ctx, img, gains_bgr);
}

// coefficient set-up of cv::resize(INTER_LINEAR) for CV_32F [OCV-MEM]: f = (float)((d + 0.5) * scale - 0.5), s = floor(f),
// f -= s; horizontal offsets are clamped with f = 0 at both ends, vertical ones are not (rows are clamped when fetched)
static void linear_f32_table(int src_n, int dst_n, bool clamp_offsets, std::vector<int>& t)
{
    t.resize(2 * (size_t)dst_n);
    const double scale = 1.0 / ((double)dst_n / (double)src_n);
    for (int d = 0; d < dst_n; d++) {
        float f = (float)(((double)d + 0.5) * scale - 0.5);
        int sidx = (int)std::floor(f);
        f = f - (float)sidx;
        if (clamp_offsets) {
            if (sidx < 0) { sidx = 0; f = 0.f; }
            else if (sidx >= src_n - 1) { sidx = src_n - 1; f = 0.f; }
        }
        int bits;
        memcpy(&bits, &f, 4);
        t[2 * (size_t)d] = sidx;
        t[2 * (size_t)d + 1] = bits;
    }
}

// one image through the one-pixel-per-lane kernel: any alignment (views), any gain-map size
static int block_gain_plain(stx_ctx* ctx, stx_buf* img, const stx_buf* gain_map)
{
    std::vector<int> xt, yt;
    linear_f32_table(gain_map->w, img->w, true, xt);
    linear_f32_table(gain_map->h, img->h, false, yt);
    const size_t nx = xt.size();
    xt.resize((nx + 7) & ~(size_t)7, 0);  // entries in whole groups of 4 columns (the 4-pixel seam kernel reads 4 at once), 32-byte rows
    std::vector<int> both(xt);
    both.insert(both.end(), yt.begin(), yt.end());
    StxDevBlock d_tab;
    STX_TRY(upload_small(ctx, both.data(), both.size() * sizeof(int), &d_tab));
    return stx_launch_block_gain(ctx, img, gain_map, (const int*)d_tab.get(), (const int*)d_tab.get() + xt.size());
}

int block_gain_check(stx_ctx* ctx, const stx_buf* img, const stx_buf* gain_map)
{
    if (!gain_map) return stx_fail(STX_ERR_INVALID, "null argument");
    if (img && (img->elem != STX_U8 || img->c != 3)) return stx_fail(STX_ERR_INVALID, "block gain apply needs a u8x3 image");
    if (gain_map->elem != STX_F32 || (gain_map->c != 1 && gain_map->c != 3))
        return stx_fail(STX_ERR_INVALID, "the gain map must be f32x1 (gain_blocks) or f32x3 (channel_blocks)");
    if ((img && img->ctx != ctx) || gain_map->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "buffers belong to another context");
    return STX_OK;
}

// flags_or_null[i] & STX_GAIN_MAP_BOUNDED: the caller has checked that every gain of map i is finite and |g| < 2^31 / 255 (then no
// product p * g can leave the int range, and the kernel drops the cvRound overflow test)
STX_EXPORT int stx_block_gain_apply_batch(stx_ctx* ctx, int n, stx_buf* const* imgs, const stx_buf* const* gain_maps,
                                          const int* full_wh_xy0, const int* flags_or_null)
{
    if (!ctx || n < 0 || (n > 0 && (!imgs || !gain_maps))) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (n == 0) return STX_OK;
    STX_TRY(stx_set_device(ctx));
    for (int i = 0; i < n; i++) {
        if (!imgs[i]) return stx_fail(STX_ERR_INVALID, "null argument");
        STX_TRY(block_gain_check(ctx, imgs[i], gain_maps[i]));
        if (full_wh_xy0) {
            const int* q = full_wh_xy0 + 4 * i;
            if (q[2] < 0 || q[3] < 0 || q[2] + imgs[i]->w > q[0] || q[3] + imgs[i]->h > q[1])
                return stx_fail(STX_ERR_INVALID, "image %d: rectangle (%d,%d,%dx%d) outside the full image %dx%d", i, q[2], q[3], imgs[i]->w, imgs[i]->h, q[0], q[1]);
        }
    }
    // the batched kernels want whole buffers of the library's own (dword rows, 4-pixel groups) and gain maps of block size (their
    // horizontally interpolated rows are kept: gh x w floats); anything else takes the plain kernel, one image at a time
    std::vector<stx_buf*> bi;
    std::vector<const stx_buf*> bg;
    std::vector<int> sub, fast, plain;
    size_t scratch = 0;
    std::vector<size_t> offH, offY;
    // classify and validate EVERY image before anything is launched: the product is written in place, so a call that fails must not
    // have multiplied some of its images already (a caller could not retry it)
    for (int i = 0; i < n; i++) {
        const stx_buf* im = imgs[i];
        const bool whole = !im->parent && ((uintptr_t)im->ptr & 3) == 0 && (im->stride & 3) == 0 && (size_t)((im->w + 3) & ~3) * 3 <= im->stride;
        const size_t hbytes = (size_t)gain_maps[i]->h * ((im->w + 3) & ~3) * gain_maps[i]->c * sizeof(float);
        int first_c = -1;
        for (int j = 0; j < i && first_c < 0; j++)
            if (std::find(plain.begin(), plain.end(), j) == plain.end()) first_c = gain_maps[j]->c;
        const bool same_c = first_c < 0 || gain_maps[i]->c == first_c;
        if (!whole || hbytes > ((size_t)64 << 20) || !same_c) {
            if (full_wh_xy0 && (full_wh_xy0[4 * i] != im->w || full_wh_xy0[4 * i + 1] != im->h))
                return stx_fail(STX_ERR_UNSUPPORTED, "image %d: a rectangle of a larger image must be a whole buffer with a block-sized gain map", i);
            plain.push_back(i);
        }
    }
    for (int i = 0; i < n; i++) {
        if (std::find(plain.begin(), plain.end(), i) != plain.end()) continue;
        const stx_buf* im = imgs[i];
        const size_t hbytes = (size_t)gain_maps[i]->h * ((im->w + 3) & ~3) * gain_maps[i]->c * sizeof(float);
        bi.push_back(imgs[i]); bg.push_back(gain_maps[i]);
        for (int k = 0; k < 4; k++) sub.push_back(full_wh_xy0 ? full_wh_xy0[4 * i + k] : (k == 0 ? im->w : (k == 1 ? im->h : 0)));
        fast.push_back(flags_or_null && (flags_or_null[i] & STX_GAIN_MAP_BOUNDED) ? 1 : 0);
        offH.push_back(scratch); scratch += align_up(hbytes, 256);
        offY.push_back(scratch); scratch += align_up((size_t)im->h * 8, 256);
    }
    StxDevBlock d;  // the one allocation of the batched path, made before the first launch for the same reason
    if (!bi.empty()) STX_TRY(stx_dev_alloc(ctx, scratch, &d));
    for (int i : plain) STX_TRY(block_gain_plain(ctx, imgs[i], gain_maps[i]));
    if (bi.empty()) return STX_OK;
    std::vector<float*> Hs(bi.size());
    std::vector<void*> yts(bi.size());
    for (size_t i = 0; i < bi.size(); i++) { Hs[i] = (float*)((uint8_t*)d.get() + offH[i]); yts[i] = (uint8_t*)d.get() + offY[i]; }
    return stx_launch_block_gain_batch(ctx, (int)bi.size(), bi.data(), bg.data(), sub.data(), Hs.data(), yts.data(), fast.data());
}
