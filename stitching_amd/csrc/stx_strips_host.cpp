// stx_strips_host.cpp — image-strip sharding of the multi-band blender: which columns / rows of a warped image another rank's band
// depends on, packing them into flat buffers, feeding received strips.
#include <algorithm>

#include "stx_internal.h"

// ---- image-strip sharding -------------------------------------------------------------------------------------
// Instead of per-level contributions ((short)(L W) and W: 13.3 bytes per strip pixel, plus an export pass on the sender)
// a rank can ship the COLUMNS of its warped image and mask that the other band depends on (4 bytes per pixel, copied out
// by the DMA engine) and let the receiver feed them like an image of its own.  The receiver's pyramids of the strip equal
// the owner's wherever the band looks, provided the strip holds every source column that reaches the band's region:
//   * [sx0, sx1): the level-0 columns where the band needs this image's contributions (mb_contrib_range);
//   * + gap + 2^B on both sides: a Laplacian sample depends on the bordered image within 3 * 2^B = gap columns
//     (pyrDown support 2 (2^B - 1), pyrUp of the next level 2^B more), one more 2^B for the grid snapping;
//   * where that range runs into the image's own left / right edge the border is copyMakeBorder(REFLECT): the columns the
//     reflection reads (as many as the range sticks out) must be in the strip as well.
// A cut edge of the strip is then at least gap + 2^B away from everything the band reads; what the receiver computes
// beyond it (it reflects where the owner had real pixels) is never looked at.  Rows are not cut.
static bool mb_strip_range(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int bx0, int bx1, int* x0, int* x1)
{
    int fx, fy, fw, fh, sx0, sx1;
    mb_feed_rect(b, img_w, img_h, tlx, tly, &fx, &fy, &fw, &fh);
    if (!mb_contrib_range(b, fx, fw, bx0, bx1, &sx0, &sx1)) return false;
    const int nb = b->num_bands, reach = 3 * (1 << nb) + (1 << nb);
    const int ix0 = tlx - b->rx, ix1 = ix0 + img_w;
    const int qlo = std::max(sx0 - reach, fx), qhi = std::min(sx1 + reach, fx + fw);
    int lo = std::max(ix0, qlo), hi = std::min(ix1, qhi);
    if (qlo < ix0) hi = std::max(hi, std::min(ix1, 2 * ix0 - qlo));
    if (qhi > ix1) lo = std::min(lo, std::max(ix0, 2 * ix1 - qhi));
    if (img_w < 2 * reach) { lo = ix0; hi = ix1; }  // narrower than a border: several reflections, send it whole
    lo = ix0 + ((lo - ix0) & ~7);                    // 8-pixel groups, as the rows of every image buffer
    hi = std::min(ix1, ix0 + ((hi - ix0 + 7) & ~7));
    *x0 = lo - ix0; *x1 = hi - ix0;
    return hi > lo;
}

// flags & STX_STRIP_MASK_BITS: the mask rows hold one bit per pixel (0 / 255 masks only)
static void strip_layout(int w, int h, int flags, size_t* img_stride, size_t* mask_stride, size_t* bytes)
{
    *img_stride = align_up(align_up((size_t)w, 8) * 3, 64);
    *mask_stride = (flags & STX_STRIP_MASK_BITS) ? align_up(align_up((size_t)w, 8) / 8, 64) : align_up(align_up((size_t)w, 8), 64);
    *bytes = (*img_stride + *mask_stride) * (size_t)h;
}

STX_EXPORT int stx_strip_bytes(int w, int h, int flags, size_t* out_bytes)
{
    if (!out_bytes || w <= 0 || h <= 0) return stx_fail(STX_ERR_INVALID, "strip of %dx%d", w, h);
    size_t si, sm;
    strip_layout(w, h, flags, &si, &sm, out_bytes);
    return STX_OK;
}

// The same range along y (rows [y0, y1) of an image that the rows [by0, by1) of the panorama depend on): pyrDown / pyrUp and
// the feed geometry are the same along both axes, so this is mb_level_regions + mb_contrib_range + mb_strip_range with
// (ry, rh, fy, fh, tly, img_h) in the places of (rx, rw, fx, fw, tlx, img_w).  The column version's 8-sample region alignment
// (vector lanes of the kernels) is kept: a wider region is a superset.  Rows are cut to even positions only.
static bool mb_strip_range_y(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int by0, int by1, int* y0, int* y1)
{
    int fx, fy, fw, fh;
    mb_feed_rect(b, img_w, img_h, tlx, tly, &fx, &fy, &fw, &fh);
    const int nb = b->num_bands;
    int yb[STX_MAX_BANDS + 1], ye[STX_MAX_BANDS + 1];
    yb[0] = by0; ye[0] = by1;
    for (int i = 1; i <= nb; i++) {
        const int ph = b->rh >> i;
        const int al = i <= nb - 3 ? 7 : 1;
        yb[i] = std::max(0, (yb[i - 1] >> 1) - 1) & ~al;
        ye[i] = std::min(ph, ((((ye[i - 1] - 1) >> 1) + 2) + al) & ~al);
    }
    const int al = (1 << nb) - 1;
    long long lo = yb[0], hi = ye[0];
    for (int i = 1; i <= nb; i++) {
        lo = std::min(lo, (long long)yb[i] << i);
        hi = std::max(hi, (long long)ye[i] << i);
    }
    lo = lo & ~(long long)al;
    hi = (hi + al) & ~(long long)al;
    lo = std::max(lo, (long long)fy);
    hi = std::min(hi, (long long)fy + fh);
    if (hi <= lo) return false;
    const int sy0 = (int)lo, sy1 = (int)hi;
    const int reach = 3 * (1 << nb) + (1 << nb);
    const int iy0 = tly - b->ry, iy1 = iy0 + img_h;
    const int qlo = std::max(sy0 - reach, fy), qhi = std::min(sy1 + reach, fy + fh);
    int l = std::max(iy0, qlo), h = std::min(iy1, qhi);
    if (qlo < iy0) h = std::max(h, std::min(iy1, 2 * iy0 - qlo));
    if (qhi > iy1) l = std::min(l, std::max(iy0, 2 * iy1 - qhi));
    if (img_h < 2 * reach) { l = iy0; h = iy1; }
    l = iy0 + ((l - iy0) & ~1);
    h = std::min(iy1, iy0 + ((h - iy0 + 1) & ~1));
    *y0 = l - iy0; *y1 = h - iy0;
    return h > l;
}

STX_EXPORT int stx_view_rect(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int band_x0, int band_x1, int band_y0,
                             int band_y1, int out_x0x1y0y1[4])
{
    if (!b || !out_x0x1y0y1) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_UNSUPPORTED, "multi-band blender only");
    int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    if (!mb_strip_range(b, img_w, img_h, tlx, tly, band_x0, band_x1, &x0, &x1) ||
        !mb_strip_range_y(b, img_w, img_h, tlx, tly, band_y0, band_y1, &y0, &y1))
        x0 = x1 = y0 = y1 = 0;
    out_x0x1y0y1[0] = x0; out_x0x1y0y1[1] = x1; out_x0x1y0y1[2] = y0; out_x0x1y0y1[3] = y1;
    return STX_OK;
}

STX_EXPORT int stx_strip_rect(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int band_x0, int band_x1, int out_x0x1[2],
                              size_t* out_bytes)
{
    if (!b || !out_x0x1) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_UNSUPPORTED, "multi-band blender only");
    int x0 = 0, x1 = 0;
    if (!mb_strip_range(b, img_w, img_h, tlx, tly, band_x0, band_x1, &x0, &x1)) x0 = x1 = 0;
    out_x0x1[0] = x0; out_x0x1[1] = x1;
    if (out_bytes) {
        size_t si, sm, nb = 0;
        if (x1 > x0) strip_layout(x1 - x0, img_h, 0, &si, &sm, &nb);
        *out_bytes = nb;
    }
    return STX_OK;
}

// columns [x0, x1) of u8x3 images and of their u8 masks -> one flat buffer each: the image rows (pitch as an image buffer
// of that width has it), then the mask rows.  All strips of a call are copied by one kernel launch per 16 strips.
static int strip_pack_batch_impl(stx_ctx* ctx, int n, const stx_buf* const* imgs, const stx_buf* const* masks, const int* x0s,
                                 const int* x1s, int flags, stx_buf** out_packed)
{
    if (!ctx || n < 0 || (n > 0 && (!imgs || !masks || !x0s || !x1s || !out_packed))) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    std::vector<StxBufRef> flats(n);
    std::vector<int> ws(n);
    std::vector<size_t> si(n), sm(n);
    for (int i = 0; i < n; i++) {
        const stx_buf *img = imgs[i], *mask = masks[i];
        if (!img || !mask || img->elem != STX_U8 || img->c != 3 || mask->elem != STX_U8 || mask->c != 1 || mask->w != img->w || mask->h != img->h)
            return stx_fail(STX_ERR_INVALID, "strip: u8x3 image with a u8 mask of the same size");
        if (x0s[i] < 0 || x1s[i] > img->w || x1s[i] <= x0s[i] || (x0s[i] & 7))
            return stx_fail(STX_ERR_INVALID, "strip columns [%d,%d) of %d (x0 must be a multiple of 8)", x0s[i], x1s[i], img->w);
        if (img->parent || mask->parent)
            return stx_fail(STX_ERR_INVALID, "strip: whole image buffers only (rows of whole 8-pixel groups)");
        if ((flags & STX_STRIP_MASK_BITS) && !mask->mask_binary)
            return stx_fail(STX_ERR_INVALID, "strip: a mask can travel as bits only when it is known to hold 0 / 255");
        ws[i] = x1s[i] - x0s[i];
        size_t nbytes;
        strip_layout(ws[i], img->h, flags, &si[i], &sm[i], &nbytes);
        if (nbytes > ((size_t)1 << 30)) return stx_fail(STX_ERR_UNSUPPORTED, "strip larger than 1 GiB");
        STX_TRY(stx_buf_new(ctx, (int)nbytes, 1, 1, STX_U8, &flats[i]));
        flats[i]->mask_binary = mask->mask_binary;
    }
    STX_TRY(stx_launch_strip_pack(ctx, n, imgs, masks, x0s, ws.data(), stx_buf_ptrs(flats).data(), si.data(), sm.data(), (flags & STX_STRIP_MASK_BITS) != 0));
    for (int i = 0; i < n; i++) out_packed[i] = flats[i].release();
    return STX_OK;
}

STX_EXPORT int stx_strip_pack_batch_ex(stx_ctx* ctx, int n, const stx_buf* const* imgs, const stx_buf* const* masks, const int* x0s,
                                       const int* x1s, int flags, stx_buf** out_packed)
{
    return strip_pack_batch_impl(ctx, n, imgs, masks, x0s, x1s, flags, out_packed);
}

STX_EXPORT int stx_strip_pack(stx_ctx* ctx, const stx_buf* img, const stx_buf* mask, int x0, int x1, stx_buf** out_packed)
{
    return strip_pack_batch_impl(ctx, 1, &img, &mask, &x0, &x1, 0, out_packed);
}

// the image and mask of received strips: views of the flat buffers (which they keep alive); with STX_STRIP_MASK_BITS the masks
// are fresh buffers filled by one expand launch per 16 strips
static int strip_unpack_impl(int n, const stx_buf* const* packed, const int* ws, const int* hs, int flags, std::vector<StxBufRef>& out_imgs,
                             std::vector<StxBufRef>& out_masks)
{
    const bool bits = (flags & STX_STRIP_MASK_BITS) != 0;
    std::vector<const uint8_t*> bit_rows(n, nullptr);
    std::vector<size_t> sms(n, 0);
    out_imgs = std::vector<StxBufRef>(n);
    out_masks = std::vector<StxBufRef>(n);
    for (int i = 0; i < n; i++) {
        const stx_buf* p = packed[i];
        size_t si, sm, nbytes;
        if (!p || ws[i] <= 0 || hs[i] <= 0) return stx_fail(STX_ERR_INVALID, "strip of %dx%d", ws[i], hs[i]);
        strip_layout(ws[i], hs[i], flags, &si, &sm, &nbytes);
        if (p->elem != STX_U8 || p->c != 1 || p->h != 1 || (size_t)p->w < nbytes)
            return stx_fail(STX_ERR_INVALID, "packed strip of %d bytes, %zu needed for %dx%d", p->w, nbytes, ws[i], hs[i]);
        stx_buf* root = const_cast<stx_buf*>(p);
        for (int k = 0; k < (bits ? 1 : 2); k++) {
            stx_buf* v = new stx_buf();
            v->ctx = p->ctx; v->base = p->base;
            v->ptr = p->ptr + (k ? si * (size_t)hs[i] : 0);
            v->w = ws[i]; v->h = hs[i]; v->c = k ? 1 : 3; v->elem = STX_U8;
            v->stride = k ? sm : si;
            v->parent = root;
            v->mask_binary = k && (flags & STX_CONTRIB_U8_BINARY) ? 1 : 0;
            stx_buf_retain(root);
            (k ? out_masks : out_imgs)[i].reset(v);
        }
        if (bits) {
            STX_TRY(stx_buf_new(p->ctx, ws[i], hs[i], 1, STX_U8, &out_masks[i]));
            out_masks[i]->mask_binary = 1;
            bit_rows[i] = p->ptr + si * (size_t)hs[i];
            sms[i] = sm;
        }
    }
    if (bits && n > 0) {
        STX_TRY(stx_set_device(packed[0]->ctx));
        STX_TRY(stx_launch_strip_bits_expand(packed[0]->ctx, n, bit_rows.data(), sms.data(), stx_buf_ptrs(out_masks).data()));
    }
    return STX_OK;
}

STX_EXPORT int stx_strip_unpack(const stx_buf* packed, int w, int h, int flags, stx_buf** out_img, stx_buf** out_mask)
{
    if (!packed || !out_img || !out_mask) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_img = *out_mask = nullptr;  // also what a failure leaves
    std::vector<StxBufRef> img, mask;
    STX_TRY(strip_unpack_impl(1, &packed, &w, &h, flags, img, mask));
    *out_img = img[0].release();
    *out_mask = mask[0].release();
    return STX_OK;
}

STX_EXPORT int stx_blend_feed_strips(stx_blender* b, int n, const stx_buf* const* packed, const int* ws, const int* hs, const int* tlxs,
                                     const int* tlys, const int* orders, int flags)
{
    if (!b || n < 0 || (n > 0 && (!packed || !ws || !hs || !tlxs || !tlys || !orders))) return stx_fail(STX_ERR_INVALID, "null argument");
    if (n == 0) return STX_OK;
    std::vector<StxBufRef> imgs, masks;  // dropped on return: the blender holds its own references
    STX_TRY(strip_unpack_impl(n, packed, ws, hs, flags, imgs, masks));
    for (int i = 0; i < n; i++) STX_TRY(stx_blend_feed_ex(b, imgs[i].get(), masks[i].get(), tlxs[i], tlys[i], orders[i]));
    return STX_OK;
}
