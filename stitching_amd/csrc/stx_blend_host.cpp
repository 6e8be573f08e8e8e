// stx_blend_host.cpp — host side of the three Blender state machines (multi-band, feather, "no": feed, deferred gather at blend())
// and of the per-level contributions of sharded multi-band blending.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "stx_blend_kernels.h"
#include "stx_internal.h"

STX_EXPORT int stx_debug_feather_dist_cap(void) { return STX_FEATHER_DIST_CAP; }

// ---------------------------------------------------------------------------------------------
// blenders
// ---------------------------------------------------------------------------------------------
STX_EXPORT int stx_result_roi(int n, const int* corners_xy, const int* sizes_wh, int out_xywh[4])
{
    if (n <= 0 || !corners_xy || !sizes_wh || !out_xywh) return stx_fail(STX_ERR_INVALID, "bad argument");
    int tlx = INT_MAX, tly = INT_MAX, brx = INT_MIN, bry = INT_MIN;
    for (int i = 0; i < n; i++) {
        tlx = std::min(tlx, corners_xy[2 * i]);
        tly = std::min(tly, corners_xy[2 * i + 1]);
        brx = std::max(brx, corners_xy[2 * i] + sizes_wh[2 * i]);
        bry = std::max(bry, corners_xy[2 * i + 1] + sizes_wh[2 * i + 1]);
    }
    out_xywh[0] = tlx; out_xywh[1] = tly; out_xywh[2] = brx - tlx; out_xywh[3] = bry - tly;
    return STX_OK;
}

constexpr size_t MB_FRONT_PAD = 64;  // bytes in front of every int16 pyramid / finished-level buffer (keeps 64-byte alignment)

static void blender_release(stx_blender* b)
{
    for (stx_buf* h : b->held) stx_buf_release(h);
    b->held.clear();
    for (void* p : b->pyr_allocs) stx_dev_free(b->ctx, p);
    b->pyr_allocs.clear();
    for (void* p : b->wt_allocs) stx_dev_free(b->ctx, p);
    b->wt_allocs.clear();
    stx_mb_weights_release(b->keep);
    stx_mb_weights_release(b->adopted);
    b->keep = b->adopted = nullptr;
    b->d_all = b->d_gather = nullptr;
    b->images.clear();
    b->built.clear();
    b->no_images.clear();
    b->feather_images.clear();
}

STX_EXPORT int stx_blend_create(stx_ctx* ctx, int kind, int num_bands, float sharpness, const int roi_xywh[4],
                                stx_blender** out)
{
    if (!roi_xywh || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    // ctx == NULL: geometry-only multi-band blender (band count, feed / contribution rectangles) for
    // planning on hosts without a GPU; it cannot be fed
    if (!ctx && kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (ctx) STX_TRY(stx_set_device(ctx));
    if (kind < STX_BLEND_NO || kind > STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_INVALID, "unknown blender kind %d", kind);
    int w = roi_xywh[2], h = roi_xywh[3];
    if (w <= 0 || h <= 0) return stx_fail(STX_ERR_INVALID, "empty destination roi %dx%d", w, h);
    std::unique_ptr<stx_blender> b(new stx_blender());
    b->ctx = ctx;
    b->kind = kind;
    b->sharpness = sharpness;
    b->fw = w; b->fh = h;
    if (kind == STX_BLEND_MULTIBAND) {
        if (num_bands < 0) return stx_fail(STX_ERR_INVALID, "num_bands %d", num_bands);  // CV_Assert(val >= 0)
        // MultiBandBlender::prepare: crop unnecessary bands, pad to a multiple of 2^bands
        double max_len = (double)std::max(w, h);
        int nb = std::min(num_bands, (int)std::ceil(std::log(max_len) / std::log(2.0)));
        if (nb > STX_MAX_BANDS) nb = STX_MAX_BANDS;
        b->num_bands = nb;
        w += ((1 << nb) - w % (1 << nb)) % (1 << nb);
        h += ((1 << nb) - h % (1 << nb)) % (1 << nb);
    }
    b->rx = roi_xywh[0]; b->ry = roi_xywh[1]; b->rw = w; b->rh = h;
    b->band_x0 = 0; b->band_x1 = b->fw;
    b->pyr_mode = pyrdown_now();
    *out = b.release();
    return STX_OK;
}

STX_EXPORT int stx_blend_num_bands(const stx_blender* b, int* out_num_bands)
{
    if (!b || !out_num_bands) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_num_bands = b->num_bands;
    return STX_OK;
}

// MultiBandBlender::feed geometry: keep the image with a gap, snap to the 2^bands grid, stay inside dst_roi_.
// Returns the feed rectangle (tl_new .. br_new) relative to the padded roi.
void mb_feed_rect(const stx_blender* b, int w, int h, int tlx, int tly, int* fx, int* fy, int* fw, int* fh)
{
    const int nb = b->num_bands;
    const int gap = 3 * (1 << nb);
    int tlnx = std::max(b->rx, tlx - gap), tlny = std::max(b->ry, tly - gap);
    int brnx = std::min(b->rx + b->rw, tlx + w + gap), brny = std::min(b->ry + b->rh, tly + h + gap);
    tlnx = b->rx + (((tlnx - b->rx) >> nb) << nb);
    tlny = b->ry + (((tlny - b->ry) >> nb) << nb);
    int width = brnx - tlnx, height = brny - tlny;
    width += ((1 << nb) - width % (1 << nb)) % (1 << nb);
    height += ((1 << nb) - height % (1 << nb)) % (1 << nb);
    brnx = tlnx + width;
    brny = tlny + height;
    const int dy = std::max(brny - (b->ry + b->rh), 0), dx = std::max(brnx - (b->rx + b->rw), 0);
    tlnx -= dx; tlny -= dy;
    *fx = tlnx - b->rx; *fy = tlny - b->ry; *fw = width; *fh = height;
}

// Region of every level that the columns [bx0, bx1) of the final panorama depend on (pyrUp halo:
// level i needs level i+1 at (x >> 1) +- 1).  Origins are multiples of 8 for the levels of the vector kernels
// (<= B - 3: a lane owns 8 adjacent samples) and multiples of 2 for the coarser levels of the per-sample kernel (the finer
// level reads them through dword-aligned windows): 8 samples of the coarsest level are 8 * 2^B panorama columns, which used
// to widen every band's region — and with it every strip another rank has to supply — by up to 256 columns at 5 bands.
static void mb_level_regions(const stx_blender* b, int bx0, int bx1, int* xb, int* xe)
{
    xb[0] = bx0; xe[0] = bx1;
    for (int i = 1; i <= b->num_bands; i++) {
        const int pw = b->rw >> i;
        const int al = i <= b->num_bands - 3 ? 7 : 1;
        xb[i] = std::max(0, (xb[i - 1] >> 1) - 1) & ~al;
        xe[i] = std::min(pw, ((((xe[i - 1] - 1) >> 1) + 2) + al) & ~al);
    }
}

// Level-0 column range [sx0, sx1) (2^bands aligned, clipped to the feed rect [fx, fx+fw)) of the
// contribution an image must supply to the rank that owns the columns [bx0, bx1).
bool mb_contrib_range(const stx_blender* b, int fx, int fw, int bx0, int bx1, int* sx0, int* sx1)
{
    int xb[STX_MAX_BANDS + 1], xe[STX_MAX_BANDS + 1];
    mb_level_regions(b, bx0, bx1, xb, xe);
    const int nb = b->num_bands, al = (1 << nb) - 1;
    long long lo = xb[0], hi = xe[0];
    for (int i = 1; i <= nb; i++) {
        lo = std::min(lo, (long long)xb[i] << i);
        hi = std::max(hi, (long long)xe[i] << i);
    }
    lo = lo & ~(long long)al;
    hi = (hi + al) & ~(long long)al;
    lo = std::max(lo, (long long)fx);
    hi = std::min(hi, (long long)fx + fw);
    *sx0 = (int)lo; *sx1 = (int)hi;
    return hi > lo;
}

// packed layout of a contribution strip of size (w, h) at level 0: per level i the three int16 planes
// then the fp32 weights; every section starts on a 256-byte boundary
struct ContribLayout {
    size_t g_off[STX_MAX_BANDS + 1], w_off[STX_MAX_BANDS + 1];
    long long g_stride[STX_MAX_BANDS + 1], w_stride[STX_MAX_BANDS + 1];
    size_t bytes;
};
static void mb_contrib_layout(int nb, int w, int h, ContribLayout* L)
{
    size_t off = 0;
    for (int i = 0; i <= nb; i++) {
        const int lw = w >> i, lh = h >> i;
        L->g_stride[i] = (long long)align_up((size_t)std::max(lw, 1), 32);
        L->w_stride[i] = (long long)align_up((size_t)std::max(lw, 1), 16);
        L->g_off[i] = off;
        off = align_up(off + (size_t)L->g_stride[i] * std::max(lh, 1) * 3 * sizeof(short), 256);
        L->w_off[i] = off;
        off = align_up(off + (size_t)L->w_stride[i] * std::max(lh, 1) * sizeof(float), 256);
    }
    L->bytes = off;
}

static void mb_insert_sorted(stx_blender* b, const StxMbImage& im, bool is_built)
{
    size_t pos = b->images.size();
    while (pos > 0 && b->images[pos - 1].order > im.order) pos--;
    b->images.insert(b->images.begin() + pos, im);
    b->built.insert(b->built.begin() + pos, is_built ? 1 : 0);
    b->d_all = nullptr;
}

static int mb_feed(stx_blender* b, const stx_buf* img, const stx_buf* mask, int tlx, int tly, int order)
{
    stx_ctx* ctx = b->ctx;
    const int nb = b->num_bands, w = img->w, h = img->h;
    StxMbImage im;
    memset(&im, 0, sizeof(im));
    im.kind = 0;
    im.order = order;
    mb_feed_rect(b, w, h, tlx, tly, &im.fx, &im.fy, &im.fw, &im.fh);
    im.img0 = img->ptr; im.img0_stride = (long long)img->stride; im.img0_is_s16 = img->elem == STX_S16;
    im.mask0 = mask->ptr; im.mask0_stride = (long long)mask->stride; im.mask_binary = mask->mask_binary;
    im.iw = w; im.ih = h;
    im.ix = tlx - b->rx; im.iy = tly - b->ry;
    im.left = im.ix - im.fx; im.top = im.iy - im.fy;
    // the Gaussian levels of a u8 image are 0..255: stored as bytes (3 instead of 6 bytes per sample on every pyramid pass)
    im.g_u8 = img->elem == STX_U8 ? 1 : 0;
    // W_1 of a 0 / 255 mask is k / 256, k <= 256: stored as halves, exactly (StxMbImage::w1_f16).  STITCHING_AMD_W1_F32: diagnostic (fp32 as before)
    static const bool w1_f32 = getenv("STITCHING_AMD_W1_F32") != nullptr;
    im.w1_f16 = (mask->mask_binary && !w1_f32) ? 1 : 0;
    for (int i = 1; i <= nb; i++) {
        const int lw = im.fw >> i, lh = im.fh >> i;
        // rows of 64 bytes either way
        const long long gs = (long long)align_up((size_t)lw, im.g_u8 ? 64 : 32), ws = (long long)align_up((size_t)lw, 16);
        void* g = nullptr;
        // MB_FRONT_PAD in front, 64 bytes behind: the pyrUp tap windows of the gather kernels start up to 4 bytes in front of a row
        // and end up to 8 bytes behind its last sample (up_patch_pks_load / up_patch_pk_load)
        STX_TRY(stx_dev_alloc(ctx, MB_FRONT_PAD + (size_t)gs * lh * 3 * (im.g_u8 ? 1 : sizeof(short)) + 64, &g));
        b->pyr_allocs.push_back(g);
        im.g[i] = (short*)((uint8_t*)g + MB_FRONT_PAD); im.g_stride[i] = gs; im.g_plane[i] = gs * lh;
        // the weights' blocks are taken where the pyramids are built (mb_ensure_pyramids): a blender that adopts a handle's weights
        // before that (stx_blend_use_weights) never takes any — and leaves the allocator's free blocks to the next panorama of the rig as
        // it found them, which keeps the addresses in its descriptor table the same from panorama to panorama
        im.wt[i] = nullptr; im.wt_stride[i] = ws;
    }
    // deferred: the pyramids of all images are built together (one launch per level), at the first
    // export / blend() that needs them
    mb_insert_sorted(b, im, nb == 0);
    stx_buf_retain(const_cast<stx_buf*>(img));
    stx_buf_retain(const_cast<stx_buf*>(mask));
    b->held.push_back(const_cast<stx_buf*>(img));
    b->held.push_back(const_cast<stx_buf*>(mask));
    return STX_OK;
}

// upload `n` descriptors through the context's pinned ring: asynchronous, in stream order, no host wait
static int mb_upload(stx_blender* b, const StxMbImage* h, int n, StxMbImage** d_out)
{
    stx_ctx* ctx = b->ctx;
    void* d = nullptr;
    STX_TRY(stx_dev_alloc(ctx, sizeof(StxMbImage) * std::max(n, 1), &d));
    b->pyr_allocs.push_back(d);
    if (n > 0) STX_TRY(stx_stage_upload(ctx, d, h, sizeof(StxMbImage) * (size_t)n));
    ctx->blend_uploads++;
    *d_out = (StxMbImage*)d;
    return STX_OK;
}

// The descriptor table of a blender that adopted `w`, all n = w->images.size() of its images: the resident copy that equals it byte for
// byte, or the least recently used slot after an upload into it.  Stream order keeps the gathers of earlier blends, which may still read
// the slot, in front of the copy; the handle outlives the launches (the blender holds a reference until it is released behind them, and
// the handle's blocks go back to the allocator in stream order).
static int mb_resident_table(stx_blender* b, stx_mb_weights* w, const StxMbImage* h, int n, StxMbImage** d_out)
{
    stx_ctx* ctx = b->ctx;
    const size_t bytes = sizeof(StxMbImage) * (size_t)n;
    stx_mb_weights::Resident* lru = &w->resident[0];
    for (stx_mb_weights::Resident& r : w->resident) {
        if (r.d && r.shadow.size() == (size_t)n && memcmp(r.shadow.data(), h, bytes) == 0) {
            r.used = ++w->resident_clock;
            *d_out = r.d;
            return STX_OK;
        }
        if (r.used < lru->used) lru = &r;
    }
    if (!lru->d) {
        void* d = nullptr;
        STX_TRY(stx_dev_alloc(ctx, bytes, &d));
        w->allocs.push_back(d);
        lru->d = (StxMbImage*)d;
    }
    lru->shadow.clear();  // no shadow answers for a slot whose upload failed
    STX_TRY(stx_stage_upload(ctx, lru->d, h, bytes));
    ctx->blend_uploads++;
    lru->shadow.assign(h, h + n);
    lru->used = ++w->resident_clock;
    *d_out = lru->d;
    return STX_OK;
}

static int mb_ensure_pyramids(stx_blender* b)
{
    // weight blocks of the images about to be built, unless they came with an adopted handle (mb_feed left them open)
    for (size_t i = 0; i < b->images.size(); i++) {
        StxMbImage& im = b->images[i];
        if (im.kind != 0 || b->built[i]) continue;
        for (int l = 1; l <= b->num_bands; l++) {
            if (im.wt[l]) continue;
            void* wt = nullptr;
            STX_TRY(stx_dev_alloc(b->ctx, (size_t)im.wt_stride[l] * (im.fh >> l) * ((l == 1 && im.w1_f16) ? sizeof(uint16_t) : sizeof(float)), &wt));
            b->wt_allocs.push_back(wt);
            im.wt[l] = (float*)wt;
            b->d_all = nullptr;
        }
    }
    std::vector<StxMbImage> todo;
    for (size_t i = 0; i < b->images.size(); i++)
        if (b->images[i].kind == 0 && !b->built[i]) todo.push_back(b->images[i]);
    if (todo.empty()) return STX_OK;
    // occupancy maps of the weight pyramids (StxMbImage::occ): one arena for this batch.  Only where every level is built by
    // the batched LDS kernels, which write them (int16 sources take the generic level-0 kernel).
    static const bool occ_off = getenv("STITCHING_AMD_NO_OCC") != nullptr;  // diagnostic: A/B of the bookkeeping
    const int pyr = b->pyr_mode;  // (the blender's own, fixed at creation) != scalar: the generic kernels build every level, and they keep no occupancy maps
    // (adopted weights: the maps came with them, and todo is every image of the blender — stx_blend_use_weights)
    if (!b->adopted && todo.size() <= 65535 && !occ_off && (pyr & 255) == STX_PYRDOWN_SCALAR) {
        const int nl = b->num_bands + 1;
        std::vector<size_t> off(todo.size() * (size_t)nl, 0);
        size_t bytes = 0;
        for (size_t t = 0; t < todo.size(); t++) {
            if (todo[t].img0_is_s16) continue;
            for (int i = 1; i < nl; i++) {
                off[t * nl + i] = bytes;
                // rows of ((fw >> i) / 64 rounded up, then to a multiple of 4) bytes; one more row = slack for the 12-byte reads
                bytes += (size_t)((((todo[t].fh >> i) + 1) >> 1) + 1) * (size_t)(((((todo[t].fw >> i) + 63) >> 6) + 3) & ~3);
            }
        }
        if (bytes > 0) {
            void* arena = nullptr;
            STX_TRY(stx_dev_alloc(b->ctx, bytes + 16, &arena));
            b->wt_allocs.push_back(arena);
            size_t t = 0;
            for (size_t i = 0; i < b->images.size(); i++) {
                if (!(b->images[i].kind == 0 && !b->built[i])) continue;
                if (!todo[t].img0_is_s16)
                    for (int l = 1; l < nl; l++) todo[t].occ[l] = b->images[i].occ[l] = (uint8_t*)arena + off[t * nl + l];
                t++;
            }
        }
    }
    StxMbImage* d = nullptr;
    // an adopted blender (todo is then every image, as many as the handle recorded): the handle's resident copies; all others upload
    b->d_all_resident = b->adopted && todo.size() == b->images.size() && todo.size() == b->adopted->images.size();
    if (b->d_all_resident) STX_TRY(mb_resident_table(b, b->adopted, todo.data(), (int)todo.size(), &d));
    else STX_TRY(mb_upload(b, todo.data(), (int)todo.size(), &d));
    // every image of the blender in this pass (the usual case): blend() reads the very same table — one upload, one copy dispatch fewer
    // between the pyramids and the collapse
    b->d_all = todo.size() == b->images.size() && memcmp(todo.data(), b->images.data(), sizeof(StxMbImage) * todo.size()) == 0 ? d : nullptr;
    STX_TRY(stx_launch_mb_pyramids(b->ctx, d, todo.data(), (int)todo.size(), b->num_bands, pyr & 255, pyr >> 8, b->adopted == nullptr));
    for (size_t i = 0; i < b->images.size(); i++) b->built[i] = 1;
    return STX_OK;
}

static double mb_level_bytes(const stx_blender* b, const std::vector<StxMbImage>& imgs, int lv, int x0, int x1, bool emit,
                             bool with16)
{
    // algorithmic bytes: every input element of the region once, every output element once
    const int nb = b->num_bands;
    const int ph = lv == 0 ? b->fh : b->rh >> lv;
    double bytes = 0.0;
    for (const StxMbImage& im : imgs) {
        int rx = im.fx >> lv, rw = im.fw >> lv, ry = im.fy >> lv, rh = im.fh >> lv;
        if (lv == 0 && im.kind == 0) { rx = im.ix; rw = im.iw; ry = im.iy; rh = im.ih; }
        const double cols = std::max(0, std::min(rx + rw, x1) - std::max(rx, x0)), rows = std::min(ry + rh, ph) - ry;
        if (cols <= 0 || rows <= 0) continue;
        const double g3 = im.g_u8 ? 3.0 : 6.0;  // the three Gaussian planes of a sample: bytes (u8 image) or int16
        if (im.kind == 1) bytes += cols * rows * 10.0;
        else if (lv == 0) bytes += cols * rows * ((im.img0_is_s16 ? 6 : 3) + 1) + (nb > 0 ? cols * rows * g3 / 4.0 : 0.0);
        else bytes += cols * rows * (g3 + ((lv == 1 && im.w1_f16) ? 2.0 : 4.0)) + (lv < nb ? cols * rows * g3 / 4.0 : 0.0);
    }
    const double area = (double)(x1 - x0) * ph;
    if (emit) return bytes + area * 10.0;
    if (lv < nb) bytes += area * 6.0 / 4.0;
    bytes += lv == 0 ? area * (4 + (with16 ? 6 : 0)) : area * 6.0;
    return bytes;
}

STX_EXPORT int stx_blend_feed_ex(stx_blender* b, const stx_buf* img, const stx_buf* mask, int tlx, int tly, int order)
{
    if (!b || !img || !mask) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->finished) return stx_fail(STX_ERR_STATE, "feed after blend()");
    if (b->adopted) return stx_fail(STX_ERR_STATE, "feed after stx_blend_use_weights adopted weights");
    if (!b->ctx) return stx_fail(STX_ERR_STATE, "geometry-only blender (created without a context)");
    STX_TRY(stx_set_device(b->ctx));
    // CV_Assert(img.type() == CV_16SC3 [|| CV_8UC3]); CV_Assert(mask.type() == CV_8U)
    if (img->c != 3 || (img->elem != STX_U8 && img->elem != STX_S16))
        return stx_fail(STX_ERR_INVALID, "feed: image must be u8x3 or s16x3");
    if (mask->c != 1 || mask->elem != STX_U8) return stx_fail(STX_ERR_INVALID, "feed: mask must be u8x1");
    if (mask->w != img->w || mask->h != img->h)
        return stx_fail(STX_ERR_INVALID, "feed: mask %dx%d does not match image %dx%d", mask->w, mask->h, img->w, img->h);
    if (img->ctx != b->ctx || mask->ctx != b->ctx) return stx_fail(STX_ERR_INVALID, "feed: buffers belong to another context");
    // the image must lie inside the roi given to prepare() (OpenCV would write out of bounds)
    const int ux = b->kind == STX_BLEND_MULTIBAND ? b->rx + b->fw : b->rx + b->rw;
    const int uy = b->kind == STX_BLEND_MULTIBAND ? b->ry + b->fh : b->ry + b->rh;
    if (tlx < b->rx || tly < b->ry || tlx + img->w > ux || tly + img->h > uy)
        return stx_fail(STX_ERR_INVALID, "feed: image at (%d,%d) size %dx%d leaves the prepared roi (%d,%d,%d,%d)", tlx, tly,
                        img->w, img->h, b->rx, b->ry, ux - b->rx, uy - b->ry);
    // the row pass of the feather blender's distance transform holds a whole row in LDS (stx_internal.h: stx_feather_rows_per_block)
    if (b->kind == STX_BLEND_FEATHER) STX_TRY(stx_feather_refuse_width(img->w));
    if (order < 0) order = b->next_order;
    b->next_order = std::max(b->next_order, order + 1);
    if (b->kind == STX_BLEND_MULTIBAND) return mb_feed(b, img, mask, tlx, tly, order);
    if (b->kind == STX_BLEND_NO) {  // deferred: the image joins the table, the gather runs in blend()
        NoImg im;
        memset(&im, 0, sizeof(im));
        im.img = img->ptr; im.istride = (long long)img->stride; im.is_s16 = img->elem == STX_S16;
        im.mask = mask->ptr; im.mstride = (long long)mask->stride;
        im.x = tlx - b->rx; im.y = tly - b->ry; im.w = img->w; im.h = img->h;
        im.mask_binary = mask->mask_binary;
        b->no_images.push_back(im);
        stx_buf_retain(const_cast<stx_buf*>(img));
        stx_buf_retain(const_cast<stx_buf*>(mask));
        b->held.push_back(const_cast<stx_buf*>(img));
        b->held.push_back(const_cast<stx_buf*>(mask));
        return STX_OK;
    }
    // feather, deferred: the image joins the table; distance transforms, weights and the gather run in blend()
    FeatherImg im;
    memset(&im, 0, sizeof(im));
    im.img = img->ptr; im.istride = (long long)img->stride; im.is_s16 = img->elem == STX_S16;
    im.mask = mask->ptr; im.mstride = (long long)mask->stride;
    im.x = tlx - b->rx; im.y = tly - b->ry; im.w = img->w; im.h = img->h;
    im.dstride = ((long long)img->w + 15) & ~15ll;
    im.n_chunks = (img->h + STX_DT_RC - 1) / STX_DT_RC;
    void *wm = nullptr, *summ = nullptr;
    // 64 bytes in front and behind: a lane's group of 4 distances may start up to 3 samples left of a row / end 3 right of it
    STX_TRY(stx_dev_alloc(b->ctx, 64 + sizeof(uint16_t) * (size_t)im.dstride * img->h + 64, &wm));
    b->pyr_allocs.push_back(wm);
    wm = (uint8_t*)wm + 64;
    // per (chunk, column): the zero rows as a 64-bit set, then the first and the last of them
    STX_TRY(stx_dev_alloc(b->ctx, (sizeof(unsigned long long) + 2 * sizeof(int)) * (size_t)im.dstride * im.n_chunks, &summ));
    b->pyr_allocs.push_back(summ);
    im.dist = (uint16_t*)wm;
    im.zbits = (unsigned long long*)summ;
    im.first = (int*)(im.zbits + (size_t)im.dstride * im.n_chunks); im.last = im.first + (size_t)im.dstride * im.n_chunks;
    b->feather_images.push_back(im);
    stx_buf_retain(const_cast<stx_buf*>(img));
    stx_buf_retain(const_cast<stx_buf*>(mask));
    b->held.push_back(const_cast<stx_buf*>(img));
    b->held.push_back(const_cast<stx_buf*>(mask));
    return STX_OK;
}

STX_EXPORT int stx_blend_feed(stx_blender* b, const stx_buf* img, const stx_buf* mask, int tlx, int tly)
{
    return stx_blend_feed_ex(b, img, mask, tlx, tly, -1);
}

static void mb_fill_common(const stx_blender* b, MbLevelK* K, const StxMbImage* d_images, int n, int lv)
{
    memset(K, 0, sizeof(*K));
    K->images = d_images; K->n_images = n; K->level = lv; K->num_bands = b->num_bands;
    K->pw = b->rw >> lv; K->ph = b->rh >> lv;
    K->all_u8 = 1;
}

// rows [0, y1) of level lv that blend() computes
static int mb_level_y1(const stx_blender* b, int lv) { return lv == 0 ? b->fh : b->rh >> lv; }

// the adopted handle's cover table for the level K is about to run, or null: the table answers for the region and the tile map it was
// recorded over and for no other (a band set after adoption, another tile height)
static const unsigned long long* mb_cover_for(const stx_mb_weights* w, const MbLevelK& K)
{
    if (!w || K.level < 0 || K.level > STX_MAX_BANDS || K.n_images > 64 || K.n_images != (int)w->images.size()) return nullptr;
    const stx_mb_weights::Cover& c = w->cover[K.level];
    int tx, ty, br;
    stx_fast_mb_cover_dims(K.x0, K.x1, K.y0, K.y1, &tx, &ty, &br);
    if (!c.table || c.x0 != K.x0 || c.x1 != K.x1 || c.y0 != K.y0 || c.y1 != K.y1 || c.tiles_x != tx || c.tiles_y != ty || c.band_rows != br)
        return nullptr;
    return c.table;
}

// *pmask: the panorama mask — a new buffer the level-0 launch stores, or, for a blender that adopted a handle over the output region the
// handle's mask was recorded for, that very buffer (one more reference): the launch then stores no mask
static int mb_finish(stx_blender* b, stx_buf* pano, StxBufRef* pmask, stx_buf* pano16)
{
    stx_ctx* ctx = b->ctx;
    const int nb = b->num_bands, n = (int)b->images.size();
    STX_TRY(mb_ensure_pyramids(b));
    StxMbImage* d_images = b->d_all;
    // a resident copy found by an earlier stx_blend_build may have been evicted by other adopters since: looked up again (a hit is a memcmp)
    if (d_images && b->d_all_resident) STX_TRY(mb_resident_table(b, b->adopted, b->images.data(), n, &d_images));
    if (!d_images) STX_TRY(mb_upload(b, b->images.data(), n, &d_images));
    b->d_gather = d_images;
    bool all_u8 = true, has_contrib = false, pk_ok = true;
    for (const StxMbImage& im : b->images) {
        if (im.kind == 0 && im.img0_is_s16) all_u8 = false;
        if (im.kind == 1) has_contrib = true;
        if ((im.kind == 0 && im.img0_is_s16) || !im.mask_binary) pk_ok = false;
    }
    int xb[STX_MAX_BANDS + 1], xe[STX_MAX_BANDS + 1];
    mb_level_regions(b, b->band_x0, b->band_x1, xb, xe);
    std::vector<short*> out(nb + 2, nullptr);
    std::vector<long long> ostride(nb + 2, 0), oplane(nb + 2, 0);
    // The three coarsest levels go through one launch (mb_coarse_kernel: the finished levels B and B-1 live in LDS only) when
    // there are at least 3 bands, i.e. when level B-2 is not the panorama itself.  STITCHING_AMD_NO_COARSE_FUSION: diagnostic.
    static const bool no_fusion = getenv("STITCHING_AMD_NO_COARSE_FUSION") != nullptr;
    const bool fuse = nb >= 3 && !no_fusion;
    for (int lv = fuse ? nb - 2 : nb; lv >= 0; lv--) {
        MbLevelK K;
        mb_fill_common(b, &K, d_images, n, lv);
        K.all_u8 = all_u8 ? 1 : 0;
        K.has_contrib = has_contrib ? 1 : 0;
        K.pk_ok = pk_ok ? 1 : 0;
        K.x0 = xb[lv]; K.x1 = xe[lv]; K.y0 = 0; K.y1 = mb_level_y1(b, lv);
        if (b->adopted && !has_contrib) K.cover = mb_cover_for(b->adopted, K);
        if (lv < nb) {
            K.up = out[lv + 1]; K.up_stride = ostride[lv + 1]; K.up_plane = oplane[lv + 1];
            K.up_x0 = xb[lv + 1]; K.up_y0 = 0;
        }
        if (lv == 0) {
            K.pano = pano->ptr; K.pano_stride = (long long)pano->stride;
            if (pano16) { K.pano16 = (short*)pano16->ptr; K.pano16_stride = (long long)pano16->stride; }
            K.pano_x0 = b->band_x0; K.pano_y0 = 0;
            // the panorama mask of a known rig: kept with the weights, for the output region it was made over and no other (the cover
            // table's test, which K.cover has passed); only the REPLAY instantiations pass over a null — the launcher says whether K takes them
            const stx_mb_weights* w = b->adopted;
            K.pmask = nullptr;
            if (w && w->pmask && K.cover && w->pmask_x0 == b->band_x0 && w->pmask_x1 == b->band_x1 && w->pmask_h == b->fh &&
                w->pmask->w == pano->w && w->pmask->h == pano->h && stx_fast_mb_level0_skips_mask(K)) {
                stx_buf_retain(w->pmask);
                pmask->reset(w->pmask);
            } else {
                STX_TRY(stx_buf_new(ctx, pano->w, pano->h, 1, STX_U8, pmask));
                K.pmask = (*pmask)->ptr; K.pmask_stride = (long long)(*pmask)->stride;
            }
            ctx->blend_mask_stored = K.pmask ? 1 : 0;
        } else {
            const int w = xe[lv] - xb[lv], ph = b->rh >> lv;
            const long long st = (long long)align_up((size_t)std::max(w, 1), 32);
            void* p = nullptr;
            STX_TRY(stx_dev_alloc(ctx, MB_FRONT_PAD + (size_t)st * ph * 3 * sizeof(short), &p));
            b->pyr_allocs.push_back(p);
            out[lv] = (short*)((uint8_t*)p + MB_FRONT_PAD); ostride[lv] = st; oplane[lv] = st * ph;
            K.out = out[lv]; K.out_stride = st; K.out_plane = st * ph;
            K.out_x0 = xb[lv]; K.out_y0 = 0;
        }
        if (fuse && lv == nb - 2) {
            // algorithmic bytes: the inputs of the three levels over their regions once, the finished level B-2 once
            double bytes = mb_level_bytes(b, b->images, lv, K.x0, K.x1, false, false) - (double)(K.x1 - K.x0) * (b->rh >> lv) * 6.0 / 4.0;
            for (int l2 = nb - 1; l2 <= nb; l2++)
                bytes += mb_level_bytes(b, b->images, l2, xb[l2], xe[l2], false, false) - (double)(xe[l2] - xb[l2]) * (b->rh >> l2) * (l2 < nb ? 7.5 : 6.0);
            K.up = nullptr;
            STX_TRY(stx_launch_mb_coarse(ctx, K, bytes));
            continue;
        }
        STX_TRY(stx_launch_mb_level(ctx, K, mb_level_bytes(b, b->images, lv, K.x0, K.x1, false, pano16 != nullptr)));
    }
    return STX_OK;
}

// ---- weight pyramids that outlive a blender (include/stitching_amd.h: stx_blend_keep_weights) --------------------
void stx_mb_weights_release(stx_mb_weights* w)
{
    if (!w || --w->refs > 0) return;
    if (w->ctx) hipSetDevice(w->ctx->device);
    for (StxMbKept& k : w->images) stx_buf_release(k.mask);
    if (w->pmask) stx_buf_release(w->pmask);  // (whoever was handed the mask holds a reference of their own)
    for (void* p : w->allocs) stx_dev_free(w->ctx, p);  // stream-ordered, as blender_release
    delete w;
}

// what stx_blend_keep_weights asks of a blender; `built`: also of its finished pyramids (the occupancy maps were recorded)
static bool mb_weights_eligible(const stx_blender* b, bool built)
{
    if (b->kind != STX_BLEND_MULTIBAND || !b->ctx || b->num_bands < 1 || b->adopted) return false;
    if ((b->pyr_mode & 255) != STX_PYRDOWN_SCALAR || getenv("STITCHING_AMD_NO_OCC") != nullptr || b->images.size() > 65535) return false;
    for (const StxMbImage& im : b->images) {
        if (im.kind != 0 || im.img0_is_s16) return false;
        if (built && !im.occ[1]) return false;
    }
    return true;
}

// blend() succeeded: the weights and occupancy maps of a blender marked by stx_blend_keep_weights move to its handle
static void mb_hand_over_weights(stx_blender* b, stx_buf* pmask)
{
    stx_mb_weights* w = b->keep;
    if (!w || b->images.empty() || !mb_weights_eligible(b, true)) return;
    // held: (img, mask) of image k at 2 k, 2 k + 1 in FEED order; images is sorted by .order — find every mask by its pointer
    w->num_bands = b->num_bands; w->pyr_mode = b->pyr_mode;
    w->rx = b->rx; w->ry = b->ry; w->rw = b->rw; w->rh = b->rh;
    for (const StxMbImage& im : b->images) {
        StxMbKept k;
        memset(&k, 0, sizeof(k));
        for (size_t h = 1; h < b->held.size(); h += 2)
            if (b->held[h]->ptr == im.mask0 && (long long)b->held[h]->stride == im.mask0_stride) k.mask = b->held[h];
        if (!k.mask) {  // (cannot happen: every kind-0 image holds its mask)
            for (StxMbKept& q : w->images) stx_buf_release(q.mask);
            w->images.clear();
            return;
        }
        stx_buf_retain(k.mask);
        k.mask0 = im.mask0; k.mask0_stride = im.mask0_stride; k.mask_binary = im.mask_binary; k.w1_f16 = im.w1_f16;
        k.iw = im.iw; k.ih = im.ih; k.ix = im.ix; k.iy = im.iy; k.fx = im.fx; k.fy = im.fy; k.fw = im.fw; k.fh = im.fh;
        k.left = im.left; k.top = im.top;
        for (int i = 1; i <= b->num_bands; i++) { k.wt[i] = im.wt[i]; k.wt_stride[i] = im.wt_stride[i]; k.occ[i] = im.occ[i]; }
        w->images.push_back(k);
    }
    w->allocs.swap(b->wt_allocs);
    // the resident descriptor tables' device blocks, all of them now: an adopter that took one from the allocator between its feeds and its
    // launches would leave the next adopter another set of free blocks, and with it other addresses in the very table the slot is to match
    for (stx_mb_weights::Resident& r : w->resident) {
        void* d = nullptr;
        if (stx_dev_alloc(b->ctx, sizeof(StxMbImage) * b->images.size(), &d) != STX_OK) break;
        w->allocs.push_back(d);
        r.d = (StxMbImage*)d;
    }
    // the finished panorama mask over this blender's output region: what every later blend of the rig over that region would store again
    stx_buf_retain(pmask);
    w->pmask = pmask;
    w->pmask_x0 = b->band_x0; w->pmask_x1 = b->band_x1; w->pmask_h = b->fh;
    // the image search of the packed gathers (levels 0 .. B - 3), recorded while this blender's descriptor table is still alive: rectangles,
    // occupancy maps, tile positions and feed order are the rig's, and stx_blend_use_weights pins every one of them.  One word per tile
    // holds 64 images: larger rigs keep no cover and search as ever.
    if (b->images.size() > 64 || !b->d_gather) return;
    int xb[STX_MAX_BANDS + 1], xe[STX_MAX_BANDS + 1];
    mb_level_regions(b, b->band_x0, b->band_x1, xb, xe);
    for (int lv = 0; lv <= b->num_bands - 3; lv++) {
        stx_mb_weights::Cover c;
        c.x0 = xb[lv]; c.x1 = xe[lv]; c.y0 = 0; c.y1 = mb_level_y1(b, lv);
        if (c.x1 <= c.x0 || c.y1 <= c.y0) continue;
        stx_fast_mb_cover_dims(c.x0, c.x1, c.y0, c.y1, &c.tiles_x, &c.tiles_y, &c.band_rows);
        void* t = nullptr;
        if (stx_dev_alloc(b->ctx, sizeof(unsigned long long) * (size_t)c.tiles_x * (size_t)c.tiles_y, &t) != STX_OK) return;
        w->allocs.push_back(t);
        c.table = (unsigned long long*)t;
        if (!stx_fast_mb_cover(b->ctx, b->d_gather, (int)b->images.size(), lv, c.x0, c.x1, c.y0, c.y1, c.table)) return;
        w->cover[lv] = c;
    }
}

STX_EXPORT int stx_blend_keep_weights(stx_blender* b, stx_mb_weights** out)
{
    if (!b || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    *out = nullptr;
    if (b->finished) return stx_fail(STX_ERR_STATE, "keep_weights after blend()");
    if (b->keep) return stx_fail(STX_ERR_STATE, "keep_weights was already called on this blender");
    if (b->images.empty() || !mb_weights_eligible(b, false)) return STX_OK;  // not eligible: the blender builds and frees as ever
    stx_mb_weights* w = new stx_mb_weights();
    w->ctx = b->ctx;
    w->refs = 2;  // the caller's and the blender's
    b->keep = w;
    *out = w;
    return STX_OK;
}

STX_EXPORT int stx_blend_use_weights(stx_blender* b, stx_mb_weights* w, int* out_adopted)
{
    if (!b || !w || !out_adopted) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_adopted = 0;
    if (b->finished) return stx_fail(STX_ERR_STATE, "use_weights after blend()");
    if (b->ctx != w->ctx) return stx_fail(STX_ERR_INVALID, "use_weights: the handle belongs to another context (no cross-stream use)");
    if (b->adopted || b->keep || w->images.empty() || w->images.size() != b->images.size() || !mb_weights_eligible(b, false)) return STX_OK;
    if (b->num_bands != w->num_bands || b->pyr_mode != w->pyr_mode || b->rx != w->rx || b->ry != w->ry || b->rw != w->rw || b->rh != w->rh)
        return STX_OK;
    for (size_t i = 0; i < b->images.size(); i++) {
        const StxMbImage& im = b->images[i];
        const StxMbKept& k = w->images[i];
        if (b->built[i]) return STX_OK;
        if (im.mask0 != k.mask0 || im.mask0_stride != k.mask0_stride || im.mask_binary != k.mask_binary || im.w1_f16 != k.w1_f16 ||
            im.iw != k.iw || im.ih != k.ih || im.ix != k.ix || im.iy != k.iy || im.fx != k.fx || im.fy != k.fy || im.fw != k.fw ||
            im.fh != k.fh || im.left != k.left || im.top != k.top)
            return STX_OK;
        for (int l = 1; l <= b->num_bands; l++)
            if (im.wt_stride[l] != k.wt_stride[l]) return STX_OK;
    }
    STX_TRY(stx_set_device(b->ctx));
    for (size_t i = 0; i < b->images.size(); i++)
        for (int l = 1; l <= b->num_bands; l++) { b->images[i].wt[l] = w->images[i].wt[l]; b->images[i].occ[l] = w->images[i].occ[l]; }
    b->d_all = nullptr;  // (the blender has no weight blocks of its own yet: mb_ensure_pyramids takes them)
    w->refs++;
    b->adopted = w;
    *out_adopted = 1;
    return STX_OK;
}

STX_EXPORT int stx_debug_blend_replayed(stx_ctx* ctx, int* out_launches)
{
    if (!ctx || !out_launches) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_launches = ctx->blend_replayed;
    return STX_OK;
}

STX_EXPORT int stx_debug_blend_mask_stored(stx_ctx* ctx, int* out_stored)
{
    if (!ctx || !out_stored) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_stored = ctx->blend_mask_stored;
    return STX_OK;
}

STX_EXPORT int stx_debug_blend_uploads(stx_ctx* ctx, int* out_uploads)
{
    if (!ctx || !out_uploads) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_uploads = ctx->blend_uploads;
    return STX_OK;
}

STX_EXPORT int stx_mb_weights_free(stx_mb_weights* w)
{
    stx_mb_weights_release(w);
    return STX_OK;
}

// ---- sharded multi-band blending (one blender per rank) -------------------------------
STX_EXPORT int stx_blend_set_band(stx_blender* b, int x0, int x1)
{
    if (!b) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_UNSUPPORTED, "bands exist for the multi-band blender only");
    if (b->finished) return stx_fail(STX_ERR_STATE, "set_band after blend()");
    const int al = (1 << b->num_bands) - 1;
    if (x0 < 0 || x1 > b->fw || x1 <= x0 || (x0 & al) || ((x1 & al) && x1 != b->fw) || (x0 & 7))
        return stx_fail(STX_ERR_INVALID, "band [%d,%d) must lie in [0,%d) with edges on multiples of max(8, 2^bands)", x0, x1, b->fw);
    b->band_x0 = x0; b->band_x1 = x1;
    return STX_OK;
}

STX_EXPORT int stx_blend_contrib_rect(const stx_blender* b, int img_w, int img_h, int tlx, int tly, int band_x0, int band_x1,
                                      int out_rect_xywh[4], size_t* out_bytes)
{
    if (!b || !out_rect_xywh) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_UNSUPPORTED, "multi-band blender only");
    int fx, fy, fw, fh, sx0, sx1;
    mb_feed_rect(b, img_w, img_h, tlx, tly, &fx, &fy, &fw, &fh);
    if (!mb_contrib_range(b, fx, fw, band_x0, band_x1, &sx0, &sx1)) {
        out_rect_xywh[0] = out_rect_xywh[1] = out_rect_xywh[2] = out_rect_xywh[3] = 0;
        if (out_bytes) *out_bytes = 0;
        return STX_OK;
    }
    out_rect_xywh[0] = sx0; out_rect_xywh[1] = fy; out_rect_xywh[2] = sx1 - sx0; out_rect_xywh[3] = fh;
    if (out_bytes) {
        ContribLayout L;
        mb_contrib_layout(b->num_bands, sx1 - sx0, fh, &L);
        *out_bytes = L.bytes;
    }
    return STX_OK;
}

STX_EXPORT int stx_blend_export_contrib(stx_blender* b, int order, int band_x0, int band_x1, stx_buf** out_packed,
                                        int out_rect_xywh[4])
{
    return stx_blend_export_contribs(b, 1, &order, &band_x0, &band_x1, out_packed, out_rect_xywh);
}

// All strips a rank owes in one call: the (strip, level) argument blocks are grouped by kernel instantiation and every
// group is ONE launch (blockIdx.z = block), instead of levels x strips small launches.
STX_EXPORT int stx_blend_export_contribs(stx_blender* b, int n, const int* orders, const int* band_x0s, const int* band_x1s,
                                         stx_buf** out_packed, int* out_rects_xywh)
{
    if (!b || n < 0 || (n > 0 && (!orders || !band_x0s || !band_x1s || !out_packed || !out_rects_xywh)))
        return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_UNSUPPORTED, "multi-band blender only");
    if (b->finished) return stx_fail(STX_ERR_STATE, "export after blend()");
    if (!b->ctx) return stx_fail(STX_ERR_STATE, "geometry-only blender (created without a context)");
    if (n == 0) return STX_OK;
    STX_TRY(stx_set_device(b->ctx));
    const int nb = b->num_bands;
    std::vector<StxMbImage> srcs(n);
    std::vector<int> sx0(n), sx1(n);
    for (int i = 0; i < n; i++) {
        const StxMbImage* src = nullptr;
        for (const StxMbImage& im : b->images) if (im.kind == 0 && im.order == orders[i]) src = &im;
        if (!src) return stx_fail(STX_ERR_INVALID, "no fed image with order %d", orders[i]);
        if (!mb_contrib_range(b, src->fx, src->fw, band_x0s[i], band_x1s[i], &sx0[i], &sx1[i]))
            return stx_fail(STX_ERR_INVALID, "image %d does not reach the columns [%d,%d)", orders[i], band_x0s[i], band_x1s[i]);
        srcs[i] = *src;
    }
    STX_TRY(mb_ensure_pyramids(b));
    // (the copies above were taken before the pyramids' weight blocks were: mb_ensure_pyramids takes them at the first build)
    for (int i = 0; i < n; i++)
        for (const StxMbImage& im : b->images)
            if (im.kind == 0 && im.order == orders[i])
                for (int l = 1; l <= nb; l++) srcs[i].wt[l] = im.wt[l];
    std::vector<StxBufRef> packed(n);
    std::vector<ContribLayout> Ls(n);
    for (int i = 0; i < n; i++) {
        mb_contrib_layout(nb, sx1[i] - sx0[i], srcs[i].fh, &Ls[i]);
        STX_TRY(stx_buf_new(b->ctx, (int)std::min<size_t>(Ls[i].bytes, 1u << 30), (int)((Ls[i].bytes + (1u << 30) - 1) >> 30), 1, STX_U8,
                            &packed[i]));
        if (packed[i]->stride * (size_t)packed[i]->h < Ls[i].bytes) return stx_fail(STX_ERR_OOM, "contribution too large");
    }
    StxMbImage* d_srcs = nullptr;
    STX_TRY(mb_upload(b, srcs.data(), n, &d_srcs));
    // one argument block per (strip, level), sorted by the kernel instantiation it needs
    struct Item { int cls; MbLevelK K; };
    std::vector<Item> items;
    double bytes = 0.0;
    for (int i = 0; i < n; i++) {
        const StxMbImage& one = srcs[i];
        const int sh = one.fh;
        std::vector<StxMbImage> single(1, one);
        for (int lv = 0; lv <= nb; lv++) {
            MbLevelK K;
            mb_fill_common(b, &K, d_srcs + i, 1, lv);
            K.all_u8 = one.img0_is_s16 ? 0 : 1;
            K.x0 = sx0[i] >> lv; K.x1 = sx1[i] >> lv; K.y0 = one.fy >> lv; K.y1 = (one.fy + sh) >> lv;
            K.emit = 1;
            K.out = (short*)(packed[i]->ptr + Ls[i].g_off[lv]); K.out_stride = Ls[i].g_stride[lv];
            K.out_plane = Ls[i].g_stride[lv] * std::max(sh >> lv, 1);
            K.out_x0 = K.x0; K.out_y0 = K.y0;
            K.out_w = (float*)(packed[i]->ptr + Ls[i].w_off[lv]); K.out_w_stride = Ls[i].w_stride[lv];
            if (K.x1 <= K.x0 || K.y1 <= K.y0) continue;
            Item it;
            it.cls = stx_fast_mb_emit_class(K, &it.K);
            if (it.cls < 0) it.cls = lv == 0 ? -1 : -2;  // generic kernel, level 0 / level >= 1 instantiation
            items.push_back(it);
            bytes += mb_level_bytes(b, single, lv, K.x0, K.x1, true, false);
        }
    }
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& c) { return a.cls < c.cls; });
    std::vector<MbLevelK> Ks(items.size());
    std::vector<int> classes(items.size());
    for (size_t i = 0; i < items.size(); i++) { Ks[i] = items[i].K; classes[i] = items[i].cls; }
    StxDevBlock d_Ks;
    STX_TRY(upload_small(b->ctx, Ks.data(), Ks.size() * sizeof(MbLevelK), &d_Ks));
    STX_TRY(stx_launch_mb_emit_batch(b->ctx, (const MbLevelK*)d_Ks.get(), Ks.data(), classes.data(), (int)Ks.size(), bytes));
    d_Ks.reset();  // stream-ordered reuse
    for (int i = 0; i < n; i++) {
        out_rects_xywh[4 * i] = sx0[i]; out_rects_xywh[4 * i + 1] = srcs[i].fy;
        out_rects_xywh[4 * i + 2] = sx1[i] - sx0[i]; out_rects_xywh[4 * i + 3] = srcs[i].fh;
        packed[i]->mask_binary = (!srcs[i].img0_is_s16 && srcs[i].mask_binary) ? 1 : 0;  // read back with stx_buf_flags
        out_packed[i] = packed[i].release();
    }
    return STX_OK;
}

STX_EXPORT int stx_blend_build(stx_blender* b)
{
    if (!b) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return STX_OK;
    if (b->finished) return stx_fail(STX_ERR_STATE, "build after blend()");
    if (!b->ctx) return stx_fail(STX_ERR_STATE, "geometry-only blender (created without a context)");
    STX_TRY(stx_set_device(b->ctx));
    return mb_ensure_pyramids(b);
}

STX_EXPORT int stx_blend_feed_contrib_ex(stx_blender* b, int order, const int rect_xywh[4], const stx_buf* packed, int flags)
{
    if (!b || !rect_xywh || !packed) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->kind != STX_BLEND_MULTIBAND) return stx_fail(STX_ERR_UNSUPPORTED, "multi-band blender only");
    if (b->finished) return stx_fail(STX_ERR_STATE, "feed after blend()");
    if (b->adopted) return stx_fail(STX_ERR_STATE, "feed after stx_blend_use_weights adopted weights");
    if (!b->ctx) return stx_fail(STX_ERR_STATE, "geometry-only blender (created without a context)");
    const int nb = b->num_bands, al = (1 << nb) - 1;
    const int x = rect_xywh[0], y = rect_xywh[1], w = rect_xywh[2], h = rect_xywh[3];
    if (w <= 0 || h <= 0 || ((x | y | w | h) & al) || x < 0 || y < 0 || x + w > b->rw || y + h > b->rh)
        return stx_fail(STX_ERR_INVALID, "contribution rect (%d,%d,%d,%d) is not a 2^bands-aligned part of the roi", x, y, w, h);
    ContribLayout L;
    mb_contrib_layout(nb, w, h, &L);
    if (packed->elem != STX_U8 || packed->c != 1 || packed->stride * (size_t)packed->h < L.bytes)
        return stx_fail(STX_ERR_INVALID, "contribution buffer holds %zu bytes, layout needs %zu", packed->stride * (size_t)packed->h, L.bytes);
    StxMbImage im;
    memset(&im, 0, sizeof(im));
    im.kind = 1;
    im.order = order;
    im.mask_binary = (flags & STX_CONTRIB_U8_BINARY) ? 1 : 0;
    im.fx = x; im.fy = y; im.fw = w; im.fh = h;
    for (int i = 0; i <= nb; i++) {
        im.g[i] = (short*)(packed->ptr + L.g_off[i]); im.g_stride[i] = L.g_stride[i];
        im.g_plane[i] = L.g_stride[i] * std::max(h >> i, 1);
        im.wt[i] = (float*)(packed->ptr + L.w_off[i]); im.wt_stride[i] = L.w_stride[i];
    }
    mb_insert_sorted(b, im, true);
    b->next_order = std::max(b->next_order, order + 1);
    stx_buf_retain(const_cast<stx_buf*>(packed));
    b->held.push_back(const_cast<stx_buf*>(packed));
    return STX_OK;
}

// FeatherBlender::blend: weights of all fed images (batched distance transforms), then one gather over the panorama
static int feather_finish(stx_blender* b, stx_buf* pano, stx_buf* pmask, stx_buf* p16)
{
    stx_ctx* ctx = b->ctx;
    const int n = (int)b->feather_images.size();
    StxDevBlock tab;
    STX_TRY(upload_small(ctx, b->feather_images.data(), sizeof(FeatherImg) * (size_t)n, &tab));
    void* const d_tab = tab.release();  // the blender's from here
    b->pyr_allocs.push_back(d_tab);
    STX_TRY(stx_launch_feather_weights(ctx, (const FeatherImg*)d_tab, b->feather_images.data(), n));
    double bytes = 4.0 * pano->w * pano->h + (p16 ? 6.0 * pano->w * pano->h : 0.0);
    for (const FeatherImg& im : b->feather_images) bytes += (double)im.w * im.h * ((im.is_s16 ? 6 : 3) + 2);
    FeatherGatherK K;
    K.imgs = (const FeatherImg*)d_tab; K.n = n; K.w = pano->w; K.h = pano->h; K.sharpness = b->sharpness;
    K.pano = pano->ptr; K.pano_stride = (long long)pano->stride; K.pmask = pmask->ptr; K.pmask_stride = (long long)pmask->stride;
    K.pano16 = p16 ? (short*)p16->ptr : nullptr; K.pano16_stride = p16 ? (long long)p16->stride : 0;
    return stx_launch_feather_gather(ctx, K, bytes);
}

// Blender::blend of the "no" blender: one gather over the panorama (stx_blend.hip: no_gather_kernel)
static int no_finish(stx_blender* b, stx_buf* pano, stx_buf* pmask, stx_buf* p16)
{
    stx_ctx* ctx = b->ctx;
    const int n = (int)b->no_images.size();
    void* d_tab = nullptr;
    STX_TRY(stx_dev_alloc(ctx, sizeof(NoImg) * std::max(n, 1), &d_tab));
    b->pyr_allocs.push_back(d_tab);
    bool all_binary = true;
    double bytes = 4.0 * pano->w * pano->h + (p16 ? 6.0 * pano->w * pano->h : 0.0);
    for (const NoImg& im : b->no_images) {
        all_binary = all_binary && im.mask_binary;
        bytes += (double)im.w * im.h;  // every mask once; the image bytes of the winners are counted with the output
    }
    bytes += 3.0 * pano->w * pano->h;
    if (n > 0) STX_TRY(stx_stage_upload(ctx, d_tab, b->no_images.data(), sizeof(NoImg) * (size_t)n));
    NoGatherK K;
    K.imgs = (const NoImg*)d_tab; K.n = n; K.all_binary = all_binary ? 1 : 0;
    K.w = pano->w; K.h = pano->h;
    K.pano = pano->ptr; K.pano_stride = (long long)pano->stride; K.pmask = pmask->ptr; K.pmask_stride = (long long)pmask->stride;
    K.pano16 = p16 ? (short*)p16->ptr : nullptr; K.pano16_stride = p16 ? (long long)p16->stride : 0;
    return stx_launch_no_gather(ctx, K, bytes);
}

STX_EXPORT int stx_blend_finish_ex(stx_blender* b, stx_buf** out_pano_u8, stx_buf** out_mask_u8, stx_buf** out_pano_s16)
{
    if (!b) return stx_fail(STX_ERR_INVALID, "null argument");
    if (b->finished) return stx_fail(STX_ERR_STATE, "blend() was already called on this blender");
    if (!b->ctx) return stx_fail(STX_ERR_STATE, "geometry-only blender (created without a context)");
    STX_TRY(stx_set_device(b->ctx));
    stx_ctx* ctx = b->ctx;
    ctx->blend_replayed = 0;
    ctx->blend_uploads = 0;
    ctx->blend_mask_stored = 0;
    const int ow = b->kind == STX_BLEND_MULTIBAND ? b->band_x1 - b->band_x0 : b->rw, oh = b->kind == STX_BLEND_MULTIBAND ? b->fh : b->rh;
    StxBufRef p16, pmask, pano;  // (what the caller does not take is released in the order pano, pmask, p16)
    const int rc = [&]() {
        STX_TRY(stx_buf_new(ctx, ow, oh, 3, STX_U8, &pano));
        if (b->kind != STX_BLEND_MULTIBAND) STX_TRY(stx_buf_new(ctx, ow, oh, 1, STX_U8, &pmask));  // (multi-band: mb_finish's, or the rig's)
        if (out_pano_s16) STX_TRY(stx_buf_new(ctx, ow, oh, 3, STX_S16, &p16));
        if (b->kind == STX_BLEND_MULTIBAND) return mb_finish(b, pano.get(), &pmask, p16.get());
        if (b->kind == STX_BLEND_NO) return no_finish(b, pano.get(), pmask.get(), p16.get());
        return feather_finish(b, pano.get(), pmask.get(), p16.get());
    }();
    if (rc == STX_OK && b->kind == STX_BLEND_MULTIBAND) mb_hand_over_weights(b, pmask.get());
    // whatever the outcome, the blender is spent
    b->finished = true;
    blender_release(b);  // stream-ordered: the kernels above were enqueued before any reuse
    STX_TRY(rc);
    if (out_pano_u8) *out_pano_u8 = pano.release();
    if (out_mask_u8) *out_mask_u8 = pmask.release();
    if (out_pano_s16) *out_pano_s16 = p16.release();
    return STX_OK;
}

STX_EXPORT int stx_blend_finish(stx_blender* b, stx_buf** out_pano_u8, stx_buf** out_mask_u8)
{
    return stx_blend_finish_ex(b, out_pano_u8, out_mask_u8, nullptr);
}

STX_EXPORT int stx_blend_destroy(stx_blender* b)
{
    if (!b) return STX_OK;
    if (b->ctx) {
        hipSetDevice(b->ctx->device);
        blender_release(b);
    }
    delete b;
    return STX_OK;
}
