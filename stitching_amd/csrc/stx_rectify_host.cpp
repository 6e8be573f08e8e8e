// stx_rectify_host.cpp — lens rectification (stx_lens_map_create / stx_lens_map_free / stx_rectify): the nodes of a camera's lens grid
// in device memory, validation, the descriptor table of one launch.  The kernel is in stx_rectify.hip; DESIGN.md section 22.
#include "stx_internal.h"

namespace {
constexpr int kNodeLimit = 1 << 21;  // |Q6 coordinate|: the contract clips to [-16384 * 64, 32767 * 64], so S stays below 2^30

int nodes_for(int side) { return (side + STX_LENS_CELL - 1) / STX_LENS_CELL + 1; }
}  // namespace

STX_EXPORT int stx_lens_map_create(stx_ctx* ctx, int dst_w, int dst_h, int src_w, int src_h, int nx, int ny, const int* nodes_xy_q6,
                                   stx_lens_map** out)
{
    if (!ctx || !nodes_xy_q6 || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    *out = nullptr;
    if (dst_w < 1 || dst_h < 1 || src_w < 1 || src_h < 1 || dst_w > STX_RECTIFY_MAX_SIDE || dst_h > STX_RECTIFY_MAX_SIDE ||
        src_w > STX_RECTIFY_MAX_SIDE || src_h > STX_RECTIFY_MAX_SIDE)
        return stx_fail(STX_ERR_INVALID, "lens map from %dx%d to %dx%d: sides are 1 .. %d", src_w, src_h, dst_w, dst_h, STX_RECTIFY_MAX_SIDE);
    if (nx != nodes_for(dst_w) || ny != nodes_for(dst_h))
        return stx_fail(STX_ERR_INVALID, "lens map of %d x %d nodes for a %dx%d destination: it takes %d x %d (one every %d pixels, the edges included)",
                        nx, ny, dst_w, dst_h, nodes_for(dst_w), nodes_for(dst_h), STX_LENS_CELL);
    const size_t count = (size_t)nx * ny * 2;
    for (size_t k = 0; k < count; k++)
        if (nodes_xy_q6[k] < -kNodeLimit || nodes_xy_q6[k] > kNodeLimit)
            return stx_fail(STX_ERR_INVALID, "lens map: node %zu holds %d, outside the clip limits of the Q6 coordinates (+- %d)", k / 2, nodes_xy_q6[k],
                            kNodeLimit);
    STX_TRY(stx_set_device(ctx));
    std::unique_ptr<stx_lens_map> M(new stx_lens_map);
    M->ctx = ctx; M->dst_w = dst_w; M->dst_h = dst_h; M->src_w = src_w; M->src_h = src_h; M->nx = nx; M->ny = ny;
    STX_TRY(stx_dev_alloc(ctx, count * sizeof(int), &M->d_nodes));
    STX_HIP(hipMemcpyAsync(M->d_nodes.get(), nodes_xy_q6, count * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));  // the caller's array is free again
    *out = M.release();
    return STX_OK;
}

STX_EXPORT int stx_lens_map_free(stx_lens_map* M)
{
    if (!M) return STX_OK;
    delete M;  // the block goes back to the context's allocator: stream-ordered reuse, launches that read it are ahead in the stream
    return STX_OK;
}

STX_EXPORT int stx_rectify(stx_ctx* ctx, int n, const stx_buf* const* srcs, const stx_lens_map* const* maps, int border, int want_masks,
                           stx_buf** out_imgs, stx_buf** out_masks)
{
    if (!ctx || !srcs || !maps || !out_imgs || (want_masks && !out_masks)) return stx_fail(STX_ERR_INVALID, "null argument");
    if (n <= 0) return stx_fail(STX_ERR_INVALID, "rectify of %d images", n);
    if (border != STX_RECTIFY_CONSTANT && border != STX_RECTIFY_REPLICATE) return stx_fail(STX_ERR_INVALID, "rectify: border %d", border);
    std::vector<StxRectifyItem> items((size_t)n);
    long long tiles = 0;
    double bytes = 0.0;
    for (int i = 0; i < n; i++) {
        const stx_buf* S = srcs[i];
        const stx_lens_map* M = maps[i];
        if (!S) return stx_fail(STX_ERR_INVALID, "rectify: image %d is a null handle", i);
        if (!M) return stx_fail(STX_ERR_INVALID, "rectify: lens map %d is a null handle", i);
        if (S->ctx != ctx || M->ctx != ctx) return stx_fail(STX_ERR_INVALID, "rectify: image or lens map %d belongs to another context", i);
        if (S->elem != STX_U8 || (S->c != 1 && S->c != 3))
            return stx_fail(STX_ERR_INVALID, "rectify: image %d has %d channel(s) of element type %d: u8 with 1 or 3 channels is taken", i, S->c, S->elem);
        if (S->w != M->src_w || S->h != M->src_h)
            return stx_fail(STX_ERR_INVALID, "rectify: image %d is %dx%d, its lens map was made for %dx%d", i, S->w, S->h, M->src_w, M->src_h);
        // the kernel's 32-bit offsets and 24-bit row multiply; an image of the library's own of these sides stays far below both, a
        // view of a very wide parent may not
        if (S->stride >= (size_t)1 << 24 || (unsigned long long)(S->h - 1) * S->stride + (unsigned long long)S->w * S->c + 32 > 0x7fffffffull)
            return stx_fail(STX_ERR_INVALID, "rectify: image %d spans %llu bytes with a pitch of %zu: below 2^31 and 2^24 is taken", i,
                            (unsigned long long)(S->h - 1) * S->stride + (unsigned long long)S->w * S->c, S->stride);
        // sides and node counts were checked when the map was made; the source's are the map's
        StxRectifyItem& K = items[i];
        K = StxRectifyItem{};
        K.src = S->ptr; K.sstride = (long long)S->stride;
        K.nodes = (const int2*)M->d_nodes.get(); K.nx = M->nx;
        K.sw = S->w; K.sh = S->h; K.dw = M->dst_w; K.dh = M->dst_h; K.c = S->c;
        K.tiles_x = (M->dst_w + STX_RECTIFY_TW - 1) / STX_RECTIFY_TW;
        K.tile0 = (int)tiles;
        tiles += (long long)K.tiles_x * ((M->dst_h + STX_RECTIFY_TH - 1) / STX_RECTIFY_TH);
        if (tiles > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "rectify of more than 2^31 tiles");
        // what the pass has to move: the source once, the destination (and the mask) once
        bytes += (double)S->w * S->h * S->c + (double)M->dst_w * M->dst_h * (S->c + (want_masks ? 1 : 0));
    }
    // nothing was allocated or queued up to here
    STX_TRY(stx_set_device(ctx));
    std::vector<StxBufRef> dsts((size_t)n), masks((size_t)n);
    for (int i = 0; i < n; i++) {
        STX_TRY(stx_buf_new(ctx, items[i].dw, items[i].dh, items[i].c, STX_U8, &dsts[i]));
        items[i].dst = dsts[i]->ptr; items[i].dstride = (long long)dsts[i]->stride;
        if (want_masks) {
            STX_TRY(stx_buf_new(ctx, items[i].dw, items[i].dh, 1, STX_U8, &masks[i]));
            items[i].mask = masks[i]->ptr; items[i].mstride = (long long)masks[i]->stride;
            masks[i]->mask_binary = 1;
        }
    }
    StxDevBlock d_items;
    STX_TRY(upload_small(ctx, items.data(), items.size() * sizeof(StxRectifyItem), &d_items));
    STX_TRY(stx_launch_rectify(ctx, (const StxRectifyItem*)d_items.get(), n, (int)tiles, border, bytes));
    for (int i = 0; i < n; i++) {
        out_imgs[i] = dsts[i].release();
        if (want_masks) out_masks[i] = masks[i].release();
    }
    return STX_OK;  // the descriptor block goes back here: stream-ordered reuse
}
