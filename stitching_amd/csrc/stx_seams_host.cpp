// stx_seams_host.cpp — host side of seam finding (SeamFinder::find for "voronoi" and "no"): PairwiseSeamFinder::run's pairs, their
// dependency levels, the result buffers and the launches of stx_seams.hip.  tests/numpy_seams.py is the contract.  The same pairs and
// levels drive the project's own colour-aware finder (stx_color_seam_find, stx_color_seams.hip; contract: tests/numpy_color_seams.py).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "stx_internal.h"

namespace {

struct SeamPlanPair { int i, j, x, y, w, h, level; };

struct Rect { int x0, y0, x1, y1; };
bool meets(const Rect& a, const Rect& b) { return a.x0 < b.x1 && b.x0 < a.x1 && a.y0 < b.y1 && b.y0 < a.y1; }
Rect clip(const Rect& a, const Rect& b) { return {std::max(a.x0, b.x0), std::max(a.y0, b.y0), std::min(a.x1, b.x1), std::min(a.y1, b.y1)}; }

// run()'s pairs in order with their overlapRoi, and each pair's level: 0 without dependencies, else 1 + the highest level of the earlier
// pairs it depends on.  q depends on an earlier p when they share an image k and, in k, the write region of one (its roi) meets the
// read window of the other (roi +- gap, clipped to k).  Pairs of one level then touch disjoint pixels of every image, and running the
// levels in order gives the sequential result.
int seam_plan(int n, const int* sizes, const int* corners, std::vector<SeamPlanPair>& out, int* nlevels)
{
    if (n < 0 || (n > 0 && (!sizes || !corners))) return stx_fail(STX_ERR_INVALID, "bad argument");
    for (int k = 0; k < n; k++)
        if (sizes[2 * k] <= 0 || sizes[2 * k + 1] <= 0) return stx_fail(STX_ERR_INVALID, "image %d has no pixels", k);
    auto rect = [&](int k) {
        return Rect{corners[2 * k], corners[2 * k + 1], corners[2 * k] + sizes[2 * k], corners[2 * k + 1] + sizes[2 * k + 1]};
    };
    out.clear();
    for (int i = 0; i + 1 < n; i++)
        for (int j = i + 1; j < n; j++) {
            const Rect r = clip(rect(i), rect(j));
            if (r.x0 < r.x1 && r.y0 < r.y1) out.push_back({i, j, r.x0, r.y0, r.x1 - r.x0, r.y1 - r.y0, 0});
        }
    const int g = STX_SEAM_GAP;
    int levels = out.empty() ? 0 : 1;
    for (size_t q = 0; q < out.size(); q++) {
        SeamPlanPair& Q = out[q];
        const Rect wq{Q.x, Q.y, Q.x + Q.w, Q.y + Q.h}, rq{Q.x - g, Q.y - g, Q.x + Q.w + g, Q.y + Q.h + g};
        for (size_t p = 0; p < q; p++) {
            const SeamPlanPair& Pp = out[p];
            if (Pp.level < Q.level) continue;  // cannot raise Q's level
            const Rect wp{Pp.x, Pp.y, Pp.x + Pp.w, Pp.y + Pp.h}, rp{Pp.x - g, Pp.y - g, Pp.x + Pp.w + g, Pp.y + Pp.h + g};
            const int shared[2] = {Q.i, Q.j};
            for (int k : shared) {
                if (k != Pp.i && k != Pp.j) continue;
                const Rect img = rect(k);
                if (meets(wp, clip(rq, img)) || meets(wq, clip(rp, img))) {
                    Q.level = Pp.level + 1;
                    break;
                }
            }
        }
        levels = std::max(levels, Q.level + 1);
    }
    *nlevels = levels;
    return STX_OK;
}

// The frame both finders share.  Members go in the reverse order of their declaration: the guard's wait first, behind it the pair table,
// the arena, the events and, on a failure, the results.
struct SeamRun {
    stx_ctx* ctx;
    std::vector<StxBufRef> outs;  // handed to masks_out at the end
    StxEventTimer timer;          // start, masks copied, levels queued
    StxDevBlock d_arena, d_pairs;
    StxRunGuard wait;
    SeamRun(stx_ctx* c, int n) : ctx(c), outs(n), wait(c) {}
};

// n, the pointers and every mask — with `images` (with_images) every image as well —: type, size, context
int seam_check(stx_ctx* ctx, int n, const int* sizes_wh, const int* corners_xy, bool with_images, const stx_buf* const* images,
               const stx_buf* const* masks_in, stx_buf** masks_out)
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (n < 0 || (n > 0 && (!sizes_wh || !corners_xy || (with_images && !images) || !masks_in || !masks_out)))
        return stx_fail(STX_ERR_INVALID, "bad argument");
    for (int k = 0; k < n; k++) {
        const stx_buf* m = masks_in[k];
        const stx_buf* im = with_images ? images[k] : nullptr;
        const int w = sizes_wh[2 * k], h = sizes_wh[2 * k + 1];
        if (!m) return stx_fail(STX_ERR_INVALID, "null mask %d", k);
        if (with_images && !im) return stx_fail(STX_ERR_INVALID, "null image %d", k);
        if (m->elem != STX_U8 || m->c != 1) return stx_fail(STX_ERR_INVALID, "seam finding needs u8x1 masks (mask %d)", k);
        if (im && (im->elem != STX_U8 || im->c != 3)) return stx_fail(STX_ERR_INVALID, "colour seams need u8x3 images (image %d)", k);
        if (m->w != w || m->h != h) return stx_fail(STX_ERR_INVALID, "mask %d is %dx%d, its image %dx%d", k, m->w, m->h, w, h);
        if (im && (im->w != w || im->h != h))
            return stx_fail(STX_ERR_INVALID, "image %d is %dx%d, its size is given as %dx%d", k, im->w, im->h, w, h);
        if (m->ctx != ctx) return stx_fail(STX_ERR_INVALID, "mask %d belongs to another context", k);
        if (im && im->ctx != ctx) return stx_fail(STX_ERR_INVALID, "image %d belongs to another context", k);
    }
    return STX_OK;
}

// what the caller learns of the plan, and no results yet
void seam_report(const std::vector<SeamPlanPair>& plan, int nlevels, int n, stx_buf** masks_out, double* out_info)
{
    if (out_info) { out_info[0] = (double)plan.size(); out_info[1] = nlevels; out_info[2] = 0.0; out_info[3] = 0.0; }
    for (int k = 0; k < n; k++) masks_out[k] = nullptr;
}

// the results: copies of the inputs (the caller's masks are never written)
int seam_copy_masks(SeamRun& X, int n, const stx_buf* const* masks_in, bool timed)
{
    stx_ctx* ctx = X.ctx;
    if (timed) STX_TRY(X.timer.arm(3));
    STX_TRY(X.timer.mark(0, ctx->stream));
    for (int k = 0; k < n; k++) {
        const stx_buf* m = masks_in[k];
        STX_TRY(stx_buf_new(ctx, m->w, m->h, 1, STX_U8, &X.outs[k]));
        X.outs[k]->mask_binary = m->mask_binary;  // zeroing keeps a 0 / 255 mask binary
        if (hipMemcpy2DAsync(X.outs[k]->ptr, X.outs[k]->stride, m->ptr, m->stride, (size_t)m->w, m->h, hipMemcpyDeviceToDevice,
                             ctx->stream) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "hipMemcpy2DAsync of a seam mask failed");
    }
    return X.timer.mark(1, ctx->stream);
}

// pairs grouped by level (stable: run() order inside a level): order[t] is the pair of table row t, level l has the rows
// lstart[l] .. lstart[l + 1]
void seam_group_levels(const std::vector<SeamPlanPair>& plan, int nlevels, std::vector<int>& order, std::vector<int>& lstart)
{
    order.resize(plan.size());
    for (size_t p = 0; p < plan.size(); p++) order[p] = (int)p;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return plan[a].level < plan[b].level; });
    lstart.assign(nlevels + 1, 0);
    for (const SeamPlanPair& P : plan) lstart[P.level + 1]++;
    for (int l = 0; l < nlevels; l++) lstart[l + 1] += lstart[l];
}

// the pair table on the device and one arena, of the largest level
int seam_upload(SeamRun& X, const void* tab, size_t tab_bytes, size_t arena_bytes)
{
    STX_TRY(stx_dev_alloc(X.ctx, tab_bytes, &X.d_pairs));
    STX_TRY(stx_dev_alloc(X.ctx, arena_bytes, &X.d_arena));
    if (hipMemcpyAsync(X.d_pairs.get(), tab, tab_bytes, hipMemcpyHostToDevice, X.ctx->stream) != hipSuccess)
        return stx_fail(STX_ERR_HIP, "seam pair table upload failed");
    return STX_OK;
}

// the one wait, the two times, and the results are the caller's
int seam_finish(SeamRun& X, const char* what, int n, stx_buf** masks_out, double* out_info)
{
    STX_TRY(X.timer.mark(2, X.ctx->stream));
    if (hipStreamSynchronize(X.ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "%s failed", what);
    if (out_info) {
        STX_TRY(X.timer.ms(1, 2, &out_info[2]));
        STX_TRY(X.timer.ms(0, 2, &out_info[3]));
    }
    for (int k = 0; k < n; k++) masks_out[k] = X.outs[k].release();
    return STX_OK;
}

}  // namespace

STX_EXPORT int stx_seam_schedule(int n, const int* sizes_wh, const int* corners_xy, int* inout_npairs, int* out_pairs, int* out_levels)
{
    if (!inout_npairs) return stx_fail(STX_ERR_INVALID, "inout_npairs is null");
    std::vector<SeamPlanPair> plan;
    int nlevels = 0;
    STX_TRY(seam_plan(n, sizes_wh, corners_xy, plan, &nlevels));
    const int np = (int)plan.size();
    if (!out_pairs) { *inout_npairs = np; return STX_OK; }
    if (*inout_npairs < np || !out_levels) return stx_fail(STX_ERR_INVALID, "output arrays hold %d pairs, %d needed", *inout_npairs, np);
    for (int p = 0; p < np; p++) {
        const SeamPlanPair& P = plan[p];
        const int v[6] = {P.i, P.j, P.x, P.y, P.w, P.h};
        for (int k = 0; k < 6; k++) out_pairs[6 * p + k] = v[k];
        out_levels[p] = P.level;
    }
    *inout_npairs = np;
    return STX_OK;
}

STX_EXPORT int stx_seam_find(stx_ctx* ctx, int kind, int n, const int* sizes_wh, const int* corners_xy, const stx_buf* const* masks_in,
                             stx_buf** masks_out, double out_info[4])
{
    if (kind != STX_SEAM_NO && kind != STX_SEAM_VORONOI) return stx_fail(STX_ERR_INVALID, "unknown seam finder kind %d", kind);
    STX_TRY(seam_check(ctx, n, sizes_wh, corners_xy, false, nullptr, masks_in, masks_out));
    std::vector<SeamPlanPair> plan;
    int nlevels = 0;
    if (kind == STX_SEAM_VORONOI) STX_TRY(seam_plan(n, sizes_wh, corners_xy, plan, &nlevels));  // "no": the copies are the result
    seam_report(plan, nlevels, n, masks_out, out_info);
    if (n == 0) return STX_OK;  // nothing to copy or cut: the device is not touched
    STX_TRY(stx_set_device(ctx));
    SeamRun X(ctx, n);
    STX_TRY(seam_copy_masks(X, n, masks_in, out_info != nullptr));
    if (!plan.empty()) {
        // arena offsets per level
        std::vector<int> order, lstart;
        seam_group_levels(plan, nlevels, order, lstart);
        std::vector<StxSeamPair> tab(plan.size());
        std::vector<int> lrows(nlevels, 0), lcols(nlevels, 0);
        std::vector<long long> lsize(nlevels, 0);
        std::vector<double> lbytes(nlevels, 0.0);
        const int g = STX_SEAM_GAP;
        for (size_t t = 0; t < order.size(); t++) {
            const SeamPlanPair& P = plan[order[t]];
            const stx_buf* a = X.outs[P.i].get();
            const stx_buf* b = X.outs[P.j].get();
            StxSeamPair& S = tab[t];
            S.m1 = a->ptr; S.s1 = (long long)a->stride; S.w1 = a->w; S.h1 = a->h;
            S.m2 = b->ptr; S.s2 = (long long)b->stride; S.w2 = b->w; S.h2 = b->h;
            S.ox1 = P.x - g - corners_xy[2 * P.i]; S.oy1 = P.y - g - corners_xy[2 * P.i + 1];
            S.ox2 = P.x - g - corners_xy[2 * P.j]; S.oy2 = P.y - g - corners_xy[2 * P.j + 1];
            S.ww = P.w + 2 * g; S.wh = P.h + 2 * g; S.rw = P.w; S.rh = P.h;
            // the roi (written unchecked by the column kernel) lies inside both images
            if (S.ox1 + g < 0 || S.oy1 + g < 0 || S.ox1 + g + P.w > a->w || S.oy1 + g + P.h > a->h || S.ox2 + g < 0 || S.oy2 + g < 0 ||
                S.ox2 + g + P.w > b->w || S.oy2 + g + P.h > b->h)
                return stx_fail(STX_ERR_INVALID, "internal: seam roi outside its images");
            S.off = lsize[P.level];
            lsize[P.level] += 2ll * S.wh * S.rw;
            lrows[P.level] = std::max(lrows[P.level], S.wh);
            lcols[P.level] = std::max(lcols[P.level], S.rw);
            lbytes[P.level] += 2.0 * S.ww * S.wh + 12.0 * S.wh * S.rw + (double)S.rw * S.rh;
        }
        const long long arena = *std::max_element(lsize.begin(), lsize.end());
        STX_TRY(seam_upload(X, tab.data(), sizeof(StxSeamPair) * tab.size(), sizeof(uint16_t) * (size_t)arena));
        const StxSeamPair* d_pairs = (const StxSeamPair*)X.d_pairs.get();
        for (int l = 0; l < nlevels; l++)
            STX_TRY(stx_launch_seam_level(ctx, d_pairs + lstart[l], lstart[l + 1] - lstart[l], lrows[l], lcols[l], (uint16_t*)X.d_arena.get(),
                                          lbytes[l]));
    }
    return seam_finish(X, "seam finding", n, masks_out, out_info);
}

// The project's own colour-aware finder (tests/numpy_color_seams.py is the contract; not OpenCV's DpSeamFinder): the same pairs, the same
// levels — a pair reads its roi without a gap, which the schedule's windows contain — and stx_color_seams.hip's two launches per level.
STX_EXPORT int stx_color_seam_find(stx_ctx* ctx, int n, const int* sizes_wh, const int* corners_xy, const stx_buf* const* images,
                                   const stx_buf* const* masks_in, stx_buf** masks_out, double out_info[4])
{
    STX_TRY(seam_check(ctx, n, sizes_wh, corners_xy, true, images, masks_in, masks_out));
    std::vector<SeamPlanPair> plan;
    int nlevels = 0;
    STX_TRY(seam_plan(n, sizes_wh, corners_xy, plan, &nlevels));
    // orientation and limits of every pair, before anything is allocated or launched
    struct Geo { int L, W, vertical, first_is_i; };
    std::vector<Geo> geo(plan.size());
    for (size_t p = 0; p < plan.size(); p++) {
        const SeamPlanPair& P = plan[p];
        const long long dx = (2ll * corners_xy[2 * P.i] + sizes_wh[2 * P.i]) - (2ll * corners_xy[2 * P.j] + sizes_wh[2 * P.j]);
        const long long dy = (2ll * corners_xy[2 * P.i + 1] + sizes_wh[2 * P.i + 1]) - (2ll * corners_xy[2 * P.j + 1] + sizes_wh[2 * P.j + 1]);
        Geo& G = geo[p];
        G.vertical = std::llabs(dx) >= std::llabs(dy);
        G.first_is_i = (G.vertical ? dx : dy) <= 0;
        G.L = G.vertical ? P.h : P.w;
        G.W = G.vertical ? P.w : P.h;
        if (G.L > STX_COLOR_SEAM_MAX_LENGTH)
            return stx_fail(STX_ERR_INVALID, "colour seam of images %d and %d: a %s seam of %d pixels, at most %d (u32 accumulators)", P.i, P.j,
                            G.vertical ? "vertical" : "horizontal", G.L, STX_COLOR_SEAM_MAX_LENGTH);
        if (G.W > STX_COLOR_SEAM_MAX_CROSS)
            return stx_fail(STX_ERR_INVALID, "colour seam of images %d and %d: %d pixels across the %s seam, at most %d (accumulator rows in LDS)",
                            P.i, P.j, G.W, G.vertical ? "vertical" : "horizontal", STX_COLOR_SEAM_MAX_CROSS);
    }
    seam_report(plan, nlevels, n, masks_out, out_info);
    if (n == 0) return STX_OK;  // nothing to copy or cut: the device is not touched
    STX_TRY(stx_set_device(ctx));
    SeamRun X(ctx, n);
    STX_TRY(seam_copy_masks(X, n, masks_in, out_info != nullptr));
    if (!plan.empty()) {
        std::vector<int> order, lstart;
        seam_group_levels(plan, nlevels, order, lstart);
        std::vector<StxColorSeamPair> tab(plan.size());
        std::vector<int> lcross(nlevels, 0);
        std::vector<long long> lsize(nlevels, 0), larea(nlevels, 0);
        std::vector<double> lbytes(nlevels, 0.0);
        for (size_t t = 0; t < order.size(); t++) {
            const SeamPlanPair& P = plan[order[t]];
            const Geo& G = geo[order[t]];
            const stx_buf* ia = images[P.i];
            const stx_buf* ib = images[P.j];
            const stx_buf* a = X.outs[P.i].get();
            const stx_buf* b = X.outs[P.j].get();
            const int xa = P.x - corners_xy[2 * P.i], ya = P.y - corners_xy[2 * P.i + 1];
            const int xb = P.x - corners_xy[2 * P.j], yb = P.y - corners_xy[2 * P.j + 1];
            // the roi (read and written unchecked by the kernels) lies inside both images
            if (xa < 0 || ya < 0 || xa + P.w > a->w || ya + P.h > a->h || xb < 0 || yb < 0 || xb + P.w > b->w || yb + P.h > b->h)
                return stx_fail(STX_ERR_INVALID, "internal: seam roi outside its images");
            StxColorSeamPair& S = tab[t];
            S.si1 = (long long)ia->stride; S.si2 = (long long)ib->stride; S.sm1 = (long long)a->stride; S.sm2 = (long long)b->stride;
            S.i1 = ia->ptr + ya * S.si1 + 3ll * xa; S.i2 = ib->ptr + yb * S.si2 + 3ll * xb;
            S.m1 = a->ptr + ya * S.sm1 + xa; S.m2 = b->ptr + yb * S.sm2 + xb;
            S.L = G.L; S.W = G.W; S.vertical = G.vertical; S.first_is_i = G.first_is_i;
            const long long area = (long long)G.L * G.W;
            S.off_choice = lsize[P.level];
            S.off_seam = (long long)align_up((size_t)(S.off_choice + area), 4);
            lsize[P.level] = S.off_seam + 4ll * G.L;
            lcross[P.level] = std::max(lcross[P.level], G.W);
            larea[P.level] = std::max(larea[P.level], area);
            lbytes[P.level] += 8.0 * area + 2.0 * area + 2.0 * area;  // images and masks, the choices (written, read back at most once), the masks again
        }
        const long long arena = *std::max_element(lsize.begin(), lsize.end());
        STX_TRY(seam_upload(X, tab.data(), sizeof(StxColorSeamPair) * tab.size(), (size_t)arena));
        const StxColorSeamPair* d_pairs = (const StxColorSeamPair*)X.d_pairs.get();
        for (int l = 0; l < nlevels; l++)
            STX_TRY(stx_launch_color_seam_level(ctx, d_pairs + lstart[l], lstart[l + 1] - lstart[l], lcross[l], larea[l], (uint8_t*)X.d_arena.get(),
                                                lbytes[l]));
    }
    return seam_finish(X, "colour seam finding", n, masks_out, out_info);
}
