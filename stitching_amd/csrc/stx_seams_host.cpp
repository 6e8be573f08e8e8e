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

struct SeamRun {
    stx_ctx* ctx = nullptr;
    StxDevBlock d_pairs, d_arena;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~SeamRun()
    {
        if (!ctx) return;
        hipStreamSynchronize(ctx->stream);
        d_pairs.reset();  // behind the synchronisation
        d_arena.reset();
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    }
};

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
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (n < 0 || (n > 0 && (!sizes_wh || !corners_xy || !masks_in || !masks_out))) return stx_fail(STX_ERR_INVALID, "bad argument");
    for (int k = 0; k < n; k++) {
        const stx_buf* m = masks_in[k];
        if (!m) return stx_fail(STX_ERR_INVALID, "null mask %d", k);
        if (m->elem != STX_U8 || m->c != 1) return stx_fail(STX_ERR_INVALID, "seam finding needs u8x1 masks (mask %d)", k);
        if (m->w != sizes_wh[2 * k] || m->h != sizes_wh[2 * k + 1])
            return stx_fail(STX_ERR_INVALID, "mask %d is %dx%d, its image %dx%d", k, m->w, m->h, sizes_wh[2 * k], sizes_wh[2 * k + 1]);
        if (m->ctx != ctx) return stx_fail(STX_ERR_INVALID, "mask %d belongs to another context", k);
    }
    std::vector<SeamPlanPair> plan;
    int nlevels = 0;
    if (kind == STX_SEAM_VORONOI) STX_TRY(seam_plan(n, sizes_wh, corners_xy, plan, &nlevels));
    if (out_info) { out_info[0] = (double)plan.size(); out_info[1] = nlevels; out_info[2] = 0.0; out_info[3] = 0.0; }
    for (int k = 0; k < n; k++) masks_out[k] = nullptr;
    if (n == 0) return STX_OK;
    STX_TRY(stx_set_device(ctx));
    std::vector<StxBufRef> outs(n);  // handed to masks_out at the end; on a failure released behind X's synchronisation
    SeamRun X;
    X.ctx = ctx;
    if (out_info) {
        for (hipEvent_t& e : X.ev)
            if (hipEventCreate(&e) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventCreate failed");
        if (hipEventRecord(X.ev[0], ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventRecord failed");
    }
    // the results: copies of the inputs (the caller's masks are never written)
    for (int k = 0; k < n; k++) {
        const stx_buf* m = masks_in[k];
        STX_TRY(stx_buf_new(ctx, m->w, m->h, 1, STX_U8, &outs[k]));
        outs[k]->mask_binary = m->mask_binary;  // zeroing keeps a 0 / 255 mask binary
        if (hipMemcpy2DAsync(outs[k]->ptr, outs[k]->stride, m->ptr, m->stride, (size_t)m->w, m->h, hipMemcpyDeviceToDevice,
                             ctx->stream) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "hipMemcpy2DAsync of a seam mask failed");
    }
    if (out_info && hipEventRecord(X.ev[1], ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventRecord failed");
    if (!plan.empty()) {
        // pairs grouped by level (stable: run() order inside a level), arena offsets per level, one arena of the largest level
        std::vector<int> order(plan.size());
        for (size_t p = 0; p < plan.size(); p++) order[p] = (int)p;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return plan[a].level < plan[b].level; });
        std::vector<StxSeamPair> tab(plan.size());
        std::vector<int> lstart(nlevels + 1, 0), lrows(nlevels, 0), lcols(nlevels, 0);
        std::vector<long long> lsize(nlevels, 0);
        std::vector<double> lbytes(nlevels, 0.0);
        const int g = STX_SEAM_GAP;
        for (size_t t = 0; t < order.size(); t++) {
            const SeamPlanPair& P = plan[order[t]];
            const stx_buf* a = outs[P.i].get();
            const stx_buf* b = outs[P.j].get();
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
            lstart[P.level + 1]++;
            lrows[P.level] = std::max(lrows[P.level], S.wh);
            lcols[P.level] = std::max(lcols[P.level], S.rw);
            lbytes[P.level] += 2.0 * S.ww * S.wh + 12.0 * S.wh * S.rw + (double)S.rw * S.rh;
        }
        for (int l = 0; l < nlevels; l++) lstart[l + 1] += lstart[l];
        const long long arena = *std::max_element(lsize.begin(), lsize.end());
        STX_TRY(stx_dev_alloc(ctx, sizeof(StxSeamPair) * tab.size(), &X.d_pairs));
        STX_TRY(stx_dev_alloc(ctx, sizeof(uint16_t) * (size_t)arena, &X.d_arena));
        const StxSeamPair* d_pairs = (const StxSeamPair*)X.d_pairs.get();
        if (hipMemcpyAsync(X.d_pairs.get(), tab.data(), sizeof(StxSeamPair) * tab.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "seam pair table upload failed");
        for (int l = 0; l < nlevels; l++)
            STX_TRY(stx_launch_seam_level(ctx, d_pairs + lstart[l], lstart[l + 1] - lstart[l], lrows[l], lcols[l], (uint16_t*)X.d_arena.get(),
                                          lbytes[l]));
    }
    if (out_info && hipEventRecord(X.ev[2], ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventRecord failed");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "seam finding failed");
    if (out_info) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, X.ev[1], X.ev[2]) != hipSuccess || hipEventElapsedTime(&b, X.ev[0], X.ev[2]) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "hipEventElapsedTime failed");
        out_info[2] = a;
        out_info[3] = b;
    }
    for (int k = 0; k < n; k++) masks_out[k] = outs[k].release();
    return STX_OK;
}

// The project's own colour-aware finder (tests/numpy_color_seams.py is the contract; not OpenCV's DpSeamFinder): the same pairs, the same
// levels — a pair reads its roi without a gap, which the schedule's windows contain — and stx_color_seams.hip's two launches per level.
STX_EXPORT int stx_color_seam_find(stx_ctx* ctx, int n, const int* sizes_wh, const int* corners_xy, const stx_buf* const* images,
                                   const stx_buf* const* masks_in, stx_buf** masks_out, double out_info[4])
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (n < 0 || (n > 0 && (!sizes_wh || !corners_xy || !images || !masks_in || !masks_out))) return stx_fail(STX_ERR_INVALID, "bad argument");
    for (int k = 0; k < n; k++) {
        const stx_buf* m = masks_in[k];
        const stx_buf* im = images[k];
        if (!m) return stx_fail(STX_ERR_INVALID, "null mask %d", k);
        if (!im) return stx_fail(STX_ERR_INVALID, "null image %d", k);
        if (m->elem != STX_U8 || m->c != 1) return stx_fail(STX_ERR_INVALID, "seam finding needs u8x1 masks (mask %d)", k);
        if (im->elem != STX_U8 || im->c != 3) return stx_fail(STX_ERR_INVALID, "colour seams need u8x3 images (image %d)", k);
        if (m->w != sizes_wh[2 * k] || m->h != sizes_wh[2 * k + 1])
            return stx_fail(STX_ERR_INVALID, "mask %d is %dx%d, its image %dx%d", k, m->w, m->h, sizes_wh[2 * k], sizes_wh[2 * k + 1]);
        if (im->w != sizes_wh[2 * k] || im->h != sizes_wh[2 * k + 1])
            return stx_fail(STX_ERR_INVALID, "image %d is %dx%d, its size is given as %dx%d", k, im->w, im->h, sizes_wh[2 * k], sizes_wh[2 * k + 1]);
        if (m->ctx != ctx) return stx_fail(STX_ERR_INVALID, "mask %d belongs to another context", k);
        if (im->ctx != ctx) return stx_fail(STX_ERR_INVALID, "image %d belongs to another context", k);
    }
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
    if (out_info) { out_info[0] = (double)plan.size(); out_info[1] = nlevels; out_info[2] = 0.0; out_info[3] = 0.0; }
    for (int k = 0; k < n; k++) masks_out[k] = nullptr;
    if (n == 0) return STX_OK;
    STX_TRY(stx_set_device(ctx));
    std::vector<StxBufRef> outs(n);  // handed to masks_out at the end; on a failure released behind X's synchronisation
    SeamRun X;
    X.ctx = ctx;
    if (out_info) {
        for (hipEvent_t& e : X.ev)
            if (hipEventCreate(&e) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventCreate failed");
        if (hipEventRecord(X.ev[0], ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventRecord failed");
    }
    for (int k = 0; k < n; k++) {
        const stx_buf* m = masks_in[k];
        STX_TRY(stx_buf_new(ctx, m->w, m->h, 1, STX_U8, &outs[k]));
        outs[k]->mask_binary = m->mask_binary;  // zeroing keeps a 0 / 255 mask binary
        if (hipMemcpy2DAsync(outs[k]->ptr, outs[k]->stride, m->ptr, m->stride, (size_t)m->w, m->h, hipMemcpyDeviceToDevice,
                             ctx->stream) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "hipMemcpy2DAsync of a seam mask failed");
    }
    if (out_info && hipEventRecord(X.ev[1], ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventRecord failed");
    if (!plan.empty()) {
        std::vector<int> order(plan.size());
        for (size_t p = 0; p < plan.size(); p++) order[p] = (int)p;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return plan[a].level < plan[b].level; });
        std::vector<StxColorSeamPair> tab(plan.size());
        std::vector<int> lstart(nlevels + 1, 0), lcross(nlevels, 0);
        std::vector<long long> lsize(nlevels, 0), larea(nlevels, 0);
        std::vector<double> lbytes(nlevels, 0.0);
        for (size_t t = 0; t < order.size(); t++) {
            const SeamPlanPair& P = plan[order[t]];
            const Geo& G = geo[order[t]];
            const stx_buf* ia = images[P.i];
            const stx_buf* ib = images[P.j];
            const stx_buf* a = outs[P.i].get();
            const stx_buf* b = outs[P.j].get();
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
            lstart[P.level + 1]++;
            lcross[P.level] = std::max(lcross[P.level], G.W);
            larea[P.level] = std::max(larea[P.level], area);
            lbytes[P.level] += 8.0 * area + 2.0 * area + 2.0 * area;  // images and masks, the choices (written, read back at most once), the masks again
        }
        for (int l = 0; l < nlevels; l++) lstart[l + 1] += lstart[l];
        const long long arena = *std::max_element(lsize.begin(), lsize.end());
        STX_TRY(stx_dev_alloc(ctx, sizeof(StxColorSeamPair) * tab.size(), &X.d_pairs));
        STX_TRY(stx_dev_alloc(ctx, (size_t)arena, &X.d_arena));
        const StxColorSeamPair* d_pairs = (const StxColorSeamPair*)X.d_pairs.get();
        if (hipMemcpyAsync(X.d_pairs.get(), tab.data(), sizeof(StxColorSeamPair) * tab.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "seam pair table upload failed");
        for (int l = 0; l < nlevels; l++)
            STX_TRY(stx_launch_color_seam_level(ctx, d_pairs + lstart[l], lstart[l + 1] - lstart[l], lcross[l], larea[l], (uint8_t*)X.d_arena.get(),
                                                lbytes[l]));
    }
    if (out_info && hipEventRecord(X.ev[2], ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "hipEventRecord failed");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "colour seam finding failed");
    if (out_info) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, X.ev[1], X.ev[2]) != hipSuccess || hipEventElapsedTime(&b, X.ev[0], X.ev[2]) != hipSuccess)
            return stx_fail(STX_ERR_HIP, "hipEventElapsedTime failed");
        out_info[2] = a;
        out_info[3] = b;
    }
    for (int k = 0; k < n; k++) masks_out[k] = outs[k].release();
    return STX_OK;
}
