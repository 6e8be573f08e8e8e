// stx_features_host.cpp — host side of FeatureEstimator (the project's own detector, not cv.ORB): argument checks, the pyramid through
// stx_resize_linear_exact_batch, the descriptor tables of the batched kernels (stx_features.hip), the one wait for the candidate
// counts, and the results' way back.  tests/numpy_features.py is the contract; DESIGN.md section 15.
#include <algorithm>
#include <cstring>

#include "stx_internal.h"

STX_EXPORT int stx_features_detect(stx_ctx* ctx, int n, const stx_buf* const* images, const stx_buf* const* masks, int nfeatures, int nlevels,
                                   int fast_threshold, const int* level_counts, const int* level_wh, const int* quotas, const int* cxcy,
                                   const signed char* patterns, int* out_counts, int* out_lxyb, long long* out_R, unsigned char* out_desc,
                                   double out_info[4])
{
    constexpr int ML = STX_FEATURES_MAX_LEVELS;
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (n < 0 || (n > 0 && (!images || !level_counts || !level_wh || !quotas || !cxcy || !patterns || !out_counts || !out_lxyb || !out_R || !out_desc)))
        return stx_fail(STX_ERR_INVALID, "bad argument");
    if (nlevels < 1 || nlevels > ML) return stx_fail(STX_ERR_INVALID, "feature detection with %d levels: 1 .. %d", nlevels, ML);
    if (nfeatures < 1 || nfeatures > STX_FEATURES_MAX_FEATURES)
        return stx_fail(STX_ERR_INVALID, "feature detection with %d features per image: 1 .. %d", nfeatures, STX_FEATURES_MAX_FEATURES);
    if (fast_threshold < 0 || fast_threshold > 255) return stx_fail(STX_ERR_INVALID, "fast threshold %d: 0 .. 255", fast_threshold);
    if (out_info) std::fill(out_info, out_info + 4, 0.0);
    if (n == 0) return STX_OK;
    // every check before anything is allocated or launched
    for (int i = 0; i < n; i++) {
        const stx_buf* im = images[i];
        if (!im) return stx_fail(STX_ERR_INVALID, "null argument");
        if (im->elem != STX_U8 || im->c != 3) return stx_fail(STX_ERR_INVALID, "image %d: feature detection needs u8x3 images", i);
        if (im->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "image lives on another device");
        if (im->w > STX_FEATURES_MAX_SIDE || im->h > STX_FEATURES_MAX_SIDE)
            return stx_fail(STX_ERR_INVALID, "image %d is %dx%d: feature detection takes sides up to %d", i, im->w, im->h, STX_FEATURES_MAX_SIDE);
        const stx_buf* m = masks ? masks[i] : nullptr;
        if (m) {
            if (m->elem != STX_U8 || m->c != 1) return stx_fail(STX_ERR_INVALID, "mask %d: feature detection needs u8x1 masks", i);
            if (m->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "image lives on another device");
            if (m->w != im->w || m->h != im->h)  // the reference's message (stitching/feature_detector.py:35-38), shapes as (rows, cols)
                return stx_fail(STX_ERR_INVALID, "Resolution of mask %d (%d, %d) does not match the resolution of image %d (%d, %d).", i + 1,
                                m->h, m->w, i + 1, im->h, im->w);
        }
        const int L = level_counts[i];
        if (L < 0 || L > nlevels) return stx_fail(STX_ERR_INVALID, "image %d: %d levels of at most %d", i, L, nlevels);
        long long qsum = 0;
        for (int l = 0; l < L; l++) {
            const int w = level_wh[(i * ML + l) * 2], h = level_wh[(i * ML + l) * 2 + 1], q = quotas[i * ML + l];
            if (w < 2 * STX_FEAT_BORDER + 1 || h < 2 * STX_FEAT_BORDER + 1 || w > im->w || h > im->h || (l == 0 && (w != im->w || h != im->h)))
                return stx_fail(STX_ERR_INVALID, "image %d (%dx%d): level %d of %dx%d", i, im->w, im->h, l, w, h);
            if (q < 0) return stx_fail(STX_ERR_INVALID, "image %d: quota %d of level %d", i, q, l);
            qsum += q;
        }
        if (qsum > nfeatures) return stx_fail(STX_ERR_INVALID, "image %d: the quotas add up to %lld of %d features", i, qsum, nfeatures);
    }
    for (int k = 0; k < 36 * 256 * 4; k++)
        if (patterns[k] < -13 || patterns[k] > 13) return stx_fail(STX_ERR_INVALID, "pattern coordinate %d outside +-13", (int)patterns[k]);
    STX_TRY(stx_set_device(ctx));
    std::fill(out_counts, out_counts + n, 0);

    // grey level 0 of the images that have a level at all
    std::vector<std::vector<StxBufRef>> grey((size_t)n);  // [image][level]
    std::vector<StxFeatImage> gi;
    long long tiles = 0;
    double bytes = 0.0;
    int max_levels = 0;
    for (int i = 0; i < n; i++) {
        const int L = level_counts[i];
        max_levels = std::max(max_levels, L);
        if (L == 0) continue;
        const stx_buf* im = images[i];
        grey[i].resize((size_t)L);
        STX_TRY(stx_buf_new(ctx, im->w, im->h, 1, STX_U8, &grey[i][0]));
        StxFeatImage K{};
        K.img = im->ptr; K.istride = (long long)im->stride; K.grey = grey[i][0]->ptr; K.gstride = (long long)grey[i][0]->stride;
        K.w = im->w; K.h = im->h;
        K.tiles_x = (im->w + STX_FEAT_GREY_TW - 1) / STX_FEAT_GREY_TW;
        K.tile0 = (int)tiles;
        tiles += (long long)K.tiles_x * ((im->h + STX_FEAT_GREY_TH - 1) / STX_FEAT_GREY_TH);
        bytes += 4.0 * im->w * im->h;
        gi.push_back(K);
    }
    if (gi.empty()) return STX_OK;  // no image reaches 33 x 33
    {
        StxDevBlock d_gi;
        STX_TRY(upload_small(ctx, gi.data(), gi.size() * sizeof(StxFeatImage), &d_gi));
        STX_TRY(stx_launch_feat_grey(ctx, (const StxFeatImage*)d_gi.get(), (int)gi.size(), (int)tiles, bytes));
    }
    // levels 1 ..: one batched exact resize per level, over the images that still have one
    for (int l = 1; l < max_levels; l++) {
        std::vector<const stx_buf*> srcs;
        std::vector<int> wh, who;
        for (int i = 0; i < n; i++) {
            if (level_counts[i] <= l) continue;
            srcs.push_back(grey[i][l - 1].get());
            wh.push_back(level_wh[(i * ML + l) * 2]);
            wh.push_back(level_wh[(i * ML + l) * 2 + 1]);
            who.push_back(i);
        }
        std::vector<stx_buf*> outs(srcs.size(), nullptr);
        STX_TRY(stx_resize_linear_exact_batch(ctx, (int)srcs.size(), srcs.data(), wh.data(), outs.data()));
        for (size_t k = 0; k < who.size(); k++) grey[who[k]][l].reset(outs[k]);
    }
    // the level table: blur buffers, tile lists, candidate arena
    std::vector<StxFeatLevel> lv;
    std::vector<int> lv_img, lv_level;
    std::vector<StxBufRef> blur;
    long long btiles = 0, stiles = 0, arena = 0;
    double bbytes = 0.0, sbytes = 0.0;
    for (int i = 0; i < n; i++) {
        for (int l = 0; l < level_counts[i]; l++) {
            const stx_buf* g = grey[i][l].get();
            const stx_buf* m = masks ? masks[i] : nullptr;
            blur.emplace_back();
            STX_TRY(stx_buf_new(ctx, g->w, g->h, 1, STX_U8, &blur.back()));
            StxFeatLevel K{};
            K.g = g->ptr; K.gstride = (long long)g->stride; K.blur = blur.back()->ptr; K.bstride = (long long)blur.back()->stride;
            K.mask = m ? m->ptr : nullptr; K.mstride = m ? (long long)m->stride : 0;
            K.w = g->w; K.h = g->h; K.w0 = images[i]->w; K.h0 = images[i]->h;
            K.btiles_x = (g->w + STX_FEAT_BLUR_TW - 1) / STX_FEAT_BLUR_TW;
            K.btile0 = (int)btiles;
            btiles += (long long)K.btiles_x * ((g->h + STX_FEAT_BLUR_TH - 1) / STX_FEAT_BLUR_TH);
            const int iw = g->w - 2 * STX_FEAT_BORDER, ih = g->h - 2 * STX_FEAT_BORDER;  // the interior: >= 1 x 1
            K.stiles_x = (iw + STX_FEAT_SCORE_TW - 1) / STX_FEAT_SCORE_TW;
            K.stile0 = (int)stiles;
            stiles += (long long)K.stiles_x * ((ih + STX_FEAT_SCORE_TH - 1) / STX_FEAT_SCORE_TH);
            K.cand_off = arena;
            K.cand_cap = (long long)((iw + 1) / 2) * ((ih + 1) / 2);
            arena += K.cand_cap;
            bbytes += 2.0 * g->w * g->h;
            sbytes += (double)g->w * g->h;
            lv.push_back(K); lv_img.push_back(i); lv_level.push_back(l);
        }
    }
    if (btiles > 0x7fffffffLL || stiles > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "feature detection over more than 2^31 tiles");
    const int nl = (int)lv.size();
    StxDevBlock d_lv, d_cand, d_counts;
    STX_TRY(upload_small(ctx, lv.data(), lv.size() * sizeof(StxFeatLevel), &d_lv));
    STX_TRY(stx_dev_alloc(ctx, (size_t)arena * sizeof(unsigned long long), &d_cand));
    STX_TRY(stx_dev_alloc(ctx, (size_t)nl * sizeof(int), &d_counts));
    STX_HIP(hipMemsetAsync(d_counts.get(), 0, (size_t)nl * sizeof(int), ctx->stream));
    STX_TRY(stx_launch_feat_blur(ctx, (const StxFeatLevel*)d_lv.get(), nl, (int)btiles, bbytes));
    STX_TRY(stx_launch_feat_score(ctx, (const StxFeatLevel*)d_lv.get(), nl, (int)stiles, fast_threshold, (unsigned long long*)d_cand.get(),
                                  (int*)d_counts.get(), sbytes));
    // the one wait: how many candidates every level has decides where its keypoints go
    std::vector<int> counts((size_t)nl, 0);
    STX_HIP(hipMemcpyAsync(counts.data(), d_counts.get(), (size_t)nl * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<StxFeatSel> sel((size_t)nl);
    int total = 0;
    long long ncand = 0;
    for (int k = 0; k < nl; k++) {
        if (counts[k] < 0 || counts[k] > lv[k].cand_cap)
            return stx_fail(STX_ERR_HIP, "feature detection: %d candidates on a level that can hold %lld", counts[k], lv[k].cand_cap);
        StxFeatSel& S = sel[k];
        S = StxFeatSel{};
        S.cand_off = lv[k].cand_off; S.count = counts[k];
        S.keep = std::min(counts[k], quotas[lv_img[k] * ML + lv_level[k]]);
        S.out_off = total;
        total += S.keep;
        ncand += counts[k];
        out_counts[lv_img[k]] += S.keep;
    }
    if (out_info) { out_info[0] = nl; out_info[1] = (double)ncand; out_info[2] = total; }
    if (total == 0) return STX_OK;
    StxDevBlock d_sel, d_tmp, d_keys, d_item, d_bins, d_desc, d_cxcy, d_pat;
    STX_TRY(upload_small(ctx, sel.data(), sel.size() * sizeof(StxFeatSel), &d_sel));
    STX_TRY(upload_small(ctx, cxcy, 72 * sizeof(int), &d_cxcy));
    STX_TRY(upload_small(ctx, patterns, 36 * 256 * 4, &d_pat));
    STX_TRY(stx_dev_alloc(ctx, (size_t)total * sizeof(unsigned long long), &d_tmp));
    STX_TRY(stx_dev_alloc(ctx, (size_t)total * sizeof(unsigned long long), &d_keys));
    STX_TRY(stx_dev_alloc(ctx, (size_t)total * sizeof(int), &d_item));
    STX_TRY(stx_dev_alloc(ctx, (size_t)total * sizeof(int), &d_bins));
    STX_TRY(stx_dev_alloc(ctx, (size_t)total * 32, &d_desc));
    STX_HIP(hipMemsetAsync(d_item.get(), 0, (size_t)total * sizeof(int), ctx->stream));  // 0: not written (feat_describe checks)
    STX_TRY(stx_launch_feat_select(ctx, (const StxFeatSel*)d_sel.get(), nl, (const unsigned long long*)d_cand.get(),
                                   (unsigned long long*)d_tmp.get(), (unsigned long long*)d_keys.get(), (int*)d_item.get()));
    STX_TRY(stx_launch_feat_describe(ctx, (const StxFeatLevel*)d_lv.get(), nl, (const unsigned long long*)d_keys.get(), (const int*)d_item.get(), total,
                                     (const int*)d_cxcy.get(), (const signed char*)d_pat.get(), (int*)d_bins.get(), (uint8_t*)d_desc.get()));
    std::vector<unsigned long long> keys((size_t)total);
    std::vector<int> bins((size_t)total);
    std::vector<uint8_t> desc((size_t)total * 32);
    STX_HIP(hipMemcpyAsync(keys.data(), d_keys.get(), keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipMemcpyAsync(bins.data(), d_bins.get(), bins.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipMemcpyAsync(desc.data(), d_desc.get(), desc.size(), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));
    for (int b : bins)
        if (b < 0) return stx_fail(STX_ERR_HIP, "feature detection: the selection left a keypoint slot unfilled");
    // levels are listed image by image, so an image's keypoints are one run of the flat output
    std::vector<int> at((size_t)n, 0);
    for (int k = 0; k < nl; k++) {
        const int i = lv_img[k];
        for (int j = 0; j < sel[k].keep; j++) {
            const int s = sel[k].out_off + j;
            const size_t o = (size_t)i * nfeatures + at[i]++;
            const unsigned long long key = keys[s];
            out_lxyb[o * 4] = lv_level[k];
            out_lxyb[o * 4 + 1] = (int)(key & 0x7fffu);
            out_lxyb[o * 4 + 2] = (int)((key >> 15) & 0x7fffu);
            out_lxyb[o * 4 + 3] = bins[s];
            out_R[o] = STX_FEAT_R_BIAS - (long long)(key >> 30);
            memcpy(out_desc + o * 32, desc.data() + (size_t)s * 32, 32);
        }
    }
    return STX_OK;  // the scratch blocks go back here, behind the synchronisation
}
