// stx_matches_host.cpp — host side of MatchEstimator (the project's own matcher, not cv.detail.BestOf2NearestMatcher): argument checks,
// the job and pair tables of the batched kernels (stx_matches.hip), the uploads, and the one wait at the end.
// tests/numpy_matches.py is the contract; DESIGN.md section 16.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "stx_internal.h"

namespace {
// STX_MATCH_TRAIN=uniform: match_2nn loads the train descriptors wave-uniformly from memory instead of through LDS tiles (the same
// results; read at every call, for the A/B of tools/bench_matches.py)
bool train_through_lds()
{
    const char* v = getenv("STX_MATCH_TRAIN");
    return !(v && !strcmp(v, "uniform"));
}
}  // namespace

STX_EXPORT int stx_match_features(stx_ctx* ctx, int n, const unsigned char* const* desc, const int* desc_shape, const double* const* pts,
                                  const int* pts_rows, int ratio_T, int range_width, int ransac_iters, double threshold_sq, unsigned seed,
                                  int* out_counts, int* out_matches, unsigned char* out_mask, int* out_pick, double* out_H,
                                  double out_info[4])
{
    return stx_match_features_model(ctx, n, desc, desc_shape, pts, pts_rows, ratio_T, range_width, ransac_iters, threshold_sq, seed,
                                    STX_MATCH_MODEL_HOMOGRAPHY, out_counts, out_matches, out_mask, out_pick, out_H, out_info);
}

STX_EXPORT int stx_match_features_model(stx_ctx* ctx, int n, const unsigned char* const* desc, const int* desc_shape,
                                        const double* const* pts, const int* pts_rows, int ratio_T, int range_width, int ransac_iters,
                                        double threshold_sq, unsigned seed, int model, int* out_counts, int* out_matches,
                                        unsigned char* out_mask, int* out_pick, double* out_H, double out_info[4])
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (model != STX_MATCH_MODEL_HOMOGRAPHY && model != STX_MATCH_MODEL_AFFINE_PARTIAL && model != STX_MATCH_MODEL_AFFINE_FULL)
        return stx_fail(STX_ERR_INVALID, "feature matching with the model %d: homography (0), affine partial (1) or affine full (2)", model);
    if (n < 0 || (n > 0 && (!desc || !desc_shape || !pts || !pts_rows))) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (ransac_iters < 1 || ransac_iters > STX_MATCH_MAX_ITERS)
        return stx_fail(STX_ERR_INVALID, "feature matching with %d RANSAC hypotheses: 1 .. %d", ransac_iters, STX_MATCH_MAX_ITERS);
    if (ratio_T < 0 || ratio_T > 1024) return stx_fail(STX_ERR_INVALID, "ratio threshold %d: 0 .. 1024 (match_conf in 0 .. 1)", ratio_T);
    if (!(threshold_sq >= 0.0) || !(threshold_sq <= 1e12)) return stx_fail(STX_ERR_INVALID, "squared RANSAC threshold %g: 0 .. 1e12", threshold_sq);
    if (out_info) std::fill(out_info, out_info + 4, 0.0);
    // every check before anything is allocated or launched
    std::vector<int> off((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
        const int rows = desc_shape[i * 3], cols = desc_shape[i * 3 + 1], bytes = desc_shape[i * 3 + 2];
        if (rows < 0 || (rows > 0 && (cols != 32 || bytes != 1)))
            return stx_fail(STX_ERR_INVALID, "image %d: descriptors of shape (%d, %d) and %d bytes per element: feature matching needs n x 32 u8",
                            i, rows, cols, bytes);
        if (rows > STX_MATCH_MAX_FEATURES)
            return stx_fail(STX_ERR_INVALID, "image %d has %d features: feature matching takes up to %d", i, rows, STX_MATCH_MAX_FEATURES);
        if (pts_rows[i] != rows) return stx_fail(STX_ERR_INVALID, "image %d: %d descriptors and %d keypoints", i, rows, pts_rows[i]);
        if (rows > 0 && (!desc[i] || !pts[i])) return stx_fail(STX_ERR_INVALID, "null argument");
        if ((long long)off[i] + rows > 0x3fffffffLL) return stx_fail(STX_ERR_INVALID, "feature matching over more than 2^30 features");
        off[i + 1] = off[i] + rows;
    }
    // the pairs i < j within range_width, row-major, and the directions of them that can match at all
    std::vector<StxMatchPair> pairs;
    std::vector<StxMatchJob> jobs;
    long long blocks = 0, nn_total = 0, cap = 0;
    double compares = 0.0;
    auto add_job = [&](int a, int b) -> long long {
        const int na = off[a + 1] - off[a], nb = off[b + 1] - off[b];
        if (na == 0 || nb < 2) return -1;
        StxMatchJob J{};
        J.a_off = off[a]; J.b_off = off[b]; J.na = na; J.nb = nb; J.block0 = (int)blocks; J.nn_off = nn_total;
        jobs.push_back(J);
        blocks += (na + STX_MATCH_NN_WG - 1) / STX_MATCH_NN_WG;
        nn_total += na;
        compares += (double)na * nb;
        return J.nn_off;
    };
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) {
            if (range_width >= 0 && j - i > range_width) continue;
            if (blocks > 0x3fffffffLL) return stx_fail(STX_ERR_INVALID, "feature matching over more than 2^30 workgroups");
            StxMatchPair P{};
            P.i_off = off[i]; P.j_off = off[j]; P.ni = off[i + 1] - off[i]; P.nj = off[j + 1] - off[j];
            P.p = (int)((unsigned)i * (unsigned)n + (unsigned)j);
            P.nn_f = add_job(i, j); P.nn_b = add_job(j, i);
            P.out_off = cap;
            cap += P.ni + P.nj;
            pairs.push_back(P);
        }
    const size_t np = pairs.size();
    const int hb = (ransac_iters + STX_MATCH_HYP_PER_WG - 1) / STX_MATCH_HYP_PER_WG;
    if ((long long)np * hb > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "feature matching over %zu pairs x %d hypotheses: more than 2^31 workgroups", np, hb);
    if (np > 0 && (!out_counts || !out_pick || !out_H || (cap > 0 && (!out_matches || !out_mask)))) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (out_info) out_info[0] = (double)np;
    if (np == 0) return STX_OK;
    STX_TRY(stx_set_device(ctx));
    const int total = off[n];
    StxEventTimer timer;  // start, uploads queued, kernels queued, copies back queued
    if (out_info) STX_TRY(timer.arm(4));
    STX_TRY(timer.mark(0, ctx->stream));
    StxDevBlock d_desc, d_pts, d_jobs, d_pairs, d_nn, d_counts, d_matches, d_xyuv, d_hyp, d_pick, d_H, d_mask;
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)total * 32, 32), &d_desc));
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)total * 16, 16), &d_pts));
    for (int i = 0; i < n; i++) {
        const size_t rows = (size_t)(off[i + 1] - off[i]);
        if (rows == 0) continue;
        STX_HIP(hipMemcpyAsync((uint8_t*)d_desc.get() + (size_t)off[i] * 32, desc[i], rows * 32, hipMemcpyHostToDevice, ctx->stream));
        STX_HIP(hipMemcpyAsync((uint8_t*)d_pts.get() + (size_t)off[i] * 16, pts[i], rows * 16, hipMemcpyHostToDevice, ctx->stream));
    }
    STX_TRY(upload_small(ctx, pairs.data(), np * sizeof(StxMatchPair), &d_pairs));
    if (!jobs.empty()) STX_TRY(upload_small(ctx, jobs.data(), jobs.size() * sizeof(StxMatchJob), &d_jobs));
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)nn_total * sizeof(uint2), 8), &d_nn));
    STX_TRY(stx_dev_alloc(ctx, np * sizeof(int), &d_counts));
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)cap * 3 * sizeof(int), 4), &d_matches));
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)cap * 4 * sizeof(double), 8), &d_xyuv));
    STX_TRY(stx_dev_alloc(ctx, np * (size_t)ransac_iters * sizeof(int), &d_hyp));
    STX_TRY(stx_dev_alloc(ctx, np * 2 * sizeof(int), &d_pick));
    STX_TRY(stx_dev_alloc(ctx, np * 9 * sizeof(double), &d_H));
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)cap, 1), &d_mask));
    if (cap > 0) STX_HIP(hipMemsetAsync(d_mask.get(), 0, (size_t)cap, ctx->stream));
    STX_TRY(timer.mark(1, ctx->stream));
    if (!jobs.empty())
        STX_TRY(stx_launch_match_2nn(ctx, (const StxMatchJob*)d_jobs.get(), (int)jobs.size(), (int)blocks, (const uint32_t*)d_desc.get(),
                                     (uint2*)d_nn.get(), compares, train_through_lds()));
    STX_TRY(stx_launch_match_union(ctx, (const StxMatchPair*)d_pairs.get(), (int)np, (const uint2*)d_nn.get(), (const double*)d_pts.get(), ratio_T,
                                   (int*)d_counts.get(), (int*)d_matches.get(), (double*)d_xyuv.get()));
    STX_TRY(stx_launch_match_ransac(ctx, (const StxMatchPair*)d_pairs.get(), (int)np, (const int*)d_counts.get(), (const double*)d_xyuv.get(),
                                    ransac_iters, threshold_sq, seed, model, (int*)d_hyp.get()));
    STX_TRY(stx_launch_match_pick(ctx, (const StxMatchPair*)d_pairs.get(), (int)np, (const int*)d_counts.get(), (const double*)d_xyuv.get(),
                                  ransac_iters, threshold_sq, seed, model, (const int*)d_hyp.get(), (int*)d_pick.get(), (double*)d_H.get(),
                                  (uint8_t*)d_mask.get()));
    STX_TRY(timer.mark(2, ctx->stream));
    STX_HIP(hipMemcpyAsync(out_counts, d_counts.get(), np * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipMemcpyAsync(out_pick, d_pick.get(), np * 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipMemcpyAsync(out_H, d_H.get(), np * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (cap > 0) {
        STX_HIP(hipMemcpyAsync(out_matches, d_matches.get(), (size_t)cap * 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        STX_HIP(hipMemcpyAsync(out_mask, d_mask.get(), (size_t)cap, hipMemcpyDeviceToHost, ctx->stream));
    }
    STX_TRY(timer.mark(3, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));  // the one wait
    long long matches = 0;
    for (size_t k = 0; k < np; k++) {
        if (out_counts[k] < 0 || out_counts[k] > pairs[k].ni + pairs[k].nj)
            return stx_fail(STX_ERR_HIP, "feature matching: %d matches of a pair that can have %d", out_counts[k], pairs[k].ni + pairs[k].nj);
        matches += out_counts[k];
    }
    if (out_info) {
        out_info[1] = (double)matches;
        STX_TRY(timer.ms(1, 2, &out_info[2]));
        STX_TRY(timer.ms(0, 3, &out_info[3]));
    }
    return STX_OK;  // the scratch blocks go back here, behind the synchronisation
}
