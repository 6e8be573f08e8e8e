// stx_cameras_host.cpp — host side of CameraSolver's bundle adjustments (the project's own solver, not cv.detail.BundleAdjusterRay):
// a problem handle that keeps the edges and their points on the device, and one evaluation of the normal equations per call
// (stx_cameras.hip): upload of the variants, one launch, one wait.  tests/numpy_cameras.py is the contract; the
// affine and the reprojection adjustment (tests/numpy_affine.py, tests/numpy_reproj.py; sections 18 and 19) evaluate on the same handle.
#include <algorithm>
#include <cmath>

#include "stx_internal.h"

STX_EXPORT int stx_ray_problem_create(stx_ctx* ctx, int n_edges, const int* edge_cams, const long long* offsets, const double* pts,
                                      stx_ray_problem** out)
{
    if (!ctx || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_edges < 0 || n_edges > STX_RAY_MAX_CAMERAS * (STX_RAY_MAX_CAMERAS - 1) / 2)
        return stx_fail(STX_ERR_INVALID, "ray adjustment over %d edges: 0 .. %d", n_edges, STX_RAY_MAX_CAMERAS * (STX_RAY_MAX_CAMERAS - 1) / 2);
    if (n_edges > 0 && (!edge_cams || !offsets)) return stx_fail(STX_ERR_INVALID, "null argument");
    // every check before anything is allocated
    int max_cam = -1;
    for (int e = 0; e < n_edges; e++) {
        const int i = edge_cams[2 * e], j = edge_cams[2 * e + 1];
        if (i < 0 || j >= STX_RAY_MAX_CAMERAS) return stx_fail(STX_ERR_INVALID, "edge %d joins the cameras %d and %d: 0 .. %d", e, i, j, STX_RAY_MAX_CAMERAS - 1);
        if (i >= j) return stx_fail(STX_ERR_INVALID, "edge %d joins the cameras %d and %d: the first must be the smaller", e, i, j);
        const long long m = offsets[e + 1] - offsets[e];
        if (offsets[e] < 0 || m < 0 || (e == 0 && offsets[0] != 0)) return stx_fail(STX_ERR_INVALID, "edge %d: the offsets do not ascend from 0", e);
        if (m > STX_RAY_MAX_MATCHES) return stx_fail(STX_ERR_INVALID, "edge %d has %lld matches: ray adjustment takes up to %d", e, m, STX_RAY_MAX_MATCHES);
        max_cam = j > max_cam ? j : max_cam;
    }
    const long long total = n_edges > 0 ? offsets[n_edges] : 0;
    if (total > 0 && !pts) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    std::unique_ptr<stx_ray_problem> P(new stx_ray_problem);
    P->ctx = ctx; P->n_edges = n_edges; P->min_cams = max_cam + 1; P->total = total;
    if (n_edges > 0) {
        STX_TRY(stx_dev_alloc(ctx, (size_t)n_edges * 2 * sizeof(int), &P->d_edge_cams));
        STX_TRY(stx_dev_alloc(ctx, ((size_t)n_edges + 1) * sizeof(long long), &P->d_offsets));
        STX_TRY(stx_dev_alloc(ctx, std::max<size_t>((size_t)total * 4 * sizeof(double), 8), &P->d_pts));
        // the blocks of an evaluation, sized for the widest of the three adjustments (the reprojection's: 270 doubles a camera, 120 sums an edge)
        STX_TRY(stx_dev_alloc(ctx, (size_t)P->min_cams * STX_RAY_MAX_CAMERA_DOUBLES * sizeof(double), &P->d_variants));
        STX_TRY(stx_dev_alloc(ctx, (size_t)n_edges * STX_RAY_MAX_SUMS * sizeof(double), &P->d_out));
        STX_HIP(hipMemcpyAsync(P->d_edge_cams.get(), edge_cams, (size_t)n_edges * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        STX_HIP(hipMemcpyAsync(P->d_offsets.get(), offsets, ((size_t)n_edges + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        if (total > 0) STX_HIP(hipMemcpyAsync(P->d_pts.get(), pts, (size_t)total * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        STX_TRY(P->timer.arm(4));
        STX_HIP(hipStreamSynchronize(ctx->stream));  // the caller's arrays are free again
    }
    *out = P.release();
    return STX_OK;
}

namespace {
using NormalEquationsLaunch = int (*)(stx_ctx*, int, const int*, const long long*, const double*, const double*, double*, hipEvent_t, hipEvent_t);

// one evaluation of any of the adjustments: a camera's `count` variants are `width` doubles each (at most STX_RAY_MAX_CAMERA_DOUBLES a
// camera), an edge gets `sums` doubles (at most STX_RAY_MAX_SUMS)
int problem_eval(stx_ray_problem* P, const char* what, int count, int width, int sums, NormalEquationsLaunch launch, int n_cams,
                 const double* variants, double* out, double out_info[4])
{
    static_assert(15 * 18 <= STX_RAY_MAX_CAMERA_DOUBLES && 120 <= STX_RAY_MAX_SUMS, "the problem's blocks hold the widest adjustment");
    const size_t per_cam = (size_t)width * count;
    if (!P) return stx_fail(STX_ERR_INVALID, "problem is null");
    if (out_info) std::fill(out_info, out_info + 4, 0.0);
    if (n_cams < P->min_cams || n_cams > STX_RAY_MAX_CAMERAS)
        return stx_fail(STX_ERR_INVALID, "%s adjustment of %d cameras: the edges name %d, the limit is %d", what, n_cams, P->min_cams, STX_RAY_MAX_CAMERAS);
    if (n_cams > 0 && !variants) return stx_fail(STX_ERR_INVALID, "null argument");
    for (size_t k = 0; k < (size_t)n_cams * per_cam; k++)
        if (!std::isfinite(variants[k]))
            return stx_fail(STX_ERR_INVALID, "camera %zu: variant %zu is not finite", k / per_cam, (k % per_cam) / (size_t)width);
    if (out_info) { out_info[0] = P->n_edges; out_info[1] = (double)P->total; }
    if (P->n_edges == 0) return STX_OK;
    if (!out) return stx_fail(STX_ERR_INVALID, "null argument");
    stx_ctx* ctx = P->ctx;
    STX_TRY(stx_set_device(ctx));
    STX_TRY(P->timer.mark(0, ctx->stream));
    STX_HIP(hipMemcpyAsync(P->d_variants.get(), variants, (size_t)P->min_cams * per_cam * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    STX_TRY(launch(ctx, P->n_edges, (const int*)P->d_edge_cams.get(), (const long long*)P->d_offsets.get(), (const double*)P->d_pts.get(),
                   (const double*)P->d_variants.get(), (double*)P->d_out.get(), P->timer.ev[1], P->timer.ev[2]));
    STX_HIP(hipMemcpyAsync(out, P->d_out.get(), (size_t)P->n_edges * sums * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    STX_TRY(P->timer.mark(3, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));  // the one wait
    if (out_info) {
        STX_TRY(P->timer.ms(1, 2, &out_info[2]));
        STX_TRY(P->timer.ms(0, 3, &out_info[3]));
    }
    return STX_OK;
}
}  // namespace

STX_EXPORT int stx_ray_problem_eval(stx_ray_problem* P, int n_cams, const double* variants, double* out, double out_info[4])
{
    return problem_eval(P, "ray", 9, 10, 45, stx_launch_ray_normal_equations, n_cams, variants, out, out_info);
}

STX_EXPORT int stx_affine_problem_eval(stx_ray_problem* P, int n_cams, const double* variants, double* out, double out_info[4])
{
    return problem_eval(P, "affine", 9, 8, 45, stx_launch_affine_normal_equations, n_cams, variants, out, out_info);
}

STX_EXPORT int stx_reproj_problem_eval(stx_ray_problem* P, int n_cams, const double* variants, double* out, double out_info[4])
{
    return problem_eval(P, "reprojection", 15, 18, 120, stx_launch_reproj_normal_equations, n_cams, variants, out, out_info);
}

STX_EXPORT int stx_ray_problem_free(stx_ray_problem* P)
{
    if (!P) return STX_OK;
    if (P->n_edges > 0 && P->ctx) {
        if (stx_set_device(P->ctx) == STX_OK) hipStreamSynchronize(P->ctx->stream);
    }
    delete P;  // the events go; the blocks go back to the context's allocator
    return STX_OK;
}
