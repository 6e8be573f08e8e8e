// stx_cameras.hip — the ray bundle adjustment of CameraSolver on gfx950: the project's OWN solver (not cv.detail.BundleAdjusterRay).
// tests/numpy_cameras.py is the contract, in the bits of all 45 float64 sums of every edge; DESIGN.md section 17.  One launch per
// Levenberg-Marquardt evaluation:
//   ray_normal_equations  one workgroup of 256 threads per edge (a pair of cameras with its inlier matches).  The 2 x 9 variants of the
//                         two cameras (10 doubles each: f', H') are the same in every lane (scalar loads); a lane strides over the
//                         edge's matches and keeps the 45 sums E, g[8], B[36] in registers.  Per match: the two base rays, then one
//                         Jacobian column at a time from the + and - variant of one parameter, consumed at once (g_k, B_lk for l <= k),
//                         so that only the 8 columns and not 18 rays are live.  The lane sums are folded in the contract's order:
//                         strides 128 and 64 through LDS, 32 .. 1 inside the first wavefront, v[l] += v[l + s] either way.
//   affine_normal_equations  the same launch shape, sums and fold for CameraSolver(model="affine") (tests/numpy_affine.py, DESIGN.md
//                         section 18): a camera is a similarity of the plane, 9 variants of 8 doubles (the map and its inverse); the
//                         residual is (u, v) - T_j^-1 T_i (x, y) in image j's pixels — multiplies, adds and subtractions only.
//   reproj_normal_equations  CameraSolver(model="reproj") (tests/numpy_reproj.py): 7 parameters a camera (focal,
//                         principal point, aspect, Rodrigues vector), 15 variants of 18 doubles (P = R K^-1 and Q = K R^T); the residual
//                         is (u, v) - the projection of Q_j P_i (x, y, 1) in image j's pixels.  120 sums E, g[14], B[105] an edge, too
//                         many for one lane's registers and one workgroup's LDS: the grid is (edges, 3) and a workgroup keeps one part
//                         of the terms — E, g_i, B_ii (36) | g_j, B_jj (35) | B_ij (49) — over all matches of its edge, so every sum
//                         is still one lane sum folded in the contract's order.  Each part forms the base residual and the Jacobian
//                         columns it needs and writes its slice of the edge's 120 outputs.
// The fp64 arithmetic is IEEE multiply, add, subtract, divide and square root in the contract's order: no FMA (the file is compiled with
// -ffp-contract=off and says so itself below), no MFMA.
#include "stx_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int RAY_WG = STX_RAY_LANES;
constexpr int RAY_SUMS = 45;

struct Ray3 { double a, b, c; };

// the unit ray of variant V (f', h0 .. h8) at the point (x, y)
__device__ inline Ray3 ray_of(const double* __restrict__ V, double x, double y)
{
    const double X0 = __dadd_rn(__dadd_rn(__dmul_rn(V[1], x), __dmul_rn(V[2], y)), V[3]);
    const double X1 = __dadd_rn(__dadd_rn(__dmul_rn(V[4], x), __dmul_rn(V[5], y)), V[6]);
    const double X2 = __dadd_rn(__dadd_rn(__dmul_rn(V[7], x), __dmul_rn(V[8], y)), V[9]);
    const double s = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(X0, X0), __dmul_rn(X1, X1)), __dmul_rn(X2, X2)));
    return Ray3{__ddiv_rn(X0, s), __ddiv_rn(X1, s), __ddiv_rn(X2, s)};
}

// sqrt(fi fj) (p - q)
__device__ inline Ray3 residual_of(double fi, double fj, const Ray3& p, const Ray3& q)
{
    const double s = __dsqrt_rn(__dmul_rn(fi, fj));
    return Ray3{__dmul_rn(s, __dsub_rn(p.a, q.a)), __dmul_rn(s, __dsub_rn(p.b, q.b)), __dmul_rn(s, __dsub_rn(p.c, q.c))};
}

__device__ inline double dot3(const Ray3& p, const Ray3& q)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(p.a, q.a), __dmul_rn(p.b, q.b)), __dmul_rn(p.c, q.c));
}

// first index of row k of the upper triangle of an 8 x 8 matrix, row-major
__device__ constexpr int tri_row(int k) { return k * 8 - k * (k - 1) / 2; }

// the 256 lane sums of a workgroup folded in the contract's order, v[l] += v[l + s] for s = 128 .. 1, and written by lane 0 to out[at(a)]:
// strides 128 and 64 through LDS (the upper half of the live lanes writes; fold holds N x 128 doubles), 32 .. 1 inside the first wavefront
template <int N, class At>
__device__ inline void fold_lane_sums(double (&acc)[N], double* fold, int tid, double* __restrict__ out, At at)
{
#pragma unroll
    for (int s = RAY_WG / 2; s >= 64; s >>= 1) {
        if (tid >= s && tid < 2 * s) {
#pragma unroll
            for (int a = 0; a < N; a++) fold[a * (RAY_WG / 2) + (tid - s)] = acc[a];
        }
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int a = 0; a < N; a++) acc[a] = __dadd_rn(acc[a], fold[a * (RAY_WG / 2) + tid]);
        }
        __syncthreads();
    }
    if (tid >= 64) return;  // three whole wavefronts
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int a = 0; a < N; a++) acc[a] = __dadd_rn(acc[a], __shfl_down(acc[a], s, 64));  // lanes >= s: not used below
    }
    if (tid == 0) {
#pragma unroll
        for (int a = 0; a < N; a++) out[at(a)] = acc[a];
    }
}

template <int N>
__device__ inline void fold_lane_sums(double (&acc)[N], double* fold, int tid, double* __restrict__ out)
{
    fold_lane_sums(acc, fold, tid, out, [](int a) { return a; });
}

__global__ __launch_bounds__(RAY_WG) void ray_normal_equations_kernel(const int* __restrict__ edge_cams, const long long* __restrict__ offsets,
                                                                      const double* __restrict__ pts, const double* __restrict__ variants,
                                                                      double* __restrict__ out)
{
    __shared__ double fold[RAY_SUMS * (RAY_WG / 2)];
    const int e = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ Vi = variants + (size_t)edge_cams[2 * e] * 90;
    const double* __restrict__ Vj = variants + (size_t)edge_cams[2 * e + 1] * 90;
    const long long first = offsets[e], last = offsets[e + 1];
    double acc[RAY_SUMS];
#pragma unroll
    for (int a = 0; a < RAY_SUMS; a++) acc[a] = 0.0;
    for (long long m = first + tid; m < last; m += RAY_WG) {
        const double2 xy = *(const double2*)(pts + m * 4), uv = *(const double2*)(pts + m * 4 + 2);
        const Ray3 bi = ray_of(Vi, xy.x, xy.y), bj = ray_of(Vj, uv.x, uv.y);
        const Ray3 r = residual_of(Vi[0], Vj[0], bi, bj);
        acc[0] = __dadd_rn(acc[0], dot3(r, r));
        Ray3 J[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            Ray3 p, q;
            if (k < 4) {
                const double* __restrict__ Vp = Vi + (1 + 2 * k) * 10;
                const double* __restrict__ Vm = Vi + (2 + 2 * k) * 10;
                p = residual_of(Vp[0], Vj[0], ray_of(Vp, xy.x, xy.y), bj);
                q = residual_of(Vm[0], Vj[0], ray_of(Vm, xy.x, xy.y), bj);
            } else {
                const double* __restrict__ Vp = Vj + (1 + 2 * (k - 4)) * 10;
                const double* __restrict__ Vm = Vj + (2 + 2 * (k - 4)) * 10;
                p = residual_of(Vi[0], Vp[0], bi, ray_of(Vp, uv.x, uv.y));
                q = residual_of(Vi[0], Vm[0], bi, ray_of(Vm, uv.x, uv.y));
            }
            J[k] = Ray3{__dmul_rn(__dsub_rn(p.a, q.a), 500.0), __dmul_rn(__dsub_rn(p.b, q.b), 500.0), __dmul_rn(__dsub_rn(p.c, q.c), 500.0)};
            acc[1 + k] = __dadd_rn(acc[1 + k], dot3(J[k], r));
#pragma unroll
            for (int l = 0; l <= k; l++) acc[9 + tri_row(l) + (k - l)] = __dadd_rn(acc[9 + tri_row(l) + (k - l)], dot3(J[l], J[k]));
        }
    }
    fold_lane_sums(acc, fold, tid, out + (size_t)e * RAY_SUMS);
}

// ---- affine partial ----------------------------------------------------------------------------------------------------------------------
struct Vec2 { double a, b; };

// (a x - b y) + tx, (b x + a y) + ty for S = {a, b, tx, ty}
__device__ inline Vec2 similarity_of(const double* __restrict__ S, double x, double y)
{
    return Vec2{__dadd_rn(__dsub_rn(__dmul_rn(S[0], x), __dmul_rn(S[1], y)), S[2]),
                __dadd_rn(__dadd_rn(__dmul_rn(S[1], x), __dmul_rn(S[0], y)), S[3])};
}

// (u, v) - Tj^-1 p: Vj is a variant of camera j, whose inverse map is its second half
__device__ inline Vec2 affine_residual_of(const double* __restrict__ Vj, const Vec2& p, double u, double v)
{
    const Vec2 q = similarity_of(Vj + 4, p.a, p.b);
    return Vec2{__dsub_rn(u, q.a), __dsub_rn(v, q.b)};
}

__device__ inline double dot2(const Vec2& p, const Vec2& q) { return __dadd_rn(__dmul_rn(p.a, q.a), __dmul_rn(p.b, q.b)); }

__global__ __launch_bounds__(RAY_WG) void affine_normal_equations_kernel(const int* __restrict__ edge_cams, const long long* __restrict__ offsets,
                                                                         const double* __restrict__ pts, const double* __restrict__ variants,
                                                                         double* __restrict__ out)
{
    __shared__ double fold[RAY_SUMS * (RAY_WG / 2)];
    const int e = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ Vi = variants + (size_t)edge_cams[2 * e] * 72;
    const double* __restrict__ Vj = variants + (size_t)edge_cams[2 * e + 1] * 72;
    const long long first = offsets[e], last = offsets[e + 1];
    double acc[RAY_SUMS];
#pragma unroll
    for (int a = 0; a < RAY_SUMS; a++) acc[a] = 0.0;
    for (long long m = first + tid; m < last; m += RAY_WG) {
        const double2 xy = *(const double2*)(pts + m * 4), uv = *(const double2*)(pts + m * 4 + 2);
        const Vec2 P = similarity_of(Vi, xy.x, xy.y);
        const Vec2 r = affine_residual_of(Vj, P, uv.x, uv.y);
        acc[0] = __dadd_rn(acc[0], dot2(r, r));
        Vec2 J[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            Vec2 p, q;
            if (k < 4) {
                p = affine_residual_of(Vj, similarity_of(Vi + (1 + 2 * k) * 8, xy.x, xy.y), uv.x, uv.y);
                q = affine_residual_of(Vj, similarity_of(Vi + (2 + 2 * k) * 8, xy.x, xy.y), uv.x, uv.y);
            } else {
                p = affine_residual_of(Vj + (1 + 2 * (k - 4)) * 8, P, uv.x, uv.y);
                q = affine_residual_of(Vj + (2 + 2 * (k - 4)) * 8, P, uv.x, uv.y);
            }
            J[k] = Vec2{__dmul_rn(__dsub_rn(p.a, q.a), 500.0), __dmul_rn(__dsub_rn(p.b, q.b), 500.0)};
            acc[1 + k] = __dadd_rn(acc[1 + k], dot2(J[k], r));
#pragma unroll
            for (int l = 0; l <= k; l++) acc[9 + tri_row(l) + (k - l)] = __dadd_rn(acc[9 + tri_row(l) + (k - l)], dot2(J[l], J[k]));
        }
    }
    fold_lane_sums(acc, fold, tid, out + (size_t)e * RAY_SUMS);
}

// ---- reprojection ----------------------------------------------------------------------------------------------------------------------
constexpr int REPROJ_PARAMS = 7, REPROJ_VARIANT = 18, REPROJ_CAMERA = 15 * REPROJ_VARIANT, REPROJ_SUMS = 120;
constexpr int REPROJ_FOLD = 49;  // sums of the largest part (E, g_i, B_ii: 36 | g_j, B_jj: 35 | B_ij: 49): 49 x 128 doubles of LDS

// first index of row k of the upper triangle of an n x n matrix, row-major
__device__ constexpr int tri_row_of(int n, int k) { return k * n - k * (k - 1) / 2; }

// X = P (x, y, 1) for the variant V = {P, Q}
__device__ inline Ray3 world_of(const double* __restrict__ V, double x, double y)
{
    return Ray3{__dadd_rn(__dadd_rn(__dmul_rn(V[0], x), __dmul_rn(V[1], y)), V[2]),
                __dadd_rn(__dadd_rn(__dmul_rn(V[3], x), __dmul_rn(V[4], y)), V[5]),
                __dadd_rn(__dadd_rn(__dmul_rn(V[6], x), __dmul_rn(V[7], y)), V[8])};
}

// (u, v) - the projection of Q X for the variant V = {P, Q}
__device__ inline Vec2 reproj_residual_of(const double* __restrict__ V, const Ray3& X, double u, double v)
{
    const double Y0 = __dadd_rn(__dadd_rn(__dmul_rn(V[9], X.a), __dmul_rn(V[10], X.b)), __dmul_rn(V[11], X.c));
    const double Y1 = __dadd_rn(__dadd_rn(__dmul_rn(V[12], X.a), __dmul_rn(V[13], X.b)), __dmul_rn(V[14], X.c));
    const double Y2 = __dadd_rn(__dadd_rn(__dmul_rn(V[15], X.a), __dmul_rn(V[16], X.b)), __dmul_rn(V[17], X.c));
    return Vec2{__dsub_rn(u, __ddiv_rn(Y0, Y2)), __dsub_rn(v, __ddiv_rn(Y1, Y2))};
}

// Jacobian column k of camera i (its + and - variant, camera j at its base) / of camera j (the base X)
__device__ inline Vec2 reproj_column_i(const double* __restrict__ Vi, const double* __restrict__ Vj, int k, double x, double y, double u, double v)
{
    const Vec2 p = reproj_residual_of(Vj, world_of(Vi + (1 + 2 * k) * REPROJ_VARIANT, x, y), u, v);
    const Vec2 q = reproj_residual_of(Vj, world_of(Vi + (2 + 2 * k) * REPROJ_VARIANT, x, y), u, v);
    return Vec2{__dmul_rn(__dsub_rn(p.a, q.a), 500.0), __dmul_rn(__dsub_rn(p.b, q.b), 500.0)};
}

__device__ inline Vec2 reproj_column_j(const double* __restrict__ Vj, const Ray3& X, int k, double u, double v)
{
    const Vec2 p = reproj_residual_of(Vj + (1 + 2 * k) * REPROJ_VARIANT, X, u, v);
    const Vec2 q = reproj_residual_of(Vj + (2 + 2 * k) * REPROJ_VARIANT, X, u, v);
    return Vec2{__dmul_rn(__dsub_rn(p.a, q.a), 500.0), __dmul_rn(__dsub_rn(p.b, q.b), 500.0)};
}

// One part of an edge's 120 sums over all its matches.  SECOND = false: E, g and the diagonal block of camera i (acc[0] = E, then g[7],
// then the 28 of the upper triangle); SECOND = true: g and the diagonal block of camera j (no E).
template <bool SECOND>
__device__ inline void reproj_diagonal_part(const double* __restrict__ Vi, const double* __restrict__ Vj, const double* __restrict__ pts,
                                            long long first, long long last, double* fold, int tid, double* __restrict__ out)
{
    constexpr int N = SECOND ? 35 : 36, G = SECOND ? 0 : 1, B = G + REPROJ_PARAMS;
    double acc[N];
#pragma unroll
    for (int a = 0; a < N; a++) acc[a] = 0.0;
    for (long long m = first + tid; m < last; m += RAY_WG) {
        const double2 xy = *(const double2*)(pts + m * 4), uv = *(const double2*)(pts + m * 4 + 2);
        const Ray3 X = world_of(Vi, xy.x, xy.y);
        const Vec2 r = reproj_residual_of(Vj, X, uv.x, uv.y);
        if (!SECOND) acc[0] = __dadd_rn(acc[0], dot2(r, r));
        Vec2 J[REPROJ_PARAMS];
#pragma unroll
        for (int k = 0; k < REPROJ_PARAMS; k++) {
            J[k] = SECOND ? reproj_column_j(Vj, X, k, uv.x, uv.y) : reproj_column_i(Vi, Vj, k, xy.x, xy.y, uv.x, uv.y);
            acc[G + k] = __dadd_rn(acc[G + k], dot2(J[k], r));
#pragma unroll
            for (int l = 0; l <= k; l++) {
                const int at = B + tri_row_of(REPROJ_PARAMS, l) + (k - l);
                acc[at] = __dadd_rn(acc[at], dot2(J[l], J[k]));
            }
        }
    }
    // where a sum lives among the edge's 120: E, g[14], then the upper triangle of 14 x 14
    fold_lane_sums(acc, fold, tid, out, [](int a) {
        constexpr int off = SECOND ? REPROJ_PARAMS : 0;
        if (a < G) return 0;
        if (a < B) return 1 + off + (a - G);
        int t = a - B, l = 0;
        while (t >= REPROJ_PARAMS - l) { t -= REPROJ_PARAMS - l; l++; }
        return 15 + tri_row_of(14, off + l) + t;
    });
}

// the 49 sums of the block between camera i's and camera j's columns: the 7 columns of camera i stay live, a column of camera j is
// consumed as it is formed
__device__ inline void reproj_cross_part(const double* __restrict__ Vi, const double* __restrict__ Vj, const double* __restrict__ pts,
                                         long long first, long long last, double* fold, int tid, double* __restrict__ out)
{
    constexpr int N = REPROJ_PARAMS * REPROJ_PARAMS;
    double acc[N];
#pragma unroll
    for (int a = 0; a < N; a++) acc[a] = 0.0;
    for (long long m = first + tid; m < last; m += RAY_WG) {
        const double2 xy = *(const double2*)(pts + m * 4), uv = *(const double2*)(pts + m * 4 + 2);
        const Ray3 X = world_of(Vi, xy.x, xy.y);
        Vec2 Ji[REPROJ_PARAMS];
#pragma unroll
        for (int l = 0; l < REPROJ_PARAMS; l++) Ji[l] = reproj_column_i(Vi, Vj, l, xy.x, xy.y, uv.x, uv.y);
#pragma unroll
        for (int k = 0; k < REPROJ_PARAMS; k++) {
            const Vec2 Jj = reproj_column_j(Vj, X, k, uv.x, uv.y);
#pragma unroll
            for (int l = 0; l < REPROJ_PARAMS; l++) acc[l * REPROJ_PARAMS + k] = __dadd_rn(acc[l * REPROJ_PARAMS + k], dot2(Ji[l], Jj));
        }
    }
    fold_lane_sums(acc, fold, tid, out, [](int a) { return 15 + tri_row_of(14, a / REPROJ_PARAMS) + (REPROJ_PARAMS - a / REPROJ_PARAMS) + a % REPROJ_PARAMS; });
}

// grid (edges, 3): blockIdx.y is the part of the edge's sums this workgroup keeps
__global__ __launch_bounds__(RAY_WG) void reproj_normal_equations_kernel(const int* __restrict__ edge_cams, const long long* __restrict__ offsets,
                                                                         const double* __restrict__ pts, const double* __restrict__ variants,
                                                                         double* __restrict__ out)
{
    __shared__ double fold[REPROJ_FOLD * (RAY_WG / 2)];
    const int e = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ Vi = variants + (size_t)edge_cams[2 * e] * REPROJ_CAMERA;
    const double* __restrict__ Vj = variants + (size_t)edge_cams[2 * e + 1] * REPROJ_CAMERA;
    const long long first = offsets[e], last = offsets[e + 1];
    double* __restrict__ sums = out + (size_t)e * REPROJ_SUMS;
    if (blockIdx.y == 0) reproj_diagonal_part<false>(Vi, Vj, pts, first, last, fold, tid, sums);
    else if (blockIdx.y == 1) reproj_diagonal_part<true>(Vi, Vj, pts, first, last, fold, tid, sums);
    else reproj_cross_part(Vi, Vj, pts, first, last, fold, tid, sums);
}

}  // namespace

int stx_launch_reproj_normal_equations(stx_ctx* ctx, int n_edges, const int* d_edge_cams, const long long* d_offsets, const double* d_pts,
                                       const double* d_variants, double* d_out, hipEvent_t start, hipEvent_t stop)
{
    StxProfScope prof(ctx, "reproj_normal_equations", 0.0);
    if (start) STX_HIP(hipEventRecord(start, ctx->stream));
    hipLaunchKernelGGL(reproj_normal_equations_kernel, dim3(n_edges, 3), dim3(RAY_WG), 0, ctx->stream, d_edge_cams, d_offsets, d_pts, d_variants,
                       d_out);
    STX_TRY(stx_check_launch("reproj_normal_equations"));
    if (stop) STX_HIP(hipEventRecord(stop, ctx->stream));
    return STX_OK;
}

int stx_launch_affine_normal_equations(stx_ctx* ctx, int n_edges, const int* d_edge_cams, const long long* d_offsets, const double* d_pts,
                                       const double* d_variants, double* d_out, hipEvent_t start, hipEvent_t stop)
{
    StxProfScope prof(ctx, "affine_normal_equations", 0.0);
    if (start) STX_HIP(hipEventRecord(start, ctx->stream));
    hipLaunchKernelGGL(affine_normal_equations_kernel, dim3(n_edges), dim3(RAY_WG), 0, ctx->stream, d_edge_cams, d_offsets, d_pts, d_variants,
                       d_out);
    STX_TRY(stx_check_launch("affine_normal_equations"));
    if (stop) STX_HIP(hipEventRecord(stop, ctx->stream));
    return STX_OK;
}

int stx_launch_ray_normal_equations(stx_ctx* ctx, int n_edges, const int* d_edge_cams, const long long* d_offsets, const double* d_pts,
                                    const double* d_variants, double* d_out, hipEvent_t start, hipEvent_t stop)
{
    StxProfScope prof(ctx, "ray_normal_equations", 0.0);
    if (start) STX_HIP(hipEventRecord(start, ctx->stream));
    hipLaunchKernelGGL(ray_normal_equations_kernel, dim3(n_edges), dim3(RAY_WG), 0, ctx->stream, d_edge_cams, d_offsets, d_pts, d_variants,
                       d_out);
    STX_TRY(stx_check_launch("ray_normal_equations"));
    if (stop) STX_HIP(hipEventRecord(stop, ctx->stream));
    return STX_OK;
}
