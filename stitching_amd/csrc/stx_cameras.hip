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

// the 256 lane sums of a workgroup folded in the contract's order, v[l] += v[l + s] for s = 128 .. 1, and written by lane 0: strides 128
// and 64 through LDS (the upper half of the live lanes writes), 32 .. 1 inside the first wavefront
__device__ inline void fold_lane_sums(double (&acc)[RAY_SUMS], double* fold, int tid, double* __restrict__ out)
{
#pragma unroll
    for (int s = RAY_WG / 2; s >= 64; s >>= 1) {
        if (tid >= s && tid < 2 * s) {
#pragma unroll
            for (int a = 0; a < RAY_SUMS; a++) fold[a * (RAY_WG / 2) + (tid - s)] = acc[a];
        }
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int a = 0; a < RAY_SUMS; a++) acc[a] = __dadd_rn(acc[a], fold[a * (RAY_WG / 2) + tid]);
        }
        __syncthreads();
    }
    if (tid >= 64) return;  // three whole wavefronts
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int a = 0; a < RAY_SUMS; a++) acc[a] = __dadd_rn(acc[a], __shfl_down(acc[a], s, 64));  // lanes >= s: not used below
    }
    if (tid == 0) {
#pragma unroll
        for (int a = 0; a < RAY_SUMS; a++) out[a] = acc[a];
    }
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

}  // namespace

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
