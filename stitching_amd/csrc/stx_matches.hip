// stx_matches.hip — MatchEstimator on gfx950: the project's OWN descriptor matcher and homography RANSAC (not
// cv.detail.BestOf2NearestMatcher).  tests/numpy_matches.py is the contract, byte for byte in every integer array and in the float64
// bits of the winning sample homography; DESIGN.md section 16.  Four launches, no host wait between them:
//   match_2nn     one workgroup per 256 queries of one direction of a pair (flat grid over all ordered pairs).  A lane keeps its query
//                 descriptor in 8 registers; the other image's descriptors pass through an 8 KiB LDS tile, every lane of a wavefront
//                 reading the same address (a broadcast); 8 xor + 8 popcount per compare, ascending scan with strict <.
//   match_union   one workgroup per pair i < j: ratio test, duplicate test, a block prefix sum that places the forward matches and then
//                 the backward extras; writes the matches, their coordinates (x, y, u, v) and the count.
//   match_ransac  one wavefront per hypothesis: the 4 indices and H are the same in every lane, the lanes stride over the pair's
//                 matches, the count is ballot + popcount.  The geometric model (STX_MATCH_MODEL_*) is a template parameter of this
//                 kernel and the next: only the hypothesis differs — the homography of 4 matches, or for scans and flat tiles the
//                 similarity of 2 or the affine map of 3 (tests/numpy_affine.py), homogeneous 3 x 3 all of them.
//   match_pick    one workgroup per pair: arg-max of the counts (the smallest k among equals), H of that k once more, the inlier mask.
// The fp64 arithmetic is IEEE multiplies, adds and subtractions in the contract's order: no FMA (the file is compiled with
// -ffp-contract=off and says so itself below), no division, no libm, no MFMA.
#include <climits>

#include "stx_internal.h"

#pragma clang fp contract(off)

namespace {

// ---- two nearest neighbours ----------------------------------------------------------------------------------------------------------
// LDS: the train descriptors pass through an LDS tile; else every lane loads them from memory at the same address (wave-uniform loads,
// which the compiler turns into scalar loads): STX_MATCH_TRAIN=uniform, kept for the measurement in profiles/matches.json
template <bool LDS>
__global__ __launch_bounds__(STX_MATCH_NN_WG) void match_2nn_kernel(const StxMatchJob* __restrict__ jobs, int njobs,
                                                                    const uint32_t* __restrict__ desc, uint2* __restrict__ nn)
{
    __shared__ uint4 T[LDS ? STX_MATCH_NN_WG * 2 : 1];
    int lo = 0, hi = njobs - 1;  // the last job that starts at or before this workgroup
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const StxMatchJob J = jobs[lo];
    const int tid = threadIdx.x;
    const int q = ((int)blockIdx.x - J.block0) * STX_MATCH_NN_WG + tid;
    const bool live = q < J.na;
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (live) {
        const uint4* s = (const uint4*)(desc + (size_t)(J.a_off + q) * 8);
        qa = s[0]; qb = s[1];
    }
    unsigned d1 = STX_MATCH_NO_D, d2 = STX_MATCH_NO_D, i1 = 0;
    for (int t0 = 0; t0 < J.nb; t0 += STX_MATCH_NN_WG) {
        const int cnt = min(STX_MATCH_NN_WG, J.nb - t0);
        const uint4* train = (const uint4*)(desc + (size_t)(J.b_off + t0) * 8);
        if (LDS) {
            __syncthreads();  // the tile before has been read
            if (tid < cnt) { T[2 * tid] = train[2 * tid]; T[2 * tid + 1] = train[2 * tid + 1]; }
            __syncthreads();
        }
        for (int t = 0; t < cnt; t++) {
            const uint4 a = LDS ? T[2 * t] : train[2 * t], b = LDS ? T[2 * t + 1] : train[2 * t + 1];
            const unsigned d = __popc(a.x ^ qa.x) + __popc(a.y ^ qa.y) + __popc(a.z ^ qa.z) + __popc(a.w ^ qa.w) + __popc(b.x ^ qb.x) +
                               __popc(b.y ^ qb.y) + __popc(b.z ^ qb.z) + __popc(b.w ^ qb.w);
            if (d < d1) { d2 = d1; d1 = d; i1 = (unsigned)(t0 + t); }
            else if (d < d2) d2 = d;
        }
    }
    if (live) nn[J.nn_off + q] = make_uint2(i1, d1 | (d2 << 16));
}

// ---- union -----------------------------------------------------------------------------------------------------------------------------
__device__ inline bool nn_matched(uint2 e, unsigned T) { return 1024u * (e.y & 0xffffu) < T * (e.y >> 16); }  // T <= 1024, d <= 0xffff

// the slot of this thread's flagged element among the workgroup's (256 threads), and how many there are
__device__ inline int block_place(bool flag, int* s_w, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    __syncthreads();  // the round before has read s_w
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < 4; w++) {
        const int c = s_w[w];
        if (w < wave) before += c;
        total += c;
    }
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void match_union_kernel(const StxMatchPair* __restrict__ pairs, const uint2* __restrict__ nn,
                                                          const double* __restrict__ pts, unsigned T, int* __restrict__ counts,
                                                          int* __restrict__ matches, double* __restrict__ xyuv)
{
    __shared__ int s_w[4];
    const StxMatchPair P = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    int* mo = matches + P.out_off * 3;
    double* co = xyuv + P.out_off * 4;
    int base = 0, total;
    if (P.nn_f >= 0) {  // forward: (q, i1, d1) by ascending q
        for (int q0 = 0; q0 < P.ni; q0 += 256) {
            const int q = q0 + tid;
            uint2 e = make_uint2(0, 0);
            bool flag = false;
            if (q < P.ni) { e = nn[P.nn_f + q]; flag = nn_matched(e, T); }
            const int at = base + block_place(flag, s_w, total);
            if (flag) {  // at < ni
                mo[at * 3] = q; mo[at * 3 + 1] = (int)e.x; mo[at * 3 + 2] = (int)(e.y & 0xffffu);
                const double* a = pts + (size_t)(P.i_off + q) * 2;
                const double* b = pts + (size_t)(P.j_off + (int)e.x) * 2;
                co[at * 4] = a[0]; co[at * 4 + 1] = a[1]; co[at * 4 + 2] = b[0]; co[at * 4 + 3] = b[1];
            }
            base += total;
        }
    }
    if (P.nn_b >= 0) {  // backward: (i1(t), t, d1) by ascending t unless the forward pass has that very pair
        for (int t0 = 0; t0 < P.nj; t0 += 256) {
            const int t = t0 + tid;
            uint2 e = make_uint2(0, 0);
            bool flag = false;
            if (t < P.nj) {
                e = nn[P.nn_b + t];
                flag = nn_matched(e, T);
                if (flag && P.nn_f >= 0) {
                    const uint2 f = nn[P.nn_f + (int)e.x];  // e.x < ni
                    if (nn_matched(f, T) && (int)f.x == t) flag = false;
                }
            }
            const int at = base + block_place(flag, s_w, total);
            if (flag) {  // at < ni + nj
                mo[at * 3] = (int)e.x; mo[at * 3 + 1] = t; mo[at * 3 + 2] = (int)(e.y & 0xffffu);
                const double* a = pts + (size_t)(P.i_off + (int)e.x) * 2;
                const double* b = pts + (size_t)(P.j_off + t) * 2;
                co[at * 4] = a[0]; co[at * 4 + 1] = a[1]; co[at * 4 + 2] = b[0]; co[at * 4 + 3] = b[1];
            }
            base += total;
        }
    }
    if (tid == 0) counts[blockIdx.x] = base;
}

// ---- RANSAC ----------------------------------------------------------------------------------------------------------------------------
__device__ inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// the first S <= 4 distinct match indices of hypothesis k of pair p with m >= 4 matches, in the order drawn: no rejection loop
template <int S>
__device__ inline void match_sample(uint32_t seed, uint32_t p, uint32_t k, int m, int out[S])
{
    int s[S];  // the choices so far, ascending
    for (int t = 0; t < S; t++) {
        int r = (int)(mix32(seed ^ mix32(p * 0x9E3779B9u + mix32(4u * k + (uint32_t)t + 1u))) % (uint32_t)(m - t));
        for (int c = 0; c < t; c++)
            if (r >= s[c]) r++;
        out[t] = r;
        int at = t;
        while (at > 0 && s[at - 1] > r) { s[at] = s[at - 1]; at--; }
        s[at] = r;
    }
}

__device__ inline double minor2(double a, double b, double c, double d) { return __dsub_rn(__dmul_rn(a, b), __dmul_rn(c, d)); }
__device__ inline double sum3(double a, double b, double c) { return __dadd_rn(__dadd_rn(a, b), c); }

// adjugate of a row-major 3 x 3: every entry one a*b - c*d
__device__ inline void adj3(const double* m, double* a)
{
    a[0] = minor2(m[4], m[8], m[5], m[7]); a[1] = minor2(m[2], m[7], m[1], m[8]); a[2] = minor2(m[1], m[5], m[2], m[4]);
    a[3] = minor2(m[5], m[6], m[3], m[8]); a[4] = minor2(m[0], m[8], m[2], m[6]); a[5] = minor2(m[2], m[3], m[0], m[5]);
    a[6] = minor2(m[3], m[7], m[4], m[6]); a[7] = minor2(m[1], m[6], m[0], m[7]); a[8] = minor2(m[0], m[4], m[1], m[3]);
}

// M diag(adj(M) p3) of 4 points: the matrix that takes the projective basis to them
__device__ inline void basis3(const double* x, const double* y, double* A)
{
    const double m[9] = {x[0], x[1], x[2], y[0], y[1], y[2], 1.0, 1.0, 1.0};
    double a[9];
    adj3(m, a);
    for (int c = 0; c < 3; c++) {
        const double lam = sum3(__dmul_rn(a[3 * c], x[3]), __dmul_rn(a[3 * c + 1], y[3]), __dmul_rn(a[3 * c + 2], 1.0));
        for (int r = 0; r < 3; r++) A[3 * r + c] = __dmul_rn(m[3 * r + c], lam);
    }
}

// the similarity (x, y) -> (u, v) of 2 sampled matches, times W = |p1 - p0|^2: H = [A, -B, C, B, A, D, 0, 0, W]
__device__ inline void affine_partial_form(const double* x, const double* y, const double* u, const double* v, double* H)
{
    const double dx = __dsub_rn(x[1], x[0]), dy = __dsub_rn(y[1], y[0]), du = __dsub_rn(u[1], u[0]), dv = __dsub_rn(v[1], v[0]);
    const double W = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    const double A = __dadd_rn(__dmul_rn(du, dx), __dmul_rn(dv, dy));
    const double B = __dsub_rn(__dmul_rn(dv, dx), __dmul_rn(du, dy));
    H[0] = A; H[1] = -B; H[2] = __dsub_rn(__dmul_rn(u[0], W), __dsub_rn(__dmul_rn(A, x[0]), __dmul_rn(B, y[0])));
    H[3] = B; H[4] = A; H[5] = __dsub_rn(__dmul_rn(v[0], W), __dadd_rn(__dmul_rn(B, x[0]), __dmul_rn(A, y[0])));
    H[6] = 0.0; H[7] = 0.0; H[8] = W;
}

// the affine map of 3 sampled matches, times det M: rows 0 and 1 of N adj(M), M the source points as homogeneous columns
__device__ inline void affine_full_form(const double* x, const double* y, const double* u, const double* v, double* H)
{
    const double m[9] = {x[0], x[1], x[2], y[0], y[1], y[2], 1.0, 1.0, 1.0};
    double a[9];
    adj3(m, a);
    for (int cc = 0; cc < 3; cc++) {
        H[cc] = sum3(__dmul_rn(u[0], a[cc]), __dmul_rn(u[1], a[3 + cc]), __dmul_rn(u[2], a[6 + cc]));
        H[3 + cc] = sum3(__dmul_rn(v[0], a[cc]), __dmul_rn(v[1], a[3 + cc]), __dmul_rn(v[2], a[6 + cc]));
    }
    H[6] = 0.0; H[7] = 0.0; H[8] = sum3(__dmul_rn(x[0], a[0]), __dmul_rn(x[1], a[3]), __dmul_rn(x[2], a[6]));
}

// H of hypothesis k of an affine model with the sign rule applied (h6 = h7 = +0.0 stay); false: h8 == 0 (coincident or collinear
// sample points), the hypothesis has no inliers
template <int MODEL>
__device__ inline bool affine_hypothesis(const double* __restrict__ c, int m, uint32_t seed, uint32_t p, uint32_t k, double* H)
{
    constexpr int S = MODEL == STX_MATCH_MODEL_AFFINE_PARTIAL ? 2 : 3;
    int idx[S];
    match_sample<S>(seed, p, k, m, idx);
    double x[S], y[S], u[S], v[S];
    for (int t = 0; t < S; t++) {
        const double2 a = *(const double2*)(c + (size_t)idx[t] * 4), b = *(const double2*)(c + (size_t)idx[t] * 4 + 2);
        x[t] = a.x; y[t] = a.y; u[t] = b.x; v[t] = b.y;
    }
    if (MODEL == STX_MATCH_MODEL_AFFINE_PARTIAL) affine_partial_form(x, y, u, v, H);
    else affine_full_form(x, y, u, v, H);
    const double w = H[8];
    if (w < 0.0) {
        for (int i = 0; i < 6; i++) H[i] = -H[i];
        H[8] = -w;
    }
    return w != 0.0;
}

// H of hypothesis k with the sign rule applied; false: W at sample point 0 is 0, the hypothesis has no inliers
template <int MODEL>
__device__ inline bool match_hypothesis(const double* __restrict__ c, int m, uint32_t seed, uint32_t p, uint32_t k, double* H)
{
    if (MODEL != STX_MATCH_MODEL_HOMOGRAPHY) return affine_hypothesis<MODEL>(c, m, seed, p, k, H);
    int idx[4];
    match_sample<4>(seed, p, k, m, idx);
    double x[4], y[4], u[4], v[4];
    for (int t = 0; t < 4; t++) {
        const double2 a = *(const double2*)(c + (size_t)idx[t] * 4), b = *(const double2*)(c + (size_t)idx[t] * 4 + 2);
        x[t] = a.x; y[t] = a.y; u[t] = b.x; v[t] = b.y;
    }
    double A[9], B[9], a[9];
    basis3(x, y, A);
    adj3(A, a);
    basis3(u, v, B);
    for (int r = 0; r < 3; r++)
        for (int cc = 0; cc < 3; cc++)
            H[3 * r + cc] = sum3(__dmul_rn(B[3 * r], a[cc]), __dmul_rn(B[3 * r + 1], a[3 + cc]), __dmul_rn(B[3 * r + 2], a[6 + cc]));
    const double w0 = sum3(__dmul_rn(H[6], x[0]), __dmul_rn(H[7], y[0]), H[8]);
    if (w0 < 0.0)
        for (int i = 0; i < 9; i++) H[i] = -H[i];
    return w0 != 0.0;
}

__device__ inline bool match_inlier(const double* H, const double* __restrict__ c, int e, double t2)
{
    const double2 a = *(const double2*)(c + (size_t)e * 4), b = *(const double2*)(c + (size_t)e * 4 + 2);
    const double X = sum3(__dmul_rn(H[0], a.x), __dmul_rn(H[1], a.y), H[2]);
    const double Y = sum3(__dmul_rn(H[3], a.x), __dmul_rn(H[4], a.y), H[5]);
    const double W = sum3(__dmul_rn(H[6], a.x), __dmul_rn(H[7], a.y), H[8]);
    const double ex = __dsub_rn(X, __dmul_rn(b.x, W)), ey = __dsub_rn(Y, __dmul_rn(b.y, W));
    return W > 0.0 && __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)) <= __dmul_rn(t2, __dmul_rn(W, W));
}

// grid: pair * hb + block of STX_MATCH_HYP_PER_WG hypotheses, hb = ceil(iters / STX_MATCH_HYP_PER_WG)
template <int MODEL>
__global__ __launch_bounds__(64 * STX_MATCH_HYP_PER_WG) void match_ransac_kernel(const StxMatchPair* __restrict__ pairs,
                                                                                 const int* __restrict__ counts,
                                                                                 const double* __restrict__ xyuv, int iters, int hb,
                                                                                 double t2, uint32_t seed, int* __restrict__ hyp)
{
    const int pi = (int)(blockIdx.x / (unsigned)hb);
    const int m = counts[pi];
    if (m < 6) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)(blockIdx.x % (unsigned)hb) * STX_MATCH_HYP_PER_WG + (threadIdx.x >> 6);
    if (k >= iters) return;  // a whole wavefront
    const StxMatchPair P = pairs[pi];
    const double* c = xyuv + P.out_off * 4;
    double H[9];
    int n = 0;
    if (match_hypothesis<MODEL>(c, m, seed, (uint32_t)P.p, (uint32_t)k, H)) {
        for (int e0 = 0; e0 < m; e0 += 64) {
            const int e = e0 + lane;
            n += __popcll(__ballot(e < m && match_inlier(H, c, e, t2)));
        }
    }
    if (lane == 0) hyp[(size_t)pi * iters + k] = n;
}

template <int MODEL>
__global__ __launch_bounds__(256) void match_pick_kernel(const StxMatchPair* __restrict__ pairs, const int* __restrict__ counts,
                                                         const double* __restrict__ xyuv, int iters, double t2, uint32_t seed,
                                                         const int* __restrict__ hyp, int* __restrict__ pick, double* __restrict__ Hs,
                                                         uint8_t* __restrict__ mask)
{
    __shared__ int s_n[256], s_k[256];
    const int pi = blockIdx.x, tid = threadIdx.x;
    const int m = counts[pi];
    if (m < 6) {  // no RANSAC ran (the mask arena was cleared before)
        if (tid == 0) { pick[2 * pi] = 0; pick[2 * pi + 1] = -1; }
        if (tid < 9) Hs[(size_t)pi * 9 + tid] = 0.0;
        return;
    }
    const StxMatchPair P = pairs[pi];
    int best = -1, bk = INT_MAX;
    for (int k = tid; k < iters; k += 256) {  // ascending: strict > keeps the smallest k
        const int n = hyp[(size_t)pi * iters + k];
        if (n > best) { best = n; bk = k; }
    }
    s_n[tid] = best; s_k[tid] = bk;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) {
            const int n = s_n[tid + o], k = s_k[tid + o];
            if (n > s_n[tid] || (n == s_n[tid] && k < s_k[tid])) { s_n[tid] = n; s_k[tid] = k; }
        }
        __syncthreads();
    }
    const int k = s_k[0];
    const double* c = xyuv + P.out_off * 4;
    double H[9];
    const bool ok = match_hypothesis<MODEL>(c, m, seed, (uint32_t)P.p, (uint32_t)k, H);
    for (int e = tid; e < m; e += 256) mask[P.out_off + e] = ok && match_inlier(H, c, e, t2) ? 1 : 0;
    if (tid == 0) {
        pick[2 * pi] = s_n[0]; pick[2 * pi + 1] = k;
        for (int i = 0; i < 9; i++) Hs[(size_t)pi * 9 + i] = H[i];
    }
}

}  // namespace

int stx_launch_match_2nn(stx_ctx* ctx, const StxMatchJob* d_jobs, int njobs, int blocks, const uint32_t* d_desc, uint2* d_nn, double compares,
                         bool lds)
{
    StxProfScope prof(ctx, "match_2nn", compares * 32.0);
    if (lds) hipLaunchKernelGGL(match_2nn_kernel<true>, dim3(blocks), dim3(STX_MATCH_NN_WG), 0, ctx->stream, d_jobs, njobs, d_desc, d_nn);
    else hipLaunchKernelGGL(match_2nn_kernel<false>, dim3(blocks), dim3(STX_MATCH_NN_WG), 0, ctx->stream, d_jobs, njobs, d_desc, d_nn);
    return stx_check_launch("match_2nn");
}

int stx_launch_match_union(stx_ctx* ctx, const StxMatchPair* d_pairs, int np, const uint2* d_nn, const double* d_pts, int ratio_T,
                           int* d_counts, int* d_matches, double* d_xyuv)
{
    StxProfScope prof(ctx, "match_union", 0.0);
    hipLaunchKernelGGL(match_union_kernel, dim3(np), dim3(256), 0, ctx->stream, d_pairs, d_nn, d_pts, (unsigned)ratio_T, d_counts, d_matches,
                       d_xyuv);
    return stx_check_launch("match_union");
}

int stx_launch_match_ransac(stx_ctx* ctx, const StxMatchPair* d_pairs, int np, const int* d_counts, const double* d_xyuv, int iters,
                            double threshold_sq, uint32_t seed, int model, int* d_hyp)
{
    const int hb = (iters + STX_MATCH_HYP_PER_WG - 1) / STX_MATCH_HYP_PER_WG;
    StxProfScope prof(ctx, "match_ransac", 0.0);
    const dim3 grid((unsigned)np * (unsigned)hb), wg(64 * STX_MATCH_HYP_PER_WG);
    switch (model) {
    case STX_MATCH_MODEL_HOMOGRAPHY:
        hipLaunchKernelGGL(match_ransac_kernel<STX_MATCH_MODEL_HOMOGRAPHY>, grid, wg, 0, ctx->stream, d_pairs, d_counts, d_xyuv, iters, hb,
                           threshold_sq, seed, d_hyp);
        break;
    case STX_MATCH_MODEL_AFFINE_PARTIAL:
        hipLaunchKernelGGL(match_ransac_kernel<STX_MATCH_MODEL_AFFINE_PARTIAL>, grid, wg, 0, ctx->stream, d_pairs, d_counts, d_xyuv, iters, hb,
                           threshold_sq, seed, d_hyp);
        break;
    case STX_MATCH_MODEL_AFFINE_FULL:
        hipLaunchKernelGGL(match_ransac_kernel<STX_MATCH_MODEL_AFFINE_FULL>, grid, wg, 0, ctx->stream, d_pairs, d_counts, d_xyuv, iters, hb,
                           threshold_sq, seed, d_hyp);
        break;
    default:
        return stx_fail(STX_ERR_INVALID, "unknown match model %d", model);
    }
    return stx_check_launch("match_ransac");
}

int stx_launch_match_pick(stx_ctx* ctx, const StxMatchPair* d_pairs, int np, const int* d_counts, const double* d_xyuv, int iters,
                          double threshold_sq, uint32_t seed, int model, const int* d_hyp, int* d_pick, double* d_H, uint8_t* d_mask)
{
    StxProfScope prof(ctx, "match_pick", 0.0);
    switch (model) {
    case STX_MATCH_MODEL_HOMOGRAPHY:
        hipLaunchKernelGGL(match_pick_kernel<STX_MATCH_MODEL_HOMOGRAPHY>, dim3(np), dim3(256), 0, ctx->stream, d_pairs, d_counts, d_xyuv, iters,
                           threshold_sq, seed, d_hyp, d_pick, d_H, d_mask);
        break;
    case STX_MATCH_MODEL_AFFINE_PARTIAL:
        hipLaunchKernelGGL(match_pick_kernel<STX_MATCH_MODEL_AFFINE_PARTIAL>, dim3(np), dim3(256), 0, ctx->stream, d_pairs, d_counts, d_xyuv,
                           iters, threshold_sq, seed, d_hyp, d_pick, d_H, d_mask);
        break;
    case STX_MATCH_MODEL_AFFINE_FULL:
        hipLaunchKernelGGL(match_pick_kernel<STX_MATCH_MODEL_AFFINE_FULL>, dim3(np), dim3(256), 0, ctx->stream, d_pairs, d_counts, d_xyuv, iters,
                           threshold_sq, seed, d_hyp, d_pick, d_H, d_mask);
        break;
    default:
        return stx_fail(STX_ERR_INVALID, "unknown match model %d", model);
    }
    return stx_check_launch("match_pick");
}
