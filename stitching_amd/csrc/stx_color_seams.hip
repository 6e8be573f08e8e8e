// stx_color_seams.hip — the project's own colour-aware seam finder for gfx950 (NOT OpenCV's DpSeamFinder; tests/numpy_color_seams.py is the
// contract): the pairs of one dependency level at a time (stx_seams_host.cpp builds the levels, as for "voronoi"), two launches per level.
//
// Of a pair, r runs along the seam axis (0 <= r < L) and t along the cross axis (0 <= t < W); a vertical seam has (r, t) = (y, x) of the
// roi, a horizontal one (x, y).  c(r, t) = sum over the channels of (I_i - I_j)^2 where both masks are set, else 0.
//   dp:    one workgroup of 256 lanes per pair (blockIdx.x = the pair within its level), lanes along t, lane l owning the columns
//          l + 256 k (k < K, K a template parameter chosen from the level's largest W).  The accumulator row A(r - 1, .) sits in LDS,
//          ping-pong, one barrier per r; both ends carry a sentinel of 2^32 - 1 no neighbour comparison can prefer (A < 2^32 - 1 for
//          L <= STX_COLOR_SEAM_MAX_LENGTH).  c does not depend on the dynamic programme: the image and mask loads of the next RB rows leave
//          as one batch while the dependent chain works through the current RB.  The choice (0 straight, 1 t - 1, 2 t + 1) of every (r, t)
//          goes to the level's arena as a byte.  Then wavefront 0 finds the smallest t that minimises A(L - 1, t) and the seam is walked
//          back 64 rows at a time: all lanes fetch the choices the walk can reach (64 rows, 63 columns either side) into LDS, lane 0
//          walks them there and writes s(r) — one trip to memory per 64 rows instead of one per row.
//          A horizontal seam runs through the same kernel with transposed indexing: its lanes lie along y, so its image loads are
//          strided (one cache line per lane and load).  At the ~0.1 Mpx images seams are found on, that is accepted here; no transpose pass.
//   apply: one lane per roi pixel (lanes along x in both orientations: coalesced), pixels held by both masks only: t < s(r) zeroes the
//          second image's mask, t >= s(r) the first's.
// Only the apply kernel writes masks, and only this pair's `both` pixels, which no other pair of the level reads (the schedule's rule):
// both kernels see the masks as they were at the start of the level.  Images are read only.
#include "stx_internal.h"

namespace {

constexpr int CS_WG = 256;
constexpr int CS_BACK = 64;                    // rows per walk-back step
constexpr int CS_BACK_W = 2 * CS_BACK - 1;     // columns the walk can reach in them
constexpr uint32_t CS_SENTINEL = 0xFFFFFFFFu;

__device__ inline uint32_t cs_cost(const StxColorSeamPair& P, int r, int t)
{
    const int x = P.vertical ? t : r, y = P.vertical ? r : t;
    const uint8_t ma = P.m1[y * P.sm1 + x], mb = P.m2[y * P.sm2 + x];
    const uint8_t* a = P.i1 + y * P.si1 + 3 * x;
    const uint8_t* b = P.i2 + y * P.si2 + 3 * x;
    const int d0 = (int)a[0] - (int)b[0], d1 = (int)a[1] - (int)b[1], d2 = (int)a[2] - (int)b[2];
    return (ma != 0 && mb != 0) ? (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2) : 0u;
}

struct ColorSeamK { const StxColorSeamPair* pairs; uint8_t* arena; };

template <int K, int RB>
__global__ __launch_bounds__(CS_WG) void color_seam_dp_kernel(ColorSeamK Q)
{
    __shared__ uint32_t acc[2][STX_COLOR_SEAM_MAX_CROSS + 2];  // acc[b][t + 1] = A(r, t); [0] and [W + 1]: sentinels
    __shared__ uint8_t win[CS_BACK * CS_BACK_W];
    __shared__ int s_cur;
    const StxColorSeamPair P = Q.pairs[blockIdx.x];
    const int L = P.L, W = P.W, tid = threadIdx.x;
    if (W > K * CS_WG) return;  // never: the host picks K from the level's largest W
    uint8_t* choice = Q.arena + P.off_choice;
    int* seam = (int*)(Q.arena + P.off_seam);

    for (int t = tid; t < W; t += CS_WG) acc[1][t + 1] = 0;  // "row -1": A(0, t) = c(0, t) + 0, straight
    if (tid == 0) { acc[0][0] = acc[1][0] = CS_SENTINEL; acc[0][W + 1] = acc[1][W + 1] = CS_SENTINEL; }
    uint32_t cur[RB][K], nxt[RB][K];
    auto fetch = [&](uint32_t (&c)[RB][K], int r0) {
#pragma unroll
        for (int j = 0; j < RB; j++)
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int t = tid + k * CS_WG;
                c[j][k] = (r0 + j < L && t < W) ? cs_cost(P, r0 + j, t) : 0u;
            }
    };
    fetch(cur, 0);
    __syncthreads();
    for (int r0 = 0; r0 < L; r0 += RB) {
        fetch(nxt, r0 + RB);
#pragma unroll
        for (int j = 0; j < RB; j++) {
            const int r = r0 + j;
            if (r < L) {  // uniform over the workgroup
                const uint32_t* prev = acc[(r & 1) ^ 1];
                uint32_t* out = acc[r & 1];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int t = tid + k * CS_WG;
                    if (t < W) {
                        uint32_t best = prev[t + 1];
                        const uint32_t left = prev[t], right = prev[t + 2];
                        uint8_t ch = 0;
                        if (left < best) { best = left; ch = 1; }
                        if (right < best) { best = right; ch = 2; }
                        out[t + 1] = best + cur[j][k];
                        choice[(long long)r * W + t] = ch;
                    }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int j = 0; j < RB; j++)
#pragma unroll
            for (int k = 0; k < K; k++) cur[j][k] = nxt[j][k];
    }
    // the smallest t that minimises A(L - 1, t)
    if (tid < 64) {
        const uint32_t* last = acc[(L - 1) & 1];
        uint32_t bv = CS_SENTINEL;
        int bt = 0x7FFFFFFF;
        for (int t = tid; t < W; t += 64) {
            const uint32_t v = last[t + 1];
            if (v < bv) { bv = v; bt = t; }
        }
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t ov = __shfl_xor(bv, o);
            const int ot = __shfl_xor(bt, o);
            if (ov < bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; }
        }
        if (tid == 0) { s_cur = bt; seam[L - 1] = bt; }
    }
    __syncthreads();
    // walk back: s(r_hi) is known; the next n = min(CS_BACK, r_hi) rows read the choices of the rows r_hi - q (q < n) within q columns of it
    for (int r_hi = L - 1; r_hi > 0;) {
        const int n = min(CS_BACK, r_hi), s_hi = s_cur, base = s_hi - (CS_BACK - 1);
        for (int idx = tid; idx < n * CS_BACK_W; idx += CS_WG) {
            const int q = idx / CS_BACK_W, o = idx % CS_BACK_W, t = base + o;
            if (abs(t - s_hi) <= q && t >= 0 && t < W) win[idx] = choice[(long long)(r_hi - q) * W + t];
        }
        __syncthreads();
        if (tid == 0) {
            int t = s_hi;
            for (int q = 0; q < n; q++) {
                const uint8_t ch = win[q * CS_BACK_W + (t - base)];
                t += ch == 1 ? -1 : (ch == 2 ? 1 : 0);
                seam[r_hi - q - 1] = t;
            }
            s_cur = t;
        }
        __syncthreads();
        r_hi -= n;
    }
}

__global__ __launch_bounds__(CS_WG) void color_seam_apply_kernel(ColorSeamK Q)
{
    const StxColorSeamPair P = Q.pairs[blockIdx.y];
    const int rw = P.vertical ? P.W : P.L, rh = P.vertical ? P.L : P.W;
    const long long idx = (long long)blockIdx.x * CS_WG + threadIdx.x;
    if (idx >= (long long)rw * rh) return;
    const int y = (int)(idx / rw), x = (int)(idx % rw);
    uint8_t* pa = P.m1 + y * P.sm1 + x;
    uint8_t* pb = P.m2 + y * P.sm2 + x;
    if (*pa == 0 || *pb == 0) return;
    const int r = P.vertical ? y : x, t = P.vertical ? x : y;
    const int* seam = (const int*)(Q.arena + P.off_seam);
    const bool second_keeps = t >= seam[r];
    if (second_keeps == (P.first_is_i != 0)) *pa = 0;
    else *pb = 0;
}

template <int K, int RB>
void cs_launch_dp(stx_ctx* ctx, const ColorSeamK& Q, int np)
{
    hipLaunchKernelGGL((color_seam_dp_kernel<K, RB>), dim3(np), dim3(CS_WG), 0, ctx->stream, Q);
}

}  // namespace

int stx_launch_color_seam_level(stx_ctx* ctx, const StxColorSeamPair* d_pairs, int np, int max_cross, long long max_area, uint8_t* d_arena,
                                double algo_bytes)
{
    if (np <= 0) return STX_OK;
    if (max_cross < 1 || max_cross > STX_COLOR_SEAM_MAX_CROSS) return stx_fail(STX_ERR_INVALID, "internal: cross extent %d", max_cross);
    ColorSeamK Q{d_pairs, d_arena};
    {
        StxProfScope prof(ctx, "color_seam_dp", algo_bytes);
        // lanes own K columns each; the rows fetched ahead shrink as K grows (RB * K cost registers, twice)
        if (max_cross <= CS_WG) cs_launch_dp<1, 8>(ctx, Q, np);
        else if (max_cross <= 2 * CS_WG) cs_launch_dp<2, 8>(ctx, Q, np);
        else if (max_cross <= 4 * CS_WG) cs_launch_dp<4, 4>(ctx, Q, np);
        else if (max_cross <= 8 * CS_WG) cs_launch_dp<8, 2>(ctx, Q, np);
        else cs_launch_dp<16, 1>(ctx, Q, np);
        STX_TRY(stx_check_launch("color_seam_dp"));
    }
    StxProfScope prof(ctx, "color_seam_apply", 0.0);
    hipLaunchKernelGGL(color_seam_apply_kernel, dim3((unsigned)((max_area + CS_WG - 1) / CS_WG), np), dim3(CS_WG), 0, ctx->stream, Q);
    return stx_check_launch("color_seam_apply");
}
