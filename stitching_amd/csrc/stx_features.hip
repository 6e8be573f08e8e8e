// stx_features.hip — kernels of FeatureEstimator: the project's own corner detector and binary descriptor (NOT cv.ORB), integer only.
// tests/numpy_features.py states every step exactly and is the contract, byte for byte; DESIGN.md section 15 has the launch shapes.
//   feat_grey      u8x3 -> grey level 0, all images in one launch
//   (levels 1 ..   stx_resize_linear_exact_batch, one launch per level: stx_features_host.cpp)
//   feat_blur      5 x 5 binomial of every level of every image in one launch (halo of 2 in LDS)
//   feat_score     segment-test score, 3 x 3 suppression, mask, response; the survivors' keys are appended to the level's arena
//   feat_select    per level: the `keep` smallest keys, in order (radix select, then ranks by counting): nothing depends on the order
//                  in which the atomics of feat_score filled the arena, because the keys are unique
//   feat_describe  one wavefront per keypoint: moments of the radius-15 disc, the bin, 256 comparisons of the blurred level
#include <climits>

#include "stx_internal.h"

namespace {

// the last item whose first tile is <= tile (uniform over the workgroup: scalar loads)
#define FEAT_FIND(items, n, tile, first, out)                     \
    do {                                                          \
        int lo_ = 0, hi_ = (n) - 1;                               \
        while (lo_ < hi_) {                                       \
            const int mid_ = (lo_ + hi_ + 1) >> 1;                \
            if ((items)[mid_].first <= (tile)) lo_ = mid_;        \
            else hi_ = mid_ - 1;                                  \
        }                                                         \
        (out) = lo_;                                              \
    } while (0)

__global__ __launch_bounds__(256) void feat_grey_kernel(const StxFeatImage* __restrict__ imgs, int n)
{
    const int tile = blockIdx.x;
    int k;
    FEAT_FIND(imgs, n, tile, tile0, k);
    const StxFeatImage& D = imgs[k];
    const int t = tile - D.tile0, tyi = t / D.tiles_x, txi = t - tyi * D.tiles_x;
    const int x = txi * STX_FEAT_GREY_TW + (threadIdx.x & 63);
    const int y = tyi * STX_FEAT_GREY_TH + (threadIdx.x >> 6);
    if (x >= D.w || y >= D.h) return;
    const uint8_t* p = D.img + (long long)y * D.istride + 3 * x;
    D.grey[(long long)y * D.gstride + x] = (uint8_t)((1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14);
}

__device__ __forceinline__ int feat_reflect101(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return min(max(i, 0), n - 1);  // only tile overhang (pixels that are not written) gets here out of range
}

constexpr int BLUR_LW = STX_FEAT_BLUR_TW + 4, BLUR_LH = STX_FEAT_BLUR_TH + 4;

__global__ __launch_bounds__(512) void feat_blur_kernel(const StxFeatLevel* __restrict__ levels, int n)
{
    __shared__ uint8_t T[BLUR_LH][BLUR_LW];
    const int tile = blockIdx.x;
    int k;
    FEAT_FIND(levels, n, tile, btile0, k);
    const StxFeatLevel& D = levels[k];
    const int t = tile - D.btile0, tyi = t / D.btiles_x, txi = t - tyi * D.btiles_x;
    const int x0 = txi * STX_FEAT_BLUR_TW, y0 = tyi * STX_FEAT_BLUR_TH;
    for (int i = threadIdx.x; i < BLUR_LW * BLUR_LH; i += 512) {
        const int ly = i / BLUR_LW, lx = i - ly * BLUR_LW;
        const int sx = feat_reflect101(x0 + lx - 2, D.w), sy = feat_reflect101(y0 + ly - 2, D.h);
        T[ly][lx] = D.g[(long long)sy * D.gstride + sx];
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= D.w || y >= D.h) return;
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint8_t* r = &T[ly + j][lx];
        const int row = r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4];
        acc += (j == 0 || j == 4 ? 1 : (j == 2 ? 6 : 4)) * row;
    }
    D.blur[(long long)y * D.bstride + x] = (uint8_t)((acc + 128) >> 8);
}

constexpr int SC_GW = STX_FEAT_SCORE_TW + 8, SC_GH = STX_FEAT_SCORE_TH + 8;  // grey tile: halo of 4
constexpr int SC_SW = STX_FEAT_SCORE_TW + 2, SC_SH = STX_FEAT_SCORE_TH + 2;  // score tile: halo of 1

// the segment-test score of the pixel at c (a grey tile of pitch SC_GW): the largest t for which 9 contiguous ring pixels are all
// brighter than c + t or all darker than c - t, as a signed value; `thr` stands for every score that is <= thr (the suppression only
// ever compares such a score with one above thr).  Any 9 of the 16 contiguous ring pixels hold two of the four compass points.
__device__ __forceinline__ int feat_score_at(const uint8_t* c, int thr)
{
    const int v = c[0];
    const int n0 = c[-3 * SC_GW] - v, n4 = c[3] - v, n8 = c[3 * SC_GW] - v, n12 = c[-3] - v;
    const int bright = (n0 > thr) + (n4 > thr) + (n8 > thr) + (n12 > thr);
    const int dark = (n0 < -thr) + (n4 < -thr) + (n8 < -thr) + (n12 < -thr);
    if (bright < 2 && dark < 2) return thr;
    int d[16];
    d[0] = n0; d[4] = n4; d[8] = n8; d[12] = n12;
    d[1] = c[-3 * SC_GW + 1] - v; d[2] = c[-2 * SC_GW + 2] - v; d[3] = c[-SC_GW + 3] - v;
    d[5] = c[SC_GW + 3] - v; d[6] = c[2 * SC_GW + 2] - v; d[7] = c[3 * SC_GW + 1] - v;
    d[9] = c[3 * SC_GW - 1] - v; d[10] = c[2 * SC_GW - 2] - v; d[11] = c[SC_GW - 3] - v;
    d[13] = c[-SC_GW - 3] - v; d[14] = c[-2 * SC_GW - 2] - v; d[15] = c[-3 * SC_GW - 1] - v;
    // minima and maxima of all 16 windows of 9 by doubling: 2, 4, 8, then the ninth
    int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { lo2[i] = min(d[i], d[(i + 1) & 15]); hi2[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; i++) { lo4[i] = min(lo2[i], lo2[(i + 2) & 15]); hi4[i] = max(hi2[i], hi2[(i + 2) & 15]); }
    int s = -256;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int lo9 = min(min(lo4[i], lo4[(i + 4) & 15]), d[(i + 8) & 15]);
        const int hi9 = max(max(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
        s = max(s, max(lo9, -hi9));
    }
    return max(s, thr);
}

__global__ __launch_bounds__(256) void feat_score_kernel(const StxFeatLevel* __restrict__ levels, int n, int thr,
                                                         unsigned long long* __restrict__ cand, int* __restrict__ counts)
{
    __shared__ uint8_t G[SC_GH][SC_GW];
    __shared__ short S[SC_SH][SC_SW];
    const int tile = blockIdx.x;
    int k;
    FEAT_FIND(levels, n, tile, stile0, k);
    const StxFeatLevel& D = levels[k];
    const int t = tile - D.stile0, tyi = t / D.stiles_x, txi = t - tyi * D.stiles_x;
    const int x0 = STX_FEAT_BORDER + txi * STX_FEAT_SCORE_TW, y0 = STX_FEAT_BORDER + tyi * STX_FEAT_SCORE_TH;
    // grey tile at (x0 - 4, y0 - 4): never left of or above the level (x0, y0 >= 16); clamped where the tile hangs over its far edges
    for (int i = threadIdx.x; i < SC_GW * SC_GH; i += 256) {
        const int ly = i / SC_GW, lx = i - ly * SC_GW;
        const int sx = min(x0 - 4 + lx, D.w - 1), sy = min(y0 - 4 + ly, D.h - 1);
        G[ly][lx] = D.g[(long long)sy * D.gstride + sx];
    }
    __syncthreads();
    // scores at (x0 - 1, y0 - 1) ..: the tile and its ring of neighbours
    for (int i = threadIdx.x; i < SC_SW * SC_SH; i += 256) {
        const int ly = i / SC_SW, lx = i - ly * SC_SW;
        S[ly][lx] = (short)feat_score_at(&G[ly + 3][lx + 3], thr);
    }
    __syncthreads();
    const int lx = threadIdx.x & (STX_FEAT_SCORE_TW - 1), ly = threadIdx.x / STX_FEAT_SCORE_TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x > D.w - 1 - STX_FEAT_BORDER || y > D.h - 1 - STX_FEAT_BORDER) return;
    const int s = S[ly + 1][lx + 1];
    if (s <= thr) return;
    if (s <= S[ly][lx] || s <= S[ly][lx + 1] || s <= S[ly][lx + 2] || s <= S[ly + 1][lx] || s <= S[ly + 1][lx + 2] ||
        s <= S[ly + 2][lx] || s <= S[ly + 2][lx + 1] || s <= S[ly + 2][lx + 2])
        return;
    if (D.mask) {
        const long long my = ((long long)(2 * y + 1) * D.h0) / (2ll * D.h), mx = ((long long)(2 * x + 1) * D.w0) / (2ll * D.w);
        if (D.mask[my * D.mstride + mx] == 0) return;
    }
    int a = 0, b = 0, c = 0;
    for (int dy = 0; dy < 7; dy++) {
        const uint8_t* r = &G[ly + 1 + dy][lx + 1];  // the window's row dy, column 0 is r[0]: pixel (x - 3, y - 3 + dy)
#pragma unroll
        for (int dx = 0; dx < 7; dx++) {
            const int ix = r[dx + 1] - r[dx - 1], iy = r[dx + SC_GW] - r[dx - SC_GW];
            a += ix * ix; b += ix * iy; c += iy * iy;
        }
    }
    const long long la = a, lb = b, lc = c;
    const long long R = (25 * (la * lc - lb * lb) - (la + lc) * (la + lc)) >> 16;
    const unsigned long long key = ((unsigned long long)(STX_FEAT_R_BIAS - R) << 30) | ((unsigned long long)y << 15) | (unsigned long long)x;
    const int slot = atomicAdd(&counts[k], 1);
    if (slot < D.cand_cap) cand[D.cand_off + slot] = key;  // cap is the most strict 3 x 3 maxima a level can hold: never exceeded
}

__global__ __launch_bounds__(256) void feat_select_kernel(const StxFeatSel* __restrict__ sel, const unsigned long long* __restrict__ cand,
                                                          unsigned long long* __restrict__ tmp, unsigned long long* __restrict__ keys,
                                                          int* __restrict__ item)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned long long stage[256];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_remaining, s_n;
    const StxFeatSel D = sel[blockIdx.x];
    if (D.keep <= 0) return;
    const unsigned long long* in = cand + D.cand_off;
    const int tid = threadIdx.x;
    // the keep-th smallest key, a byte at a time from the top (keys are unique: exactly `keep` keys are <= it)
    unsigned long long cut = ~0ull;
    if (D.count > D.keep) {
        unsigned long long prefix = 0;
        unsigned remaining = (unsigned)D.keep;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const unsigned long long high = shift == 56 ? 0ull : (~0ull << (shift + 8));
            for (int i = tid; i < D.count; i += 256) {
                const unsigned long long v = in[i];
                if ((v & high) == prefix) atomicAdd(&hist[(unsigned)(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0;
                int d = 0;
                for (; d < 255; d++) {
                    if (cum + hist[d] >= remaining) break;
                    cum += hist[d];
                }
                s_prefix = prefix | ((unsigned long long)d << shift);
                s_remaining = remaining - cum;
            }
            __syncthreads();
            prefix = s_prefix;
            remaining = s_remaining;
        }
        cut = prefix;
    }
    // the survivors in any order ...
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long* mine = tmp + D.out_off;
    for (int i = tid; i < D.count; i += 256) {
        const unsigned long long v = in[i];
        if (v <= cut) {
            const unsigned slot = atomicAdd(&s_n, 1u);
            if (slot < (unsigned)D.keep) mine[slot] = v;
        }
    }
    __syncthreads();
    // ... and each to the place its rank gives it
    for (int i0 = 0; i0 < D.keep; i0 += 256) {
        const bool have = i0 + tid < D.keep;
        const unsigned long long v = have ? mine[i0 + tid] : 0ull;
        int rank = 0;
        for (int j0 = 0; j0 < D.keep; j0 += 256) {
            __syncthreads();
            stage[tid] = j0 + tid < D.keep ? mine[j0 + tid] : ~0ull;
            __syncthreads();
            const int m = min(256, D.keep - j0);
            for (int j = 0; j < m; j++) rank += stage[j] < v ? 1 : 0;
        }
        if (have) {
            keys[D.out_off + rank] = v;
            item[D.out_off + rank] = blockIdx.x + 1;  // 1-based: 0 is a slot that was never written
        }
    }
}

__global__ __launch_bounds__(256) void feat_describe_kernel(const StxFeatLevel* __restrict__ levels, int nl,
                                                            const unsigned long long* __restrict__ keys,
                                                            const int* __restrict__ item, int total, const int* __restrict__ cxcy,
                                                            const signed char* __restrict__ patterns, int* __restrict__ bins,
                                                            uint8_t* __restrict__ desc)
{
    const int lane = threadIdx.x & 63;
    const int kp = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (kp >= total) return;  // a whole wavefront; nothing below synchronises the workgroup
    const unsigned long long key = keys[kp];
    const int it = item[kp];
    const int x = (int)(key & 0x7fffu), y = (int)((key >> 15) & 0x7fffu);
    // a slot the selection did not fill (it fills every one: keys are unique) must not become an address: bin -1 fails the call
    if (it <= 0 || it > nl || x < STX_FEAT_BORDER || y < STX_FEAT_BORDER || x > levels[it - 1].w - 1 - STX_FEAT_BORDER ||
        y > levels[it - 1].h - 1 - STX_FEAT_BORDER) {
        if (lane == 0) bins[kp] = -1;
        return;
    }
    const StxFeatLevel& D = levels[it - 1];
    // moments of the disc u^2 + v^2 <= 225 (inside the level: x, y >= 16)
    const uint8_t* g = D.g + (long long)y * D.gstride + x;
    int m10 = 0, m01 = 0;
    for (int i = lane; i < 31 * 31; i += 64) {
        const int v = i / 31 - 15, u = i - (v + 15) * 31 - 15;
        if (u * u + v * v <= 225) {
            const int p = g[(long long)v * D.gstride + u];
            m10 += u * p; m01 += v * p;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m10 += __shfl_xor(m10, o); m01 += __shfl_xor(m01, o); }
    long long best = lane < 36 ? (long long)m10 * cxcy[lane] + (long long)m01 * cxcy[36 + lane] : LLONG_MIN;
    int bin = lane < 36 ? lane : 64;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bin, o);
        if (ob > best || (ob == best && oi < bin)) { best = ob; bin = oi; }
    }
    // 4 comparisons per lane: bits 4 lane .. 4 lane + 3, two lanes to a byte
    const uint8_t* B = D.blur + (long long)y * D.bstride + x;
    const signed char* P = patterns + ((long long)bin * 256 + 4 * lane) * 4;
    unsigned nib = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int p = B[(long long)P[4 * q + 1] * D.bstride + P[4 * q]], r = B[(long long)P[4 * q + 3] * D.bstride + P[4 * q + 2]];
        nib |= (p < r ? 1u : 0u) << q;
    }
    const unsigned mine = nib << (4 * (lane & 1));
    const unsigned other = __shfl_xor(mine, 1);
    if ((lane & 1) == 0) desc[(long long)kp * 32 + (lane >> 1)] = (uint8_t)(mine | other);
    if (lane == 0) bins[kp] = bin;
}

}  // namespace

int stx_launch_feat_grey(stx_ctx* ctx, const StxFeatImage* d_imgs, int n, int tiles, double algo_bytes)
{
    StxProfScope prof(ctx, "feat_grey", algo_bytes);
    hipLaunchKernelGGL(feat_grey_kernel, dim3(tiles), dim3(256), 0, ctx->stream, d_imgs, n);
    return stx_check_launch("feat_grey");
}

int stx_launch_feat_blur(stx_ctx* ctx, const StxFeatLevel* d_levels, int n, int tiles, double algo_bytes)
{
    StxProfScope prof(ctx, "feat_blur", algo_bytes);
    hipLaunchKernelGGL(feat_blur_kernel, dim3(tiles), dim3(512), 0, ctx->stream, d_levels, n);
    return stx_check_launch("feat_blur");
}

int stx_launch_feat_score(stx_ctx* ctx, const StxFeatLevel* d_levels, int n, int tiles, int threshold, unsigned long long* d_cand,
                          int* d_counts, double algo_bytes)
{
    StxProfScope prof(ctx, "feat_score", algo_bytes);
    hipLaunchKernelGGL(feat_score_kernel, dim3(tiles), dim3(256), 0, ctx->stream, d_levels, n, threshold, d_cand, d_counts);
    return stx_check_launch("feat_score");
}

int stx_launch_feat_select(stx_ctx* ctx, const StxFeatSel* d_sel, int n, const unsigned long long* d_cand, unsigned long long* d_tmp,
                           unsigned long long* d_keys, int* d_item)
{
    StxProfScope prof(ctx, "feat_select", 0.0);
    hipLaunchKernelGGL(feat_select_kernel, dim3(n), dim3(256), 0, ctx->stream, d_sel, d_cand, d_tmp, d_keys, d_item);
    return stx_check_launch("feat_select");
}

int stx_launch_feat_describe(stx_ctx* ctx, const StxFeatLevel* d_levels, int nl, const unsigned long long* d_keys, const int* d_item, int total,
                             const int* d_cxcy, const signed char* d_patterns, int* d_bins, uint8_t* d_desc)
{
    StxProfScope prof(ctx, "feat_describe", (double)total * (709 + 512 + 36));
    hipLaunchKernelGGL(feat_describe_kernel, dim3((total + 3) / 4), dim3(256), 0, ctx->stream, d_levels, nl, d_keys, d_item, total, d_cxcy,
                       d_patterns, d_bins, d_desc);
    return stx_check_launch("feat_describe");
}
