// stx_resize.hip — cv::resize(INTER_LINEAR_EXACT) of 8-bit images and seam masks for gfx950.
//
// Replaces, for stitching/images.py's resize and stitching/seam_finder.py:37-43 (SeamFinder.resize), OpenCV's
// cv::resize(INTER_LINEAR_EXACT) for CV_8U and cv::dilate(3x3) followed by the AND with the final mask.  These are "next" rows of the
// scope table: consumers / producers either side of the warp -> blend path.  Host side: stx_resize_host.cpp.
#include <algorithm>

#include "stx_device_math.h"
#include "stx_internal.h"

using namespace stxd;

// ---------------------------------------------------------------------------------------------
// cv::resize(INTER_LINEAR_EXACT) for 8-bit images (next rows N2 / N3): 8.8 fixed-point coefficients made on the host in
// double precision exactly as interpolationLinear<ufixedpoint16>::getCoeffs does (tables: x = offset, y = coeff1 |
// interior << 16), horizontal sums p0 * c0 + p1 * c1 in 8.8, vertical (h0 * d0 + h1 * d1 + 2^15) >> 16, rows
// outside the source (h + 128) >> 8.  DILATE: the source is read through cv::dilate(3x3) on the fly and the result is
// ANDed with a mask of the destination size (SeamFinder.resize, stitching/seam_finder.py:37-43).
// ---------------------------------------------------------------------------------------------
namespace {
struct ResizeK {
    const uint8_t* src; long long sstride; int sw, sh;
    uint8_t* dst; long long dstride; int dw, dh;
    const int2* xt; const int2* yt;
    const uint8_t* andmask; long long amstride;
};
template <int C, bool DILATE>
STX_DEV uint32_t resize_src(const ResizeK& P, int x, int y, int ch)
{
    if (!DILATE) return P.src[(long long)y * P.sstride + x * C + ch];
    uint32_t m = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int xx = x + dx, yy = y + dy;
            if ((unsigned)xx < (unsigned)P.sw && (unsigned)yy < (unsigned)P.sh) m = max(m, (uint32_t)P.src[(long long)yy * P.sstride + xx]);
        }
    return m;
}
// one destination pixel (x, y) from its table entries tx / ty = (offset, coeff1 | interior << 16): the body of the single-image and of
// the batched kernel
template <int C, bool DILATE>
STX_DEV void resize_exact_pixel(const ResizeK& P, int x, int y, int2 tx, int2 ty)
{
    const int ox = tx.x, oy = ty.x;
    const uint32_t cx1 = (uint32_t)tx.y & 0xffffu, cx0 = 256u - cx1, cy1 = (uint32_t)ty.y & 0xffffu, cy0 = 256u - cy1;
    const bool iy = (ty.y >> 16) != 0;
    const int ox1 = min(ox + 1, P.sw - 1), oy1 = min(oy + 1, P.sh - 1);
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
        const uint32_t h0 = resize_src<C, DILATE>(P, ox, oy, ch) * cx0 + resize_src<C, DILATE>(P, ox1, oy, ch) * cx1;
        uint32_t v;
        if (iy) {
            const uint32_t h1 = resize_src<C, DILATE>(P, ox, oy1, ch) * cx0 + resize_src<C, DILATE>(P, ox1, oy1, ch) * cx1;
            v = (h0 * cy0 + h1 * cy1 + 32768u) >> 16;
        } else {
            v = (h0 + 128u) >> 8;
        }
        v = min(v, 255u);
        if (P.andmask) v &= P.andmask[(long long)y * P.amstride + x];
        P.dst[(long long)y * P.dstride + x * C + ch] = (uint8_t)v;
    }
}
template <int C, bool DILATE>
__global__ __launch_bounds__(256) void resize_exact_kernel(ResizeK P)
{
    const int x = blockIdx.x * STX_RESIZE_TW + (threadIdx.x & 63);
    const int y = blockIdx.y * STX_RESIZE_TH + (threadIdx.x >> 6);
    if (x >= P.dw || y >= P.dh) return;
    resize_exact_pixel<C, DILATE>(P, x, y, P.xt[x], P.yt[y]);
}
}  // namespace

namespace {
// SeamFinder.resize, fast form (the reference's default pipeline runs it once per image and panorama): the 3x3 dilation of
// the small low-resolution mask is done once into a scratch image (a few tens of KB, L2 resident) instead of nine
// bounds-checked byte loads per tap; a lane then produces 4 adjacent destination pixels (taps from the scratch, one
// dword of the final warped mask, one dword store).  Same integer arithmetic as resize_exact_kernel<1, true>.
__global__ __launch_bounds__(256) void dilate3x3_kernel(const uint8_t* __restrict__ src, long long sstride, int w, int h,
                                                        uint8_t* __restrict__ dst, long long dstride)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    uint32_t m = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int xx = x + dx, yy = y + dy;
            if ((unsigned)xx < (unsigned)w && (unsigned)yy < (unsigned)h) m = max(m, (uint32_t)src[(long long)yy * sstride + xx]);
        }
    dst[(long long)y * dstride + x] = (uint8_t)m;
}

constexpr int SEAM_ROWS = 16;  // destination rows per lane (seam_resize4_body)
STX_DEV void seam_resize4_body(const ResizeK& P);
__global__ __launch_bounds__(256) void seam_resize4_kernel(ResizeK P) { seam_resize4_body(P); }  // P.src: the dilated low-resolution mask
// all seam masks of a panorama in one launch each (blockIdx.z = image); the argument blocks travel as kernel arguments
constexpr int SEAM_BATCH = 16;
struct SeamBatchK { ResizeK k[SEAM_BATCH]; const uint8_t* raw[SEAM_BATCH]; long long raw_stride[SEAM_BATCH]; };
__global__ __launch_bounds__(256) void seam_resize4_batch_kernel(SeamBatchK B) { seam_resize4_body(B.k[blockIdx.z]); }
__global__ __launch_bounds__(256) void dilate3x3_batch_kernel(SeamBatchK B)
{
    const ResizeK& P = B.k[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= P.sw || y >= P.sh) return;
    const uint8_t* src = B.raw[blockIdx.z];
    const long long ss = B.raw_stride[blockIdx.z];
    uint32_t m = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int xx = x + dx, yy = y + dy;
            if ((unsigned)xx < (unsigned)P.sw && (unsigned)yy < (unsigned)P.sh) m = max(m, (uint32_t)src[(long long)yy * ss + xx]);
        }
    const_cast<uint8_t*>(P.src)[(long long)y * P.sstride + x] = (uint8_t)m;
}
// One lane = 4 adjacent columns of SEAM_ROWS consecutive destination rows.  The seam masks are enlarged (0.1 Mpix -> final
// size, about 11 x): consecutive destination rows interpolate between the same two source rows, so the horizontal sums
// (8.8 fixed point) are kept in registers and recomputed only when the source row changes (a wave-uniform test: the row is);
// a destination pixel then costs the vertical blend, the AND and a quarter of a dword store.
STX_DEV void seam_resize4_body(const ResizeK& P)
{
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int yb = (blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * SEAM_ROWS;
    if (x4 >= P.dw || yb >= P.dh) return;
    // the table holds dw entries rounded up to 4 (host), so the four reads are always inside it
    const int4 ta = *reinterpret_cast<const int4*>(P.xt + x4), tb = *reinterpret_cast<const int4*>(P.xt + x4 + 2);
    const int ox[4] = {ta.x, ta.z, tb.x, tb.z}, cf[4] = {ta.y, ta.w, tb.y, tb.w};
    uint32_t h0[4] = {0, 0, 0, 0}, h1[4] = {0, 0, 0, 0};
    int cur = -1;
    uint32_t am[SEAM_ROWS];  // the final-size masks of all rows first: SEAM_ROWS loads in flight instead of one per iteration
#pragma unroll
    for (int r = 0; r < SEAM_ROWS; r++)
        am[r] = yb + r < P.dh ? *reinterpret_cast<const uint32_t*>(P.andmask + (long long)(yb + r) * P.amstride + x4) : 0u;
#pragma unroll
    for (int r = 0; r < SEAM_ROWS; r++) {
        const int y = yb + r;
        if (y >= P.dh) break;
        const int2 ty = P.yt[y];
        if (ty.x != cur) {
            cur = ty.x;
            const uint8_t* r0 = P.src + (long long)cur * P.sstride;
            const uint8_t* r1 = P.src + (long long)min(cur + 1, P.sh - 1) * P.sstride;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int o0 = ox[j], o1 = min(o0 + 1, P.sw - 1);
                const uint32_t cx1 = (uint32_t)cf[j] & 0xffffu, cx0 = 256u - cx1;
                h0[j] = (uint32_t)r0[o0] * cx0 + (uint32_t)r0[o1] * cx1;
                h1[j] = (uint32_t)r1[o0] * cx0 + (uint32_t)r1[o1] * cx1;
            }
        }
        const uint32_t cy1 = (uint32_t)ty.y & 0xffffu, cy0 = 256u - cy1;
        const bool iy = (ty.y >> 16) != 0;
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = iy ? (h0[j] * cy0 + h1[j] * cy1 + 32768u) >> 16 : (h0[j] + 128u) >> 8;
            out |= min(v, 255u) << (8 * j);
        }
        out &= am[r];
        uint8_t* d = P.dst + (long long)y * P.dstride + x4;
        if (x4 + 4 <= P.dw) *reinterpret_cast<uint32_t*>(d) = out;
        else for (int j = 0; x4 + j < P.dw; j++) d[j] = (uint8_t)(out >> (8 * j));
    }
}
}  // namespace

// SeamFinder.resize for n images: tmp[i] = scratch of the dilated low-resolution mask (pitch tstride[i]), d_xt / d_yt per image
int stx_launch_seam_resize_batch(stx_ctx* ctx, int n, const stx_buf* const* seams, const stx_buf* const* masks, stx_buf* const* dsts,
                                 const int* const* d_xt, const int* const* d_yt, uint8_t* const* tmp, const size_t* tstride)
{
    for (int base = 0; base < n; base += SEAM_BATCH) {
        const int m = std::min(SEAM_BATCH, n - base);
        SeamBatchK B = {};
        int msw = 0, msh = 0, mdw = 0, mdh = 0;
        double bytes = 0.0;
        for (int i = 0; i < m; i++) {
            const int g = base + i;
            ResizeK& K = B.k[i];
            K.src = tmp[g]; K.sstride = (long long)tstride[g]; K.sw = seams[g]->w; K.sh = seams[g]->h;
            K.dst = dsts[g]->ptr; K.dstride = (long long)dsts[g]->stride; K.dw = dsts[g]->w; K.dh = dsts[g]->h;
            K.xt = (const int2*)d_xt[g]; K.yt = (const int2*)d_yt[g];
            K.andmask = masks[g]->ptr; K.amstride = (long long)masks[g]->stride;
            B.raw[i] = seams[g]->ptr; B.raw_stride[i] = (long long)seams[g]->stride;
            msw = std::max(msw, K.sw); msh = std::max(msh, K.sh); mdw = std::max(mdw, K.dw); mdh = std::max(mdh, K.dh);
            bytes += (double)K.sw * K.sh + 2.0 * K.dw * K.dh;
        }
        StxProfScope prof(ctx, "seam_mask_resize", bytes);
        hipLaunchKernelGGL(dilate3x3_batch_kernel, dim3((msw + 63) / 64, (msh + 3) / 4, m), dim3(256), 0, ctx->stream, B);
        hipLaunchKernelGGL(seam_resize4_batch_kernel, dim3((mdw + 255) / 256, (mdh + 4 * SEAM_ROWS - 1) / (4 * SEAM_ROWS), m), dim3(256), 0, ctx->stream, B);
        ctx->seam_resize_paths[1] += m;
    }
    return stx_check_launch("seam_mask_resize");
}

// ---------------------------------------------------------------------------------------------
// SeamFinder.resize as ONE launch (round 6; stitching/seam_finder.py:37-43, stitching/stitcher.py:124,223-225).
// Until round 5 a panorama's seam masks took a table upload (448 KB of coefficients made by the host in double precision), a dilate
// launch into a global scratch and the resize launch with byte gathers from that scratch (81.6 us for config 2's eight masks, 0.24 of
// the HBM peak).  Here a workgroup owns a 512 x 32 tile of the destination:
//   * the coefficients of its 512 columns and 32 rows are made IN the kernel with the same IEEE double operations the host table used
//     (scale * (v + 0.5) - 0.5, floor, rint of the fraction * 256 — interpolationLinear<ufixedpoint16>::getCoeffs; this file is built
//     with -ffp-contract=off) and kept in LDS: nothing is uploaded;
//   * the low-resolution source window under the tile (+ 1 px) goes to LDS, is dilated 3 x 3 there, and every tap is an LDS byte;
//   * a lane makes 8 adjacent pixels of 8 rows (rows per lane, one box, interleaved: 4: 48.4-50.0 us, 6: 48.6-49.4, 8: 47.7-49.1,
//     16: 52.2-55.4, 32: 69.7-73.3 for config 2's eight masks): the final-mask dwords of all its rows are requested before the window is prepared,
//     the horizontal 8.8 sums live in registers and are redone only when the source row changes, a pixel costs two 24-bit
//     multiply-adds and 3/4 of a byte permute, a row leaves as one 8-byte store.
// Same integers as resize_exact_kernel<1, true> (the tests compare both with the CPU checker).
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int SEAM1_COLS = 8, SEAM1_ROWS = 8;  // pixels and rows per lane (the A/B of 4 / 6 / 8 / 16 / 32 rows is quoted above)
constexpr int SEAM1_TW = 64 * SEAM1_COLS, SEAM1_TH = 4 * SEAM1_ROWS;
struct Seam1K {
    const uint8_t* src; long long sstride; int sw, sh;  // the low-resolution seam mask as the seam finder made it
    uint8_t* dst; long long dstride; int dw, dh;         // the destination rectangle ...
    const uint8_t* am; long long amstride;               // ... and the same rectangle of the final warped mask
    int x0, y0;                                          // where the rectangle lies in the full final mask
    double xscale, yscale;                               // 1 / (full width / sw), 1 / (full height / sh): the host's doubles
};
struct Seam1BatchK { Seam1K k[SEAM_BATCH]; int pitch, raw_bytes; };

// interpolationLinear<ufixedpoint16>::getCoeffs for destination index v: (offset, coeff1 | interior << 16) — stx_resize_host.cpp linear_exact_table
STX_DEV int2 seam1_coeff(int v, double scale, int src_n)
{
    const double fval = scale * ((double)v + 0.5) - 0.5;
    const int ival = (int)floor(fval);
    int ofs = 0, c1 = 0, interior = 0;
    if (ival >= 0 && src_n > 1) {
        if (ival < src_n - 1) { ofs = ival; c1 = (int)rint((fval - (double)ival) * 256.0); interior = 1; }
        else ofs = src_n - 1;
    }
    return make_int2(ofs, c1 | (interior << 16));
}

__global__ __launch_bounds__(256) void seam_resize_lds_kernel(Seam1BatchK B)
{
    extern __shared__ uint8_t s_win[];
    __shared__ int2 s_xt[SEAM1_TW];
    __shared__ int2 s_yt[SEAM1_TH];
    const Seam1K& P = B.k[blockIdx.z];
    const int X0 = blockIdx.x * SEAM1_TW, Y0 = blockIdx.y * SEAM1_TH;
    if (X0 >= P.dw || Y0 >= P.dh) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x8 = X0 + lane * SEAM1_COLS, yb = Y0 + wv * SEAM1_ROWS;
    const bool mine = x8 < P.dw && yb < P.dh;  // (the row pitch holds whole 8-pixel groups: host-checked)
    // the final-mask bytes of this lane's rows: in flight while the window is prepared
    uint2 am[SEAM1_ROWS];
#pragma unroll
    for (int r = 0; r < SEAM1_ROWS; r++)
        am[r] = mine && yb + r < P.dh ? *reinterpret_cast<const uint2*>(P.am + (long long)(yb + r) * P.amstride + x8) : make_uint2(0u, 0u);
    for (int i = tid; i < SEAM1_TW; i += 256) s_xt[i] = seam1_coeff(P.x0 + min(X0 + i, P.dw - 1), P.xscale, P.sw);
    if (tid < SEAM1_TH) s_yt[tid] = seam1_coeff(P.y0 + min(Y0 + tid, P.dh - 1), P.yscale, P.sh);
    __syncthreads();
    // the source window under this tile
    const int nx = min(SEAM1_TW, P.dw - X0), ny = min(SEAM1_TH, P.dh - Y0);
    const int wx0 = s_xt[0].x, wx1 = min(s_xt[nx - 1].x + 1, P.sw - 1);
    const int wy0 = s_yt[0].x, wy1 = min(s_yt[ny - 1].x + 1, P.sh - 1);
    const int cw = wx1 - wx0 + 1, rh = wy1 - wy0 + 1, cw2 = cw + 2, pitch = B.pitch;
    uint8_t* const s_raw = s_win;                 // (rh + 2) x (cw + 2): the window and one pixel around it, 0 outside the image
    uint8_t* const s_dil = s_win + B.raw_bytes;   // rh x cw: cv::dilate(3 x 3) of it (pixels outside the image do not take part: 0 = no-op for max)
    const float inv2 = 1.0f / (float)cw2, inv1 = 1.0f / (float)cw;
    for (int i = tid; i < (rh + 2) * cw2; i += 256) {
        int r = (int)((float)i * inv2);  // i / cw2: the estimate is one off at most (i < 2^24)
        int c = i - r * cw2;
        if (c < 0) { r--; c += cw2; } else if (c >= cw2) { r++; c -= cw2; }
        const int sy = wy0 - 1 + r, sx = wx0 - 1 + c;
        s_raw[r * pitch + c] = ((unsigned)sx < (unsigned)P.sw && (unsigned)sy < (unsigned)P.sh) ? P.src[(long long)sy * P.sstride + sx] : (uint8_t)0;
    }
    __syncthreads();
    for (int i = tid; i < rh * cw; i += 256) {
        int r = (int)((float)i * inv1);
        int c = i - r * cw;
        if (c < 0) { r--; c += cw; } else if (c >= cw) { r++; c -= cw; }
        uint32_t m = 0;
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) m = max(m, (uint32_t)s_raw[(r + dy) * pitch + c + dx]);
        s_dil[r * pitch + c] = (uint8_t)m;
    }
    __syncthreads();
    if (!mine) return;
    int o0[SEAM1_COLS], o1[SEAM1_COLS];
    uint32_t c1[SEAM1_COLS];
#pragma unroll
    for (int j = 0; j < SEAM1_COLS; j++) {
        const int2 t = s_xt[lane * SEAM1_COLS + j];
        o0[j] = t.x - wx0;
        o1[j] = min(t.x + 1, P.sw - 1) - wx0;
        c1[j] = (uint32_t)t.y & 0xffffu;
    }
    uint32_t h0[SEAM1_COLS], h1[SEAM1_COLS];
    int cur = -(1 << 30);
    const uint32_t keep_lo = x8 + 4 <= P.dw ? 0xffffffffu : (x8 + 0 < P.dw ? 0xffffffffu >> (8 * (4 - (P.dw - x8))) : 0u);
    const uint32_t keep_hi = x8 + 8 <= P.dw ? 0xffffffffu : (x8 + 4 < P.dw ? 0xffffffffu >> (8 * (8 - (P.dw - x8))) : 0u);
#pragma unroll
    for (int r = 0; r < SEAM1_ROWS; r++) {
        const int y = yb + r;
        if (y >= P.dh) break;
        const int2 ty = s_yt[wv * SEAM1_ROWS + r];
        const int row = __builtin_amdgcn_readfirstlane(ty.x);
        if (row != cur) {
            cur = row;
            const uint8_t* d0 = s_dil + (cur - wy0) * pitch;
            const uint8_t* d1 = s_dil + (min(cur + 1, P.sh - 1) - wy0) * pitch;
#pragma unroll
            for (int j = 0; j < SEAM1_COLS; j++) {
                const uint32_t a0 = 256u - c1[j];
                h0[j] = (uint32_t)d0[o0[j]] * a0 + (uint32_t)d0[o1[j]] * c1[j];
                h1[j] = (uint32_t)d1[o0[j]] * a0 + (uint32_t)d1[o1[j]] * c1[j];
            }
        }
        const uint32_t cy1 = (uint32_t)__builtin_amdgcn_readfirstlane(ty.y) & 0xffffu, cy0 = 256u - cy1;
        const bool iy = (__builtin_amdgcn_readfirstlane(ty.y) >> 16) != 0;
        uint32_t sum[SEAM1_COLS];  // the result is byte 2 of every sum: (h0 cy0 + h1 cy1 + 2^15) >> 16 <= 255, ((h0 + 128) >> 8) << 16 likewise
#pragma unroll
        for (int j = 0; j < SEAM1_COLS; j++)
            sum[j] = iy ? __umul24(h1[j], cy1) + (__umul24(h0[j], cy0) + 32768u) : (h0[j] + 128u) << 8;
        uint2 out;
        out.x = __builtin_amdgcn_perm(sum[1], sum[0], 0x0c0c0602u) | __builtin_amdgcn_perm(sum[3], sum[2], 0x06020c0cu);
        out.y = __builtin_amdgcn_perm(sum[5], sum[4], 0x0c0c0602u) | __builtin_amdgcn_perm(sum[7], sum[6], 0x06020c0cu);
        out.x &= am[r].x & keep_lo;  // bytes beyond the image inside the row pitch: 0, whatever stands in the final mask's padding
        out.y &= am[r].y & keep_hi;
        *reinterpret_cast<uint2*>(P.dst + (long long)y * P.dstride + x8) = out;
    }
}
}  // namespace

// -> STX_OK and *done = true when the images qualified and the launch was made; *done = false: the caller takes the table path
int stx_launch_seam_resize_lds(stx_ctx* ctx, int n, const stx_buf* const* seams, const stx_buf* const* masks, stx_buf* const* dsts,
                               const int* full_wh_xy0, bool* done)
{
    *done = false;
    static const bool off = getenv("STITCHING_AMD_SEAM_LDS") && atoi(getenv("STITCHING_AMD_SEAM_LDS")) == 0;
    if (off) return STX_OK;
    int pitch = 0, rows = 0;
    for (int i = 0; i < n; i++) {
        const stx_buf *m = masks[i], *d = dsts[i];
        const size_t w8 = ((size_t)d->w + 7) & ~(size_t)7;
        if (((uintptr_t)m->ptr & 7) || (m->stride & 7) || w8 > m->stride || ((uintptr_t)d->ptr & 7) || (d->stride & 7) || w8 > d->stride) return STX_OK;
        const int fw = full_wh_xy0 ? full_wh_xy0[4 * i] : d->w, fh = full_wh_xy0 ? full_wh_xy0[4 * i + 1] : d->h;
        const double xs = 1.0 / ((double)fw / (double)seams[i]->w), ys = 1.0 / ((double)fh / (double)seams[i]->h);
        // source columns / rows under a tile: floor((n - 1) scale) + 2, and one more for the fraction the first one starts at
        pitch = std::max(pitch, std::min(seams[i]->w, (int)std::ceil(SEAM1_TW * xs) + 3) + 2);
        rows = std::max(rows, std::min(seams[i]->h, (int)std::ceil(SEAM1_TH * ys) + 3));
    }
    pitch = (pitch + 3) & ~3;
    const size_t raw_bytes = (size_t)pitch * (rows + 2), lds = raw_bytes + (size_t)pitch * rows;
    if (lds > (40u << 10)) return STX_OK;  // an enlargement factor near 1: the window would not leave room for a second workgroup per CU
    for (int base = 0; base < n; base += SEAM_BATCH) {
        const int m = std::min(SEAM_BATCH, n - base);
        Seam1BatchK B = {};
        B.pitch = pitch; B.raw_bytes = (int)raw_bytes;
        int mdw = 0, mdh = 0;
        double bytes = 0.0;
        for (int i = 0; i < m; i++) {
            const int g = base + i;
            Seam1K& K = B.k[i];
            K.src = seams[g]->ptr; K.sstride = (long long)seams[g]->stride; K.sw = seams[g]->w; K.sh = seams[g]->h;
            K.dst = dsts[g]->ptr; K.dstride = (long long)dsts[g]->stride; K.dw = dsts[g]->w; K.dh = dsts[g]->h;
            K.am = masks[g]->ptr; K.amstride = (long long)masks[g]->stride;
            const int fw = full_wh_xy0 ? full_wh_xy0[4 * g] : K.dw, fh = full_wh_xy0 ? full_wh_xy0[4 * g + 1] : K.dh;
            K.x0 = full_wh_xy0 ? full_wh_xy0[4 * g + 2] : 0; K.y0 = full_wh_xy0 ? full_wh_xy0[4 * g + 3] : 0;
            K.xscale = 1.0 / ((double)fw / (double)K.sw); K.yscale = 1.0 / ((double)fh / (double)K.sh);
            mdw = std::max(mdw, K.dw); mdh = std::max(mdh, K.dh);
            bytes += (double)K.sw * K.sh + 2.0 * K.dw * K.dh;
        }
        StxProfScope prof(ctx, "seam_mask_resize", bytes);
        hipLaunchKernelGGL(seam_resize_lds_kernel, dim3((mdw + SEAM1_TW - 1) / SEAM1_TW, (mdh + SEAM1_TH - 1) / SEAM1_TH, m), dim3(256), lds, ctx->stream, B);
        ctx->seam_resize_paths[0] += m;
    }
    *done = true;
    return stx_check_launch("seam_mask_resize");
}

int stx_launch_resize_exact(stx_ctx* ctx, const stx_buf* src, stx_buf* dst, const int* d_xt, const int* d_yt, bool dilate,
                            const stx_buf* andmask)
{
    ResizeK K;
    K.src = src->ptr; K.sstride = (long long)src->stride; K.sw = src->w; K.sh = src->h;
    K.dst = dst->ptr; K.dstride = (long long)dst->stride; K.dw = dst->w; K.dh = dst->h;
    K.xt = (const int2*)d_xt; K.yt = (const int2*)d_yt;
    K.andmask = andmask ? andmask->ptr : nullptr; K.amstride = andmask ? (long long)andmask->stride : 0;
    const dim3 grid((dst->w + STX_RESIZE_TW - 1) / STX_RESIZE_TW, (dst->h + STX_RESIZE_TH - 1) / STX_RESIZE_TH);
    StxProfScope prof(ctx, dilate ? "seam_mask_resize" : "resize_linear_exact", (double)src->w * src->h * src->c + (double)dst->w * dst->h * dst->c * (andmask ? 2 : 1));
    // dword access to the destination and to the final mask: 4-byte aligned rows (every stx_buf_new image; views may not be),
    // and the mask rows must be readable up to the next multiple of 4 columns
    const bool fast = dilate && andmask && ((uintptr_t)dst->ptr & 3) == 0 && (dst->stride & 3) == 0 && ((uintptr_t)andmask->ptr & 3) == 0 &&
                      (andmask->stride & 3) == 0 && (size_t)((dst->w + 3) & ~3) <= andmask->stride && (size_t)((dst->w + 3) & ~3) <= dst->stride;
    if (fast) {
        StxDevBlock tmp;  // back to the allocator behind the second launch: stream-ordered reuse
        const size_t tstride = ((size_t)src->w + 63) & ~(size_t)63;
        STX_TRY(stx_dev_alloc(ctx, tstride * src->h, &tmp));
        hipLaunchKernelGGL(dilate3x3_kernel, dim3((src->w + 63) / 64, (src->h + 3) / 4), dim3(256), 0, ctx->stream, src->ptr,
                           (long long)src->stride, src->w, src->h, (uint8_t*)tmp.get(), (long long)tstride);
        K.src = (const uint8_t*)tmp.get(); K.sstride = (long long)tstride;
        hipLaunchKernelGGL(seam_resize4_kernel, dim3((dst->w + 255) / 256, (dst->h + 4 * SEAM_ROWS - 1) / (4 * SEAM_ROWS)), dim3(256), 0, ctx->stream, K);
        ctx->seam_resize_paths[2]++;
    } else if (dilate) {
        hipLaunchKernelGGL((resize_exact_kernel<1, true>), grid, dim3(256), 0, ctx->stream, K);
        ctx->seam_resize_paths[3]++;
    }
    else if (src->c == 1) hipLaunchKernelGGL((resize_exact_kernel<1, false>), grid, dim3(256), 0, ctx->stream, K);
    else if (src->c == 3) hipLaunchKernelGGL((resize_exact_kernel<3, false>), grid, dim3(256), 0, ctx->stream, K);
    else return stx_fail(STX_ERR_UNSUPPORTED, "resize: 1 or 3 channels");
    return stx_check_launch("resize_linear_exact");
}

// ---------------------------------------------------------------------------------------------
// cv::resize(INTER_LINEAR_EXACT) of n images of unequal sizes as ONE launch (the LOW pass of Images.resize: 64 frames -> 0.1 Mpx is 64
// launches, table uploads and allocations of a kernel that runs a few microseconds).  The grid is the flat list of the destination
// tiles of all images, image after image: a workgroup finds its image by bisecting the descriptors' first-tile numbers (uniform over
// the workgroup: scalar loads), so no workgroup exists for an image smaller than the largest.  A tile is the single-image kernel's:
// 64 adjacent pixels of a row per wavefront (a row segment leaves as 64 or 192 contiguous bytes), 4 rows per workgroup.  Nothing but
// the descriptors is uploaded: a lane makes its own two coefficients with the IEEE double operations of the host table (seam1_coeff,
// as the one-launch seam-mask resize does) and hands them to the single-image kernel's pixel body.
// ---------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void resize_exact_batch_kernel(const StxResizeItem* __restrict__ items, int n)
{
    const int tile = blockIdx.x;
    int lo = 0, hi = n - 1;  // the last image whose first tile is <= tile (tile0 is ascending, items[0].tile0 = 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const StxResizeItem& D = items[lo];
    const int t = tile - D.tile0, tyi = t / D.tiles_x, txi = t - tyi * D.tiles_x;
    const int x = txi * STX_RESIZE_TW + (threadIdx.x & 63);
    const int y = tyi * STX_RESIZE_TH + (threadIdx.x >> 6);
    if (x >= D.dw || y >= D.dh) return;
    ResizeK P;
    P.src = D.src; P.sstride = D.sstride; P.sw = D.sw; P.sh = D.sh;
    P.dst = D.dst; P.dstride = D.dstride; P.dw = D.dw; P.dh = D.dh;
    P.xt = nullptr; P.yt = nullptr; P.andmask = nullptr; P.amstride = 0;
    const int2 tx = seam1_coeff(x, D.xscale, D.sw), ty = seam1_coeff(y, D.yscale, D.sh);
    if (D.c == 3) resize_exact_pixel<3, false>(P, x, y, tx, ty);
    else resize_exact_pixel<1, false>(P, x, y, tx, ty);
}
}  // namespace

int stx_launch_resize_exact_batch(stx_ctx* ctx, const StxResizeItem* d_items, int n, int total_tiles, double algo_bytes)
{
    StxProfScope prof(ctx, "resize_linear_exact_batch", algo_bytes);
    hipLaunchKernelGGL(resize_exact_batch_kernel, dim3(total_tiles), dim3(256), 0, ctx->stream, d_items, n);
    return stx_check_launch("resize_linear_exact_batch");
}

// ---------------------------------------------------------------------------------------------
// Conservative shrink of source validity masks (stx_mask_shrink_batch): destination pixel (x, y) of a dw x dh result is 255 iff EVERY
// source pixel of its footprint — columns [x sw / dw, ((x + 1) sw + dw - 1) / dw), rows likewise, integer divisions — is non-zero,
// else 0: a pixel of the smaller frame counts as picture only where all the pixels it was averaged from are.  Integers only.  The grid
// is the flat tile list of the batched resize above; a lane owns one destination pixel and walks its footprint (dw <= sw, dh <= sh:
// never empty, never beyond the source: ((x + 1) sw + dw - 1) / dw <= sw for x + 1 <= dw).
// ---------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void mask_shrink_batch_kernel(const StxResizeItem* __restrict__ items, int n)
{
    const int tile = blockIdx.x;
    int lo = 0, hi = n - 1;  // the last image whose first tile is <= tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const StxResizeItem& D = items[lo];
    const int t = tile - D.tile0, tyi = t / D.tiles_x, txi = t - tyi * D.tiles_x;
    const int x = txi * STX_RESIZE_TW + (threadIdx.x & 63);
    const int y = tyi * STX_RESIZE_TH + (threadIdx.x >> 6);
    if (x >= D.dw || y >= D.dh) return;
    const int x0 = (int)((long long)x * D.sw / D.dw), x1 = (int)(((long long)(x + 1) * D.sw + D.dw - 1) / D.dw);
    const int y0 = (int)((long long)y * D.sh / D.dh), y1 = (int)(((long long)(y + 1) * D.sh + D.dh - 1) / D.dh);
    bool all = true;
    for (int sy = y0; sy < y1 && all; sy++) {
        const uint8_t* row = D.src + (long long)sy * D.sstride;
        for (int sx = x0; sx < x1; sx++) all = all && row[sx] != 0;
    }
    D.dst[(long long)y * D.dstride + x] = all ? 255 : 0;
}
}  // namespace

int stx_launch_mask_shrink_batch(stx_ctx* ctx, const StxResizeItem* d_items, int n, int total_tiles, double algo_bytes)
{
    StxProfScope prof(ctx, "mask_shrink_batch", algo_bytes);
    hipLaunchKernelGGL(mask_shrink_batch_kernel, dim3(total_tiles), dim3(256), 0, ctx->stream, d_items, n);
    return stx_check_launch("mask_shrink_batch");
}
