// stx_gain.hip — exposure gains multiplied into warped images on gfx950: one gain per image or channel, and block gain maps.
//
// Replaces, for stitching/exposure_error_compensator.py's apply(), OpenCV's GainCompensator::apply / ChannelsCompensator::apply
// (cv::multiply by a scalar) and BlocksCompensator::apply (cv::resize(INTER_LINEAR) of the gain map + cv::multiply).  These are "next"
// rows of the scope table: consumers / producers either side of the warp -> blend path.  Host side: stx_gain_host.cpp;
// stx_warp_host.cpp and stx_exposure_host.cpp call stx_launch_gain_rows for kernels that multiply the gain in themselves.
#include <algorithm>
#include <cstring>

#include "stx_device_math.h"
#include "stx_internal.h"

using namespace stxd;

namespace {
// GainCompensator::apply / ChannelsCompensator::apply: cv::multiply(u8x3 image, double scalar) evaluates in fp32
// (arithm_op demotes a CV_64F scalar to CV_32F for 8-bit sources) and stores saturate_cast<uchar>(float) = cvRound + clamp
// dwords: host-proved, the first row and the row pitch are multiples of 4 bytes, so every 4-pixel group starts on a dword.  A view
// (odd first column, odd pitch) is not: its rows go byte by byte, 4 pixels per lane all the same
struct GainK { uint8_t* img; long long stride; int w, h; float g[3]; int dwords; };
__global__ __launch_bounds__(256) void gain_apply_kernel(GainK P)
{
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;  // 4 pixels = 12 bytes = 3 dwords per lane
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x4 >= P.w || y >= P.h) return;
    uint8_t* row = P.img + (long long)y * P.stride;
    if (P.dwords && x4 + 4 <= P.w) {
        uint32_t* q = reinterpret_cast<uint32_t*>(row + (long long)x4 * 3);
        uint32_t d[3] = {q[0], q[1], q[2]}, o[3] = {0, 0, 0};
#pragma unroll
        for (int b = 0; b < 12; b++) {
            const float v = stxd::fmul((float)((d[b >> 2] >> (8 * (b & 3))) & 255u), P.g[b % 3]);
            const int r = min(max(stxd::cv_round(v), 0), 255);
            o[b >> 2] |= (uint32_t)r << (8 * (b & 3));
        }
        q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
    } else {
        const int xe = min(x4 + 4, P.w);
        for (int x = x4; x < xe; x++)
            for (int c = 0; c < 3; c++) {
                const float v = stxd::fmul((float)row[x * 3 + c], P.g[c]);
                row[x * 3 + c] = (uint8_t)min(max(stxd::cv_round(v), 0), 255);
            }
    }
}
}  // namespace

int stx_launch_gain_apply(stx_ctx* ctx, stx_buf* img, const float g[3])
{
    GainK K;
    K.img = img->ptr; K.stride = (long long)img->stride; K.w = img->w; K.h = img->h;
    K.g[0] = g[0]; K.g[1] = g[1]; K.g[2] = g[2];
    K.dwords = ((uintptr_t)img->ptr & 3) == 0 && (img->stride & 3) == 0;
    StxProfScope prof(ctx, "gain_apply", 6.0 * img->w * img->h);
    hipLaunchKernelGGL(gain_apply_kernel, dim3((img->w + 255) / 256, (img->h + 3) / 4), dim3(256), 0, ctx->stream, K);
    return stx_check_launch("gain_apply");
}

// ---------------------------------------------------------------------------------------------
// BlocksCompensator::apply (next row N1, the reference's default "gain_blocks" compensator): the small fp32 gain map is
// interpolated to the image size exactly as cv::resize(INTER_LINEAR) does for CV_32F — fp32 throughout, horizontal
// S[s] * a0 + S[s+1] * a1 (S[s] alone at the right end), vertical R0 * b0 + R1 * b1 with the rows clamped, no FMA — and
// multiplied in with cv::multiply's fp32 product + cvRound + saturation.  Fused: the full-size gain map never exists.
// Tables (host, double -> float as upstream): x = (s, bits of f), y likewise (s may be -1).
// ---------------------------------------------------------------------------------------------
namespace {
struct BlockGainK {
    uint8_t* img; long long stride; int w, h;
    const float* gmap; long long gstride; int gw, gh, gc;  // gstride in floats; gc = 1 (one map) or 3 (BGR maps, interleaved)
    const int2* xt; const int2* yt;
};
STX_DEV float gain_hrow(const BlockGainK& P, int row, int sx, int ch, float a0, float a1)
{
    const float* r = P.gmap + (long long)row * P.gstride + ch;
    if (sx >= P.gw - 1) return r[sx * P.gc];
    return stxd::fadd(stxd::fmul(r[sx * P.gc], a0), stxd::fmul(r[(sx + 1) * P.gc], a1));
}
__global__ __launch_bounds__(256) void block_gain_kernel(BlockGainK P)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= P.w || y >= P.h) return;
    const int2 tx = P.xt[x], ty = P.yt[y];
    const float a1 = __int_as_float(tx.y), a0 = stxd::fsub(1.f, a1), b1 = __int_as_float(ty.y), b0 = stxd::fsub(1.f, b1);
    const int r0 = min(max(ty.x, 0), P.gh - 1), r1 = min(max(ty.x + 1, 0), P.gh - 1);
    uint8_t* p = P.img + (long long)y * P.stride + x * 3;
    float g = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c == 0 || P.gc == 3)
            g = stxd::fadd(stxd::fmul(gain_hrow(P, r0, tx.x, c, a0, a1), b0), stxd::fmul(gain_hrow(P, r1, tx.x, c, a0, a1), b1));
        p[c] = (uint8_t)min(max(stxd::cv_round(stxd::fmul((float)p[c], g)), 0), 255);
    }
}
}  // namespace

int stx_launch_block_gain(stx_ctx* ctx, stx_buf* img, const stx_buf* gmap, const int* d_xt, const int* d_yt)
{
    BlockGainK K;
    K.img = img->ptr; K.stride = (long long)img->stride; K.w = img->w; K.h = img->h;
    K.gmap = (const float*)gmap->ptr; K.gstride = (long long)(gmap->stride / sizeof(float)); K.gw = gmap->w; K.gh = gmap->h;
    K.gc = gmap->c;
    K.xt = (const int2*)d_xt; K.yt = (const int2*)d_yt;
    StxProfScope prof(ctx, "block_gain_apply", 6.0 * img->w * img->h);
    hipLaunchKernelGGL(block_gain_kernel, dim3((img->w + 63) / 64, (img->h + 3) / 4), dim3(256), 0, ctx->stream, K);
    return stx_check_launch("block_gain_apply");
}

// ---------------------------------------------------------------------------------------------
// The same product for all images of a panorama in two launches, at HBM rate (stx_block_gain_apply_batch).  cv::resize(INTER_LINEAR)
// is separable and rounds each pass to fp32, so the horizontal pass is made ONCE per gain-map row: H[r][x] = S[r][s] a0 + S[r][s+1] a1
// for every column x of the image (gain_rows_kernel: gh x w floats per image, a few hundred KB, L2 resident; the coefficient set-up
// f = (float)((x + 0.5) scale - 0.5) runs on the device in IEEE double, operation for operation the host loop of linear_f32_table).
// The product pass then needs two 16-byte reads of H per 4 pixels and row: g = H[r0][x] b0 + H[r1][x] b1, cvRound(p g) saturated.
// One lane = 4 pixels (three dwords in, three out), one wavefront = 256 pixels of a row, 4 rows one after the other.
// An image may be the rectangle at (x0, y0) of a larger warped image (full_w x full_h: StitchJob's seam-cell crops): the gain map is
// laid over the FULL image, as BlocksCompensator::apply lays it over the whole warped image.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int GAIN_BATCH = 16;
struct BlockGain4K {
    uint8_t* img; long long stride; int w, h;          // the (sub-)image, whole rows of the library's own buffers (4-pixel groups)
    int x0, y0, full_w, full_h;                        // its place in the full warped image
    const float* gmap; long long gstride; int gw, gh;  // gstride in floats
    double xscale, yscale;                             // 1 / (full / gain-map size), host double
    float* H; long long hstride;                       // [gh][hstride] floats x GC; hstride = w rounded up to 4 (x GC)
    int2* yt;                                          // [h]: (source row, bits of the fraction)
    int fast;                                          // host-proved: every gain finite and below 2^31 / 255 (no product leaves int range)
};
struct BlockGainBatchK { BlockGain4K k[GAIN_BATCH]; };

STX_DEV void gain_coeff(int d, double scale, int src_n, bool clamp, int& sidx, float& f)
{
    f = (float)(((double)d + 0.5) * scale - 0.5);
    sidx = (int)floorf(f);
    f = stxd::fsub(f, (float)sidx);
    if (clamp) {
        if (sidx < 0) { sidx = 0; f = 0.f; }
        else if (sidx >= src_n - 1) { sidx = src_n - 1; f = 0.f; }
    }
}

template <int GC>
__global__ __launch_bounds__(256) void gain_rows_kernel(BlockGainBatchK B)
{
    const BlockGain4K& P = B.k[blockIdx.z];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.y == 0) {  // row table
        if (i < P.h) {
            int sy; float f;
            gain_coeff(P.y0 + i, P.yscale, P.gh, false, sy, f);
            P.yt[i] = make_int2(sy, __float_as_int(f));
        }
        return;
    }
    const int r = blockIdx.y - 1;  // gain-map row
    // the columns w .. round_up4(w) - 1 of the row pitch are written too (the gain of the last column): the consumers read a row in
    // groups of 4 and multiply the image's ROW PADDING with what stands there — scratch left as it was made those padding bytes differ
    // from run to run
    const int wpad = (P.w + 3) & ~3;
    if (r >= P.gh || i >= wpad) return;
    int sx; float a1;
    gain_coeff(P.x0 + min(i, P.w - 1), P.xscale, P.gw, true, sx, a1);
    const float a0 = stxd::fsub(1.f, a1);
    const float* row = P.gmap + (long long)r * P.gstride;
#pragma unroll
    for (int c = 0; c < GC; c++) {
        float v;
        if (sx >= P.gw - 1) v = row[sx * GC + c];
        else v = stxd::fadd(stxd::fmul(row[sx * GC + c], a0), stxd::fmul(row[(sx + 1) * GC + c], a1));
        P.H[(long long)r * P.hstride + (long long)i * GC + c] = v;
    }
}

// cvRound(p g) saturated to u8 into byte `sel` of `old`: v_cvt_pk_u8_f32 is the round-half-even of cvRound AND the saturation
template <bool FAST>
STX_DEV uint32_t gain_px(uint32_t old, int sel, float p, float g)
{
    float v = stxd::fmul(p, g);
    if (!FAST) v = v < 2147483648.f ? v : 0.f;  // cvRound's INT_MIN for NaN / out-of-range products saturates to 0
    return __builtin_amdgcn_cvt_pk_u8_f32(v, (uint32_t)sel, old);  // rounds to nearest even and saturates itself: tools/ubench/cvt_pk_u8.hip
}

template <int GC, bool FAST>
__global__ __launch_bounds__(256) void block_gain4_kernel(BlockGainBatchK B)
{
    const BlockGain4K& P = B.k[blockIdx.z];
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (x4 >= P.w) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = blockIdx.y * 16 + wv * 4 + j;
        if (y >= P.h) break;
        const int2 ty = P.yt[y];
        const float b1 = __int_as_float(ty.y), b0 = stxd::fsub(1.f, b1);
        const int r0 = min(max(ty.x, 0), P.gh - 1), r1 = min(max(ty.x + 1, 0), P.gh - 1);
        const float* h0 = P.H + (long long)r0 * P.hstride + (long long)x4 * GC;
        const float* h1 = P.H + (long long)r1 * P.hstride + (long long)x4 * GC;
        float g[4 * GC];
#pragma unroll
        for (int q = 0; q < GC; q++) {
            const float4 u = reinterpret_cast<const float4*>(h0)[q], v = reinterpret_cast<const float4*>(h1)[q];
            g[4 * q + 0] = stxd::fadd(stxd::fmul(u.x, b0), stxd::fmul(v.x, b1));
            g[4 * q + 1] = stxd::fadd(stxd::fmul(u.y, b0), stxd::fmul(v.y, b1));
            g[4 * q + 2] = stxd::fadd(stxd::fmul(u.z, b0), stxd::fmul(v.z, b1));
            g[4 * q + 3] = stxd::fadd(stxd::fmul(u.w, b0), stxd::fmul(v.w, b1));
        }
        uint32_t* p = reinterpret_cast<uint32_t*>(P.img + (long long)y * P.stride + (long long)x4 * 3);
        uint32_t d[3] = {p[0], p[1], p[2]}, o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 12; k++) {  // byte k of the 12: pixel k / 3, channel k % 3
            const float pv = (float)((d[k >> 2] >> (8 * (k & 3))) & 255u);
            o[k >> 2] = gain_px<FAST>(o[k >> 2], k & 3, pv, GC == 1 ? g[k / 3] : g[k]);
        }
        p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
    }
}
}  // namespace

// H rows + row tables of n rectangles (see stx_launch_block_gain_batch); imgs may be null (a consumer that multiplies the gain in itself)
static void fill_gain_k(BlockGain4K& K, stx_buf* img, int w, int h, const stx_buf* gmap, const int* q, float* H, void* yt, int fast)
{
    K.img = img ? img->ptr : nullptr; K.stride = img ? (long long)img->stride : 0; K.w = w; K.h = h;
    K.full_w = q ? q[0] : w; K.full_h = q ? q[1] : h;
    K.x0 = q ? q[2] : 0; K.y0 = q ? q[3] : 0;
    K.gmap = (const float*)gmap->ptr; K.gstride = (long long)(gmap->stride / sizeof(float));
    K.gw = gmap->w; K.gh = gmap->h;
    K.xscale = 1.0 / ((double)K.full_w / (double)K.gw);
    K.yscale = 1.0 / ((double)K.full_h / (double)K.gh);
    K.H = H; K.hstride = (long long)((w + 3) & ~3) * gmap->c;
    K.yt = (int2*)yt;
    K.fast = fast;
}

static void launch_gain_rows(stx_ctx* ctx, const BlockGainBatchK& B, int m, int gc)
{
    int mt = 0, mgh = 0;
    double rows_bytes = 0.0;
    for (int i = 0; i < m; i++) {
        mt = std::max(mt, std::max(B.k[i].w, B.k[i].h));
        mgh = std::max(mgh, B.k[i].gh);
        rows_bytes += 4.0 * gc * B.k[i].gh * B.k[i].w + 8.0 * B.k[i].h;
    }
    StxProfScope prof(ctx, "block_gain_rows", rows_bytes);
    const dim3 grid((mt + 255) / 256, mgh + 1, m);
    if (gc == 1) hipLaunchKernelGGL(gain_rows_kernel<1>, grid, dim3(256), 0, ctx->stream, B);
    else hipLaunchKernelGGL(gain_rows_kernel<3>, grid, dim3(256), 0, ctx->stream, B);
}

int stx_launch_gain_rows(stx_ctx* ctx, int n, const int* wh, const stx_buf* const* gmaps, const int* full_wh_xy0, float* const* Hs,
                         void* const* yts)
{
    for (int base = 0; base < n; base += GAIN_BATCH) {
        const int m = std::min(GAIN_BATCH, n - base);
        BlockGainBatchK B;
        memset(&B, 0, sizeof(B));
        for (int i = 0; i < m; i++) {
            const int g = base + i;
            fill_gain_k(B.k[i], nullptr, wh[2 * g], wh[2 * g + 1], gmaps[g], full_wh_xy0 ? full_wh_xy0 + 4 * g : nullptr, Hs[g], yts[g], 1);
        }
        launch_gain_rows(ctx, B, m, gmaps[base]->c);
    }
    return stx_check_launch("block_gain_rows");
}

// Hs / yts: per image device scratch (gh x hstride x gc floats, h int2), carved by the caller from one allocation
int stx_launch_block_gain_batch(stx_ctx* ctx, int n, stx_buf* const* imgs, const stx_buf* const* gmaps, const int* full_wh_xy0,
                                float* const* Hs, void* const* yts, const int* fast)
{
    for (int base = 0; base < n; base += GAIN_BATCH) {
        const int m = std::min(GAIN_BATCH, n - base);
        const int gc = gmaps[base]->c;
        BlockGainBatchK B;
        memset(&B, 0, sizeof(B));
        int mw = 0, mh = 0;
        bool all_fast = true;
        double bytes = 0.0;
        for (int i = 0; i < m; i++) {
            const int g = base + i;
            fill_gain_k(B.k[i], imgs[g], imgs[g]->w, imgs[g]->h, gmaps[g], full_wh_xy0 ? full_wh_xy0 + 4 * g : nullptr, Hs[g], yts[g], fast[g]);
            all_fast = all_fast && fast[g];
            mw = std::max(mw, B.k[i].w); mh = std::max(mh, B.k[i].h);
            bytes += 6.0 * B.k[i].w * B.k[i].h;
        }
        launch_gain_rows(ctx, B, m, gc);
        StxProfScope prof(ctx, "block_gain_apply", bytes);
        const dim3 grid((mw + 255) / 256, (mh + 15) / 16, m);
        if (gc == 1 && all_fast) hipLaunchKernelGGL((block_gain4_kernel<1, true>), grid, dim3(256), 0, ctx->stream, B);
        else if (gc == 1) hipLaunchKernelGGL((block_gain4_kernel<1, false>), grid, dim3(256), 0, ctx->stream, B);
        else if (all_fast) hipLaunchKernelGGL((block_gain4_kernel<3, true>), grid, dim3(256), 0, ctx->stream, B);
        else hipLaunchKernelGGL((block_gain4_kernel<3, false>), grid, dim3(256), 0, ctx->stream, B);
    }
    return stx_check_launch("block_gain_apply");
}
