// stx_emit.hip — device frame emit: images of the library's own -> the caller's surfaces, n items of unequal sizes and formats in ONE
// launch (tests/numpy_emit.py is the contract, byte for byte).  The mirror of stx_ingest.hip, with its geometry:
// lanes run along x with STX_INGEST_LANE_PX pixels each, a workgroup is 64 lanes x STX_INGEST_ROWS row units, the grid is the flat list
// of the items' tiles.  The 4:2:0 formats take two rows per lane, so a block's chroma is made from the loads its luma needs anyway.
// Every load of a lane is issued before its arithmetic; no LDS.
//
// Alignment is the buffer's, not assumed, on BOTH sides: a source may be a crop view that starts at any x, a target has any base and
// pitch.  The host marks the source, the alpha image and each target plane "wide" (base and pitch multiples of the access) or not; a
// lane of a wide buffer that owns all its pixels moves whole words, every other lane — a narrow buffer, the last lane of a row, the
// last row of an odd height — moves exactly the bytes it owns, one at a time.  No store lands in a target row's padding or past a
// plane's last byte; no load reaches past a source row's last pixel.
#include "stx_internal.h"
#include "stx_lane_io.h"

namespace {
// clip8(s >> SH) with the offset and the rounding term already in s, clamped BEFORE the shift, as shift_clip8 of stx_ingest.hip and for
// its reason (the packed shift-and-saturate instruction the other order selects returned wrong bytes on the MI355X):
// min(max(s, 0), (256 << SH) - 1) >> SH is the same value for every int s.
template <int SH>
__device__ __forceinline__ uint32_t shift_clip8(int s) { return (uint32_t)min(max(s, 0), (256 << SH) - 1) >> SH; }

// four BGR pixels at p: three words, or — a tail lane, a source that starts at an odd byte — pixel min(i, npx - 1) for i = 0 .. 3 byte by
// byte: what lies past the row's end repeats its last pixel, which is the contract's clamped coordinate
__device__ __forceinline__ void load_bgr4(const uint8_t* __restrict__ p, int npx, bool words, uint32_t (&s)[3])
{
    if (words) {
#pragma unroll
        for (int i = 0; i < 3; i++) s[i] = ((const uint32_t*)p)[i];
    } else {
        s[0] = s[1] = s[2] = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint8_t* q = p + min(i, npx - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int j = i * 3 + c;
                s[j >> 2] |= (uint32_t)q[c] << ((j & 3) * 8);
            }
        }
    }
}

// a row of bytes, 16 per lane
__device__ __forceinline__ void copy_lane(const StxEmitItem& D, int xu, int y)
{
    const int xb = xu * 4;  // xu counts 4-byte words
    const int n = min(16, D.w - xb);
    if (n <= 0) return;
    uint32_t s[4];
    load_words<4>(D.src + (long long)y * D.sstride + xb, n, (D.wide & STX_EMIT_WIDE_SRC) && n == 16, s);
    store_words<4>(D.dst[0] + (long long)y * D.dpitch[0] + xb, s, n, (D.wide & STX_EMIT_WIDE_DST0) && n == 16);
}

// 3-byte pixels with the first and third channel swapped
__device__ __forceinline__ void rev3_lane(const StxEmitItem& D, int x, int y)
{
    const int npx = min(STX_INGEST_LANE_PX, D.w - x);
    if (npx <= 0) return;
    const bool full = npx == STX_INGEST_LANE_PX;
    uint32_t s[3], o[3] = {0u, 0u, 0u};
    load_words<3>(D.src + (long long)y * D.sstride + (long long)x * 3, npx * 3, (D.wide & STX_EMIT_WIDE_SRC) && full, s);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int j = i * 3 + c;
            o[j >> 2] |= byte_of(s, i * 3 + 2 - c) << ((j & 3) * 8);
        }
    store_words<3>(D.dst[0] + (long long)y * D.dpitch[0] + (long long)x * 3, o, npx * 3, (D.wide & STX_EMIT_WIDE_DST0) && full);
}

// 3-byte pixels -> 4-byte pixels: the alpha image's byte, or 255, behind the colour; REV swaps the first and third channel
template <bool REV>
__device__ __forceinline__ void alpha_lane(const StxEmitItem& D, int x, int y)
{
    const int npx = min(STX_INGEST_LANE_PX, D.w - x);
    if (npx <= 0) return;
    const bool full = npx == STX_INGEST_LANE_PX;
    uint32_t s[3], a[1] = {0xffffffffu}, o[4];
    load_words<3>(D.src + (long long)y * D.sstride + (long long)x * 3, npx * 3, (D.wide & STX_EMIT_WIDE_SRC) && full, s);
    if (D.alpha) load_words<1>(D.alpha + (long long)y * D.astride + x, npx, (D.wide & STX_EMIT_WIDE_ALPHA) && full, a);
#pragma unroll
    for (int i = 0; i < 4; i++)
        o[i] = byte_of(s, i * 3 + (REV ? 2 : 0)) | (byte_of(s, i * 3 + 1) << 8) | (byte_of(s, i * 3 + (REV ? 0 : 2)) << 16) | (byte_of(a, i) << 24);
    store_words<4>(D.dst[0] + (long long)y * D.dpitch[0] + (long long)x * 4, o, npx * 4, (D.wide & STX_EMIT_WIDE_DST0) && full);
}

// BGR -> 4:2:0: four pixels of two rows; PLANAR: U and V planes (I420), else interleaved pairs (NV12)
template <bool PLANAR>
__device__ __forceinline__ void yuv_lane(const StxEmitItem& D, const StxEmitCoef& K, int x, int y)
{
    const int npx = min(STX_INGEST_LANE_PX, D.w - x);
    if (npx <= 0) return;
    const bool full = npx == STX_INGEST_LANE_PX, two = y + 1 < D.h;
    const int nch = (npx + 1) >> 1;  // chroma samples of the lane
    const uint8_t* ps = D.src + (long long)y * D.sstride + (long long)x * 3;
    const bool sw = (D.wide & STX_EMIT_WIDE_SRC) && full;
    uint32_t rows[2][3];
    load_bgr4(ps, npx, sw, rows[0]);
    load_bgr4(two ? ps + D.sstride : ps, npx, sw, rows[1]);  // the last row of an odd height is its own partner
    const int ybias = 32768 + (K.yoff << 16), cbias = 131072 + (128 << 18);
    uint32_t yo[2][1] = {{0u}, {0u}};
    int sb[2] = {0, 0}, sg[2] = {0, 0}, sr[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int b = (int)byte_of(rows[r], i * 3), g = (int)byte_of(rows[r], i * 3 + 1), rd = (int)byte_of(rows[r], i * 3 + 2);
            yo[r][0] |= shift_clip8<16>(K.ky[0] * b + K.ky[1] * g + K.ky[2] * rd + ybias) << (8 * i);
            sb[i >> 1] += b; sg[i >> 1] += g; sr[i >> 1] += rd;
        }
    uint32_t u[2], v[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        u[k] = shift_clip8<18>(K.ku[0] * sb[k] + K.ku[1] * sg[k] + K.ku[2] * sr[k] + cbias);
        v[k] = shift_clip8<18>(K.kv[0] * sb[k] + K.kv[1] * sg[k] + K.kv[2] * sr[k] + cbias);
    }
    uint8_t* py = D.dst[0] + (long long)y * D.dpitch[0] + x;
    const bool yw = (D.wide & STX_EMIT_WIDE_DST0) && full;
    store_words<1>(py, yo[0], npx, yw);
    if (two) store_words<1>(py + D.dpitch[0], yo[1], npx, yw);
    if (PLANAR) {
        store_pair(D.dst[1] + (long long)(y >> 1) * D.dpitch[1] + (x >> 1), u[0] | (u[1] << 8), nch, (D.wide & (STX_EMIT_WIDE_DST0 << 1)) && full);
        store_pair(D.dst[2] + (long long)(y >> 1) * D.dpitch[2] + (x >> 1), v[0] | (v[1] << 8), nch, (D.wide & (STX_EMIT_WIDE_DST0 << 2)) && full);
    } else {
        // U0 V0 U1 V1: x is a multiple of 4, so the pair of pixel x starts at byte x of the row
        const uint32_t uv[1] = {u[0] | (v[0] << 8) | (u[1] << 16) | (v[1] << 24)};
        store_words<1>(D.dst[1] + (long long)(y >> 1) * D.dpitch[1] + x, uv, nch * 2, (D.wide & (STX_EMIT_WIDE_DST0 << 1)) && full);
    }
}

__global__ __launch_bounds__(256) void emit_kernel(const StxEmitItem* __restrict__ items, int n, StxEmitCoef K)
{
    const int tile = blockIdx.x;
    int lo = 0, hi = n - 1;  // the last item whose first tile is <= tile (tile0 is ascending, items[0].tile0 = 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const StxEmitItem D = items[lo];
    const int t = tile - D.tile0, tyi = t / D.tiles_x, txi = t - tyi * D.tiles_x;
    const int xu = (txi * 64 + (int)(threadIdx.x & 63)) * STX_INGEST_LANE_PX;  // first pixel (COPY: first word) of the lane
    const int ru = tyi * STX_INGEST_ROWS + (int)(threadIdx.x >> 6);           // row unit
    const bool yuv = D.kind == STX_EMIT_K_NV12 || D.kind == STX_EMIT_K_I420;
    const int y = yuv ? ru * 2 : ru;
    if (y >= D.h) return;
    switch (D.kind) {  // uniform over the workgroup
    case STX_EMIT_K_COPY: copy_lane(D, xu, y); break;
    case STX_EMIT_K_REV3: rev3_lane(D, xu, y); break;
    case STX_EMIT_K_ALPHA:
        if (D.reverse) alpha_lane<true>(D, xu, y); else alpha_lane<false>(D, xu, y);
        break;
    case STX_EMIT_K_NV12: yuv_lane<false>(D, K, xu, y); break;
    default: yuv_lane<true>(D, K, xu, y); break;
    }
}
}  // namespace

int stx_launch_emit(stx_ctx* ctx, const StxEmitItem* d_items, int n, int total_tiles, const StxEmitCoef& coef, double algo_bytes)
{
    StxProfScope prof(ctx, "emit", algo_bytes);
    hipLaunchKernelGGL(emit_kernel, dim3(total_tiles), dim3(256), 0, ctx->stream, d_items, n, coef);
    return stx_check_launch("emit");
}
