// stx_ingest.hip — device frame ingest: foreign device memory -> images of the library's own, n frames of unequal sizes and formats
// in ONE launch (tests/numpy_ingest.py is the contract, byte for byte).
//
// A pure stream: lanes run along x with STX_INGEST_LANE_PX pixels each, a workgroup is 64 lanes x STX_INGEST_ROWS row units, the grid
// is the flat list of the frames' tiles.  The 4:2:0 formats take two rows per lane, so a chroma pair is loaded once for its 2 x 2
// block.  Every load of a lane is issued before its arithmetic; no LDS.
//
// Alignment is the frame's, not assumed: the host marks each source plane "wide" (base and pitch multiples of the access) or not, and
// a lane of a wide plane that owns all its pixels reads whole words.  Every other lane — a plane that starts at an odd byte, the last
// lane of a row (1 .. 4 pixels), the last row pair of an odd height (one row) — reads exactly the bytes it owns, one at a time: no load
// reaches past a plane's last byte, which is all the host has checked against the allocation.  The destination is an image of the
// library's own (base and pitch multiples of 64): a full lane stores words, a tail lane the bytes of its pixels.
#include "stx_internal.h"
#include "stx_lane_io.h"

namespace {
// clip8(s >> 8) of the contract, clamped BEFORE the shift: min(max(s, 0), 65535) >> 8 is the same value for every int s (s < 0 -> 0,
// s >= 65536 -> 255, floor in between) and compiles to v_med3_i32 and a shift.  Written as shift-then-clamp, the compiler selects
// v_ashr_pk_u8_i32 for pairs of these bytes, and the MI355X then returned a wrong byte beside one that saturates (R = 255 for 198 next
// to a clipped B; the same source run as host C++ is right): keep this form, and look for that instruction in the ISA after a change.
__device__ __forceinline__ uint32_t shift_clip8(int s) { return (uint32_t)min(max(s, 0), 65535) >> 8; }

// a row of bytes, 16 per lane
__device__ __forceinline__ void copy_lane(const StxIngestItem& D, int xu, int y)
{
    const int xb = xu * 4;  // xu counts 4-byte words
    const int n = min(16, D.w - xb);
    if (n <= 0) return;
    uint32_t s[4];
    load_words<4>(D.p[0] + (long long)y * D.pitch[0] + xb, n, (D.wide & 1) && n == 16, s);
    store_words<4>(D.dst + (long long)y * D.dstride + xb, s, n);
}

// CPP-byte pixels -> 3-byte pixels: alpha dropped (CPP = 4), first and third channel swapped (REV)
template <int CPP, bool REV>
__device__ __forceinline__ void pack_lane(const StxIngestItem& D, int x, int y)
{
    const int npx = min(STX_INGEST_LANE_PX, D.w - x);
    if (npx <= 0) return;
    uint32_t s[CPP], o[3] = {0u, 0u, 0u};
    load_words<CPP>(D.p[0] + (long long)y * D.pitch[0] + (long long)x * CPP, npx * CPP, (D.wide & 1) && npx == STX_INGEST_LANE_PX, s);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int j = i * 3 + c;
            o[j >> 2] |= byte_of(s, i * CPP + (REV ? 2 - c : c)) << ((j & 3) * 8);
        }
    store_words<3>(D.dst + (long long)y * D.dstride + (long long)x * 3, o, npx * 3);
}

// 4:2:0 -> BGR: four pixels of two rows; PLANAR: U and V planes (I420), else interleaved pairs (NV12)
template <bool PLANAR>
__device__ __forceinline__ void yuv_lane(const StxIngestItem& D, const StxIngestCoef& K, int x, int y)
{
    const int npx = min(STX_INGEST_LANE_PX, D.w - x);
    if (npx <= 0) return;
    const bool full = npx == STX_INGEST_LANE_PX, two = y + 1 < D.h;
    const int nch = (npx + 1) >> 1;  // chroma samples of the lane
    uint32_t y0[1], y1[1] = {0u}, u2, v2;
    const uint8_t* py = D.p[0] + (long long)y * D.pitch[0] + x;
    load_words<1>(py, npx, (D.wide & 1) && full, y0);
    if (two) load_words<1>(py + D.pitch[0], npx, (D.wide & 1) && full, y1);
    if (PLANAR) {
        u2 = load_pair(D.p[1] + (long long)(y >> 1) * D.pitch[1] + (x >> 1), nch, (D.wide & 2) && full);
        v2 = load_pair(D.p[2] + (long long)(y >> 1) * D.pitch[2] + (x >> 1), nch, (D.wide & 4) && full);
    } else {
        uint32_t uv[1];  // U0 V0 U1 V1: x is a multiple of 4, so the pair of pixel x starts at byte x of the row
        load_words<1>(D.p[1] + (long long)(y >> 1) * D.pitch[1] + x, nch * 2, (D.wide & 2) && full, uv);
        u2 = (uv[0] & 255u) | ((uv[0] >> 8) & 0xff00u);
        v2 = ((uv[0] >> 8) & 255u) | ((uv[0] >> 16) & 0xff00u);
    }
    int rt[2], gt[2], bt[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int d = (int)((u2 >> (8 * k)) & 255u) - 128, e = (int)((v2 >> (8 * k)) & 255u) - 128;
        rt[k] = K.rv * e + 128;
        gt[k] = -K.gu * d - K.gv * e + 128;
        bt[k] = K.bu * d + 128;
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r == 1 && !two) break;
        const uint32_t yy = r == 0 ? y0[0] : y1[0];
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = K.yk * ((int)((yy >> (8 * i)) & 255u) - K.yoff), k = i >> 1;
            const uint32_t bgr[3] = {shift_clip8(c + bt[k]), shift_clip8(c + gt[k]), shift_clip8(c + rt[k])};
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int j = i * 3 + ch;
                o[j >> 2] |= bgr[ch] << ((j & 3) * 8);
            }
        }
        store_words<3>(D.dst + (long long)(y + r) * D.dstride + (long long)x * 3, o, npx * 3);
    }
}

__global__ __launch_bounds__(256) void ingest_kernel(const StxIngestItem* __restrict__ items, int n, StxIngestCoef K)
{
    const int tile = blockIdx.x;
    int lo = 0, hi = n - 1;  // the last frame whose first tile is <= tile (tile0 is ascending, items[0].tile0 = 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const StxIngestItem D = items[lo];
    const int t = tile - D.tile0, tyi = t / D.tiles_x, txi = t - tyi * D.tiles_x;
    const int xu = (txi * 64 + (int)(threadIdx.x & 63)) * STX_INGEST_LANE_PX;  // first pixel (COPY: first word) of the lane
    const int ru = tyi * STX_INGEST_ROWS + (int)(threadIdx.x >> 6);           // row unit
    const bool yuv = D.kind == STX_INGEST_K_NV12 || D.kind == STX_INGEST_K_I420;
    const int y = yuv ? ru * 2 : ru;
    if (y >= D.h) return;
    switch (D.kind) {  // uniform over the workgroup
    case STX_INGEST_K_COPY: copy_lane(D, xu, y); break;
    case STX_INGEST_K_PACK3:
        if (D.reverse) pack_lane<3, true>(D, xu, y); else pack_lane<3, false>(D, xu, y);
        break;
    case STX_INGEST_K_PACK4:
        if (D.reverse) pack_lane<4, true>(D, xu, y); else pack_lane<4, false>(D, xu, y);
        break;
    case STX_INGEST_K_NV12: yuv_lane<false>(D, K, xu, y); break;
    default: yuv_lane<true>(D, K, xu, y); break;
    }
}
}  // namespace

int stx_launch_ingest(stx_ctx* ctx, const StxIngestItem* d_items, int n, int total_tiles, const StxIngestCoef& coef, double algo_bytes)
{
    StxProfScope prof(ctx, "ingest", algo_bytes);
    hipLaunchKernelGGL(ingest_kernel, dim3(total_tiles), dim3(256), 0, ctx->stream, d_items, n, coef);
    return stx_check_launch("ingest");
}
