// stx_rectify.hip — lens rectification: n distorted frames of unequal sizes -> pinhole frames (and validity masks), each through its
// camera's lens grid, in ONE launch (tests/numpy_rectify.py is the contract, byte for byte).  Integer only.
//
// A wavefront owns one cell of the grid — 16 x 16 destination pixels, whose four nodes are the same for every lane and come by scalar
// loads — and a lane four pixels of one row of it, so that it stores whole words (12 bytes of BGR, 4 of gray, 4 of the mask).  A
// workgroup is four cells side by side (64 x 16 pixels: 5 x 2 nodes), the grid the flat list of the images' tiles.  No LDS: a cell's
// taps fall into a source patch of about its own size, which the vector L1 serves.
//
// Every tap is read at its CLAMPED indices, which always lie inside the source, whatever the nodes say.  STX_RECTIFY_REPLICATE is then
// the contract as it stands; for STX_RECTIFY_CONSTANT a tap whose index was clamped is set to 0.  The two taps of a row are 2 C
// contiguous bytes at any byte offset: they are read as the aligned words around them and shifted into place (v_alignbyte), which costs
// less than byte-exact unaligned loads (the warp kernel's measurement, stx_warp.hip).  The words reach up to 3 bytes in front of the
// left tap and up to 9 behind it (the left tap may be the row's last pixel): inside the 64 bytes that lie in front of and behind every
// image the library allocates (stx_buf_new), and inside the parent for a crop view.  Offsets are 32-bit and rows are found by a 24-bit
// multiply: the host checks that the source spans less than 2^31 bytes with a pitch below 2^24.
#include "stx_internal.h"
#include "stx_lane_io.h"

namespace {
#define STX_GAS __attribute__((address_space(1)))
#define STX_CAS __attribute__((address_space(4)))
typedef unsigned short v2h __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));  // a node as the scalar loads deliver it

__device__ __forceinline__ v2h as_v2h(uint32_t v) { return __builtin_bit_cast(v2h, v); }

// the taps (x, x + 1) of one row, C bytes each at byte offset a from the 4-aligned base: each in the low bits of its word
template <int C>
__device__ __forceinline__ void load_taps(const STX_GAS uint8_t* base, uint32_t a, uint32_t& t0, uint32_t& t1)
{
    const STX_GAS uint32_t* q = reinterpret_cast<const STX_GAS uint32_t*>(base + (a & ~3u));
    if constexpr (C == 3) {
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
        const uint32_t l = __builtin_amdgcn_alignbyte(d1, d0, a), h = __builtin_amdgcn_alignbyte(d2, d1, a);  // bytes 0 .. 3 and 4 .. 7 from a
        t0 = l & 0xffffffu;
        t1 = __builtin_amdgcn_alignbyte(h, l, 3u) & 0xffffffu;
    } else {
        const uint32_t d0 = q[0], d1 = q[1];
        const uint32_t l = __builtin_amdgcn_alignbyte(d1, d0, a);
        t0 = l & 255u;
        t1 = (l >> 8) & 255u;
    }
}

template <int C>
__device__ __forceinline__ void rectify_lane(const StxRectifyItem& D, int border, v2i n00, v2i n10, v2i n01, v2i n11, int x0, int y, int ax0,
                                             int ay)
{
    // S = (16 - ay) ((16 - ax) N00 + ax N10) + ay ((16 - ax) N01 + ax N11) = 16 L + ax (R - L) with the cell's edges at this row
    // L = 16 N00 + ay (N01 - N00), R likewise: the same integers (|N| <= 2^21: |N01 - N00| < 2^23 for the 24-bit multiply, |16 L| <= 2^29,
    // |ax (R - L)| < 2^30, and the sum is the bounded S)
    const int lx = (n00.x << 4) + __mul24(ay, n01.x - n00.x), rx = (n10.x << 4) + __mul24(ay, n11.x - n10.x);
    const int ly = (n00.y << 4) + __mul24(ay, n01.y - n00.y), ry = (n10.y << 4) + __mul24(ay, n11.y - n10.y);
    const int dx = rx - lx, dy = ry - ly;
    int sx = (lx << 4) + ax0 * dx + 256, sy = (ly << 4) + ax0 * dy + 256;
    const uintptr_t src = (uintptr_t)D.src;
    const STX_GAS uint8_t* base = (const STX_GAS uint8_t*)(src & ~(uintptr_t)3);
    const uint32_t bias = (uint32_t)(src & 3u), stride = (uint32_t)D.sstride;
    uint32_t o[C], m[1] = {0u};
#pragma unroll
    for (int k = 0; k < C; k++) o[k] = 0u;
#pragma unroll
    for (int i = 0; i < STX_RECTIFY_LANE_PX; i++) {  // a pixel past the image's edge is computed (its reads are clamped) and not stored
        const int qx = sx >> 9, qy = sy >> 9;
        sx += dx; sy += dy;
        const int ix = qx >> 5, iy = qy >> 5;
        const uint32_t fx = (uint32_t)qx & 31u, fy = (uint32_t)qy & 31u;
        const int cx0 = min(max(ix, 0), D.sw - 1), cx1 = min(max(ix + 1, 0), D.sw - 1);
        const int cy0 = min(max(iy, 0), D.sh - 1), cy1 = min(max(iy + 1, 0), D.sh - 1);
        const bool vx0 = cx0 == ix, vx1 = cx1 == ix + 1, vy0 = cy0 == iy, vy1 = cy1 == iy + 1;  // the tap's index lies inside
        const uint32_t a0 = bias + __umul24((uint32_t)cy0, stride) + (uint32_t)cx0 * C, a1 = a0 + (cy1 != cy0 ? stride : 0u);
        uint32_t t00, t10, t01, t11;  // t<x><y>
        load_taps<C>(base, a0, t00, t10);
        load_taps<C>(base, a1, t01, t11);
        if (cx1 == cx0) { t10 = t00; t11 = t01; }  // both clamped to one column
        if (border == STX_RECTIFY_CONSTANT) {
            t00 = vx0 && vy0 ? t00 : 0u; t10 = vx1 && vy0 ? t10 : 0u;
            t01 = vx0 && vy1 ? t01 : 0u; t11 = vx1 && vy1 ? t11 : 0u;
        }
        // (w00 p00 + w10 p10 + w01 p01 + w11 p11 + 512) >> 10 as ((32 - fy) p.0 + fy p.1) . (32 - fx, fx): the same products, packed
        const uint32_t wy1 = fy * 0x10001u, wy0 = 0x200020u - wy1, wx = (32u - fx) | (fx << 16);
#pragma unroll
        for (int k = 0; k < C; k++) {
            const uint32_t sel = k == 0 ? 0x0c040c00u : (k == 1 ? 0x0c050c01u : 0x0c060c02u);  // byte k of the left and of the right tap
            const v2h top = as_v2h(__builtin_amdgcn_perm(t10, t00, sel)), bottom = as_v2h(__builtin_amdgcn_perm(t11, t01, sel));
            const v2h v = top * as_v2h(wy0) + bottom * as_v2h(wy1);  // <= 255 * 32
            const uint32_t out = __builtin_amdgcn_udot2(v, as_v2h(wx), 512u, false) >> 10;
            const int j = i * C + k;
            o[j >> 2] |= out << ((j & 3) * 8);
        }
        m[0] |= (vx0 && vx1 && vy0 && vy1 ? 255u : 0u) << (i * 8);
    }
    const int npx = min(STX_RECTIFY_LANE_PX, D.dw - x0);
    store_words<C>(D.dst + (long long)y * D.dstride + (long long)x0 * C, o, npx * C);
    if (D.mask) store_words<1>(D.mask + (long long)y * D.mstride + x0, m, npx);
}

__global__ __launch_bounds__(256) void rectify_kernel(const StxRectifyItem* __restrict__ items, int n, int border)
{
    const int tile = blockIdx.x;
    int lo = 0, hi = n - 1;  // the last image whose first tile is <= tile (tile0 is ascending, items[0].tile0 = 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const StxRectifyItem D = items[lo];
    const int t = tile - D.tile0, tyi = t / D.tiles_x, txi = t - tyi * D.tiles_x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int cell = txi * (STX_RECTIFY_TW / STX_LENS_CELL) + wave;  // cell column; the cell row is tyi
    if (cell * STX_LENS_CELL >= D.dw) return;                         // the whole wavefront
    // cell <= (dw - 1) / 16 and tyi <= (dh - 1) / 16: the nodes (cell + 1, tyi + 1) exist (nx = (dw + 15) / 16 + 1, ny likewise)
    const STX_CAS v2i* nd = (const STX_CAS v2i*)D.nodes + ((long long)tyi * D.nx + cell);  // wave-uniform reads: scalar loads
    const v2i n00 = nd[0], n10 = nd[1], n01 = nd[D.nx], n11 = nd[D.nx + 1];
    const int ay = lane >> 2, ax0 = (lane & 3) * STX_RECTIFY_LANE_PX;
    const int x0 = cell * STX_LENS_CELL + ax0, y = tyi * STX_RECTIFY_TH + ay;
    if (x0 >= D.dw || y >= D.dh) return;
    if (D.c == 3) rectify_lane<3>(D, border, n00, n10, n01, n11, x0, y, ax0, ay);  // uniform over the workgroup
    else rectify_lane<1>(D, border, n00, n10, n01, n11, x0, y, ax0, ay);
}
}  // namespace

int stx_launch_rectify(stx_ctx* ctx, const StxRectifyItem* d_items, int n, int total_tiles, int border, double algo_bytes)
{
    StxProfScope prof(ctx, "rectify", algo_bytes);
    hipLaunchKernelGGL(rectify_kernel, dim3(total_tiles), dim3(256), 0, ctx->stream, d_items, n, border);
    return stx_check_launch("rectify");
}
