// stx_exposure_track.hip — exposure-gain tracking on a known rig for gfx950: the measurement that rides along with the steady state
// (host side: stx_exposure_track_host.cpp; contract: tests/numpy_exposure_track.py).
//
// The lattice of stride s holds the panorama pixels (l s, m s).  Three kernels:
//   exposure_track_grid_kernel   once per rig: the warped masks -> one byte V per lattice point inside an image's rectangle
//                                (1: the mask is 255 there) and c_ii, the number of such points.  The masks are not kept.
//   exposure_track_stats_kernel  every run: one 256-lane workgroup per tile of STX_TRACK_TILE x STX_TRACK_TILE lattice points of one
//                                pair of images.  A lane gathers the two 3-byte pixels of its samples where V_a & V_b, counts the sample
//                                if all six bytes lie in 1 .. 254 and sums its channels, else counts it as rejected: eight u32 partials
//                                per lane (bounded by the tile size: static_assert in stx_internal.h), a wave64 cross-lane sum, LDS
//                                across the four wavefronts, then one 64-bit integer atomicAdd per value and workgroup into the pair's
//                                eight accumulators.  Integer sums only: the same bits in any order.  No float atomics.
//   gain_maps_scale_kernel       out = map * factor in fp32 for all gain maps of a rig in one launch (f32x1 -> f32x1 or f32x3,
//                                f32x3 -> f32x3); the factors are kernel arguments: no upload, no wait.
#include "stx_device_math.h"
#include "stx_internal.h"

namespace {

constexpr int WAVES = STX_TRACK_WG / 64;

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the wavefront's sum
}

struct TrackGridK {
    const StxTrackGeo* geo;
    const StxTrackPix* masks;
    uint8_t* grid;
    unsigned long long* self;
    int stride;
};

__global__ __launch_bounds__(STX_TRACK_WG) void exposure_track_grid_kernel(TrackGridK K)
{
    const StxTrackGeo G = K.geo[blockIdx.y];
    const StxTrackPix M = K.masks[blockIdx.y];
    const long long total = (long long)G.nx * G.ny;
    const int ox = G.lx0 * K.stride - G.x, oy = G.ly0 * K.stride - G.y;  // the first lattice point inside the mask
    unsigned count = 0;
    // at most 2^31 / (gridDim.x * 256) + 1 iterations of one lane: far below 2^32 counts
    for (long long p = (long long)blockIdx.x * STX_TRACK_WG + threadIdx.x; p < total; p += (long long)gridDim.x * STX_TRACK_WG) {
        const int ly = (int)(p / G.nx), lx = (int)(p - (long long)ly * G.nx);
        const unsigned v = M.img[(long long)(oy + ly * K.stride) * M.istride + ox + lx * K.stride] == 255 ? 1u : 0u;
        K.grid[G.voff + p] = (uint8_t)v;
        count += v;
    }
    __shared__ unsigned part[WAVES];
    count = wave_sum(count);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < WAVES; w++) s += part[w];
        if (s) atomicAdd(&K.self[blockIdx.y], s);
    }
}

struct TrackStatsK {
    const StxTrackGeo* geo;
    const StxTrackPix* pix;
    const StxTrackTile* tiles;
    const uint8_t* grid;
    unsigned long long* acc;  // 8 per pair: c, B G R of a, B G R of b, rejected
    int stride;
};

__global__ __launch_bounds__(STX_TRACK_WG) void exposure_track_stats_kernel(TrackStatsK K)
{
    const StxTrackTile T = K.tiles[blockIdx.x];
    const StxTrackGeo Ga = K.geo[T.a], Gb = K.geo[T.b];
    const StxTrackPix Pa = K.pix[T.a], Pb = K.pix[T.b];
    unsigned v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int tx = threadIdx.x & (STX_TRACK_TILE - 1);
#pragma unroll
    for (int k = 0; k < STX_TRACK_TILE * STX_TRACK_TILE / STX_TRACK_WG; k++) {
        const int ty = (threadIdx.x + k * STX_TRACK_WG) / STX_TRACK_TILE;
        if (tx >= T.nx || ty >= T.ny) continue;
        const int lx = T.lx + tx, ly = T.ly + ty;
        const uint8_t va = K.grid[Ga.voff + (long long)(ly - Ga.ly0) * Ga.nx + (lx - Ga.lx0)];
        const uint8_t vb = K.grid[Gb.voff + (long long)(ly - Gb.ly0) * Gb.nx + (lx - Gb.lx0)];
        if (!(va & vb)) continue;
        const int X = lx * K.stride, Y = ly * K.stride;
        const uint8_t* pa = Pa.img + (long long)(Y - Ga.y) * Pa.istride + 3ll * (X - Ga.x);
        const uint8_t* pb = Pb.img + (long long)(Y - Gb.y) * Pb.istride + 3ll * (X - Gb.x);
        const unsigned a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
        // 1 .. 254: (x - 1) as unsigned is below 254
        const bool ok = (a0 - 1u) < 254u && (a1 - 1u) < 254u && (a2 - 1u) < 254u && (b0 - 1u) < 254u && (b1 - 1u) < 254u && (b2 - 1u) < 254u;
        if (ok) {
            v[0] += 1u; v[1] += a0; v[2] += a1; v[3] += a2; v[4] += b0; v[5] += b1; v[6] += b2;
        } else {
            v[7] += 1u;
        }
    }
    __shared__ unsigned part[WAVES][8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const unsigned s = wave_sum(v[q]);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        unsigned long long s = 0;
        for (int w = 0; w < WAVES; w++) s += part[w][threadIdx.x];
        if (s) atomicAdd(&K.acc[8ll * T.pair + threadIdx.x], s);
    }
}

struct ScaleMapsK { StxScaleMap m[STX_SCALE_MAPS_PER_LAUNCH]; };

__global__ __launch_bounds__(256) void gain_maps_scale_kernel(ScaleMapsK K)
{
    const StxScaleMap& M = K.m[blockIdx.y];
    const int total = M.w * M.h * M.dc;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int q = i / M.dc, ch = i - q * M.dc;
        const int y = q / M.w, x = q - y * M.w;
        const float s = M.src[(long long)y * M.sstride + (long long)x * M.sc + (M.sc == 3 ? ch : 0)];
        M.dst[(long long)y * M.dstride + (long long)x * M.dc + ch] = stxd::fmul(s, M.f[ch]);
    }
}

}  // namespace

int stx_launch_exposure_track_grid(stx_ctx* ctx, int n, const StxTrackGeo* d_geo, const StxTrackPix* d_masks, int stride, long long max_points,
                                   uint8_t* d_grid, unsigned long long* d_self)
{
    if (n <= 0 || max_points <= 0) return STX_OK;
    TrackGridK K;
    K.geo = d_geo; K.masks = d_masks; K.grid = d_grid; K.self = d_self; K.stride = stride;
    const int gx = (int)std::min<long long>(1024, (max_points + STX_TRACK_WG - 1) / STX_TRACK_WG);
    StxProfScope prof(ctx, "exposure_track_grid", 0.0);
    hipLaunchKernelGGL(exposure_track_grid_kernel, dim3(gx, n), dim3(STX_TRACK_WG), 0, ctx->stream, K);
    return stx_check_launch("exposure_track_grid");
}

int stx_launch_exposure_track_stats(stx_ctx* ctx, const StxTrackGeo* d_geo, const StxTrackPix* d_pix, const StxTrackTile* d_tiles, int ntiles,
                                    int stride, const uint8_t* d_grid, unsigned long long* d_acc, double algo_bytes)
{
    if (ntiles <= 0) return STX_OK;
    TrackStatsK K;
    K.geo = d_geo; K.pix = d_pix; K.tiles = d_tiles; K.grid = d_grid; K.acc = d_acc; K.stride = stride;
    StxProfScope prof(ctx, "exposure_track_stats", algo_bytes);
    hipLaunchKernelGGL(exposure_track_stats_kernel, dim3(ntiles), dim3(STX_TRACK_WG), 0, ctx->stream, K);
    return stx_check_launch("exposure_track_stats");
}

int stx_launch_gain_maps_scale(stx_ctx* ctx, const StxScaleMap* maps, int n)
{
    for (int i0 = 0; i0 < n; i0 += STX_SCALE_MAPS_PER_LAUNCH) {
        const int k = std::min(STX_SCALE_MAPS_PER_LAUNCH, n - i0);
        ScaleMapsK K = {};
        int most = 1;
        for (int i = 0; i < k; i++) {
            K.m[i] = maps[i0 + i];
            most = std::max(most, maps[i0 + i].w * maps[i0 + i].h * maps[i0 + i].dc);
        }
        StxProfScope prof(ctx, "gain_maps_scale", 0.0);
        hipLaunchKernelGGL(gain_maps_scale_kernel, dim3(std::min(64, (most + 255) / 256), k), dim3(256), 0, ctx->stream, K);
        STX_TRY(stx_check_launch("gain_maps_scale"));
    }
    return STX_OK;
}
