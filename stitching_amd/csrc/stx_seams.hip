// stx_seams.hip — VoronoiSeamFinder::findInPair for gfx950: the pairs of one dependency level at a time (stx_seams_host.cpp builds
// the levels), two launches per level.
//
// A pair's window is its overlap roi with a gap of STX_SEAM_GAP pixels on every side; mask pixels outside an image read as 0.
//   rows:    one wavefront per window row (4 per workgroup, blockIdx.y = the pair), 256 pixels (4 per lane) per step.  unique1 =
//            m1 != 0 && m2 == 0, unique2 the other way round.  A right-to-left sweep (wave suffix-min scan of the first source column,
//            a carry between steps) writes r(x) = first source >= x minus x; the left-to-right sweep (prefix-max scan of the last
//            source column) makes l(x) and overwrites the value with min(l, r, 8192).  Each lane reads back only what it wrote
//            itself.  Only the roi's columns are stored: u16 distances of both masks in the level's scratch arena.
//   columns: one lane per roi column (lanes along x: coalesced u16 rows), a(y) = min(g(y), a(y - 1) + 1) down the whole window in
//            place, then f(y) = min(a(y), f(y + 1) + 1) up to the roi's first row; on roi rows dist1 < dist2 zeroes mask j, otherwise
//            mask i.  Loads go out eight rows at a time.
// Pairs of one level read and write disjoint pixels (the schedule's rule), so the launches of a level need no ordering inside.
#include "stx_internal.h"

namespace {

constexpr int SEAM_WG = 256;
constexpr int SEAM_PX = 4;                 // pixels per lane and step of the row sweeps
constexpr int SEAM_STEP = 64 * SEAM_PX;    // pixels per wavefront step
constexpr int SEAM_BIG = 1 << 28;
constexpr int SEAM_SAT = 8192;

__device__ inline uint8_t seam_px(const uint8_t* m, long long stride, int w, int h, int x, int y)
{
    return (x >= 0 && y >= 0 && x < w && y < h) ? m[(long long)y * stride + x] : (uint8_t)0;
}

struct SeamRowsK { const StxSeamPair* pairs; uint16_t* arena; };

__global__ __launch_bounds__(SEAM_WG) void seam_rows_kernel(SeamRowsK K)
{
    const StxSeamPair P = K.pairs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (SEAM_WG / 64) + (threadIdx.x >> 6);
    if (r >= P.wh) return;  // wave-uniform; no barriers below
    const int iy = P.oy1 + r, jy = P.oy2 + r;
    const int steps = (P.ww + SEAM_STEP - 1) / SEAM_STEP;
    uint16_t* d1 = K.arena + P.off + (long long)r * P.rw;
    uint16_t* d2 = d1 + (long long)P.wh * P.rw;
    // the unique bits of this lane's 4 pixels of step s: bit k of u1 / u2
    auto bits = [&](int s, unsigned& u1, unsigned& u2) {
        u1 = u2 = 0;
        const int x0 = s * SEAM_STEP + lane * SEAM_PX;
#pragma unroll
        for (int k = 0; k < SEAM_PX; k++) {
            const int x = x0 + k;
            if (x >= P.ww) break;
            const bool a = seam_px(P.m1, P.s1, P.w1, P.h1, P.ox1 + x, iy) != 0;
            const bool b = seam_px(P.m2, P.s2, P.w2, P.h2, P.ox2 + x, jy) != 0;
            u1 |= (unsigned)(a && !b) << k;
            u2 |= (unsigned)(b && !a) << k;
        }
    };
    // right to left: r(x) = first source column >= x, minus x
    int n1 = SEAM_BIG, n2 = SEAM_BIG;  // carry: first source column right of the step
    for (int s = steps - 1; s >= 0; s--) {
        unsigned u1, u2;
        bits(s, u1, u2);
        const int x0 = s * SEAM_STEP + lane * SEAM_PX;
        int f1 = u1 ? x0 + __builtin_ctz(u1) : SEAM_BIG, f2 = u2 ? x0 + __builtin_ctz(u2) : SEAM_BIG;
        for (int o = 1; o < 64; o <<= 1) {  // inclusive suffix minimum over lanes
            const int t1 = __shfl_down(f1, o), t2 = __shfl_down(f2, o);
            if (lane + o < 64) { f1 = min(f1, t1); f2 = min(f2, t2); }
        }
        int e1 = __shfl_down(f1, 1), e2 = __shfl_down(f2, 1);
        if (lane == 63) { e1 = SEAM_BIG; e2 = SEAM_BIG; }
        e1 = min(e1, n1); e2 = min(e2, n2);
        n1 = min(n1, __shfl(f1, 0)); n2 = min(n2, __shfl(f2, 0));
#pragma unroll
        for (int k = SEAM_PX - 1; k >= 0; k--) {
            const int x = x0 + k;
            if ((u1 >> k) & 1) e1 = x;
            if ((u2 >> k) & 1) e2 = x;
            const int c = x - STX_SEAM_GAP;
            if (x < P.ww && c >= 0 && c < P.rw) {
                d1[c] = (uint16_t)min(e1 - x, SEAM_SAT);
                d2[c] = (uint16_t)min(e2 - x, SEAM_SAT);
            }
        }
    }
    // left to right: l(x) = x minus last source column <= x; min with r
    int l1 = -SEAM_BIG, l2 = -SEAM_BIG;
    for (int s = 0; s < steps; s++) {
        unsigned u1, u2;
        bits(s, u1, u2);
        const int x0 = s * SEAM_STEP + lane * SEAM_PX;
        int f1 = u1 ? x0 + 31 - __builtin_clz(u1) : -SEAM_BIG, f2 = u2 ? x0 + 31 - __builtin_clz(u2) : -SEAM_BIG;
        for (int o = 1; o < 64; o <<= 1) {  // inclusive prefix maximum over lanes
            const int t1 = __shfl_up(f1, o), t2 = __shfl_up(f2, o);
            if (lane >= o) { f1 = max(f1, t1); f2 = max(f2, t2); }
        }
        int e1 = __shfl_up(f1, 1), e2 = __shfl_up(f2, 1);
        if (lane == 0) { e1 = -SEAM_BIG; e2 = -SEAM_BIG; }
        e1 = max(e1, l1); e2 = max(e2, l2);
        l1 = max(l1, __shfl(f1, 63)); l2 = max(l2, __shfl(f2, 63));
#pragma unroll
        for (int k = 0; k < SEAM_PX; k++) {
            const int x = x0 + k;
            if ((u1 >> k) & 1) e1 = x;
            if ((u2 >> k) & 1) e2 = x;
            const int c = x - STX_SEAM_GAP;
            if (x < P.ww && c >= 0 && c < P.rw) {
                d1[c] = (uint16_t)min((int)d1[c], min(x - e1, SEAM_SAT));
                d2[c] = (uint16_t)min((int)d2[c], min(x - e2, SEAM_SAT));
            }
        }
    }
}

struct SeamColsK { const StxSeamPair* pairs; uint16_t* arena; };

constexpr int SEAM_BATCH = 8;

__global__ __launch_bounds__(SEAM_WG) void seam_cols_kernel(SeamColsK K)
{
    const StxSeamPair P = K.pairs[blockIdx.y];
    const int c = blockIdx.x * SEAM_WG + threadIdx.x;
    if (c >= P.rw) return;
    uint16_t* p1 = K.arena + P.off + c;
    uint16_t* p2 = p1 + (long long)P.wh * P.rw;
    const long long rw = P.rw;
    // down: a(y) = min(g(y), a(y - 1) + 1), in place
    int a1 = SEAM_BIG, a2 = SEAM_BIG;
    int y = 0;
    for (; y + SEAM_BATCH <= P.wh; y += SEAM_BATCH) {
        int v1[SEAM_BATCH], v2[SEAM_BATCH];
#pragma unroll
        for (int k = 0; k < SEAM_BATCH; k++) { v1[k] = p1[(y + k) * rw]; v2[k] = p2[(y + k) * rw]; }
#pragma unroll
        for (int k = 0; k < SEAM_BATCH; k++) {
            a1 = min(v1[k], a1 + 1); a2 = min(v2[k], a2 + 1);
            p1[(y + k) * rw] = (uint16_t)a1; p2[(y + k) * rw] = (uint16_t)a2;
        }
    }
    for (; y < P.wh; y++) {
        a1 = min((int)p1[y * rw], a1 + 1); a2 = min((int)p2[y * rw], a2 + 1);
        p1[y * rw] = (uint16_t)a1; p2[y * rw] = (uint16_t)a2;
    }
    // up, to the roi's first row: f(y) = min(a(y), f(y + 1) + 1); roi rows decide
    const int top = STX_SEAM_GAP, bot = STX_SEAM_GAP + P.rh;  // roi rows of the window: [top, bot)
    const int xi = P.ox1 + STX_SEAM_GAP + c, xj = P.ox2 + STX_SEAM_GAP + c;
    auto decide = [&](int yy, int f1, int f2) {
        if (yy < top || yy >= bot) return;
        if (f1 < f2) P.m2[(long long)(P.oy2 + yy) * P.s2 + xj] = 0;
        else P.m1[(long long)(P.oy1 + yy) * P.s1 + xi] = 0;
    };
    int f1 = SEAM_BIG, f2 = SEAM_BIG;
    y = P.wh - 1;
    for (; y - SEAM_BATCH + 1 >= top; y -= SEAM_BATCH) {
        int v1[SEAM_BATCH], v2[SEAM_BATCH];
#pragma unroll
        for (int k = 0; k < SEAM_BATCH; k++) { v1[k] = p1[(y - k) * rw]; v2[k] = p2[(y - k) * rw]; }
#pragma unroll
        for (int k = 0; k < SEAM_BATCH; k++) {
            f1 = min(v1[k], f1 + 1); f2 = min(v2[k], f2 + 1);
            decide(y - k, f1, f2);
        }
    }
    for (; y >= top; y--) {
        f1 = min((int)p1[y * rw], f1 + 1); f2 = min((int)p2[y * rw], f2 + 1);
        decide(y, f1, f2);
    }
}

}  // namespace

int stx_launch_seam_level(stx_ctx* ctx, const StxSeamPair* d_pairs, int np, int max_rows, int max_cols, uint16_t* d_arena, double algo_bytes)
{
    if (np <= 0) return STX_OK;
    {
        SeamRowsK K{d_pairs, d_arena};
        StxProfScope prof(ctx, "seam_rows", algo_bytes);
        hipLaunchKernelGGL(seam_rows_kernel, dim3((max_rows + SEAM_WG / 64 - 1) / (SEAM_WG / 64), np), dim3(SEAM_WG), 0, ctx->stream, K);
        STX_TRY(stx_check_launch("seam_rows"));
    }
    SeamColsK K{d_pairs, d_arena};
    StxProfScope prof(ctx, "seam_cols", 0.0);
    hipLaunchKernelGGL(seam_cols_kernel, dim3((max_cols + SEAM_WG - 1) / SEAM_WG, np), dim3(SEAM_WG), 0, ctx->stream, K);
    return stx_check_launch("seam_cols");
}
