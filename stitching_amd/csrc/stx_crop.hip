// stx_crop.hip — Cropper.estimate_largest_interior_rectangle for gfx950 (stitching/cropper.py:91-106): the contour check and the
// largest interior rectangle of a u8x1 panorama mask, on the device.  tests/numpy_lir.py is the contract; nonzero means true.
//
// Contour check (findContours' hierarchy is one entry with no parent, child or sibling): union-find over the zero-framed grid.
//   Labels are 1 + y * w + x; label 0 is the frame ("outside").  A label never exceeds its index and only ever decreases.
//   runs:    one wavefront per row; every pixel's label starts as the first pixel of its horizontal run of its own class (a wave
//            prefix-max scan of the run starts, a carry between steps of 64 pixels), so horizontal neighbours need no union.
//   merge:   one lane per pixel.  A foreground run is joined to every foreground run of the row above that it touches through the
//            8-neighbourhood, a background run to every background run above that it shares a column with (4-neighbourhood), and a
//            background run on the image border to the frame.  Each such pair is joined once: at the first column they share, or
//            diagonally at the run's ends.  The union is Playne & Hawick's (2018) lock-free one: an integer atomicMin links the larger
//            root under the smaller one, a failed link retries from the value it found.
//   count:   a pixel whose label is its own index is a root: one per foreground component, one per hole (every background component
//            that touches the border is joined to the frame, whose root is 0).  Exact integer counts, one atomicAdd per workgroup.
// Largest interior rectangle (max area; ties: smallest y, then smallest x, then largest w):
//   columns: one lane per column, bottom-up: v(y, x) = mask(y, x) ? v(y + 1, x) + 1 : 0 (the run of true cells downward).
//   rows:    one workgroup per row (grid-stride), the row v(y, .) as a histogram.  Nearest strictly smaller bar on the left and on the
//            right of every bar, lane chunk by lane chunk: inside the chunk with the amortised pointer walk, then the bars whose walk
//            left the chunk continue through the other chunks' pointers.  Every pointer ever stored p(x) keeps "the bars strictly
//            between p(x) and x are >= v(x)", so a walk may read another lane's pointer before or after it is final and still stops
//            exactly at the nearest smaller bar.  Bar x then gives the rectangle of height v(x) over (left, right): every
//            maximum-area rectangle with top row y is one of these, so the tie rule's winner is too.  Block reduction to the row's
//            best (area, x, w, h).  The row's heights and pointers live in LDS when they fit, in a global scratch slice otherwise.
//   reduce:  one workgroup over the rows' bests with the full tie rule.
// No floating point anywhere; every result is independent of scheduling (the union-find's roots may differ between runs, their count
// does not; the pointer walks end at the same bars).
#include "stx_internal.h"

namespace {

constexpr int CROP_WG = 256;
constexpr int CROP_ROWS_GRID = 2048;       // workgroups of the row stage (grid-stride over the rows)
constexpr int CROP_LDS_MAX_W = 4864;       // rows up to this width keep heights + two pointer arrays in LDS (57 KiB + 5 KiB static)
constexpr int CROP_BATCH = 8;

struct CropMask { const uint8_t* p; long long stride; int w, h; };

__device__ inline bool crop_on(const CropMask& M, int x, int y) { return M.p[(long long)y * M.stride + x] != 0; }

__device__ inline int uf_load(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int uf_find(const int* lab, int x)
{
    int p = uf_load(lab + x);
    while (p != x) {
        x = p;
        p = uf_load(lab + x);
    }
    return x;
}

__device__ inline void uf_union(int* lab, int a, int b)
{
    bool done = false;
    while (!done) {
        a = uf_find(lab, a);
        b = uf_find(lab, b);
        if (a < b) {
            const int old = atomicMin(lab + b, a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(lab + a, b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    }
}

// labels: every pixel -> the first pixel of its run; label 0 (the frame) -> 0.  One wavefront per row.
__global__ __launch_bounds__(CROP_WG) void crop_runs_kernel(CropMask M, int* lab)
{
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * (CROP_WG / 64) + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) lab[0] = 0;
    if (y >= M.h) return;  // wave-uniform
    const long long row = 1 + (long long)y * M.w;
    int carry = 0;
    for (int x0 = 0; x0 < M.w; x0 += 64) {
        const int x = x0 + lane;
        int s = -1;
        if (x < M.w) s = (x == 0 || crop_on(M, x, y) != crop_on(M, x - 1, y)) ? x : -1;
        for (int o = 1; o < 64; o <<= 1) {  // inclusive prefix maximum over lanes
            const int t = __shfl_up(s, o);
            if (lane >= o) s = max(s, t);
        }
        s = max(s, carry);
        carry = __shfl(s, 63);
        if (x < M.w) lab[row + x] = (int)(row + s);
    }
}

// the unions between this row's runs and the row above, and of border background runs with the frame.  One lane per pixel.
__global__ __launch_bounds__(CROP_WG) void crop_merge_kernel(CropMask M, int* lab)
{
    const int x = blockIdx.x * CROP_WG + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= M.w) return;
    const int W = M.w;
    const int p = 1 + y * W + x;
    const bool c = crop_on(M, x, y);
    const bool first = x == 0 || crop_on(M, x - 1, y) != c;
    const bool last = x == W - 1 || crop_on(M, x + 1, y) != c;
    if (c) {
        if (y == 0) return;
        const int q = p - W;
        const bool up = crop_on(M, x, y - 1);
        const bool up_first = x == 0 || !crop_on(M, x - 1, y - 1);  // a foreground run above starts here
        if (up && (first || up_first)) uf_union(lab, p, q);
        if (!up && first && x > 0 && crop_on(M, x - 1, y - 1)) uf_union(lab, p, q - 1);
        if (!up && last && x < W - 1 && crop_on(M, x + 1, y - 1)) uf_union(lab, p, q + 1);
    } else {
        if (first && (y == 0 || y == M.h - 1 || x == 0)) uf_union(lab, p, 0);
        if (last && x == W - 1) uf_union(lab, p, 0);
        if (y > 0) {
            const bool up = crop_on(M, x, y - 1);
            const bool up_first = x == 0 || crop_on(M, x - 1, y - 1);  // a background run above starts here
            if (!up && (first || up_first)) uf_union(lab, p, p - W);
        }
    }
}

// roots: counts[0] += foreground components, counts[1] += holes
__global__ __launch_bounds__(CROP_WG) void crop_count_kernel(CropMask M, const int* lab, int* counts)
{
    const int x = blockIdx.x * CROP_WG + threadIdx.x;
    const int y = blockIdx.y;
    bool fg_root = false, bg_root = false;
    if (x < M.w) {
        const int p = 1 + y * M.w + x;
        if (lab[p] == p) {
            fg_root = crop_on(M, x, y);
            bg_root = !fg_root;
        }
    }
    const int nf = __syncthreads_count(fg_root);
    const int nb = __syncthreads_count(bg_root);
    if (threadIdx.x == 0) {
        if (nf) atomicAdd(counts, nf);
        if (nb) atomicAdd(counts + 1, nb);
    }
}

// v(y, x): the run of true cells from (x, y) downward.  One lane per column.
__global__ __launch_bounds__(CROP_WG) void crop_cols_kernel(CropMask M, int* v)
{
    const int x = blockIdx.x * CROP_WG + threadIdx.x;
    if (x >= M.w) return;
    const long long W = M.w;
    int run = 0;
    int y = M.h - 1;
    for (; y - CROP_BATCH + 1 >= 0; y -= CROP_BATCH) {
        uint8_t m[CROP_BATCH];
#pragma unroll
        for (int k = 0; k < CROP_BATCH; k++) m[k] = M.p[(long long)(y - k) * M.stride + x];
#pragma unroll
        for (int k = 0; k < CROP_BATCH; k++) {
            run = m[k] ? run + 1 : 0;
            v[(y - k) * W + x] = run;
        }
    }
    for (; y >= 0; y--) {
        run = M.p[(long long)y * M.stride + x] ? run + 1 : 0;
        v[y * W + x] = run;
    }
}

struct CropBest { long long area; int x, y, w, h; };

// a better than b by the tie rule (both of one row: y is equal)
__device__ inline bool crop_better(long long aa, int ay, int ax, int aw, long long ba, int by, int bx, int bw)
{
    if (aa != ba) return aa > ba;
    if (ay != by) return ay < by;
    if (ax != bx) return ax < bx;
    return aw > bw;
}

__device__ inline int ptr_load(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void ptr_store(int* a, int v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

struct CropRowsK { const int* v; int W, H; int* scratch; CropBest* best; };

__global__ __launch_bounds__(CROP_WG) void crop_rows_kernel(CropRowsK K)
{
    extern __shared__ int crop_lds[];
    __shared__ long long r_area[CROP_WG];
    __shared__ int r_x[CROP_WG], r_w[CROP_WG], r_h[CROP_WG];
    const int W = K.W, t = threadIdx.x;
    const bool in_lds = W <= CROP_LDS_MAX_W;
    int* lf = in_lds ? crop_lds + W : K.scratch + (long long)blockIdx.x * 2 * W;
    int* rt = lf + W;
    const int c = (W + CROP_WG - 1) / CROP_WG;
    const int s = min(t * c, W), e = min(s + c, W);  // this lane's chunk [s, e)
    for (int y = blockIdx.x; y < K.H; y += gridDim.x) {
        const int* vrow = K.v + (long long)y * W;
        const int* hv = vrow;
        if (in_lds) {
            for (int x = t; x < W; x += CROP_WG) crop_lds[x] = vrow[x];
            hv = crop_lds;
        }
        __syncthreads();
        // inside the chunk: nearest smaller on the left (a walk that leaves the chunk stops at s - 1) and on the right (stops at e)
        for (int x = s; x < e; x++) {
            const int h = hv[x];
            int j = x - 1;
            while (j >= s && hv[j] >= h) j = lf[j];
            ptr_store(lf + x, j);
        }
        for (int x = e - 1; x >= s; x--) {
            const int h = hv[x];
            int j = x + 1;
            while (j < e && hv[j] >= h) j = rt[j];
            ptr_store(rt + x, j);
        }
        __syncthreads();
        // the walks that left the chunk, through the other chunks: their bars are monotone (every bar before an open left bar in the
        // chunk is >= it), so each walk goes on from where the previous one ended
        {
            int j = s - 1;
            for (int x = s; x < e; x++) {
                if (ptr_load(lf + x) != s - 1) continue;
                const int h = hv[x];
                while (j >= 0 && hv[j] >= h) j = ptr_load(lf + j);
                ptr_store(lf + x, j);
            }
            j = e;
            for (int x = e - 1; x >= s; x--) {
                if (ptr_load(rt + x) != e) continue;
                const int h = hv[x];
                while (j < W && hv[j] >= h) j = ptr_load(rt + j);
                ptr_store(rt + x, j);
            }
        }
        __syncthreads();
        long long ba = 0;
        int bx = 0, bw = 0, bh = 0;
        for (int x = s; x < e; x++) {
            const int h = hv[x];
            if (h == 0) continue;
            const int x0 = lf[x] + 1, w = rt[x] - x0;
            const long long a = (long long)h * w;
            if (crop_better(a, 0, x0, w, ba, 0, bx, bw)) { ba = a; bx = x0; bw = w; bh = h; }
        }
        r_area[t] = ba; r_x[t] = bx; r_w[t] = bw; r_h[t] = bh;
        __syncthreads();
        for (int o = CROP_WG / 2; o > 0; o >>= 1) {
            if (t < o && crop_better(r_area[t + o], 0, r_x[t + o], r_w[t + o], r_area[t], 0, r_x[t], r_w[t])) {
                r_area[t] = r_area[t + o]; r_x[t] = r_x[t + o]; r_w[t] = r_w[t + o]; r_h[t] = r_h[t + o];
            }
            __syncthreads();
        }
        if (t == 0) K.best[y] = CropBest{r_area[0], r_x[0], y, r_w[0], r_h[0]};
        __syncthreads();  // LDS and the pointer slice are reused by the next row
    }
}

// the rows' bests -> res[2..5] = x, y, w, h (all 0 when the mask holds no true cell)
__global__ __launch_bounds__(CROP_WG) void crop_reduce_kernel(const CropBest* best, int H, int* res)
{
    __shared__ CropBest r[CROP_WG];
    const int t = threadIdx.x;
    CropBest b{0, 0, 0, 0, 0};
    for (int y = t; y < H; y += CROP_WG) {
        const CropBest q = best[y];
        if (crop_better(q.area, q.y, q.x, q.w, b.area, b.y, b.x, b.w)) b = q;
    }
    r[t] = b;
    __syncthreads();
    for (int o = CROP_WG / 2; o > 0; o >>= 1) {
        if (t < o && crop_better(r[t + o].area, r[t + o].y, r[t + o].x, r[t + o].w, r[t].area, r[t].y, r[t].x, r[t].w)) r[t] = r[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const bool any = r[0].area > 0;
        res[2] = any ? r[0].x : 0;
        res[3] = any ? r[0].y : 0;
        res[4] = any ? r[0].w : 0;
        res[5] = any ? r[0].h : 0;
    }
}

}  // namespace

STX_EXPORT int stx_crop_lir(stx_ctx* ctx, const stx_buf* mask, int out_xywh[4], int out_contours[2], double out_info[1])
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (!mask || !out_xywh || !out_contours) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (mask->elem != STX_U8 || mask->c != 1) return stx_fail(STX_ERR_INVALID, "the largest interior rectangle needs a u8x1 mask");
    if (mask->ctx != ctx) return stx_fail(STX_ERR_INVALID, "the mask belongs to another context");
    const int W = mask->w, H = mask->h;
    if (W <= 0 || H <= 0) return stx_fail(STX_ERR_INVALID, "empty mask");
    if (H > 65535) return stx_fail(STX_ERR_INVALID, "mask of %d rows: at most 65535", H);
    if ((long long)W * H >= (1ll << 31) - 1) return stx_fail(STX_ERR_INVALID, "mask of %d x %d pixels: at most 2^31 - 2 pixels", W, H);
    STX_TRY(stx_set_device(ctx));
    // locals go in the reverse order of their declaration: the guard's wait first, behind it the blocks in the order they were taken
    // (lab, scratch, best, res), then the events
    StxEventTimer timer;
    StxDevBlock res, best, scratch, lab;
    StxRunGuard wait(ctx);
    const long long N = (long long)W * H;
    const int grid = std::min(H, CROP_ROWS_GRID);
    const bool in_lds = W <= CROP_LDS_MAX_W;
    STX_TRY(stx_dev_alloc(ctx, sizeof(int) * (size_t)(N + 1), &lab));
    STX_TRY(stx_dev_alloc(ctx, in_lds ? 4 : sizeof(int) * 2 * (size_t)W * grid, &scratch));
    STX_TRY(stx_dev_alloc(ctx, sizeof(CropBest) * (size_t)H, &best));
    STX_TRY(stx_dev_alloc(ctx, sizeof(int) * 8, &res));
    int* d_lab = (int*)lab.get();
    int* d_res = (int*)res.get();
    if (out_info) STX_TRY(timer.arm(2));
    STX_TRY(timer.mark(0, ctx->stream));
    STX_HIP(hipMemsetAsync(d_res, 0, sizeof(int) * 8, ctx->stream));
    const CropMask M{mask->ptr, (long long)mask->stride, W, H};
    const dim3 px((W + CROP_WG - 1) / CROP_WG, H);
    {
        StxProfScope prof(ctx, "crop_runs", (double)N * 5);
        hipLaunchKernelGGL(crop_runs_kernel, dim3((H + CROP_WG / 64 - 1) / (CROP_WG / 64)), dim3(CROP_WG), 0, ctx->stream, M, d_lab);
        STX_TRY(stx_check_launch("crop_runs"));
    }
    {
        StxProfScope prof(ctx, "crop_merge", (double)N * 2);
        hipLaunchKernelGGL(crop_merge_kernel, px, dim3(CROP_WG), 0, ctx->stream, M, d_lab);
        STX_TRY(stx_check_launch("crop_merge"));
    }
    {
        StxProfScope prof(ctx, "crop_count", (double)N * 5);
        hipLaunchKernelGGL(crop_count_kernel, px, dim3(CROP_WG), 0, ctx->stream, M, (const int*)d_lab, d_res);
        STX_TRY(stx_check_launch("crop_count"));
    }
    // the labels are dead from here: their buffer holds v
    int* d_v = d_lab;
    {
        StxProfScope prof(ctx, "crop_cols", (double)N * 5);
        hipLaunchKernelGGL(crop_cols_kernel, dim3((W + CROP_WG - 1) / CROP_WG), dim3(CROP_WG), 0, ctx->stream, M, d_v);
        STX_TRY(stx_check_launch("crop_cols"));
    }
    {
        CropRowsK K{d_v, W, H, (int*)scratch.get(), (CropBest*)best.get()};
        StxProfScope prof(ctx, "crop_rows", (double)N * 4);
        hipLaunchKernelGGL(crop_rows_kernel, dim3(grid), dim3(CROP_WG), in_lds ? sizeof(int) * 3 * (size_t)W : 0, ctx->stream, K);
        STX_TRY(stx_check_launch("crop_rows"));
    }
    {
        StxProfScope prof(ctx, "crop_reduce", (double)H * sizeof(CropBest));
        hipLaunchKernelGGL(crop_reduce_kernel, dim3(1), dim3(CROP_WG), 0, ctx->stream, (const CropBest*)best.get(), H, d_res);
        STX_TRY(stx_check_launch("crop_reduce"));
    }
    STX_TRY(timer.mark(1, ctx->stream));
    int h_res[8] = {0};
    STX_HIP(hipMemcpyAsync(h_res, d_res, sizeof(h_res), hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));
    out_contours[0] = h_res[0];
    out_contours[1] = h_res[1];
    for (int k = 0; k < 4; k++) out_xywh[k] = h_res[2 + k];
    if (out_info) STX_TRY(timer.ms(0, 1, &out_info[0]));
    return STX_OK;
}
