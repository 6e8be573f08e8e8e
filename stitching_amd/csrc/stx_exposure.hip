// stx_exposure.hip — overlap statistics of exposure-gain estimation (ExposureCompensator::feed) for gfx950.
//
// One launch per feed over a table of pair jobs (stx_exposure_host.cpp builds it): a job is two units (whole images or blocks) whose
// rectangles overlap, or a unit paired with itself, and the intersection rectangle in both images.  One workgroup per job produces
// c = the number of pixels where both masks are 255 and the sums of the pixels' norms over them:
//   EXP_TREE    ("gain": whole-image overlaps, up to 1e5 pixels) fp64 norms, every lane sums a fixed stride of the pixels, then a fixed
//               LDS tree: identical run to run, not the sequential sum's bits.  No float atomics.
//   EXP_ORDERED ("gain_blocks": at most one block of pixels) fp64 norms made in parallel a row-major chunk of 256 at a time, summed
//               in row-major order by one lane per image (the restatement's order: its I is bit-identical).  A pixel outside the
//               masks adds 0.0, which leaves a sum of non-negative values unchanged.
//   EXP_INT     (the channel kinds) per-channel integer sums: exact in any order.
// Norms come from a host-made table sqrt(k), k = b^2 + g^2 + r^2 <= 3 * 255^2 (correctly rounded by the host's libm), so they are the
// restatement's by construction.
#include "stx_device_math.h"
#include "stx_internal.h"

namespace {

constexpr int EXP_WG = 256;

struct ExpStatsK {
    const StxExpImg* imgs;
    const StxExpJob* jobs;
    const double* sqrt_tab;
    long long* out_i;  // 7 per job: c, B G R sums of a, B G R sums of b (EXP_INT)
    double* out_d;     // 2 per job: norm sums of a and b (EXP_TREE / EXP_ORDERED)
    int mode;
};

__global__ __launch_bounds__(EXP_WG) void exposure_stats_kernel(ExpStatsK K)
{
    const StxExpJob J = K.jobs[blockIdx.x];
    const StxExpImg A = K.imgs[J.ia], B = K.imgs[J.ib];
    const int tid = threadIdx.x;
    const int n = J.w * J.h;
    __shared__ double sa[EXP_WG], sb[EXP_WG];
    __shared__ long long si[EXP_WG];
    long long c = 0, ia[3] = {0, 0, 0}, ib[3] = {0, 0, 0};
    double da = 0.0, db = 0.0;
    for (int base = 0; base < n; base += EXP_WG) {
        const int p = base + tid;
        double va = 0.0, vb = 0.0;
        if (p < n) {
            const int y = p / J.w, x = p - y * J.w;
            const bool in = A.mask[(long long)(J.ay + y) * A.mstride + J.ax + x] == 255 &&
                            B.mask[(long long)(J.by + y) * B.mstride + J.bx + x] == 255;
            if (in) {
                const uint8_t* pa = A.img + (long long)(J.ay + y) * A.istride + 3ll * (J.ax + x);
                const uint8_t* pb = B.img + (long long)(J.by + y) * B.istride + 3ll * (J.bx + x);
                c++;
                if (K.mode == STX_EXP_INT) {
                    for (int k = 0; k < 3; k++) { ia[k] += pa[k]; ib[k] += pb[k]; }
                } else {
                    va = K.sqrt_tab[pa[0] * pa[0] + pa[1] * pa[1] + pa[2] * pa[2]];
                    vb = K.sqrt_tab[pb[0] * pb[0] + pb[1] * pb[1] + pb[2] * pb[2]];
                }
            }
        }
        if (K.mode == STX_EXP_TREE) {
            da += va;  // lane t sums pixels t, t + 256, ... in that order
            db += vb;
        } else if (K.mode == STX_EXP_ORDERED) {
            sa[tid] = va;
            sb[tid] = vb;
            __syncthreads();
            const int cnt = min(EXP_WG, n - base);
            if (tid == 0) {
                for (int t = 0; t < cnt; t++) da += sa[t];
            } else if (tid == 64) {  // another wavefront: the two chains run side by side
                for (int t = 0; t < cnt; t++) db += sb[t];
            }
            __syncthreads();
        }
    }
    // count (and integer sums): any order
    long long vals[7] = {c, ia[0], ia[1], ia[2], ib[0], ib[1], ib[2]};
    const int nv = K.mode == STX_EXP_INT ? 7 : 1;
    for (int v = 0; v < nv; v++) {
        si[tid] = vals[v];
        __syncthreads();
        for (int s = EXP_WG / 2; s > 0; s >>= 1) {
            if (tid < s) si[tid] += si[tid + s];
            __syncthreads();
        }
        if (tid == 0) K.out_i[7ll * blockIdx.x + v] = si[0];
        __syncthreads();
    }
    if (K.mode == STX_EXP_TREE) {
        sa[tid] = da;
        sb[tid] = db;
        __syncthreads();
        for (int s = EXP_WG / 2; s > 0; s >>= 1) {  // fixed pairing: lane t adds lane t + s
            if (tid < s) { sa[tid] += sa[tid + s]; sb[tid] += sb[tid + s]; }
            __syncthreads();
        }
        if (tid == 0) { K.out_d[2ll * blockIdx.x] = sa[0]; K.out_d[2ll * blockIdx.x + 1] = sb[0]; }
    } else if (K.mode == STX_EXP_ORDERED) {
        if (tid == 0) K.out_d[2ll * blockIdx.x] = da;
        if (tid == 64) K.out_d[2ll * blockIdx.x + 1] = db;
    }
}

// between feeds: every pixel multiplied by the gain (BGR triple) of its block, as cv::multiply rounds (fp32 product, cvRound, saturate)
struct ExpBlockMulK { const StxExpBlockMul* tab; };
__global__ __launch_bounds__(EXP_WG) void exposure_block_mul_kernel(ExpBlockMulK K)
{
    const StxExpBlockMul P = K.tab[blockIdx.y];
    const int n = P.w * P.h;
    for (int p = blockIdx.x * EXP_WG + threadIdx.x; p < n; p += gridDim.x * EXP_WG) {
        const int y = p / P.w, x = p - y * P.w;
        const float* g = P.g + (long long)((y / P.bh) * P.bpw + x / P.bw) * (P.g3 ? 3 : 1);
        uint8_t* px = P.img + (long long)y * P.stride + 3ll * x;
        for (int k = 0; k < 3; k++) {
            const float v = stxd::fmul((float)px[k], g[P.g3 ? k : 0]);
            px[k] = (uint8_t)min(max(stxd::cv_round(v), 0), 255);
        }
    }
}

}  // namespace

int stx_launch_exposure_stats(stx_ctx* ctx, const StxExpImg* d_imgs, const StxExpJob* d_jobs, int njobs, int mode, const double* d_sqrt,
                              long long* d_out_i, double* d_out_d, double algo_bytes)
{
    if (njobs <= 0) return STX_OK;
    ExpStatsK K;
    K.imgs = d_imgs; K.jobs = d_jobs; K.sqrt_tab = d_sqrt; K.out_i = d_out_i; K.out_d = d_out_d; K.mode = mode;
    StxProfScope prof(ctx, "exposure_stats", algo_bytes);
    hipLaunchKernelGGL(exposure_stats_kernel, dim3(njobs), dim3(EXP_WG), 0, ctx->stream, K);
    return stx_check_launch("exposure_stats");
}

int stx_launch_exposure_block_mul(stx_ctx* ctx, const StxExpBlockMul* d_tab, int n, int max_pixels)
{
    if (n <= 0) return STX_OK;
    ExpBlockMulK K;
    K.tab = d_tab;
    const int gx = std::min(64, std::max(1, (max_pixels + EXP_WG - 1) / EXP_WG));
    StxProfScope prof(ctx, "exposure_block_mul", 0.0);
    hipLaunchKernelGGL(exposure_block_mul_kernel, dim3(gx, n), dim3(EXP_WG), 0, ctx->stream, K);
    return stx_check_launch("exposure_block_mul");
}
