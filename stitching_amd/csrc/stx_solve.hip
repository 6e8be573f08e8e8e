// stx_solve.hip — cv::solve(DECOMP_LU) in fp64 on gfx950 for the exposure compensators' gain systems: the bits of the host solve
// (lu_solve_sparse in stx_exposure_host.cpp; tests/numpy_exposure.py::lu_solve(skip_zeros=False) is the dense statement).
//
// The matrix is dense row-major fp64 in one allocator block, augmented by b as column n: a row swap and the update
// b[j] = b[j] + alpha * b[i] are then the same operations as on any other column.  A blocked right-looking elimination, LU_NB pivots
// per step, four launches per step and no host synchronisation before the end:
//   1. lu_panel_kernel     one workgroup factors the LU_NB panel columns over all rows below: pivot search (largest |a|, the smallest
//                          row among equals), swap inside the panel, alpha = a[j][i] * (-1 / a[i][i]) stored in place of a[j][i],
//                          a[j][k] = a[j][k] + alpha * a[i][k] for the panel's remaining columns.  Pivot rows go to piv[] on the device.
//   2. lu_swap_trsm_kernel one thread per column right of the panel: the panel's row swaps in order, then the panel's own LU_NB rows
//                          brought up to date pivot by pivot.
//   3. lu_trail_kernel     one 64 x 64 tile of the trailing block per workgroup, 4 x 4 values per thread in registers; the panel's
//                          pivots are applied ONE AFTER THE OTHER, in order, as a = a + l * u from LDS copies of the alphas and of the
//                          pivot rows — never sum(l * u) first.  Every element therefore receives its updates from the pivots
//                          0, 1, 2, ... in ascending order, each as one rounded product and one rounded sum: the host loop's sequence.
// A tile whose alphas or whose pivot-row part are all zero is passed over: x + alpha * 0 == x and x + 0 * u == x while x is never -0
// (the argument above lu_solve_sparse: a stored value is an input or a rounded sum, and a sum that cancels is +0); rows with a zero
// in the pivot column are passed over in the panel for the same reason.  The inputs must hold no -0, Inf or NaN.
// No FMA anywhere: the file is compiled with -ffp-contract=off (Makefile) and says so itself below; MFMA f64 accumulates fused and is not used.
//
// The back substitution is one dependent chain (row i's sum starts at x[i + 1]), so it stays on the host: the non-zeros of every row
// of U and the transformed b are compacted on the device (lu_count_kernel, lu_fill_kernel), copied back, and substituted in the
// host loop's order.  The dense matrix never crosses PCIe.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>

#include "stx_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int LU_NB = 32;       // pivots per step
constexpr int LU_T = 64;        // tile edge of the trailing update
constexpr int LU_PANEL_WG = 1024;

// the larger magnitude, among equals the smaller row: what the ascending strict-> search of the host finds
__device__ inline void lu_better(double& v, int& i, double ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ void lu_scatter_kernel(double* A, long long lda, const StxLuEntry* ent, long long count)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) A[(long long)ent[e].row * lda + ent[e].col] = ent[e].v;
}

// *info: 0, or 1 + the row the system was found singular at (every later launch then returns at once)
__global__ __launch_bounds__(LU_PANEL_WG) void lu_panel_kernel(double* A, long long lda, int n, int k0, int* piv, int* info)
{
    __shared__ double s_row[LU_NB];
    __shared__ double s_v[LU_PANEL_WG / 64];
    __shared__ int s_i[LU_PANEL_WG / 64];
    __shared__ int s_p;
    if (*info) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hl = tid & 31, grp = tid >> 5;  // elimination: 32 lanes per row, lane = panel column
    const int kend = min(k0 + LU_NB, n);
    for (int c = k0; c < kend; c++) {
        double best = 0.0;
        int bi = INT_MAX;
        for (int j = c + tid; j < n; j += LU_PANEL_WG) {
            const double v = fabs(A[(long long)j * lda + c]);
            if (v > best) { best = v; bi = j; }
        }
        for (int o = 32; o; o >>= 1) {
            const double ov = __shfl_down(best, o);
            const int oi = __shfl_down(bi, o);
            lu_better(best, bi, ov, oi);
        }
        if (lane == 0) { s_v[wave] = best; s_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < LU_PANEL_WG / 64; w++) lu_better(best, bi, s_v[w], s_i[w]);
            if (!(best > 0.0)) { *info = c + 1; s_p = -1; }
            else { s_p = bi; piv[c] = bi; }
        }
        __syncthreads();
        const int p = s_p;
        if (p < 0) return;
        if (tid < LU_NB) {  // the swap inside the panel; the pivot row to LDS
            double* rc = A + (long long)c * lda + k0 + tid;
            double* rp = A + (long long)p * lda + k0 + tid;
            const double vc = *rc, vp = *rp;
            if (p != c) { *rc = vp; *rp = vc; }
            s_row[tid] = vp;
        }
        __syncthreads();
        const int ci = c - k0;
        const double d = -1.0 / s_row[ci];
        const double u = s_row[hl];
        for (int j = c + 1 + grp; j < n; j += LU_PANEL_WG / 32) {
            double* r = A + (long long)j * lda + k0;
            const double v = r[hl];
            const double ac = __shfl(v, ci, 32);
            if (ac != 0.0) {
                const double alpha = ac * d;
                if (hl == ci) r[hl] = alpha;
                else if (hl > ci) r[hl] = v + alpha * u;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void lu_swap_trsm_kernel(double* A, long long lda, int Nc, int k0, int npiv, const int* piv, const int* info)
{
    __shared__ double s_L[LU_NB][LU_NB + 1];
    __shared__ int s_piv[LU_NB];
    if (*info) return;
    const int tid = threadIdx.x;
    for (int e = tid; e < LU_NB * LU_NB; e += 64) s_L[e >> 5][e & 31] = A[(long long)(k0 + (e >> 5)) * lda + k0 + (e & 31)];
    if (tid < LU_NB) s_piv[tid] = tid < npiv ? piv[k0 + tid] : k0 + tid;
    __syncthreads();
    const int k = k0 + LU_NB + blockIdx.x * 64 + tid;
    if (k >= Nc) return;
    double* col = A + k;
    for (int i = 0; i < npiv; i++) {
        const int p = s_piv[i];
        if (p != k0 + i) {
            const double a = col[(long long)(k0 + i) * lda], b = col[(long long)p * lda];
            col[(long long)(k0 + i) * lda] = b;
            col[(long long)p * lda] = a;
        }
    }
    double v[LU_NB];
#pragma unroll
    for (int r = 0; r < LU_NB; r++) v[r] = col[(long long)(k0 + r) * lda];
#pragma unroll
    for (int p = 0; p < LU_NB - 1; p++) {
        if (p < npiv) {
#pragma unroll
            for (int r = p + 1; r < LU_NB; r++) v[r] = v[r] + s_L[r][p] * v[p];
        }
    }
#pragma unroll
    for (int r = 1; r < LU_NB; r++) col[(long long)(k0 + r) * lda] = v[r];
}

__global__ __launch_bounds__(256) void lu_trail_kernel(double* A, long long lda, int n, int Nc, int k0, const int* info)
{
    __shared__ double sL[LU_NB][LU_T + 2];  // sL[p][r]: alpha of row r0 + r for pivot k0 + p
    __shared__ double sU[LU_NB][LU_T];      // sU[p][c]: pivot row k0 + p at column c0 + c
    if (*info) return;
    const int tid = threadIdx.x;
    const int r0 = k0 + LU_NB + blockIdx.y * LU_T, c0 = k0 + LU_NB + blockIdx.x * LU_T;
    int nz = 0;
    for (int e = tid; e < LU_T * LU_NB; e += 256) {
        const int r = e >> 5, p = e & 31;
        const double v = r0 + r < n ? A[(long long)(r0 + r) * lda + k0 + p] : 0.0;
        sL[p][r] = v;
        nz |= v != 0.0;
    }
    if (!__syncthreads_or(nz)) return;
    nz = 0;
    for (int e = tid; e < LU_T * LU_NB; e += 256) {
        const int p = e >> 6, c = e & 63;
        const double v = c0 + c < Nc ? A[(long long)(k0 + p) * lda + c0 + c] : 0.0;
        sU[p][c] = v;
        nz |= v != 0.0;
    }
    if (!__syncthreads_or(nz)) return;
    const int ty = tid >> 4, tx = tid & 15;
    const bool cin = c0 + tx * 4 < Nc;  // Nc is a multiple of 4: a thread's four columns are inside or outside together
    double a[4][4];
    double* base = A + (long long)(r0 + ty * 4) * lda + c0 + tx * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (cin && r0 + ty * 4 + i < n) {
            const double2 x = *(const double2*)(base + i * lda), y = *(const double2*)(base + i * lda + 2);
            a[i][0] = x.x; a[i][1] = x.y; a[i][2] = y.x; a[i][3] = y.y;
        } else {
            a[i][0] = a[i][1] = a[i][2] = a[i][3] = 0.0;
        }
    }
#pragma unroll 8
    for (int p = 0; p < LU_NB; p++) {
        const double2 l0 = *(const double2*)&sL[p][ty * 4], l1 = *(const double2*)&sL[p][ty * 4 + 2];
        const double2 u0 = *(const double2*)&sU[p][tx * 4], u1 = *(const double2*)&sU[p][tx * 4 + 2];
        const double l[4] = {l0.x, l0.y, l1.x, l1.y}, u[4] = {u0.x, u0.y, u1.x, u1.y};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) a[i][j] = __dadd_rn(a[i][j], __dmul_rn(l[i], u[j]));
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (cin && r0 + ty * 4 + i < n) {
            *(double2*)(base + i * lda) = make_double2(a[i][0], a[i][1]);
            *(double2*)(base + i * lda + 2) = make_double2(a[i][2], a[i][3]);
        }
    }
}

// one wavefront per row of U: its non-zeros from the diagonal on (the diagonal is a pivot: never zero)
__global__ __launch_bounds__(256) void lu_count_kernel(const double* A, long long lda, int n, int* cnt)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    int c = 0;
    for (int k = row + lane; k < n; k += 64) c += A[(long long)row * lda + k] != 0.0;
    for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
    if (lane == 0) cnt[row] = c;
}

__global__ __launch_bounds__(256) void lu_fill_kernel(const double* A, long long lda, int n, const long long* off, int* cols, double* vals,
                                                     double* bout)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    long long at = off[row];
    for (int kk = row; kk < n; kk += 64) {  // columns ascending: the order of the host's sum
        const int k = kk + lane;
        const double v = k < n ? A[(long long)row * lda + k] : 0.0;
        const bool keep = v != 0.0;
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const long long o = at + __popcll(m & ((1ull << lane) - 1ull));
            cols[o] = k;
            vals[o] = v;
        }
        at += __popcll(m);
    }
    if (lane == 0) bout[row] = A[(long long)row * lda + n];
}

}  // namespace

// Solves the n x n system given by its non-zero entries (col < n) and its right side (col == n) -> x[n].  out (or null): {device ms of
// scatter + elimination (HIP events), ms of compaction + copy + host back substitution, non-zeros of U}.
int stx_lu_device(stx_ctx* ctx, int n, const StxLuEntry* ent, size_t count, double* x, double out[3])
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (n < 1 || !x || (count > 0 && !ent)) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (n > STX_LU_MAX_N)
        return stx_fail(STX_ERR_INVALID, "device LU: n = %d unknowns exceed the limit of %d (the dense fp64 matrix takes 8 n^2 bytes)", n,
                        STX_LU_MAX_N);
    for (size_t e = 0; e < count; e++)
        if (ent[e].row < 0 || ent[e].row >= n || ent[e].col < 0 || ent[e].col > n)
            return stx_fail(STX_ERR_INVALID, "internal: LU entry outside the system");
    STX_TRY(stx_set_device(ctx));
    const int Nr = (n + LU_NB - 1) / LU_NB * LU_NB, Nc = (n + 1 + LU_NB - 1) / LU_NB * LU_NB;
    const long long lda = Nc;
    const size_t bytes = (size_t)Nr * Nc * sizeof(double);
    StxDevBlock d_A, d_ent, d_piv, d_cnt, d_off, d_cols, d_vals, d_b;
    STX_TRY(stx_dev_alloc(ctx, bytes, &d_A));
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>(1, count) * sizeof(StxLuEntry), &d_ent));
    STX_TRY(stx_dev_alloc(ctx, sizeof(int) * (Nr + 1), &d_piv));  // piv[Nr] is the info word
    STX_TRY(stx_dev_alloc(ctx, sizeof(int) * n, &d_cnt));
    STX_TRY(stx_dev_alloc(ctx, sizeof(long long) * (n + 1), &d_off));
    STX_TRY(stx_dev_alloc(ctx, sizeof(double) * n, &d_b));
    double* A = (double*)d_A.get();
    int* piv = (int*)d_piv.get();
    int* info = piv + Nr;
    StxEventTimer timer;
    if (out) STX_TRY(timer.arm(2));
    hipStream_t st = ctx->stream;
    STX_TRY(timer.mark(0, st));
    STX_HIP(hipMemsetAsync(A, 0, bytes, st));
    STX_HIP(hipMemsetAsync(piv, 0, sizeof(int) * (Nr + 1), st));
    if (count) {
        STX_HIP(hipMemcpyAsync(d_ent.get(), ent, count * sizeof(StxLuEntry), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lu_scatter_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, A, lda, (const StxLuEntry*)d_ent.get(),
                           (long long)count);
        STX_TRY(stx_check_launch("lu_scatter"));
    }
    for (int k0 = 0; k0 < n; k0 += LU_NB) {
        hipLaunchKernelGGL(lu_panel_kernel, dim3(1), dim3(LU_PANEL_WG), 0, st, A, lda, n, k0, piv, info);
        const int right = Nc - k0 - LU_NB, below = n - k0 - LU_NB;
        if (right > 0)
            hipLaunchKernelGGL(lu_swap_trsm_kernel, dim3((right + 63) / 64), dim3(64), 0, st, A, lda, Nc, k0, std::min(LU_NB, n - k0),
                               (const int*)piv, (const int*)info);
        if (right > 0 && below > 0)
            hipLaunchKernelGGL(lu_trail_kernel, dim3((right + LU_T - 1) / LU_T, (below + LU_T - 1) / LU_T), dim3(256), 0, st, A, lda, n, Nc, k0,
                               (const int*)info);
    }
    STX_TRY(stx_check_launch("lu elimination"));
    STX_TRY(timer.mark(1, st));
    hipLaunchKernelGGL(lu_count_kernel, dim3((n + 3) / 4), dim3(256), 0, st, (const double*)A, lda, n, (int*)d_cnt.get());
    STX_TRY(stx_check_launch("lu_count"));
    std::vector<int> cnt(n);
    int h_info = 0;
    STX_HIP(hipMemcpyAsync(cnt.data(), d_cnt.get(), sizeof(int) * n, hipMemcpyDeviceToHost, st));
    STX_HIP(hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, st));
    STX_HIP(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    if (out) {
        STX_TRY(timer.ms(0, 1, &out[0]));
        out[1] = 0.0; out[2] = 0.0;
    }
    if (h_info) return stx_fail(STX_ERR_INVALID, "exposure system is singular at row %d", h_info - 1);
    std::vector<long long> off(n + 1, 0);
    for (int i = 0; i < n; i++) {
        if (cnt[i] < 1) return stx_fail(STX_ERR_INVALID, "internal: row %d of U has no diagonal", i);
        off[i + 1] = off[i] + cnt[i];
    }
    const long long nnz = off[n];
    STX_TRY(stx_dev_alloc(ctx, sizeof(int) * nnz, &d_cols));
    STX_TRY(stx_dev_alloc(ctx, sizeof(double) * nnz, &d_vals));
    STX_HIP(hipMemcpyAsync(d_off.get(), off.data(), sizeof(long long) * (n + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lu_fill_kernel, dim3((n + 3) / 4), dim3(256), 0, st, (const double*)A, lda, n, (const long long*)d_off.get(),
                       (int*)d_cols.get(), (double*)d_vals.get(), (double*)d_b.get());
    STX_TRY(stx_check_launch("lu_fill"));
    std::vector<int> cols(nnz);
    std::vector<double> vals(nnz);
    STX_HIP(hipMemcpyAsync(cols.data(), d_cols.get(), sizeof(int) * nnz, hipMemcpyDeviceToHost, st));
    STX_HIP(hipMemcpyAsync(vals.data(), d_vals.get(), sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
    STX_HIP(hipMemcpyAsync(x, d_b.get(), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    STX_HIP(hipStreamSynchronize(st));
    // the host loop of lu_solve_sparse: s -= a[i][k] * x[k] with k ascending over the non-zeros, then the division by the pivot
    for (int i = n - 1; i >= 0; i--) {
        double s = x[i];
        for (long long e = off[i] + 1; e < off[i + 1]; e++) s -= vals[e] * x[cols[e]];
        x[i] = s / vals[off[i]];
    }
    if (out) {
        out[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        out[2] = (double)nnz;
    }
    return STX_OK;
}
