// stx_exposure_host.cpp — host side of exposure-gain estimation (ExposureCompensator::feed): units and pair jobs, the feeds, the
// assembly and solve of GainCompensator::singleFeed, the gain-map filter of the block compensators.  Compiled without contraction
// (Makefile: -ffp-contract=off): every product and sum is the separate IEEE operation the restatement (tests/numpy_exposure.py) makes.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "stx_internal.h"

namespace {

constexpr double EXP_ALPHA = 0.01, EXP_BETA = 100.0;
constexpr int EXP_SQRT_N = 3 * 255 * 255 + 1;

bool kind_blocks(int kind) { return kind == STX_EXPOSURE_GAIN_BLOCKS || kind == STX_EXPOSURE_CHANNELS_BLOCKS; }
bool kind_channels(int kind) { return kind == STX_EXPOSURE_CHANNELS || kind == STX_EXPOSURE_CHANNELS_BLOCKS; }

// ---------------------------------------------------------------------------------------------------------------------------------
// assembly + cv::solve(DECOMP_LU)
// ---------------------------------------------------------------------------------------------------------------------------------
struct PairStat { int i, j; double n, iij, iji; };
using SparseRow = std::vector<std::pair<int, double>>;  // (column, value), columns increasing, no zero values

double det2(const double* S) { return S[0] * S[3] - S[1] * S[2]; }
double det3(const double* S)
{
    return S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
}

// cv::solve's branch for m <= 3: x = b / a, Cramer's rule with d = 1 / det (S row-major m x m)
void solve_small(int m, const double* S, const double* B, double* x)
{
    if (m == 1) {
        x[0] = B[0] / S[0];
    } else if (m == 2) {
        const double d = 1.0 / det2(S);
        const double t = (B[0] * S[3] - B[1] * S[1]) * d;
        x[1] = (B[1] * S[0] - B[0] * S[2]) * d;
        x[0] = t;
    } else {
        const double d = 1.0 / det3(S);
        x[0] = d * (B[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (B[1] * S[8] - S[5] * B[2]) + S[2] * (B[1] * S[7] - S[4] * B[2]));
        x[1] = d * (S[0] * (B[1] * S[8] - S[5] * B[2]) - B[0] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * B[2] - B[1] * S[6]));
        x[2] = d * (S[0] * (S[4] * B[2] - B[1] * S[7]) - S[1] * (S[3] * B[2] - B[1] * S[6]) + B[0] * (S[3] * S[7] - S[4] * S[6]));
    }
}

// OpenCV's LU with partial pivoting and back substitution, touching only non-zero entries.  Adding alpha * 0 changes no value (A never
// holds -0: every stored value is a product-free copy or a rounded sum, and a sum that cancels is +0), a zero is never the largest pivot
// candidate of a non-singular system and s -= 0 * x leaves s: the bits of the dense loop.  Before step i no row j >= i holds a column < i.
int lu_solve_sparse(std::vector<SparseRow>& R, std::vector<double>& b)
{
    const int m = (int)R.size();
    SparseRow merged, tail;
    for (int i = 0; i < m; i++) {
        int p = i;
        double best = (!R[i].empty() && R[i][0].first == i) ? std::fabs(R[i][0].second) : 0.0;
        for (int j = i + 1; j < m; j++)
            if (!R[j].empty() && R[j][0].first == i && std::fabs(R[j][0].second) > best) { best = std::fabs(R[j][0].second); p = j; }
        if (!(best > 0.0)) return stx_fail(STX_ERR_INVALID, "exposure system is singular at row %d", i);
        if (p != i) { std::swap(R[i], R[p]); std::swap(b[i], b[p]); }
        const double d = -1.0 / R[i][0].second;
        tail.assign(R[i].begin() + 1, R[i].end());
        for (int j = i + 1; j < m; j++) {
            SparseRow& r = R[j];
            if (r.empty() || r[0].first != i) continue;
            const double alpha = r[0].second * d;
            merged.clear();
            size_t a = 1, t = 0;
            while (a < r.size() || t < tail.size()) {
                double v;
                int col;
                if (t == tail.size() || (a < r.size() && r[a].first < tail[t].first)) {
                    col = r[a].first; v = r[a].second; a++;
                } else if (a == r.size() || tail[t].first < r[a].first) {
                    col = tail[t].first; v = 0.0 + alpha * tail[t].second; t++;
                } else {
                    col = r[a].first; v = r[a].second + alpha * tail[t].second; a++; t++;
                }
                if (v != 0.0) merged.emplace_back(col, v);
            }
            r.swap(merged);
            b[j] = b[j] + alpha * b[i];
        }
    }
    for (int i = m - 1; i >= 0; i--) {
        double s = b[i];
        for (size_t k = 1; k < R[i].size(); k++) s -= R[i][k].second * b[R[i][k].first];
        b[i] = s / R[i][0].second;
    }
    return STX_OK;
}

// The same system by the dense LU on the device (stx_solve.hip): the assembled rows and b (as column m) are its entries.  acc (or null)
// gathers {device elimination ms, compaction + copy + back substitution ms, non-zeros of U} over the solves of a feed.
int lu_solve_device(stx_ctx* dev, const std::vector<SparseRow>& R, std::vector<double>& b, double* acc)
{
    const int m = (int)R.size();
    std::vector<StxLuEntry> ent;
    for (int r = 0; r < m; r++) {
        for (const auto& e : R[r]) ent.push_back({r, e.first, e.second});
        if (b[r] != 0.0) ent.push_back({r, m, b[r]});
    }
    double info[3] = {0.0, 0.0, 0.0};
    STX_TRY(stx_lu_device(dev, m, ent.data(), ent.size(), b.data(), info));
    if (acc)
        for (int k = 0; k < 3; k++) acc[k] += info[k];
    return STX_OK;
}

// GainCompensator::singleFeed's system over the non-skipped units, solved: gains of all m units (skipped ones 1).  dev: null for the
// host LU, else the context whose device runs the elimination (more than 3 unknowns; Cramer's rule stays on the host)
int exp_solve(int m, const std::vector<PairStat>& pairs, const std::vector<char>& skip, double* gains, stx_ctx* dev = nullptr,
              double* dev_acc = nullptr)
{
    std::vector<int> k(m, -1);
    int mm = 0;
    for (int u = 0; u < m; u++) {
        gains[u] = 1.0;
        if (!skip[u]) k[u] = mm++;
    }
    if (mm == 0) return STX_OK;
    // per unit, its partners in index order (each pair once per direction)
    struct Adj { int j; double n, iij, iji; };
    std::vector<std::vector<Adj>> adj(m);
    for (const PairStat& p : pairs) {
        if (k[p.i] < 0 || k[p.j] < 0 || p.n == 0.0) continue;
        adj[p.i].push_back({p.j, p.n, p.iij, p.iji});
        if (p.i != p.j) adj[p.j].push_back({p.i, p.n, p.iji, p.iij});
    }
    std::vector<SparseRow> R(mm);
    std::vector<double> b(mm, 0.0);
    for (int i = 0; i < m; i++) {
        if (k[i] < 0) continue;
        std::vector<Adj>& a = adj[i];
        std::sort(a.begin(), a.end(), [](const Adj& x, const Adj& y) { return x.j < y.j; });
        const int ki = k[i];
        double diag = 0.0, bb = 0.0;
        SparseRow& row = R[ki];
        for (const Adj& e : a) {
            bb += EXP_BETA * e.n;
            diag += EXP_BETA * e.n;
            if (e.j != i) {
                diag += 2 * EXP_ALPHA * e.iij * e.iij * e.n;
                const double off = 0.0 - 2 * EXP_ALPHA * e.iij * e.iji * e.n;
                if (off != 0.0) row.emplace_back(k[e.j], off);
            }
        }
        if (diag != 0.0) row.emplace_back(ki, diag);
        std::sort(row.begin(), row.end());
        b[ki] = bb;
    }
    std::vector<double> x(mm);
    if (mm <= 3) {
        double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int r = 0; r < mm; r++)
            for (auto& e : R[r]) S[r * mm + e.first] = e.second;
        solve_small(mm, S, b.data(), x.data());
    } else {
        if (dev) STX_TRY(lu_solve_device(dev, R, b, dev_acc));
        else STX_TRY(lu_solve_sparse(R, b));
        x = b;
    }
    for (int u = 0; u < m; u++)
        if (k[u] >= 0) gains[u] = x[k[u]];
    return STX_OK;
}

// sepFilter2D([.25 .5 .25] x [.25 .5 .25]) twice, REFLECT_101, fp32 as 0.5f * c + 0.25f * (l + r); a 1-long axis stays; ch channels
void filter_map(std::vector<float>& g, int w, int h, int ch)
{
    std::vector<float> t(g.size());
    auto refl = [](int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); };
    for (int pass = 0; pass < 2; pass++) {
        if (w > 1) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++)
                    for (int c = 0; c < ch; c++) {
                        const float l = g[((size_t)y * w + refl(x - 1, w)) * ch + c], r = g[((size_t)y * w + refl(x + 1, w)) * ch + c];
                        t[((size_t)y * w + x) * ch + c] = 0.5f * g[((size_t)y * w + x) * ch + c] + 0.25f * (l + r);
                    }
            g.swap(t);
        }
        if (h > 1) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++)
                    for (int c = 0; c < ch; c++) {
                        const float l = g[((size_t)refl(y - 1, h) * w + x) * ch + c], r = g[((size_t)refl(y + 1, h) * w + x) * ch + c];
                        t[((size_t)y * w + x) * ch + c] = 0.5f * g[((size_t)y * w + x) * ch + c] + 0.25f * (l + r);
                    }
            g.swap(t);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// units and pair jobs
// ---------------------------------------------------------------------------------------------------------------------------------
struct ExpGrid { int bpw, bph, bw, bh, first; };
struct ExpPlan {
    int kind = 0, n = 0, units = 0;
    std::vector<ExpGrid> grid;          // per image
    std::vector<int> uimg, ux0, uy0, ux1, uy1;  // per unit: image, rectangle in image coordinates
    std::vector<StxExpJob> jobs;
    std::vector<int> ab;                // 2 per job
    long long out_count = 0;
};

int exp_plan(int kind, int n, const stx_buf* const* imgs, const stx_buf* const* masks, const int* corners, int bl, bool jobs, ExpPlan& P)
{
    if (kind < STX_EXPOSURE_GAIN || kind > STX_EXPOSURE_CHANNELS_BLOCKS) return stx_fail(STX_ERR_INVALID, "unknown exposure kind %d", kind);
    if (n < 0 || (n > 0 && (!imgs || !masks || !corners))) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (bl < 1) return stx_fail(STX_ERR_INVALID, "block size must be >= 1");
    P.kind = kind; P.n = n;
    const stx_ctx* c0 = n > 0 && imgs[0] ? imgs[0]->ctx : nullptr;
    const bool blocks = kind_blocks(kind);
    for (int i = 0; i < n; i++) {
        const stx_buf* im = imgs[i];
        const stx_buf* mk = masks[i];
        if (!im || !mk) return stx_fail(STX_ERR_INVALID, "null image or mask %d", i);
        if (im->elem != STX_U8 || im->c != 3) return stx_fail(STX_ERR_INVALID, "exposure estimation needs u8x3 images (image %d)", i);
        if (mk->elem != STX_U8 || mk->c != 1) return stx_fail(STX_ERR_INVALID, "exposure estimation needs u8x1 masks (mask %d)", i);
        if (mk->w != im->w || mk->h != im->h) return stx_fail(STX_ERR_INVALID, "mask %d is not the size of its image", i);
        if (im->ctx != c0 || mk->ctx != c0) return stx_fail(STX_ERR_INVALID, "images and masks must belong to one context");
        ExpGrid g;
        g.bpw = blocks ? (im->w + bl - 1) / bl : 1;
        g.bph = blocks ? (im->h + bl - 1) / bl : 1;
        g.bw = (im->w + g.bpw - 1) / g.bpw;
        g.bh = (im->h + g.bph - 1) / g.bph;
        g.first = P.units;
        P.grid.push_back(g);
        for (int by = 0; by < g.bph; by++)
            for (int bx = 0; bx < g.bpw; bx++) {
                P.uimg.push_back(i);
                P.ux0.push_back(bx * g.bw); P.uy0.push_back(by * g.bh);
                P.ux1.push_back(std::min(bx * g.bw + g.bw, im->w)); P.uy1.push_back(std::min(by * g.bh + g.bh, im->h));
            }
        P.units += g.bpw * g.bph;
        P.out_count += (long long)(blocks ? g.bpw * g.bph : 1) * (kind_channels(kind) ? 3 : 1);
    }
    if (!jobs) return STX_OK;
    auto add = [&](int u, int v) {
        const int ia = P.uimg[u], ib = P.uimg[v];
        const int ax = corners[2 * ia] + P.ux0[u], ay = corners[2 * ia + 1] + P.uy0[u];
        const int bx = corners[2 * ib] + P.ux0[v], by = corners[2 * ib + 1] + P.uy0[v];
        const int tx = std::max(ax, bx), ty = std::max(ay, by);
        const int rx = std::min(ax + P.ux1[u] - P.ux0[u], bx + P.ux1[v] - P.ux0[v]);
        const int ry = std::min(ay + P.uy1[u] - P.uy0[u], by + P.uy1[v] - P.uy0[v]);
        if (!(tx < rx && ty < ry)) return;
        StxExpJob J;
        J.ia = ia; J.ib = ib;
        J.ax = tx - corners[2 * ia]; J.ay = ty - corners[2 * ia + 1];
        J.bx = tx - corners[2 * ib]; J.by = ty - corners[2 * ib + 1];
        J.w = rx - tx; J.h = ry - ty;
        P.jobs.push_back(J);
        P.ab.push_back(u); P.ab.push_back(v);
    };
    for (int ia = 0; ia < n; ia++) {
        const ExpGrid& ga = P.grid[ia];
        for (int u = ga.first; u < ga.first + ga.bpw * ga.bph; u++) add(u, u);  // blocks of one image never overlap each other
        const int ax0 = corners[2 * ia], ay0 = corners[2 * ia + 1];
        for (int ib = ia + 1; ib < n; ib++) {
            const ExpGrid& gb = P.grid[ib];
            const int bx0 = corners[2 * ib], by0 = corners[2 * ib + 1];
            const int tx = std::max(ax0, bx0), ty = std::max(ay0, by0);
            const int rx = std::min(ax0 + imgs[ia]->w, bx0 + imgs[ib]->w), ry = std::min(ay0 + imgs[ia]->h, by0 + imgs[ib]->h);
            if (!(tx < rx && ty < ry)) continue;
            // blocks of a meeting the overlap, and for each the blocks of b meeting that block (grid arithmetic)
            for (int qy = (ty - ay0) / ga.bh; qy <= (ry - 1 - ay0) / ga.bh; qy++)
                for (int qx = (tx - ax0) / ga.bw; qx <= (rx - 1 - ax0) / ga.bw; qx++) {
                    const int u = ga.first + qy * ga.bpw + qx;
                    const int ux = std::max(ax0 + P.ux0[u], tx), uy = std::max(ay0 + P.uy0[u], ty);
                    const int urx = std::min(ax0 + P.ux1[u], rx), ury = std::min(ay0 + P.uy1[u], ry);
                    if (!(ux < urx && uy < ury)) continue;
                    for (int sy = (uy - by0) / gb.bh; sy <= (ury - 1 - by0) / gb.bh; sy++)
                        for (int sx = (ux - bx0) / gb.bw; sx <= (urx - 1 - bx0) / gb.bw; sx++)
                            add(u, gb.first + sy * gb.bpw + sx);
                }
        }
    }
    // bounds of every job inside both images (the kernel reads them unchecked)
    for (const StxExpJob& J : P.jobs)
        if (J.ax < 0 || J.ay < 0 || J.bx < 0 || J.by < 0 || J.w <= 0 || J.h <= 0 || J.ax + J.w > imgs[J.ia]->w ||
            J.ay + J.h > imgs[J.ia]->h || J.bx + J.w > imgs[J.ib]->w || J.by + J.h > imgs[J.ib]->h)
            return stx_fail(STX_ERR_INVALID, "internal: exposure job outside its images");
    return STX_OK;
}

std::mutex exp_sqrt_mutex;

int exp_sqrt_table(stx_ctx* ctx)
{
    std::lock_guard<std::mutex> lock(exp_sqrt_mutex);
    if (ctx->exp_sqrt) return STX_OK;
    std::vector<double> t(EXP_SQRT_N);
    for (int k = 0; k < EXP_SQRT_N; k++) t[k] = std::sqrt((double)k);
    StxDevBlock d;
    STX_TRY(stx_dev_alloc(ctx, t.size() * sizeof(double), &d));
    STX_HIP(hipMemcpyAsync(d.get(), t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->exp_sqrt = (double*)d.release();  // the context's from here
    return STX_OK;
}

// device side of the feeds: the job table once, the statistics of one feed per call; between feeds the multiplied images and their gain tables
// Members go in the reverse order of their declaration: the guard's wait first, and behind it everything goes back in this order — the
// scratch images, d_bg, d_bt, d_imgs, d_jobs, d_oi, d_od, the events.
struct ExpRun {
    stx_ctx* ctx;
    StxEventTimer timer;  // around the statistics launch
    StxDevBlock d_od, d_oi, d_jobs, d_imgs;
    StxDevBlock d_bt, d_bg;          // StxExpBlockMul per image, float gains per block
    std::vector<StxBufRef> scratch;  // the images multiplied between feeds (the caller's are never written)
    StxRunGuard wait;
    explicit ExpRun(stx_ctx* c) : ctx(c), wait(c) {}
};

int exp_stats(ExpRun& X, const ExpPlan& P, const stx_buf* const* imgs, const stx_buf* const* masks, std::vector<long long>& oi,
              std::vector<double>& od, double* ms)
{
    stx_ctx* ctx = X.ctx;
    const int nj = (int)P.jobs.size();
    oi.assign(7 * (size_t)nj, 0);
    od.assign(2 * (size_t)nj, 0.0);
    if (nj == 0) return STX_OK;
    if (!X.d_jobs) {
        STX_TRY(stx_dev_alloc(ctx, sizeof(StxExpImg) * P.n, &X.d_imgs));
        STX_TRY(stx_dev_alloc(ctx, sizeof(StxExpJob) * nj, &X.d_jobs));
        STX_TRY(stx_dev_alloc(ctx, sizeof(long long) * 7 * nj, &X.d_oi));
        STX_TRY(stx_dev_alloc(ctx, sizeof(double) * 2 * nj, &X.d_od));
        STX_HIP(hipMemcpyAsync(X.d_jobs.get(), P.jobs.data(), sizeof(StxExpJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<StxExpImg> tab(P.n);
    double bytes = 0.0;
    for (int i = 0; i < P.n; i++) tab[i] = {imgs[i]->ptr, (long long)imgs[i]->stride, masks[i]->ptr, (long long)masks[i]->stride};
    for (const StxExpJob& J : P.jobs) bytes += 8.0 * J.w * J.h;
    STX_HIP(hipMemcpyAsync(X.d_imgs.get(), tab.data(), sizeof(StxExpImg) * P.n, hipMemcpyHostToDevice, ctx->stream));
    const int mode = kind_channels(P.kind) ? STX_EXP_INT : (P.kind == STX_EXPOSURE_GAIN_BLOCKS ? STX_EXP_ORDERED : STX_EXP_TREE);
    if (ms) STX_TRY(X.timer.arm(2));
    STX_TRY(X.timer.mark(0, ctx->stream));
    STX_TRY(stx_launch_exposure_stats(ctx, (const StxExpImg*)X.d_imgs.get(), (const StxExpJob*)X.d_jobs.get(), nj, mode, ctx->exp_sqrt,
                                      (long long*)X.d_oi.get(), (double*)X.d_od.get(), bytes));
    STX_TRY(X.timer.mark(1, ctx->stream));
    STX_HIP(hipMemcpyAsync(oi.data(), X.d_oi.get(), sizeof(long long) * 7 * nj, hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipMemcpyAsync(od.data(), X.d_od.get(), sizeof(double) * 2 * nj, hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipStreamSynchronize(ctx->stream));
    if (ms) {
        double e = 0.0;
        STX_TRY(X.timer.ms(0, 1, &e));
        *ms += e;
    }
    return STX_OK;
}

int exp_check_ctx(stx_ctx* ctx, const ExpPlan& P, const stx_buf* const* imgs)
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (P.n > 0 && imgs[0]->ctx != ctx) return stx_fail(STX_ERR_INVALID, "images belong to another context");
    return STX_OK;
}

}  // namespace

namespace {

int exp_solve_abi(stx_ctx* dev, int m, int npairs, const int* pairs_ij, const double* n_iij_iji, const unsigned char* skip, double* out_gains,
                  double* dev_acc)
{
    if (m < 0 || npairs < 0 || (m > 0 && (!skip || !out_gains)) || (npairs > 0 && (!pairs_ij || !n_iij_iji)))
        return stx_fail(STX_ERR_INVALID, "bad argument");
    std::vector<PairStat> pairs(npairs);
    for (int p = 0; p < npairs; p++) {
        const int i = pairs_ij[2 * p], j = pairs_ij[2 * p + 1];
        if (i < 0 || j < i || j >= m) return stx_fail(STX_ERR_INVALID, "pair %d: need 0 <= i <= j < m", p);
        pairs[p] = {i, j, n_iij_iji[3 * p], n_iij_iji[3 * p + 1], n_iij_iji[3 * p + 2]};
    }
    std::vector<char> sk(skip, skip + m);
    return exp_solve(m, pairs, sk, out_gains, dev, dev_acc);
}

}  // namespace

STX_EXPORT int stx_exposure_solve(int m, int npairs, const int* pairs_ij, const double* n_iij_iji, const unsigned char* skip,
                                  double* out_gains)
{
    return exp_solve_abi(nullptr, m, npairs, pairs_ij, n_iij_iji, skip, out_gains, nullptr);
}

STX_EXPORT int stx_exposure_solve_device(stx_ctx* ctx, int m, int npairs, const int* pairs_ij, const double* n_iij_iji,
                                         const unsigned char* skip, double* out_gains, double out_info[4])
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    double acc[3] = {0.0, 0.0, 0.0};
    if (out_info) out_info[0] = out_info[1] = out_info[2] = out_info[3] = 0.0;
    STX_TRY(exp_solve_abi(ctx, m, npairs, pairs_ij, n_iij_iji, skip, out_gains, acc));
    if (out_info) { out_info[0] = acc[0]; out_info[1] = acc[1]; out_info[2] = acc[2]; }
    return STX_OK;
}

STX_EXPORT int stx_lu_solve_device(stx_ctx* ctx, int n, const double* A, const double* b, double* x_out, double out_info[4])
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (n < 1 || !A || !b || !x_out) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (n > STX_LU_MAX_N)
        return stx_fail(STX_ERR_INVALID, "device LU: n = %d unknowns exceed the limit of %d (the dense fp64 matrix takes 8 n^2 bytes)", n,
                        STX_LU_MAX_N);
    std::vector<StxLuEntry> ent;
    for (int r = 0; r < n; r++) {
        for (int c = 0; c < n; c++)
            if (A[(size_t)r * n + c] != 0.0) ent.push_back({r, c, A[(size_t)r * n + c]});
        if (b[r] != 0.0) ent.push_back({r, n, b[r]});
    }
    double info[3] = {0.0, 0.0, 0.0};
    if (out_info) out_info[0] = out_info[1] = out_info[2] = out_info[3] = 0.0;
    STX_TRY(stx_lu_device(ctx, n, ent.data(), ent.size(), x_out, info));
    if (out_info) { out_info[0] = info[0]; out_info[1] = info[1]; out_info[2] = info[2]; }
    return STX_OK;
}

STX_EXPORT int stx_exposure_stats(stx_ctx* ctx, int kind, int n, const stx_buf* const* imgs, const stx_buf* const* masks,
                                  const int* corners_xy, int block_size, long long* inout_jobs, int* out_ab, long long* out_c,
                                  double* out_sums)
{
    if (!inout_jobs) return stx_fail(STX_ERR_INVALID, "inout_jobs is null");
    ExpPlan P;
    STX_TRY(exp_plan(kind, n, imgs, masks, corners_xy, block_size, true, P));
    const long long nj = (long long)P.jobs.size();
    if (!out_ab) { *inout_jobs = nj; return STX_OK; }
    if (*inout_jobs < nj || !out_c || !out_sums) return stx_fail(STX_ERR_INVALID, "output arrays hold %lld jobs, %lld needed", *inout_jobs, nj);
    STX_TRY(exp_check_ctx(ctx, P, imgs));
    STX_TRY(stx_set_device(ctx));
    STX_TRY(exp_sqrt_table(ctx));
    ExpRun X(ctx);
    std::vector<long long> oi;
    std::vector<double> od;
    STX_TRY(exp_stats(X, P, imgs, masks, oi, od, nullptr));
    const bool ch = kind_channels(kind);
    for (long long j = 0; j < nj; j++) {
        out_ab[2 * j] = P.ab[2 * j]; out_ab[2 * j + 1] = P.ab[2 * j + 1];
        out_c[j] = oi[7 * j];
        for (int k = 0; k < 6; k++) out_sums[6 * j + k] = ch ? (double)oi[7 * j + 1 + k] : (k < 2 ? od[2 * j + k] : 0.0);
    }
    *inout_jobs = nj;
    return STX_OK;
}

STX_EXPORT int stx_exposure_feed_ex(stx_ctx* ctx, int kind, int n, const stx_buf* const* imgs, const stx_buf* const* masks,
                                    const int* corners_xy, int block_size, int nr_feeds, int solver, double* out_gains,
                                    long long* inout_count, double out_info[8])
{
    if (solver == STX_EXPOSURE_SOLVER_DEFAULT) solver = exposure_solver_now();
    if (solver != STX_EXPOSURE_SOLVER_HOST && solver != STX_EXPOSURE_SOLVER_DEVICE) return stx_fail(STX_ERR_INVALID, "exposure solver %d", solver);
    if (!inout_count) return stx_fail(STX_ERR_INVALID, "inout_count is null");
    if (nr_feeds < 1) return stx_fail(STX_ERR_INVALID, "nr_feeds must be >= 1");
    ExpPlan P;
    STX_TRY(exp_plan(kind, n, imgs, masks, corners_xy, block_size, out_gains != nullptr, P));
    if (!out_gains) { *inout_count = P.out_count; return STX_OK; }
    if (*inout_count < P.out_count) return stx_fail(STX_ERR_INVALID, "out_gains holds %lld values, %lld needed", *inout_count, P.out_count);
    *inout_count = P.out_count;
    if (out_info) {
        for (int k = 0; k < 8; k++) out_info[k] = 0.0;
        out_info[0] = P.units; out_info[1] = (double)P.jobs.size(); out_info[4] = solver;
    }
    if (n == 0) return STX_OK;
    STX_TRY(exp_check_ctx(ctx, P, imgs));
    STX_TRY(stx_set_device(ctx));
    STX_TRY(exp_sqrt_table(ctx));
    const int m = P.units, planes = kind_channels(kind) ? 3 : 1;
    const bool blocks = kind_blocks(kind);
    std::vector<double> acc((size_t)planes * m, 1.0), g((size_t)planes * m, 1.0);
    std::vector<const stx_buf*> cur(imgs, imgs + n);
    ExpRun X(ctx);
    std::vector<StxBufRef>& scratch = X.scratch;
    double stats_ms = 0.0, host_ms = 0.0, dev_acc[3] = {0.0, 0.0, 0.0};
    stx_ctx* const solve_on = solver == STX_EXPOSURE_SOLVER_DEVICE ? ctx : nullptr;
    std::vector<long long> oi;
    std::vector<double> od;
    for (int feed = 0; feed < nr_feeds; feed++) {
        if (feed > 0) {
            if (scratch.empty()) {
                for (int i = 0; i < n; i++) {
                    scratch.emplace_back();
                    StxBufRef& s = scratch.back();
                    STX_TRY(stx_buf_new(ctx, imgs[i]->w, imgs[i]->h, 3, STX_U8, &s));
                    if (hipMemcpy2DAsync(s->ptr, s->stride, imgs[i]->ptr, imgs[i]->stride, 3 * (size_t)imgs[i]->w, imgs[i]->h,
                                         hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
                        return stx_fail(STX_ERR_HIP, "hipMemcpy2DAsync of an exposure scratch image failed");
                    cur[i] = s.get();
                }
            }
            if (!blocks) {  // one gain (BGR triple) per image: cv::multiply as GainCompensator::apply
                for (int i = 0; i < n; i++) {
                    float g3[3];
                    for (int c = 0; c < 3; c++) g3[c] = (float)g[(size_t)(planes == 3 ? c : 0) * m + i];
                    STX_TRY(stx_launch_gain_apply(ctx, scratch[i].get(), g3));
                }
            } else {
                std::vector<float> hg((size_t)m * planes);
                for (int u = 0; u < m; u++)
                    for (int c = 0; c < planes; c++) hg[(size_t)u * planes + c] = (float)g[(size_t)c * m + u];
                std::vector<StxExpBlockMul> tab(n);
                int maxpx = 0;
                for (int i = 0; i < n; i++) {
                    const ExpGrid& gr = P.grid[i];
                    tab[i] = {scratch[i]->ptr, (long long)scratch[i]->stride, scratch[i]->w, scratch[i]->h, gr.bw, gr.bh, gr.bpw,
                              nullptr, planes == 3};
                    maxpx = std::max(maxpx, scratch[i]->w * scratch[i]->h);
                }
                if (!X.d_bg) {
                    STX_TRY(stx_dev_alloc(ctx, hg.size() * sizeof(float), &X.d_bg));
                    STX_TRY(stx_dev_alloc(ctx, tab.size() * sizeof(StxExpBlockMul), &X.d_bt));
                }
                float* const d_bg = (float*)X.d_bg.get();
                StxExpBlockMul* const d_bt = (StxExpBlockMul*)X.d_bt.get();
                for (int i = 0; i < n; i++) tab[i].g = d_bg + (size_t)P.grid[i].first * planes;
                hipStreamSynchronize(ctx->stream);  // the previous feed's tables may still be read
                if (hipMemcpyAsync(d_bg, hg.data(), hg.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                    hipMemcpyAsync(d_bt, tab.data(), tab.size() * sizeof(StxExpBlockMul), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                    return stx_fail(STX_ERR_HIP, "exposure gain table upload failed");
                STX_TRY(stx_launch_exposure_block_mul(ctx, d_bt, n, maxpx));
                if (hipStreamSynchronize(ctx->stream) != hipSuccess) return stx_fail(STX_ERR_HIP, "exposure block multiply failed");
            }
        }
        STX_TRY(exp_stats(X, P, cur.data(), masks, oi, od, out_info ? &stats_ms : nullptr));
        const auto t0 = std::chrono::steady_clock::now();
        const int nj = (int)P.jobs.size();
        std::vector<char> skip(m, 1);
        for (int j = 0; j < nj; j++)
            if (oi[7 * (size_t)j] > 0 && P.ab[2 * j] != P.ab[2 * j + 1]) skip[P.ab[2 * j]] = skip[P.ab[2 * j + 1]] = 0;
        std::vector<PairStat> pairs(nj);
        for (int c = 0; c < planes; c++) {
            for (int j = 0; j < nj; j++) {
                const long long cnt = oi[7 * (size_t)j];
                const double nn = (double)std::max(1LL, cnt);
                double sa = 0.0, sb = 0.0;
                if (cnt > 0) {
                    sa = planes == 3 ? (double)oi[7 * (size_t)j + 1 + c] : od[2 * (size_t)j];
                    sb = planes == 3 ? (double)oi[7 * (size_t)j + 4 + c] : od[2 * (size_t)j + 1];
                }
                pairs[j] = {P.ab[2 * j], P.ab[2 * j + 1], nn, cnt > 0 ? sa / nn : 0.0, cnt > 0 ? sb / nn : 0.0};
            }
            STX_TRY(exp_solve(m, pairs, skip, g.data() + (size_t)c * m, solve_on, dev_acc));
        }
        for (size_t k = 0; k < acc.size(); k++) acc[k] = acc[k] * g[k];
        host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const auto t0 = std::chrono::steady_clock::now();
    double* o = out_gains;
    for (int i = 0; i < n; i++) {
        const ExpGrid& gr = P.grid[i];
        if (!blocks) {
            for (int c = 0; c < planes; c++) *o++ = acc[(size_t)c * m + gr.first];
            continue;
        }
        const int k = gr.bpw * gr.bph;
        std::vector<float> map((size_t)k * planes);
        for (int u = 0; u < k; u++)
            for (int c = 0; c < planes; c++) map[(size_t)u * planes + c] = (float)acc[(size_t)c * m + gr.first + u];
        filter_map(map, gr.bpw, gr.bph, planes);
        for (float v : map) *o++ = v;
    }
    host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (out_info) {
        out_info[2] = stats_ms; out_info[3] = host_ms;
        for (int k = 0; k < 3; k++) out_info[5 + k] = dev_acc[k];
    }
    return STX_OK;
}
