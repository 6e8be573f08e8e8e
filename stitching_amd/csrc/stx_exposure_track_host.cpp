// stx_exposure_track_host.cpp — host side of exposure-gain tracking on a known rig (kernels: stx_exposure_track.hip; contract:
// tests/numpy_exposure_track.py): the lattice geometry of the rectangles, the pair jobs and their tiles, the
// handle that keeps the V grids, and the measure / collect pair whose only host wait is the one on the PREVIOUS measure's event.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "stx_internal.h"

struct stx_exposure_track {
    stx_ctx* ctx = nullptr;
    int n = 0, stride = 0, ntiles = 0;
    std::vector<int> rects;          // x, y, w, h per image
    std::vector<int> ab;             // 2 per pair job
    std::vector<long long> self;     // c_ii per image
    long long grid_bytes = 0;
    double sample_bytes = 0.0;       // what one measure reads at most: two V bytes and two pixels per lattice point of a tile
    StxDevBlock d_geo, d_pix, d_tiles, d_grid, d_acc;  // d_acc: two slots of 8 accumulators per pair
    unsigned long long* h_acc = nullptr;               // page-locked, two slots as d_acc
    hipEvent_t ev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // per slot: before the launch, behind it, behind the copy
    int pending[2] = {0, 0}, npending = 0;  // the slots of the measures not yet collected, oldest first
    long long measures = 0;
    double last_ms = 0.0, last_wait_ms = 0.0;
    ~stx_exposure_track()
    {
        for (auto& slot : ev)
            for (hipEvent_t e : slot)
                if (e) hipEventDestroy(e);
        if (h_acc) hipHostFree(h_acc);
    }
};

namespace {

long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// the lattice indices l with x0 <= l s < x1: the first, and how many (0: none)
void lattice_range(long long x0, long long x1, int s, long long* first, long long* count)
{
    *first = -floor_div(-x0, s);
    *count = std::max(0ll, floor_div(x1 - 1, s) - *first + 1);
}

int check_image(const stx_exposure_track* t, const stx_buf* b, int i, int channels, const char* what)
{
    if (!b) return stx_fail(STX_ERR_INVALID, "exposure tracking: %s %d is null", what, i);
    if (b->ctx != t->ctx) return stx_fail(STX_ERR_INVALID, "exposure tracking: %s %d belongs to another context", what, i);
    if (b->elem != STX_U8 || b->c != channels) return stx_fail(STX_ERR_INVALID, "exposure tracking: %s %d must be u8x%d", what, i, channels);
    if (b->w != t->rects[4 * i + 2] || b->h != t->rects[4 * i + 3])
        return stx_fail(STX_ERR_INVALID, "exposure tracking: %s %d is %d x %d, its rectangle %d x %d", what, i, b->w, b->h, t->rects[4 * i + 2],
                        t->rects[4 * i + 3]);
    return STX_OK;
}

}  // namespace

STX_EXPORT int stx_exposure_track_create(stx_ctx* ctx, int n, const int* rects_xywh, const stx_buf* const* masks_u8, int stride,
                                         stx_exposure_track** out)
{
    if (!ctx || !out) return stx_fail(STX_ERR_INVALID, "exposure tracking: null argument");
    *out = nullptr;
    if (n < 1 || n > STX_TRACK_MAX_IMAGES) return stx_fail(STX_ERR_INVALID, "exposure tracking over %d images: 1 .. %d", n, STX_TRACK_MAX_IMAGES);
    if (stride < 1 || stride > STX_TRACK_MAX_STRIDE) return stx_fail(STX_ERR_INVALID, "exposure tracking: stride %d outside 1 .. %d", stride, STX_TRACK_MAX_STRIDE);
    if (!rects_xywh || !masks_u8) return stx_fail(STX_ERR_INVALID, "exposure tracking: null argument");
    std::unique_ptr<stx_exposure_track> t(new stx_exposure_track);
    t->ctx = ctx; t->n = n; t->stride = stride;
    t->rects.assign(rects_xywh, rects_xywh + 4 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const int* r = &t->rects[4 * i];
        if (r[2] < 1 || r[3] < 1 || (long long)r[0] + r[2] > (1ll << 30) || (long long)r[1] + r[3] > (1ll << 30) || r[0] < -(1 << 30) || r[1] < -(1 << 30))
            return stx_fail(STX_ERR_INVALID, "exposure tracking: rectangle %d (%d, %d, %d x %d) is empty or out of range", i, r[0], r[1], r[2], r[3]);
        STX_TRY(check_image(t.get(), masks_u8[i], i, 1, "mask"));
    }
    // lattice geometry of every image
    std::vector<StxTrackGeo> geo(n);
    long long max_points = 0;
    for (int i = 0; i < n; i++) {
        const int* r = &t->rects[4 * i];
        long long lx0, nx, ly0, ny;
        lattice_range(r[0], (long long)r[0] + r[2], stride, &lx0, &nx);
        lattice_range(r[1], (long long)r[1] + r[3], stride, &ly0, &ny);
        geo[i] = {r[0], r[1], (int)lx0, (int)ly0, (int)nx, (int)ny, t->grid_bytes};
        t->grid_bytes += nx * ny;
        max_points = std::max(max_points, nx * ny);
    }
    // pair jobs (a < b, rectangles intersect) in lexicographic order, and the tiles of their lattice points
    std::vector<StxTrackTile> tiles;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) {
            const int* ra = &t->rects[4 * a];
            const int* rb = &t->rects[4 * b];
            const long long x0 = std::max(ra[0], rb[0]), x1 = std::min((long long)ra[0] + ra[2], (long long)rb[0] + rb[2]);
            const long long y0 = std::max(ra[1], rb[1]), y1 = std::min((long long)ra[1] + ra[3], (long long)rb[1] + rb[3]);
            if (!(x0 < x1 && y0 < y1)) continue;
            const int pair = (int)(t->ab.size() / 2);
            t->ab.push_back(a); t->ab.push_back(b);
            long long lx0, nx, ly0, ny;
            lattice_range(x0, x1, stride, &lx0, &nx);
            lattice_range(y0, y1, stride, &ly0, &ny);
            if (nx == 0 || ny == 0) continue;  // a strip narrower than the stride: a pair without samples
            const long long tiles_of_pair = ((nx + STX_TRACK_TILE - 1) / STX_TRACK_TILE) * ((ny + STX_TRACK_TILE - 1) / STX_TRACK_TILE);
            if ((long long)tiles.size() + tiles_of_pair > STX_TRACK_MAX_TILES)
                return stx_fail(STX_ERR_INVALID, "exposure tracking: more than %d tile jobs at stride %d: take a larger stride", STX_TRACK_MAX_TILES, stride);
            for (long long ty = 0; ty < ny; ty += STX_TRACK_TILE)
                for (long long tx = 0; tx < nx; tx += STX_TRACK_TILE) {
                    StxTrackTile T = {a, b, pair, (int)(lx0 + tx), (int)(ly0 + ty), (int)std::min<long long>(STX_TRACK_TILE, nx - tx),
                                      (int)std::min<long long>(STX_TRACK_TILE, ny - ty), 0};
                    // inside both images' grids (the kernel reads them unchecked)
                    for (int i : {a, b})
                        if (T.lx < geo[i].lx0 || T.ly < geo[i].ly0 || T.lx + T.nx > geo[i].lx0 + geo[i].nx || T.ly + T.ny > geo[i].ly0 + geo[i].ny)
                            return stx_fail(STX_ERR_INVALID, "internal: exposure tracking tile outside its images");
                    tiles.push_back(T);
                    t->sample_bytes += 8.0 * T.nx * T.ny;
                }
        }
    t->ntiles = (int)tiles.size();
    const size_t npairs = t->ab.size() / 2;
    // everything is checked: the device from here on
    STX_TRY(stx_set_device(ctx));
    StxDevBlock d_masks, d_self;
    std::vector<StxTrackPix> mk(n);
    for (int i = 0; i < n; i++) mk[i] = {masks_u8[i]->ptr, (long long)masks_u8[i]->stride};
    STX_TRY(stx_dev_alloc(ctx, sizeof(StxTrackGeo) * n, &t->d_geo));
    STX_TRY(stx_dev_alloc(ctx, sizeof(StxTrackPix) * n, &t->d_pix));
    STX_TRY(stx_dev_alloc(ctx, (size_t)std::max(1ll, t->grid_bytes), &t->d_grid));
    STX_TRY(stx_dev_alloc(ctx, sizeof(StxTrackTile) * std::max<size_t>(1, tiles.size()), &t->d_tiles));
    STX_TRY(stx_dev_alloc(ctx, sizeof(unsigned long long) * 16 * std::max<size_t>(1, npairs), &t->d_acc));
    STX_TRY(stx_dev_alloc(ctx, sizeof(StxTrackPix) * n, &d_masks));
    STX_TRY(stx_dev_alloc(ctx, sizeof(unsigned long long) * n, &d_self));
    STX_HIP(hipHostMalloc((void**)&t->h_acc, sizeof(unsigned long long) * 16 * std::max<size_t>(1, npairs), hipHostMallocDefault));
    for (auto& slot : t->ev)
        for (hipEvent_t& e : slot) STX_HIP(hipEventCreate(&e));
    std::vector<unsigned long long> self(n, 0);
    hipError_t e = hipMemcpyAsync(t->d_geo.get(), geo.data(), sizeof(StxTrackGeo) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_masks.get(), mk.data(), sizeof(StxTrackPix) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && !tiles.empty())
        e = hipMemcpyAsync(t->d_tiles.get(), tiles.data(), sizeof(StxTrackTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_self.get(), 0, sizeof(unsigned long long) * n, ctx->stream);
    int rc = STX_OK;
    if (e == hipSuccess)
        rc = stx_launch_exposure_track_grid(ctx, n, (const StxTrackGeo*)t->d_geo.get(), (const StxTrackPix*)d_masks.get(), stride, max_points,
                                            (uint8_t*)t->d_grid.get(), (unsigned long long*)d_self.get());
    if (e == hipSuccess && rc == STX_OK)
        e = hipMemcpyAsync(self.data(), d_self.get(), sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, ctx->stream);
    // the one wait of a rig: the host tables above and the masks are read until here, and c_ii comes back
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc != STX_OK) return rc;
    if (e != hipSuccess || es != hipSuccess)
        return stx_fail(STX_ERR_HIP, "exposure tracking: building the grids failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
    t->self.assign(self.begin(), self.end());
    *out = t.release();
    return STX_OK;
}

STX_EXPORT int stx_exposure_track_pairs(stx_exposure_track* t, int* inout_count, int* out_ab, long long* out_self_counts)
{
    if (!t || !inout_count) return stx_fail(STX_ERR_INVALID, "exposure tracking: null argument");
    const int np = (int)(t->ab.size() / 2);
    if (!out_ab && !out_self_counts) { *inout_count = np; return STX_OK; }
    if (*inout_count < np || (np > 0 && !out_ab) || !out_self_counts)
        return stx_fail(STX_ERR_INVALID, "exposure tracking: the output arrays hold %d pairs, %d needed", *inout_count, np);
    for (size_t k = 0; k < t->ab.size(); k++) out_ab[k] = t->ab[k];
    for (int i = 0; i < t->n; i++) out_self_counts[i] = t->self[i];
    *inout_count = np;
    return STX_OK;
}

STX_EXPORT int stx_exposure_track_measure(stx_exposure_track* t, const stx_buf* const* imgs_u8x3)
{
    if (!t || !imgs_u8x3) return stx_fail(STX_ERR_INVALID, "exposure tracking: null argument");
    for (int i = 0; i < t->n; i++) STX_TRY(check_image(t, imgs_u8x3[i], i, 3, "image"));
    if (t->npending >= 2) return stx_fail(STX_ERR_INVALID, "exposure tracking: two measures are pending: collect one first");
    stx_ctx* ctx = t->ctx;
    STX_TRY(stx_set_device(ctx));
    const int slot = (int)(t->measures % 2);
    const size_t npairs = t->ab.size() / 2;
    std::vector<StxTrackPix> px(t->n);
    for (int i = 0; i < t->n; i++) px[i] = {imgs_u8x3[i]->ptr, (long long)imgs_u8x3[i]->stride};
    unsigned long long* d_acc = (unsigned long long*)t->d_acc.get() + 8 * npairs * slot;
    if (t->ntiles > 0) STX_TRY(stx_stage_upload(ctx, t->d_pix.get(), px.data(), sizeof(StxTrackPix) * t->n));
    if (npairs > 0) STX_HIP(hipMemsetAsync(d_acc, 0, sizeof(unsigned long long) * 8 * npairs, ctx->stream));
    STX_HIP(hipEventRecord(t->ev[slot][0], ctx->stream));
    STX_TRY(stx_launch_exposure_track_stats(ctx, (const StxTrackGeo*)t->d_geo.get(), (const StxTrackPix*)t->d_pix.get(),
                                            (const StxTrackTile*)t->d_tiles.get(), t->ntiles, t->stride, (const uint8_t*)t->d_grid.get(), d_acc,
                                            t->sample_bytes));
    STX_HIP(hipEventRecord(t->ev[slot][1], ctx->stream));
    if (npairs > 0)
        STX_HIP(hipMemcpyAsync(t->h_acc + 8 * npairs * slot, d_acc, sizeof(unsigned long long) * 8 * npairs, hipMemcpyDeviceToHost, ctx->stream));
    STX_HIP(hipEventRecord(t->ev[slot][2], ctx->stream));
    t->pending[t->npending++] = slot;
    t->measures++;
    return STX_OK;
}

STX_EXPORT int stx_exposure_track_collect(stx_exposure_track* t, long long* out_stats)
{
    if (!t) return stx_fail(STX_ERR_INVALID, "exposure tracking: null argument");
    if (t->npending == 0) return stx_fail(STX_ERR_INVALID, "exposure tracking: no measure is pending");
    const size_t npairs = t->ab.size() / 2;
    if (npairs > 0 && !out_stats) return stx_fail(STX_ERR_INVALID, "exposure tracking: out_stats is null");
    STX_TRY(stx_set_device(t->ctx));
    const int slot = t->pending[0];
    const auto t0 = std::chrono::steady_clock::now();
    STX_HIP(hipEventSynchronize(t->ev[slot][2]));
    t->last_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t->pending[0] = t->pending[1];
    t->npending--;
    float ms = 0.f;
    STX_HIP(hipEventElapsedTime(&ms, t->ev[slot][0], t->ev[slot][1]));
    t->last_ms = ms;
    static_assert(sizeof(long long) == sizeof(unsigned long long), "the accumulators are read as signed");
    if (npairs > 0) memcpy(out_stats, t->h_acc + 8 * npairs * slot, sizeof(long long) * 8 * npairs);
    return STX_OK;
}

STX_EXPORT int stx_exposure_track_info(stx_exposure_track* t, double out_info[6])
{
    if (!t || !out_info) return stx_fail(STX_ERR_INVALID, "exposure tracking: null argument");
    out_info[0] = (double)(t->ab.size() / 2); out_info[1] = t->ntiles; out_info[2] = (double)t->grid_bytes;
    out_info[3] = t->last_ms; out_info[4] = t->last_wait_ms; out_info[5] = (double)t->measures;
    return STX_OK;
}

STX_EXPORT int stx_exposure_track_free(stx_exposure_track* t)
{
    if (!t) return STX_OK;
    if (t->ctx && stx_set_device(t->ctx) == STX_OK) hipStreamSynchronize(t->ctx->stream);  // a measure may still read the grids
    delete t;  // the events and the page-locked block go; the device blocks go back to the context's allocator
    return STX_OK;
}

STX_EXPORT int stx_gain_maps_scale(stx_ctx* ctx, int n, const stx_buf* const* maps_f32, const float* factors, int planes, stx_buf** outs)
{
    if (!ctx || !maps_f32 || !factors || !outs) return stx_fail(STX_ERR_INVALID, "gain map scaling: null argument");
    if (n < 1 || n > STX_TRACK_MAX_IMAGES) return stx_fail(STX_ERR_INVALID, "gain map scaling of %d maps: 1 .. %d", n, STX_TRACK_MAX_IMAGES);
    if (planes != 1 && planes != 3) return stx_fail(STX_ERR_INVALID, "gain map scaling: %d factor planes: 1 or 3", planes);
    for (int i = 0; i < n; i++) {
        const stx_buf* m = maps_f32[i];
        if (!m) return stx_fail(STX_ERR_INVALID, "gain map scaling: map %d is null", i);
        if (m->ctx != ctx) return stx_fail(STX_ERR_INVALID, "gain map scaling: map %d belongs to another context", i);
        if (m->elem != STX_F32 || (m->c != 1 && m->c != 3)) return stx_fail(STX_ERR_INVALID, "gain map scaling: map %d must be f32x1 or f32x3", i);
        if ((long long)m->w * m->h * 3 >= (1ll << 31)) return stx_fail(STX_ERR_INVALID, "gain map scaling: map %d is too large", i);
    }
    STX_TRY(stx_set_device(ctx));
    std::vector<StxBufRef> made(n);
    std::vector<StxScaleMap> tab(n);
    for (int i = 0; i < n; i++) {
        const stx_buf* m = maps_f32[i];
        const int dc = std::max(m->c, planes);
        STX_TRY(stx_buf_new(ctx, m->w, m->h, dc, STX_F32, &made[i]));
        StxScaleMap& S = tab[i];
        S.src = (const float*)m->ptr; S.dst = (float*)made[i]->ptr;
        S.sstride = (long long)(m->stride / sizeof(float)); S.dstride = (long long)(made[i]->stride / sizeof(float));
        S.w = m->w; S.h = m->h; S.sc = m->c; S.dc = dc; S.pad_ = 0;
        for (int c = 0; c < 3; c++) S.f[c] = factors[(size_t)i * planes + (planes == 3 ? c : 0)];
    }
    STX_TRY(stx_launch_gain_maps_scale(ctx, tab.data(), n));
    for (int i = 0; i < n; i++) outs[i] = made[i].release();
    return STX_OK;
}
