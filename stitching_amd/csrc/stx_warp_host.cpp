// stx_warp_host.cpp — host side of the Warper entry points: ProjectorBase::setCameraParams, ROI finalisation and its cache, the warp
// launches.  Compiled with -ffp-contract=off: the fp32 host arithmetic below restates OpenCV's baseline (non-FMA) evaluation order.
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "stx_internal.h"

// ---------------------------------------------------------------------------------------------
// projector: ProjectorBase::setCameraParams, AffineWarper::getRTfromHomogeneous
// ---------------------------------------------------------------------------------------------
static void inv3x3_f32(const float* m, float* o)
{
    // cv::invert for a 3x3 CV_32F matrix: cofactors and determinant in double, cast to float
    auto M = [&](int i, int j) { return (double)m[i * 3 + j]; };
    double d = m[0] * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) - m[1] * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) +
               m[2] * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0));
    if (d == 0.) {
        for (int i = 0; i < 9; i++) o[i] = 0.f;
        return;
    }
    d = 1. / d;
    o[0] = (float)((M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d);
    o[1] = (float)((M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d);
    o[2] = (float)((M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d);
    o[3] = (float)((M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d);
    o[4] = (float)((M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d);
    o[5] = (float)((M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d);
    o[6] = (float)((M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d);
    o[7] = (float)((M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d);
    o[8] = (float)((M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d);
}

static void mul3x3_f32(const float* a, const float* b, float* d)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float t = a[i * 3] * b[j];
            t = t + a[i * 3 + 1] * b[3 + j];
            t = t + a[i * 3 + 2] * b[6 + j];
            d[i * 3 + j] = t;
        }
}

int stx_make_projector(int type, float scale, const float* K, const float* R, StxProjector* p)
{
    if (type < STX_WARP_PLANE || type >= STX_WARP_TYPE_COUNT)
        return stx_fail(STX_ERR_UNSUPPORTED, "warper type id %d is not implemented by this back end", type);
    if (!K || !R) return stx_fail(STX_ERR_INVALID, "K and R must be 3x3 fp32");
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i]) || !std::isfinite(R[i])) return stx_fail(STX_ERR_INVALID, "K/R contain non-finite values");
    p->type = type;
    p->scale = scale;
    p->trig = trig_mode_now();
    p->remap = remap_mode_now();
    // PyRotationWarper's constructor: "compressedPlaneA2B1" -> CompressedRectilinearWarper(2.0f, 1.0f), "...A1.5B1" -> (1.5f, 1.0f), ...
    static const struct { int family; float a; } kTypes[STX_WARP_TYPE_COUNT] = {
        {STX_F_PLANE, 1.f}, {STX_F_PLANE, 1.f}, {STX_F_CYLINDRICAL, 1.f}, {STX_F_SPHERICAL, 1.f}, {STX_F_FISHEYE, 1.f},
        {STX_F_STEREOGRAPHIC, 1.f}, {STX_F_CRECT, 2.0f}, {STX_F_CRECT, 1.5f}, {STX_F_CRECT_PORTRAIT, 2.0f},
        {STX_F_CRECT_PORTRAIT, 1.5f}, {STX_F_PANINI, 2.0f}, {STX_F_PANINI, 1.5f}, {STX_F_PANINI_PORTRAIT, 2.0f},
        {STX_F_PANINI_PORTRAIT, 1.5f}, {STX_F_MERCATOR, 1.f}, {STX_F_TRANSVERSE_MERCATOR, 1.f}};
    p->family = kTypes[type].family;
    p->a = kTypes[type].a;
    p->b = 1.0f;
    float Rm[9], T[3] = {0.f, 0.f, 0.f};
    if (type == STX_WARP_AFFINE) {
        // R' = (H with H[0,2] = H[1,2] = 0)^T ; T' = -(R' * (H[0,2], H[1,2], 0)); the caller's scale is kept
        // (cv::AffineWarper::create(scale) -> detail::AffineWarper(scale) : PlaneWarper(scale))
        float H[9];
        memcpy(H, R, sizeof(H));
        const float t0 = H[2], t1 = H[5];
        H[2] = 0.f;
        H[5] = 0.f;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rm[i * 3 + j] = H[j * 3 + i];
        for (int i = 0; i < 3; i++) {
            float v = Rm[i * 3] * t0;
            v = v + Rm[i * 3 + 1] * t1;
            v = v + Rm[i * 3 + 2] * 0.f;
            T[i] = v * -1.f;
        }
    } else {
        memcpy(Rm, R, sizeof(Rm));
    }
    memcpy(p->k, K, sizeof(p->k));
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) p->rinv[i * 3 + j] = Rm[j * 3 + i];
    float kinv[9];
    inv3x3_f32(K, kinv);
    mul3x3_f32(Rm, kinv, p->r_kinv);
    mul3x3_f32(K, p->rinv, p->k_rinv);
    p->t[0] = T[0]; p->t[1] = T[1]; p->t[2] = T[2];
    return STX_OK;
}

// (int)float as x86 cvttss2si
static int trunc_i32(float v)
{
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)v;
}

// PlaneProjector::mapForward for the 4 corners (PlaneWarper::detectResultRoi)
static void plane_forward(const StxProjector& p, float x, float y, float& u, float& v)
{
    const float* rk = p.r_kinv;
    float x_ = rk[0] * x;
    x_ = x_ + rk[1] * y;
    x_ = x_ + rk[2];
    float y_ = rk[3] * x;
    y_ = y_ + rk[4] * y;
    y_ = y_ + rk[5];
    float z_ = rk[6] * x;
    z_ = z_ + rk[7] * y;
    z_ = z_ + rk[8];
    float q = x_ / z_;
    q = q * (1 - p.t[2]);
    x_ = p.t[0] + q;
    q = y_ / z_;
    q = q * (1 - p.t[2]);
    y_ = p.t[1] + q;
    u = p.scale * x_;
    v = p.scale * y_;
}

static void finish_roi(const StxProjector& p, int w, int h, const float* mm, int* out_xywh)
{
    int tlx = trunc_i32(mm[0]), tly = trunc_i32(mm[1]), brx = trunc_i32(mm[2]), bry = trunc_i32(mm[3]);
    if (p.type == STX_WARP_SPHERICAL) {
        // SphericalWarper::detectResultRoi: include the poles when they project inside the image
        float tl_uf = (float)tlx, tl_vf = (float)tly, br_uf = (float)brx, br_vf = (float)bry;
        float x = p.rinv[1], y = p.rinv[4], z = p.rinv[7];
        if (y > 0.f) {
            float a = p.k[0] * x;
            a = a + p.k[1] * y;
            float x_ = a / z + p.k[2];
            float y_ = p.k[4] * y / z + p.k[5];
            if (x_ > 0.f && x_ < w && y_ > 0.f && y_ < h) {
                float pv = static_cast<float>(3.14159265358979323846 * p.scale);
                tl_uf = std::min(tl_uf, 0.f); tl_vf = std::min(tl_vf, pv);
                br_uf = std::max(br_uf, 0.f); br_vf = std::max(br_vf, pv);
            }
        }
        y = -p.rinv[4];
        if (y > 0.f) {
            float a = p.k[0] * x;
            a = a + p.k[1] * y;
            float x_ = a / z + p.k[2];
            float y_ = p.k[4] * y / z + p.k[5];
            if (x_ > 0.f && x_ < w && y_ > 0.f && y_ < h) {
                tl_uf = std::min(tl_uf, 0.f); tl_vf = std::min(tl_vf, 0.f);
                br_uf = std::max(br_uf, 0.f); br_vf = std::max(br_vf, 0.f);
            }
        }
        tlx = trunc_i32(tl_uf); tly = trunc_i32(tl_vf); brx = trunc_i32(br_uf); bry = trunc_i32(br_vf);
    }
    out_xywh[0] = tlx; out_xywh[1] = tly;
    out_xywh[2] = brx - tlx + 1; out_xywh[3] = bry - tly + 1;
}

static int rois_impl(stx_ctx* ctx, int n, const StxProjector* projs, const int* sizes_wh, int* out_xywh)
{
    std::vector<float> mm(4 * (size_t)n);
    std::vector<int> dev_idx;
    for (int i = 0; i < n; i++) {
        const int w = sizes_wh[2 * i], h = sizes_wh[2 * i + 1];
        if (w <= 0 || h <= 0) return stx_fail(STX_ERR_INVALID, "image size %dx%d", w, h);
        if (projs[i].type == STX_WARP_PLANE || projs[i].type == STX_WARP_AFFINE) {
            float mn_u = std::numeric_limits<float>::max(), mn_v = mn_u, mx_u = -mn_u, mx_v = -mn_u, u, v;
            const float xs[2] = {0.f, (float)(w - 1)}, ys[2] = {0.f, (float)(h - 1)};
            for (int a = 0; a < 2; a++)
                for (int b = 0; b < 2; b++) {
                    plane_forward(projs[i], xs[a], ys[b], u, v);
                    mn_u = std::min(mn_u, u); mn_v = std::min(mn_v, v);
                    mx_u = std::max(mx_u, u); mx_v = std::max(mx_v, v);
                }
            mm[4 * i] = mn_u; mm[4 * i + 1] = mn_v; mm[4 * i + 2] = mx_u; mm[4 * i + 3] = mx_v;
        } else {
            dev_idx.push_back(i);
        }
    }
    if (!dev_idx.empty()) {
        const int m = (int)dev_idx.size();
        std::vector<StxProjector> dp(m);
        std::vector<int> dsz(2 * (size_t)m);
        std::vector<float> dmm(4 * (size_t)m);
        for (int j = 0; j < m; j++) {
            dp[j] = projs[dev_idx[j]];
            dsz[2 * j] = sizes_wh[2 * dev_idx[j]];
            dsz[2 * j + 1] = sizes_wh[2 * dev_idx[j] + 1];
        }
        STX_TRY(stx_launch_roi_minmax(ctx, m, dp.data(), dsz.data(), dmm.data()));
        for (int j = 0; j < m; j++) memcpy(&mm[4 * dev_idx[j]], &dmm[4 * j], 16);
    }
    for (int i = 0; i < n; i++) finish_roi(projs[i], sizes_wh[2 * i], sizes_wh[2 * i + 1], &mm[4 * i], out_xywh + 4 * i);
    return STX_OK;
}

// ROI cache: the reference recomputes detectResultRoi inside every warp()/warpRoi() call
// (stitching/warper.py:44,59,80 build three warpers per image); we compute it once per camera.
struct RoiKey {
    int type, w, h, trig;
    float scale, K[9], R[9];
    bool operator<(const RoiKey& o) const { return memcmp(this, &o, sizeof(RoiKey)) < 0; }
};
static thread_local std::map<RoiKey, std::array<int, 4>>* g_roi_cache = nullptr;

static RoiKey make_key(int type, float scale, const float* K, const float* R, int w, int h)
{
    RoiKey k;
    memset(&k, 0, sizeof(k));
    k.type = type; k.w = w; k.h = h; k.scale = scale;
    k.trig = trig_mode_now();  // the forward maps of the per-pixel projector families call sinf / cosf
    memcpy(k.K, K, 36);
    memcpy(k.R, R, 36);
    return k;
}

static bool roi_cache_find(const RoiKey& key, int* out_xywh)
{
    if (!g_roi_cache) return false;
    auto it = g_roi_cache->find(key);
    if (it == g_roi_cache->end()) return false;
    memcpy(out_xywh, it->second.data(), 16);
    return true;
}

static void roi_cache_insert(const RoiKey& key, const int* xywh)
{
    if (!g_roi_cache) g_roi_cache = new std::map<RoiKey, std::array<int, 4>>();
    if (g_roi_cache->size() > 8192) g_roi_cache->clear();
    (*g_roi_cache)[key] = {xywh[0], xywh[1], xywh[2], xywh[3]};
}

// ROIs for n projectors: cached ones as they are where use_cache allows, all missing ones in ONE device pass (one synchronisation);
// what was computed enters the cache either way
static int rois_cached(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s, const StxProjector* ps,
                       const int* sizes_wh, bool use_cache, int* out_xywh)
{
    std::vector<RoiKey> keys(n);
    std::vector<int> miss;
    for (int i = 0; i < n; i++) {
        keys[i] = make_key(type, scale, K9s + 9 * i, R9s + 9 * i, sizes_wh[2 * i], sizes_wh[2 * i + 1]);
        if (!use_cache || !roi_cache_find(keys[i], out_xywh + 4 * i)) miss.push_back(i);
    }
    if (miss.empty()) return STX_OK;
    const int m = (int)miss.size();
    std::vector<StxProjector> mp(m);
    std::vector<int> msz(2 * (size_t)m), mroi(4 * (size_t)m);
    for (int j = 0; j < m; j++) { mp[j] = ps[miss[j]]; msz[2 * j] = sizes_wh[2 * miss[j]]; msz[2 * j + 1] = sizes_wh[2 * miss[j] + 1]; }
    STX_TRY(rois_impl(ctx, m, mp.data(), msz.data(), mroi.data()));
    for (int j = 0; j < m; j++) {
        memcpy(out_xywh + 4 * miss[j], &mroi[4 * j], 16);
        roi_cache_insert(keys[miss[j]], &mroi[4 * j]);
    }
    return STX_OK;
}

STX_EXPORT int stx_warp_roi(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], int w, int h,
                            int out_xywh[4])
{
    if (!ctx || !out_xywh) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    StxProjector p;
    STX_TRY(stx_make_projector(type, scale, K, R, &p));
    if (w <= 0 || h <= 0) return stx_fail(STX_ERR_INVALID, "image size %dx%d", w, h);
    const int sz[2] = {w, h};
    return rois_cached(ctx, type, scale, 1, K, R, &p, sz, true, out_xywh);
}

STX_EXPORT int stx_warp_rois(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s,
                             const int* sizes_wh, int* out_xywh)
{
    if (!ctx || !K9s || !R9s || !sizes_wh || !out_xywh || n < 0) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (n == 0) return STX_OK;
    STX_TRY(stx_set_device(ctx));
    std::vector<StxProjector> ps(n);
    for (int i = 0; i < n; i++) STX_TRY(stx_make_projector(type, scale, K9s + 9 * i, R9s + 9 * i, &ps[i]));
    return rois_cached(ctx, type, scale, n, K9s, R9s, ps.data(), sizes_wh, false, out_xywh);  // always computed: the call IS the ROI pass
}

static int check_warp_rect(const int* r)
{
    if (r[2] <= 0 || r[3] <= 0 || (long long)r[2] * r[3] > (1ll << 33))
        return stx_fail(STX_ERR_INVALID, "degenerate warp roi %dx%d (camera parameters?)", r[2], r[3]);
    return STX_OK;
}

// the launch of one image: destination rectangle `rect` of projector p; src may be null (mask only: sw x sh is all that is read of it),
// dimg / dmask likewise
static StxWarpLaunch warp_launch(const StxProjector& p, const int* rect, const stx_buf* src, int sw, int sh, const stx_buf* dimg,
                                 const stx_buf* dmask)
{
    StxWarpLaunch L;
    L.proj = p;
    L.tlx = rect[0]; L.tly = rect[1]; L.dw = rect[2]; L.dh = rect[3];
    L.src = src ? src->ptr : nullptr;
    L.sw = sw; L.sh = sh;
    L.sstride = src ? src->stride : 0;
    L.src_channels = src ? src->c : 0;
    L.nearest_src = 0;
    // the validity mask the source carries (stx_buf_with_validity) is honoured where a mask is written
    if (src && src->validity && dmask) { L.vsrc = src->validity->ptr; L.vstride = src->validity->stride; }
    L.dimg = dimg ? dimg->ptr : nullptr; L.dimg_stride = dimg ? dimg->stride : 0;
    L.dmask = dmask ? dmask->ptr : nullptr; L.dmask_stride = dmask ? dmask->stride : 0;
    return L;
}

static int warp_impl(stx_ctx* ctx, int type, float scale, const float* K, const float* R, const stx_buf* src, int sw,
                     int sh, bool want_img, bool want_mask, bool nearest_src, stx_buf** out_img, stx_buf** out_mask,
                     int* out_xywh)
{
    StxProjector p;
    STX_TRY(stx_make_projector(type, scale, K, R, &p));
    int roi[4];
    const int sz[2] = {sw, sh};
    STX_TRY(rois_cached(ctx, type, scale, 1, K, R, &p, sz, true, roi));
    STX_TRY(check_warp_rect(roi));
    StxBufRef bi, bm;
    if (want_img) STX_TRY(stx_buf_new(ctx, roi[2], roi[3], nearest_src ? 1 : 3, STX_U8, &bi));
    if (want_mask) STX_TRY(stx_buf_new(ctx, roi[2], roi[3], 1, STX_U8, &bm));
    // generic INTER_NEAREST warp of a u8x1 source: the "mask" path writes the image
    StxWarpLaunch L = nearest_src ? warp_launch(p, roi, src, sw, sh, nullptr, bi.get()) : warp_launch(p, roi, src, sw, sh, bi.get(), bm.get());
    L.nearest_src = nearest_src ? 1 : 0;
    STX_TRY(stx_launch_warp(ctx, L));
    // remapNearest of a 255-filled source with a constant-0 border; of a validity mask: binary when that is
    if (bm) bm->mask_binary = L.vsrc ? src->validity->mask_binary : 1;
    if (out_img) *out_img = bi.release();
    if (out_mask) *out_mask = bm.release();
    if (out_xywh) memcpy(out_xywh, roi, 16);
    return STX_OK;
}

STX_EXPORT int stx_warp(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], const stx_buf* src,
                        int interp, int border, stx_buf** out, int out_tl[2])
{
    if (!ctx || !src || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    if (src->elem != STX_U8) return stx_fail(STX_ERR_INVALID, "warp source must be 8-bit");
    int roi[4];
    if (interp == STX_INTER_LINEAR && border == STX_BORDER_REFLECT) {
        if (src->c != 3) return stx_fail(STX_ERR_UNSUPPORTED, "INTER_LINEAR warp needs a 3-channel u8 image");
        STX_TRY(warp_impl(ctx, type, scale, K, R, src, src->w, src->h, true, false, false, out, nullptr, roi));
    } else if (interp == STX_INTER_NEAREST && border == STX_BORDER_CONSTANT) {
        if (src->c != 1) return stx_fail(STX_ERR_UNSUPPORTED, "INTER_NEAREST warp needs a 1-channel u8 mask");
        STX_TRY(warp_impl(ctx, type, scale, K, R, src, src->w, src->h, true, false, true, out, nullptr, roi));
    } else {
        return stx_fail(STX_ERR_UNSUPPORTED,
                        "only (INTER_LINEAR, BORDER_REFLECT) and (INTER_NEAREST, BORDER_CONSTANT) are on the path "
                        "(stitching/warper.py:49-50,65-66)");
    }
    if (out_tl) { out_tl[0] = roi[0]; out_tl[1] = roi[1]; }
    return STX_OK;
}

// The tables of one batched call (include/stitching_amd.h: stx_warp_batch, `tables`): the caller's handle, or a fresh one that becomes
// the caller's when the call succeeds and is given back when it fails — the handle of a failed call stays empty.
struct WarpTablesSlot {
    stx_warp_tables** slot;
    std::unique_ptr<stx_warp_tables> fresh;
    WarpTablesSlot(stx_ctx* ctx, stx_warp_tables** slot_) : slot(slot_)
    {
        if (slot && !*slot) {
            fresh.reset(new stx_warp_tables());
            fresh->ctx = ctx;
        }
    }
    ~WarpTablesSlot()
    {
        if (fresh && fresh->block) { stx_set_device(fresh->ctx); stx_dev_free(fresh->ctx, fresh->block); }
    }
    stx_warp_tables* get() const { return fresh ? fresh.get() : (slot ? *slot : nullptr); }
    int keep()
    {
        if (fresh) *slot = fresh.release();
        return STX_OK;
    }
};

// rects_xywh: null -> the destination rectangle of image i is its ROI (found here, cached); else the caller's rectangle in warp
// coordinates (any sub-rectangle of the ROI gives exactly the ROI warp's pixels there: every pixel is mapped on its own)
STX_EXPORT int stx_warp_batch(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s,
                              const stx_buf* const* srcs, const int* rects_xywh, const stx_buf* const* gain_maps, const int* gain_flags,
                              int flags, stx_buf** out_imgs, stx_buf** out_masks, int* out_xywh, stx_warp_tables** tables)
{
    const bool fresh_rois = (flags & STX_WARP_FRESH_ROIS) != 0;
    if (!ctx || !K9s || !R9s || !srcs || n < 0) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (!out_imgs && !out_masks) return stx_fail(STX_ERR_INVALID, "nothing requested: out_imgs and out_masks are both null");
    if (gain_maps && !out_imgs) return stx_fail(STX_ERR_INVALID, "gains without images: gain_maps needs out_imgs");
    if (flags & ~STX_WARP_FRESH_ROIS) return stx_fail(STX_ERR_INVALID, "unknown flags 0x%x", flags & ~STX_WARP_FRESH_ROIS);
    if (fresh_rois && !out_xywh) return stx_fail(STX_ERR_INVALID, "STX_WARP_FRESH_ROIS needs out_xywh: the ROIs of the call are its result");
    if (fresh_rois && rects_xywh) return stx_fail(STX_ERR_INVALID, "STX_WARP_FRESH_ROIS with rects_xywh: given rectangles need no ROI pass");
    if (tables && !rects_xywh && !fresh_rois)
        return stx_fail(STX_ERR_INVALID, "tables needs rects_xywh or STX_WARP_FRESH_ROIS: kept tables belong to given rectangles");
    if (tables && *tables && (*tables)->ctx != ctx)
        return stx_fail(STX_ERR_INVALID, "warp tables: the handle belongs to another context (no cross-stream use)");
    WarpTablesSlot kept(ctx, tables);
    if (n == 0) return kept.keep();
    STX_TRY(stx_set_device(ctx));
    std::vector<StxProjector> ps(n);
    std::vector<int> sizes(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        if (!srcs[i] || srcs[i]->elem != STX_U8 || srcs[i]->c != 3) return stx_fail(STX_ERR_INVALID, "warp source %d must be u8x3", i);
        // sources may live in another context of the same device (long-lived read-only inputs shared by several streams)
        if (srcs[i]->ctx->device != ctx->device) return stx_fail(STX_ERR_INVALID, "warp source %d lives on another device", i);
        STX_TRY(stx_make_projector(type, scale, K9s + 9 * i, R9s + 9 * i, &ps[i]));
        sizes[2 * i] = srcs[i]->w;
        sizes[2 * i + 1] = srcs[i]->h;
    }
    // with gains the ROI of every image is needed even under caller-given rectangles: the gain map lies over the WHOLE warped image.
    // STX_WARP_FRESH_ROIS: the ROI pass belongs to this call, whatever the cache holds.
    std::vector<int> full_rois(4 * (size_t)n);
    if (!rects_xywh || gain_maps)
        STX_TRY(rois_cached(ctx, type, scale, n, K9s, R9s, ps.data(), sizes.data(), !fresh_rois, full_rois.data()));
    const std::vector<int> rois = rects_xywh ? std::vector<int>(rects_xywh, rects_xywh + 4 * (size_t)n) : full_rois;
    if (gain_maps) {
        for (int i = 0; i < n; i++) STX_TRY(block_gain_check(ctx, nullptr, gain_maps[i]));
        for (int i = 0; i < n && rects_xywh; i++) {
            const int *r = &rois[4 * i], *f = &full_rois[4 * i];
            if (r[0] < f[0] || r[1] < f[1] || r[0] + r[2] > f[0] + f[2] || r[1] + r[3] > f[1] + f[3])
                return stx_fail(STX_ERR_INVALID, "image %d: with gains the rectangle must lie inside the warp roi", i);
        }
    }

    std::vector<StxBufRef> bi(n), bm(n);
    std::vector<StxWarpLaunch> Ls(n);
    for (int i = 0; i < n; i++) {
        const int* roi = &rois[4 * i];
        STX_TRY(check_warp_rect(roi));
        if (out_imgs) STX_TRY(stx_buf_new(ctx, roi[2], roi[3], 3, STX_U8, &bi[i]));
        if (out_masks) STX_TRY(stx_buf_new(ctx, roi[2], roi[3], 1, STX_U8, &bm[i]));
        Ls[i] = warp_launch(ps[i], roi, srcs[i], srcs[i]->w, srcs[i]->h, bi[i].get(), bm[i].get());
    }
    // Exposure gains (BlocksCompensator::apply, stitching/stitcher.py:123,219-221).  Fused into the warp's epilogue when every image runs
    // the tuned kernel and every map is a bounded single-channel one: the warped bytes leave LDS already multiplied, the 6 bytes per
    // pixel of a separate pass never move.  Anything else: warp, then stx_block_gain_apply_batch — the same bytes either way.
    std::vector<int> sub;
    StxDevBlock gscratch;
    bool fused = false;
    if (gain_maps) {
        for (int i = 0; i < n; i++) {
            sub.push_back(full_rois[4 * i + 2]); sub.push_back(full_rois[4 * i + 3]);
            sub.push_back(rois[4 * i] - full_rois[4 * i]); sub.push_back(rois[4 * i + 1] - full_rois[4 * i + 1]);
        }
        static const bool no_fuse = getenv("STITCHING_AMD_NO_GAIN_FUSION") != nullptr;  // diagnostic: A/B against the separate pass
        fused = !no_fuse;
        for (int i = 0; i < n && fused; i++)
            // (a validity mask: the tuned kernel has no gain x validity form; this launch runs once per rig, the second pass gives the same bytes)
            fused = !Ls[i].vsrc && gain_maps[i]->c == 1 && gain_flags && (gain_flags[i] & STX_GAIN_MAP_BOUNDED) && stx_warp_fast_eligible(Ls[i]) &&
                    (size_t)gain_maps[i]->h * (size_t)Ls[i].dw < ((size_t)16 << 20);
        if (fused) {
            std::vector<size_t> offH(n), offY(n);
            size_t bytes = 0;
            for (int i = 0; i < n; i++) {
                offH[i] = bytes; bytes += align_up((size_t)gain_maps[i]->h * ((Ls[i].dw + 3) & ~3) * sizeof(float), 256);
                offY[i] = bytes; bytes += align_up((size_t)Ls[i].dh * 8, 256);
            }
            STX_TRY(stx_dev_alloc(ctx, bytes, &gscratch));
            std::vector<float*> Hs(n);
            std::vector<void*> yts(n);
            std::vector<int> wh(2 * (size_t)n);
            for (int i = 0; i < n; i++) {
                Hs[i] = (float*)((uint8_t*)gscratch.get() + offH[i]); yts[i] = (uint8_t*)gscratch.get() + offY[i];
                wh[2 * i] = Ls[i].dw; wh[2 * i + 1] = Ls[i].dh;
                Ls[i].gain_H = Hs[i]; Ls[i].gain_hstride = (Ls[i].dw + 3) & ~3; Ls[i].gain_yt = yts[i]; Ls[i].gain_gh = gain_maps[i]->h;
            }
            STX_TRY(stx_launch_gain_rows(ctx, n, wh.data(), gain_maps, sub.data(), Hs.data(), yts.data()));
        }
    }
    STX_TRY(stx_launch_warp_batch(ctx, Ls.data(), n, kept.get()));
    gscratch.reset();  // stream-ordered reuse
    if (gain_maps && !fused) STX_TRY(stx_block_gain_apply_batch(ctx, n, stx_buf_ptrs(bi).data(), gain_maps, sub.data(), gain_flags));
    for (int i = 0; i < n; i++) {
        if (bm[i]) bm[i]->mask_binary = Ls[i].vsrc ? srcs[i]->validity->mask_binary : 1;
        if (out_imgs) out_imgs[i] = bi[i].release();
        if (out_masks) out_masks[i] = bm[i].release();
    }
    if (out_xywh) memcpy(out_xywh, rois.data(), sizeof(int) * 4 * (size_t)n);
    return kept.keep();
}

// The warp through the lens (include/stitching_amd.h): K, R and the rectangles are the rectified frame's, whose
// size is the map's destination size; the source is the map's distorted frame.  Images only.
STX_EXPORT int stx_warp_lens_batch(stx_ctx* ctx, int type, float scale, int n, const float* K9s, const float* R9s, const stx_buf* const* srcs,
                                   const stx_lens_map* const* maps, const int* rects_xywh, stx_buf** out_imgs, int* out_xywh,
                                   stx_warp_tables** tables)
{
    if (!ctx || !K9s || !R9s || !srcs || !maps || !out_imgs || n < 0) return stx_fail(STX_ERR_INVALID, "bad argument");
    if (tables && *tables && (*tables)->ctx != ctx)
        return stx_fail(STX_ERR_INVALID, "warp tables: the handle belongs to another context (no cross-stream use)");
    if (remap_mode_now() != STX_REMAP_Q15)
        return stx_fail(STX_ERR_INVALID, "warp through the lens: the sampler has one arithmetic, the remap mode must be q15");
    std::vector<StxProjector> ps((size_t)n);
    std::vector<int> sizes(2 * (size_t)n);
    std::vector<StxLensK> lens((size_t)n);
    for (int i = 0; i < n; i++) {
        const stx_buf* S = srcs[i];
        const stx_lens_map* M = maps[i];
        if (!S) return stx_fail(STX_ERR_INVALID, "warp through the lens: image %d is a null handle", i);
        if (!M) return stx_fail(STX_ERR_INVALID, "warp through the lens: lens map %d is a null handle", i);
        if (S->ctx != ctx || M->ctx != ctx) return stx_fail(STX_ERR_INVALID, "warp through the lens: image or lens map %d belongs to another context", i);
        if (S->elem != STX_U8 || S->c != 3) return stx_fail(STX_ERR_INVALID, "warp through the lens: source %d must be u8x3", i);
        if (S->w != M->src_w || S->h != M->src_h)
            return stx_fail(STX_ERR_INVALID, "warp through the lens: image %d is %dx%d, its lens map was made for %dx%d", i, S->w, S->h, M->src_w, M->src_h);
        // the sampler's 32-bit offsets and 24-bit row multiply (stx_rectify's limits)
        if (S->stride >= (size_t)1 << 24 || (unsigned long long)(S->h - 1) * S->stride + (unsigned long long)S->w * 3 + 32 > 0x7fffffffull)
            return stx_fail(STX_ERR_INVALID, "warp through the lens: image %d spans %llu bytes with a pitch of %zu: below 2^31 and 2^24 is taken", i,
                            (unsigned long long)(S->h - 1) * S->stride + (unsigned long long)S->w * 3, S->stride);
        if (rects_xywh) STX_TRY(check_warp_rect(rects_xywh + 4 * i));
        STX_TRY(stx_make_projector(type, scale, K9s + 9 * i, R9s + 9 * i, &ps[i]));
        sizes[2 * i] = M->dst_w;
        sizes[2 * i + 1] = M->dst_h;
        StxLensK& L = lens[i];
        L.nodes = (const int2*)M->d_nodes.get(); L.nx = M->nx; L.w = M->dst_w; L.h = M->dst_h;
        L.src = S->ptr; L.spitch = (int)S->stride; L.sw = S->w; L.sh = S->h;
    }
    // nothing was allocated or queued up to here
    WarpTablesSlot kept(ctx, tables);
    if (n == 0) return kept.keep();
    STX_TRY(stx_set_device(ctx));
    std::vector<int> rois(4 * (size_t)n);
    if (rects_xywh) rois.assign(rects_xywh, rects_xywh + 4 * (size_t)n);
    else STX_TRY(rois_cached(ctx, type, scale, n, K9s, R9s, ps.data(), sizes.data(), true, rois.data()));
    std::vector<StxBufRef> bi((size_t)n);
    std::vector<StxWarpLaunch> Ls((size_t)n);
    for (int i = 0; i < n; i++) {
        const int* roi = &rois[4 * i];
        STX_TRY(check_warp_rect(roi));
        STX_TRY(stx_buf_new(ctx, roi[2], roi[3], 3, STX_U8, &bi[i]));
        Ls[i] = warp_launch(ps[i], roi, nullptr, sizes[2 * i], sizes[2 * i + 1], bi[i].get(), nullptr);
    }
    STX_TRY(stx_launch_warp_lens_batch(ctx, Ls.data(), lens.data(), n, kept.get()));
    for (int i = 0; i < n; i++) out_imgs[i] = bi[i].release();
    if (out_xywh) memcpy(out_xywh, rois.data(), sizeof(int) * 4 * (size_t)n);
    return kept.keep();
}

STX_EXPORT int stx_warp_tables_free(stx_warp_tables* t)
{
    if (!t) return STX_OK;
    if (t->block) {
        hipSetDevice(t->ctx->device);
        stx_dev_free(t->ctx, t->block);  // stream-ordered, as stx_mb_weights_free
    }
    delete t;
    return STX_OK;
}

STX_EXPORT int stx_debug_warp_table_launches(stx_ctx* ctx, int* out_launches)
{
    if (!ctx || !out_launches) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_launches = ctx->warp_table_launches;
    return STX_OK;
}

STX_EXPORT int stx_warp_image_and_mask(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9],
                                       const stx_buf* src, stx_buf** out_img, stx_buf** out_mask, int out_xywh[4])
{
    if (!ctx || !src) return stx_fail(STX_ERR_INVALID, "null argument");
    if (!out_img && !out_mask) return stx_fail(STX_ERR_INVALID, "nothing requested");
    STX_TRY(stx_set_device(ctx));
    if (src->elem != STX_U8 || src->c != 3) return stx_fail(STX_ERR_INVALID, "warp source must be u8x3");
    return warp_impl(ctx, type, scale, K, R, src, src->w, src->h, out_img != nullptr, out_mask != nullptr, false,
                     out_img, out_mask, out_xywh);
}

STX_EXPORT int stx_warp_mask(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], int w, int h,
                             stx_buf** out_mask, int out_xywh[4])
{
    if (!ctx || !out_mask) return stx_fail(STX_ERR_INVALID, "null argument");
    if (w <= 0 || h <= 0) return stx_fail(STX_ERR_INVALID, "image size %dx%d", w, h);
    STX_TRY(stx_set_device(ctx));
    return warp_impl(ctx, type, scale, K, R, nullptr, w, h, false, true, false, nullptr, out_mask, out_xywh);
}

// Test hook (include/stitching_amd_debug.h): the fp32 backward map of a warp as the device projector computes it.
STX_EXPORT int stx_debug_warp_maps(stx_ctx* ctx, int type, float scale, const float K[9], const float R[9], int w, int h, int which,
                                   const int rect_xywh[4], stx_buf** out_xmap, stx_buf** out_ymap, int out_xywh[4])
{
    if (!ctx || !K || !R || !out_xmap || !out_ymap) return stx_fail(STX_ERR_INVALID, "null argument");
    if (w <= 0 || h <= 0) return stx_fail(STX_ERR_INVALID, "image size %dx%d", w, h);
    if (which != 1 && which != 2) return stx_fail(STX_ERR_INVALID, "which = %d (1: the kernel a warp takes, 2: the generic kernel)", which);
    STX_TRY(stx_set_device(ctx));
    StxProjector p;
    STX_TRY(stx_make_projector(type, scale, K, R, &p));
    int roi[4];
    const int sz[2] = {w, h};
    if (rect_xywh) memcpy(roi, rect_xywh, 16);
    else STX_TRY(rois_cached(ctx, type, scale, 1, K, R, &p, sz, true, roi));
    if (roi[2] <= 0 || roi[3] <= 0 || (long long)roi[2] * roi[3] > (1ll << 30))
        return stx_fail(STX_ERR_INVALID, "degenerate warp roi %dx%d", roi[2], roi[3]);
    StxBufRef bx, by;
    STX_TRY(stx_buf_new(ctx, roi[2], roi[3], 1, STX_F32, &bx));
    STX_TRY(stx_buf_new(ctx, roi[2], roi[3], 1, STX_F32, &by));
    StxWarpLaunch L = warp_launch(p, roi, nullptr, w, h, bx.get(), by.get());
    L.debug_maps = which;
    STX_TRY(stx_launch_warp(ctx, L));
    *out_xmap = bx.release();
    *out_ymap = by.release();
    if (out_xywh) memcpy(out_xywh, roi, 16);
    return STX_OK;
}
