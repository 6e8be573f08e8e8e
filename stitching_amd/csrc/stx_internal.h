// stx_internal.h — host-side structures shared by the C-ABI translation units.
// gfx950 only; no CUDA compatibility layer.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/stitching_amd.h"
#include "../../include/stitching_amd_debug.h"

#define STX_EXPORT extern "C" __attribute__((visibility("default")))
#define STX_MAX_BANDS 16

// ---------------------------------------------------------------------------------------------
// error reporting
// ---------------------------------------------------------------------------------------------
void stx_set_error(const char* fmt, ...);
int stx_fail(int code, const char* fmt, ...);

#define STX_HIP(call)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return stx_fail(e_ == hipErrorOutOfMemory ? STX_ERR_OOM : STX_ERR_HIP, "%s failed: %s (%s:%d)", \
                            #call, hipGetErrorString(e_), __FILE__, __LINE__);                             \
    } while (0)

// after a kernel launch (or a run of them): the launch error, if any, as "<what> launch failed: ..."
inline int stx_check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return stx_fail(STX_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return STX_OK;
}

#define STX_TRY(call)           \
    do {                        \
        int rc_ = (call);       \
        if (rc_ != STX_OK) return rc_; \
    } while (0)

// the timing events of one estimator run, at most 4.  arm(n) where the caller asked for timings; mark(k) records event k and does nothing
// while the timer is not armed; ms(a, b) reads the time between two marks once the stream has been waited for
struct StxEventTimer {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int armed = 0;  // events created
    StxEventTimer() = default;
    StxEventTimer(const StxEventTimer&) = delete;
    StxEventTimer& operator=(const StxEventTimer&) = delete;
    ~StxEventTimer() { for (int k = 0; k < armed; k++) hipEventDestroy(ev[k]); }
    int arm(int n)
    {
        for (; armed < n && armed < 4; armed++) STX_HIP(hipEventCreate(&ev[armed]));
        return STX_OK;
    }
    int mark(int k, hipStream_t stream)
    {
        if (k < armed) STX_HIP(hipEventRecord(ev[k], stream));
        return STX_OK;
    }
    int ms(int a, int b, double* out) const
    {
        float t = 0.f;
        STX_HIP(hipEventElapsedTime(&t, ev[a], ev[b]));
        *out = t;
        return STX_OK;
    }
};

// `waiter` goes on behind what `signaller` has queued so far: an untimed event there, waited for by `waiter` — no host wait.  The runtime
// releases the event once it has completed.  what: the caller's words for the message, "<what> failed: ..."
inline int stx_stream_wait(hipStream_t waiter, hipStream_t signaller, const char* what)
{
    hipEvent_t ev = nullptr;
    STX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, signaller);
    if (e == hipSuccess) e = hipStreamWaitEvent(waiter, ev, 0);
    hipEventDestroy(ev);
    if (e != hipSuccess) return stx_fail(STX_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return STX_OK;
}

// ---------------------------------------------------------------------------------------------
// context: stream, caching allocator, profiler
// ---------------------------------------------------------------------------------------------
struct StxProfEntry {
    std::string name;
    int64_t calls = 0;
    double total_ms = 0.0;
    double algo_bytes = 0.0;
};

struct StxPendingEvent {
    hipEvent_t start, stop;
    int entry;
};

struct stx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // side stream + private device scratch of the ROI pass: it depends on nothing queued on `stream`, so a
    // pipeline of panoramas can take its ROIs while the previous panorama is still blending
    hipStream_t aux_stream = nullptr;
    void* aux_scratch = nullptr;
    // caching allocator: bucket size -> free blocks (alloc_mutex: Python finalizers may free buffers from any thread)
    std::mutex alloc_mutex;
    std::map<size_t, std::vector<void*>> free_blocks;
    std::map<void*, size_t> block_size;
    size_t bytes_allocated = 0;
    // pinned scratch for small device->host results (ROI min/max)
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    uint32_t roi_seq = 0;  // sequence number of the last ROI pass (the stamp its blocks write behind their results)
    // pinned ring for small host->device uploads (descriptor tables): truly asynchronous copies.  The ring is cut into
    // STX_STAGE_SEGS segments; leaving a segment records an event behind its last copy, entering one waits for the event of
    // its previous lap (recorded three segments of uploads ago: normally long complete) — not for the whole stream, which
    // with a deep queue of panoramas costs the host tens of milliseconds and the GPU a bubble (stx_stage_upload)
    uint8_t* stage = nullptr;
    size_t stage_bytes = 0, stage_off = 0;
    hipEvent_t stage_ev[4] = {};
    bool stage_ev_set[4] = {};
    int stage_seg = 0;
    // profiler
    bool prof_on = false;
    std::vector<StxProfEntry> prof;
    std::map<std::string, int> prof_index;
    std::vector<StxPendingEvent> prof_pending;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t marks[16] = {};
    // exposure estimation: sqrt(k) for k = 0 .. 3 * 255^2 in fp64, uploaded at the first feed (an allocator block: freed with the context)
    double* exp_sqrt = nullptr;
    // gather launches of the last blend() that took their images from a cover table (stx_debug_blend_replayed)
    int blend_replayed = 0;
    // table kernels the last batched warp launched (stx_debug_warp_table_launches), descriptor uploads of the last blend()
    // (stx_debug_blend_uploads)
    int warp_table_launches = 0;
    int blend_uploads = 0;
    int blend_mask_stored = 0;  // the level-0 launch of the last multi-band blend() stored the panorama mask (stx_debug_blend_mask_stored)
    // seam masks sent through {one-launch LDS, table 4-pixel batch, single 4-pixel, per-pixel} since the context was made
    // (stx_debug_seam_resize_paths): bumped where stx_resize.hip makes the launches
    int seam_resize_paths[4] = {0, 0, 0, 0};
};

#define STX_STAGE_SEGS 4
int stx_dev_alloc(stx_ctx* ctx, size_t bytes, void** out);
// host -> device copy of a small table through the context's pinned ring: queued on ctx->stream, no host wait in the common case
int stx_stage_upload(stx_ctx* ctx, void* d, const void* h, size_t bytes);
void stx_dev_free(stx_ctx* ctx, void* p);
int stx_set_device(stx_ctx* ctx);
// owner of one allocator block: whatever leaves the scope early (STX_TRY / STX_HIP) gives it back.  reset() where the last launch that
// uses a scratch block has been queued (stream-ordered reuse: the next stx_dev_alloc may hand it out again), release() to pass it on.
struct StxDevFree { stx_ctx* ctx; void operator()(void* p) const { stx_dev_free(ctx, p); } };
using StxDevBlock = std::unique_ptr<void, StxDevFree>;
inline int stx_dev_alloc(stx_ctx* ctx, size_t bytes, StxDevBlock* out)
{
    void* p = nullptr;
    STX_TRY(stx_dev_alloc(ctx, bytes, &p));
    *out = StxDevBlock(p, StxDevFree{ctx});
    return STX_OK;
}
// guard of an estimator run: waits for the context's stream when the run ends, on a refusal or a HIP error as well.  Members and locals
// go in the reverse order of their declaration, so declare it BEHIND the blocks, scratch images and timer of the run: it then waits
// before any of them is given back, and they go back last-declared first.
struct StxRunGuard {
    stx_ctx* ctx;
    explicit StxRunGuard(stx_ctx* c) : ctx(c) {}
    StxRunGuard(const StxRunGuard&) = delete;
    StxRunGuard& operator=(const StxRunGuard&) = delete;
    ~StxRunGuard() { if (ctx) hipStreamSynchronize(ctx->stream); }
};
// small host array -> a fresh block through the context's pinned ring (asynchronous)
int upload_small(stx_ctx* ctx, const void* h, size_t bytes, StxDevBlock* d_out);
size_t align_up(size_t v, size_t a);

// profiling bracket around one kernel launch
struct StxProfScope {
    stx_ctx* ctx;
    int pending = -1;
    hipStream_t stream;  // the stream the bracketed kernel is launched on (default: the context's main stream)
    bool attached;       // true: the scope holds ONE launch and the caller attaches start() / stop() to it (hipExtLaunchKernelGGL): the
                         // events then carry the dispatch's own begin / end stamps, as rocprofv3 reports them.  false: an event recorded
                         // before and one after whatever the scope launches — 3-5 us more than the kernel (tools/ubench/event_bracket.hip)
    StxProfScope(stx_ctx* c, const char* name, double algo_bytes, hipStream_t on = nullptr, bool attach = false);
    ~StxProfScope();
    hipEvent_t start() const;  // null while the profiler is off: launch plainly
    hipEvent_t stop() const;
};

// ---------------------------------------------------------------------------------------------
// device image
// ---------------------------------------------------------------------------------------------
struct stx_buf {
    stx_ctx* ctx = nullptr;
    void* base = nullptr;  // allocation (owned when parent == nullptr)
    uint8_t* ptr = nullptr;
    int w = 0, h = 0, c = 0, elem = 0;
    size_t stride = 0;  // bytes
    stx_buf* parent = nullptr;
    // the validity mask a u8x3 frame carries (stx_buf_with_validity): a u8x1 image of this size, one reference held; read by
    // stx_warp_batch and stx_warp_image_and_mask alone, never written
    stx_buf* validity = nullptr;
    int mask_binary = 0;  // 1: a u8x1 image known to hold only 0 and 255 (warped masks; scanned host uploads)
    std::atomic<int> refs{1};
};

// readable bytes in front of the first row of every image the library allocates (views inherit them from their parent: whatever
// precedes a view's first pixel is memory of the same allocation)
constexpr size_t STX_BUF_FRONT_PAD = 64;
inline int stx_elem_bytes(int elem) { return elem == STX_U8 ? 1 : (elem == STX_S16 ? 2 : 4); }
int stx_buf_new(stx_ctx* ctx, int w, int h, int c, int elem, stx_buf** out);
void stx_buf_retain(stx_buf* b);
void stx_buf_release(stx_buf* b);
// owner of one reference to an image: dropped at scope exit, handed to the caller with release()
struct StxBufRelease { void operator()(stx_buf* b) const { stx_buf_release(b); } };
using StxBufRef = std::unique_ptr<stx_buf, StxBufRelease>;
inline int stx_buf_new(stx_ctx* ctx, int w, int h, int c, int elem, StxBufRef* out)
{
    stx_buf* b = nullptr;
    STX_TRY(stx_buf_new(ctx, w, h, c, elem, &b));
    out->reset(b);
    return STX_OK;
}
// the raw pointers of a vector of handles, for the launchers' argument arrays
inline std::vector<stx_buf*> stx_buf_ptrs(const std::vector<StxBufRef>& v)
{
    std::vector<stx_buf*> p;
    for (const StxBufRef& b : v) p.push_back(b.get());
    return p;
}

// process-wide arithmetic modes (stx_modes.cpp): the value now, read from the environment on first use ------------------------------
int trig_mode_now();     // STX_TRIG_*
int remap_mode_now();    // STX_REMAP_*
int pyrdown_now();       // STX_PYRDOWN_* | lanes << 8
int exposure_solver_now();  // STX_EXPOSURE_SOLVER_*

// ---------------------------------------------------------------------------------------------
// projector (host side of ProjectorBase::setCameraParams)
// ---------------------------------------------------------------------------------------------
// projector families behind the 16 warper ids (id -> family, a, b: stx_make_projector)
enum { STX_F_PLANE = 0, STX_F_CYLINDRICAL, STX_F_SPHERICAL, STX_F_FISHEYE, STX_F_STEREOGRAPHIC, STX_F_CRECT,
       STX_F_CRECT_PORTRAIT, STX_F_PANINI, STX_F_PANINI_PORTRAIT, STX_F_MERCATOR, STX_F_TRANSVERSE_MERCATOR };
struct StxProjector {
    int type;
    int family;
    float a, b;
    float scale;
    float k[9], rinv[9], r_kinv[9], k_rinv[9], t[3];
    int trig;  // STX_TRIG_*: the process-wide trig mode at the time the projector was made (stx_set_trig_mode)
    int remap; // STX_REMAP_*: likewise the interpolation model of the image samples (stx_set_remap_mode)
};
int stx_make_projector(int type, float scale, const float* K, const float* R, StxProjector* out);

// kernels' host launchers (defined in the .hip files) --------------------------------------------
struct StxWarpLaunch {
    StxProjector proj;
    int tlx, tly, dw, dh;          // destination roi
    const uint8_t* src; int sw, sh; size_t sstride; int src_channels;  // src may be null (mask only)
    uint8_t* dimg; size_t dimg_stride;    // u8x3 or null
    uint8_t* dmask; size_t dmask_stride;  // u8x1 or null
    int nearest_src;               // 1: out image = nearest sample of a u8x1 source (generic mask warp)
    // source validity mask (stx_buf_with_validity): u8x1 of sw x sh with its own pitch; the warped mask is its nearest sample.  null: 255
    const uint8_t* vsrc = nullptr; size_t vstride = 0;
    int debug_maps = 0;            // stx_debug_warp_maps (test hook): dimg / dmask are f32 maps of x / y; 1: the kernel a warp would take, 2: the generic one
    // fused exposure gain (stx_warp_batch with gain_maps): device tables made by stx_launch_gain_rows for this destination rectangle; null: none
    const float* gain_H = nullptr; long long gain_hstride = 0; const void* gain_yt = nullptr; int gain_gh = 0;
};
// typed projectors only (plane / affine / cylindrical / spherical / mercator), Q15 or float remap: what a fused gain needs
bool stx_warp_fast_eligible(const StxWarpLaunch& L);
// The column / row tables of one batched warp call of the typed projectors, kept between calls (stx_warp_batch with tables): the device
// block and, per image, everything warp_tables_kernel reads.  The launcher compares the record with the call in front of it and rebuilds
// the tables into the handle on any difference: the decision is never the caller's.
struct StxWarpTabRec { int family, dw, dh, tlx, tly, trig; float scale, t0, t1, kr1, kr4, kr7; };
struct stx_warp_tables {
    stx_ctx* ctx = nullptr;
    int type = -1;                   // the launcher's instantiation (STX_WARP_PLANE / _CYLINDRICAL / _SPHERICAL); -1: nothing recorded
    std::vector<StxWarpTabRec> rec;  // one per image of the call, in order
    void* block = nullptr;           // an allocator block of `floats2` float2: the cursor layout of launch_typed follows from dw and dh
    size_t floats2 = 0;
};
int stx_launch_warp(stx_ctx* ctx, const StxWarpLaunch& L);
int stx_launch_warp_batch(stx_ctx* ctx, const StxWarpLaunch* Ls, int n, stx_warp_tables* kept = nullptr);
// The warp through the lens (stx_warp_lens_batch): what its sampler reads, a kernel argument of its own next to the projector's —
// the nodes of the camera's lens grid (stx_lens_map: nx per row, Q6) over the rectified w x h, and the distorted u8x3 source.
struct StxLensK {
    const int2* nodes; int nx;
    int w, h;  // the rectified frame: what the projector's K, R and the clip of the map's positions belong to
    const uint8_t* src; int spitch; int sw, sh;
};
// Ls[i]: the projector and the destination rectangle with sw x sh the RECTIFIED size, an image and no mask, no source (lens[i] has it)
int stx_launch_warp_lens_batch(stx_ctx* ctx, const StxWarpLaunch* Ls, const StxLensK* lens, int n, stx_warp_tables* kept);
int stx_launch_roi_minmax(stx_ctx* ctx, int n, const StxProjector* projs, const int* sizes_wh, float* out_minmax4);

// multi-band -------------------------------------------------------------------------------------
struct StxMbImage {  // device-visible descriptor of one fed image (all levels)
    // kind 0: an image fed on this rank.  kind 1: a contribution strip received from another rank:
    // per level i, g[i] holds (short)(L_i * W_i) and wt[i] holds W_i over the rect (fx,fy,fw,fh) >> i.
    int kind; int order;
    const uint8_t* img0; long long img0_stride; int img0_is_s16;
    const uint8_t* mask0; long long mask0_stride; int mask_binary;
    int iw, ih;            // image size
    int ix, iy;            // image corner relative to the (padded) panorama roi
    int fx, fy, fw, fh;    // feed rect (tl_new .. br_new) relative to the panorama roi, level 0
    int left, top;         // copyMakeBorder offsets: bordered(x,y) = img(reflect(x-left), reflect(y-top))
    // levels 1..B: planar Gaussian pyramid (3 planes) and fp32 weight pyramid.  g_u8 = 1 (every image fed as u8: all values are
    // 0..255): the planes hold one BYTE per sample — g[] then points to bytes, g_stride / g_plane count samples either way.  int16
    // images (and received contribution strips, kind 1) keep int16 planes.  64 readable bytes in front of every allocation.
    int g_u8;
    short* g[STX_MAX_BANDS + 1]; long long g_stride[STX_MAX_BANDS + 1]; long long g_plane[STX_MAX_BANDS + 1];
    float* wt[STX_MAX_BANDS + 1]; long long wt_stride[STX_MAX_BANDS + 1];
    // w1_f16 = 1 (round 6: an image fed on this rank whose mask holds only 0 / 255): wt[1] points to IEEE HALF values (wt_stride[1] still counts
    // samples).  W_0 is then exactly 0.f / 1.f, pyrDown's 25-tap sum a small integer k <= 256 in whatever order it is taken, and
    // W_1 = k / 256 has a 9-bit significand: the half holds it exactly, the conversion back is exact, every consumer sees the same
    // fp32 value as before — at 2 instead of 4 of the 7 bytes a level-1 sample costs (written once, read by the level-1 pyrDown and by
    // the level-1 gather).  Levels >= 2 need 17 and more bits and stay fp32.
    int w1_f16;
    // occupancy of the weight pyramid (null: not recorded): occ[i][p * nt + t] != 0 iff W_i has a non-zero value in the rows
    // 2 p, 2 p + 1 and the columns 64 t .. 64 t + 63 of level i (frame coordinates), nt = ((fw >> i) + 63) / 64 rounded up to 4.  Every entry is
    // written by the pyramid kernel that produces the level (one byte store per half-wavefront: no atomics, no clearing);
    // the gather kernels read it to pass over the empty parts of a feed rectangle (bounding boxes of pitched / rolled frames,
    // seam masks, exchange strips) a wavefront at a time.
    uint8_t* occ[STX_MAX_BANDS + 1];
};
// the gather kernels fetch (iw, ih, ix, iy) and (fx, fy, fw, fh) as ONE 16-byte load each, from &im.iw and &im.fx, on 4-byte alignment
static_assert(offsetof(StxMbImage, ih) == offsetof(StxMbImage, iw) + 4 && offsetof(StxMbImage, ix) == offsetof(StxMbImage, iw) + 8 &&
                  offsetof(StxMbImage, iy) == offsetof(StxMbImage, iw) + 12 && offsetof(StxMbImage, iw) % 4 == 0,
              "StxMbImage: iw, ih, ix, iy must be four adjacent ints");
static_assert(offsetof(StxMbImage, fy) == offsetof(StxMbImage, fx) + 4 && offsetof(StxMbImage, fw) == offsetof(StxMbImage, fx) + 8 &&
                  offsetof(StxMbImage, fh) == offsetof(StxMbImage, fx) + 12 && offsetof(StxMbImage, fx) % 4 == 0,
              "StxMbImage: fx, fy, fw, fh must be four adjacent ints");
// pyr_mode / pyr_lanes: STX_PYRDOWN_* (include/stitching_amd.h); anything but SCALAR builds every level with the generic kernels
// weights = false: the G planes alone (all images of the call; their weights were adopted from a stx_mb_weights handle)
int stx_launch_mb_pyramids(stx_ctx* ctx, const StxMbImage* d_images, const StxMbImage* h_images, int n, int num_bands, int pyr_mode,
                           int pyr_lanes, bool weights);
struct MbLevelK;
int stx_launch_mb_level(stx_ctx* ctx, const MbLevelK& K, double algo_bytes);
int stx_launch_mb_coarse(stx_ctx* ctx, const MbLevelK& K_level_Bm2, double algo_bytes);  // levels B, B-1, B-2 in one launch

// pointwise exposure gain (next row N1; stx_gain.hip) --------------------------------------------------------------
int stx_launch_gain_apply(stx_ctx* ctx, stx_buf* img, const float g[3]);
int block_gain_check(stx_ctx* ctx, const stx_buf* img, const stx_buf* gain_map);  // img may be null: the map alone
int stx_launch_block_gain(stx_ctx* ctx, stx_buf* img, const stx_buf* gmap, const int* d_xt, const int* d_yt);
int stx_launch_block_gain_batch(stx_ctx* ctx, int n, stx_buf* const* imgs, const stx_buf* const* gmaps, const int* full_wh_xy0,
                                float* const* Hs, void* const* yts, const int* fast);
// only the first half of it — H rows and row tables of n rectangles (w, h at (x0, y0) of a full_w x full_h image each) — for a consumer
// that multiplies the gain in itself (the warp kernel's epilogue); wh = {w, h} per rectangle
int stx_launch_gain_rows(stx_ctx* ctx, int n, const int* wh, const stx_buf* const* gmaps, const int* full_wh_xy0, float* const* Hs,
                         void* const* yts);
// exposure-gain estimation (stx_exposure.hip, stx_exposure_host.cpp) ---------------------------------------------------------------
struct StxExpImg { const uint8_t* img; long long istride; const uint8_t* mask; long long mstride; };
// a pair job: images ia / ib, the intersection's top-left in each image (ax, ay) / (bx, by), its size w x h
struct StxExpJob { int ia, ib, ax, ay, bx, by, w, h; };
enum { STX_EXP_TREE = 0, STX_EXP_ORDERED = 1, STX_EXP_INT = 2 };
int stx_launch_exposure_stats(stx_ctx* ctx, const StxExpImg* d_imgs, const StxExpJob* d_jobs, int njobs, int mode, const double* d_sqrt,
                              long long* d_out_i, double* d_out_d, double algo_bytes);
// one u8x3 image multiplied by per-block gains g (bpw blocks of bw x bh per row, 1 or 3 (g3) floats per block)
struct StxExpBlockMul { uint8_t* img; long long stride; int w, h, bw, bh, bpw; const float* g; int g3; };
int stx_launch_exposure_block_mul(stx_ctx* ctx, const StxExpBlockMul* d_tab, int n, int max_pixels);
// cv::solve(DECOMP_LU) in fp64 on the device (stx_solve.hip): the n x n system given by its non-zero entries (col < n) and its right side
// (col == n) -> x[n], the bits of the host's lu_solve_sparse.  The dense matrix takes 8 n^2 bytes of device memory: n <= STX_LU_MAX_N
// (2 GiB).  out (or null): {device ms of scatter + elimination, ms of compaction + copy + host back substitution, non-zeros of U}.
struct StxLuEntry { int row, col; double v; };
constexpr int STX_LU_MAX_N = 16384;
int stx_lu_device(stx_ctx* ctx, int n, const StxLuEntry* entries, size_t count, double* x, double out[3]);
// exposure-gain tracking on a known rig (stx_exposure_track.hip, stx_exposure_track_host.cpp) -----------------
// The lattice of stride s: panorama pixels (l s, m s).  Per image, made once per rig: the rectangle's corner, the first lattice
// indices inside it (lx0, ly0), the lattice points per row (nx) and rows (ny), and where its V bytes start in the handle's grid block.
struct StxTrackGeo { int x, y, lx0, ly0, nx, ny; long long voff; };
// per image and measure: the warped, compensated u8x3 image of the rectangle
struct StxTrackPix { const uint8_t* img; long long istride; };
// a tile of one pair's lattice points: images a < b, the pair's index, the tile's first lattice indices and its extent
// (1 .. STX_TRACK_TILE each way)
struct StxTrackTile { int a, b, pair, lx, ly, nx, ny, pad_; };
constexpr int STX_TRACK_WG = 256, STX_TRACK_TILE = 32, STX_TRACK_MAX_TILES = STX_TRACK_TILES_MAX, STX_TRACK_MAX_IMAGES = STX_TRACK_IMAGES_MAX,
              STX_TRACK_MAX_STRIDE = STX_TRACK_STRIDE_MAX;  // the limits of include/stitching_amd.h
// a lane's u32 partial holds at most (tile points / lanes) samples of at most 255 each, a wavefront's 64 times that
static_assert((long long)STX_TRACK_TILE * STX_TRACK_TILE / STX_TRACK_WG * 255 * 64 < (1ll << 32), "tracking: a partial sum must fit 32 bits");
// masks (u8x1 of the rectangles' sizes: pointer and pitch per image) -> V bytes (1: the mask is 255 at the lattice point) and c_ii
// added into d_self[n] (cleared by the caller); max_points: the most lattice points of one image
int stx_launch_exposure_track_grid(stx_ctx* ctx, int n, const StxTrackGeo* d_geo, const StxTrackPix* d_masks, int stride, long long max_points,
                                   uint8_t* d_grid, unsigned long long* d_self);
// one workgroup per tile; eight 64-bit integer sums per pair added into d_acc[8 pairs] (cleared by the caller)
int stx_launch_exposure_track_stats(stx_ctx* ctx, const StxTrackGeo* d_geo, const StxTrackPix* d_pix, const StxTrackTile* d_tiles, int ntiles,
                                    int stride, const uint8_t* d_grid, unsigned long long* d_acc, double algo_bytes);
// out = map * factor in fp32, up to STX_SCALE_MAPS_PER_LAUNCH maps a launch; the factors travel in the kernel's arguments
constexpr int STX_SCALE_MAPS_PER_LAUNCH = 32;
struct StxScaleMap { const float* src; float* dst; long long sstride, dstride; int w, h, sc, dc; float f[3]; int pad_; };  // strides in floats
int stx_launch_gain_maps_scale(stx_ctx* ctx, const StxScaleMap* maps, int n);
// seam finding (stx_seams.hip, stx_seams_host.cpp) ----------------------------------------------------------------------------------
// a pair of one level: masks i (m1) and j (m2) with their strides and sizes, the window's top-left in each image (roi - gap - corner),
// window ww x wh, roi rw x rh (at (gap, gap) of the window), off: the pair's u16 distances in the level's arena (mask i's wh x rw plane,
// then mask j's)
struct StxSeamPair { uint8_t* m1; uint8_t* m2; long long s1, s2, off; int w1, h1, w2, h2, ox1, oy1, ox2, oy2, ww, wh, rw, rh; };
int stx_launch_seam_level(stx_ctx* ctx, const StxSeamPair* d_pairs, int np, int max_rows, int max_cols, uint16_t* d_arena, double algo_bytes);
// the project's own colour-aware seams (stx_color_seams.hip; host side in stx_seams_host.cpp) ------------------------------------------
// a pair of one level: images (u8x3) and masks of i (i1, m1) and j (i2, m2), every pointer at the roi's first pixel, strides in bytes;
// L x W: seam length x cross extent (a vertical seam: roi h x w, a horizontal one: w x h); off_choice / off_seam: byte offsets of the
// pair's L * W choice bytes and its L int32 cut positions (4-aligned) in the level's arena
struct StxColorSeamPair {
    const uint8_t* i1; const uint8_t* i2; uint8_t* m1; uint8_t* m2;
    long long si1, si2, sm1, sm2, off_choice, off_seam;
    int L, W, vertical, first_is_i;
};
int stx_launch_color_seam_level(stx_ctx* ctx, const StxColorSeamPair* d_pairs, int np, int max_cross, long long max_area, uint8_t* d_arena,
                                double algo_bytes);
// feature detection (stx_features.hip; host side in stx_features_host.cpp) ----------------------------------------------------------
// the grids are flat lists of tiles, image after image / level after level, as the batched resize's (tile0 ascending, first 0)
constexpr int STX_FEAT_GREY_TW = 64, STX_FEAT_GREY_TH = 4;    // grey: one pixel per lane
constexpr int STX_FEAT_BLUR_TW = 64, STX_FEAT_BLUR_TH = 8;    // blur: halo of 2 in LDS
constexpr int STX_FEAT_SCORE_TW = 32, STX_FEAT_SCORE_TH = 8;  // score + suppression + response: halo of 4 in LDS
constexpr int STX_FEAT_BORDER = 16;                           // keypoints lie in [16, w - 17] x [16, h - 17]
struct StxFeatImage { const uint8_t* img; long long istride; uint8_t* grey; long long gstride; int w, h, tiles_x, tile0; };
// one level of one image: grey level g, its blur, the image's level-0 mask (or null) of size w0 x h0; cand_off / cand_cap: the level's
// keys in the candidate arena (cap = one per 2 x 2 cell of the interior: strict 3 x 3 maxima cannot be denser)
struct StxFeatLevel {
    const uint8_t* g; long long gstride; uint8_t* blur; long long bstride; const uint8_t* mask; long long mstride;
    long long cand_off, cand_cap;
    int w, h, w0, h0, btiles_x, btile0, stiles_x, stile0;
};
// selection of one level: `count` candidates at cand_off, the first `keep` of them in key order go to out_off .. of the flat output
struct StxFeatSel { long long cand_off; int count, keep, out_off, pad_; };
// (response, y, x) as one ascending 64-bit key: (2^33 - R) << 30 | y << 15 | x, |R| < 2^33, x, y < 2^15
constexpr long long STX_FEAT_R_BIAS = 1ll << 33;
int stx_launch_feat_grey(stx_ctx* ctx, const StxFeatImage* d_imgs, int n, int tiles, double algo_bytes);
int stx_launch_feat_blur(stx_ctx* ctx, const StxFeatLevel* d_levels, int n, int tiles, double algo_bytes);
int stx_launch_feat_score(stx_ctx* ctx, const StxFeatLevel* d_levels, int n, int tiles, int threshold, unsigned long long* d_cand,
                          int* d_counts, double algo_bytes);
int stx_launch_feat_select(stx_ctx* ctx, const StxFeatSel* d_sel, int n, const unsigned long long* d_cand, unsigned long long* d_tmp,
                           unsigned long long* d_keys, int* d_item);
int stx_launch_feat_describe(stx_ctx* ctx, const StxFeatLevel* d_levels, int nl, const unsigned long long* d_keys, const int* d_item, int total,
                             const int* d_cxcy, const signed char* d_patterns, int* d_bins, uint8_t* d_desc);
// feature matching (stx_matches.hip; host side in stx_matches_host.cpp) ------------------------------------------------------------
// all images' descriptors (8 dwords each) and centred points (x, y doubles) lie in two flat arrays; an image is its first row there
constexpr int STX_MATCH_NN_WG = 256;     // match_2nn: queries per workgroup, and train descriptors per LDS tile
constexpr int STX_MATCH_HYP_PER_WG = 4;  // match_ransac: one wavefront per hypothesis
constexpr unsigned STX_MATCH_NO_D = 0xffffu;  // "no distance yet": above every Hamming distance of 256 bits
// one direction of a pair that can match at all (na > 0 queries, nb >= 2 train descriptors): the queries of image a among image b's;
// block0: the job's first workgroup of the flat grid (ascending, first 0); nn_off: its na results {i1, d1 | d2 << 16}
struct StxMatchJob { int a_off, b_off, na, nb, block0, pad_; long long nn_off; };
// a pair i < j: nn_f / nn_b: the results of i -> j / j -> i (-1: that direction has no job); out_off: the pair's first slot of the
// match arena (ni + nj slots: the union cannot be larger); p = i n + j
struct StxMatchPair { int i_off, j_off, ni, nj, p, pad_; long long nn_f, nn_b, out_off; };
int stx_launch_match_2nn(stx_ctx* ctx, const StxMatchJob* d_jobs, int njobs, int blocks, const uint32_t* d_desc, uint2* d_nn,
                         double compares, bool lds);
int stx_launch_match_union(stx_ctx* ctx, const StxMatchPair* d_pairs, int np, const uint2* d_nn, const double* d_pts, int ratio_T,
                           int* d_counts, int* d_matches, double* d_xyuv);
// model: STX_MATCH_MODEL_* (checked by the caller), the hypothesis function of both kernels
int stx_launch_match_ransac(stx_ctx* ctx, const StxMatchPair* d_pairs, int np, const int* d_counts, const double* d_xyuv, int iters,
                            double threshold_sq, uint32_t seed, int model, int* d_hyp);
int stx_launch_match_pick(stx_ctx* ctx, const StxMatchPair* d_pairs, int np, const int* d_counts, const double* d_xyuv, int iters,
                          double threshold_sq, uint32_t seed, int model, const int* d_hyp, int* d_pick, double* d_H, uint8_t* d_mask);
// ray bundle adjustment (stx_cameras.hip; host side in stx_cameras_host.cpp) ---------------------------------------------------------
// the edges of one adjustment, on the device for all its evaluations: cameras (i < j) per edge, the edges' first points (ascending,
// first 0, n_edges + 1 entries), the points x, y, u, v; variants / out: the blocks every evaluation writes and reads
constexpr int STX_RAY_LANES = 256;  // lanes of the ordered sum: the workgroup of ray_normal_equations
constexpr int STX_RAY_MAX_CAMERA_DOUBLES = 270, STX_RAY_MAX_SUMS = 120;  // of the widest adjustment (the reprojection's): a camera's variants, an edge's sums
struct stx_ray_problem {
    stx_ctx* ctx = nullptr;
    int n_edges = 0, min_cams = 0;  // min_cams: the largest camera an edge names, plus one
    long long total = 0;
    StxDevBlock d_edge_cams, d_offsets, d_pts, d_variants, d_out;
    StxEventTimer timer;  // start, launch, launch done, copy back queued: armed with the problem, destroyed with it (before the blocks)
};
// E, g[8], B upper triangle[36] of every edge -> d_out[45 n_edges]; start / stop (or null): recorded around the launch
int stx_launch_ray_normal_equations(stx_ctx* ctx, int n_edges, const int* d_edge_cams, const long long* d_offsets, const double* d_pts,
                                    const double* d_variants, double* d_out, hipEvent_t start, hipEvent_t stop);
// the same sums of the affine-partial residual; d_variants: 72 doubles per camera
int stx_launch_affine_normal_equations(stx_ctx* ctx, int n_edges, const int* d_edge_cams, const long long* d_offsets, const double* d_pts,
                                       const double* d_variants, double* d_out, hipEvent_t start, hipEvent_t stop);
// E, g[14], B upper triangle[105] of the reprojection residual -> d_out[120 n_edges]; d_variants: 270 doubles per camera; grid (edges, 3)
int stx_launch_reproj_normal_equations(stx_ctx* ctx, int n_edges, const int* d_edge_cams, const long long* d_offsets, const double* d_pts,
                                       const double* d_variants, double* d_out, hipEvent_t start, hipEvent_t stop);
// cv::resize(INTER_LINEAR_EXACT) u8 (next rows N2 / N3; stx_resize.hip); d_xt / d_yt: device tables of (offset, coeff1 | interior << 16)
int stx_launch_resize_exact(stx_ctx* ctx, const stx_buf* src, stx_buf* dst, const int* d_xt, const int* d_yt, bool dilate,
                            const stx_buf* andmask);
// the same for n images in one launch: device descriptors, one per image; the grid is the flat list of their STX_RESIZE_TW x
// STX_RESIZE_TH destination tiles (tile0: the image's first, ascending; tiles_x: tiles per tile row)
constexpr int STX_RESIZE_TW = 64, STX_RESIZE_TH = 4;
struct StxResizeItem {
    const uint8_t* src; long long sstride; uint8_t* dst; long long dstride;
    int sw, sh, dw, dh, c, tiles_x, tile0, pad_;
    double xscale, yscale;  // 1 / (dw / sw), 1 / (dh / sh) in double, as linear_exact_table takes them
};
int stx_launch_resize_exact_batch(stx_ctx* ctx, const StxResizeItem* d_items, int n, int total_tiles, double algo_bytes);
// conservative shrink of u8x1 validity masks over the same descriptors and tile list (c, xscale, yscale unused)
int stx_launch_mask_shrink_batch(stx_ctx* ctx, const StxResizeItem* d_items, int n, int total_tiles, double algo_bytes);
// device frame ingest (stx_ingest.hip; host side in stx_ingest_host.cpp) -----------------------------------------------------------
// A lane takes STX_INGEST_LANE_PX pixels of a row (RAW: as many 4-byte words of it; a row is then w BYTES), a workgroup 64 lanes x
// STX_INGEST_ROWS row units; a row unit is two rows of the 4:2:0 formats (one chroma pair serves its 2 x 2 block), one row otherwise.
// The grid is the flat list of the frames' tiles, as the batched resize's (tile0 ascending, first 0).
constexpr int STX_INGEST_LANE_PX = 4, STX_INGEST_ROWS = 4, STX_INGEST_TW = 64 * STX_INGEST_LANE_PX;
// kind: what the kernel does with a row (several STX_INGEST_* formats share one)
enum { STX_INGEST_K_COPY = 0, STX_INGEST_K_PACK3, STX_INGEST_K_PACK4, STX_INGEST_K_NV12, STX_INGEST_K_I420 };
// wide: bit p set = plane p is read in whole words (base and pitch multiples of 4 — 2 for the chroma planes of I420, read 2 bytes at a
// time); clear = byte by byte.  Decided per frame on the host, so the branch is uniform over a workgroup.  The destination is an image
// of the library's own: base and pitch are multiples of 64.
struct StxIngestItem {
    const uint8_t* p[3]; long long pitch[3]; uint8_t* dst; long long dstride;
    int w, h;       // pixels; COPY: bytes of a row
    int kind, wide, reverse;  // reverse: PACK3 / PACK4 swap the first and third channel
    int tiles_x, tile0, pad_;
};
struct StxIngestCoef { int yoff, yk, rv, gu, gv, bu; };
int stx_launch_ingest(stx_ctx* ctx, const StxIngestItem* d_items, int n, int total_tiles, const StxIngestCoef& coef, double algo_bytes);
// one plane of foreign memory: `rows` rows of `row_bytes` bytes, `pitch` bytes apart
struct StxForeignPlane { const uint8_t* p; long long pitch, row_bytes; int rows; };
// the plane is device memory of the context's device and lies, first byte to last, inside one allocation; row_bytes <= pitch <= 2^40.
// what / item name the caller in the message ("ingest" / "frame"), host_hint ends the message about host memory
int stx_check_foreign_plane(const stx_ctx* ctx, const char* what, const char* item, int index, int plane, const StxForeignPlane& P,
                            const char* host_hint);
// device frame emit (stx_emit.hip; host side in stx_emit_host.cpp): the mirror of ingest, with its lane and tile geometry
// (STX_INGEST_LANE_PX pixels of a row unit per lane — COPY: as many 4-byte words —, 64 lanes x STX_INGEST_ROWS row units per workgroup,
// a row unit is two rows of the 4:2:0 formats) and the flat tile list.
// kind: what the kernel does with a row unit
enum { STX_EMIT_K_COPY = 0, STX_EMIT_K_REV3, STX_EMIT_K_ALPHA, STX_EMIT_K_NV12, STX_EMIT_K_I420 };
// wide: which buffers are moved in whole words (base and pitch multiples of 4; 2 for the chroma planes of I420, stored 2 bytes at a
// time), decided per item on the host so that the branch is uniform over a workgroup; a clear bit moves bytes.
enum { STX_EMIT_WIDE_SRC = 1, STX_EMIT_WIDE_ALPHA = 2, STX_EMIT_WIDE_DST0 = 4 };  // plane p of the target: STX_EMIT_WIDE_DST0 << p
struct StxEmitItem {
    const uint8_t* src; long long sstride;
    const uint8_t* alpha; long long astride;  // ALPHA: null = the alpha byte is 255
    uint8_t* dst[3]; long long dpitch[3];
    int w, h;       // pixels; COPY: bytes of a row
    int kind, wide, reverse;  // reverse: ALPHA swaps the first and third channel
    int tiles_x, tile0, pad_;
};
// the 16-bit-fraction constants of tests/numpy_emit.py in (B, G, R) order; yoff: 16 or 0
struct StxEmitCoef { int ky[3], ku[3], kv[3], yoff; };
int stx_launch_emit(stx_ctx* ctx, const StxEmitItem* d_items, int n, int total_tiles, const StxEmitCoef& coef, double algo_bytes);
// lens rectification (stx_rectify.hip; host side in stx_rectify_host.cpp) -------------------------------------
// A wavefront owns one cell of the lens grid (STX_LENS_CELL x STX_LENS_CELL destination pixels: its four nodes are wave-uniform), a
// lane STX_RECTIFY_LANE_PX pixels of one row of it; a workgroup is STX_RECTIFY_TW / STX_LENS_CELL cells side by side.  The grid is the
// flat list of the images' tiles (tile0 ascending, first 0).
constexpr int STX_RECTIFY_LANE_PX = 4, STX_RECTIFY_TW = 64, STX_RECTIFY_TH = 16;
static_assert(STX_LENS_CELL * STX_LENS_CELL == 64 * STX_RECTIFY_LANE_PX && STX_RECTIFY_TH == STX_LENS_CELL, "a wavefront is one cell");
// the nodes of one camera in device memory: (sx, sy) in Q6 per node, ny rows of nx
struct stx_lens_map {
    stx_ctx* ctx = nullptr;
    int dst_w = 0, dst_h = 0, src_w = 0, src_h = 0, nx = 0, ny = 0;
    StxDevBlock d_nodes;
};
struct StxRectifyItem {
    const uint8_t* src; long long sstride;
    uint8_t* dst; long long dstride;
    uint8_t* mask; long long mstride;  // null: no mask wanted
    const int2* nodes;
    int nx, sw, sh, dw, dh, c, tiles_x, tile0;
};
int stx_launch_rectify(stx_ctx* ctx, const StxRectifyItem* d_items, int n, int total_tiles, int border, double algo_bytes);

int stx_launch_seam_resize_batch(stx_ctx* ctx, int n, const stx_buf* const* seams, const stx_buf* const* masks, stx_buf* const* dsts,
                                 const int* const* d_xt, const int* const* d_yt, uint8_t* const* tmp, const size_t* tstride);
// SeamFinder.resize of n images as ONE launch (coefficients made in the kernel, dilation in LDS); full_wh_xy0 as stx_seam_mask_resize_batch_sub
int stx_launch_seam_resize_lds(stx_ctx* ctx, int n, const stx_buf* const* seams, const stx_buf* const* masks, stx_buf* const* dsts,
                               const int* full_wh_xy0, bool* done);
// image-strip sharding (stx_strips.hip): pack the columns [x0, x0 + w) of n images + masks into n flat buffers (one launch per 16 strips)
int stx_launch_strip_pack(stx_ctx* ctx, int n, const stx_buf* const* imgs, const stx_buf* const* masks, const int* x0, const int* w,
                          stx_buf* const* dsts, const size_t* si, const size_t* sm, bool mask_bits);
int stx_launch_strip_bits_expand(stx_ctx* ctx, int n, const uint8_t* const* bits, const size_t* sm, stx_buf* const* masks);

// saturation of the L1 distance transform (OpenCV's 16.16 fixed point clamps at INT_MAX >> 2 = 8192.0f): the kernels clamp to it, the
// sharded feather blender sizes its halo by it (stx_debug_feather_dist_cap -> distributed.FEATHER_DIST_CAP, checked by a host test)
constexpr int STX_FEATHER_DIST_CAP = 8192;
constexpr int STX_DT_RC = 64;  // rows per chunk of the distance transform's column pass (stx_blend.hip: DT_RC)
// dt_rows_batch_kernel keeps a row's forward sweep in LDS, one 16-byte slot per 8 pixels over whole 512-pixel steps (2 bytes per column),
// and a workgroup takes 4, 2 or 1 rows, whichever fits STX_FEATHER_LDS_BYTES.  0 rows: the image is too wide for the kernel —
// stx_blend_feed_ex refuses it with stx_feather_refuse_width, so the launcher never meets one.  The widest image with a row per
// workgroup is STX_FEATHER_MAX_WIDTH (include/stitching_amd.h), which the assertion below holds to this arithmetic
constexpr int STX_FEATHER_LDS_BYTES = 65536;
constexpr int stx_feather_lds_pitch(int w) { return ((w + 511) / 512) * 64; }  // 16-byte slots per row
constexpr int stx_feather_rows_per_block(int w)
{
    return stx_feather_lds_pitch(w) * 16 * 4 <= STX_FEATHER_LDS_BYTES ? 4
         : stx_feather_lds_pitch(w) * 16 * 2 <= STX_FEATHER_LDS_BYTES ? 2
         : stx_feather_lds_pitch(w) * 16 <= STX_FEATHER_LDS_BYTES ? 1 : 0;
}
static_assert(stx_feather_rows_per_block(STX_FEATHER_MAX_WIDTH) == 1 && stx_feather_rows_per_block(STX_FEATHER_MAX_WIDTH + 1) == 0, "feather width limit");
// STX_OK, or the refusal of an image w columns wide: the one text for the limit
inline int stx_feather_refuse_width(int w)
{
    if (stx_feather_rows_per_block(w) > 0) return STX_OK;
    return stx_fail(STX_ERR_INVALID, "feed: the feather blender takes images up to %d columns wide, this one has %d", STX_FEATHER_MAX_WIDTH, w);
}
// feather blender as a deferred gather: device table of the fed images, in feed order
struct FeatherImg {
    const uint8_t* img; long long istride; int is_s16;
    const uint8_t* mask; long long mstride;
    int x, y, w, h;                 // rectangle inside the panorama roi
    uint16_t* dist; long long dstride; // L1 distance to the nearest zero of the mask, saturated at 8192; elements per row (multiple of 16)
    int* first; int* last; unsigned long long* zbits; int n_chunks;  // column-pass summaries (DT_RC rows per chunk): first / last zero row, zero rows as a bit set
};
struct FeatherGatherK {
    const FeatherImg* imgs; int n; int w, h; float sharpness;
    uint8_t* pano; long long pano_stride; uint8_t* pmask; long long pmask_stride; short* pano16; long long pano16_stride;
};
int stx_launch_feather_weights(stx_ctx* ctx, const FeatherImg* d_imgs, const FeatherImg* h_imgs, int n);
int stx_launch_feather_gather(stx_ctx* ctx, const FeatherGatherK& K, double algo_bytes);

// "no" blender as a deferred gather: device table of the fed images, in feed order
struct NoImg { const uint8_t* img; long long istride; const uint8_t* mask; long long mstride; int is_s16; int x, y, w, h; int mask_binary; };
struct NoGatherK {
    const NoImg* imgs; int n; int all_binary;  // all_binary: every mask holds only 0 / 255
    int w, h;
    uint8_t* pano; long long pano_stride; uint8_t* pmask; long long pmask_stride; short* pano16; long long pano16_stride;
};
int stx_launch_no_gather(stx_ctx* ctx, const NoGatherK& K, double algo_bytes);

// blender state (stx_blend_host.cpp; the strip sharding of stx_strips_host.cpp reads its geometry) ---------------------------------
struct stx_blender {
    stx_ctx* ctx = nullptr;
    int kind = 0, num_bands = 0;
    float sharpness = 0.02f;
    int rx = 0, ry = 0, rw = 0, rh = 0;  // dst_roi_ (padded for multiband)
    int fw = 0, fh = 0;                  // dst_roi_final_ size
    bool finished = false;
    // multiband (deferred gather)
    std::vector<StxMbImage> images;   // kept sorted by .order (the global feed order)
    std::vector<char> built;          // pyramid of images[i] exists (kind 0)
    std::vector<stx_buf*> held;
    std::vector<void*> pyr_allocs;
    std::vector<void*> wt_allocs;     // the weight pyramids wt[1..B] of the fed images and the occupancy arena: the part of a blender that
                                      // depends on the masks and the geometry alone; moved to `keep` at blend() when one is set
    stx_mb_weights* keep = nullptr;   // stx_blend_keep_weights: filled at blend() (one reference held until then)
    stx_mb_weights* adopted = nullptr;  // stx_blend_use_weights: the handle whose weights the images point to (one reference held);
                                      // the pyramids are then built without their weight half
    StxMbImage* d_all = nullptr;      // device copy of `images` as the pyramid pass uploaded it, while it still equals `images` (else null)
    bool d_all_resident = false;      // d_all is a resident copy of the adopted handle (mb_resident_table), not one of pyr_allocs
    StxMbImage* d_gather = nullptr;   // the device table the gathers of blend() ran on (one of pyr_allocs; mb_hand_over_weights records the cover from it)
    int band_x0 = 0, band_x1 = 0;     // columns of the final roi this blender produces (sharded blending)
    int next_order = 0;
    int pyr_mode = 0;                 // STX_PYRDOWN_* | lanes << 8, captured at stx_blend_create: one summation order per panorama
                                      // whatever stx_set_pyrdown_mode is called with between feed() and blend()
    // no: deferred gather over the fed images (stx_launch_no_gather)
    std::vector<NoImg> no_images;
    // feather: deferred gather as well (stx_launch_feather_weights / _gather)
    std::vector<FeatherImg> feather_images;
};
// weight pyramids that outlive their blender (stx_blend_keep_weights / stx_blend_use_weights) --------------------------------------
struct StxMbKept {  // what the weights of one fed image depend on, and the weights
    stx_buf* mask;  // (one reference held: the memory cannot be handed out again while the record compares pointers with it)
    const uint8_t* mask0; long long mask0_stride; int mask_binary, w1_f16;
    int iw, ih, ix, iy, fx, fy, fw, fh, left, top;
    float* wt[STX_MAX_BANDS + 1]; long long wt_stride[STX_MAX_BANDS + 1];
    uint8_t* occ[STX_MAX_BANDS + 1];
};
struct stx_mb_weights {
    stx_ctx* ctx = nullptr;
    std::atomic<int> refs{1};  // (Python finalizers may drop handles from any thread)
    int num_bands = 0, pyr_mode = 0;
    int rx = 0, ry = 0, rw = 0, rh = 0;
    std::vector<StxMbKept> images;  // in feed order; empty until the blender it was taken from has blended
    std::vector<void*> allocs;
    // the image search of the packed gathers, recorded once (levels 0 .. num_bands - 3, at most 64 images; table null: none): per level
    // the region and tile dimensions the table was made for — a blender whose level differs in any of them searches as ever.
    // 8 bytes per 512 x 2 tile (one of `allocs`)
    struct Cover { int x0, x1, y0, y1, tiles_x, tiles_y, band_rows; unsigned long long* table; };
    Cover cover[STX_MAX_BANDS + 1] = {};
    // device copies of the descriptor table (StxMbImage per image) of the blenders that adopted this handle, each with its host shadow:
    // the table is the rig's constants plus buffer addresses, and the context's caching allocator hands the same addresses out again
    // (the lowest free block of a size: stx_dev_alloc), in a cycle of a few sets where the caller holds results across panoramas.  A blender whose table equals a shadow byte for byte runs on
    // that copy without an upload; else the least recently used slot is overwritten in stream order (mb_resident_table).  The device
    // blocks are among `allocs`.
    struct Resident { StxMbImage* d = nullptr; std::vector<StxMbImage> shadow; unsigned long long used = 0; };
    static constexpr int kResidentSlots = 4;
    Resident resident[kResidentSlots];
    unsigned long long resident_clock = 0;
    // the finished panorama mask of the blend that filled the handle (one reference held; null: none): a function of the fed masks alone,
    // so an adopted blender whose output region is [pmask_x0, pmask_x1) x [0, pmask_h) hands this buffer out, shared and read-only, and its
    // level-0 gather stores no mask (mb_finish).  w * h bytes of the panorama.
    stx_buf* pmask = nullptr;
    int pmask_x0 = 0, pmask_x1 = 0, pmask_h = 0;
};
void stx_mb_weights_release(stx_mb_weights* w);
// MultiBandBlender::feed geometry: the feed rectangle (tl_new .. br_new) relative to the padded roi
void mb_feed_rect(const stx_blender* b, int w, int h, int tlx, int tly, int* fx, int* fy, int* fw, int* fh);
// level-0 column range [sx0, sx1) of the contribution an image fed at [fx, fx + fw) owes the owner of the columns [bx0, bx1)
bool mb_contrib_range(const stx_blender* b, int fx, int fw, int bx0, int bx1, int* sx0, int* sx1);
