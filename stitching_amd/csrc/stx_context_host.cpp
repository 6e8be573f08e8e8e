// stx_context_host.cpp — error strings, the context (streams, stream-ordered caching allocator, pinned upload ring) and the profiler.
#include <algorithm>
#include <cstring>

#include "stx_internal.h"

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void stx_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int stx_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

STX_EXPORT const char* stx_last_error(void) { return g_err; }
STX_EXPORT int stx_version(void) { return STX_VERSION; }

STX_EXPORT int stx_device_count(int* out_n)
{
    if (!out_n) return stx_fail(STX_ERR_INVALID, "out_n is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_n = 0;
        return stx_fail(STX_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out_n = n;
    return STX_OK;
}

// ---------------------------------------------------------------------------------------------
// context, allocator
// ---------------------------------------------------------------------------------------------
int stx_set_device(stx_ctx* ctx)
{
    STX_HIP(hipSetDevice(ctx->device));
    return STX_OK;
}

STX_EXPORT int stx_ctx_create(int device, stx_ctx** out)
{
    if (!out) return stx_fail(STX_ERR_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    STX_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return stx_fail(STX_ERR_INVALID, "device %d out of range (have %d)", device, n);
    STX_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    STX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return stx_fail(STX_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 (MI355X) only", device,
                        prop.gcnArchName);
    stx_ctx* ctx = new stx_ctx();
    ctx->device = device;
    ctx->pinned_bytes = 1 << 16;
    ctx->stage_bytes = 1 << 20;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc(&ctx->pinned, ctx->pinned_bytes, hipHostMallocCoherent | hipHostMallocMapped);  // kernels write ROI results into it
    if (e == hipSuccess) memset(ctx->pinned, 0, ctx->pinned_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->stage, ctx->stage_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&ctx->aux_scratch, ctx->pinned_bytes);
    if (e != hipSuccess) {
        stx_ctx_destroy(ctx);  // releases whatever was created
        return stx_fail(STX_ERR_HIP, "context set-up failed: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return STX_OK;
}

STX_EXPORT int stx_ctx_sync(stx_ctx* ctx)
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    STX_TRY(stx_set_device(ctx));
    STX_HIP(hipStreamSynchronize(ctx->stream));
    return STX_OK;
}

STX_EXPORT int stx_ctx_destroy(stx_ctx* ctx)
{
    if (!ctx) return STX_OK;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) hipStreamSynchronize(ctx->aux_stream);
    for (auto& kv : ctx->block_size) hipFree(kv.first);
    for (auto& p : ctx->prof_pending) { hipEventDestroy(p.start); hipEventDestroy(p.stop); }
    for (auto e : ctx->event_pool) hipEventDestroy(e);
    for (auto e : ctx->marks) if (e) hipEventDestroy(e);
    if (ctx->pinned) hipHostFree(ctx->pinned);
    if (ctx->stage) hipHostFree(ctx->stage);
    for (hipEvent_t e : ctx->stage_ev) if (e) hipEventDestroy(e);
    if (ctx->aux_scratch) hipFree(ctx->aux_scratch);
    if (ctx->aux_stream) hipStreamDestroy(ctx->aux_stream);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return STX_OK;
}

static size_t bucket_of(size_t bytes)
{
    if (bytes < 256) return 256;
    if (bytes >= (1u << 20)) return (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    size_t b = 256;
    while (b < bytes) b <<= 1;
    return b;
}

// Stream-ordered caching allocator: every kernel of a ctx runs on ctx->stream, so a block
// returned here can be handed out again immediately — its next user is enqueued after its last.
int stx_dev_alloc(stx_ctx* ctx, size_t bytes, void** out)
{
    size_t b = bucket_of(bytes + 64);  // +64: kernels may over-read up to 12 bytes past a row
    std::lock_guard<std::mutex> lock(ctx->alloc_mutex);
    auto it = ctx->free_blocks.find(b);
    if (it != ctx->free_blocks.end() && !it->second.empty()) {
        // the free block with the LOWEST address, not the one freed last: which block a request gets then depends on the set of free
        // blocks alone, never on the order they came back in (Python finalizers, a blender's release) — the n-th panorama of a rig is
        // handed the addresses of the (n - 1)-th, which the resident descriptor tables of stx_mb_weights live on.  The lists are short.
        std::vector<void*>& v = it->second;
        size_t lo = 0;
        for (size_t i = 1; i < v.size(); i++)
            if (v[i] < v[lo]) lo = i;
        *out = v[lo];
        v[lo] = v.back();
        v.pop_back();
        return STX_OK;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, b);
    if (e != hipSuccess) {
        // release the cache and retry once
        hipStreamSynchronize(ctx->stream);
        for (auto& kv : ctx->free_blocks) {
            for (void* q : kv.second) { ctx->bytes_allocated -= ctx->block_size[q]; ctx->block_size.erase(q); hipFree(q); }
            kv.second.clear();
        }
        e = hipMalloc(&p, b);
        if (e != hipSuccess) return stx_fail(STX_ERR_OOM, "hipMalloc(%zu) failed: %s", b, hipGetErrorString(e));
    }
    ctx->block_size[p] = b;
    ctx->bytes_allocated += b;
    *out = p;
    return STX_OK;
}

void stx_dev_free(stx_ctx* ctx, void* p)
{
    if (!p) return;
    std::lock_guard<std::mutex> lock(ctx->alloc_mutex);
    auto it = ctx->block_size.find(p);
    if (it == ctx->block_size.end()) return;
    ctx->free_blocks[it->second].push_back(p);
}

int stx_stage_upload(stx_ctx* ctx, void* d, const void* h, size_t bytes)
{
    if (bytes == 0) return STX_OK;
    const size_t seg = ctx->stage_bytes / STX_STAGE_SEGS;
    if (bytes > seg) {  // larger than a segment of the ring: plain synchronous copy
        STX_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        STX_HIP(hipStreamSynchronize(ctx->stream));
        return STX_OK;
    }
    size_t off = ctx->stage_off;
    int cur = ctx->stage_seg;  // the segment that holds the previous upload
    if (off + bytes > (size_t)(cur + 1) * seg) {  // does not fit into the rest of it: on to the next segment
        const int next = (cur + 1) % STX_STAGE_SEGS;
        if (!ctx->stage_ev[cur]) STX_HIP(hipEventCreateWithFlags(&ctx->stage_ev[cur], hipEventDisableTiming));
        STX_HIP(hipEventRecord(ctx->stage_ev[cur], ctx->stream));  // behind the last copy out of segment `cur`
        ctx->stage_ev_set[cur] = true;
        if (ctx->stage_ev_set[next]) STX_HIP(hipEventSynchronize(ctx->stage_ev[next]));  // its copies of the previous lap
        off = (size_t)next * seg;
        cur = next;
    }
    ctx->stage_seg = cur;
    uint8_t* slot = ctx->stage + off;
    memcpy(slot, h, bytes);
    ctx->stage_off = off + ((bytes + 255) & ~(size_t)255);
    STX_HIP(hipMemcpyAsync(d, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
    return STX_OK;
}

int upload_small(stx_ctx* ctx, const void* h, size_t bytes, StxDevBlock* d_out)
{
    StxDevBlock d;
    STX_TRY(stx_dev_alloc(ctx, std::max<size_t>(bytes, 4), &d));
    STX_TRY(stx_stage_upload(ctx, d.get(), h, bytes));
    *d_out = std::move(d);
    return STX_OK;
}

// ---------------------------------------------------------------------------------------------
// profiler: HIP events around each launch, on the stream the kernel is launched on
// ---------------------------------------------------------------------------------------------
static hipEvent_t take_event(stx_ctx* ctx)
{
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

StxProfScope::StxProfScope(stx_ctx* c, const char* name, double algo_bytes, hipStream_t on, bool attach)
    : ctx(c), stream(on ? on : c->stream), attached(attach)
{
    if (!ctx->prof_on) return;
    auto it = ctx->prof_index.find(name);
    int idx;
    if (it == ctx->prof_index.end()) {
        idx = (int)ctx->prof.size();
        ctx->prof.push_back(StxProfEntry());
        ctx->prof.back().name = name;
        ctx->prof_index[name] = idx;
    } else {
        idx = it->second;
    }
    ctx->prof[idx].calls += 1;
    ctx->prof[idx].algo_bytes += algo_bytes;
    StxPendingEvent pe;
    pe.start = take_event(ctx);
    pe.stop = take_event(ctx);
    pe.entry = idx;
    if (!attached) hipEventRecord(pe.start, stream);
    ctx->prof_pending.push_back(pe);
    pending = (int)ctx->prof_pending.size() - 1;
}

StxProfScope::~StxProfScope()
{
    if (pending >= 0 && !attached) hipEventRecord(ctx->prof_pending[pending].stop, stream);
}

hipEvent_t StxProfScope::start() const { return pending >= 0 ? ctx->prof_pending[pending].start : nullptr; }
hipEvent_t StxProfScope::stop() const { return pending >= 0 ? ctx->prof_pending[pending].stop : nullptr; }

static void prof_collect(stx_ctx* ctx)
{
    if (ctx->prof_pending.empty()) return;
    hipStreamSynchronize(ctx->stream);
    hipStreamSynchronize(ctx->aux_stream);  // the ROI pass is bracketed on the side stream it runs on
    for (auto& pe : ctx->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.start, pe.stop) == hipSuccess) ctx->prof[pe.entry].total_ms += ms;
        ctx->event_pool.push_back(pe.start);
        ctx->event_pool.push_back(pe.stop);
    }
    ctx->prof_pending.clear();
}

STX_EXPORT int stx_prof_enable(stx_ctx* ctx, int on)
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    STX_TRY(stx_set_device(ctx));
    if (!on) prof_collect(ctx);
    ctx->prof_on = on != 0;
    return STX_OK;
}

STX_EXPORT int stx_prof_reset(stx_ctx* ctx)
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    STX_TRY(stx_set_device(ctx));
    prof_collect(ctx);
    ctx->prof.clear();
    ctx->prof_index.clear();
    return STX_OK;
}

STX_EXPORT int stx_prof_count(stx_ctx* ctx, int* out_n)
{
    if (!ctx || !out_n) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    prof_collect(ctx);
    *out_n = (int)ctx->prof.size();
    return STX_OK;
}

STX_EXPORT int stx_prof_get(stx_ctx* ctx, int index, char* name, int name_cap, int64_t* calls, double* total_ms,
                            double* algo_bytes)
{
    if (!ctx) return stx_fail(STX_ERR_INVALID, "ctx is null");
    if (index < 0 || index >= (int)ctx->prof.size()) return stx_fail(STX_ERR_INVALID, "profile index out of range");
    const StxProfEntry& e = ctx->prof[index];
    if (name && name_cap > 0) {
        strncpy(name, e.name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (calls) *calls = e.calls;
    if (total_ms) *total_ms = e.total_ms;
    if (algo_bytes) *algo_bytes = e.algo_bytes;
    return STX_OK;
}

STX_EXPORT int stx_mark(stx_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= 16) return stx_fail(STX_ERR_INVALID, "bad mark slot");
    STX_TRY(stx_set_device(ctx));
    if (!ctx->marks[slot]) STX_HIP(hipEventCreate(&ctx->marks[slot]));
    STX_HIP(hipEventRecord(ctx->marks[slot], ctx->stream));
    return STX_OK;
}

STX_EXPORT int stx_mark_elapsed_ms(stx_ctx* ctx, int a, int b, double* out_ms)
{
    if (!ctx || a < 0 || a >= 16 || b < 0 || b >= 16 || !out_ms || !ctx->marks[a] || !ctx->marks[b])
        return stx_fail(STX_ERR_INVALID, "bad mark slots");
    STX_TRY(stx_set_device(ctx));
    STX_HIP(hipEventSynchronize(ctx->marks[b]));
    float ms = 0.f;
    STX_HIP(hipEventElapsedTime(&ms, ctx->marks[a], ctx->marks[b]));
    *out_ms = ms;
    return STX_OK;
}
