// stx_image_host.cpp — device images (stx_buf): allocation, reference counting, views, transfers from / to host memory, pinned host
// memory, timelapse frames.
#include <algorithm>
#include <cstring>
#include <memory>

#include "stx_internal.h"

// ---------------------------------------------------------------------------------------------
// device images
// ---------------------------------------------------------------------------------------------
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int stx_buf_new(stx_ctx* ctx, int w, int h, int c, int elem, stx_buf** out)
{
    if (w <= 0 || h <= 0 || c <= 0 || c > 4 || elem < STX_U8 || elem > STX_F32)
        return stx_fail(STX_ERR_INVALID, "bad image geometry %dx%dx%d elem %d", w, h, c, elem);
    std::unique_ptr<stx_buf> b(new stx_buf());
    b->ctx = ctx;
    b->w = w; b->h = h; b->c = c; b->elem = elem;
    // rows are 64-byte aligned and hold a whole number of 8-pixel groups (kernels store 4 or 8 px per lane)
    b->stride = align_up(align_up((size_t)w, 8) * c * stx_elem_bytes(elem), 64);
    // 64 bytes in front and 64 behind: the gather kernels read whole aligned windows around the first / last pixels of a row —
    // also where an 8-pixel group of a lane lies partly left of the image (up to 21 bytes before row 0), see mb_level0_pk_kernel
    STX_TRY(stx_dev_alloc(ctx, STX_BUF_FRONT_PAD + b->stride * h + 64, &b->base));
    b->ptr = (uint8_t*)b->base + STX_BUF_FRONT_PAD;
    *out = b.release();
    return STX_OK;
}

void stx_buf_retain(stx_buf* b) { b->refs.fetch_add(1); }

void stx_buf_release(stx_buf* b)
{
    if (!b) return;
    if (b->refs.fetch_sub(1) != 1) return;
    if (b->validity) stx_buf_release(b->validity);
    if (b->parent) stx_buf_release(b->parent);
    else stx_dev_free(b->ctx, b->base);
    delete b;
}

STX_EXPORT int stx_buf_alloc(stx_ctx* ctx, int w, int h, int channels, int elem, stx_buf** out)
{
    if (!ctx || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    return stx_buf_new(ctx, w, h, channels, elem, out);
}

// true when [p, p + bytes) is page-locked host memory known to the runtime (stx_host_alloc, hipHostMalloc, hipHostRegister)
static bool is_pinned_host(const void* p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an unregistered pointer is an expected answer, not a sticky error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

static int buf_from_host(stx_ctx* ctx, const void* host, size_t host_stride, int w, int h, int channels, int elem, bool wait,
                         stx_buf** out)
{
    if (!ctx || !host || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(ctx));
    size_t row = (size_t)w * channels * stx_elem_bytes(elem);
    if (host_stride < row) return stx_fail(STX_ERR_INVALID, "host stride %zu < row bytes %zu", host_stride, row);
    StxBufRef b;
    STX_TRY(stx_buf_new(ctx, w, h, channels, elem, &b));
    hipError_t e = hipMemcpy2DAsync(b->ptr, b->stride, host, host_stride, row, h, hipMemcpyHostToDevice, ctx->stream);
    // the host buffer is only borrowed for this call — unless the caller asked for the asynchronous form and the
    // memory is page-locked (a pageable source is staged by the runtime; waiting keeps that case simple and safe)
    if (e == hipSuccess && (wait || !is_pinned_host(host))) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return stx_fail(STX_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
    if (channels == 1 && elem == STX_U8) {  // masks: remember whether every byte is 0 or 255 (packed blend kernels)
        bool binary = true;
        for (int y = 0; y < h && binary; y++) {
            const uint8_t* r = (const uint8_t*)host + (size_t)y * host_stride;
            unsigned bad = 0;
            for (int x = 0; x < w; x++) bad |= (unsigned)((r[x] + 1) & 0xfe);  // 0 -> 0, 255 -> 0, else nonzero
            binary = bad == 0;
        }
        b->mask_binary = binary ? 1 : 0;
    }
    *out = b.release();
    return STX_OK;
}

STX_EXPORT int stx_buf_from_host(stx_ctx* ctx, const void* host, size_t host_stride, int w, int h, int channels,
                                 int elem, stx_buf** out)
{
    return buf_from_host(ctx, host, host_stride, w, h, channels, elem, true, out);
}

STX_EXPORT int stx_buf_from_host_async(stx_ctx* ctx, const void* host, size_t host_stride, int w, int h, int channels,
                                       int elem, stx_buf** out)
{
    return buf_from_host(ctx, host, host_stride, w, h, channels, elem, false, out);
}

// Page-locked host memory for the frames a decoder produces and for read-backs: copies from / to it run at PCIe
// rate without the driver's staging through pageable memory (next row N3: staging of the source frames).
STX_EXPORT int stx_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0) return stx_fail(STX_ERR_INVALID, "bad argument");
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return stx_fail(STX_ERR_OOM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    *out = p;
    return STX_OK;
}

STX_EXPORT int stx_host_free(void* p)
{
    if (p) hipHostFree(p);
    return STX_OK;
}

static int buf_to_host(const stx_buf* buf, void* host, size_t host_stride, bool wait)
{
    if (!buf || !host) return stx_fail(STX_ERR_INVALID, "null argument");
    STX_TRY(stx_set_device(buf->ctx));
    size_t row = (size_t)buf->w * buf->c * stx_elem_bytes(buf->elem);
    if (host_stride < row) return stx_fail(STX_ERR_INVALID, "host stride %zu < row bytes %zu", host_stride, row);
    STX_HIP(hipMemcpy2DAsync(host, host_stride, buf->ptr, buf->stride, row, buf->h, hipMemcpyDeviceToHost,
                             buf->ctx->stream));
    if (wait || !is_pinned_host(host)) STX_HIP(hipStreamSynchronize(buf->ctx->stream));
    return STX_OK;
}

STX_EXPORT int stx_buf_to_host(const stx_buf* buf, void* host, size_t host_stride) { return buf_to_host(buf, host, host_stride, true); }

STX_EXPORT int stx_buf_to_host_async(const stx_buf* buf, void* host, size_t host_stride)
{
    return buf_to_host(buf, host, host_stride, false);
}

// a new handle onto the rectangle (x, y, w, h) of buf's pixels (checked by the caller); holds a reference on buf
static stx_buf* view_of(const stx_buf* buf, int x, int y, int w, int h)
{
    stx_buf* root = const_cast<stx_buf*>(buf);
    stx_buf* v = new stx_buf();
    v->ctx = buf->ctx;
    v->base = buf->base;
    v->ptr = buf->ptr + (size_t)y * buf->stride + (size_t)x * buf->c * stx_elem_bytes(buf->elem);
    v->w = w; v->h = h; v->c = buf->c; v->elem = buf->elem;
    v->stride = buf->stride;
    v->parent = root;
    v->mask_binary = buf->mask_binary;
    stx_buf_retain(root);
    return v;
}

STX_EXPORT int stx_buf_view(const stx_buf* buf, int x, int y, int w, int h, stx_buf** out)
{
    if (!buf || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    if (x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > buf->w || y + h > buf->h)
        return stx_fail(STX_ERR_INVALID, "view (%d,%d,%d,%d) outside %dx%d", x, y, w, h, buf->w, buf->h);
    stx_buf* v = view_of(buf, x, y, w, h);
    if (buf->validity) v->validity = view_of(buf->validity, x, y, w, h);  // a frame's view carries the matching view of its mask
    *out = v;
    return STX_OK;
}

STX_EXPORT int stx_buf_with_validity(const stx_buf* img, const stx_buf* mask, stx_buf** out)
{
    if (!img || !mask || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    if (img->elem != STX_U8 || img->c != 3) return stx_fail(STX_ERR_INVALID, "a validity mask belongs to a u8x3 frame");
    if (mask->elem != STX_U8 || mask->c != 1) return stx_fail(STX_ERR_INVALID, "a validity mask is u8 with 1 channel");
    if (mask->w != img->w || mask->h != img->h)
        return stx_fail(STX_ERR_INVALID, "validity mask of %dx%d on a frame of %dx%d", mask->w, mask->h, img->w, img->h);
    if (mask->ctx != img->ctx) return stx_fail(STX_ERR_INVALID, "frame and validity mask belong to different contexts");
    if (img->validity) return stx_fail(STX_ERR_INVALID, "the frame already carries a validity mask");
    stx_buf* v = view_of(img, 0, 0, img->w, img->h);
    v->validity = const_cast<stx_buf*>(mask);
    stx_buf_retain(v->validity);
    *out = v;
    return STX_OK;
}

STX_EXPORT int stx_buf_validity(const stx_buf* buf, stx_buf** out)
{
    if (!buf || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    *out = buf->validity ? view_of(buf->validity, 0, 0, buf->validity->w, buf->validity->h) : nullptr;
    return STX_OK;
}

STX_EXPORT int stx_buf_info(const stx_buf* buf, int64_t info[6])
{
    if (!buf || !info) return stx_fail(STX_ERR_INVALID, "null argument");
    info[0] = buf->w; info[1] = buf->h; info[2] = buf->c; info[3] = buf->elem;
    info[4] = (int64_t)buf->stride; info[5] = buf->ctx->device;
    return STX_OK;
}

STX_EXPORT int stx_buf_flags(const stx_buf* buf, int* out_flags)
{
    if (!buf || !out_flags) return stx_fail(STX_ERR_INVALID, "null argument");
    *out_flags = buf->mask_binary ? STX_CONTRIB_U8_BINARY : 0;
    return STX_OK;
}

STX_EXPORT int stx_buf_device_ptr(const stx_buf* buf, void** out)
{
    if (!buf || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    *out = buf->ptr;
    return STX_OK;
}

STX_EXPORT int stx_buf_free(stx_buf* buf)
{
    stx_buf_release(buf);
    return STX_OK;
}

STX_EXPORT int stx_timelapse_frame(stx_ctx* ctx, const stx_buf* img, int tlx, int tly, const int dst_roi_xywh[4], stx_buf** out_frame)
{
    if (!ctx || !img || !dst_roi_xywh || !out_frame) return stx_fail(STX_ERR_INVALID, "null argument");
    if (img->ctx != ctx) return stx_fail(STX_ERR_INVALID, "image belongs to another context");
    const int rx = dst_roi_xywh[0], ry = dst_roi_xywh[1], rw = dst_roi_xywh[2], rh = dst_roi_xywh[3];
    if (rw <= 0 || rh <= 0) return stx_fail(STX_ERR_INVALID, "empty timelapse roi %dx%d", rw, rh);
    STX_TRY(stx_set_device(ctx));
    StxBufRef f;
    STX_TRY(stx_buf_new(ctx, rw, rh, img->c, img->elem, &f));
    // Timelapser::process: dst_.setTo(0); img.copyTo(dst_(Rect(tl - dst_roi_.tl(), img.size()))), clipped to the roi
    hipError_t e = hipMemsetAsync(f->ptr, 0, f->stride * (size_t)rh, ctx->stream);
    const int x0 = std::max(tlx, rx), y0 = std::max(tly, ry);
    const int x1 = std::min(tlx + img->w, rx + rw), y1 = std::min(tly + img->h, ry + rh);
    const size_t px = (size_t)img->c * stx_elem_bytes(img->elem);
    if (e == hipSuccess && x1 > x0 && y1 > y0)
        e = hipMemcpy2DAsync(f->ptr + (size_t)(y0 - ry) * f->stride + (size_t)(x0 - rx) * px, f->stride,
                             img->ptr + (size_t)(y0 - tly) * img->stride + (size_t)(x0 - tlx) * px, img->stride,
                             (size_t)(x1 - x0) * px, (size_t)(y1 - y0), hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) return stx_fail(STX_ERR_HIP, "timelapse frame: %s", hipGetErrorString(e));
    *out_frame = f.release();
    return STX_OK;
}
