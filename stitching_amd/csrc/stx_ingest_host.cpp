// stx_ingest_host.cpp — device frame ingest (stx_ingest): validation of foreign device memory, the descriptor table, ordering after
// the producer's stream.  The kernel is in stx_ingest.hip; DESIGN.md section 20.
#include <cstring>

#include "stx_internal.h"

namespace {
// the usual 8-bit-fraction roundings of the BT.601 / BT.709 matrices: {yoff, yk, rv, gu, gv, bu} by [matrix][range]
constexpr StxIngestCoef kCoef[2][2] = {{{16, 298, 409, 100, 208, 516}, {0, 256, 359, 88, 183, 454}},
                                       {{16, 298, 459, 55, 136, 541}, {0, 256, 403, 48, 120, 475}}};
constexpr long long kMaxPitch = 1ll << 40;  // rows * pitch stays far inside 64 bits

using Plane = StxForeignPlane;

bool aligned(const Plane& P, int a) { return ((uintptr_t)P.p % (uintptr_t)a) == 0 && P.pitch % a == 0; }
}  // namespace

int stx_check_foreign_plane(const stx_ctx* ctx, const char* what, const char* item, int index, int plane, const StxForeignPlane& P,
                            const char* host_hint)
{
    if (!P.p) return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d is null", what, item, index, plane);
    if (P.pitch < P.row_bytes || P.pitch > kMaxPitch)
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d has a pitch of %lld bytes for rows of %lld", what, item, index, plane, P.pitch,
                        P.row_bytes);
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    hipError_t e = hipPointerGetAttributes(&a, P.p);
    if (e != hipSuccess) (void)hipGetLastError();  // an unknown pointer is an answer, not a sticky error
    if (e != hipSuccess || a.type == hipMemoryTypeUnregistered || a.type == hipMemoryTypeHost)
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d (%p) is host memory: %s", what, item, index, plane, (const void*)P.p, host_hint);
    if (a.isManaged || a.type == hipMemoryTypeManaged)
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d (%p) is managed memory, which is not taken", what, item, index, plane,
                        (const void*)P.p);
    if (a.type != hipMemoryTypeDevice)
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d (%p) is not linear device memory", what, item, index, plane, (const void*)P.p);
    if (a.device != ctx->device)
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d lives on device %d, the context on device %d", what, item, index, plane, a.device,
                        ctx->device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)P.p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d (%p) belongs to no allocation the runtime knows", what, item, index, plane,
                        (const void*)P.p);
    }
    const unsigned long long first = (unsigned long long)(uintptr_t)P.p, end = (unsigned long long)(uintptr_t)base + size;
    const unsigned long long bytes = (unsigned long long)(P.rows - 1) * (unsigned long long)P.pitch + (unsigned long long)P.row_bytes;
    if (first < (unsigned long long)(uintptr_t)base || first >= end || bytes > end - first)
        return stx_fail(STX_ERR_INVALID, "%s: %s %d plane %d claims %llu bytes, its allocation holds %llu from there", what, item, index, plane,
                        bytes, first < end ? end - first : 0ull);
    return STX_OK;
}

STX_EXPORT int stx_ingest(stx_ctx* ctx, int n, const stx_foreign_frame* frames, int matrix, int range, void* producer_stream, int has_stream,
                          stx_buf** out)
{
    if (!ctx || !frames || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    if (n <= 0) return stx_fail(STX_ERR_INVALID, "ingest of %d frames", n);
    if (matrix < STX_INGEST_BT601 || matrix > STX_INGEST_BT709 || range < STX_INGEST_LIMITED || range > STX_INGEST_FULL)
        return stx_fail(STX_ERR_INVALID, "ingest: matrix %d / range %d", matrix, range);
    STX_TRY(stx_set_device(ctx));
    std::vector<StxIngestItem> items((size_t)n);
    std::vector<int> out_c((size_t)n), out_elem((size_t)n);
    long long tiles = 0;
    double bytes = 0.0;
    for (int i = 0; i < n; i++) {
        const stx_foreign_frame& F = frames[i];
        if (F.w < 1 || F.h < 1 || F.w > STX_INGEST_MAX_SIDE || F.h > STX_INGEST_MAX_SIDE)
            return stx_fail(STX_ERR_INVALID, "ingest: frame %d is %dx%d, images are 1 .. %d on a side", i, F.w, F.h, STX_INGEST_MAX_SIDE);
        const bool raw = F.format == STX_INGEST_RAW;
        if (F.format < STX_INGEST_RAW || F.format > STX_INGEST_I420) return stx_fail(STX_ERR_INVALID, "ingest: frame %d has format %d", i, F.format);
        if (F.elem < STX_U8 || F.elem > STX_F32 || F.channels < 1 || F.channels > 4)
            return stx_fail(STX_ERR_INVALID, "ingest: frame %d has %d channels of element type %d", i, F.channels, F.elem);
        const int want_c = raw ? F.channels : (F.format == STX_INGEST_BGR || F.format == STX_INGEST_RGB) ? 3
                         : (F.format == STX_INGEST_BGRA || F.format == STX_INGEST_RGBA) ? 4 : 1;
        if (!raw && (F.channels != want_c || F.elem != STX_U8))
            return stx_fail(STX_ERR_INVALID, "ingest: frame %d: format %d takes u8 with %d channel(s), got %d channel(s) of element type %d", i, F.format,
                            want_c, F.channels, F.elem);
        const int cw = (F.w + 1) / 2, ch = (F.h + 1) / 2;  // chroma planes of the 4:2:0 formats: the ceiling sizes
        Plane P[3];
        int np = 1;
        P[0] = Plane{(const uint8_t*)F.plane[0], F.pitch[0], (long long)F.w * F.channels * stx_elem_bytes(F.elem), F.h};
        if (F.format == STX_INGEST_NV12) { P[1] = Plane{(const uint8_t*)F.plane[1], F.pitch[1], 2ll * cw, ch}; np = 2; }
        if (F.format == STX_INGEST_I420) {
            P[1] = Plane{(const uint8_t*)F.plane[1], F.pitch[1], cw, ch};
            P[2] = Plane{(const uint8_t*)F.plane[2], F.pitch[2], cw, ch};
            np = 3;
        }
        for (int p = 0; p < np; p++) STX_TRY(stx_check_foreign_plane(ctx, "ingest", "frame", i, p, P[p], "host arrays are uploaded with from_numpy"));
        StxIngestItem& K = items[i];
        K = StxIngestItem{};
        for (int p = 0; p < np; p++) { K.p[p] = P[p].p; K.pitch[p] = P[p].pitch; }
        K.w = F.w; K.h = F.h;
        out_c[i] = 3; out_elem[i] = STX_U8;
        int units = F.w, row_units = F.h;  // along x: pixels (COPY: 4-byte words); along y: rows (4:2:0: row pairs)
        const double px = (double)F.w * F.h;
        switch (F.format) {
        case STX_INGEST_RAW: case STX_INGEST_BGR: case STX_INGEST_GRAY:
            K.kind = STX_INGEST_K_COPY; K.w = (int)P[0].row_bytes; units = (K.w + 3) / 4;
            out_c[i] = F.channels; out_elem[i] = F.elem;
            K.wide = aligned(P[0], 4) ? 1 : 0;
            bytes += 2.0 * (double)P[0].row_bytes * F.h;
            break;
        case STX_INGEST_RGB: case STX_INGEST_BGRA: case STX_INGEST_RGBA:
            K.kind = F.channels == 3 ? STX_INGEST_K_PACK3 : STX_INGEST_K_PACK4;
            K.reverse = F.format != STX_INGEST_BGRA;
            K.wide = aligned(P[0], 4) ? 1 : 0;
            bytes += px * (F.channels + 3);
            break;
        case STX_INGEST_NV12:
            K.kind = STX_INGEST_K_NV12; row_units = ch;
            K.wide = (aligned(P[0], 4) ? 1 : 0) | (aligned(P[1], 4) ? 2 : 0);
            bytes += px * 4.0 + 2.0 * cw * ch;
            break;
        default:
            K.kind = STX_INGEST_K_I420; row_units = ch;
            K.wide = (aligned(P[0], 4) ? 1 : 0) | (aligned(P[1], 2) ? 2 : 0) | (aligned(P[2], 2) ? 4 : 0);
            bytes += px * 4.0 + 2.0 * cw * ch;
            break;
        }
        K.tiles_x = (units + STX_INGEST_TW - 1) / STX_INGEST_TW;
        K.tile0 = (int)tiles;
        tiles += (long long)K.tiles_x * ((row_units + STX_INGEST_ROWS - 1) / STX_INGEST_ROWS);
        if (tiles > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "ingest of more than 2^31 tiles");
    }
    // nothing was allocated or queued up to here
    std::vector<StxBufRef> dsts((size_t)n);
    for (int i = 0; i < n; i++) {
        STX_TRY(stx_buf_new(ctx, frames[i].w, frames[i].h, out_c[i], out_elem[i], &dsts[i]));
        items[i].dst = dsts[i]->ptr; items[i].dstride = (long long)dsts[i]->stride;
        dsts[i]->mask_binary = 0;  // nothing is known about a foreign mask
    }
    StxDevBlock d_items;
    STX_TRY(upload_small(ctx, items.data(), items.size() * sizeof(StxIngestItem), &d_items));
    if (has_stream) {  // after whatever the producer has queued: an event there, waited for by the context's stream — no host wait
        // the protocol's handle 1, the legacy default stream, is the runtime's null stream (the runtime takes no handle of value 1:
        // hipEventRecord on it crashed); 2 is hipStreamPerThread's own value
        hipStream_t producer = (uintptr_t)producer_stream == 1 ? nullptr : (hipStream_t)producer_stream;
        STX_TRY(stx_stream_wait(ctx->stream, producer, "ingest: ordering after the producer's stream"));
    }
    STX_TRY(stx_launch_ingest(ctx, (const StxIngestItem*)d_items.get(), n, (int)tiles, kCoef[matrix][range], bytes));
    for (int i = 0; i < n; i++) out[i] = dsts[i].release();
    return STX_OK;  // the descriptor block goes back here: stream-ordered reuse
}
