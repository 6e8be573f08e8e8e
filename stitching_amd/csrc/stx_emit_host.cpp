// stx_emit_host.cpp — device frame emit (stx_emit): validation of the caller's target memory, the descriptor table, ordering against
// the consumer's stream.  The kernel is in stx_emit.hip; DESIGN.md section 21.
#include "stx_internal.h"

namespace {
// the 16-bit-fraction constants of tests/numpy_emit.py: {ky, ku, kv (B, G, R), yoff} by [matrix][range]
constexpr StxEmitCoef kCoef[2][2] = {
    {{{6416, 33039, 16829}, {28784, -19070, -9714}, {-4681, -24103, 28784}, 16}, {{7471, 38470, 19595}, {32768, -21710, -11058}, {-5329, -27439, 32768}, 0}},
    {{{4064, 40254, 11966}, {28784, -22188, -6596}, {-2639, -26145, 28784}, 16}, {{4732, 46871, 13933}, {32768, -25259, -7509}, {-3005, -29763, 32768}, 0}}};

using Plane = StxForeignPlane;
// a byte range of the call, for the overlap checks: a target plane, or a source / alpha image
struct Range { uintptr_t first, end; int item, plane; };  // plane: 0 .. 2 of the target; -1: source, -2: alpha

Range range_of(const uint8_t* p, long long pitch, long long row_bytes, int rows, int item, int plane)
{
    return Range{(uintptr_t)p, (uintptr_t)p + (uintptr_t)(rows - 1) * (uintptr_t)pitch + (uintptr_t)row_bytes, item, plane};
}
Range range_of(const stx_buf* b, int item, int plane)
{
    return range_of(b->ptr, (long long)b->stride, (long long)b->w * b->c * stx_elem_bytes(b->elem), b->h, item, plane);
}
bool overlap(const Range& a, const Range& b) { return a.first < b.end && b.first < a.end; }
bool aligned(const void* p, long long pitch, int a) { return ((uintptr_t)p % (uintptr_t)a) == 0 && pitch % a == 0; }

// what the planes of one item look like: count, then per plane its size as an image (w, h, c) — elem is the source's for RAW, else u8
struct Layout { int np; int w[3], h[3], c[3]; };
Layout layout_of(int format, int w, int h, int c)
{
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;  // chroma planes of the 4:2:0 formats: the ceiling sizes
    switch (format) {
    case STX_INGEST_BGRA: case STX_INGEST_RGBA: return Layout{1, {w}, {h}, {4}};
    case STX_INGEST_NV12: return Layout{2, {w, cw}, {h, ch}, {1, 2}};
    case STX_INGEST_I420: return Layout{3, {w, cw, cw}, {h, ch, ch}, {1, 1, 1}};
    default: return Layout{1, {w}, {h}, {c}};
    }
}
}  // namespace

STX_EXPORT int stx_emit(stx_ctx* ctx, int n, const stx_emit_item* in, int matrix, int range, void* consumer_stream, int has_stream, stx_buf** out)
{
    if (!ctx || !in || !out) return stx_fail(STX_ERR_INVALID, "null argument");
    if (n <= 0) return stx_fail(STX_ERR_INVALID, "emit of %d items", n);
    if (matrix < STX_INGEST_BT601 || matrix > STX_INGEST_BT709 || range < STX_INGEST_LIMITED || range > STX_INGEST_FULL)
        return stx_fail(STX_ERR_INVALID, "emit: matrix %d / range %d", matrix, range);
    STX_TRY(stx_set_device(ctx));
    std::vector<StxEmitItem> items((size_t)n);
    std::vector<Layout> layouts((size_t)n);
    std::vector<Range> targets, sources;
    long long tiles = 0;
    double bytes = 0.0;
    for (int i = 0; i < n; i++) {
        const stx_emit_item& E = in[i];
        const stx_buf* S = E.src;
        if (!S) return stx_fail(STX_ERR_INVALID, "emit: item %d has no source", i);
        if (S->ctx != ctx || (E.alpha && E.alpha->ctx != ctx)) return stx_fail(STX_ERR_INVALID, "emit: item %d belongs to another context", i);
        if (S->w < 1 || S->h < 1 || S->w > STX_INGEST_MAX_SIDE || S->h > STX_INGEST_MAX_SIDE)
            return stx_fail(STX_ERR_INVALID, "emit: item %d is %dx%d, images are 1 .. %d on a side", i, S->w, S->h, STX_INGEST_MAX_SIDE);
        if (E.format < STX_INGEST_RAW || E.format > STX_INGEST_I420) return stx_fail(STX_ERR_INVALID, "emit: item %d has format %d", i, E.format);
        const int want_c = E.format == STX_INGEST_RAW ? S->c : E.format == STX_INGEST_GRAY ? 1 : 3;
        if (E.format != STX_INGEST_RAW && (S->c != want_c || S->elem != STX_U8))
            return stx_fail(STX_ERR_INVALID, "emit: item %d: format %d is made from u8 with %d channel(s), the source has %d channel(s) of element type %d", i,
                            E.format, want_c, S->c, S->elem);
        const bool with_alpha = E.format == STX_INGEST_BGRA || E.format == STX_INGEST_RGBA;
        if (E.alpha) {
            const stx_buf* A = E.alpha;
            if (!with_alpha) return stx_fail(STX_ERR_INVALID, "emit: item %d: format %d has no alpha", i, E.format);
            if (A->elem != STX_U8 || A->c != 1 || A->w != S->w || A->h != S->h)
                return stx_fail(STX_ERR_INVALID, "emit: item %d: the alpha image is u8x1 of %dx%d, got %dx%d with %d channel(s) of element type %d", i, S->w,
                                S->h, A->w, A->h, A->c, A->elem);
            sources.push_back(range_of(A, i, -2));
        }
        sources.push_back(range_of(S, i, -1));
        const int es = E.format == STX_INGEST_RAW ? stx_elem_bytes(S->elem) : 1;
        const Layout L = layouts[i] = layout_of(E.format, S->w, S->h, S->c);
        StxEmitItem& K = items[i];
        K = StxEmitItem{};
        K.src = S->ptr; K.sstride = (long long)S->stride;
        K.wide = aligned(S->ptr, K.sstride, 4) ? STX_EMIT_WIDE_SRC : 0;
        if (E.alpha) {
            K.alpha = E.alpha->ptr; K.astride = (long long)E.alpha->stride;
            if (aligned(K.alpha, K.astride, 4)) K.wide |= STX_EMIT_WIDE_ALPHA;
        }
        K.w = S->w; K.h = S->h;
        if (E.has_target)
            for (int p = 0; p < L.np; p++) {
                const Plane P{(const uint8_t*)E.plane[p], E.pitch[p], (long long)L.w[p] * L.c[p] * es, L.h[p]};
                STX_TRY(stx_check_foreign_plane(ctx, "emit", "item", i, p, P, "a target is device memory"));
                K.dst[p] = (uint8_t*)E.plane[p]; K.dpitch[p] = E.pitch[p];
                targets.push_back(range_of(P.p, P.pitch, P.row_bytes, P.rows, i, p));
            }
        int units = S->w, row_units = S->h;  // along x: pixels (COPY: 4-byte words); along y: rows (4:2:0: row pairs)
        const double px = (double)S->w * S->h;
        switch (E.format) {
        case STX_INGEST_RAW: case STX_INGEST_BGR: case STX_INGEST_GRAY:
            K.kind = STX_EMIT_K_COPY; K.w = S->w * S->c * es; units = (K.w + 3) / 4;
            bytes += 2.0 * K.w * S->h;
            break;
        case STX_INGEST_RGB: K.kind = STX_EMIT_K_REV3; bytes += px * 6.0; break;
        case STX_INGEST_BGRA: case STX_INGEST_RGBA:
            K.kind = STX_EMIT_K_ALPHA; K.reverse = E.format == STX_INGEST_RGBA;
            bytes += px * (E.alpha ? 8.0 : 7.0);
            break;
        default:
            K.kind = E.format == STX_INGEST_NV12 ? STX_EMIT_K_NV12 : STX_EMIT_K_I420; row_units = L.h[1];
            bytes += px * 4.0 + 2.0 * L.w[1] * L.h[1];
            break;
        }
        K.tiles_x = (units + STX_INGEST_TW - 1) / STX_INGEST_TW;
        K.tile0 = (int)tiles;
        tiles += (long long)K.tiles_x * ((row_units + STX_INGEST_ROWS - 1) / STX_INGEST_ROWS);
        if (tiles > 0x7fffffffLL) return stx_fail(STX_ERR_INVALID, "emit of more than 2^31 tiles");
    }
    // a launch writes every target plane while it reads every source: none of them may share a byte
    for (size_t a = 0; a < targets.size(); a++) {
        for (size_t b = a + 1; b < targets.size(); b++)
            if (overlap(targets[a], targets[b]))
                return stx_fail(STX_ERR_INVALID, "emit: item %d plane %d overlaps item %d plane %d", targets[a].item, targets[a].plane, targets[b].item,
                                targets[b].plane);
        for (const Range& s : sources)
            if (overlap(targets[a], s))
                return stx_fail(STX_ERR_INVALID, "emit: item %d plane %d overlaps the %s image of item %d", targets[a].item, targets[a].plane,
                                s.plane == -1 ? "source" : "alpha", s.item);
    }
    // nothing was allocated or queued up to here
    std::vector<StxBufRef> made((size_t)n * 3);
    for (int i = 0; i < n; i++) {
        const Layout& L = layouts[i];
        for (int p = 0; p < L.np; p++) {
            if (!in[i].has_target) {
                StxBufRef& B = made[(size_t)i * 3 + p];
                STX_TRY(stx_buf_new(ctx, L.w[p], L.h[p], L.c[p], in[i].format == STX_INGEST_RAW ? in[i].src->elem : STX_U8, &B));
                items[i].dst[p] = B->ptr; items[i].dpitch[p] = (long long)B->stride;
            }
            const int a = items[i].kind == STX_EMIT_K_I420 && p > 0 ? 2 : 4;  // I420's chroma is stored 2 bytes at a time
            if (aligned(items[i].dst[p], items[i].dpitch[p], a)) items[i].wide |= STX_EMIT_WIDE_DST0 << p;
        }
    }
    StxDevBlock d_items;
    STX_TRY(upload_small(ctx, items.data(), items.size() * sizeof(StxEmitItem), &d_items));
    // the protocol's handle 1, the legacy default stream, is the runtime's null stream; 2 is hipStreamPerThread's own value (stx_ingest)
    hipStream_t consumer = (uintptr_t)consumer_stream == 1 ? nullptr : (hipStream_t)consumer_stream;
    // after whatever the consumer has queued (it may still read the surface): no host wait
    if (has_stream) STX_TRY(stx_stream_wait(ctx->stream, consumer, "emit: ordering after the consumer's stream"));
    STX_TRY(stx_launch_emit(ctx, (const StxEmitItem*)d_items.get(), n, (int)tiles, kCoef[matrix][range], bytes));
    // and the consumer's stream after the launch
    if (has_stream) STX_TRY(stx_stream_wait(consumer, ctx->stream, "emit: ordering the consumer's stream after the launch"));
    for (size_t k = 0; k < made.size(); k++) out[k] = made[k].release();
    return STX_OK;  // the descriptor block goes back here: stream-ordered reuse
}
