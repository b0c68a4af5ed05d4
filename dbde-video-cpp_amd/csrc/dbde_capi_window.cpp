// dbde_capi_window.cpp -- the window families of include/dbde_hip.h that write pixels or streams per frame: window
// decode (roi), histograms, binned, scaled and mask decode, compressed-domain crop and window encode.  Host side only;
// what they share with the other families is in dbde_host.h.
#include "dbde_host.h"

#include "dbde_binned_kernels.h"
#include "dbde_crop_kernels.h"
#include "dbde_hist_kernels.h"
#include "dbde_mask_kernels.h"
#include "dbde_scaled_kernels.h"
#include "dbde_wenc_kernels.h"

using namespace dbde;
using namespace dbde_host;

extern "C" {

// ---- window decode ----------------------------------------------------------------------------------------
static void report_roi_plan(const RoiPlan &pl, dbde_hip_roi_plan_t *plan) {
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl);
    plan->max_tiles_x = (int32_t)pl.max_tx;
    plan->max_tiles_y = (int32_t)pl.max_ty;
    plan->threads = pl.threads;
    plan->pieces_x = pl.pieces;
    plan->grid = pl.grid;
    plan->grid_origins = pl.grid_origins;
}

int dbde_hip_roi_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_roi_plan_t *plan) {
    RoiPlan pl;
    if (!plan || plan_roi(W, H, n_frames, x0, y0, rw, rh, pl)) return DBDE_HIP_ERR_ARG;
    report_roi_plan(pl, plan);
    return DBDE_HIP_OK;
}

int dbde16_hip_roi_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_roi_plan_t *plan) {
    RoiPlan pl;
    if (!plan || plan_roi(W, H, n_frames, x0, y0, rw, rh, pl, kRoi16WideThreads)) return DBDE_HIP_ERR_ARG;
    report_roi_plan(pl, plan);
    return DBDE_HIP_OK;
}

// Both window decoders: the index (min_bytes: 1 = DBDE, 2 = DBDE16) in timing slot 1, the window kernel in slot 2.
static int decode_roi_common(dbde_hip_ctx *ctx, const char *name, uint32_t min_bytes, const uint8_t *d_stream,
                             size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                             int y0, int rw, int rh, const int32_t *d_origins, void *d_out,
                             dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    RoiPlan pl;
    const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl, min_bytes == 2u ? kRoi16WideThreads : kRoiWideThreads);
    if (why)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames,
                    rw, rh, x0, y0);
    if (!d_stream || !d_frame_offsets || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, min_bytes, pl.split);
    if (rc) return rc;

    RoiParams p;
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    fill_roi_params(p, pl, W, H, x0, y0, rw, rh, d_origins, d_origins ? pl.pieces : pl.pieces_fixed);
    p.out = static_cast<uint8_t *>(d_out);
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_roi(p, (uint32_t)n_frames, pl.threads, min_bytes, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_roi(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                        int W, int H, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                        uint8_t *d_out, dbde_hip_frame_result *d_results) {
    return decode_roi_common(ctx, "decode_roi", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                             rh, d_origins, d_out, d_results);
}

int dbde16_hip_decode_roi(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                          const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                          const int32_t *d_origins, uint16_t *d_out, dbde_hip_frame_result *d_results) {
    return decode_roi_common(ctx, "decode_roi16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                             rw, rh, d_origins, d_out, d_results);
}


// ---- per-frame histograms ---------------------------------------------------------------------------------
struct HistPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t pieces_x, pieces, segments, pps, lds_bins;
    uint64_t grid, init_grid, atomics, workspace;
};
// A segment is cut only to fill the device (about 16 workgroups per CU) and never below the pieces whose pixels
// outnumber its flush 64 times (64 * bins pixels, and at least kHistMinPieces pieces).
static constexpr uint32_t kHistMinPieces = 16;
static const char *plan_histogram(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                                  unsigned outputs, int n_cu, uint32_t pix, HistPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    const int max_shift = pix == 1u ? 7 : 15;
    if (shift < 0 || shift > max_shift) return "shift outside [0, 7] (DBDE) / [0, 15] (DBDE16)";
    const uint32_t range = (pix == 1u ? 256u : 65536u) >> shift;
    const uint32_t most = pix == 1u ? range : (range < kHistLargeBins ? range : kHistLargeBins);
    if (bins < 1 || (uint32_t)bins > most) return "bins outside [1, 256 >> shift] (DBDE) / [1, min(4096, 65536 >> shift)] (DBDE16)";
    if (outputs < 1u || outputs > 3u) return "no output (or an unknown one) requested";
    const uint32_t tiles = kHistTilesOf(pix);
    pl.pieces_x = (pl.roi.ntx + tiles - 1u) / tiles;
    pl.pieces = pl.pieces_x * pl.roi.nty;
    pl.lds_bins = kHistLdsBinsOf((uint32_t)bins);
    const uint64_t n = (uint64_t)n_frames;
    const uint64_t px_piece = 64ull * tiles;
    uint64_t min_pieces = (64ull * (uint64_t)bins + px_piece - 1u) / px_piece;
    if (min_pieces < kHistMinPieces) min_pieces = kHistMinPieces;
    const uint64_t target = 16ull * (uint64_t)(n_cu > 0 ? n_cu : 1);
    uint64_t seg = (target + (n > 0 ? n : 1) - 1u) / (n > 0 ? n : 1);
    const uint64_t by_len = (pl.pieces + min_pieces - 1u) / min_pieces;
    if (seg > by_len) seg = by_len;
    if (seg < 1u) seg = 1u;
    const uint64_t pps = (pl.pieces + seg - 1u) / seg;
    seg = (pl.pieces + pps - 1u) / pps;   // no empty segment
    pl.segments = (uint32_t)seg;
    pl.pps = (uint32_t)pps;
    pl.grid = n * seg;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t rows = (n > 0 ? n : 1) * (uint64_t)bins;
    pl.init_grid = (rows + kHistRowThreads - 1u) / kHistRowThreads;
    if (pl.init_grid >= (1ull << 31)) return "too many workgroups in one call";
    pl.atomics = seg * (uint64_t)bins * (uint64_t)(((outputs & 1u) ? 1u : 0u) + ((outputs & 2u) ? 1u : 0u));
    pl.workspace = n * (pl.roi.dg.cpf + 1u) * 4u + n * 4u;
    return nullptr;
}

static int histogram_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                                 unsigned outputs, int n_cu, uint32_t pix, dbde_hip_histogram_plan_t *plan) {
    HistPlan pl;
    if (!plan || n_cu < 1 || plan_histogram(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    plan->threads = kHistThreads;
    plan->tiles_per_piece = kHistTilesOf(pix);
    plan->pieces_x = pl.pieces_x;
    plan->pieces = pl.pieces;
    plan->segments = pl.segments;
    plan->pieces_per_segment = pl.pps;
    plan->lds_bins = pl.lds_bins;
    plan->lds_copies = kHistCopiesOf(pl.lds_bins);
    plan->lds_bytes = kHistLdsBytesOf(pl.lds_bins);
    plan->grid = pl.grid;
    plan->init_grid = pl.init_grid;
    plan->global_atomics_per_frame = pl.atomics;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

int dbde_hip_histogram_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                            unsigned outputs, int n_cu, dbde_hip_histogram_plan_t *plan) {
    return histogram_plan_common(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, n_cu, 1u, plan);
}

int dbde16_hip_histogram_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                              unsigned outputs, int n_cu, dbde_hip_histogram_plan_t *plan) {
    return histogram_plan_common(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, n_cu, 2u, plan);
}

// Both histograms: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the histogram kernels
// in slot 2.
static int histogram_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                            size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                            int y0, int rw, int rh, int shift, int bins, int accumulate, uint32_t *d_hist,
                            uint64_t *d_total, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned outputs = (d_hist ? 1u : 0u) | (d_total ? 2u : 0u);
    HistPlan pl;
    if (const char *why = plan_histogram(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d shift %d bins %d)", name, why,
                    W, H, n_frames, rw, rh, x0, y0, shift, bins);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (d_total && !d_count) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: d_total needs d_count", name);
    if (misaligned(7u, d_total, d_count))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if (misaligned(3u, d_hist))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U32 rows must be 4-byte aligned", name);
    if (n_frames == 0 && (accumulate || !d_total)) return DBDE_HIP_OK;   // nothing to add or to reset
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;
    HistParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    p.n_frames = (uint32_t)n_frames;
    set_window(p, pl.roi, x0, y0, rw, rh);
    p.rows = pl.roi.nty;
    p.pieces = pl.pieces_x;
    p.segments = pl.segments;
    p.pps = pl.pps;
    p.shift = (uint32_t)shift;
    p.bins = (uint32_t)bins;
    p.accumulate = accumulate ? 1 : 0;
    p.out_hist = d_hist;
    p.out_total = d_total;
    p.out_count = d_total ? d_count : nullptr;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_histogram(p, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_histogram(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                       int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins, int accumulate,
                       uint32_t *d_hist, uint64_t *d_total, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return histogram_common(ctx, "histogram", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                            rh, shift, bins, accumulate, d_hist, d_total, d_count, d_results);
}

int dbde16_hip_histogram(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         int shift, int bins, int accumulate, uint32_t *d_hist, uint64_t *d_total, uint64_t *d_count,
                         dbde_hip_frame_result *d_results) {
    return histogram_common(ctx, "histogram16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                            rh, shift, bins, accumulate, d_hist, d_total, d_count, d_results);
}

// ---- binned decode -----------------------------------------------------------------------------------------
struct BinnedPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t threads, pieces, ow, oh;
    uint64_t grid, sum_bytes, mm_bytes;
};
static const char *plan_binned(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                               uint32_t pix, BinnedPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, kBinWideThreadsOf(pix))) return why;
    if (bin != 2 && bin != 4 && bin != 8) return "bin other than 2, 4, 8";
    if (x0 % bin || y0 % bin) return "window origin not a multiple of the bin";
    if (stats < 1u || stats > 7u) return "no statistic (or an unknown one) requested";
    pl.threads = pl.roi.ntx <= kBinNarrowThreads ? kBinNarrowThreads : kBinWideThreadsOf(pix);
    pl.pieces = (pl.roi.ntx + pl.threads - 1u) / pl.threads;
    pl.ow = ((uint32_t)rw + (uint32_t)bin - 1u) / (uint32_t)bin;
    pl.oh = ((uint32_t)rh + (uint32_t)bin - 1u) / (uint32_t)bin;
    pl.grid = (uint64_t)n_frames * pl.roi.nty * pl.pieces;   // below 2^31: at most plan_roi's grid_origins
    const uint64_t elems = (uint64_t)n_frames * pl.oh * pl.ow;
    pl.sum_bytes = elems * 2u * pix;
    pl.mm_bytes = elems * pix;
    return nullptr;
}

static int binned_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                              uint32_t pix, dbde_hip_binned_plan_t *plan) {
    BinnedPlan pl;
    if (!plan || plan_binned(W, H, n_frames, x0, y0, rw, rh, bin, stats, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    plan->out_w = pl.ow;
    plan->out_h = pl.oh;
    plan->threads = pl.threads;
    plan->pieces_x = pl.pieces;
    plan->lds_bytes = kBinLdsBytesOf(pl.threads, pix);
    plan->grid = pl.grid;
    plan->sum_bytes = (stats & DBDE_HIP_BINNED_SUM) ? pl.sum_bytes : 0u;
    plan->max_bytes = (stats & DBDE_HIP_BINNED_MAX) ? pl.mm_bytes : 0u;
    plan->min_bytes = (stats & DBDE_HIP_BINNED_MIN) ? pl.mm_bytes : 0u;
    return DBDE_HIP_OK;
}

int dbde_hip_binned_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                         dbde_hip_binned_plan_t *plan) {
    return binned_plan_common(W, H, n_frames, x0, y0, rw, rh, bin, stats, 1u, plan);
}

int dbde16_hip_binned_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                           dbde_hip_binned_plan_t *plan) {
    return binned_plan_common(W, H, n_frames, x0, y0, rw, rh, bin, stats, 2u, plan);
}

// Both binned decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the binning kernel
// in slot 2.
static int decode_binned_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                                int y0, int rw, int rh, int bin, void *d_sum, void *d_max, void *d_min,
                                dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_sum ? DBDE_HIP_BINNED_SUM : 0u) | (d_max ? DBDE_HIP_BINNED_MAX : 0u) | (d_min ? DBDE_HIP_BINNED_MIN : 0u);
    BinnedPlan pl;
    if (const char *why = plan_binned(W, H, n_frames, x0, y0, rw, rh, bin, stats, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d bin %d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, bin);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (misaligned(2u * pix - 1u, d_sum))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the sum plane must be %u-byte aligned", name, 2u * pix);
    if (misaligned(pix - 1u, d_max, d_min))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 planes must be 2-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;
    BinnedParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_window(p, pl.roi, x0, y0, rw, rh);
    p.rows = pl.roi.nty;
    p.pieces = pl.pieces;
    p.ow = pl.ow;
    p.oh = pl.oh;
    p.out_sum = d_sum;
    p.out_max = d_max;
    p.out_min = d_min;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_binned(p, (uint32_t)n_frames, pl.threads, pix, (uint32_t)bin, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_binned(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           int bin, uint16_t *d_sum, uint8_t *d_max, uint8_t *d_min, dbde_hip_frame_result *d_results) {
    return decode_binned_common(ctx, "decode_binned", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                y0, rw, rh, bin, d_sum, d_max, d_min, d_results);
}

int dbde16_hip_decode_binned(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                             int bin, uint32_t *d_sum, uint16_t *d_max, uint16_t *d_min,
                             dbde_hip_frame_result *d_results) {
    return decode_binned_common(ctx, "decode_binned16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                y0, rw, rh, bin, d_sum, d_max, d_min, d_results);
}

// ---- scaled float decode -------------------------------------------------------------------------------------
struct ScaledPlan {
    RoiPlan roi;                      // arguments, tile window, index geometry and launch: the window decoder's (plan_roi)
    uint32_t elem;                    // bytes of an output element
    uint64_t out_bytes;
};
static const char *plan_scaled(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type, uint32_t pix,
                               ScaledPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, kScaledWideThreadsOf(pix))) return why;
    if (out_type != DBDE_HIP_OUT_F32 && out_type != DBDE_HIP_OUT_F16 && out_type != DBDE_HIP_OUT_BF16)
        return "output type other than F32, F16, BF16";
    pl.elem = kScaledElemBytesOf((uint32_t)out_type);
    pl.out_bytes = (uint64_t)n_frames * (uint64_t)rw * (uint64_t)rh * pl.elem;
    return nullptr;
}

static int scaled_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type, uint32_t pix,
                              dbde_hip_scaled_plan_t *plan) {
    ScaledPlan pl;
    if (!plan || plan_scaled(W, H, n_frames, x0, y0, rw, rh, out_type, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    plan->max_tiles_x = (int32_t)pl.roi.max_tx;
    plan->max_tiles_y = (int32_t)pl.roi.max_ty;
    plan->threads = pl.roi.threads;
    plan->pieces_x = pl.roi.pieces;
    plan->lds_bytes = kScaledLdsBytesOf(pl.roi.threads, pix);
    plan->elem_bytes = pl.elem;
    plan->grid = pl.roi.grid;
    plan->grid_origins = pl.roi.grid_origins;
    plan->out_bytes = pl.out_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_scaled_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type,
                         dbde_hip_scaled_plan_t *plan) {
    return scaled_plan_common(W, H, n_frames, x0, y0, rw, rh, out_type, 1u, plan);
}

int dbde16_hip_scaled_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type,
                           dbde_hip_scaled_plan_t *plan) {
    return scaled_plan_common(W, H, n_frames, x0, y0, rw, rh, out_type, 2u, plan);
}

// Both scaled decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the scaling kernel
// in slot 2.
static int decode_scaled_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                                int y0, int rw, int rh, const int32_t *d_origins, int out_type, const float *d_dark,
                                float dark0, const float *d_gain, float gain0, void *d_out,
                                dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    ScaledPlan pl;
    if (const char *why = plan_scaled(W, H, n_frames, x0, y0, rw, rh, out_type, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d type %d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, out_type);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames > 0 && !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null output", name);
    if (misaligned(pl.elem - 1u, d_out))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the output must be %u-byte aligned", name, pl.elem);
    if (misaligned(3u, d_dark, d_gain))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the maps must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;

    ScaledParams p;
    memset(&p, 0, sizeof p);
    set_stream(p.roi, ctx, d_stream, stream_bytes, d_frame_offsets);
    fill_roi_params(p.roi, pl.roi, W, H, x0, y0, rw, rh, d_origins, d_origins ? pl.roi.pieces : pl.roi.pieces_fixed);
    p.roi.out = static_cast<uint8_t *>(d_out);
    p.dark = d_dark;
    p.gain = d_gain;
    p.dark0 = dark0;
    p.gain0 = gain0;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_scaled(p, (uint32_t)n_frames, pl.roi.threads, pix, (uint32_t)out_type, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_scaled(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           const int32_t *d_origins, int out_type, const float *d_dark, float dark0, const float *d_gain,
                           float gain0, void *d_out, dbde_hip_frame_result *d_results) {
    return decode_scaled_common(ctx, "decode_scaled", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                y0, rw, rh, d_origins, out_type, d_dark, dark0, d_gain, gain0, d_out, d_results);
}

int dbde16_hip_decode_scaled(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                             const int32_t *d_origins, int out_type, const float *d_dark, float dark0,
                             const float *d_gain, float gain0, void *d_out, dbde_hip_frame_result *d_results) {
    return decode_scaled_common(ctx, "decode_scaled16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames,
                                x0, y0, rw, rh, d_origins, out_type, d_dark, dark0, d_gain, gain0, d_out, d_results);
}

// ---- threshold mask decode ----------------------------------------------------------------------------------
struct MaskPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t words, threads;
    uint32_t piece_words, pieces;               // with per-frame origins: any x mod 8
    uint32_t piece_words_fixed, pieces_fixed;   // at (x0, y0): one more word per piece when x0 is a multiple of 8
    uint64_t grid, grid_origins, mask_bytes;
};
// Pieces are cut in window coordinates (whole mask words), so their number does not depend on the origin.
static const char *plan_mask(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint32_t pix, MaskPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, kMaskWideThreadsOf(pix))) return why;
    pl.words = ((uint32_t)rw + 63u) / 64u;
    pl.threads = pl.words <= kMaskNarrowWords ? kMaskNarrowThreads : kMaskWideThreadsOf(pix);
    // as few pieces as the workgroup's tiles allow, the words spread evenly over them
    const uint32_t cap = kMaskPieceWordsOf(pl.threads), cap_fixed = x0 % 8 == 0 ? kMaskAlignedPieceWordsOf(pl.threads) : cap;
    pl.pieces = (pl.words + cap - 1u) / cap;
    pl.piece_words = (pl.words + pl.pieces - 1u) / pl.pieces;
    pl.pieces_fixed = (pl.words + cap_fixed - 1u) / cap_fixed;
    pl.piece_words_fixed = (pl.words + pl.pieces_fixed - 1u) / pl.pieces_fixed;
    pl.grid = (uint64_t)n_frames * pl.roi.nty * pl.pieces_fixed;
    pl.grid_origins = (uint64_t)n_frames * pl.roi.max_ty * pl.pieces;
    if (pl.grid_origins >= (1ull << 31)) return "too many workgroups in one call";
    pl.mask_bytes = (uint64_t)n_frames * (uint64_t)rh * pl.words * 8u;
    return nullptr;
}

static int mask_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint32_t pix,
                            dbde_hip_mask_plan_t *plan) {
    MaskPlan pl;
    if (!plan || plan_mask(W, H, n_frames, x0, y0, rw, rh, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    plan->max_tiles_x = (int32_t)pl.roi.max_tx;
    plan->max_tiles_y = (int32_t)pl.roi.max_ty;
    plan->threads = pl.threads;
    plan->pieces_x = pl.pieces;
    plan->piece_words = pl.piece_words;
    plan->lds_bytes = kMaskLdsBytesOf(pl.threads, pix);
    plan->words = pl.words;
    plan->pieces_x_fixed = pl.pieces_fixed;
    plan->piece_words_fixed = pl.piece_words_fixed;
    plan->grid = pl.grid;
    plan->grid_origins = pl.grid_origins;
    plan->mask_bytes = pl.mask_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_mask_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_mask_plan_t *plan) {
    return mask_plan_common(W, H, n_frames, x0, y0, rw, rh, 1u, plan);
}

int dbde16_hip_mask_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_mask_plan_t *plan) {
    return mask_plan_common(W, H, n_frames, x0, y0, rw, rh, 2u, plan);
}

// Both mask decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the counts' and boxes'
// initialisation and the mask kernel in slot 2.
static int decode_mask_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                              size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                              int y0, int rw, int rh, const int32_t *d_origins, int mode, const void *d_lo_map,
                              uint32_t lo0, const void *d_hi_map, uint32_t hi0, uint64_t *d_mask, uint32_t *d_counts,
                              int32_t *d_boxes, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    MaskPlan pl;
    if (const char *why = plan_mask(W, H, n_frames, x0, y0, rw, rh, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames,
                    rw, rh, x0, y0);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (mode != DBDE_HIP_MASK_INSIDE && mode != DBDE_HIP_MASK_OUTSIDE)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: mode %d is neither INSIDE nor OUTSIDE", name, mode);
    const uint32_t pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    if (lo0 > pix_max || hi0 > pix_max)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: thresholds %u, %u above %u", name, lo0, hi0, pix_max);
    if (!d_mask && !d_counts && !d_boxes) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: no output requested", name);
    if (misaligned(7u, d_mask))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the mask must be 8-byte aligned", name);
    if (misaligned(3u, d_counts, d_boxes))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the counts and boxes must be 4-byte aligned", name);
    if (misaligned(pix - 1u, d_lo_map, d_hi_map))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the maps must be %u-byte aligned", name, pix);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;

    MaskParams p;
    memset(&p, 0, sizeof p);
    set_stream(p.roi, ctx, d_stream, stream_bytes, d_frame_offsets);
    fill_roi_params(p.roi, pl.roi, W, H, x0, y0, rw, rh, d_origins, d_origins ? pl.pieces : pl.pieces_fixed);
    p.lo_map = d_lo_map;
    p.hi_map = d_hi_map;
    p.lo0 = lo0;
    p.hi0 = hi0;
    p.outside = mode == DBDE_HIP_MASK_OUTSIDE ? kMaskOutside : kMaskInside;
    p.words = pl.words;
    p.piece_words = d_origins ? pl.piece_words : pl.piece_words_fixed;
    p.mask = d_mask;
    p.counts = d_counts;
    p.boxes = d_boxes;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_mask_init(d_counts, d_boxes, (uint32_t)n_frames, rw, rh, ctx->stream));
    HIP_TRY(ctx, launch_decode_mask(p, (uint32_t)n_frames, pl.threads, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_mask(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         const int32_t *d_origins, int mode, const uint8_t *d_lo_map, uint32_t lo0,
                         const uint8_t *d_hi_map, uint32_t hi0, uint64_t *d_mask, uint32_t *d_counts, int32_t *d_boxes,
                         dbde_hip_frame_result *d_results) {
    return decode_mask_common(ctx, "decode_mask", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                              rw, rh, d_origins, mode, d_lo_map, lo0, d_hi_map, hi0, d_mask, d_counts, d_boxes, d_results);
}

int dbde16_hip_decode_mask(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           const int32_t *d_origins, int mode, const uint16_t *d_lo_map, uint32_t lo0,
                           const uint16_t *d_hi_map, uint32_t hi0, uint64_t *d_mask, uint32_t *d_counts,
                           int32_t *d_boxes, dbde_hip_frame_result *d_results) {
    return decode_mask_common(ctx, "decode_mask16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                              rw, rh, d_origins, mode, d_lo_map, lo0, d_hi_map, hi0, d_mask, d_counts, d_boxes, d_results);
}

// ---- compressed-domain crop ---------------------------------------------------------------------------------
struct CropPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t Tout, recoded;
    uint64_t max_frame, capacity, rows;
    uint64_t tables_bytes, rec_fixed_bytes, rec_origins_bytes;
};
static uint64_t crop_max_frame_bytes(uint64_t T, uint32_t pix) { return 20u + 12u + (pix == 2u ? 131u : 66u) * T; }
static uint64_t round16(uint64_t v) { return (v + 15u) & ~(uint64_t)15; }
static const char *plan_crop(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                             uint32_t pix, CropPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi)) return why;
    if ((x0 | y0) & 7) return "window origin not a multiple of 8";
    const RoiPlan &r = pl.roi;
    pl.Tout = r.ntx * r.nty;
    pl.max_frame = crop_max_frame_bytes(pl.Tout, pix);
    if (slot_stride && slot_stride < pl.max_frame) return "slot_stride below the cropped frame's worst case";
    pl.capacity = n_frames == 0 ? 0u : (slot_stride ? (uint64_t)(n_frames - 1) * slot_stride + pl.max_frame : (uint64_t)n_frames * pl.max_frame);
    pl.rows = (uint64_t)n_frames * r.nty;
    if (pl.rows >= (1ull << 31)) return "too many workgroups in one call";
    const uint32_t rm = (uint32_t)rw - 8u * (r.ntx - 1u), dm = (uint32_t)rh - 8u * (r.nty - 1u);
    const uint32_t srm = (uint32_t)W - 8u * (r.tx0 + r.ntx - 1u), sdm = (uint32_t)H - 8u * (r.ty0 + r.nty - 1u);
    const bool cut_col = rm != (srm < 8u ? srm : 8u), cut_row = dm != (sdm < 8u ? sdm : 8u);
    pl.recoded = cut_row ? (cut_col ? r.ntx + r.nty - 1u : r.ntx) : (cut_col ? r.nty : 0u);
    // three U32 per (frame, window tile row), two U64 per frame; the records behind them
    pl.tables_bytes = round16(3u * 4u * pl.rows) + 2u * 8u * (uint64_t)n_frames;
    pl.rec_origins_bytes = (uint64_t)n_frames * (r.ntx + r.nty - 1u) * kCropRecBytes;
    pl.rec_fixed_bytes = pl.recoded ? pl.rec_origins_bytes : 0u;
    return nullptr;
}

static int crop_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride, uint32_t pix,
                            dbde_hip_crop_plan_t *plan) {
    CropPlan pl;
    if (!plan || plan_crop(W, H, n_frames, x0, y0, rw, rh, slot_stride, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    plan->out_tiles = pl.Tout;
    plan->recoded_tiles = pl.recoded;
    plan->size_threads = kCropThreads;
    plan->size_lds_bytes = kCropSizeLds;
    plan->rows_threads = kCropThreads;
    plan->rows_lds_bytes = kCropRowsLds;
    plan->place_threads = kCropPlaceThreads;
    plan->place_lds_bytes = kCropPlaceLds;
    plan->copy_threads = kCropThreads;
    plan->copy_lds_bytes = kCropCopyLds;
    plan->repack_threads = kCropThreads;
    plan->repack_lds_bytes = kCropRepackLds;
    plan->repack_grid = pl.recoded ? (uint64_t)n_frames * ((pl.roi.ntx + pl.roi.nty - 1u + kCropThreads - 1u) / kCropThreads) : 0u;
    plan->size_grid = pl.rows;
    plan->rows_grid = (uint64_t)n_frames;
    plan->place_grid = n_frames ? 1u : 0u;
    plan->copy_grid = pl.rows;
    plan->max_out_frame_bytes = pl.max_frame;
    plan->out_capacity = pl.capacity;
    plan->workspace_bytes = pl.tables_bytes + pl.rec_origins_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_crop_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                       dbde_hip_crop_plan_t *plan) {
    return crop_plan_common(W, H, n_frames, x0, y0, rw, rh, slot_stride, 1u, plan);
}

int dbde16_hip_crop_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                         dbde_hip_crop_plan_t *plan) {
    return crop_plan_common(W, H, n_frames, x0, y0, rw, rh, slot_stride, 2u, plan);
}

// Both crops: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the crop kernels in slot 2.
static int crop_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                       const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                       const int32_t *d_origins, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                       uint64_t *d_out_offsets, uint64_t *d_out_bytes, int32_t *d_origins_used,
                       dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    CropPlan pl;
    if (const char *why = plan_crop(W, H, n_frames, x0, y0, rw, rh, slot_stride, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames, rw,
                    rh, x0, y0);
    if (!d_stream || !d_frame_offsets || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    if ((uint64_t)out_capacity < pl.capacity)
        return fail(ctx, DBDE_HIP_ERR_CAPACITY, "%s: out_capacity %zu below the worst case %llu", name, out_capacity,
                    (unsigned long long)pl.capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t rec_bytes = d_origins ? pl.rec_origins_bytes : pl.rec_fixed_bytes;
    int rc = grow(ctx, ctx->crop_ws, ctx->crop_ws_bytes, (size_t)(pl.tables_bytes + rec_bytes), 1);
    if (rc) return rc;
    rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;

    CropParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    p.origins = d_origins;
    p.origins_used = d_origins_used;
    p.out = d_out;
    p.slot_stride = slot_stride;
    p.out_offsets = d_out_offsets;
    p.out_bytes = d_out_bytes;
    uint8_t *ws = ctx->crop_ws;
    p.frame_bytes = reinterpret_cast<uint64_t *>(ws);
    p.frame_off = p.frame_bytes + n_frames;
    p.row_src = reinterpret_cast<uint32_t *>(ws + 16u * (size_t)n_frames);
    p.row_copy = p.row_src + pl.rows;
    p.row_words = p.row_copy + pl.rows;
    p.rec = ws + pl.tables_bytes;
    p.W = W;
    p.H = H;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.w = pl.roi.g.w;
    p.T = pl.roi.g.T;
    p.geom = pl.roi.dg;
    p.ntx = pl.roi.ntx;
    p.nty = pl.roi.nty;
    p.Tout = pl.Tout;
    p.n_frames = (uint32_t)n_frames;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_crop(p, pix, d_origins != nullptr || pl.recoded != 0u, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_crop_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                         int W, int H, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                         uint8_t *d_out, size_t out_capacity, uint64_t slot_stride, uint64_t *d_out_offsets,
                         uint64_t *d_out_bytes, int32_t *d_origins_used, dbde_hip_frame_result *d_results) {
    return crop_common(ctx, "crop_frames", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                       d_origins, d_out, out_capacity, slot_stride, d_out_offsets, d_out_bytes, d_origins_used, d_results);
}

int dbde16_hip_crop_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           const int32_t *d_origins, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                           uint64_t *d_out_offsets, uint64_t *d_out_bytes, int32_t *d_origins_used,
                           dbde_hip_frame_result *d_results) {
    return crop_common(ctx, "crop_frames16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                       d_origins, d_out, out_capacity, slot_stride, d_out_offsets, d_out_bytes, d_origins_used, d_results);
}

// ---- window encode (include/dbde_hip.h) ------------------------------------------------------------
struct WencPlan {
    Geometry g;                       // of the window
    uint64_t pitch, frame_stride, min_image_bytes, max_frame, capacity, workspace;
    uint32_t lanes_per_row, units, cpf;
    bool forwards;
    int code;                         // of the broken rule
};
// nullptr when the arguments are good, else what is wrong with them (pl.code: the error code).  pix: 1 = DBDE, 2 = DBDE16.
static const char *plan_wenc(uint64_t image_address, uint64_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                             int n_frames, int x0, int y0, int rw, int rh, bool has_origins, uint64_t out_capacity,
                             bool check_capacity, uint64_t slot_stride, uint32_t pix, WencPlan &pl) {
    pl.code = DBDE_HIP_ERR_ARG;
    Geometry src;
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, src)) return "bad source size";
    if (rw < 1 || rh < 1 || rw > W || rh > H) return "window size outside [1, W] x [1, H]";
    if (x0 < 0 || y0 < 0 || x0 > W - rw || y0 > H - rh) return "window origin outside [0, W-rw] x [0, H-rh]";
    if (!geometry(rw, rh, pl.g)) return "window too large";
    const uint64_t row_bytes = (uint64_t)W * pix;
    pl.pitch = pitch ? pitch : row_bytes;
    if (pl.pitch < row_bytes) return "pitch below W * PIX";
    if (pl.pitch >= (1ull << 40)) return "pitch too large";
    const uint64_t frame_extent = (uint64_t)(H - 1) * pl.pitch + row_bytes;
    pl.frame_stride = frame_stride ? frame_stride : (uint64_t)H * pl.pitch;
    if (pl.frame_stride < frame_extent) return "frame_stride below (H-1) * pitch + W * PIX";
    if (pl.frame_stride >= (1ull << 48)) return "frame_stride too large";
    if (pix == 2u && ((pl.pitch | pl.frame_stride | image_address) & 1u)) return "DBDE16: odd pitch, frame_stride or base address";
    pl.min_image_bytes = n_frames ? (uint64_t)(n_frames - 1) * pl.frame_stride + frame_extent : 0u;
    if (image_bytes < pl.min_image_bytes) return "image_bytes below (n-1) * frame_stride + (H-1) * pitch + W * PIX";
    pl.max_frame = 32ull + (pix == 2u ? 131ull : 66ull) * pl.g.T;
    pl.capacity = n_frames == 0 ? 0u : (slot_stride ? (uint64_t)(n_frames - 1) * slot_stride + pl.max_frame : (uint64_t)n_frames * pl.max_frame);
    if (slot_stride && slot_stride < pl.max_frame) {
        if (pix == 2u) pl.code = DBDE_HIP_ERR_CAPACITY;   // (each as its frame encoder reports it)
        return "slot_stride below the window's worst case";
    }
    if (check_capacity && out_capacity < pl.capacity) { pl.code = DBDE_HIP_ERR_CAPACITY; return "out_capacity below the worst case"; }
    pl.forwards = !has_origins && rw == W && rh == H && pl.pitch == row_bytes && pl.frame_stride == (uint64_t)H * row_bytes;
    pl.lanes_per_row = pix == 2u ? pl.g.w : (pl.g.w + 1u) / 2u;
    const uint64_t units = (uint64_t)pl.g.h * pl.lanes_per_row;
    pl.units = (uint32_t)units;
    pl.cpf = (uint32_t)((units + kWencThreads - 1u) / kWencThreads);
    if (!pl.forwards && (uint64_t)n_frames * pl.cpf >= (1ull << 31)) return "too many chunks in one call";
    const uint64_t n = (uint64_t)n_frames, gpf = (pl.cpf + kWencGroup - 1u) / kWencGroup;
    pl.workspace = 16u + 8u * (n * pl.cpf + n * gpf + n + (n + kWencGroup - 1u) / kWencGroup);
    return nullptr;
}

static int wenc_plan_common(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                            int n_frames, int x0, int y0, int rw, int rh, int has_origins, size_t out_capacity,
                            uint64_t slot_stride, int n_cu, uint32_t pix, dbde_hip_window_encode_plan_t *plan) {
    WencPlan pl;
    if (!plan || n_cu < 1) return DBDE_HIP_ERR_ARG;
    if (plan_wenc(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw, rh, has_origins != 0,
                  out_capacity, out_capacity != 0, slot_stride, pix, pl))
        return pl.code;
    memset(plan, 0, sizeof *plan);
    plan->forwards = pl.forwards ? 1u : 0u;
    plan->tiles_x = pl.g.w;
    plan->tiles_y = pl.g.h;
    plan->tiles = pl.g.T;
    plan->pitch = pl.pitch;
    plan->frame_stride = pl.frame_stride;
    plan->min_image_bytes = pl.min_image_bytes;
    plan->max_out_frame_bytes = pl.max_frame;
    plan->out_capacity = pl.capacity;
    if (pl.forwards) return DBDE_HIP_OK;
    plan->lanes_per_row = pl.lanes_per_row;
    plan->chunks_per_frame = pl.cpf;
    plan->chunk_tiles = wenc_chunk_tiles(pix);
    plan->record_group = kWencGroup;
    plan->threads = kWencThreads;
    plan->lds_bytes = kWencLdsBytes;
    const uint64_t chunks = (uint64_t)n_frames * pl.cpf, resident = (uint64_t)n_cu * kWencBlocksPerCu;
    plan->grid = chunks < resident ? chunks : resident;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

int dbde_hip_window_encode_plan(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                                int n_frames, int x0, int y0, int rw, int rh, int has_origins, size_t out_capacity,
                                uint64_t slot_stride, int n_cu, dbde_hip_window_encode_plan_t *plan) {
    return wenc_plan_common(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw, rh, has_origins,
                            out_capacity, slot_stride, n_cu, 1u, plan);
}

int dbde16_hip_window_encode_plan(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                                  int n_frames, int x0, int y0, int rw, int rh, int has_origins, size_t out_capacity,
                                  uint64_t slot_stride, int n_cu, dbde_hip_window_encode_plan_t *plan) {
    return wenc_plan_common(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw, rh, has_origins,
                            out_capacity, slot_stride, n_cu, 2u, plan);
}

// Both window encoders (pix: 1 = DBDE, 2 = DBDE16), timing slot 0.
static int encode_window_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_images, size_t image_bytes,
                                int W, int H, uint64_t pitch, uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh,
                                const int32_t *d_origins, uint64_t first_index, const uint64_t *d_indices,
                                const uint64_t *d_elapsed_ns, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                                uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    WencPlan pl;
    if (const char *why = plan_wenc(reinterpret_cast<uintptr_t>(d_images), image_bytes, W, H, pitch, frame_stride, n_frames, x0,
                                    y0, rw, rh, d_origins != nullptr, out_capacity, true, slot_stride, pix, pl))
        return fail(ctx, pl.code, "%s: %s (W=%d H=%d pitch=%llu stride=%llu n=%d window %dx%d at %d,%d)", name, why, W, H,
                    (unsigned long long)pitch, (unsigned long long)frame_stride, n_frames, rw, rh, x0, y0);
    if (!d_images || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    if (pl.forwards)   // exactly the frame encoders' layout: the plain case stays on the persistent encoder
        return pix == 2u ? dbde16_hip_encode_frames(ctx, reinterpret_cast<const uint16_t *>(d_images), W, H, n_frames, first_index,
                                                    d_out, out_capacity, slot_stride, d_frame_offsets, d_frame_bytes)
                         : dbde_hip_encode_frames(ctx, d_images, W, H, n_frames, first_index, d_indices, d_elapsed_ns, d_out,
                                                  out_capacity, slot_stride, d_frame_offsets, d_frame_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = grow(ctx, ctx->w16, ctx->w16_bytes, (size_t)pl.workspace, 1, true);
    if (rc) return rc;
    WencParams p;
    memset(&p, 0, sizeof p);
    p.images = d_images;
    p.image_bytes = image_bytes;
    p.pitch = pl.pitch;
    p.frame_stride = pl.frame_stride;
    p.origins = d_origins;
    p.W = W; p.H = H; p.x0 = x0; p.y0 = y0; p.rw = rw; p.rh = rh;
    p.narrow = (uint32_t)rw * pix < 16u ? 1u : 0u;
    p.out = d_out;
    p.frame_offsets = d_frame_offsets;
    p.frame_bytes = d_frame_bytes;
    p.indices = d_indices;
    p.elapsed_ns = d_elapsed_ns;
    p.first_index = first_index;
    p.slot_stride = slot_stride;
    p.w = pl.g.w; p.h = pl.g.h; p.T = pl.g.T;
    p.lanes_per_row = pl.lanes_per_row;
    p.units = pl.units;
    p.chunks_per_frame = pl.cpf;
    p.n_frames = (uint32_t)n_frames;
    const size_t n = (size_t)n_frames, gpf = (pl.cpf + kWencGroup - 1u) / kWencGroup;
    p.ticket = reinterpret_cast<uint32_t *>(ctx->w16);
    p.state = reinterpret_cast<unsigned long long *>(ctx->w16 + 16);
    p.gsum = p.state + n * pl.cpf;
    p.fsize = p.gsum + n * gpf;
    p.fgsum = p.fsize + n;
    p.sticky = ctx->sticky;
    p.force_tickets = (ctx->exp_flags & 1u) ? 1u : 0u;
    uint32_t &resident = ctx->wenc_grid[pix - 1u];
    if (!resident) resident = (uint32_t)(wenc_blocks_per_cu(pix) * ctx->n_cu);
    span_begin(ctx, 0);
    HIP_TRY(ctx, hipMemsetAsync(ctx->w16, 0, (size_t)pl.workspace, ctx->stream));
    HIP_TRY(ctx, launch_encode_window(p, pix, (ctx->exp_flags & 1024u) ? 3u : resident, ctx->stream));   // (experiment bit 10: three workgroups)
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_encode_window(dbde_hip_ctx *ctx, const uint8_t *d_images, size_t image_bytes, int W, int H, uint64_t pitch,
                           uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                           uint64_t first_index, const uint64_t *d_indices, const uint64_t *d_elapsed_ns, uint8_t *d_out,
                           size_t out_capacity, uint64_t slot_stride, uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    return encode_window_common(ctx, "encode_window", 1u, d_images, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw,
                                rh, d_origins, first_index, d_indices, d_elapsed_ns, d_out, out_capacity, slot_stride,
                                d_frame_offsets, d_frame_bytes);
}

int dbde16_hip_encode_window(dbde_hip_ctx *ctx, const uint16_t *d_images, size_t image_bytes, int W, int H, uint64_t pitch,
                             uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                             uint64_t first_index, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                             uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    return encode_window_common(ctx, "encode_window16", 2u, reinterpret_cast<const uint8_t *>(d_images), image_bytes, W, H, pitch,
                                frame_stride, n_frames, x0, y0, rw, rh, d_origins, first_index, nullptr, nullptr, d_out,
                                out_capacity, slot_stride, d_frame_offsets, d_frame_bytes);
}

}  // extern "C"
