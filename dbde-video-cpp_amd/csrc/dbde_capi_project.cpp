// dbde_capi_project.cpp -- the window families of include/dbde_hip.h that reduce over frames: temporal projections
// (plain, weighted, counts, neighbour products, lag, registered, grouped) and region traces.  Host side only; what
// they share with the other families is in dbde_host.h.
#include "dbde_host.h"

#include "dbde_counts_kernels.h"
#include "dbde_gproject_kernels.h"
#include "dbde_lag_kernels.h"
#include "dbde_pairs_kernels.h"
#include "dbde_rproject_kernels.h"
#include "dbde_trace_kernels.h"
#include "dbde_wproject_kernels.h"

using namespace dbde;
using namespace dbde_host;

// ---- temporal projections ---------------------------------------------------------------------------------
namespace dbde_host DBDE_HOST_HIDDEN {

// Frames per segment: a segment is cut only to fill the device (about 4 workgroups per CU) and never below
// kProjMinFramesPerSegment frames, whose partials would cost more traffic than they save; never above the U32 bound.
static constexpr uint32_t kProjMinFramesPerSegment = 32;
const char *plan_project(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                         uint32_t pix, ProjectPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    if (stats < 1u || stats > kProjAll) return "no statistic (or an unknown one) requested";
    pl.stats = stats;
    const uint32_t tiles = kProjTilesOf(pix);
    pl.pieces = (pl.roi.ntx + tiles - 1u) / tiles;
    return plan_project_segments(n_frames, rw, rh, n_cu, pix, pl);
}
const char *plan_project_segments(int n_frames, int rw, int rh, int n_cu, uint32_t pix, ProjectPlan &pl) {
    pl.rows = pl.roi.nty;
    const uint64_t base = (uint64_t)pl.pieces * pl.rows, n = (uint64_t)n_frames;
    const uint64_t target = 4ull * (uint64_t)(n_cu > 0 ? n_cu : 1);
    uint64_t seg = base >= target ? 1u : (target + base - 1u) / base;
    const uint64_t by_len = (n + kProjMinFramesPerSegment - 1u) / kProjMinFramesPerSegment;
    if (seg > by_len) seg = by_len;
    const uint64_t by_bound = (n + kProjMaxFramesPerSegment - 1u) / kProjMaxFramesPerSegment;
    if (seg < by_bound) seg = by_bound;
    if (seg < 1u) seg = 1u;
    uint64_t fps = (n + seg - 1u) / seg;
    if (fps > 0u) seg = (n + fps - 1u) / fps;   // no empty segment
    if (seg >= (1ull << 31)) return "too many workgroups in one call";
    pl.segments = (uint32_t)seg;
    pl.fps = (uint32_t)fps;
    pl.grid = base * seg;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t pixels = (uint64_t)rw * (uint64_t)rh;
    pl.combine_grid = seg > 1u ? (pixels + kProjCombineThreads - 1u) / kProjCombineThreads : 0u;
    if (pl.combine_grid >= (1ull << 31)) return "too many workgroups in one call";
    pl.workspace = project_workspace_bytes(pl.stats, pl.segments, pixels, pix);
    return nullptr;
}

}  // namespace dbde_host

// The per-segment partials of project's statistics in ctx->proj_ws, in project_workspace_bytes' order.
static int carve_project_workspace(dbde_hip_ctx *ctx, const ProjectPlan &pl, int rw, int rh, uint32_t pix, ProjParams &p) {
    if (!pl.workspace) return DBDE_HIP_OK;
    int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.workspace, 1);
    if (rc) return rc;
    const uint64_t pixels = (uint64_t)rw * (uint64_t)rh;
    uint8_t *w = ctx->proj_ws;
    if (pl.stats & kProjMax) { p.ws_max = w; w += project_partial_bytes(kProjMax, pl.segments, pixels, pix); }
    if (pl.stats & kProjMin) { p.ws_min = w; w += project_partial_bytes(kProjMin, pl.segments, pixels, pix); }
    if (pl.stats & kProjSum) { p.ws_sum = reinterpret_cast<uint32_t *>(w); w += project_partial_bytes(kProjSum, pl.segments, pixels, pix); }
    if (pl.stats & kProjSumSq) p.ws_sumsq = reinterpret_cast<uint32_t *>(w);
    return DBDE_HIP_OK;
}

extern "C" {

static int project_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                               uint32_t pix, dbde_hip_project_plan_t *plan) {
    ProjectPlan pl;
    if (!plan || plan_project(W, H, n_frames, x0, y0, rw, rh, stats, n_cu, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    report_segments(plan, pl);
    return DBDE_HIP_OK;
}

int dbde_hip_project_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                          dbde_hip_project_plan_t *plan) {
    return project_plan_common(W, H, n_frames, x0, y0, rw, rh, stats, n_cu, 1u, plan);
}

int dbde16_hip_project_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                            dbde_hip_project_plan_t *plan) {
    return project_plan_common(W, H, n_frames, x0, y0, rw, rh, stats, n_cu, 2u, plan);
}

// Both projections: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the projection
// kernels in slot 2.  d_max / d_min hold U8 (pix 1) or U16 (pix 2) pixels.
static int project_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                          size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                          int y0, int rw, int rh, int accumulate, void *d_max, void *d_min, uint64_t *d_sum,
                          uint64_t *d_sumsq, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_max ? kProjMax : 0u) | (d_min ? kProjMin : 0u) | (d_sum ? kProjSum : 0u) |
                           (d_sumsq ? kProjSumSq : 0u);
    ProjectPlan pl;
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, stats, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames,
                    rw, rh, x0, y0);
    if (!d_stream || !d_frame_offsets || !d_count) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (misaligned(7u, d_sum, d_sumsq, d_count))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if (misaligned(pix - 1u, d_max, d_min))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 outputs must be 2-byte aligned", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;
    ProjParams p;
    memset(&p, 0, sizeof p);
    rc = carve_project_workspace(ctx, pl, rw, rh, pix, p);
    if (rc) return rc;
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_projection(p, pl, n_frames, x0, y0, rw, rh, accumulate);
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_project(p, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                     int W, int H, int n_frames, int x0, int y0, int rw, int rh, int accumulate, uint8_t *d_max,
                     uint8_t *d_min, uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count,
                     dbde_hip_frame_result *d_results) {
    return project_common(ctx, "project", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                          accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_results);
}

int dbde16_hip_project(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                       const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                       int accumulate, uint16_t *d_max, uint16_t *d_min, uint64_t *d_sum, uint64_t *d_sumsq,
                       uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return project_common(ctx, "project16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                          rh, accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_results);
}

// ---- weighted temporal projections -------------------------------------------------------
// The window, the index geometry and the segment rule are plan_project's (any statistics set gives the same segments);
// ONE_SEGMENT forces one segment, whose F32 chain has no bound on its frames.
struct WProjectPlan {
    ProjectPlan proj;
    uint32_t regressors;
};
static const char *plan_wproject(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                 uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                 uint64_t count_address, int n_cu, uint32_t pix, WProjectPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (n_regressors < 1 || n_regressors > (int)kWProjMaxRegressors) return "n_regressors outside 1..8";
    if (flags & ~DBDE_HIP_WPROJ_ONE_SEGMENT) return "unknown flag bits";
    if (weight_stride < (uint64_t)n_frames) return "weight_stride < n_frames";
    if (!weights_address || !out_address || !count_address) return "null pointer";
    if ((weights_address | out_address) & 3u) return "F32 weights and output must be 4-byte aligned";
    if (count_address & 7u) return "the U64 count must be 8-byte aligned";
    pl.regressors = (uint32_t)n_regressors;
    if (flags & DBDE_HIP_WPROJ_ONE_SEGMENT) {
        pl.proj.segments = 1u;
        pl.proj.fps = (uint32_t)n_frames;
        pl.proj.grid = (uint64_t)pl.proj.pieces * pl.proj.rows;
        pl.proj.combine_grid = 0u;
    }
    pl.proj.workspace = wproject_workspace_bytes(pl.regressors, pl.proj.segments, (uint64_t)rw * (uint64_t)rh);
    return nullptr;
}

static int wproject_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_weighted_plan_t *plan) {
    WProjectPlan pl;
    if (!plan || plan_wproject(W, H, n_frames, x0, y0, rw, rh, n_regressors, weight_stride, flags, weights_address,
                               out_address, count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.proj.roi);
    report_segments(plan, pl.proj);
    plan->regressors = pl.regressors;
    plan->lds_bytes = kWProjLdsBytes;
    return DBDE_HIP_OK;
}

int dbde_hip_project_weighted_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                   uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                   uint64_t count_address, int n_cu, dbde_hip_project_weighted_plan_t *plan) {
    return wproject_plan_common(W, H, n_frames, x0, y0, rw, rh, n_regressors, weight_stride, flags, weights_address,
                                out_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_weighted_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                     uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                     uint64_t count_address, int n_cu, dbde_hip_project_weighted_plan_t *plan) {
    return wproject_plan_common(W, H, n_frames, x0, y0, rw, rh, n_regressors, weight_stride, flags, weights_address,
                                out_address, count_address, n_cu, 2u, plan);
}

// Both weighted projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
static int wproject_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                           size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                           int y0, int rw, int rh, const float *d_weights, int n_regressors, size_t weight_stride,
                           int accumulate, int flags, float *d_out, uint64_t *d_count,
                           dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    WProjectPlan pl;
    if (const char *why = plan_wproject(W, H, n_frames, x0, y0, rw, rh, n_regressors, (uint64_t)weight_stride, flags,
                                        reinterpret_cast<uintptr_t>(d_weights), reinterpret_cast<uintptr_t>(d_out),
                                        reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, R=%d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, n_regressors);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                        pl.proj.roi.split);
    if (rc) return rc;
    WProjParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the F32 partials [segments][R][rh * rw]
        rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        p.ws = reinterpret_cast<float *>(ctx->proj_ws);
    }
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_projection(p, pl.proj, n_frames, x0, y0, rw, rh, accumulate);
    p.regressors = pl.regressors;
    p.weights = d_weights;
    p.weight_stride = (uint64_t)weight_stride;
    p.out = d_out;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_wproject(p, pl.regressors, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_weighted(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw,
                              int rh, const float *d_weights, int n_regressors, size_t weight_stride, int accumulate,
                              int flags, float *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return wproject_common(ctx, "project_weighted", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                           rw, rh, d_weights, n_regressors, weight_stride, accumulate, flags, d_out, d_count, d_results);
}

int dbde16_hip_project_weighted(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw,
                                int rh, const float *d_weights, int n_regressors, size_t weight_stride, int accumulate,
                                int flags, float *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return wproject_common(ctx, "project_weighted16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                           y0, rw, rh, d_weights, n_regressors, weight_stride, accumulate, flags, d_out, d_count,
                           d_results);
}

// ---- count projections -------------------------------------------------------------------
// The window, the index geometry and the segment rule are plan_project's (any statistics set gives the same segments).
// The counts are integers, so the value does not depend on the segments.
struct CountsPlan {
    ProjectPlan proj;
    uint32_t levels;
};
static const char *plan_counts(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                               uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                               uint64_t count_address, int n_cu, uint32_t pix, CountsPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (n_levels < 1 || n_levels > (int)kCountsMaxLevels) return "n_levels outside 1..8";
    if (flags & ~DBDE_HIP_COUNTS_MAPS) return "unknown flag bits";
    if ((flags & DBDE_HIP_COUNTS_MAPS) && level_stride < (uint64_t)rw * (uint64_t)rh) return "level_stride < rw * rh";
    if (!thresholds_address || !out_address || !count_address) return "null pointer";
    if (thresholds_address & (pix - 1u)) return "U16 thresholds must be 2-byte aligned";
    if (out_address & 3u) return "the U32 output must be 4-byte aligned";
    if (count_address & 7u) return "the U64 count must be 8-byte aligned";
    pl.levels = (uint32_t)n_levels;
    pl.proj.workspace = counts_workspace_bytes(pl.levels, pl.proj.segments, (uint64_t)rw * (uint64_t)rh);
    return nullptr;
}

static int counts_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                              uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                              uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_counts_plan_t *plan) {
    CountsPlan pl;
    if (!plan || plan_counts(W, H, n_frames, x0, y0, rw, rh, n_levels, level_stride, flags, thresholds_address,
                             out_address, count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.proj.roi);
    report_segments(plan, pl.proj);
    plan->levels = pl.levels;
    plan->lds_bytes = kCountsLdsBytes;
    return DBDE_HIP_OK;
}

int dbde_hip_project_counts_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                                 uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                                 uint64_t count_address, int n_cu, dbde_hip_project_counts_plan_t *plan) {
    return counts_plan_common(W, H, n_frames, x0, y0, rw, rh, n_levels, level_stride, flags, thresholds_address,
                              out_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_counts_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                                   uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                                   uint64_t count_address, int n_cu, dbde_hip_project_counts_plan_t *plan) {
    return counts_plan_common(W, H, n_frames, x0, y0, rw, rh, n_levels, level_stride, flags, thresholds_address,
                              out_address, count_address, n_cu, 2u, plan);
}

// Both count projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
static int counts_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         const void *d_thresholds, int n_levels, size_t level_stride, int accumulate, int flags,
                         uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    CountsPlan pl;
    if (const char *why = plan_counts(W, H, n_frames, x0, y0, rw, rh, n_levels, (uint64_t)level_stride, flags,
                                      reinterpret_cast<uintptr_t>(d_thresholds), reinterpret_cast<uintptr_t>(d_out),
                                      reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, K=%d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, n_levels);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                        pl.proj.roi.split);
    if (rc) return rc;
    CountsParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the U32 partials [segments][K][rh * rw]
        rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        p.ws = reinterpret_cast<uint32_t *>(ctx->proj_ws);
    }
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_projection(p, pl.proj, n_frames, x0, y0, rw, rh, accumulate);
    p.levels = pl.levels;
    p.maps = (flags & DBDE_HIP_COUNTS_MAPS) ? 1 : 0;
    p.thresholds = d_thresholds;
    p.level_stride = (uint64_t)level_stride;
    p.out = d_out;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_counts(p, pl.levels, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_counts(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                            const uint8_t *d_thresholds, int n_levels, size_t level_stride, int accumulate, int flags,
                            uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return counts_common(ctx, "project_counts", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                         rh, d_thresholds, n_levels, level_stride, accumulate, flags, d_out, d_count, d_results);
}

int dbde16_hip_project_counts(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw,
                              int rh, const uint16_t *d_thresholds, int n_levels, size_t level_stride, int accumulate,
                              int flags, uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return counts_common(ctx, "project_counts16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                         rw, rh, d_thresholds, n_levels, level_stride, accumulate, flags, d_out, d_count, d_results);
}

// ---- neighbour-product projections -------------------------------------------------------
// The window and the index geometry are plan_project's.  The pieces across a window tile row overlap by the halo tiles
// of the instance that serves the mask (kPairsPiecesOf), and the segment rule is plan_project's applied to that grid.
// The sums are integers, so the value does not depend on the segments.
struct PairsPlan {
    ProjectPlan proj;
    uint32_t pairs, planes, instance;
};
static const char *plan_pairs(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs, uint64_t out_address,
                              uint64_t count_address, int n_cu, uint32_t pix, PairsPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (pairs < 1 || pairs > (int)kPairAll) return "pairs outside 1..15";
    if (!out_address || !count_address) return "null pointer";
    if ((out_address | count_address) & 7u) return "the U64 output and count must be 8-byte aligned";
    pl.pairs = (uint32_t)pairs;
    pl.planes = (uint32_t)__builtin_popcount(pl.pairs);
    pl.instance = kPairsInstanceOf(pl.pairs);
    pl.proj.pieces = kPairsPiecesOf(pl.proj.roi.ntx, pl.instance, pix);
    if (const char *why = plan_project_segments(n_frames, rw, rh, n_cu, pix, pl.proj)) return why;
    pl.proj.workspace = pairs_workspace_bytes(pl.planes, pl.proj.segments, (uint64_t)rw * (uint64_t)rh, pix);
    return nullptr;
}

static int pairs_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs, uint64_t out_address,
                             uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_pairs_plan_t *plan) {
    PairsPlan pl;
    if (!plan || plan_pairs(W, H, n_frames, x0, y0, rw, rh, pairs, out_address, count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.proj.roi);
    report_segments(plan, pl.proj);
    plan->planes = pl.planes;
    plan->lds_bytes = kPairsLdsBytesOf(pl.instance);
    plan->instance = pl.instance;
    plan->piece_tiles = kProjTilesOf(pix);
    plan->piece_stride = kPairsStrideOf(pl.instance, pix);
    plan->halo_left = kPairsHaloLeft(pl.instance);
    plan->halo_right = kPairsHaloRight(pl.instance);
    plan->rows_below = pl.instance != kPairRight ? pl.proj.roi.nty - 1u : 0u;
    return DBDE_HIP_OK;
}

int dbde_hip_project_pairs_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs,
                                uint64_t out_address, uint64_t count_address, int n_cu,
                                dbde_hip_project_pairs_plan_t *plan) {
    return pairs_plan_common(W, H, n_frames, x0, y0, rw, rh, pairs, out_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_pairs_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs,
                                  uint64_t out_address, uint64_t count_address, int n_cu,
                                  dbde_hip_project_pairs_plan_t *plan) {
    return pairs_plan_common(W, H, n_frames, x0, y0, rw, rh, pairs, out_address, count_address, n_cu, 2u, plan);
}

// Both pair projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
static int pairs_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                        const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                        int pairs, int accumulate, uint64_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    PairsPlan pl;
    if (const char *why = plan_pairs(W, H, n_frames, x0, y0, rw, rh, pairs, reinterpret_cast<uintptr_t>(d_out),
                                     reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, pairs=%d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, pairs);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                        pl.proj.roi.split);
    if (rc) return rc;
    PairsParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the partials [segments][planes][rh * rw], U32 (pix 1) or U64 (pix 2)
        rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        p.ws = ctx->proj_ws;
    }
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_projection(p, pl.proj, n_frames, x0, y0, rw, rh, accumulate);
    p.pairs = pl.pairs;
    p.planes = pl.planes;
    p.out = d_out;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_pairs(p, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_pairs(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           int pairs, int accumulate, uint64_t *d_out, uint64_t *d_count,
                           dbde_hip_frame_result *d_results) {
    return pairs_common(ctx, "project_pairs", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                        pairs, accumulate, d_out, d_count, d_results);
}

int dbde16_hip_project_pairs(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                             int pairs, int accumulate, uint64_t *d_out, uint64_t *d_count,
                             dbde_hip_frame_result *d_results) {
    return pairs_common(ctx, "project_pairs16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                        rh, pairs, accumulate, d_out, d_count, d_results);
}

// ---- lag projections ---------------------------------------------------------------------
// The window, the index geometry, the pieces and the segment rule are plan_project's (any statistics set gives the same
// segments).  The values are integers, so they do not depend on the segments.
struct LagPlan {
    ProjectPlan proj;
    uint32_t stats, instance, lag, lead, first_pair, history;
};
static const char *plan_lag(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead, unsigned stats,
                            uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                            uint64_t count_address, int n_cu, uint32_t pix, LagPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (lag < 1 || lag > (int)kLagMax) return "lag outside 1..8";
    if (lead < 0 || lead > n_frames) return "lead outside 0..n_frames";
    if (stats < 1u || stats > kLagAll) return "no statistic (or an unknown one) requested";
    if (!pairs_address || !count_address) return "null pointer";
    if ((sums_address | pairs_address | count_address) & 7u) return "U64 outputs must be 8-byte aligned";
    if (maxdiff_address & (pix - 1u)) return "the U16 maxdiff plane must be 2-byte aligned";
    pl.stats = stats;
    pl.instance = kLagInstanceOf(stats);
    pl.lag = (uint32_t)lag;
    pl.lead = (uint32_t)lead;
    pl.first_pair = pl.lead > pl.lag ? pl.lead : pl.lag;
    // segments that count a pair: those reaching past first_pair; each but the first decodes lag history frames again
    const uint32_t active = pl.first_pair < (uint32_t)n_frames ? pl.proj.segments - pl.first_pair / pl.proj.fps : 0u;
    pl.history = active > 1u ? (active - 1u) * pl.lag : 0u;
    pl.proj.workspace = lag_workspace_bytes(stats, pl.proj.segments, (uint64_t)rw * (uint64_t)rh, pix);
    return nullptr;
}

static int lag_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead, unsigned stats,
                           uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                           uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_lag_plan_t *plan) {
    LagPlan pl;
    if (!plan || plan_lag(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums_address, maxdiff_address, pairs_address,
                          count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.proj.roi);
    report_segments(plan, pl.proj);
    plan->planes = (uint32_t)__builtin_popcount(pl.stats);
    plan->lds_bytes = kLagLdsBytes;
    plan->instance = pl.instance;
    plan->first_frame = pl.first_pair - pl.lag;
    plan->history_frames = pl.history;
    plan->first_pair = pl.first_pair;
    return DBDE_HIP_OK;
}

int dbde_hip_project_lag_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead,
                              unsigned stats, uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                              uint64_t count_address, int n_cu, dbde_hip_project_lag_plan_t *plan) {
    return lag_plan_common(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums_address, maxdiff_address,
                           pairs_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_lag_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead,
                                unsigned stats, uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                                uint64_t count_address, int n_cu, dbde_hip_project_lag_plan_t *plan) {
    return lag_plan_common(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums_address, maxdiff_address,
                           pairs_address, count_address, n_cu, 2u, plan);
}

// Both lag projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
// d_maxdiff holds U8 (pix 1) or U16 (pix 2) pixels.
static int lag_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                      const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                      int lag, int lead, int accumulate, uint64_t *d_product, uint64_t *d_pairsum, uint64_t *d_absdiff,
                      uint64_t *d_sqdiff, void *d_maxdiff, uint64_t *d_pairs, uint64_t *d_count,
                      dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_product ? kLagProduct : 0u) | (d_pairsum ? kLagPairSum : 0u) | (d_absdiff ? kLagAbsDiff : 0u) |
                           (d_sqdiff ? kLagSqDiff : 0u) | (d_maxdiff ? kLagMaxDiff : 0u);
    const uint64_t sums = reinterpret_cast<uintptr_t>(d_product) | reinterpret_cast<uintptr_t>(d_pairsum) |
                          reinterpret_cast<uintptr_t>(d_absdiff) | reinterpret_cast<uintptr_t>(d_sqdiff);
    LagPlan pl;
    if (const char *why = plan_lag(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums,
                                   reinterpret_cast<uintptr_t>(d_maxdiff), reinterpret_cast<uintptr_t>(d_pairs),
                                   reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, lag=%d lead=%d)", name, why, W,
                    H, n_frames, rw, rh, x0, y0, lag, lead);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                        pl.proj.roi.split);
    if (rc) return rc;
    LagParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the partials in lag_workspace_bytes' order, each 16-byte aligned
        rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        const uint64_t pixels = (uint64_t)rw * (uint64_t)rh;
        uint8_t *w = ctx->proj_ws;
        if (d_product) { p.ws_product = w; w += lag_partial_bytes(kLagProduct, pl.proj.segments, pixels, pix); }
        if (d_pairsum) { p.ws_pairsum = w; w += lag_partial_bytes(kLagPairSum, pl.proj.segments, pixels, pix); }
        if (d_absdiff) { p.ws_absdiff = reinterpret_cast<uint32_t *>(w); w += lag_partial_bytes(kLagAbsDiff, pl.proj.segments, pixels, pix); }
        if (d_sqdiff) { p.ws_sqdiff = w; w += lag_partial_bytes(kLagSqDiff, pl.proj.segments, pixels, pix); }
        if (d_maxdiff) { p.ws_maxdiff = w; w += lag_partial_bytes(kLagMaxDiff, pl.proj.segments, pixels, pix); }
    }
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_projection(p, pl.proj, n_frames, x0, y0, rw, rh, accumulate);
    p.lag = pl.lag;
    p.lead = pl.lead;
    p.out_product = d_product;
    p.out_pairsum = d_pairsum;
    p.out_absdiff = d_absdiff;
    p.out_sqdiff = d_sqdiff;
    p.out_maxdiff = d_maxdiff;
    p.out_pairs = d_pairs;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_lag(p, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_lag(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         int lag, int lead, int accumulate, uint64_t *d_product, uint64_t *d_pairsum,
                         uint64_t *d_absdiff, uint64_t *d_sqdiff, uint8_t *d_maxdiff, uint64_t *d_pairs,
                         uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return lag_common(ctx, "project_lag", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh, lag,
                      lead, accumulate, d_product, d_pairsum, d_absdiff, d_sqdiff, d_maxdiff, d_pairs, d_count, d_results);
}

int dbde16_hip_project_lag(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           int lag, int lead, int accumulate, uint64_t *d_product, uint64_t *d_pairsum,
                           uint64_t *d_absdiff, uint64_t *d_sqdiff, uint16_t *d_maxdiff, uint64_t *d_pairs,
                           uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return lag_common(ctx, "project_lag16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                      lag, lead, accumulate, d_product, d_pairsum, d_absdiff, d_sqdiff, d_maxdiff, d_pairs, d_count,
                      d_results);
}

// ---- registered projections --------------------------------------------------------------
// The sizes and the index geometry are plan_roi's for the window at (0, 0), whose tile rows are the bands of 8 output
// rows; the pieces own kRProjColsOf(pix) output columns, and the segment rule is plan_project's applied to that grid.
static const char *plan_rproject(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu, uint32_t pix,
                                 ProjectPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, 0, 0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    if (stats < 1u || stats > kProjAll) return "no statistic (or an unknown one) requested";
    pl.stats = stats;
    pl.pieces = ((uint32_t)rw + kRProjColsOf(pix) - 1u) / kRProjColsOf(pix);
    return plan_project_segments(n_frames, rw, rh, n_cu, pix, pl);
}

static int rproject_plan_common(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu, uint32_t pix,
                                dbde_hip_project_registered_plan_t *plan) {
    ProjectPlan pl;
    if (!plan || plan_rproject(W, H, n_frames, rw, rh, stats, n_cu, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_index(plan, pl.roi.g, pl.roi.dg, pl.roi.split);
    report_segments(plan, pl);
    plan->piece_cols = kRProjColsOf(pix);
    plan->band_rows = kRProjBandRows;
    plan->bands = pl.rows;
    plan->lds_bytes = kRProjLdsBytes;
    plan->instance = kRProjInstanceOf(stats);
    return DBDE_HIP_OK;
}

int dbde_hip_project_registered_plan(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu,
                                     dbde_hip_project_registered_plan_t *plan) {
    return rproject_plan_common(W, H, n_frames, rw, rh, stats, n_cu, 1u, plan);
}

int dbde16_hip_project_registered_plan(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu,
                                       dbde_hip_project_registered_plan_t *plan) {
    return rproject_plan_common(W, H, n_frames, rw, rh, stats, n_cu, 2u, plan);
}

// Both registered projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot
// 2.  d_max / d_min hold U8 (pix 1) or U16 (pix 2) pixels.
static int rproject_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                           size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw,
                           int rh, const int32_t *d_origins, int accumulate, void *d_max, void *d_min, uint64_t *d_sum,
                           uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                           dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_max ? kProjMax : 0u) | (d_min ? kProjMin : 0u) | (d_sum ? kProjSum : 0u) |
                           (d_sumsq ? kProjSumSq : 0u);
    ProjectPlan pl;
    if (const char *why = plan_rproject(W, H, n_frames, rw, rh, stats, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d)", name, why, W, H, n_frames, rw, rh);
    if (!d_stream || !d_frame_offsets || !d_count || !d_origins)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (misaligned(7u, d_sum, d_sumsq, d_count))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if (misaligned(pix - 1u, d_max, d_min))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 outputs must be 2-byte aligned", name);
    if (misaligned(3u, d_origins, d_origins_used))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins must be 4-byte aligned", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;
    RProjParams rp;
    memset(&rp, 0, sizeof rp);
    ProjParams &p = rp.pj;
    rc = carve_project_workspace(ctx, pl, rw, rh, pix, p);
    if (rc) return rc;
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_projection(p, pl, n_frames, 0, 0, rw, rh, accumulate);   // (the plan's window is at (0, 0): the origins move it)
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    p.out_count = d_count;
    rp.origins = d_origins;
    rp.origins_used = d_origins_used;
    rp.W = W;
    rp.H = H;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_rproject(rp, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_registered(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw, int rh,
                                const int32_t *d_origins, int accumulate, uint8_t *d_max, uint8_t *d_min,
                                uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                                dbde_hip_frame_result *d_results) {
    return rproject_common(ctx, "project_registered", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, rw, rh,
                           d_origins, accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_origins_used, d_results);
}

int dbde16_hip_project_registered(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                  const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw, int rh,
                                  const int32_t *d_origins, int accumulate, uint16_t *d_max, uint16_t *d_min,
                                  uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                                  dbde_hip_frame_result *d_results) {
    return rproject_common(ctx, "project_registered16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, rw,
                           rh, d_origins, accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_origins_used, d_results);
}

// ---- grouped temporal projections --------------------------------------------------------
struct GroupsPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t stats;
    uint32_t pieces, rows, runs, gpr;
    uint64_t grid;
    uint64_t max_bytes, min_bytes, sum_bytes, sumsq_bytes, counts_bytes;
};
// Groups per run: a run is cut only to fill the device (about 4 workgroups per CU, project's segment rule with whole
// groups as the unit) and never below kGProjMinFramesPerRun frames, which would start a pipeline for a handful of
// frames.  The ragged form's groups live on the device: it counts n_frames / n_groups frames per group.
// The *_addr arguments are the call's output pointers (0 = NULL); only their alignment is looked at.
static constexpr uint32_t kGProjMinFramesPerRun = 32;
static const char *plan_groups(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                               bool has_starts, int n_groups, int sum_type, int accumulate, uint64_t max_addr,
                               uint64_t min_addr, uint64_t sum_addr, uint64_t sumsq_addr, uint64_t counts_addr,
                               int n_cu, uint32_t pix, GroupsPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    const unsigned stats = (max_addr ? kProjMax : 0u) | (min_addr ? kProjMin : 0u) | (sum_addr ? kProjSum : 0u) |
                           (sumsq_addr ? kProjSumSq : 0u);
    if (!stats) return "no plane requested";
    if (!counts_addr) return "d_counts is required";
    if (accumulate != 0 && accumulate != 1) return "accumulate must be 0 or 1";
    if (sum_type != DBDE_HIP_SUM_U32 && sum_type != DBDE_HIP_SUM_U16) return "unknown sum_type";
    if (has_starts == (group_frames != 0)) return "exactly one of group_frames and d_group_starts must be given";
    if (n_groups < 0) return "n_groups is negative";
    const uint64_t n = (uint64_t)n_frames;
    uint64_t max_group;   // frames the largest group can hold
    if (has_starts) {
        if (n_groups < 1) return "the ragged form needs n_groups >= 1";
        if (n > kGProjMaxGroupFrames) return "the ragged form needs n_frames <= 65,536";
        max_group = n;
    } else {
        if (group_frames < 1 || (uint32_t)group_frames > kGProjMaxGroupFrames) return "group_frames must be 1..65,536";
        if ((uint64_t)n_groups != (n + (uint64_t)group_frames - 1u) / (uint64_t)group_frames)
            return "n_groups must equal ceil(n_frames / group_frames)";
        max_group = (uint64_t)group_frames;
    }
    if (sum_type == DBDE_HIP_SUM_U16) {
        if (pix != 1u) return "DBDE16 sums are U32 only";
        if (max_group > kGProjMaxGroupFramesU16) return "a U16 sum needs groups of at most 257 frames";
        if (accumulate) return "a U16 sum cannot accumulate";
    }
    if ((max_addr | min_addr) & (pix - 1u)) return "U16 planes must be 2-byte aligned";
    if (sum_addr & (sum_type == DBDE_HIP_SUM_U16 ? 1u : 3u)) return "d_sum is misaligned";
    if (sumsq_addr & 7u) return "d_sumsq must be 8-byte aligned";
    if (counts_addr & 3u) return "d_counts must be 4-byte aligned";
    pl.stats = stats;
    const uint32_t tiles = kProjTilesOf(pix);
    pl.pieces = (pl.roi.ntx + tiles - 1u) / tiles;
    pl.rows = pl.roi.nty;
    const uint64_t base = (uint64_t)pl.pieces * pl.rows, ng = (uint64_t)n_groups;
    const uint64_t target = 4ull * (uint64_t)(n_cu > 0 ? n_cu : 1);
    uint64_t runs = base >= target ? 1u : (target + base - 1u) / base;
    uint64_t per_group = has_starts ? (ng ? n / ng : 0u) : (uint64_t)group_frames;   // frames of a group (ragged: the mean)
    if (per_group < 1u) per_group = 1u;
    const uint64_t min_gpr = (kGProjMinFramesPerRun + per_group - 1u) / per_group;
    uint64_t gpr = ng ? (ng + runs - 1u) / runs : 1u;
    if (gpr < min_gpr) gpr = min_gpr;
    if (gpr > ng && ng) gpr = ng;
    if (gpr < 1u) gpr = 1u;
    runs = ng ? (ng + gpr - 1u) / gpr : 0u;   // no empty run
    pl.runs = (uint32_t)runs;
    pl.gpr = (uint32_t)gpr;
    pl.grid = base * runs;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t plane = (uint64_t)rw * (uint64_t)rh * ng;
    pl.max_bytes = (stats & kProjMax) ? pix * plane : 0u;
    pl.min_bytes = (stats & kProjMin) ? pix * plane : 0u;
    pl.sum_bytes = (stats & kProjSum) ? (sum_type == DBDE_HIP_SUM_U16 ? 2u : 4u) * plane : 0u;
    pl.sumsq_bytes = (stats & kProjSumSq) ? 8u * plane : 0u;
    pl.counts_bytes = 4u * ng;
    return nullptr;
}

static int groups_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                              int has_group_starts, int n_groups, int sum_type, int accumulate, uint64_t max_address,
                              uint64_t min_address, uint64_t sum_address, uint64_t sumsq_address,
                              uint64_t counts_address, int n_cu, uint32_t pix, dbde_hip_project_groups_plan_t *plan) {
    GroupsPlan pl;
    if (!plan || (has_group_starts != 0 && has_group_starts != 1) ||
        plan_groups(W, H, n_frames, x0, y0, rw, rh, group_frames, has_group_starts != 0, n_groups, sum_type, accumulate,
                    max_address, min_address, sum_address, sumsq_address, counts_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_window(plan, pl.roi);
    plan->threads = kProjThreads;
    plan->pieces_x = pl.pieces;
    plan->runs = pl.runs;
    plan->groups_per_run = pl.gpr;
    plan->max_group_frames = kGProjMaxGroupFrames;
    plan->stats = pl.stats;
    plan->grid = pl.grid;
    plan->sum_bytes = pl.sum_bytes;
    plan->max_bytes = pl.max_bytes;
    plan->min_bytes = pl.min_bytes;
    plan->sumsq_bytes = pl.sumsq_bytes;
    plan->counts_bytes = pl.counts_bytes;
    plan->workspace_bytes = 0;
    return DBDE_HIP_OK;
}

int dbde_hip_project_groups_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                                 int has_group_starts, int n_groups, int sum_type, int accumulate, uint64_t max_address,
                                 uint64_t min_address, uint64_t sum_address, uint64_t sumsq_address,
                                 uint64_t counts_address, int n_cu, dbde_hip_project_groups_plan_t *plan) {
    return groups_plan_common(W, H, n_frames, x0, y0, rw, rh, group_frames, has_group_starts, n_groups, sum_type,
                              accumulate, max_address, min_address, sum_address, sumsq_address, counts_address, n_cu, 1u,
                              plan);
}

int dbde16_hip_project_groups_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                                   int has_group_starts, int n_groups, int sum_type, int accumulate, uint64_t max_address,
                                   uint64_t min_address, uint64_t sum_address, uint64_t sumsq_address,
                                   uint64_t counts_address, int n_cu, dbde_hip_project_groups_plan_t *plan) {
    return groups_plan_common(W, H, n_frames, x0, y0, rw, rh, group_frames, has_group_starts, n_groups, sum_type,
                              accumulate, max_address, min_address, sum_address, sumsq_address, counts_address, n_cu, 2u,
                              plan);
}

// Both grouped projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the grouped kernel in slot 2.
static int project_groups_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                 size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                                 int x0, int y0, int rw, int rh, int group_frames, const uint32_t *d_group_starts,
                                 int n_groups, int sum_type, int accumulate, void *d_max, void *d_min, void *d_sum,
                                 uint64_t *d_sumsq, uint32_t *d_counts, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    GroupsPlan pl;
    if (const char *why = plan_groups(W, H, n_frames, x0, y0, rw, rh, group_frames, d_group_starts != nullptr, n_groups,
                                      sum_type, accumulate, reinterpret_cast<uintptr_t>(d_max),
                                      reinterpret_cast<uintptr_t>(d_min), reinterpret_cast<uintptr_t>(d_sum),
                                      reinterpret_cast<uintptr_t>(d_sumsq), reinterpret_cast<uintptr_t>(d_counts),
                                      ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, g=%d groups=%d)", name, why, W,
                    H, n_frames, rw, rh, x0, y0, group_frames, n_groups);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_groups == 0) return DBDE_HIP_OK;   // (uniform form, n_frames == 0)
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;
    GProjParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    p.n_frames = (uint32_t)n_frames;
    set_window(p, pl.roi, x0, y0, rw, rh);
    p.rows = pl.rows;
    p.pieces = pl.pieces;
    p.runs = pl.runs;
    p.gpr = pl.gpr;
    p.n_groups = (uint32_t)n_groups;
    p.group_frames = (uint32_t)group_frames;
    p.group_starts = d_group_starts;
    p.accumulate = accumulate;
    p.sum16 = sum_type == DBDE_HIP_SUM_U16 ? 1u : 0u;
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    p.out_counts = d_counts;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_gproject(p, pl.stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_groups(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                            int group_frames, const uint32_t *d_group_starts, int n_groups, int sum_type, int accumulate,
                            uint8_t *d_max, uint8_t *d_min, void *d_sum, uint64_t *d_sumsq, uint32_t *d_counts,
                            dbde_hip_frame_result *d_results) {
    return project_groups_common(ctx, "project_groups", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                 y0, rw, rh, group_frames, d_group_starts, n_groups, sum_type, accumulate, d_max, d_min,
                                 d_sum, d_sumsq, d_counts, d_results);
}

int dbde16_hip_project_groups(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                              int group_frames, const uint32_t *d_group_starts, int n_groups, int sum_type, int accumulate,
                              uint16_t *d_max, uint16_t *d_min, uint32_t *d_sum, uint64_t *d_sumsq, uint32_t *d_counts,
                              dbde_hip_frame_result *d_results) {
    return project_groups_common(ctx, "project_groups16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames,
                                 x0, y0, rw, rh, group_frames, d_group_starts, n_groups, sum_type, accumulate, d_max,
                                 d_min, d_sum, d_sumsq, d_counts, d_results);
}

// ---- region traces ----------------------------------------------------------------------------------------
struct dbde_hip_trace_map {
    dbde_hip_ctx *ctx;
    dbde_hip_trace_map_info_t info;
    uint8_t *dev;                     // one allocation: the layout of trace_map_layout
    const uint32_t *span_first[2];    // [pix - 1]: first active tile of each span, [spans + 1]
    uint32_t spans_x[2], spans[2];
    const uint32_t *tile_pos, *tile_kind;
    const uint16_t *blocks;
    const uint64_t *pixels;
};

namespace {

// The host side of a trace map: the active tiles in tile order, their words (the label of a whole tile, kTraceMixed |
// block of a mixed one), the mixed tiles' label blocks, the per-label pixel counts and each pixel size's spans.
struct HostTraceMap {
    dbde_hip_trace_map_info_t info;
    std::vector<uint32_t> pos, kind, span_first[2];
    std::vector<uint16_t> blocks;
    std::vector<uint64_t> pixels;
    uint32_t spans_x[2];
};

// nullptr when the labels are good, else what is wrong.  full: also the tile lists, blocks and spans.
const char *trace_classify(const int32_t *labels, int W, int H, int n_labels, HostTraceMap &m, bool full) {
    Geometry g;
    if (!labels) return "null labels";
    if (!geometry(W, H, g)) return "bad frame size";
    if (n_labels < 1 || n_labels > 65535) return "n_labels outside [1, 65535]";
    memset(&m.info, 0, sizeof m.info);
    m.info.W = W;
    m.info.H = H;
    m.info.n_labels = (uint32_t)n_labels;
    m.info.tiles = g.T;
    m.pixels.assign((size_t)n_labels, 0);
    for (size_t i = 0; i < g.pixels; i++)
        if (labels[i] < 0 || labels[i] > n_labels) return "a label outside [0, n_labels]";
    uint16_t blk[64];
    for (uint32_t ty = 0; ty < g.h; ty++) {
        for (uint32_t tx = 0; tx < g.w; tx++) {
            const uint32_t x0 = 8u * tx, y0 = 8u * ty;
            const uint32_t vw = (uint32_t)W - x0 < 8u ? (uint32_t)W - x0 : 8u, vh = (uint32_t)H - y0 < 8u ? (uint32_t)H - y0 : 8u;
            bool any = false, same = true;
            const int32_t first = labels[(size_t)y0 * W + x0];
            for (uint32_t y = 0; y < 8; y++) {
                for (uint32_t x = 0; x < 8; x++) {
                    int32_t l = 0;
                    if (y < vh && x < vw) {
                        l = labels[(size_t)(y0 + y) * W + x0 + x];
                        if (l) m.pixels[l - 1]++;
                        same = same && l == first;
                    }
                    any = any || l != 0;
                    blk[8 * y + x] = (uint16_t)l;
                }
            }
            if (!any) continue;
            const bool whole = same && vw == 8u && vh == 8u;
            m.info.tiles_active++;
            if (whole) m.info.tiles_whole++;
            else m.info.tiles_mixed++;
            if (!full) continue;
            m.pos.push_back(ty * g.w + tx);
            if (whole) {
                m.kind.push_back((uint32_t)first);
            } else {
                m.kind.push_back(kTraceMixed | (uint32_t)(m.blocks.size() / 64u));
                m.blocks.insert(m.blocks.end(), blk, blk + 64);
            }
        }
    }
    if (!full) return nullptr;
    for (uint32_t pix = 1; pix <= 2u; pix++) {
        const uint32_t K = kTraceTilesOf(pix), sx = (g.w + K - 1u) / K;
        std::vector<uint32_t> &sf = m.span_first[pix - 1u];
        m.spans_x[pix - 1u] = sx;
        sf.resize((size_t)sx * g.h + 1u);
        size_t a = 0;
        for (uint32_t s = 0; s < sx * g.h; s++) {   // spans in stream order: tiles [ty * w + (s % sx) * K, + K) of row ty
            const uint32_t ty = s / sx, p0 = ty * g.w + (s - ty * sx) * K;
            while (a < m.pos.size() && m.pos[a] < p0) a++;
            sf[s] = (uint32_t)a;
        }
        sf[(size_t)sx * g.h] = (uint32_t)m.pos.size();
    }
    return nullptr;
}

// Byte offsets of the device map: [span_first pix 1][span_first pix 2][tile_pos][tile_kind][blocks][pixels], each
// 16-byte aligned.
struct TraceMapLayout {
    size_t sf1, sf2, pos, kind, blocks, pixels, total;
};
TraceMapLayout trace_map_layout(const HostTraceMap &m) {
    auto up = [](size_t v) { return (v + 15u) & ~(size_t)15; };
    TraceMapLayout l;
    l.sf1 = 0;
    l.sf2 = l.sf1 + up(4u * m.span_first[0].size());
    l.pos = l.sf2 + up(4u * m.span_first[1].size());
    l.kind = l.pos + up(4u * m.pos.size());
    l.blocks = l.kind + up(4u * m.kind.size());
    l.pixels = l.blocks + up(2u * m.blocks.size());
    l.total = l.pixels + up(8u * m.pixels.size());
    return l;
}

}  // namespace

int dbde_hip_trace_map_summary(const int32_t *labels, int W, int H, int n_labels, dbde_hip_trace_map_info_t *info,
                               uint64_t *pixels) {
    HostTraceMap m;
    if (trace_classify(labels, W, H, n_labels, m, true)) return DBDE_HIP_ERR_ARG;
    m.info.device_bytes = trace_map_layout(m).total;
    if (info) *info = m.info;
    if (pixels) memcpy(pixels, m.pixels.data(), 8u * m.pixels.size());
    return DBDE_HIP_OK;
}

int dbde_hip_trace_map_create(dbde_hip_ctx *ctx, const int32_t *labels, int W, int H, int n_labels,
                              dbde_hip_trace_map **out) {
    if (!ctx || !out) return fail(ctx, DBDE_HIP_ERR_ARG, "trace_map_create: null pointer");
    *out = nullptr;
    HostTraceMap m;
    if (const char *why = trace_classify(labels, W, H, n_labels, m, true))
        return fail(ctx, DBDE_HIP_ERR_ARG, "trace_map_create: %s (W=%d H=%d n_labels=%d)", why, W, H, n_labels);
    const TraceMapLayout l = trace_map_layout(m);
    m.info.device_bytes = l.total;
    std::vector<uint8_t> host(l.total, 0);
    auto put = [&](size_t at, const void *src, size_t n) { if (n) memcpy(host.data() + at, src, n); };
    put(l.sf1, m.span_first[0].data(), 4u * m.span_first[0].size());
    put(l.sf2, m.span_first[1].data(), 4u * m.span_first[1].size());
    put(l.pos, m.pos.data(), 4u * m.pos.size());
    put(l.kind, m.kind.data(), 4u * m.kind.size());
    put(l.blocks, m.blocks.data(), 2u * m.blocks.size());
    put(l.pixels, m.pixels.data(), 8u * m.pixels.size());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *dev = nullptr;
    HIP_TRY(ctx, hipMalloc(&dev, l.total));
    hipError_t e = hipMemcpyAsync(dev, host.data(), l.total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return fail(ctx, DBDE_HIP_ERR_HIP, "trace_map_create: copy failed: %s", hipGetErrorString(e));
    }
    dbde_hip_trace_map *tm = new dbde_hip_trace_map;
    uint8_t *d = static_cast<uint8_t *>(dev);
    tm->ctx = ctx;
    tm->info = m.info;
    tm->dev = d;
    tm->span_first[0] = reinterpret_cast<const uint32_t *>(d + l.sf1);
    tm->span_first[1] = reinterpret_cast<const uint32_t *>(d + l.sf2);
    for (int k = 0; k < 2; k++) {
        tm->spans_x[k] = m.spans_x[k];
        tm->spans[k] = (uint32_t)(m.span_first[k].size() - 1u);
    }
    tm->tile_pos = reinterpret_cast<const uint32_t *>(d + l.pos);
    tm->tile_kind = reinterpret_cast<const uint32_t *>(d + l.kind);
    tm->blocks = reinterpret_cast<const uint16_t *>(d + l.blocks);
    tm->pixels = reinterpret_cast<const uint64_t *>(d + l.pixels);
    *out = tm;
    return DBDE_HIP_OK;
}

void dbde_hip_trace_map_destroy(dbde_hip_trace_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);   // queued traces may still read it
    (void)hipFree(m->dev);
    delete m;
}

int dbde_hip_trace_map_info(const dbde_hip_trace_map *m, dbde_hip_trace_map_info_t *info) {
    if (!m || !info) return DBDE_HIP_ERR_ARG;
    *info = m->info;
    return DBDE_HIP_OK;
}

const uint64_t *dbde_hip_trace_map_pixels(const dbde_hip_trace_map *m) { return m ? m->pixels : nullptr; }

namespace {

struct TracePlan {
    Geometry g;
    DecGeom dg;                       // the index's chunks (roi_index_geometry)
    uint32_t split, tiles, spans_x, spans, segments, fps;
    uint64_t grid, row_grid, workspace;
};
// Frames per segment: segments only fill the device (about 4 busy workgroups per CU, the busy spans counted as the
// fewest that can hold the active tiles) and never hold fewer than kTraceMinFramesPerSegment frames.  Segments cost no
// extra traffic: each (frame, span) is traced by one workgroup.
constexpr uint32_t kTraceMinFramesPerSegment = 16;
const char *plan_trace(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                       uint32_t pix, TracePlan &pl) {
    if (!info) return "null map info";
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, pl.g)) return "bad frame size";
    if (info->W != W || info->H != H) return "W / H differ from the map's";
    if (info->n_labels < 1u || info->n_labels > 65535u || info->tiles != pl.g.T || info->tiles_active > pl.g.T)
        return "map info does not describe a map of this frame size";
    if (stats < 1u || stats > kProjAll) return "no statistic (or an unknown one) requested";
    if (n_cu < 1) return "n_cu < 1";
    pl.dg = roi_index_geometry(pl.g.w, pl.g.h);
    if (pl.dg.cpf > kMaxChunksPerFrame) return "frame too large";
    if ((uint64_t)n_frames * (pl.dg.cpf + 1u) >= (1ull << 31)) return "too many chunks in one call";
    pl.split = index_split_for(n_frames, pl.dg.cpf);
    pl.tiles = kTraceTilesOf(pix);
    pl.spans_x = (pl.g.w + pl.tiles - 1u) / pl.tiles;
    pl.spans = pl.spans_x * pl.g.h;
    const uint64_t n = (uint64_t)n_frames;
    const uint64_t busy = info->tiles_active ? (info->tiles_active + pl.tiles - 1u) / pl.tiles : 1u;
    const uint64_t target = 4ull * (uint64_t)n_cu;
    uint64_t seg = busy >= target ? 1u : (target + busy - 1u) / busy;
    const uint64_t by_len = (n + kTraceMinFramesPerSegment - 1u) / kTraceMinFramesPerSegment;
    if (seg > by_len) seg = by_len;
    if (seg < 1u) seg = 1u;
    uint64_t fps = (n + seg - 1u) / seg;
    if (fps > 0u) seg = (n + fps - 1u) / fps;   // no empty segment
    pl.segments = (uint32_t)seg;
    pl.fps = (uint32_t)fps;
    pl.grid = (uint64_t)pl.spans * seg;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t rows = n * info->n_labels;
    pl.row_grid = (rows + kTraceRowThreads - 1u) / kTraceRowThreads;
    if (pl.row_grid >= (1ull << 31)) return "too many outputs in one call";
    const uint64_t ws = (4u * rows + 15u) & ~(uint64_t)15;
    pl.workspace = ((stats & kProjMax) ? ws : 0u) + ((stats & kProjMin) ? ws : 0u);
    return nullptr;
}

int trace_plan_common(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                      uint32_t pix, dbde_hip_trace_plan_t *plan) {
    TracePlan pl;
    if (!plan || plan_trace(W, H, n_frames, info, stats, n_cu, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    report_index(plan, pl.g, pl.dg, pl.split);
    plan->threads = kTraceThreads;
    plan->tiles_per_workgroup = pl.tiles;
    plan->spans_x = pl.spans_x;
    plan->spans = pl.spans;
    plan->segments = pl.segments;
    plan->frames_per_segment = pl.fps;
    plan->grid = pl.grid;
    plan->row_grid = pl.row_grid;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

// Both trace entry points: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the trace
// kernels in slot 2.  d_max / d_min hold U8 (pix 1) or U16 (pix 2) values.
int traces_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                  const uint64_t *d_frame_offsets, int W, int H, int n_frames, const dbde_hip_trace_map *map,
                  void *d_max, void *d_min, uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    if (!map) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null map", name);
    if (map->ctx != ctx) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the map belongs to another context", name);
    const unsigned stats = (d_max ? kProjMax : 0u) | (d_min ? kProjMin : 0u) | (d_sum ? kProjSum : 0u) |
                           (d_sumsq ? kProjSumSq : 0u);
    TracePlan pl;
    if (const char *why = plan_trace(W, H, n_frames, &map->info, stats, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, map %dx%d)", name, why, W, H, n_frames,
                    map->info.W, map->info.H);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (misaligned(7u, d_sum, d_sumsq))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if (misaligned(pix - 1u, d_max, d_min))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 outputs must be 2-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, pix, pl.split);
    if (rc) return rc;
    TraceParams p;
    memset(&p, 0, sizeof p);
    if (pl.workspace) {   // U32 max, then U32 min, [n_frames][n_labels] each, 16-byte aligned
        rc = grow(ctx, ctx->trace_ws, ctx->trace_ws_bytes, (size_t)pl.workspace, 1);
        if (rc) return rc;
        const uint64_t ws = (4u * (uint64_t)n_frames * map->info.n_labels + 15u) & ~(uint64_t)15;
        uint8_t *w = ctx->trace_ws;
        if (d_max) { p.ws_max = reinterpret_cast<uint32_t *>(w); w += ws; }
        if (d_min) p.ws_min = reinterpret_cast<uint32_t *>(w);
    }
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    p.n_frames = (uint32_t)n_frames;
    p.T = pl.g.T;
    p.w = pl.g.w;
    p.geom = pl.dg;
    p.spans_x = pl.spans_x;
    p.spans = pl.spans;
    p.segments = pl.segments;
    p.fps = pl.fps;
    p.n_labels = map->info.n_labels;
    p.pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    p.span_first = map->span_first[pix - 1u];
    p.tile_pos = map->tile_pos;
    p.tile_kind = map->tile_kind;
    p.blocks = map->blocks;
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_traces(p, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

}  // namespace

int dbde_hip_trace_plan(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                        dbde_hip_trace_plan_t *plan) {
    return trace_plan_common(W, H, n_frames, info, stats, n_cu, 1u, plan);
}

int dbde16_hip_trace_plan(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                          dbde_hip_trace_plan_t *plan) {
    return trace_plan_common(W, H, n_frames, info, stats, n_cu, 2u, plan);
}

int dbde_hip_traces(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                    int W, int H, int n_frames, const dbde_hip_trace_map *map, uint8_t *d_max, uint8_t *d_min,
                    uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results) {
    return traces_common(ctx, "traces", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, map, d_max, d_min,
                         d_sum, d_sumsq, d_results);
}

int dbde16_hip_traces(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                      int W, int H, int n_frames, const dbde_hip_trace_map *map, uint16_t *d_max, uint16_t *d_min,
                      uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results) {
    return traces_common(ctx, "traces16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, map, d_max,
                         d_min, d_sum, d_sumsq, d_results);
}

}  // extern "C"
