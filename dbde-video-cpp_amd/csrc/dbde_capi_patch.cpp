// dbde_capi_patch.cpp -- the patch families of include/dbde_hip.h: many small windows per frame at per-patch origins
// (patch decode, patch moments, patch match).  Host side only; what they share with the other families is in
// dbde_host.h.
#include "dbde_host.h"

#include "dbde_match_kernels.h"
#include "dbde_moment_kernels.h"
#include "dbde_patch_kernels.h"

using namespace dbde;
using namespace dbde_host;

// ---- patch decode -------------------------------------------------------------------------------------------
struct PatchPlan {
    Geometry g;
    DecGeom dg;                       // the index's chunks (roi_index_geometry)
    uint32_t mtx, mty;                // the most tiles any origin makes a patch span
    uint32_t G, groups, split;
    uint64_t grid, out_bytes;
};
// nullptr when the arguments are good, else what is wrong with them.
static const char *plan_patches(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                                PatchPlan &pl) {
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, pl.g)) return "bad frame size";
    if (edge_mode != DBDE_HIP_PATCH_CLAMP && edge_mode != DBDE_HIP_PATCH_FILL) return "edge mode is neither CLAMP nor FILL";
    if (n_patches < 1) return "n_patches < 1";
    if (pw < 1 || ph < 1) return "patch size below 1";
    if (((uint32_t)pw + 6u) / 8u + 1u > kPatchMaxTilesX) return "a patch could be more than 64 tiles across (pw > 505)";
    const bool clamp = edge_mode == DBDE_HIP_PATCH_CLAMP;
    if (clamp && (pw > W || ph > H)) return "CLAMP mode: patch size outside [1, W] x [1, H]";
    pl.dg = roi_index_geometry(pl.g.w, pl.g.h);
    if (pl.dg.cpf > kMaxChunksPerFrame) return "frame too large";
    // x mod 8 reaches 7 in general, min(7, W - pw) over the origins clamping leaves (plan_roi)
    const uint64_t mx = clamp && (uint32_t)(W - pw) < 7u ? (uint32_t)(W - pw) : 7u;
    const uint64_t my = clamp && (uint32_t)(H - ph) < 7u ? (uint32_t)(H - ph) : 7u;
    pl.mtx = (uint32_t)((mx + (uint64_t)pw + 7u) / 8u);
    pl.mty = (uint32_t)((my + (uint64_t)ph + 7u) / 8u);
    pl.G = kPatchThreads / pl.mtx < 1u ? 1u : kPatchThreads / pl.mtx;
    pl.groups = (pl.mty + pl.G - 1u) / pl.G;
    pl.split = index_split_for(n_frames, pl.dg.cpf);
    // (n_frames, n_patches < 2^31 and groups < 2^29: np is bounded before it is multiplied by groups, so nothing wraps)
    const uint64_t np = (uint64_t)n_frames * (uint64_t)n_patches;
    if (np >= (1ull << 31)) return "too many workgroups in one call";
    pl.grid = np * pl.groups;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    if ((uint64_t)n_frames * (pl.dg.cpf + 1u) >= (1ull << 31)) return "too many chunks in one call";
    pl.out_bytes = np * (uint64_t)ph * (uint64_t)pw * pix;   // (ph <= 512 groups: np * ph < 2^40)
    return nullptr;
}

// The origins, sizes and geometry members that the params of the three patch families have.
template <typename Params>
static void set_patches(Params &p, const PatchPlan &pl, int W, int H, int pw, int ph, int n_patches,
                        const int32_t *d_origins, const uint32_t *d_counts, int32_t *d_used) {
    p.origins = d_origins;
    p.counts = d_counts;
    p.used = d_used;
    p.W = W;
    p.H = H;
    p.pw = pw;
    p.ph = ph;
    p.n_patches = (uint32_t)n_patches;
    p.w = pl.g.w;
    p.h = pl.g.h;
    p.T = pl.g.T;
    p.geom = pl.dg;
    p.mtx = pl.mtx;
    p.G = pl.G;
}

extern "C" {

static int patches_plan_common(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                               dbde_hip_patches_plan_t *plan) {
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (!plan || plan_patches(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->max_tiles_x = (int32_t)pl.mtx;
    plan->max_tiles_y = (int32_t)pl.mty;
    plan->rows_per_workgroup = pl.G;
    plan->groups_per_patch = pl.groups;
    plan->threads = kPatchThreads;
    report_index(plan, pl.g, pl.dg, pl.split);
    plan->lds_bytes = kPatchPayBytesOf(pix);
    plan->grid = pl.grid;
    plan->out_bytes = pl.out_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_patches_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                          dbde_hip_patches_plan_t *plan) {
    return patches_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 1u, plan);
}

int dbde16_hip_patches_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                            dbde_hip_patches_plan_t *plan) {
    return patches_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 2u, plan);
}

// Both patch decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the patch kernel in
// slot 2.
static int decode_patches_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                 size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw,
                                 int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode,
                                 uint32_t fill, void *d_out, int32_t *d_used, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (const char *why = plan_patches(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, %d patches of %dx%d, edge mode %d)", name, why, W, H,
                    n_frames, n_patches, pw, ph, edge_mode);
    if (!d_stream || !d_frame_offsets || !d_origins || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    const uint32_t pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    if (fill > pix_max) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: fill %u above %u", name, fill, pix_max);
    if (misaligned(pix - 1u, d_out))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the output must be %u-byte aligned", name, pix);
    if (misaligned(3u, d_origins, d_counts, d_used))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins, counts and used origins must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, pix, pl.split);
    if (rc) return rc;

    PatchParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_patches(p, pl, W, H, pw, ph, n_patches, d_origins, d_counts, d_used);
    p.out = static_cast<uint8_t *>(d_out);
    p.groups = pl.groups;
    p.mode = edge_mode == DBDE_HIP_PATCH_FILL ? kPatchFill : kPatchClamp;
    p.fill = fill;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_patches(p, (uint32_t)n_frames, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                            const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                            uint8_t *d_out, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return decode_patches_common(ctx, "decode_patches", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw,
                                 ph, n_patches, d_origins, d_counts, edge_mode, fill, d_out, d_used, d_results);
}

int dbde16_hip_decode_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                              const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                              uint16_t *d_out, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return decode_patches_common(ctx, "decode_patches16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw,
                                 ph, n_patches, d_origins, d_counts, edge_mode, fill, d_out, d_used, d_results);
}

// ---- patch moments ------------------------------------------------------------------------------------------
// The sizes and the edge mode are the patch decoder's (plan_patches); what is added is the height limit that keeps every
// sum inside 64 bits, and the launch: one workgroup per patch that walks the patch's groups of tile rows itself.
static const char *plan_moments(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                                PatchPlan &pl) {
    if (const char *why = plan_patches(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl)) return why;
    if (ph > kMomentMaxHeight) return "patch higher than 512 rows (the sums could pass 64 bits)";
    static_assert(kMomentMaxTilesX == kPatchMaxTilesX && kMomentThreads == kPatchThreads, "plan_patches' geometry is the kernel's");
    static_assert(kMomentClamp == DBDE_HIP_PATCH_CLAMP && kMomentFill == DBDE_HIP_PATCH_FILL, "edge modes");
    static_assert(kMomentCount == DBDE_HIP_MOMENT_COUNT && kMomentValue == DBDE_HIP_MOMENT_VALUE &&
                  kMomentAbove == DBDE_HIP_MOMENT_ABOVE && kMomentBelow == DBDE_HIP_MOMENT_BELOW, "weight modes");
    return nullptr;
}

static int moments_plan_common(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                               dbde_hip_patch_moments_plan_t *plan) {
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (!plan || plan_moments(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->max_tiles_x = (int32_t)pl.mtx;
    plan->max_tiles_y = (int32_t)pl.mty;
    plan->rows_per_workgroup = pl.G;
    plan->steps_per_patch = pl.groups;
    plan->threads = kMomentThreads;
    report_index(plan, pl.g, pl.dg, pl.split);
    plan->lds_bytes = kMomentPayBytesOf(pix);
    plan->grid = (uint64_t)n_frames * (uint64_t)n_patches;
    plan->moments_bytes = plan->grid * 64u;
    return DBDE_HIP_OK;
}

int dbde_hip_patch_moments_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                                dbde_hip_patch_moments_plan_t *plan) {
    return moments_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 1u, plan);
}

int dbde16_hip_patch_moments_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                                  dbde_hip_patch_moments_plan_t *plan) {
    return moments_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 2u, plan);
}

// Both calls: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the moments kernel in slot 2.
static int patch_moments_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw,
                                int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode,
                                uint32_t lo, uint32_t hi, int weight_mode, uint64_t *d_moments, int32_t *d_bbox,
                                int32_t *d_used, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (const char *why = plan_moments(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, %d patches of %dx%d, edge mode %d)", name, why, W, H,
                    n_frames, n_patches, pw, ph, edge_mode);
    if (!d_stream || !d_frame_offsets || !d_origins || !d_moments) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    const uint32_t pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    if (lo > pix_max || hi > pix_max)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: threshold %u above %u", name, lo > pix_max ? lo : hi, pix_max);
    if (weight_mode < DBDE_HIP_MOMENT_COUNT || weight_mode > DBDE_HIP_MOMENT_BELOW)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: unknown weight mode %d", name, weight_mode);
    if (misaligned(7u, d_moments))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the moments must be 8-byte aligned", name);
    if (misaligned(3u, d_origins, d_counts, d_used, d_bbox))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins, counts, boxes and used origins must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, pix, pl.split);
    if (rc) return rc;

    MomentParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_patches(p, pl, W, H, pw, ph, n_patches, d_origins, d_counts, d_used);
    p.moments = d_moments;
    p.bbox = d_bbox;
    p.steps = pl.groups;
    p.mode = edge_mode == DBDE_HIP_PATCH_FILL ? kMomentFill : kMomentClamp;
    p.lo = lo;
    p.hi = hi;
    p.weight = (uint32_t)weight_mode;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_patch_moments(p, (uint32_t)n_frames, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_patch_moments(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                           const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t lo, uint32_t hi,
                           int weight_mode, uint64_t *d_moments, int32_t *d_bbox, int32_t *d_used,
                           dbde_hip_frame_result *d_results) {
    return patch_moments_common(ctx, "patch_moments", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw, ph,
                                n_patches, d_origins, d_counts, edge_mode, lo, hi, weight_mode, d_moments, d_bbox, d_used,
                                d_results);
}

int dbde16_hip_patch_moments(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                             const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t lo, uint32_t hi,
                             int weight_mode, uint64_t *d_moments, int32_t *d_bbox, int32_t *d_used,
                             dbde_hip_frame_result *d_results) {
    return patch_moments_common(ctx, "patch_moments16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw,
                                ph, n_patches, d_origins, d_counts, edge_mode, lo, hi, weight_mode, d_moments, d_bbox,
                                d_used, d_results);
}

// ---- patch match --------------------------------------------------------------------------------------------
// The search patch's size and the edge mode go through the patch decoder's plan (plan_patches); what is added are the
// template and radius limits that keep an 8-bit entry inside 32 bits, the split of a shift's rows over lanes, and the LDS.
struct MatchPlan {
    PatchPlan pp;
    int pw, ph;
    uint32_t D, dwaves, steps, slices;
    MatchLayout lds;
    uint64_t surface_bytes;
};
static const char *plan_match(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                              int edge_mode, uint32_t fill, unsigned stats, uint32_t pix, MatchPlan &pl) {
    if (tw < 1 || th < 1 || tw > kMatchMaxTemplate || th > kMatchMaxTemplate) return "template size outside [1, 128]";
    if (S < 0 || S > kMatchMaxRadius) return "search radius outside [0, 16]";
    pl.pw = tw + 2 * S;
    pl.ph = th + 2 * S;
    if (const char *why = plan_patches(W, H, n_frames, pl.pw, pl.ph, n_patches, edge_mode, pix, pl.pp)) return why;
    if (fill > (pix == 1u ? 0xFFu : 0xFFFFu)) return "fill above the pixel type";
    if (n_templates != 1 && n_templates != n_patches) return "n_templates is neither 1 nor n_patches";
    if (stats == 0u || (stats & ~7u)) return "stats empty or with unknown bits";
    static_assert(kMatchClamp == DBDE_HIP_PATCH_CLAMP && kMatchFill == DBDE_HIP_PATCH_FILL, "edge modes");
    static_assert(kMatchProd == DBDE_HIP_MATCH_PROD && kMatchSum == DBDE_HIP_MATCH_SUM && kMatchSq == DBDE_HIP_MATCH_SQ, "surfaces");
    static_assert(kPatchThreads == 64u, "plan_patches' G is tile rows per wave");
    pl.D = 2u * (uint32_t)S + 1u;
    pl.dwaves = pl.pp.groups < kMatchWaves ? pl.pp.groups : kMatchWaves;
    pl.steps = (pl.pp.groups + pl.dwaves - 1u) / pl.dwaves;
    // the row slices: a lane's cost is its passes over the items times an item's cost, the batches of kMatchBatch dwords
    // in the rows of its slice plus a fixed part: ceil(nsh r / 256) * (ceil(th / r) * batches + kMatchItemCost).  The count
    // up to 16 (and th) with the least cost, the smallest on a tie
    const uint32_t nsh = pl.D * pl.D, rmax = (uint32_t)th < kMatchMaxSlices ? (uint32_t)th : kMatchMaxSlices;
    const uint32_t batches = (((uint32_t)tw * pix + 3u) / 4u + kMatchBatch - 1u) / kMatchBatch;
    uint32_t best = 0xFFFFFFFFu;
    pl.slices = 1u;
    for (uint32_t r = 1; r <= rmax; r++) {
        const uint32_t passes = (nsh * r + kMatchThreads - 1u) / kMatchThreads;
        const uint32_t cost = passes * ((((uint32_t)th + r - 1u) / r) * batches + kMatchItemCost);
        if (cost < best) {
            best = cost;
            pl.slices = r;
        }
    }
    pl.lds = match_layout(pix, (uint32_t)tw, (uint32_t)th, (uint32_t)S, pl.pp.mtx, pl.pp.mty, pl.pp.G, pl.dwaves, pl.slices);
    pl.surface_bytes = (uint64_t)n_frames * (uint64_t)n_patches * nsh * 8u;   // (below 2^31 * 1089 * 8)
    return nullptr;
}

static int match_plan_common(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                             int edge_mode, uint32_t fill, unsigned stats, uint32_t pix, dbde_hip_match_plan_t *plan) {
    MatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (!plan || plan_match(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->pw = pl.pw;
    plan->ph = pl.ph;
    plan->D = (int32_t)pl.D;
    plan->max_tiles_x = (int32_t)pl.pp.mtx;
    plan->max_tiles_y = (int32_t)pl.pp.mty;
    plan->rows_per_wave = pl.pp.G;
    plan->decode_waves = pl.dwaves;
    plan->steps_per_patch = pl.steps;
    plan->row_slices = pl.slices;
    plan->threads = kMatchThreads;
    report_index(plan, pl.pp.g, pl.pp.dg, pl.pp.split);
    plan->lds_bytes = pl.lds.bytes;
    plan->grid = (uint64_t)n_frames * (uint64_t)n_patches;
    plan->surface_bytes = pl.surface_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_match_plan(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                        int edge_mode, uint32_t fill, unsigned stats, dbde_hip_match_plan_t *plan) {
    return match_plan_common(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, 1u, plan);
}

int dbde16_hip_match_plan(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                          int edge_mode, uint32_t fill, unsigned stats, dbde_hip_match_plan_t *plan) {
    return match_plan_common(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, 2u, plan);
}

// Both calls: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the match kernel in slot 2.
static int match_patches_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int tw,
                                int th, int S, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                                int edge_mode, uint32_t fill, const void *d_templates, int n_templates, unsigned stats,
                                uint64_t *d_prod, uint64_t *d_sum, uint64_t *d_sq, int32_t *d_used,
                                dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    MatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (const char *why = plan_match(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, %d patches, %d templates of %dx%d, radius %d, edge mode %d, "
                    "fill %u, stats %u)", name, why, W, H, n_frames, n_patches, n_templates, tw, th, S, edge_mode, fill, stats);
    if (!d_stream || !d_frame_offsets || !d_origins || !d_templates) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (misaligned(pix - 1u, d_templates))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the templates must be %u-byte aligned", name, pix);
    uint64_t *const surf[3] = {d_prod, d_sum, d_sq};
    for (int i = 0; i < 3; i++)
        if ((stats >> i & 1u) && (!surf[i] || misaligned(7u, surf[i])))
            return fail(ctx, DBDE_HIP_ERR_ARG, "%s: a requested surface is null or not 8-byte aligned", name);
    if (misaligned(3u, d_origins, d_counts, d_used))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins, counts and used origins must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    int rc = index_pass(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.pp.dg, pix, pl.pp.split);
    if (rc) return rc;

    MatchParams p;
    memset(&p, 0, sizeof p);
    set_stream(p, ctx, d_stream, stream_bytes, d_frame_offsets);
    set_patches(p, pl.pp, W, H, pl.pw, pl.ph, n_patches, d_origins, d_counts, d_used);
    p.templates = static_cast<const uint8_t *>(d_templates);
    p.prod = (stats & DBDE_HIP_MATCH_PROD) ? d_prod : nullptr;
    p.sum = (stats & DBDE_HIP_MATCH_SUM) ? d_sum : nullptr;
    p.sq = (stats & DBDE_HIP_MATCH_SQ) ? d_sq : nullptr;
    p.tw = (uint32_t)tw;
    p.th = (uint32_t)th;
    p.D = pl.D;
    p.per_patch = n_templates == 1 ? 0u : 1u;
    p.dwaves = pl.dwaves;
    p.steps = pl.steps;
    p.slices = pl.slices;
    p.mode = edge_mode == DBDE_HIP_PATCH_FILL ? kMatchFill : kMatchClamp;
    p.fill = fill;
    p.stats = stats;
    p.lds = pl.lds;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_match_patches(p, (uint32_t)n_frames, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_match_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int tw, int th, int S,
                           int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                           const uint8_t *d_templates, int n_templates, unsigned stats, uint64_t *d_prod, uint64_t *d_sum,
                           uint64_t *d_sq, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return match_patches_common(ctx, "match_patches", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, tw, th, S,
                                n_patches, d_origins, d_counts, edge_mode, fill, d_templates, n_templates, stats, d_prod,
                                d_sum, d_sq, d_used, d_results);
}

int dbde16_hip_match_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int tw, int th, int S,
                             int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                             const uint16_t *d_templates, int n_templates, unsigned stats, uint64_t *d_prod, uint64_t *d_sum,
                             uint64_t *d_sq, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return match_patches_common(ctx, "match_patches16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, tw, th,
                                S, n_patches, d_origins, d_counts, edge_mode, fill, d_templates, n_templates, stats, d_prod,
                                d_sum, d_sq, d_used, d_results);
}

}  // extern "C"
