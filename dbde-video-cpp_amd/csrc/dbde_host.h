// dbde_host.h -- what the translation units of the C-ABI's host layer share (dbde_capi*.cpp): the context, argument
// and error plumbing, the decode index pass, the window plan every window family starts from, and the few lines that
// each family's plan report and params fill have in common.  Internal: nothing here is part of include/dbde_hip.h;
// everything with external linkage lives in namespace dbde_host, whose names the library does not export (hidden
// visibility: calls between the translation units bind directly, as they did inside the one file).
#pragma once

#include "../../include/dbde_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"
#include "dbde_roi_kernels.h"

// goes on every opening of namespace dbde_host: a definition takes its visibility from the block it stands in
#define DBDE_HOST_HIDDEN __attribute__((visibility("hidden")))

namespace dbde_host DBDE_HOST_HIDDEN {

struct TimedSpan {
    hipEvent_t a, b;
    int kind;
};

struct Geometry {
    uint32_t w, h, T;
    uint64_t pixels;
};

}  // namespace dbde_host

struct dbde_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;         // dbde_hip_create_on_own_stream: destroyed with the context
    std::string err;
    std::string arch;

    // look-back workspace: [two sets of control words: 2 x 8 x u32][state: n_chunks x u64].  Zeroed when it is allocated
    // and after a failed launch; otherwise every launch leaves it as it found it (persistent encoder: each record is
    // cleared by its reader, the scanner clears the control words of the launch after it; small launches tag theirs)
    uint8_t *lb = nullptr;
    size_t lb_bytes = 0;
    uint32_t enc_parity = 0;         // which set of control words the next persistent launch uses
    // scan-ahead: a second stream so that the frame-to-frame walk of the NEXT batch runs beside the decode of this one
    hipStream_t scan_stream = nullptr;
    hipEvent_t scan_ev_main = nullptr, scan_ev_done = nullptr;
    // speculative stream walk: temporary position lists of the segments
    uint8_t *scan_ws = nullptr;
    size_t scan_ws_bytes = 0;
    // DBDE16 encode workspace (per-tile depth / minimum, chunk and frame totals, frame bases, arrival counter)
    uint8_t *w16 = nullptr;
    size_t w16_bytes = 0;
    bool lb_fresh = true;            // the block holds arbitrary bits (fresh allocation): a small launch zeroes it before its first use
    uint32_t enc_epoch = 0;          // tag of the last small encode launch's records (launch_encode_small)
    // decode workspace
    uint32_t *chunk_off = nullptr;
    size_t chunk_off_n = 0;
    uint32_t *frame_ok = nullptr;
    size_t frame_ok_n = 0;
    uint32_t *idx_ctr = nullptr;     // [2 * n]: arrival counters, then flags, of the split index kernel (kept zero)
    size_t idx_ctr_n = 0;
    unsigned long long *fuse_rec = nullptr;   // records of the fused index + decode launch (epoch-tagged, never cleared)
    uint8_t *proj_ws = nullptr;      // per-segment partials of dbde_hip_project
    size_t proj_ws_bytes = 0;
    uint8_t *trace_ws = nullptr;     // U32 max / min per (frame, label) of dbde_hip_traces
    size_t trace_ws_bytes = 0;
    uint8_t *crop_ws = nullptr;      // row and frame tables, records of re-packed tiles of dbde_hip_crop_frames
    size_t crop_ws_bytes = 0;
    size_t fuse_rec_n = 0;
    uint32_t fuse_epoch = 0;
    // sticky failure word (device) + scratch
    uint32_t *sticky = nullptr;
    uint64_t *scratch64 = nullptr;   // small device scratch: [0..3]
    // staging for the host-pointer entry points
    uint8_t *st_img = nullptr;
    size_t st_img_bytes = 0;
    uint8_t *st_pack = nullptr;
    size_t st_pack_bytes = 0;
    // ... and their pinned host twins (dbde_hip_set_host_staging): the caller's pageable bytes are copied through these
    // by the calling thread, so that the DMA never has to pin (and the runtime's pinning of pageable memory, which
    // serialises concurrent callers, is out of the way)
    uint64_t *h_words = nullptr;     // pinned, device-visible: [0] the encoder's byte count, [1..4] the decoder's frame result -- the kernels write them
                                     // straight into host memory, so a call has no small copies between its two big ones
    uint8_t *d_hdr = nullptr;        // a frame header {2, 0, 0} in device memory (dbde_hip_unpack_image puts it in front of the caller's frame data)
    int host_staging = 0;
    uint8_t *h_img = nullptr;
    size_t h_img_bytes = 0;
    uint8_t *h_pack = nullptr;
    size_t h_pack_bytes = 0;
    // timing
    uint32_t exp_flags = 0;          // $DBDE_HIP_EXPERIMENT (tuning experiments only)
    uint32_t enc_grid = 0;           // resident workgroups for the persistent encoder
    uint32_t enc16_grid = 0;         // the same for the DBDE16 encoder (queried at its first call)
    uint32_t wenc_grid[2] = {0, 0};  // the same for the window encoder, DBDE and DBDE16
    int n_cu = 0;
    int mid_dec_per_cu[2][3] = {};   // resident workgroups per CU of decode_mid_kernel (decode_mid_blocks_per_cu)
    uint64_t *diag = nullptr;        // [16] phase cycle sums of diagnostic launches
    bool timing = false;
    std::vector<dbde_host::TimedSpan> spans;
    double acc_ms[4] = {0, 0, 0, 0};     // encode, decode index, decode, stream scan
    uint64_t acc_n[4] = {0, 0, 0, 0};
};

namespace dbde_host DBDE_HOST_HIDDEN {

using namespace dbde;

// The plumbing below is defined in dbde_capi.cpp.
int fail(dbde_hip_ctx *ctx, int code, const char *fmt, ...);

#define HIP_TRY(ctx, expr)                                                                                 \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return dbde_host::fail(ctx, DBDE_HIP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

bool geometry(int W, int H, Geometry &g);

template <typename Ptr>
int grow(dbde_hip_ctx *ctx, Ptr &p, size_t &have, size_t want_elems, size_t elem_bytes, bool uncached = false) {
    if (want_elems <= have) return DBDE_HIP_OK;
    // everything queued may still be using the old block
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p) HIP_TRY(ctx, hipFree(p));
    p = nullptr;
    have = 0;
    size_t n = want_elems + want_elems / 4 + 64;
    void *q = nullptr;
    // chunk records are written by one CU and polled by others through sc1 atomics: keeping them out
    // of the (per-XCD, mutually incoherent) L2s measured 1.5-2.5 % faster; plain memory if refused
    if (uncached && hipExtMallocWithFlags(&q, n * elem_bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        q = nullptr;
    }
    if (!q) HIP_TRY(ctx, hipMalloc(&q, n * elem_bytes));
    p = reinterpret_cast<Ptr>(q);
    have = n;
    return DBDE_HIP_OK;
}

void span_begin(dbde_hip_ctx *ctx, int kind);
void span_end(dbde_hip_ctx *ctx);

// True when any of the pointers has a bit of `mask` set (NULL never has).
template <typename... P>
bool misaligned(uintptr_t mask, const P *...p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & mask) != 0;
}

// The stream half of a kernel's params: the caller's stream and the decode index's tables.
template <typename Params>
void set_stream(Params &p, const dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                const uint64_t *d_frame_offsets) {
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
}

// ---- the decode index pass ----------------------------------------------------------------------------------
// Index split of the decode index kernel: few frames are cut into pieces so that the index pass fills the device too
// (>= 4 chunks per piece, about 1024 workgroups in all); from 256 frames on, one workgroup per frame.
uint32_t index_split_for(int n_frames, uint32_t cpf);

// The decode index kernel in timing slot 1: validation, results and per-chunk payload offsets (ctx->chunk_off,
// ctx->frame_ok) of n_frames > 0 frames cut into the chunks of dg.  min_bytes: 1 = DBDE, 2 = DBDE16.  split: workgroups
// per frame (1, or the split form's index_split_for).  Shared by every decoder that runs the index as a launch of its own.
int run_index(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
              int n_frames, dbde_hip_frame_result *d_results, const DecGeom &dg, uint32_t min_bytes, uint32_t split);
// What the window families do once their arguments are good: select the context's device, then run_index when there
// are frames (a call that combines into its outputs may have none).
int index_pass(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
               int n_frames, dbde_hip_frame_result *d_results, const DecGeom &dg, uint32_t min_bytes, uint32_t split);

// The index part of a public plan struct.
template <typename Plan>
void report_index(Plan *plan, const Geometry &g, const DecGeom &dg, uint32_t split) {
    plan->chunks_per_frame = dg.cpf;
    plan->chunk_tiles = dg.ct;
    plan->chunk_pieces = dg.ct == g.w || dg.pieces > 1u ? dg.pieces : 0u;
    plan->index_split = split;
}

// ---- the window plan ----------------------------------------------------------------------------------------
struct RoiPlan {
    Geometry g;
    DecGeom dg;                       // the index's chunks (roi_index_geometry)
    uint32_t tx0, ty0, ntx, nty;      // the window at (x0, y0)
    uint32_t max_tx, max_ty;          // the most any origin needs
    uint32_t split, threads, pieces, pieces_fixed;
    uint64_t grid, grid_origins;
};
// nullptr when the arguments are good, else what is wrong with them.  wide: tiles per workgroup of windows more than 64
// tiles across (kRoiWideThreads for DBDE, kRoi16WideThreads for DBDE16).
const char *plan_roi(int W, int H, int n_frames, int x0, int y0, int rw, int rh, RoiPlan &pl,
                     uint32_t wide = kRoiWideThreads);

// The window tiles and the index part of a public plan struct.
template <typename Plan>
void report_window(Plan *plan, const RoiPlan &pl) {
    plan->tile_x = (int32_t)pl.tx0;
    plan->tile_y = (int32_t)pl.ty0;
    plan->tiles_x = (int32_t)pl.ntx;
    plan->tiles_y = (int32_t)pl.nty;
    report_index(plan, pl.g, pl.dg, pl.split);
}

// The window and geometry members of the params of a family that reads the window at (x0, y0) tile row by tile row.
template <typename Params>
void set_window(Params &p, const RoiPlan &pl, int x0, int y0, int rw, int rh) {
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.g.T;
    p.w = pl.g.w;
    p.geom = pl.dg;
    p.tx0 = pl.tx0;
    p.ty0 = pl.ty0;
}

// A RoiParams but for its stream half and its output (roi, scaled, mask).  pieces: workgroups across a window tile row,
// as the family counts them with and without per-frame origins.
void fill_roi_params(RoiParams &p, const RoiPlan &pl, int W, int H, int x0, int y0, int rw, int rh,
                     const int32_t *d_origins, uint32_t pieces);

// ---- segmented projections (dbde_capi_project.cpp) ----------------------------------------------------------
struct ProjectPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t stats;
    uint32_t pieces, rows, segments, fps;
    uint64_t grid, combine_grid, workspace;
};
// pix: 1 = DBDE (dbde_hip_project), 2 = DBDE16 (dbde16_hip_project: kProjTilesOf(2) tiles per workgroup, U16 / U64
// partials); the segment rule is the same for both.
const char *plan_project(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                         uint32_t pix, ProjectPlan &pl);
// The rows, segments, grids and workspace of a projection whose pieces across a window tile row are set (pl.pieces).
const char *plan_project_segments(int n_frames, int rw, int rh, int n_cu, uint32_t pix, ProjectPlan &pl);

// The launch part of a segmented projection's public plan struct.
template <typename Plan>
void report_segments(Plan *plan, const ProjectPlan &pl) {
    plan->threads = kProjThreads;   // (DBDE16: 16 lanes per tile, threads / 16 tiles)
    plan->pieces_x = pl.pieces;
    plan->segments = pl.segments;
    plan->frames_per_segment = pl.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->grid = pl.grid;
    plan->combine_grid = pl.combine_grid;
    plan->workspace_bytes = pl.workspace;
}

// The window, geometry and segment members that the params of every segmented projection have.
template <typename Params>
void set_projection(Params &p, const ProjectPlan &pl, int n_frames, int x0, int y0, int rw, int rh, int accumulate) {
    p.n_frames = (uint32_t)n_frames;
    set_window(p, pl.roi, x0, y0, rw, rh);
    p.rows = pl.rows;
    p.pieces = pl.pieces;
    p.segments = pl.segments;
    p.fps = pl.fps;
    p.accumulate = accumulate ? 1 : 0;
}

}  // namespace dbde_host
