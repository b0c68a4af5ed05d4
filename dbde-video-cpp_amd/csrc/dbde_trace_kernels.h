// dbde_trace_kernels.h -- launch interface of the region traces (dbde_hip_traces), dbde_trace_kernels.hip.
//
// A trace reduces each frame of a batch over the pixels of each labelled region: maximum, minimum, sum and sum of
// squares per (frame, label).  The regions come from a trace map (dbde_capi.cpp: built on the host from a label image);
// validation and the per-chunk payload offsets come from the decode index kernel run with the window decoder's chunk
// geometry (roi_index_geometry), exactly as dbde_hip_project runs it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"

namespace dbde {

// A workgroup takes one span: kTraceTilesOf(pix) consecutive tile columns of one tile row (the last span of a row may
// hold fewer), one lane per tile row (pix 1) or per half tile row (pix 2), as the projection kernel maps them.
constexpr uint32_t kTraceThreads = 256;
constexpr uint32_t kTraceTilesOf(uint32_t pix) { return kTraceThreads / (8u * pix); }
// Threads per workgroup of the init / finish kernels (one (frame, label) per thread).
constexpr uint32_t kTraceRowThreads = 256;
// Kinds of a trace map's tile word (TraceParams::tile_kind): a whole tile holds its label (1..65,535); a mixed tile
// holds kTraceMixed | its index into the label blocks (64 U16 labels each, padding 0).
constexpr uint32_t kTraceMixed = 0x80000000u;

struct TraceParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    uint32_t n_frames;
    uint32_t T, w;                  // tiles in the frame, tiles across
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t spans_x, spans;        // spans across a tile row; spans_x * tile rows
    uint32_t segments, fps;         // frame segments; frames per segment (the last may hold fewer)
    uint32_t n_labels;              // L: outputs are [n_frames][L], column j = label j + 1
    uint32_t pix_max;               // 255 (pix 1) or 65,535 (pix 2): the empty minimum
    // the map (device): active tiles [A] in tile order, the first active tile of each span [spans + 1] for this pixel
    // size, and the label blocks of the mixed tiles
    const uint32_t *span_first;
    const uint32_t *tile_pos, *tile_kind;
    const uint16_t *blocks;
    // outputs; NULL = not computed.  out_max / out_min are U8 (pix 1) or U16 (pix 2) arrays.
    uint8_t *out_max, *out_min;
    uint64_t *out_sum, *out_sumsq;
    // max / min through U32 workspace [n_frames][L] (there are no byte atomics); present when the output is
    uint32_t *ws_max, *ws_min;
};

// The trace kernels: trace_init_kernel (the accepted frames' rows: sums 0, max / min workspace to the empty values),
// trace_kernel<stats, pix> (grid = spans * segments workgroups of kTraceThreads), and, when max or min is requested,
// trace_finish_kernel<pix> (the accepted frames' max / min rows from the workspace).  Rejected frames' rows are never
// written.  stats: kProj* mask, 1..15; pix: 1 = DBDE, 2 = DBDE16.
hipError_t launch_traces(const TraceParams &p, uint32_t stats, uint32_t pix, hipStream_t s);

}  // namespace dbde
