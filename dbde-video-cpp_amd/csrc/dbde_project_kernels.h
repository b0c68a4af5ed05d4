// dbde_project_kernels.h -- launch interface of the temporal projections (dbde_hip_project), dbde_project_kernels.hip.
//
// A projection reduces the rw x rh window of a batch of frames pixel by pixel over the frames: maximum, minimum, sum
// and sum of squares.  Validation and the per-chunk payload offsets come from the decode index kernel
// (dbde_kernels.hip) run with the window decoder's chunk geometry (roi_index_geometry), exactly as dbde_hip_decode_roi
// runs it; the projection kernel reads the window's tiles and accumulates them in registers, writing no image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"

namespace dbde {

// Statistics bitmask (dbde_hip_project_plan's `stats`).
constexpr uint32_t kProjMax = 1u, kProjMin = 2u, kProjSum = 4u, kProjSumSq = 8u, kProjAll = 15u;

// A workgroup takes kProjTilesOf(pix) consecutive tiles of one window tile row: one lane per tile row (pix 1: 8 lanes
// per tile) or per half tile row (pix 2, DBDE16: 16 lanes per tile).
constexpr uint32_t kProjThreads = 256;
constexpr uint32_t kProjTilesOf(uint32_t pix) { return kProjThreads / (8u * pix); }
// Frames one workgroup reduces into its U32 per-lane sums: 65,536 * 255^2 < 2^32, so the sums of squares are exact.
// DBDE16 keeps the same bound through its U32 sums (65,536 * 65,535 < 2^32); its sums of squares are U64.
constexpr uint32_t kProjMaxFramesPerSegment = 65536;
// Threads per workgroup of the combine kernel (one window pixel per thread).
constexpr uint32_t kProjCombineThreads = 256;

struct ProjParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    uint32_t n_frames;
    int x0, y0, rw, rh;
    uint32_t T;
    uint32_t w;                     // tiles across the frame
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t tx0, ty0;              // the window's first tile column / row
    uint32_t rows, pieces;          // window tile rows; workgroups (of kProjTilesOf(pix) tiles) across one
    uint32_t segments, fps;         // frame segments; frames per segment (the last may hold fewer)
    int accumulate;                 // 1: combine into what the outputs hold
    // outputs (segments == 1: written by the projection kernel; otherwise by the combine kernel); NULL = not computed.
    // The DBDE16 kernels (pix 2) read out_max / out_min as U16 arrays.
    uint8_t *out_max, *out_min;
    uint64_t *out_sum, *out_sumsq, *out_count;
    // per-segment partials [segments][rh * rw] (segments > 1 only), present for the requested statistics.  The DBDE16
    // kernels read ws_max / ws_min as U16 arrays and ws_sumsq as a U64 array.
    uint8_t *ws_max, *ws_min;
    uint32_t *ws_sum, *ws_sumsq;
};

// The projection kernel (one instance per statistics set, `stats` = kProj* mask, 1..15, and pixel size, pix: 1 = DBDE,
// 2 = DBDE16): grid = pieces * rows * segments workgroups of kProjThreads; with segments > 1 the combine kernel follows
// on the same stream.
hipError_t launch_project(const ProjParams &p, uint32_t stats, uint32_t pix, hipStream_t s);
// The combine kernel alone, for a projection kernel of another family that writes project's partials (segments > 1):
// the partials of the planes of p that are not NULL -> the outputs, and the accepted frames -> *p.out_count.
hipError_t launch_project_combine(const ProjParams &p, uint32_t pix, hipStream_t s);
// Bytes of the per-segment partials of a window of `pixels` pixels (0 for one segment), laid out in the order max, min,
// sum, sumsq, each 16-byte aligned.  pix: 1 = DBDE (U8 max / min, U32 sums), 2 = DBDE16 (U16 max / min, U32 sums, U64
// sums of squares).
uint64_t project_workspace_bytes(uint32_t stats, uint32_t segments, uint64_t pixels, uint32_t pix);
// Bytes of one statistic's partials (bit: one of kProj*), rounded up to 16.
uint64_t project_partial_bytes(uint32_t bit, uint32_t segments, uint64_t pixels, uint32_t pix);

}  // namespace dbde
