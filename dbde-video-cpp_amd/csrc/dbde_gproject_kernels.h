// dbde_gproject_kernels.h -- launch interface of the grouped projections (dbde_hip_project_groups),
// dbde_gproject_kernels.hip.
//
// A grouped projection reduces every run of frames ("group") of a batch to one set of planes: the per-pixel maximum,
// minimum, sum and sum of squares of the rw x rh window over the group's frames.  Validation and the per-chunk payload
// offsets come from the decode index kernel exactly as for dbde_hip_project; the kernel reads the window's tiles,
// accumulates them in registers and writes group k's planes when the group's last frame has been folded in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"

namespace dbde {

// Frames of one group: the U32 per-lane sums (and the DBDE U32 sums of squares) are exact up to this many.
constexpr uint32_t kGProjMaxGroupFrames = kProjMaxFramesPerSegment;
// Frames of one group whose DBDE sum still fits a U16 plane: 257 * 255 = 65,535.
constexpr uint32_t kGProjMaxGroupFramesU16 = 257;

struct GProjParams {
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
    uint32_t runs, gpr;             // runs of consecutive groups; groups per run (the last may hold fewer)
    uint32_t n_groups;
    uint32_t group_frames;          // uniform form: frames per group (group_starts == NULL)
    const uint32_t *group_starts;   // ragged form: [n_groups + 1], clamped by the kernel
    int accumulate;                 // 1: combine into what the planes and counts hold
    uint32_t sum16;                 // 1: out_sum is a U16 plane (DBDE, groups of at most 257 frames, no accumulate)
    // planes [n_groups][rh][rw]; NULL = not computed.  The DBDE16 kernels (pix 2) read out_max / out_min as U16 arrays.
    uint8_t *out_max, *out_min;
    void *out_sum;                  // U32, or U16 with sum16
    uint64_t *out_sumsq;
    uint32_t *out_counts;           // [n_groups]: accepted frames of each group
};

// The grouped projection kernel (one instance per statistics set, `stats` = kProj* mask, 1..15, and pixel size, pix:
// 1 = DBDE, 2 = DBDE16): grid = pieces * rows * runs workgroups of kProjThreads.
hipError_t launch_gproject(const GProjParams &p, uint32_t stats, uint32_t pix, hipStream_t s);

}  // namespace dbde
