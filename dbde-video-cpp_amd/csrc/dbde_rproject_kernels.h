// dbde_rproject_kernels.h -- launch interface of the registered projections (dbde_hip_project_registered),
// dbde_rproject_kernels.hip.  DESIGN.md 4.22.
//
// A registered projection is dbde_hip_project's reduction (maximum, minimum, sum, sum of squares per pixel over the
// accepted frames) of an rw x rh window whose origin moves from frame to frame: frame f contributes the window at
// origins[f], clamped into the frame exactly as dbde_hip_decode_roi clamps.  Validation and the per-chunk payload
// offsets come from the decode index kernel with the window decoder's chunk geometry (roi_index_geometry).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_project_kernels.h"

namespace dbde {

// A workgroup decodes kProjTilesOf(pix) consecutive source tiles of each frame and owns the output columns they cover
// at every column residue: one tile fewer.
constexpr uint32_t kRProjColsOf(uint32_t pix) { return 8u * (kProjTilesOf(pix) - 1u); }
// Output rows per workgroup (one band).
constexpr uint32_t kRProjBandRows = 8;
// Frames per pipeline step; dwords of one band row in LDS: 256 bytes of decoded rows and the guard behind them that the
// re-aligning read (three dwords from byte 8 * slot + pix * (x & 7)) reaches.
constexpr uint32_t kRProjGroup = 4;
constexpr uint32_t kRProjRowDwords = 68;
// LDS of every instance: the band [2][group][8 rows][row dwords], the scans' wave sums [2][group][2 tile rows][2][4
// waves] and the count's wave sums.
constexpr uint32_t kRProjLdsBytes = 2u * kRProjGroup * kRProjBandRows * kRProjRowDwords * 4u + 2u * kRProjGroup * 2u * 2u * 4u * 4u + 16u;

// The instance (a superset of the requested statistics) that serves a mask: max | min, sum | sumsq, or all four.
constexpr uint32_t kRProjInstanceOf(uint32_t stats) {
    return (stats & ~(kProjMax | kProjMin)) == 0u ? (kProjMax | kProjMin) : (stats & ~(kProjSum | kProjSumSq)) == 0u ? (kProjSum | kProjSumSq) : kProjAll;
}

struct RProjParams {
    // project's parameters.  x0, y0, tx0 and ty0 are unused (the window has no fixed place in the frame); rows counts
    // the bands of kRProjBandRows output rows, pieces the workgroups of kRProjColsOf(pix) output columns across.
    ProjParams pj;
    const int32_t *origins;   // [n_frames][2] (x, y): any value, clamped into [0, W - rw] x [0, H - rh]
    int32_t *origins_used;    // optional [n_frames][2]: the clamped origin of every accepted frame
    int W, H;
};

// grid = pieces * rows * segments workgroups of kProjThreads; with segments > 1 project's combine kernel follows on the
// same stream.  stats: the requested statistics (the planes of p.pj that are not NULL); pix: 1 = DBDE, 2 = DBDE16.
hipError_t launch_rproject(const RProjParams &p, uint32_t stats, uint32_t pix, hipStream_t s);

}  // namespace dbde
