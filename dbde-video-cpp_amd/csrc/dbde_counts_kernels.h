// dbde_counts_kernels.h -- launch interface of the count projections (dbde_hip_project_counts),
// dbde_counts_kernels.hip.
//
// A count projection folds the rw x rh window of a batch of frames pixel by pixel over the frames into K U32 planes,
// out[k][y][x] = number of accepted frames f with p_f[y][x] <= thr_k(y, x), the thresholds K device scalars or K
// window-shaped maps.  Validation and the per-chunk payload offsets come from the decode index kernel
// run with the window decoder's chunk geometry (roi_index_geometry), exactly as dbde_hip_project runs it; the launch
// shape and the load pipeline are project_kernel's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"

namespace dbde {

// Levels (thresholds, output planes) one launch counts: K * (8 counters + 2 threshold registers) per lane.
constexpr uint32_t kCountsMaxLevels = 8;
// Frames per pipeline step of counts_kernel (its own constant: project_kernel's kProjGroup is not shared).
constexpr uint32_t kCountsGroup = 4;
// LDS of one counts_kernel workgroup: the double-buffered wave totals of a group and write_count's wave counts.
constexpr uint32_t kCountsLdsBytes = 2u * kCountsGroup * 2u * (kProjThreads / 64u) * 4u + (kProjThreads / 64u) * 4u;

struct CountsParams {
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
    int accumulate;                 // 1: add this call's counts to what the planes hold
    uint32_t levels;                // K, 1..kCountsMaxLevels
    int maps;                       // 0: thresholds[k] is level k's scalar; 1: thresholds[k * level_stride + y * rw + x]
    const void *thresholds;         // U8 (pix 1) or U16 (pix 2) elements
    uint64_t level_stride;          // elements between two maps (maps only)
    uint32_t *out;                  // [K][rh][rw]
    uint64_t *out_count;
    uint32_t *ws;                   // per-segment partials [segments][K][rh * rw] (segments > 1 only)
};

// counts_kernel<K, PIX> (pix: 1 = DBDE, 2 = DBDE16): grid = pieces * rows * segments workgroups of kProjThreads; with
// segments > 1 counts_combine_kernel follows on the same stream.
hipError_t launch_counts(const CountsParams &p, uint32_t levels, uint32_t pix, hipStream_t s);
// Bytes of the per-segment partials of a window of `pixels` pixels: 4 * segments * levels * pixels rounded up to 16
// (0 for one segment).
uint64_t counts_workspace_bytes(uint32_t levels, uint32_t segments, uint64_t pixels);

}  // namespace dbde
