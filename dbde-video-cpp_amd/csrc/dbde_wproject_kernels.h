// dbde_wproject_kernels.h -- launch interface of the weighted temporal projections (dbde_hip_project_weighted),
// dbde_wproject_kernels.hip.
//
// A weighted projection folds the rw x rh window of a batch of frames pixel by pixel over the frames into R F32 planes,
// out[r][y][x] = sum over the accepted frames f of w[r][f] * p_f[y][x], as a chain of fused multiply-adds in frame
// order.  Validation and the per-chunk payload offsets come from the decode index kernel run with the
// window decoder's chunk geometry (roi_index_geometry), exactly as dbde_hip_project runs it; the launch shape and the
// load pipeline are project_kernel's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_project_kernels.h"

namespace dbde {

// Regressors (weight rows, output planes) one launch folds: R * kWProjGroup weights of a group fit one wave's lanes 0-31.
constexpr uint32_t kWProjMaxRegressors = 8;
// Frames per pipeline step of wproject_kernel (its own constant: project_kernel's kProjGroup is not shared).
constexpr uint32_t kWProjGroup = 4;
// LDS of one wproject_kernel workgroup: the double-buffered wave totals of a group and write_count's wave counts.
constexpr uint32_t kWProjLdsBytes = 2u * kWProjGroup * 2u * (kProjThreads / 64u) * 4u + (kProjThreads / 64u) * 4u;

struct WProjParams {
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
    int accumulate;                 // 1: add this call's value to what the planes hold
    uint32_t regressors;            // R, 1..kWProjMaxRegressors
    const float *weights;           // weight of frame f for regressor r: weights[r * weight_stride + f]
    uint64_t weight_stride;
    float *out;                     // [R][rh][rw]
    uint64_t *out_count;
    float *ws;                      // per-segment partials [segments][R][rh * rw] (segments > 1 only)
};

// wproject_kernel<R, PIX> (pix: 1 = DBDE, 2 = DBDE16): grid = pieces * rows * segments workgroups of kProjThreads; with
// segments > 1 wproject_combine_kernel follows on the same stream.
hipError_t launch_wproject(const WProjParams &p, uint32_t regressors, uint32_t pix, hipStream_t s);
// Bytes of the per-segment partials of a window of `pixels` pixels: 4 * segments * regressors * pixels rounded up to 16
// (0 for one segment).
uint64_t wproject_workspace_bytes(uint32_t regressors, uint32_t segments, uint64_t pixels);

}  // namespace dbde
