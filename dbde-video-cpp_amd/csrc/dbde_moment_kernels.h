// dbde_moment_kernels.h -- launch interface of the patch moments, dbde_moment_kernels.hip.
//
// Patch moments reuse the decode index kernel on the window decoder's chunk geometry (roi_index_geometry: one index
// pass serves any number of patches) and add one kernel, templated on the pixel size, that reduces K small windows of
// one size per frame to eight thresholded image moments and a bounding box each, one 64-lane workgroup per patch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_roi_kernels.h"

namespace dbde {

constexpr uint32_t kMomentThreads = 64;     // one wave per workgroup, one tile per lane
constexpr uint32_t kMomentMaxTilesX = 64;   // a patch is never wider than the workgroup
constexpr int kMomentMaxHeight = 512;       // with pw <= 505: 65535 * 511^2 * 505 * 512 < 2^63, every sum fits 64 bits

constexpr uint32_t kMomentClamp = 0;   // the origin is clamped into the frame (the window decoder's rule)
constexpr uint32_t kMomentFill = 1;    // the patch sits where the origin says; pixels outside the frame count for nothing

constexpr uint32_t kMomentCount = 0;   // w = 1
constexpr uint32_t kMomentValue = 1;   // w = p
constexpr uint32_t kMomentAbove = 2;   // w = p - lo
constexpr uint32_t kMomentBelow = 3;   // w = hi - p

// LDS of one workgroup (PIX bytes per pixel): the payload ranges of G tile rows of mtx tiles each, G * mtx <= 64.  Every
// row's range takes 64 * PIX * mtx bytes, the 16-byte-aligned head and tail and the cutter's over-read 32 more (G <= 64).
__host__ __device__ constexpr uint32_t kMomentPayBytesOf(uint32_t pix) { return 4096u * pix + 32u * 64u; }
// Bytes between the payload ranges of two tile rows of a workgroup.
__host__ __device__ constexpr uint32_t kMomentRowBytesOf(uint32_t mtx, uint32_t pix) { return 64u * pix * mtx + 32u; }

struct MomentParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    const int32_t *origins;         // [n_frames][n_patches][2] (x, y)
    const uint32_t *counts;         // optional [n_frames]: live patches of the frame (clamped to n_patches)
    uint64_t *moments;              // [n_frames][n_patches][8]: N, S, Sx, Sy, Sxx, Sxy, Syy, Sww
    int32_t *bbox;                  // optional [n_frames][n_patches][4]: j_min, i_min, j_max, i_max
    int32_t *used;                  // optional [n_frames][n_patches][2]: the origin used
    int W, H;
    int pw, ph;
    uint32_t n_patches;
    uint32_t w, h, T;
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t mtx;                   // the most tiles a patch spans across (<= kMomentMaxTilesX)
    uint32_t G;                     // tile rows per step: max(1, 64 / mtx)
    uint32_t steps;                 // steps per patch: ceil(the most tile rows a patch spans / G)
    uint32_t mode;                  // kMomentClamp / kMomentFill
    uint32_t lo, hi;                // the band: a pixel p is selected when lo <= p <= hi
    uint32_t weight;                // kMomentCount / Value / Above / Below
    uint32_t block0;                // the workgroup number of this launch's first workgroup (launch_patch_moments sets it)
};

// A launch's grid is counted in work-items: workgroups * kMomentThreads must stay below 2^32.
constexpr uint32_t kMomentMaxGrid = (1u << 26) - 1u;

// One workgroup per (frame, patch): n_frames * n_patches of them (the host keeps that below 2^31), in as many launches
// of at most kMomentMaxGrid workgroups as that takes.  pix: bytes per pixel, 1 = DBDE, 2 = DBDE16.
hipError_t launch_patch_moments(const MomentParams &p, uint32_t n_frames, uint32_t pix, hipStream_t s);

}  // namespace dbde
