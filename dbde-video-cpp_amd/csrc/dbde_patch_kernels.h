// dbde_patch_kernels.h -- launch interface of the patch decoder, dbde_patch_kernels.hip.
//
// The patch decoder reuses the decode index kernel on the window decoder's chunk geometry (roi_index_geometry: one
// index pass serves any number of windows) and adds one kernel, templated on the pixel size, that decodes K small
// windows of one size per frame, several tile rows of one patch per 64-lane workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_roi_kernels.h"

namespace dbde {

constexpr uint32_t kPatchThreads = 64;     // one wave per workgroup, one tile per lane
constexpr uint32_t kPatchMaxTilesX = 64;   // a patch is never wider than the workgroup

constexpr uint32_t kPatchClamp = 0;   // the origin is clamped into the frame (the window decoder's rule)
constexpr uint32_t kPatchFill = 1;    // the patch sits where the origin says; pixels outside the frame are `fill`

// LDS of one workgroup (PIX bytes per pixel).  G tile rows of mtx tiles each, G * mtx <= 64: every row's payload range
// takes 64 * PIX * mtx bytes, the 16-byte-aligned head and tail and the cutter's over-read 32 more (G <= 64 rows).
__host__ __device__ constexpr uint32_t kPatchPayBytesOf(uint32_t pix) { return 4096u * pix + 32u * 64u; }
// Bytes between the payload ranges of two tile rows of a workgroup.
__host__ __device__ constexpr uint32_t kPatchRowBytesOf(uint32_t mtx, uint32_t pix) { return 64u * pix * mtx + 32u; }

struct PatchParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    const int32_t *origins;         // [n_frames][n_patches][2] (x, y)
    const uint32_t *counts;         // optional [n_frames]: live patches of the frame (clamped to n_patches)
    uint8_t *out;                   // [n_frames][n_patches][ph][pw] pixels (U8; U16 for DBDE16 frames)
    int32_t *used;                  // optional [n_frames][n_patches][2]: the origin used
    int W, H;
    int pw, ph;
    uint32_t n_patches;
    uint32_t w, h, T;
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t mtx;                   // the most tiles a patch spans across (<= kPatchMaxTilesX)
    uint32_t G;                     // tile rows per workgroup: max(1, 64 / mtx)
    uint32_t groups;                // workgroups per patch: ceil(the most tile rows a patch spans / G)
    uint32_t mode;                  // kPatchClamp / kPatchFill
    uint32_t fill;                  // kPatchFill: the pixel outside the frame
    uint32_t block0;                // the workgroup number of this launch's first workgroup (launch_decode_patches sets it)
};

// A launch's grid is counted in work-items: workgroups * kPatchThreads must stay below 2^32.
constexpr uint32_t kPatchMaxGrid = (1u << 26) - 1u;

// One workgroup per (frame, patch, group of G tile rows): n_frames * n_patches * groups of them (the host keeps that
// below 2^31), in as many launches of at most kPatchMaxGrid workgroups as that takes.  pix: bytes per pixel, 1 = DBDE,
// 2 = DBDE16.
hipError_t launch_decode_patches(const PatchParams &p, uint32_t n_frames, uint32_t pix, hipStream_t s);

}  // namespace dbde
