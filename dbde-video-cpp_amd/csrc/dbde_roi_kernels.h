// dbde_roi_kernels.h -- launch interface of the window (region-of-interest) decoder, dbde_roi_kernels.hip.
//
// The window decoder reuses the decode index kernel (dbde_kernels.hip: validation and per-chunk payload offsets,
// exactly as dbde_hip_decode_frames / dbde16_hip_decode_frames run them) and adds one kernel, templated on the pixel
// size, that decodes only the tiles a window covers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"

namespace dbde {

// Tiles of one window tile row that one workgroup takes: one tile per thread.
constexpr uint32_t kRoiWideThreads = 256;   // windows more than 64 tiles across
constexpr uint32_t kRoiNarrowThreads = 64;  // windows of at most 64 tiles across: one wave per workgroup

// Chunk geometry of the window decoder's index: chunks start at every tile row (one tile row per chunk while the frame
// is at most 512 tiles across, 512-tile pieces of a row when it is wider), so that the payload offset of any tile is its
// chunk's offset plus fewer than 512 depth bytes; plain 512-tile chunks when that would exceed kMaxChunksPerFrame.
__host__ __device__ inline DecGeom roi_index_geometry(uint32_t w, uint32_t h) {
    DecGeom g;
    g.w = w; g.h = h; g.T = w * h;
    const uint32_t pieces = (w + kChunkTiles - 1u) / kChunkTiles;
    if ((uint64_t)h * pieces <= kMaxChunksPerFrame) {
        g.ct = pieces == 1u ? w : kChunkTiles;
        g.pieces = pieces;
        g.cpf = h * pieces;
    } else {
        g.ct = kChunkTiles; g.pieces = 1u; g.cpf = (g.T + kChunkTiles - 1u) / kChunkTiles;
    }
    return g;
}

struct RoiParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    const int32_t *origins;         // optional [n_frames][2] (x, y), clamped into the frame; NULL -> (x0, y0)
    uint8_t *out;                   // [n_frames][rh][rw] pixels (U8; U16 for DBDE16 frames)
    int W, H;
    int x0, y0, rw, rh;
    uint32_t w, h, T;
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t rows;                  // window tile rows the grid provides for per frame (the most any origin needs)
    uint32_t pieces;                // workgroups per window tile row (the most any origin needs)
};

// DBDE16 (U16 pixels, depth <= 16, U16 minima): a tile carries up to 128 payload bytes and a 16-byte band row, twice
// the 8-bit kernel's LDS per tile; windows more than 64 tiles across take pieces of kRoi16WideThreads tiles
// (the width is a measured choice).
#ifndef DBDE_ROI16_WIDE_THREADS
#define DBDE_ROI16_WIDE_THREADS 128
#endif
constexpr uint32_t kRoi16WideThreads = DBDE_ROI16_WIDE_THREADS;
static_assert(kRoi16WideThreads == 64u || kRoi16WideThreads == 128u || kRoi16WideThreads == 256u, "a piece is 64, 128 or 256 tiles");

// One workgroup per (frame, window tile row, piece of `threads` tiles); grid = n_frames * rows * pieces.  pix: bytes per
// pixel, 1 = DBDE (threads kRoiNarrowThreads or kRoiWideThreads), 2 = DBDE16 (kRoiNarrowThreads or kRoi16WideThreads).
hipError_t launch_decode_roi(const RoiParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, hipStream_t s);

}  // namespace dbde
