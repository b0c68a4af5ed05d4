// dbde_binned_kernels.h -- launch interface of the binned decode (dbde_hip_decode_binned), dbde_binned_kernels.hip.
//
// A binned decode reduces the rw x rh window of each frame of a batch in bins of b x b pixels (b = 2, 4 or 8) to a sum,
// a maximum and a minimum plane of ceil(rh / b) x ceil(rw / b) elements per frame, straight from the compressed bytes.
// The window starts at a multiple of b, so no bin straddles a tile.  Validation and the per-chunk payload offsets come
// from the decode index kernel run with the window decoder's chunk geometry (roi_index_geometry), exactly as
// dbde_hip_decode_roi runs it; binned_kernel has decode_roi_kernel's front half (one tile per thread, its payload cut
// out of LDS) and reduces the tile's rows in registers instead of writing them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_roi_kernels.h"

namespace dbde {

// Tiles of one window tile row that one workgroup takes (one tile per thread): the window decoder's piece widths.
constexpr uint32_t kBinNarrowThreads = kRoiNarrowThreads;   // windows of at most 64 tiles across
constexpr uint32_t kBinWideThreadsOf(uint32_t pix) { return pix == 1u ? kRoiWideThreads : kRoi16WideThreads; }
// LDS per workgroup: the piece's payload (threads tiles of depth 8 * pix, the aligned head and the cutter's over-read),
// reused as the band of output rows (at b = 2 with all three planes exactly the payload's threads * 64 * pix bytes),
// and the block scan's 2 x waves words.
constexpr uint32_t kBinPayBytesOf(uint32_t threads, uint32_t pix) { return pix == 1u ? threads * 64u + 64u : threads * 128u + 32u; }
constexpr uint32_t kBinLdsBytesOf(uint32_t threads, uint32_t pix) { return kBinPayBytesOf(threads, pix) + 8u * (threads / 64u); }

struct BinnedParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    int x0, y0, rw, rh;             // x0, y0: multiples of the bin
    uint32_t w, T;                  // tiles across the frame, tiles of the frame
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t tx0, ty0;              // the window's first tile column / row
    uint32_t rows, pieces;          // window tile rows; workgroups per window tile row
    uint32_t ow, oh;                // the planes' columns and rows: ceil(rw / b), ceil(rh / b)
    // planes [n_frames][oh][ow]; NULL = not computed.  sum: U16 (pix 1) / U32 (pix 2); max, min: U8 / U16.
    void *out_sum, *out_max, *out_min;
};

// One workgroup per (frame, window tile row, piece of `threads` tiles); grid = n_frames * rows * pieces.  pix: bytes per
// pixel, 1 = DBDE, 2 = DBDE16; threads: kBinNarrowThreads or kBinWideThreadsOf(pix); bin: 2, 4 or 8.
hipError_t launch_decode_binned(const BinnedParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, uint32_t bin,
                                hipStream_t s);

}  // namespace dbde
