// dbde_crop_kernels.h -- launch interface of the compressed-domain crop, dbde_crop_kernels.hip.
//
// The crop reuses the decode index kernel with the window decoder's chunk geometry (roi_index_geometry: validation and
// the payload offset of every tile row, exactly as dbde_hip_decode_roi runs it) and adds five kernels: a sizing pass,
// a re-pack of the few tiles the window's edge cuts, two scans that place rows and frames, and the copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_roi_kernels.h"

namespace dbde {

constexpr uint32_t kCropThreads = 256;        // size, row-scan and copy kernels: one workgroup per (frame, window tile row) / per frame
constexpr uint32_t kCropPlaceThreads = 256;   // the frame scan: one workgroup in all
// LDS of each kernel (the listing's group_segment_fixed_size; dbde_hip_crop_plan reports them)
constexpr uint32_t kCropSizeLds = 3u * (kCropThreads / 64u) * 4u;
constexpr uint32_t kCropRowsLds = (kCropThreads / 64u) * 4u;
constexpr uint32_t kCropPlaceLds = 2u * kCropPlaceThreads * 8u;
constexpr uint32_t kCropCopyLds = 0u;
constexpr uint32_t kCropRepackLds = 0u;

// Record of one re-packed tile (workspace): the payload words, then the new depth, the new minimum, the tile's word
// offset inside its window tile row's output and the payload word of its source tile.
constexpr uint32_t kCropRecBytes = 144;
constexpr uint32_t kCropRecDepth = 128, kCropRecMin = 132, kCropRecOff = 136, kCropRecSrc = 140;

struct CropParams {
    const uint8_t *stream;
    const uint64_t *frame_offsets;  // [n_frames]
    uint64_t stream_bytes;          // readable extent of stream
    const uint32_t *chunk_off;      // [n_frames][cpf + 1] from launch_decode_index
    const uint32_t *frame_ok;       // [n_frames]
    const int32_t *origins;         // optional [n_frames][2] (x, y): clamped into the frame, rounded down to 8
    int32_t *origins_used;          // optional [n_frames][2]
    uint8_t *out;
    uint64_t slot_stride;           // 0: concatenated
    uint64_t *out_offsets;          // optional [n_frames]
    uint64_t *out_bytes;            // optional [n_frames]
    // workspace
    uint32_t *row_src;              // [n_frames][nty] payload word (inside the source frame) of the row's first tile
    uint32_t *row_copy;             // [n_frames][nty] payload words copied verbatim
    uint32_t *row_words;            // [n_frames][nty] output words in front of the row (the row scan)
    uint64_t *frame_bytes;          // [n_frames] output frame length, 0 for a rejected frame
    uint64_t *frame_off;            // [n_frames] output frame start from `out`
    uint8_t *rec;                   // [n_frames][ntx + nty - 1] records of re-packed tiles
    int W, H;
    int x0, y0, rw, rh;
    uint32_t w, T;                  // source frame: tiles across, tiles
    DecGeom geom;                   // the index's chunk geometry (roi_index_geometry)
    uint32_t ntx, nty, Tout;        // the cropped frame: tiles across, down, in all
    uint32_t n_frames;
};

// pix: bytes per pixel, 1 = DBDE, 2 = DBDE16.  Launches on s: size (grid n_frames * nty), re-pack (n_frames *
// ceil((ntx + nty - 1) / 256); only if `repack`: some origin may cut a tile), row scan (n_frames), frame scan (1), copy
// (n_frames * nty).
hipError_t launch_crop(const CropParams &p, uint32_t pix, bool repack, hipStream_t s);

}  // namespace dbde
