// dbde_mask_kernels.h -- launch interface of the threshold mask decode (dbde_hip_decode_mask), dbde_mask_kernels.hip.
//
// A mask decode writes one bit per pixel of the rw x rh window of each frame: whether the decoded value lies inside (or
// outside) the band [L, Hh], L and Hh from maps in the pixel type in frame coordinates or scalars.  The mask is U64
// [n_frames][rh][words], words = ceil(rw / 64), bit (c & 63) of word (c >> 6) of row r being window pixel (r, c); the
// optional outputs are the set bits per frame and their bounding box.  Validation and the per-chunk payload offsets come
// from the decode index kernel run with the window decoder's chunk geometry (roi_index_geometry), exactly as
// dbde_hip_decode_roi runs it; decode_mask_kernel has decode_roi_kernel's steps 1-3 (one tile per thread, its payload cut
// out of LDS into a band of pixels) and turns the band into mask words on its way out.
//
// Pieces are cut in WINDOW coordinates, not at tile boundaries of the frame: a workgroup owns up to kMaskPieceWordsOf(threads)
// whole mask words of one window tile row and decodes the tiles that overlap them.  64 k window pixels at any x mod 8
// overlap at most 8 k + 1 tiles, so k = threads / 8 - 1 words fit the one-tile-per-thread kernel.  No word is shared
// between workgroups: each leaves by one plain store, and a rejected frame's words need no clearing pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbde_kernels.h"
#include "dbde_roi_kernels.h"

namespace dbde {

// Modes: the values of DBDE_HIP_MASK_INSIDE / _OUTSIDE (include/dbde_hip.h).
constexpr uint32_t kMaskInside = 0, kMaskOutside = 1;

// Threads = the most tiles one workgroup decodes (one tile per thread): the window decoder's workgroup sizes.
constexpr uint32_t kMaskNarrowThreads = kRoiNarrowThreads;
constexpr uint32_t kMaskWideThreadsOf(uint32_t pix) { return pix == 1u ? kRoiWideThreads : kRoi16WideThreads; }
// The most mask words of one window row that one workgroup can own at any x mod 8: 64 k pixels overlap at most
// 8 k + 1 <= threads tiles.  When x is a multiple of 8 in every frame (no per-frame origins), threads / 8 words are
// exactly threads tiles.
constexpr uint32_t kMaskPieceWordsOf(uint32_t threads) { return threads / 8u - 1u; }
constexpr uint32_t kMaskAlignedPieceWordsOf(uint32_t threads) { return threads / 8u; }
// Windows of at most this many words take the narrow form (one wave per workgroup).
constexpr uint32_t kMaskNarrowWords = kMaskPieceWordsOf(kMaskNarrowThreads);
// LDS per workgroup: the piece's payload (threads tiles of depth 8 * pix, the aligned head and the cutter's over-read),
// reused as the band of 8 image rows in the pixel type; the block scan's 2 x waves words; one bit per 16-byte payload
// block (fetched or not: the decided-tile rule); the count and box of each wave; rounded up to 16 bytes.
constexpr uint32_t kMaskPayBytesOf(uint32_t threads, uint32_t pix) { return pix == 1u ? threads * 64u + 64u : threads * 128u + 32u; }
constexpr uint32_t kMaskNeedWordsOf(uint32_t threads, uint32_t pix) { return (4u * pix * threads + 1u + 31u) / 32u + 1u; }
constexpr uint32_t kMaskLdsBytesOf(uint32_t threads, uint32_t pix) {
    return (kMaskPayBytesOf(threads, pix) + 8u * (threads / 64u) + 4u * kMaskNeedWordsOf(threads, pix) + 20u * (threads / 64u) + 15u) & ~15u;
}

struct MaskParams {
    RoiParams roi;          // the window decoder's parameters; roi.out is unused, roi.pieces counts pieces of mask words
    const void *lo_map;     // optional [H][W] map in the pixel type, frame coordinates; NULL -> lo0
    const void *hi_map;     // optional [H][W] map in the pixel type, frame coordinates; NULL -> hi0
    uint32_t lo0, hi0;
    uint32_t outside;       // kMaskInside / kMaskOutside
    uint32_t words;         // ceil(rw / 64)
    uint32_t piece_words;   // words of a row per workgroup: roi.pieces = ceil(words / piece_words)
    uint64_t *mask;         // optional [n_frames][rh][words]
    uint32_t *counts;       // optional [n_frames], initialised by launch_mask_init
    int32_t *boxes;         // optional [n_frames][4], initialised by launch_mask_init
};

// counts[f] = 0 and boxes[f] = (rw, rh, -1, -1) for every frame (either may be NULL).
hipError_t launch_mask_init(uint32_t *counts, int32_t *boxes, uint32_t n_frames, int rw, int rh, hipStream_t s);

// One workgroup per (frame, window tile row, piece of p.piece_words words); grid = n_frames * roi.rows * roi.pieces.  pix: bytes per pixel, 1 = DBDE, 2 = DBDE16; threads: kMaskNarrowThreads or kMaskWideThreadsOf(pix).
hipError_t launch_decode_mask(const MaskParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, hipStream_t s);

}  // namespace dbde
