// dbde_wenc_kernels.h -- launch interface of the window encoder (dbde_wenc_kernels.hip): a pitched
// rw x rh window of each source image as a DBDE (PIX = 1) or DBDE16 (PIX = 2) frame, straight from the source bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dbde {

constexpr uint32_t kWencThreads = 256;        // one workgroup; a lane holds one UNIT: a pair of adjacent tiles (PIX = 1), one tile (PIX = 2)
constexpr uint32_t kWencGroup = 64;           // records per group of the two-level sums (one per lane of the summing wave)
constexpr uint32_t kWencPayWords = 4096;      // U64 of a chunk's worst case: 512 tiles x 8 words = 256 tiles x 16 words
constexpr uint32_t kWencLdsBytes = 32824;     // the listing's group segment (tests/test_wenc_listing.py)
constexpr uint32_t kWencBlocksPerCu = 4;      // LDS-bound: 160 KiB / 32,824 bytes
// tiles a full chunk holds (PIX = 1 with an odd number of tiles across: a row's last lane holds one tile, not two)
constexpr uint32_t wenc_chunk_tiles(uint32_t pix) { return pix == 2u ? kWencThreads : 2u * kWencThreads; }

struct WencParams {
    const uint8_t *images;          // source bytes: pixel (x, y) of image f at f * frame_stride + y * pitch + x * PIX
    uint64_t image_bytes;           // readable extent of images: nothing at or beyond it is read
    uint64_t pitch, frame_stride;   // bytes
    const int32_t *origins;         // optional [n_frames][2] (x, y), clamped into [0, W - rw] x [0, H - rh]
    int W, H, x0, y0, rw, rh;
    uint32_t narrow;                // rw * PIX < 16: every fetch byte by byte
    uint8_t *out;
    uint64_t *frame_offsets;        // optional [n_frames]
    uint64_t *frame_bytes;          // optional [n_frames]
    const uint64_t *indices;        // optional [n_frames] (DBDE)
    const uint64_t *elapsed_ns;     // optional [n_frames] (DBDE)
    uint64_t first_index;
    uint64_t slot_stride;           // 0 = frames concatenated
    uint32_t w, h, T;               // tiles of the WINDOW, counted from its own corner
    uint32_t lanes_per_row;         // PIX = 1: ceil(w / 2) pairs per tile row; PIX = 2: w
    uint32_t units;                 // h * lanes_per_row: lanes of work per frame
    uint32_t chunks_per_frame;      // ceil(units / kWencThreads)
    uint32_t n_frames;
    // workspace, zeroed before every launch
    unsigned long long *state;      // [n_frames * cpf] bit 63 = published, rest = payload words of the chunk
    unsigned long long *gsum;       // [n_frames * ceil(cpf / 64)] words of a frame's group of 64 chunks
    unsigned long long *fsize;      // [n_frames] words of a frame (concatenated layout)
    unsigned long long *fgsum;      // [ceil(n_frames / 64)] words of a group of 64 frames (concatenated layout)
    uint32_t *ticket;               // [0] arrival / ticket counter, [1] how chunk ids are claimed (0 undecided, 1 static, 2 tickets)
    uint32_t force_tickets;         // tests: skip the static assignment
    uint32_t *sticky;               // context-wide failure word, OR-ed on a look-back time-out
};

int wenc_blocks_per_cu(uint32_t pix);   // resident workgroups per CU (occupancy query), at most kWencBlocksPerCu
// grid = min(chunks of the launch, resident workgroups) persistent workgroups of kWencThreads
hipError_t launch_encode_window(const WencParams &p, uint32_t pix, uint32_t resident_blocks, hipStream_t s);

}  // namespace dbde
