// dbde_mask_kernels.hip -- threshold mask decode for MI355X (gfx950, wave64): one bit per pixel of the rw x rh window of
// each frame (inside / outside a band of values), the set bits per frame and their bounding box, straight from the
// compressed bytes (no integer image is written).
//
// decode_mask_kernel<THREADS, PIX>: PIX = 1 for DBDE frames (U8 pixels), PIX = 2 for DBDE16 frames (U16 pixels).  One
// workgroup per (frame, window tile row, piece), one tile per thread.  A piece is cut in WINDOW coordinates: k <=
// THREADS / 8 - 1 whole mask words (64 k window pixels) of the tile row's up to 8 window rows, and the workgroup decodes
// the at most 8 k + 1 <= THREADS tiles that overlap them, whatever x mod 8 is (per frame, with origins); the host may
// give THREADS / 8 words when every frame's x is a multiple of 8 (exactly THREADS tiles).  No mask word is shared
// between workgroups, so every word leaves by one plain store and a rejected frame's words stay untouched.
// Steps 1-3 are decode_roi_kernel's (dbde_roi_kernels.hip), repeated here so that the window decoder's listing stays as
// it is, with one addition, the decided tiles:
//   1. the tiles' depth / minimum bytes and one block scan for the payload offsets.  In the scalar form (no map) a tile
//      of depth d and minimum m whose range [m, m + 2^d - 1] does not wrap past the pixel maximum and lies wholly inside
//      the band or wholly outside it is DECIDED: every pixel of it has the verdict of m, so it is cut as a flat tile of
//      value m (depth 0) while its real depth still places its neighbours' payload;
//   2. the piece's payload range into LDS as aligned 16-byte blocks -- only the blocks that hold a byte of an undecided
//      tile (one bit per block in LDS, set by the tiles' threads): a decided tile's payload is not requested;
//   3. each undecided tile cut into registers and then into an LDS band of 8 image rows that reuses the payload buffer.
// Then
//   4. a wave takes 64 (window row, word) pairs of the piece at a time.  For each pair lane i compares window pixel
//      64 w + i of the row (its thresholds from the maps at FRAME coordinates, or the scalars) and __ballot is the word;
//      lane j keeps the word of pair j and the wave stores its words together, 8 bytes a lane.  The words' __popcll and the
//      first / last set bit (wave-uniform scalars) give the workgroup's count and box: one atomic each per workgroup
//      that has a set bit, onto the values mask_init_kernel wrote (integers: the result does not depend on the order).
// Latency is hidden by occupancy, as in decode_roi_kernel.
#include "dbde_mask_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

}  // namespace

__global__ __launch_bounds__(256) void mask_init_kernel(uint32_t *counts, int32_t *boxes, uint32_t n_frames, int rw, int rh) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= n_frames) return;
    if (counts) counts[f] = 0u;
    if (boxes) {
        boxes[4u * (size_t)f] = rw;
        boxes[4u * (size_t)f + 1u] = rh;
        boxes[4u * (size_t)f + 2u] = -1;
        boxes[4u * (size_t)f + 3u] = -1;
    }
}

template <uint32_t THREADS, uint32_t PIX>
__global__ __launch_bounds__(THREADS) void decode_mask_kernel(MaskParams mp) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Pix;
    typedef typename std::conditional<PIX == 1u, uint2, uint4>::type Row;   // one tile row of 8 pixels
    constexpr uint32_t NW = THREADS / 64u, PW = kMaskPieceWordsOf(THREADS), kPixMax = PIX == 1u ? 0xFFu : 0xFFFFu;
    constexpr uint32_t kPayBytes = kMaskPayBytesOf(THREADS, PIX), kNeedWords = kMaskNeedWordsOf(THREADS, PIX);
    constexpr uint32_t kPitch = THREADS * 8u;   // band row in pixels: THREADS tiles of 8 pixels
    static_assert(8u * PW + 1u <= THREADS, "the tiles that a piece's words overlap at any x mod 8: one per thread");
    static_assert(kNeedWords <= THREADS, "the block bits are cleared in one pass");
    // one block, so that the LDS is the sum the plan reports (rounded up to 16 bytes)
    struct __attribute__((aligned(16))) Lds {
        uint32_t pay[kPayBytes / 4u];   // the payload, then the band
        uint32_t wsum[2][NW];
        uint32_t need[kNeedWords];      // bit i: 16-byte block i of the piece's payload range holds an undecided tile's byte
        int32_t red[NW][5];             // per wave: count, x_min, y_min, x_max, y_max
    };
    static_assert(sizeof(Lds) == kMaskLdsBytesOf(THREADS, PIX), "the plan's LDS");
    __shared__ Lds lds;
    uint32_t *const s_pay = lds.pay;
    static_assert(8u * PIX * kPitch + 4u <= kPayBytes, "the band must fit the payload buffer");
    const Pix *band = reinterpret_cast<const Pix *>(s_pay);
    uint32_t (&s_wsum)[2][NW] = lds.wsum;
    uint32_t (&s_need)[kNeedWords] = lds.need;
    int32_t (&s_red)[NW][5] = lds.red;
    const RoiParams &p = mp.roi;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per_frame = p.rows * p.pieces;
    const uint32_t f = blockIdx.x / per_frame;
    const uint32_t rem = blockIdx.x - f * per_frame;
    const uint32_t br = rem / p.pieces, pc = rem - br * p.pieces;
    if (!p.frame_ok[f]) return;   // rejected frame: its words stay untouched, its count and box stay the initial ones

    int x = p.x0, y = p.y0;
    if (p.origins) {   // a tracker's moving window, clamped into the frame
        x = p.origins[2u * f];
        y = p.origins[2u * f + 1u];
        x = x < 0 ? 0 : (x > p.W - p.rw ? p.W - p.rw : x);
        y = y < 0 ? 0 : (y > p.H - p.rh ? p.H - p.rh : y);
    }
    const uint32_t ty_a = (uint32_t)y >> 3, ty_b = (uint32_t)(y + p.rh - 1) >> 3;
    const uint32_t ty = ty_a + br;
    const uint32_t w0 = pc * mp.piece_words;   // the piece's first word: window columns [64 w0, 64 (w0 + nwp)) up to rw
    if (ty > ty_b || w0 >= mp.words) return;   // the grid covers the most any origin needs
    const uint32_t nwp = mp.words - w0 < mp.piece_words ? mp.words - w0 : mp.piece_words;
    const uint32_t c_end = 64u * (w0 + nwp) < (uint32_t)p.rw ? 64u * (w0 + nwp) : (uint32_t)p.rw;   // window columns end
    const uint32_t txp = ((uint32_t)x + 64u * w0) >> 3;                   // first tile column of the piece
    const uint32_t nt = (((uint32_t)x + c_end - 1u) >> 3) + 1u - txp;   // <= THREADS: the host's choice of piece_words
    if (nt > THREADS) return;   // (never: a piece the plan does not make)

    // ---- 1. depth / minimum bytes, offsets (decode_roi_kernel's step 1), the decided tiles ----
    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;
    const uint32_t pos0 = ty * p.w + txp;
    const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
    const uint32_t base = p.chunk_off[(size_t)f * (p.geom.cpf + 1u) + c];
    const uint32_t npre = pos0 - cb;   // < 512 (roi_index_geometry)
    uint32_t pre = 0;
#pragma unroll
    for (uint32_t k = 0; k < kChunkTiles / THREADS; k++) {
        const uint32_t j = tid + k * THREADS;
        if (j < npre) pre += darr[cb + j];
    }
    uint32_t d = 0, mn = 0;
    if (tid < nt) {
        d = darr[pos0 + tid];
        if constexpr (PIX == 1u) {
            mn = marr[pos0 + tid];
        } else {   // the U16 minima start at 28 + T, possibly at an odd address: byte by byte
            const uint8_t *m = marr + 2u * (pos0 + tid);
            mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
        }
    }
    d = d > 8u * PIX ? 8u * PIX : d;   // (a validated frame has none)
    const Pix *lo_map = static_cast<const Pix *>(mp.lo_map), *hi_map = static_cast<const Pix *>(mp.hi_map);
    const uint32_t lo0 = mp.lo0, hi0 = mp.hi0;
    uint32_t dc = d;   // the depth the tile is cut with: 0 for a decided tile
    if (!lo_map && !hi_map && d) {
        const uint32_t top = mn + (1u << d) - 1u;   // the tile's values lie in [mn, top] when top does not wrap
        if (top <= kPixMax && ((mn >= lo0 && top <= hi0) || top < lo0 || mn > hi0 || lo0 > hi0)) dc = 0u;
    }
    const uint32_t incl = wave_scan_incl(d);
    const uint32_t pre_w = wave_sum(pre);
    if (lane == 63u) s_wsum[0][wave] = incl;
    if (lane == 0u) s_wsum[1][wave] = pre_w;
    if (tid < kNeedWords) s_need[tid] = 0u;
    __syncthreads();
    uint32_t wbase = 0, PRE = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const uint32_t v = s_wsum[0][k];
        wbase += k < wave ? v : 0u;
        PRE += s_wsum[1][k];
    }
    const uint32_t woff = wbase + incl - d;   // payload words in front of this tile inside the piece

    // ---- 2. the undecided tiles' payload into LDS (decode_roi_kernel's step 2, block by block on request) ----
    const uint8_t *src0 = pay + 8ull * ((uint64_t)base + PRE);
    const uint8_t *a_lo = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(src0) & ~(uintptr_t)15);
    const uint32_t sh = (uint32_t)(src0 - a_lo);
    if (dc) {   // blocks [k0, k1] hold this tile's 8 d bytes: at most 4 PIX + 1 blocks, two words of bits
        const uint32_t k0 = (sh + 8u * woff) >> 4, k1 = (sh + 8u * (woff + d) - 1u) >> 4;
        const uint64_t bits = ((1ull << (k1 - k0 + 1u)) - 1ull) << (k0 & 31u);
        atomicOr(&s_need[k0 >> 5], (uint32_t)bits);
        if (bits >> 32) atomicOr(&s_need[(k0 >> 5) + 1u], (uint32_t)(bits >> 32));
    }
    __syncthreads();
    const uint8_t *end = p.stream + p.stream_bytes;
    // Every bit of s_need, and no word behind it: i itself is bounded.  Only bits 0 .. 4 PIX THREADS can be set (the
    // blocks of sh + 8 S <= 15 + 64 PIX THREADS bytes), so a fetched block always lies inside the payload buffer.
    static_assert(kNeedWords * 32u > 4u * PIX * THREADS, "one bit for every block of the piece's payload range");
    static_assert(16u * (4u * PIX * THREADS + 1u) <= kPayBytes, "the last block that can be requested fits the payload buffer");
    for (uint32_t i = tid; i < kNeedWords * 32u; i += THREADS) {
        if (!((s_need[i >> 5] >> (i & 31u)) & 1u)) continue;
        const uint8_t *q = a_lo + 16u * i;
        uint4 v;
        if (q + 16 <= end) {
            const u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(q));   // streamed once
            v = make_uint4(t.x, t.y, t.z, t.w);
        } else {   // the block that crosses the readable extent: only the bytes in front of it
            uint32_t wq[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 16u; b++)
                if (q + b < end) wq[b >> 2] |= (uint32_t)q[b] << (8u * (b & 3u));
            v = make_uint4(wq[0], wq[1], wq[2], wq[3]);
        }
        *reinterpret_cast<uint4 *>(s_pay + 4u * i) = v;
    }
    __syncthreads();

    // ---- 3. tile rows -> registers -> the band (decode_roi_kernel's step 3; a decided tile is flat) ----
    Row px[8];
    if (tid < nt) {
        if (dc == 0u) {
            const uint32_t mm = PIX == 1u ? mn * 0x01010101u : mn * 0x00010001u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                if constexpr (PIX == 1u) px[r] = make_uint2(mm, mm);
                else px[r] = make_uint4(mm, mm, mm, mm);
            }
        } else if constexpr (PIX == 1u) {
            const uint32_t mm = mn * 0x01010101u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t o = sh + 8u * woff + r * d;   // byte of tile row r (8d bits)
                const uint32_t q0 = o >> 2, s = o & 3u;
                const uint32_t a0 = s_pay[q0], a1 = s_pay[q0 + 1u], a2 = s_pay[q0 + 2u];
                const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(a1, a0, s) |
                                      ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, s) << 32);
                uint32_t lo, hi;
                expand_row(bits, d, lo, hi);
                px[r] = make_uint2(add_bytes(lo, mm), add_bytes(hi, mm));
            }
        } else {
            const uint32_t byte0 = sh + 8u * woff;
            const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = mn * 0x00010001u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t a = byte0 + r * d, ah = a + (d >> 1);   // the row's two 4-pixel halves
                cut_row16(s_pay + (a >> 2), s_pay + (ah >> 2), a, ah, d, m32, mn2, px[r].x, px[r].y, px[r].z, px[r].w);
            }
        }
    }
    __syncthreads();   // every tile cut: the payload buffer becomes the band
    if (tid < nt) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++)
            *reinterpret_cast<Row *>(reinterpret_cast<uint8_t *>(s_pay) + PIX * (r * kPitch + 8u * tid)) = px[r];
    }
    __syncthreads();

    // ---- 4. the band -> the piece's mask words, count and box ----
    const int r_lo = 8 * (int)ty > y ? 8 * (int)ty : y;
    const int r_hi = 8 * (int)ty + 8 < y + p.rh ? 8 * (int)ty + 8 : y + p.rh;
    const uint32_t nr = (uint32_t)(r_hi - r_lo), by = (uint32_t)(r_lo - 8 * (int)ty);
    const uint32_t wr0 = (uint32_t)(r_lo - y);                                  // the band's first window row
    const uint32_t bc0 = (uint32_t)x + 64u * w0 - 8u * txp + lane;            // band column of this lane's pixel of word w0
    const uint32_t items = nr * nwp;                                            // (window row, word) pairs, row-major
    const bool outside = mp.outside != 0u;
    uint32_t cnt = 0;
    int bx_min = p.rw, by_min = p.rh, bx_max = -1, by_max = -1;
    for (uint32_t it0 = 64u * wave; it0 < items; it0 += 64u * NW) {
        const uint32_t n = items - it0 < 64u ? items - it0 : 64u;
        uint32_t row = it0 / nwp, wd = it0 - row * nwp;
        uint64_t mine = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t col = 64u * (w0 + wd) + lane;   // window column
            bool set = false;
            if (col < (uint32_t)p.rw) {
                const uint32_t v = band[(by + row) * kPitch + bc0 + 64u * wd];
                const size_t mi = (size_t)(r_lo + (int)row) * (size_t)p.W + (size_t)((uint32_t)x + col);
                const uint32_t L = lo_map ? (uint32_t)lo_map[mi] : lo0;
                const uint32_t Hh = hi_map ? (uint32_t)hi_map[mi] : hi0;
                set = (v >= L && v <= Hh) != outside;
            }
            const uint64_t b = __ballot(set);
            if (lane == j) mine = b;
            if (b) {
                const int xa = (int)(64u * (w0 + wd)) + __ffsll((unsigned long long)b) - 1;
                const int xb = (int)(64u * (w0 + wd)) + 63 - __clzll((long long)b);
                const int yy = (int)(wr0 + row);
                cnt += (uint32_t)__popcll(b);
                bx_min = xa < bx_min ? xa : bx_min;
                bx_max = xb > bx_max ? xb : bx_max;
                by_min = yy < by_min ? yy : by_min;
                by_max = yy > by_max ? yy : by_max;
            }
            if (++wd == nwp) { wd = 0; row++; }
        }
        if (mp.mask && lane < n) {
            const uint32_t it = it0 + lane, r = it / nwp, w = it - r * nwp;
            mp.mask[((size_t)f * (size_t)p.rh + wr0 + r) * (size_t)mp.words + w0 + w] = mine;
        }
    }
    if (!mp.counts && !mp.boxes) return;
    if (lane == 0u) {
        s_red[wave][0] = (int32_t)cnt;
        s_red[wave][1] = bx_min; s_red[wave][2] = by_min; s_red[wave][3] = bx_max; s_red[wave][4] = by_max;
    }
    __syncthreads();
    if (tid == 0u) {
#pragma unroll
        for (uint32_t k = 1; k < NW; k++) {
            cnt += (uint32_t)s_red[k][0];
            bx_min = s_red[k][1] < bx_min ? s_red[k][1] : bx_min;
            by_min = s_red[k][2] < by_min ? s_red[k][2] : by_min;
            bx_max = s_red[k][3] > bx_max ? s_red[k][3] : bx_max;
            by_max = s_red[k][4] > by_max ? s_red[k][4] : by_max;
        }
        if (cnt) {
            if (mp.counts) atomicAdd(mp.counts + f, cnt);
            if (mp.boxes) {
                int32_t *bx = mp.boxes + 4u * (size_t)f;
                atomicMin(bx, bx_min);
                atomicMin(bx + 1, by_min);
                atomicMax(bx + 2, bx_max);
                atomicMax(bx + 3, by_max);
            }
        }
    }
}

hipError_t launch_mask_init(uint32_t *counts, int32_t *boxes, uint32_t n_frames, int rw, int rh, hipStream_t s) {
    if ((!counts && !boxes) || n_frames == 0u) return hipSuccess;
    hipLaunchKernelGGL(mask_init_kernel, dim3((n_frames + 255u) / 256u), dim3(256), 0, s, counts, boxes, n_frames, rw, rh);
    return hipGetLastError();
}

hipError_t launch_decode_mask(const MaskParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, hipStream_t s) {
    if ((pix != 1u && pix != 2u) || (threads != kMaskNarrowThreads && threads != kMaskWideThreadsOf(pix)))
        return hipErrorInvalidValue;
    const uint32_t grid = n_frames * p.roi.rows * p.roi.pieces;   // (the host keeps it below 2^31)
    if (pix == 1u) {
        if (threads == kMaskNarrowThreads)
            hipLaunchKernelGGL((decode_mask_kernel<kMaskNarrowThreads, 1>), dim3(grid), dim3(kMaskNarrowThreads), 0, s, p);
        else
            hipLaunchKernelGGL((decode_mask_kernel<kMaskWideThreadsOf(1), 1>), dim3(grid), dim3(kMaskWideThreadsOf(1)), 0, s, p);
    } else {
        if (threads == kMaskNarrowThreads)
            hipLaunchKernelGGL((decode_mask_kernel<kMaskNarrowThreads, 2>), dim3(grid), dim3(kMaskNarrowThreads), 0, s, p);
        else
            hipLaunchKernelGGL((decode_mask_kernel<kMaskWideThreadsOf(2), 2>), dim3(grid), dim3(kMaskWideThreadsOf(2)), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace dbde
