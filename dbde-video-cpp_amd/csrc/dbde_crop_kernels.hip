// dbde_crop_kernels.hip -- compressed-domain crop for MI355X (gfx950, wave64): a window of each frame as a new frame.
//
// Tiles are independent and a tile's record is (depth byte, minimum, 8 * depth payload bytes), so the cropped frame of a
// window whose origin is a multiple of 8 is the window's depth bytes, minima and payload ranges COPIED under new counts.
// Only tiles that the window's right or bottom edge cuts differently from the source (the last tile column and / or the
// last tile row of the window) hold other valid pixels: they are decoded, padded as the format pads, and packed again.
//
// After the decode index (dbde_kernels.hip, roi_index_geometry: the payload offset of every tile row's chunk):
//   crop_size_kernel<PIX>   one workgroup per (frame, window tile row): the row's source payload offset (its chunk's
//                           offset plus fewer than 512 depth bytes), the payload words it copies, and the payload
//                           offset of each tile of it that is cut.
//   crop_repack_kernel<PIX> one thread per cut tile (dense: a cut tile costs about a hundred times a copied tile's
//                           sizing, and left to the sizing pass one lane of 256 works while the row waits): decode,
//                           pad, pack into a workspace record (new depth, minimum, payload).  Not launched when the
//                           host knows that nothing is cut.
//   crop_rows_kernel<PIX>   one workgroup per frame: the re-packed tiles' places inside a cut last row, the exclusive
//                           scan of the rows' output words, the frame's length.
//   crop_place_kernel       one workgroup: the frames' starts (slot layout: f * slot_stride; concatenated: the
//                           exclusive scan of the lengths, rejected frames counting 0), the caller's offsets / bytes.
//   crop_copy_kernel<PIX>   one workgroup per (frame, window tile row): the row's depth bytes and minima, its payload
//                           range (a contiguous copy between two different byte alignments), the re-packed tiles'
//                           payloads; row 0 also the header and the three counts.
// PIX = 1: DBDE (U8 minima, depth <= 8, payload at 32 + 2T); PIX = 2: DBDE16 (U16 minima, depth <= 16, 32 + 3T).
// Every stream and output offset is 64-bit.  Memory is written with vector stores only.
#include "dbde_crop_kernels.h"

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// What of a frame's window is cut: per frame, from its origin.
struct CropWindow {
    uint32_t tx, ty;          // first tile column / row
    uint32_t rm, dm;          // valid pixels of the last window tile column / row
    bool cut_col, cut_row;    // the last column / row holds other valid pixels than its source tiles: re-packed
};

__device__ __forceinline__ CropWindow crop_window(const CropParams &p, uint32_t f, int &x, int &y) {
    x = p.x0;
    y = p.y0;
    if (p.origins) {   // a tracker's moving window: clamped into the frame as decode_roi clamps it, then onto the tile grid
        x = p.origins[2u * f];
        y = p.origins[2u * f + 1u];
        x = x < 0 ? 0 : (x > p.W - p.rw ? p.W - p.rw : x);
        y = y < 0 ? 0 : (y > p.H - p.rh ? p.H - p.rh : y);
        x &= ~7;
        y &= ~7;
    }
    CropWindow c;
    c.tx = (uint32_t)x >> 3;
    c.ty = (uint32_t)y >> 3;
    c.rm = (uint32_t)p.rw - 8u * (p.ntx - 1u);
    c.dm = (uint32_t)p.rh - 8u * (p.nty - 1u);
    const uint32_t srm = (uint32_t)p.W - 8u * (c.tx + p.ntx - 1u), sdm = (uint32_t)p.H - 8u * (c.ty + p.nty - 1u);
    c.cut_col = c.rm != (srm < 8u ? srm : 8u);
    c.cut_row = c.dm != (sdm < 8u ? sdm : 8u);
    return c;
}

// Slot of a re-packed tile's record inside its frame's ntx + nty - 1: the last row's tiles first, then the last column's.
__device__ __forceinline__ uint32_t crop_slot(const CropParams &p, uint32_t i, uint32_t j) {
    return j == p.nty - 1u ? i : p.ntx + j;
}

__device__ __forceinline__ uint64_t load_u64_any(const uint8_t *q) {
    uint64_t v;
    __builtin_memcpy(&v, q, 8);
    return v;
}
__device__ __forceinline__ void store_u64_any(uint8_t *q, uint64_t v) { __builtin_memcpy(q, &v, 8); }

// One cut tile: decode (wrapping add, as every decoder here), keep its rm x dm valid pixels, repeat the last valid
// column and row over the rest (dbde_pack_8x8_partial's padding), pack again; returns the new depth.  Pixels travel as
// two 16-bit lanes per dword for both formats.  tp: the tile's 8 * d payload bytes (any alignment; nothing outside them
// is read).
template <uint32_t PIX>
__device__ __forceinline__ uint32_t repack_tile(const uint8_t *tp, uint32_t d, uint32_t mn, uint32_t rm, uint32_t dm, uint8_t *rec) {
    constexpr uint32_t kPixMask = PIX == 1u ? 0xFFu : 0xFFFFu;
    uint32_t v[32];
    const uint64_t m = (1ull << d) - 1ull;
#pragma unroll
    for (uint32_t h = 0; h < 16u; h++) {   // half row h: 4 pixels, the 4d bits at bit 4dh of the tile
        uint64_t bits = 0;
        if (d) {
            const uint32_t bit = 4u * d * h, byte = bit >> 3;
            const uint32_t a = byte < 8u * d - 8u ? byte : 8u * d - 8u;   // the 8 bytes read stay inside the tile
            bits = load_u64_any(tp + a) >> (8u * (byte - a) + (bit & 7u));
        }
        const uint32_t p0 = ((uint32_t)(bits & m) + mn) & kPixMask;
        const uint32_t p1 = ((uint32_t)((bits >> d) & m) + mn) & kPixMask;
        const uint32_t p2 = ((uint32_t)((bits >> (2u * d)) & m) + mn) & kPixMask;
        const uint32_t p3 = ((uint32_t)((bits >> (3u * d)) & m) + mn) & kPixMask;
        v[2u * h] = p0 | (p1 << 16);
        v[2u * h + 1u] = p2 | (p3 << 16);
    }
    // columns from rm on repeat column rm - 1, then rows from dm on repeat row dm - 1
#pragma unroll
    for (uint32_t r = 0; r < 8u; r++) {
        uint32_t last = 0;
#pragma unroll
        for (uint32_t c = 0; c < 8u; c++) {
            uint32_t &w = v[4u * r + (c >> 1)];
            const uint32_t px = (c & 1u) ? w >> 16 : w & 0xFFFFu;
            last = c < rm ? px : last;
            w = (c & 1u) ? (w & 0xFFFFu) | (last << 16) : (w & 0xFFFF0000u) | last;
        }
    }
#pragma unroll
    for (uint32_t r = 1; r < 8u; r++)
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) v[4u * r + k] = r < dm ? v[4u * r + k] : v[4u * r - 4u + k];

    uint32_t lo = v[0], hi = v[0];
#pragma unroll
    for (uint32_t i = 1; i < 32u; i++) { lo = pk_min_u16(lo, v[i]); hi = pk_max_u16(hi, v[i]); }
    const uint32_t nmn = (lo & 0xFFFFu) < (lo >> 16) ? (lo & 0xFFFFu) : (lo >> 16);
    const uint32_t nmx = (hi & 0xFFFFu) > (hi >> 16) ? (hi & 0xFFFFu) : (hi >> 16);
    const uint32_t nd = depth_of_range(nmx - nmn);
    const uint32_t mn2 = nmn * 0x00010001u;   // every 16-bit half >= nmn: no borrow crosses a half
    Funnel fn;
    fn.reset();
    uint32_t q = 0;
#pragma unroll
    for (uint32_t h = 0; h < 16u; h++) {
        uint64_t word;
        if (fn.push(pack_four16(v[2u * h] - mn2, v[2u * h + 1u] - mn2, nd), 4u * nd, word)) {
            *reinterpret_cast<uint64_t *>(rec + 8u * q) = word;
            q++;
        }
    }
    *reinterpret_cast<uint32_t *>(rec + kCropRecDepth) = nd;
    *reinterpret_cast<uint32_t *>(rec + kCropRecMin) = nmn;
    return nd;
}

// Exclusive scan of v over the workgroup (THREADS = 64 * NW) and its total; s: NW words of LDS.
template <uint32_t NW>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *s, uint32_t lane, uint32_t wave, uint32_t &total) {
    const uint32_t incl = wave_scan_incl(v);
    __syncthreads();   // the previous use of s is over
    if (lane == 63u) s[wave] = incl;
    __syncthreads();
    uint32_t base = 0, t = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const uint32_t x = s[k];
        base += k < wave ? x : 0u;
        t += x;
    }
    total = t;
    return base + incl - v;
}

}  // namespace

// Sizing: the row's source payload offset and the payload words it copies; the source payload offset of every cut tile.
// rm == srm for every tile column but the last and dm == sdm for every row but the last, so the tiles a row copies are
// a prefix of it: all of it, all but its last tile, or (the last row, cut) none.
template <uint32_t PIX>
__global__ __launch_bounds__(kCropThreads) void crop_size_kernel(CropParams p) {
    constexpr uint32_t NW = kCropThreads / 64u;
    __shared__ uint32_t s_sum[3][NW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t f = blockIdx.x / p.nty, j = blockIdx.x - f * p.nty;
    int x, y;
    const CropWindow cw = crop_window(p, f, x, y);
    if (j == 0u && tid == 0u && p.origins_used) {
        p.origins_used[2u * f] = x;
        p.origins_used[2u * f + 1u] = y;
    }
    if (!p.frame_ok[f]) return;   // rejected frame: nothing is sized, the row scan writes its length 0

    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint32_t pos0 = (cw.ty + j) * p.w + cw.tx;
    const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
    const uint32_t base = p.chunk_off[(size_t)f * (p.geom.cpf + 1u) + c];
    const uint32_t npre = pos0 - cb;   // < 512 (roi_index_geometry)
    uint32_t pre = 0;
#pragma unroll
    for (uint32_t k = 0; k < kChunkTiles / kCropThreads; k++) {
        const uint32_t i = tid + k * kCropThreads;
        if (i < npre) pre += darr[cb + i];
    }
    const bool row_cut = cw.cut_row && j == p.nty - 1u;
    const uint32_t ncopy = row_cut ? 0u : p.ntx - (cw.cut_col ? 1u : 0u);
    uint32_t sum = 0;
    for (uint32_t i = tid; i < ncopy; i += kCropThreads) {
        const uint32_t d = darr[pos0 + i];
        sum += d > 8u * PIX ? 8u * PIX : d;   // (a validated frame has none)
    }
    pre = wave_sum(pre);
    sum = wave_sum(sum);
    if (lane == 0u) { s_sum[0][wave] = pre; s_sum[1][wave] = sum; }
    __syncthreads();
    uint32_t row0 = base, copy_words = 0;   // payload word of the row's first tile; words copied
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) { row0 += s_sum[0][k]; copy_words += s_sum[1][k]; }
    uint8_t *recs = p.rec + (size_t)f * (p.ntx + p.nty - 1u) * kCropRecBytes;
    if (row_cut) {   // every tile of the row is re-packed: each one's payload word
        uint32_t carry = 0;
        for (uint32_t i0 = 0; i0 < p.ntx; i0 += kCropThreads) {
            const uint32_t i = i0 + tid;
            uint32_t d = i < p.ntx ? darr[pos0 + i] : 0u;
            d = d > 8u * PIX ? 8u * PIX : d;
            uint32_t tot;
            const uint32_t at = carry + block_scan_excl<NW>(d, s_sum[2], lane, wave, tot);
            if (i < p.ntx) *reinterpret_cast<uint32_t *>(recs + (size_t)crop_slot(p, i, j) * kCropRecBytes + kCropRecSrc) = row0 + at;
            carry += tot;
        }
    } else if (cw.cut_col && tid == 0u) {
        *reinterpret_cast<uint32_t *>(recs + (size_t)crop_slot(p, p.ntx - 1u, j) * kCropRecBytes + kCropRecSrc) = row0 + copy_words;
    }
    if (tid == 0u) {
        const size_t r = (size_t)f * p.nty + j;
        p.row_src[r] = row0;
        p.row_copy[r] = copy_words;
    }
}

// Re-pack: one thread per record slot of a frame (the last window tile row's tiles, then the last column's); the
// slots whose tile this frame's origin does not cut do nothing.
template <uint32_t PIX>
__global__ __launch_bounds__(kCropThreads) void crop_repack_kernel(CropParams p) {
    const uint32_t slots = p.ntx + p.nty - 1u, per_frame = (slots + kCropThreads - 1u) / kCropThreads;
    const uint32_t f = blockIdx.x / per_frame, slot = (blockIdx.x - f * per_frame) * kCropThreads + threadIdx.x;
    if (slot >= slots || !p.frame_ok[f]) return;
    int x, y;
    const CropWindow cw = crop_window(p, f, x, y);
    const uint32_t i = slot < p.ntx ? slot : p.ntx - 1u, j = slot < p.ntx ? p.nty - 1u : slot - p.ntx;
    if (!((cw.cut_row && j == p.nty - 1u) || (cw.cut_col && i == p.ntx - 1u))) return;
    const uint8_t *fb = p.stream + p.frame_offsets[f];
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;
    const uint32_t pos = (cw.ty + j) * p.w + cw.tx + i;
    uint32_t d = fb[24 + pos], mn;
    d = d > 8u * PIX ? 8u * PIX : d;
    if constexpr (PIX == 1u) {
        mn = marr[pos];
    } else {
        const uint8_t *m = marr + 2u * (size_t)pos;
        mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
    }
    uint8_t *rec = p.rec + ((size_t)f * slots + slot) * kCropRecBytes;
    repack_tile<PIX>(pay + 8ull * *reinterpret_cast<const uint32_t *>(rec + kCropRecSrc), d, mn, i == p.ntx - 1u ? cw.rm : 8u,
                     j == p.nty - 1u ? cw.dm : 8u, rec);
}

// Per frame: the re-packed tiles' word offsets inside the last row, the words in front of each row, the frame's length.
template <uint32_t PIX>
__global__ __launch_bounds__(kCropThreads) void crop_rows_kernel(CropParams p) {
    constexpr uint32_t NW = kCropThreads / 64u;
    __shared__ uint32_t s_sum[NW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t f = blockIdx.x;
    if (!p.frame_ok[f]) {
        if (tid == 0u) p.frame_bytes[f] = 0;
        return;
    }
    int x, y;
    const CropWindow cw = crop_window(p, f, x, y);
    uint8_t *recs = p.rec + (size_t)f * (p.ntx + p.nty - 1u) * kCropRecBytes;
    uint32_t last_words = 0;   // re-packed words of the last row
    if (cw.cut_row) {
        for (uint32_t i0 = 0; i0 < p.ntx; i0 += kCropThreads) {
            const uint32_t i = i0 + tid;
            uint8_t *rec = recs + (size_t)(i < p.ntx ? i : 0u) * kCropRecBytes;
            const uint32_t nd = i < p.ntx ? *reinterpret_cast<const uint32_t *>(rec + kCropRecDepth) : 0u;
            uint32_t tot;
            const uint32_t ex = block_scan_excl<NW>(nd, s_sum, lane, wave, tot);
            if (i < p.ntx) *reinterpret_cast<uint32_t *>(rec + kCropRecOff) = last_words + ex;
            last_words += tot;
        }
    } else if (cw.cut_col) {
        last_words = *reinterpret_cast<const uint32_t *>(recs + (size_t)(p.ntx - 1u) * kCropRecBytes + kCropRecDepth);
    }
    const uint32_t *copy = p.row_copy + (size_t)f * p.nty;
    uint32_t *words = p.row_words + (size_t)f * p.nty;
    uint32_t carry = 0;
    for (uint32_t j0 = 0; j0 < p.nty; j0 += kCropThreads) {
        const uint32_t j = j0 + tid;
        uint32_t v = 0;
        if (j < p.nty) {
            v = copy[j];
            if (j == p.nty - 1u) v += last_words;
            else if (cw.cut_col) v += *reinterpret_cast<const uint32_t *>(recs + (size_t)(p.ntx + j) * kCropRecBytes + kCropRecDepth);
        }
        uint32_t tot;
        const uint32_t ex = block_scan_excl<NW>(v, s_sum, lane, wave, tot);
        if (j < p.nty) words[j] = carry + ex;
        carry += tot;
    }
    if (tid == 0u) p.frame_bytes[f] = 32ull + (PIX + 1ull) * p.Tout + 8ull * carry;
}

// One workgroup: where every frame starts.  Concatenated: the exclusive scan of the lengths (a rejected frame has
// length 0 and reports the position the next accepted frame takes); slot layout: f * slot_stride.
__global__ __launch_bounds__(kCropPlaceThreads) void crop_place_kernel(CropParams p) {
    __shared__ uint64_t s_scan[2][kCropPlaceThreads];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t f0 = 0; f0 < p.n_frames; f0 += kCropPlaceThreads) {
        const uint32_t f = f0 + tid;
        const uint64_t nb = f < p.n_frames ? p.frame_bytes[f] : 0ull;
        uint32_t cur = 0;
        s_scan[0][tid] = nb;
        __syncthreads();
#pragma unroll
        for (uint32_t o = 1; o < kCropPlaceThreads; o <<= 1) {
            const uint64_t a = s_scan[cur][tid] + (tid >= o ? s_scan[cur][tid - o] : 0ull);
            s_scan[cur ^ 1u][tid] = a;
            cur ^= 1u;
            __syncthreads();
        }
        const uint64_t incl = s_scan[cur][tid], tot = s_scan[cur][kCropPlaceThreads - 1u];
        __syncthreads();   // every read of this round is over before the next round writes
        if (f < p.n_frames) {
            const uint64_t off = p.slot_stride ? (uint64_t)f * p.slot_stride : carry + incl - nb;
            p.frame_off[f] = off;
            if (p.out_offsets) p.out_offsets[f] = off;
            if (p.out_bytes) p.out_bytes[f] = nb;
        }
        carry += tot;
    }
}

namespace {

// The 16 bytes at q (16-byte aligned), those at or beyond `end` as 0.
__device__ __forceinline__ uint4 load16_inside(const uint8_t *q, const uint8_t *end) {
    if (q + 16 <= end) {
        const u32x4_t t = *reinterpret_cast<const u32x4_t *>(q);
        return make_uint4(t.x, t.y, t.z, t.w);
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16u; b++)
        if (q + b < end) w[b >> 2] |= (uint32_t)q[b] << (8u * (b & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

template <uint32_t PIX>
__global__ __launch_bounds__(kCropThreads) void crop_copy_kernel(CropParams p) {
    const uint32_t tid = threadIdx.x;
    const uint32_t f = blockIdx.x / p.nty, j = blockIdx.x - f * p.nty;
    if (!p.frame_ok[f]) return;   // rejected frame: nothing is written
    int x, y;
    const CropWindow cw = crop_window(p, f, x, y);
    const uint8_t *fb = p.stream + p.frame_offsets[f];
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;
    const uint8_t *end = p.stream + p.stream_bytes;
    uint8_t *ob = p.out + p.frame_off[f];
    uint8_t *odep = ob + 24, *omin = ob + 28 + (uint64_t)p.Tout, *opay = ob + 32 + (PIX + 1ull) * p.Tout;
    const size_t r = (size_t)f * p.nty + j;
    const uint8_t *recs = p.rec + (size_t)f * (p.ntx + p.nty - 1u) * kCropRecBytes;

    // ---- header and counts (row 0) ----
    if (j == 0u && tid < 32u) {
        if (tid < 20u) {
            ob[tid] = fb[tid];   // index and elapsed_ns bits as they are
        } else {
            const uint32_t k = tid - 20u, wd = k >> 2;
            const uint32_t n64 = (uint32_t)((p.frame_bytes[f] - 32ull - (PIX + 1ull) * p.Tout) >> 3);
            const uint32_t val = wd == 0u ? p.Tout : (wd == 1u ? PIX * p.Tout : n64);
            uint8_t *at = wd == 0u ? ob + 20 : (wd == 1u ? ob + 24 + (uint64_t)p.Tout : ob + 28 + (PIX + 1ull) * p.Tout);
            at[k & 3u] = (uint8_t)(val >> (8u * (k & 3u)));
        }
    }

    // ---- the row's depth bytes and minima ----
    const uint32_t pos0 = (cw.ty + j) * p.w + cw.tx;
    const bool row_cut = cw.cut_row && j == p.nty - 1u;
    const uint32_t ncut = row_cut ? p.ntx : (cw.cut_col ? 1u : 0u);   // the row's last ncut tiles are re-packed
    const uint32_t ncopy = p.ntx - ncut;
    const uint32_t opos0 = j * p.ntx;
    for (uint32_t i = tid; i < p.ntx; i += kCropThreads) {
        uint32_t d, mn;
        if (i < ncopy) {
            d = darr[pos0 + i];
            if constexpr (PIX == 1u) {
                mn = marr[pos0 + i];
            } else {
                const uint8_t *m = marr + 2u * (size_t)(pos0 + i);
                mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
            }
        } else {
            const uint8_t *rec = recs + (size_t)crop_slot(p, i, j) * kCropRecBytes;
            d = *reinterpret_cast<const uint32_t *>(rec + kCropRecDepth);
            mn = *reinterpret_cast<const uint32_t *>(rec + kCropRecMin);
        }
        odep[opos0 + i] = (uint8_t)d;
        omin[PIX * (size_t)(opos0 + i)] = (uint8_t)mn;
        if constexpr (PIX == 2u) omin[2u * (size_t)(opos0 + i) + 1u] = (uint8_t)(mn >> 8);
    }

    // ---- the copied payload range: aligned 16-byte blocks of the output, each from two aligned blocks of the source ----
    uint8_t *dst0 = opay + 8ull * p.row_words[r];
    {
        const uint8_t *src0 = pay + 8ull * p.row_src[r];
        const uint64_t nbytes = 8ull * p.row_copy[r];
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(dst0), g1 = g0 + nbytes, a0 = g0 & ~(uintptr_t)15;
        const uint32_t nblk = nbytes ? (uint32_t)((g1 - a0 + 15u) >> 4) : 0u;
        // source byte of output block 0's first byte; its distance to the 16-byte grid is the same for every block
        const uint8_t *s0 = src0 - (g0 - a0);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s0) & 15u), k0 = sh >> 2, bs = sh & 3u;
        const uint8_t *sa0 = s0 - sh;
        for (uint32_t i = tid; i < nblk; i += kCropThreads) {
            const uint8_t *q = sa0 + 16ull * i;
            const uint4 va = load16_inside(q, end);
            uint4 vb = make_uint4(0, 0, 0, 0);
            if (sh) vb = load16_inside(q + 16, end);
            // dwords k0 .. k0 + 4 of the eight, then the byte shift
            const uint32_t e0 = k0 == 0u ? va.x : (k0 == 1u ? va.y : (k0 == 2u ? va.z : va.w));
            const uint32_t e1 = k0 == 0u ? va.y : (k0 == 1u ? va.z : (k0 == 2u ? va.w : vb.x));
            const uint32_t e2 = k0 == 0u ? va.z : (k0 == 1u ? va.w : (k0 == 2u ? vb.x : vb.y));
            const uint32_t e3 = k0 == 0u ? va.w : (k0 == 1u ? vb.x : (k0 == 2u ? vb.y : vb.z));
            const uint32_t e4 = k0 == 0u ? vb.x : (k0 == 1u ? vb.y : (k0 == 2u ? vb.z : vb.w));
            u32x4_t o;
            o.x = __builtin_amdgcn_alignbyte(e1, e0, bs);
            o.y = __builtin_amdgcn_alignbyte(e2, e1, bs);
            o.z = __builtin_amdgcn_alignbyte(e3, e2, bs);
            o.w = __builtin_amdgcn_alignbyte(e4, e3, bs);
            const uintptr_t ba = a0 + 16ull * i;
            if (ba >= g0 && ba + 16u <= g1) {
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the frame is written once
            } else {   // the range's first / last block: the bytes inside it only
                const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) : 0u, hi = ba + 16u > g1 ? (uint32_t)(g1 - ba) : 16u;
                const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (uint32_t b = 0; b < 16u; b++)
                    if (b >= lo && b < hi) reinterpret_cast<uint8_t *>(ba)[b] = (uint8_t)(ow[b >> 2] >> (8u * (b & 3u)));
            }
        }
    }

    // ---- the re-packed tiles' payloads: one 8-byte word per thread and step ----
    constexpr uint32_t kWords = 8u * PIX;   // the most a tile has
    for (uint32_t k = tid; k < ncut * kWords; k += kCropThreads) {
        const uint32_t i = ncopy + k / kWords, wd = k % kWords;
        const uint8_t *rec = recs + (size_t)crop_slot(p, i, j) * kCropRecBytes;
        // a cut last tile follows the row's copied words; the tiles of a cut last row lie where the row scan put them
        const uint32_t at = row_cut ? *reinterpret_cast<const uint32_t *>(rec + kCropRecOff) : p.row_copy[r];
        if (wd < *reinterpret_cast<const uint32_t *>(rec + kCropRecDepth))
            store_u64_any(dst0 + 8ull * (at + wd), *reinterpret_cast<const uint64_t *>(rec + 8u * wd));
    }
}

hipError_t launch_crop(const CropParams &p, uint32_t pix, bool repack, hipStream_t s) {
    const uint32_t rows = p.n_frames * p.nty;   // (the host keeps both grids below 2^31)
    const uint32_t slots = p.n_frames * ((p.ntx + p.nty - 1u + kCropThreads - 1u) / kCropThreads);
    if (pix == 1u) {
        hipLaunchKernelGGL((crop_size_kernel<1>), dim3(rows), dim3(kCropThreads), 0, s, p);
        if (repack) hipLaunchKernelGGL((crop_repack_kernel<1>), dim3(slots), dim3(kCropThreads), 0, s, p);
        hipLaunchKernelGGL((crop_rows_kernel<1>), dim3(p.n_frames), dim3(kCropThreads), 0, s, p);
    } else {
        hipLaunchKernelGGL((crop_size_kernel<2>), dim3(rows), dim3(kCropThreads), 0, s, p);
        if (repack) hipLaunchKernelGGL((crop_repack_kernel<2>), dim3(slots), dim3(kCropThreads), 0, s, p);
        hipLaunchKernelGGL((crop_rows_kernel<2>), dim3(p.n_frames), dim3(kCropThreads), 0, s, p);
    }
    hipLaunchKernelGGL(crop_place_kernel, dim3(1), dim3(kCropPlaceThreads), 0, s, p);
    if (pix == 1u)
        hipLaunchKernelGGL((crop_copy_kernel<1>), dim3(rows), dim3(kCropThreads), 0, s, p);
    else
        hipLaunchKernelGGL((crop_copy_kernel<2>), dim3(rows), dim3(kCropThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
