// dbde_binned_kernels.hip -- binned decode for MI355X (gfx950, wave64): per frame, the sum / maximum / minimum of every
// b x b bin (b = 2, 4, 8) of the rw x rh window, straight from the compressed bytes (no image is written).
//
// binned_kernel<THREADS, PIX, B>: PIX = 1 for DBDE frames (U8 pixels, depth 0..8, payload at 32 + 2T; sums U16), PIX = 2
// for DBDE16 frames (U16 pixels, depth 0..16, payload at 32 + 3T; sums U32).  One workgroup per (frame, window tile row,
// piece of THREADS tiles), one tile per thread.  Steps 1 and 2 are decode_roi_kernel's (dbde_roi_kernels.hip): the
// tiles' depth / minimum bytes and one block scan for the payload offsets, then the piece's payload range into LDS as
// aligned 16-byte blocks.  Then
//   3. each thread cuts its tile's rows out of LDS one at a time (expand_row / add_bytes, cut_row16) and folds each row
//      into the accumulators of the current bin row, so a tile is never held whole: 8 / B bin rows of 8 / B bins per
//      statistic stay in registers.  The window starts at a multiple of B and B divides 8, so every bin lies inside one
//      tile.  Pixels right of or below the window are replaced by the identity (0 for sum and max, all ones for min)
//      before they are folded: a partial bin reduces only the window's pixels, never an edge tile's padding.  A depth-0
//      tile is not cut: its bins are pixels * min, min, min.
//   4. once every tile of the piece is cut, the payload buffer becomes a band of 8 / B output rows per plane; each
//      output row of the piece leaves as one contiguous run: aligned 16-byte stores, single elements only at the run's
//      two ends.
// The statistics are chosen at run time (a plane pointer is NULL or not: uniform branches); B, PIX and THREADS are
// template parameters.  Latency is hidden by occupancy, as in decode_roi_kernel.
#include "dbde_binned_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

constexpr uint32_t kEven = 0x00FF00FFu;   // the even bytes of a dword, one per 16-bit lane

__device__ __forceinline__ uint32_t sad(uint32_t a, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, 0u, acc); }   // acc + the four bytes of a
__device__ __forceinline__ uint32_t lo16(uint32_t a) { return a & 0xFFFFu; }
__device__ __forceinline__ uint32_t hmax16(uint32_t a) { return max(lo16(a), a >> 16); }   // over the two 16-bit lanes
__device__ __forceinline__ uint32_t hmin16(uint32_t a) { return min(lo16(a), a >> 16); }
// four bytes out of four 16-bit lanes that hold one each: a's lanes, then b's
__device__ __forceinline__ uint32_t pack_lanes8(uint32_t a, uint32_t b) {
    return (a & 0xFFu) | ((a >> 8) & 0xFF00u) | ((b & 0xFFu) << 16) | ((b << 8) & 0xFF000000u);
}

// Element j (NB bytes wide) of a row of packed elements held in dwords that start as zero.
template <uint32_t NB>
__device__ __forceinline__ void set_elem(uint32_t *v, uint32_t j, uint32_t val) {
    v[(j * NB) >> 2] |= val << (8u * ((j * NB) & 3u));
}

// NB bytes (1, 2, 4, 8 or 16: the packed elements of one thread's part of a band row) to the LDS byte address a.
template <uint32_t NB>
__device__ __forceinline__ void put_lds(uint32_t *s32, uint32_t a, const uint32_t *v) {
    uint8_t *q = reinterpret_cast<uint8_t *>(s32) + a;
    if constexpr (NB == 1u) *q = (uint8_t)v[0];
    else if constexpr (NB == 2u) *reinterpret_cast<uint16_t *>(q) = (uint16_t)v[0];
    else if constexpr (NB == 4u) *reinterpret_cast<uint32_t *>(q) = v[0];
    else if constexpr (NB == 8u) *reinterpret_cast<uint2 *>(q) = make_uint2(v[0], v[1]);
    else *reinterpret_cast<uint4 *>(q) = make_uint4(v[0], v[1], v[2], v[3]);
}

// nrows runs of len elements (ES bytes each) from the band to the plane: run i starts at LDS byte src + i * pitch and
// at dst + i * stride (ES-aligned).  Whole 16-byte blocks of a run leave as aligned nontemporal stores, the elements in
// front of the first and behind the last one by one.  The dword behind the band's last is inside the LDS array.
template <uint32_t THREADS, uint32_t ES>
__device__ __forceinline__ void store_runs(const uint32_t *s32, uint32_t src, uint32_t pitch, uint8_t *dst, size_t stride,
                                           uint32_t nrows, uint32_t len, uint32_t tid) {
    typedef typename std::conditional<ES == 1u, uint8_t, typename std::conditional<ES == 2u, uint16_t, uint32_t>::type>::type Elem;
    const uint32_t nbmax = (ES * len + 30u) >> 4;   // the blocks a run touches at its worst alignment
    for (uint32_t it = tid; it < nrows * nbmax; it += THREADS) {
        const uint32_t row = it / nbmax, i = it - row * nbmax;
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(dst + (size_t)row * stride), g1 = g0 + ES * len;
        const uintptr_t ba = (g0 & ~(uintptr_t)15) + 16u * i;
        if (ba >= g1) continue;
        const uint32_t lo = ba < g0 ? (uint32_t)(g0 - ba) : 0u;           // bytes of the block inside the run
        const uint32_t hi = ba + 16u > g1 ? (uint32_t)(g1 - ba) : 16u;
        const uint32_t a = src + row * pitch + (uint32_t)(ba + lo - g0);  // LDS byte of the block's first element
        if (lo == 0u && hi == 16u) {
            u32x4_t o;
            o.x = lds_u32_at(s32, a); o.y = lds_u32_at(s32, a + 4u); o.z = lds_u32_at(s32, a + 8u); o.w = lds_u32_at(s32, a + 12u);
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(ba));   // the plane is written once
        } else {
            const Elem *e = reinterpret_cast<const Elem *>(reinterpret_cast<const uint8_t *>(s32) + a);
            for (uint32_t b = lo; b < hi; b += ES) *reinterpret_cast<Elem *>(ba + b) = *e++;
        }
    }
}

}  // namespace

template <uint32_t THREADS, uint32_t PIX, uint32_t B>
__global__ __launch_bounds__(THREADS) void binned_kernel(BinnedParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(B == 2u || B == 4u || B == 8u, "bins of 2, 4 or 8 pixels a side");
    constexpr uint32_t NW = THREADS / 64u;
    constexpr uint32_t NO = 8u / B;                      // bins across and down one tile
    constexpr uint32_t ES = 2u * PIX, EM = PIX;          // bytes of a sum / of a maximum or minimum
    constexpr uint32_t RS = NO * ES, RM = NO * EM;       // bytes of one tile's part of a band row
    constexpr uint32_t WS = RS >= 4u ? RS / 4u : 1u, WM = RM >= 4u ? RM / 4u : 1u;   // ... in dwords
    // the band: NO rows of THREADS * NO elements per plane, the sums in front; it reuses the payload buffer
    constexpr uint32_t kBandSum = 0u, kBandMax = THREADS * NO * RS, kBandMin = kBandMax + THREADS * NO * RM;
    constexpr uint32_t kPayBytes = kBinPayBytesOf(THREADS, PIX);
    static_assert(kBandMin + THREADS * NO * RM + 4u <= kPayBytes, "the band must fit the payload buffer");
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];
    __shared__ uint32_t s_wsum[2][NW];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per_frame = p.rows * p.pieces;
    const uint32_t f = blockIdx.x / per_frame;
    const uint32_t rem = blockIdx.x - f * per_frame;
    const uint32_t br = rem / p.pieces, pc = rem - br * p.pieces;
    if (!p.frame_ok[f]) return;   // rejected frame: its planes stay untouched

    const int x_end = p.x0 + p.rw, y_end = p.y0 + p.rh;
    const uint32_t tx_b = (uint32_t)(x_end - 1) >> 3;
    const uint32_t ty = p.ty0 + br, txp = p.tx0 + pc * THREADS;
    const uint32_t nt = tx_b + 1u - txp < THREADS ? tx_b + 1u - txp : THREADS;
    const bool want_sum = p.out_sum != nullptr, want_max = p.out_max != nullptr, want_min = p.out_min != nullptr;

    // ---- 1. depth / minimum bytes, offsets (decode_roi_kernel's step 1) ----
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
    const uint32_t incl = wave_scan_incl(d);
    const uint32_t pre_w = wave_sum(pre);
    if (lane == 63u) s_wsum[0][wave] = incl;
    if (lane == 0u) s_wsum[1][wave] = pre_w;
    __syncthreads();
    uint32_t wbase = 0, S = 0, PRE = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const uint32_t v = s_wsum[0][k];
        wbase += k < wave ? v : 0u;
        S += v;
        PRE += s_wsum[1][k];
    }
    const uint32_t woff = wbase + incl - d;   // payload words in front of this tile inside the piece

    // ---- 2. the piece's payload into LDS (decode_roi_kernel's step 2; nothing to fetch for a piece of depth-0 tiles) ----
    const uint8_t *src0 = pay + 8ull * ((uint64_t)base + PRE);
    const uint8_t *a_lo = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(src0) & ~(uintptr_t)15);
    const uint32_t sh = (uint32_t)(src0 - a_lo);
    const uint32_t nblk = S ? (sh + 8u * S + 15u) >> 4 : 0u;   // <= 4 * PIX * THREADS + 1
    const uint8_t *end = p.stream + p.stream_bytes;
    for (uint32_t i = tid; i < nblk; i += THREADS) {
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

    // ---- 3. tile rows -> bins, in registers ----
    // the tile's pixels inside the window: columns [0, cx), rows [0, cy) (the window starts at a bin edge, so what lies
    // left of or above it falls into bins that are not stored)
    const int px0 = 8 * (int)txp;   // first pixel column of the piece
    const uint32_t cx = (uint32_t)min(8, x_end - (px0 + 8 * (int)tid));   // >= 1 for tid < nt
    const uint32_t cy = (uint32_t)min(8, y_end - 8 * (int)ty);            // >= 1, the same for the whole workgroup
    uint32_t rs[NO][WS], rx[NO][WM], rn[NO][WM];
#pragma unroll
    for (uint32_t i = 0; i < NO; i++) {
#pragma unroll
        for (uint32_t k = 0; k < WS; k++) rs[i][k] = 0u;
#pragma unroll
        for (uint32_t k = 0; k < WM; k++) { rx[i][k] = 0u; rn[i][k] = 0u; }
    }
    if (tid < nt && d == 0u) {
        // flat tile: no cut.  Bin (i, j) holds ny * nx window pixels, all equal to the minimum.
#pragma unroll
        for (uint32_t i = 0; i < NO; i++) {
            const uint32_t ny = cy > i * B ? min(B, cy - i * B) : 0u;
#pragma unroll
            for (uint32_t j = 0; j < NO; j++) {
                const uint32_t nx = cx > j * B ? min(B, cx - j * B) : 0u;
                set_elem<ES>(rs[i], j, mn * nx * ny);
                set_elem<EM>(rx[i], j, mn);
                set_elem<EM>(rn[i], j, mn);
            }
        }
    } else if (tid < nt) {
        if constexpr (PIX == 1u) {
            // Bytes.  Sums: B = 2 adds the even and the odd bytes of a dword as two 16-bit lanes (a pair sum per lane,
            // at most 4 * 255 after two rows); B = 4, 8 take a dword's byte sum with v_sad_u8 against zero.  Maxima /
            // minima: v_pk_max_u16 / v_pk_min_u16 on the even bytes (masked into the lanes) and on the dword itself,
            // whose lanes are decided by their high bytes, so the result's high bytes are the odd bytes' (tile_minmax's
            // trick); the two meet once per bin row.
            const uint64_t keep = cx >= 8u ? ~0ull : (1ull << (8u * cx)) - 1ull;   // the bytes of a row inside the window
            const uint32_t kl = (uint32_t)keep, kh = (uint32_t)(keep >> 32);
            const uint32_t mm = mn * 0x01010101u;
            uint32_t sl = 0, sh_ = 0, xel = 0, xol = 0, xeh = 0, xoh = 0, nel = kEven, nol = ~0u, neh = kEven, noh = ~0u;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                if (r < cy) {
                    const uint32_t o = sh + 8u * woff + r * d;   // byte of tile row r (8d bits)
                    const uint32_t w0 = o >> 2, s = o & 3u;
                    const uint32_t a0 = s_pay[w0], a1 = s_pay[w0 + 1u], a2 = s_pay[w0 + 2u];
                    const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(a1, a0, s) |
                                          ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, s) << 32);
                    uint32_t lo, hi;
                    expand_row(bits, d, lo, hi);
                    lo = add_bytes(lo, mm);
                    hi = add_bytes(hi, mm);
                    const uint32_t al = lo & kl, ah = hi & kh;   // outside the window: 0
                    if (want_sum) {
                        if constexpr (B == 2u) {
                            sl += (al & kEven) + ((al >> 8) & kEven);
                            sh_ += (ah & kEven) + ((ah >> 8) & kEven);
                        } else {
                            sl = sad(al, sl);
                            sh_ = sad(ah, sh_);
                        }
                    }
                    if (want_max) {
                        xel = pk_max_u16(xel, al & kEven); xol = pk_max_u16(xol, al);
                        xeh = pk_max_u16(xeh, ah & kEven); xoh = pk_max_u16(xoh, ah);
                    }
                    if (want_min) {
                        const uint32_t ol = lo | ~kl, oh = hi | ~kh;   // outside the window: 255
                        nel = pk_min_u16(nel, ol & kEven); nol = pk_min_u16(nol, ol);
                        neh = pk_min_u16(neh, oh & kEven); noh = pk_min_u16(noh, oh);
                    }
                }
                if ((r + 1u) % B == 0u) {   // a bin row is complete (or lies below the window: identities, never stored)
                    const uint32_t i = r / B;
                    // per 16-bit lane: pixels 0-1, 2-3 (l) and 4-5, 6-7 (h) of the bin row
                    const uint32_t xl = pk_max_u16(xel, (xol >> 8) & kEven), xh = pk_max_u16(xeh, (xoh >> 8) & kEven);
                    const uint32_t nl = pk_min_u16(nel, (nol >> 8) & kEven), nh = pk_min_u16(neh, (noh >> 8) & kEven);
                    if constexpr (B == 2u) {
                        rs[i][0] = sl; rs[i][1] = sh_;
                        rx[i][0] = pack_lanes8(xl, xh);
                        rn[i][0] = pack_lanes8(nl, nh);
                    } else if constexpr (B == 4u) {
                        rs[i][0] = sl | (sh_ << 16);
                        rx[i][0] = hmax16(xl) | (hmax16(xh) << 8);
                        rn[i][0] = hmin16(nl) | (hmin16(nh) << 8);
                    } else {
                        rs[i][0] = sl + sh_;
                        rx[i][0] = hmax16(pk_max_u16(xl, xh));
                        rn[i][0] = hmin16(pk_min_u16(nl, nh));
                    }
                    sl = 0; sh_ = 0; xel = 0; xol = 0; xeh = 0; xoh = 0; nel = kEven; nol = ~0u; neh = kEven; noh = ~0u;
                }
            }
        } else {
            // U16 pixels, two per dword.  Sums: low + high half of each dword in U32 (at most 2 * 8 * 65535 per dword
            // and bin row).  Maxima / minima: v_pk_max_u16 / v_pk_min_u16 down the rows, the two lanes meet once per
            // bin row.
            uint32_t km[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) km[k] = cx >= 2u * k + 2u ? ~0u : (cx == 2u * k + 1u ? 0xFFFFu : 0u);
            const uint32_t byte0 = sh + 8u * woff;
            const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = mn * 0x00010001u;
            uint32_t sm[4] = {0, 0, 0, 0}, xm[4] = {0, 0, 0, 0}, nm[4] = {~0u, ~0u, ~0u, ~0u};
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                if (r < cy) {
                    const uint32_t a = byte0 + r * d, ah = a + (d >> 1);   // the row's two 4-pixel halves
                    uint32_t v[4];
                    cut_row16(s_pay + (a >> 2), s_pay + (ah >> 2), a, ah, d, m32, mn2, v[0], v[1], v[2], v[3]);
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t ak = v[k] & km[k];   // outside the window: 0
                        if (want_sum) sm[k] += lo16(ak) + (ak >> 16);
                        if (want_max) xm[k] = pk_max_u16(xm[k], ak);
                        if (want_min) nm[k] = pk_min_u16(nm[k], v[k] | ~km[k]);   // outside the window: 65535
                    }
                }
                if ((r + 1u) % B == 0u) {
                    const uint32_t i = r / B;
                    if constexpr (B == 2u) {
#pragma unroll
                        for (uint32_t k = 0; k < 4u; k++) rs[i][k] = sm[k];
                        rx[i][0] = hmax16(xm[0]) | (hmax16(xm[1]) << 16); rx[i][1] = hmax16(xm[2]) | (hmax16(xm[3]) << 16);
                        rn[i][0] = hmin16(nm[0]) | (hmin16(nm[1]) << 16); rn[i][1] = hmin16(nm[2]) | (hmin16(nm[3]) << 16);
                    } else if constexpr (B == 4u) {
                        rs[i][0] = sm[0] + sm[1]; rs[i][1] = sm[2] + sm[3];
                        rx[i][0] = hmax16(pk_max_u16(xm[0], xm[1])) | (hmax16(pk_max_u16(xm[2], xm[3])) << 16);
                        rn[i][0] = hmin16(pk_min_u16(nm[0], nm[1])) | (hmin16(pk_min_u16(nm[2], nm[3])) << 16);
                    } else {
                        rs[i][0] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
                        rx[i][0] = hmax16(pk_max_u16(pk_max_u16(xm[0], xm[1]), pk_max_u16(xm[2], xm[3])));
                        rn[i][0] = hmin16(pk_min_u16(pk_min_u16(nm[0], nm[1]), pk_min_u16(nm[2], nm[3])));
                    }
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) { sm[k] = 0u; xm[k] = 0u; nm[k] = ~0u; }
                }
            }
        }
    }
    __syncthreads();   // every tile cut: the payload buffer becomes the band
    if (tid < nt) {
#pragma unroll
        for (uint32_t i = 0; i < NO; i++) {
            if (want_sum) put_lds<RS>(s_pay, kBandSum + (i * THREADS + tid) * RS, rs[i]);
            if (want_max) put_lds<RM>(s_pay, kBandMax + (i * THREADS + tid) * RM, rx[i]);
            if (want_min) put_lds<RM>(s_pay, kBandMin + (i * THREADS + tid) * RM, rn[i]);
        }
    }
    __syncthreads();

    // ---- 4. the window's part of the band -> the planes (in bins) ----
    const int c_lo = px0 > p.x0 ? px0 : p.x0;                                   // pixel columns / rows of the piece inside the window
    const int c_hi = px0 + 8 * (int)nt < x_end ? px0 + 8 * (int)nt : x_end;
    const int r_lo = 8 * (int)ty > p.y0 ? 8 * (int)ty : p.y0;
    const int r_hi = 8 * (int)ty + 8 < y_end ? 8 * (int)ty + 8 : y_end;
    const uint32_t len = ((uint32_t)(c_hi - c_lo) + B - 1u) / B, nrows = ((uint32_t)(r_hi - r_lo) + B - 1u) / B;
    const uint32_t bx = (uint32_t)(c_lo - px0) / B, by = (uint32_t)(r_lo - 8 * (int)ty) / B;   // first bin of the band stored
    const size_t first = ((size_t)f * p.oh + (size_t)(r_lo - p.y0) / B) * p.ow + (size_t)(c_lo - p.x0) / B;   // ... and where it goes
    if (want_sum)
        store_runs<THREADS, ES>(s_pay, kBandSum + (by * THREADS * NO + bx) * ES, THREADS * RS,
                                static_cast<uint8_t *>(p.out_sum) + first * ES, (size_t)p.ow * ES, nrows, len, tid);
    if (want_max)
        store_runs<THREADS, EM>(s_pay, kBandMax + (by * THREADS * NO + bx) * EM, THREADS * RM,
                                static_cast<uint8_t *>(p.out_max) + first * EM, (size_t)p.ow * EM, nrows, len, tid);
    if (want_min)
        store_runs<THREADS, EM>(s_pay, kBandMin + (by * THREADS * NO + bx) * EM, THREADS * RM,
                                static_cast<uint8_t *>(p.out_min) + first * EM, (size_t)p.ow * EM, nrows, len, tid);
}

namespace {

template <uint32_t THREADS, uint32_t PIX>
hipError_t launch_bin(const BinnedParams &p, uint32_t grid, uint32_t bin, hipStream_t s) {
    if (bin == 2u) hipLaunchKernelGGL((binned_kernel<THREADS, PIX, 2>), dim3(grid), dim3(THREADS), 0, s, p);
    else if (bin == 4u) hipLaunchKernelGGL((binned_kernel<THREADS, PIX, 4>), dim3(grid), dim3(THREADS), 0, s, p);
    else hipLaunchKernelGGL((binned_kernel<THREADS, PIX, 8>), dim3(grid), dim3(THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_decode_binned(const BinnedParams &p, uint32_t n_frames, uint32_t threads, uint32_t pix, uint32_t bin,
                                hipStream_t s) {
    if ((pix != 1u && pix != 2u) || (bin != 2u && bin != 4u && bin != 8u) ||
        (threads != kBinNarrowThreads && threads != kBinWideThreadsOf(pix)))
        return hipErrorInvalidValue;
    const uint32_t grid = n_frames * p.rows * p.pieces;   // (the host keeps it below 2^31)
    if (pix == 1u)
        return threads == kBinNarrowThreads ? launch_bin<kBinNarrowThreads, 1>(p, grid, bin, s)
                                            : launch_bin<kBinWideThreadsOf(1), 1>(p, grid, bin, s);
    return threads == kBinNarrowThreads ? launch_bin<kBinNarrowThreads, 2>(p, grid, bin, s)
                                        : launch_bin<kBinWideThreadsOf(2), 2>(p, grid, bin, s);
}

}  // namespace dbde
