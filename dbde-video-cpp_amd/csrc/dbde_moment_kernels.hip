// dbde_moment_kernels.hip -- patch moments for MI355X (gfx950, wave64): for each of K small windows of one size per
// frame, the thresholded image moments up to second order and the selected pixels' bounding box, straight from the
// compressed bytes (no pixel is written).
//
// The index pass (decode_index_kernel on roi_index_geometry's chunks) gives a payload offset at the start of every tile
// row, so it runs once per call however many patches there are; patch_moments_kernel<PIX> then visits only the patches'
// tiles.
//
// patch_moments_kernel<PIX>: PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  One 64-lane workgroup per (frame,
// patch), one tile per lane: with mtx the most tiles a patch spans across, lane l takes tile (l / mtx, l % mtx) of a
// group of G = max(1, 64 / mtx) tile rows, and the workgroup walks the patch's groups in a loop, keeping the eight sums
// and the box in registers; a patch's entry leaves once, by plain stores of one lane, so a rejected frame's and a dead
// patch's entries stay untouched and nothing is zeroed beforehand.  Steps 1-3 are decode_patches_kernel's
// (dbde_patch_kernels.hip), repeated here so that the patch decoder's listing stays as it is, with the header shortcuts
// of decode_mask_kernel (dbde_mask_kernels.hip) in front:
//   0. the tiles' depth / minimum bytes.  A tile of depth d and minimum m whose range [m, m + 2^d - 1] does not wrap
//      past the pixel maximum and lies wholly outside [lo, hi] selects no pixel: it is SKIPPED, as is every tile when
//      lo > hi.  A tile row all of whose tiles are skipped or flat (depth 0) reads no prefix byte and no payload;
//   1. per tile row that needs payload, the fewer than 512 depth bytes between its chunk's start and its first tile,
//      read by the row's mtx lanes as aligned dwords with masked ends and summed with v_sad_u8; one wave scan, segmented
//      per row, of (prefix bytes << 16 | depth) gives the row's payload start and every tile's word offset in its row;
//   2. such a row's payload range, fetched by the row's lanes as 16-byte non-temporal blocks from the aligned address
//      in front of it into the row's part of LDS (the block that would cross stream_bytes byte by byte);
//   3. each lane cuts its tile's rows out of LDS (dbde_bits.h's expand_row / add_bytes, dbde_device.h's cut_row16) and
//      reduces each as it is cut: per tile row the sums of w, w c and w c^2 over its columns c = 0..7 and a byte of
//      selection bits, over the 8 rows r the six tile-local U32 sums (at most 64 * 65535 * 49).  Pixels outside the
//      patch or outside the frame (the encoder's padding included) have weight 0.  A flat tile is 64 copies of m: its
//      sums over the rectangle of live pixels have a closed form and nothing is cut;
//   4. the tile-local sums are shifted to patch coordinates in 64 bits with the tile's signed offset (dx, dy) =
//      (8 tx - x, 8 ty - y) (the binomial shift: Sxx = scc + 2 dx sc + dx^2 s, ...; dx >= -7) and added to the lane's
//      eight U64 sums.
// After the loop one DPP reduction (row shifts and row broadcasts, no LDS) leaves the wave's sums, and the box as
// packed U16 minima / maxima, in lane 63, which stores them.  All arithmetic is integer: the result is exact and does
// not depend on the geometry.  Latency is hidden by occupancy, as in the window decoder.
#include "dbde_moment_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

// Both are sized by the listing: at 8 prefix dwords or 4 tile rows in flight the U8 instance spills to scratch at the 72
// registers that 7 waves per SIMD leave it.
constexpr uint32_t kPrefixBatch = 4;   // prefix dwords a lane has in flight at once
constexpr uint32_t kRowUnroll = 2;     // tile rows in flight in a lane

// One step of a wave reduction by DPP: the value of the lane the control word names, `ident` where there is none.
#define DBDE_DPP_FROM(ident, v, ctrl, rows) \
    ((uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)(v), (ctrl), (rows), 0xF, false))

// Sum over the wave, in lane 63 (wave_scan_incl's steps on both halves of a U64).
__device__ __forceinline__ uint64_t wave_total_u64(uint64_t v) {
#define DBDE_STEP(ctrl, rows)                                                          \
    {                                                                                  \
        const uint32_t l = DBDE_DPP_FROM(0u, (uint32_t)v, ctrl, rows);                 \
        const uint32_t h = DBDE_DPP_FROM(0u, (uint32_t)(v >> 32), ctrl, rows);         \
        v += ((uint64_t)h << 32) | l;                                                  \
    }
    DBDE_STEP(0x111, 0xF)   // row_shr:1
    DBDE_STEP(0x112, 0xF)   // row_shr:2
    DBDE_STEP(0x114, 0xF)   // row_shr:4
    DBDE_STEP(0x118, 0xF)   // row_shr:8
    DBDE_STEP(0x142, 0xA)   // row_bcast:15 -> rows 1,3
    DBDE_STEP(0x143, 0xC)   // row_bcast:31 -> rows 2,3
#undef DBDE_STEP
    return v;
}

// Minimum (MAX: maximum) of both U16 halves over the wave, in lane 63.
template <bool MAX>
__device__ __forceinline__ uint32_t wave_total_pk_u16(uint32_t v) {
    constexpr uint32_t ident = MAX ? 0u : 0xFFFFFFFFu;
#define DBDE_STEP(ctrl, rows)                                           \
    {                                                                   \
        const uint32_t t = DBDE_DPP_FROM(ident, v, ctrl, rows);         \
        v = MAX ? pk_max_u16(v, t) : pk_min_u16(v, t);                  \
    }
    DBDE_STEP(0x111, 0xF)
    DBDE_STEP(0x112, 0xF)
    DBDE_STEP(0x114, 0xF)
    DBDE_STEP(0x118, 0xF)
    DBDE_STEP(0x142, 0xA)
    DBDE_STEP(0x143, 0xC)
#undef DBDE_STEP
    return v;
}

// Sum of c and of c^2 over c in [a, b), 0 <= a <= b <= 8.
__device__ __forceinline__ void span_sums(uint32_t a, uint32_t b, uint32_t &s1, uint32_t &s2) {
    s1 = (b * (b - 1u) - a * (a - 1u)) >> 1;
    s2 = ((b - 1u) * b * (2u * b - 1u) - (a - 1u) * a * (2u * a - 1u)) / 6u;   // (a = 0: the term is 0 * ...)
}

}  // namespace

// (The second launch bound is waves per SIMD, set to what the LDS admits: 160 KiB / 6 KiB / 4 SIMDs = 6.5, 160 / 10 / 4 = 4.)
template <uint32_t PIX>
__global__ __launch_bounds__(kMomentThreads, PIX == 1u ? 7 : 4) void patch_moments_kernel(MomentParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type Sq;   // a tile's sum of w^2
    constexpr uint32_t kPayBytes = kMomentPayBytesOf(PIX), kPixMax = PIX == 1u ? 0xFFu : 0xFFFFu;
    __shared__ __attribute__((aligned(16))) uint32_t s_pay[kPayBytes / 4u];   // the rows' payload ranges
    static_assert(kMomentThreads * 64u * PIX + 32u * kMomentThreads <= kPayBytes, "G <= 64 row ranges must fit");

    const uint32_t lane = threadIdx.x;
    const uint32_t b = p.block0 + blockIdx.x;
    const uint32_t k = b % p.n_patches, f = b / p.n_patches;
    if (!p.frame_ok[f]) return;   // rejected frame: its entries stay untouched
    if (p.counts) {
        const uint32_t cnt = p.counts[f];
        if (k >= (cnt < p.n_patches ? cnt : p.n_patches)) return;   // not a live patch: untouched
    }
    const size_t pi = (size_t)f * p.n_patches + k;
    const int ox = p.origins[2u * pi], oy = p.origins[2u * pi + 1u];
    const bool fill_mode = p.mode == kMomentFill;
    int x, y;
    if (!fill_mode) {   // the window decoder's rule
        x = ox < 0 ? 0 : (ox > p.W - p.pw ? p.W - p.pw : ox);
        y = oy < 0 ? 0 : (oy > p.H - p.ph ? p.H - p.ph : oy);
    } else {   // any origin at or beyond these bounds gives the same patch: no pixel inside the frame
        x = ox < -p.pw ? -p.pw : (ox > p.W ? p.W : ox);
        y = oy < -p.ph ? -p.ph : (oy > p.H ? p.H : oy);
    }
    if (p.used && lane == 0u) {
        p.used[2u * pi] = fill_mode ? ox : x;
        p.used[2u * pi + 1u] = fill_mode ? oy : y;
    }
    // tile coordinates are signed (a fill-mode patch can start left of or above the frame).  32 bits are enough: the
    // index takes at most 32768 chunks of 512 tiles, so W, H <= 2^27, and pw, ph <= 512
    const int x_end = x + p.pw, y_end = y + p.ph;
    const int tx_a = x >> 3, tx_b = (x_end - 1) >> 3;
    const int ty_a = y >> 3, ty_b = (y_end - 1) >> 3;
    // the patch's pixels inside the frame, in frame coordinates
    const int fx0 = x > 0 ? x : 0, fx1 = x_end < p.W ? x_end : p.W;
    const int fy0 = y > 0 ? y : 0, fy1 = y_end < p.H ? y_end : p.H;

    const uint32_t mtx0 = p.mtx;
    const uint32_t lr0 = lane / mtx0, lc0 = lane - lr0 * mtx0;
    const int txs = tx_a < 0 ? 0 : tx_a, txe = tx_b > (int)p.w - 1 ? (int)p.w - 1 : tx_b;

    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;

    // the weight of a selected pixel v: sa v + sb
    const uint32_t lo = p.lo, hi = p.hi, span = hi - lo;
    const bool none = lo > hi;
    const int sa = p.weight == kMomentCount ? 0 : (p.weight == kMomentBelow ? -1 : 1);
    const int sb = p.weight == kMomentCount ? 1 : (p.weight == kMomentAbove ? -(int)lo : (p.weight == kMomentBelow ? (int)hi : 0));

    uint32_t aN = 0;
    uint64_t aS = 0, aSx = 0, aSy = 0, aSxx = 0, aSxy = 0, aSyy = 0;
    uint64_t aSww = 0;
    uint32_t bmin = ((uint32_t)p.pw << 16) | (uint32_t)p.ph;   // (j_min, i_min), 16 bits each: at most 505 and 512
    uint32_t bmax = 0u;                                        // (j_max + 1, i_max + 1)

    for (uint32_t grp = 0; grp < p.steps; grp++) {
        // Nothing below is carried from one group to the next but the sums: the lane's place is taken afresh (an empty
        // statement the compiler cannot see through), or everything that depends on it alone would be computed once in
        // front of the loop and held in registers across it, which costs the occupancy the LDS allows.
        uint32_t mtx = mtx0, lr = lr0, lc = lc0;
        asm volatile("" : "+s"(mtx), "+v"(lr), "+v"(lc));
        const int tx = tx_a + (int)lc;
        const uint64_t row_lanes = lr < p.G ? (mtx >= 64u ? ~0ull : ((1ull << mtx) - 1ull) << (lr * mtx)) : 0ull;
        uint32_t *s_row = s_pay + lr * (kMomentRowBytesOf(mtx, PIX) >> 2);   // (lanes of no row never use it)
        const int tyg = ty_a + (int)(grp * p.G);   // first tile row of the group
        if (tyg > ty_b) break;                     // the steps cover the most any origin needs
        const int ty = tyg + (int)lr;
        const bool row_live = lr < p.G && ty <= ty_b;
        const bool row_has = row_live && ty >= 0 && ty < (int)p.h && txs <= txe;   // the row has tiles inside the frame
        const bool valid = row_has && tx >= txs && tx <= txe;

        // ---- 0. depth / minimum bytes, the skipped tiles ----
        uint32_t d = 0, mn = 0;
        if (valid) {
            const uint32_t pos = (uint32_t)ty * p.w + (uint32_t)tx;
            d = darr[pos];
            if constexpr (PIX == 1u) {
                mn = marr[pos];
            } else {   // the U16 minima start at 28 + T, possibly at an odd address: byte by byte
                const uint8_t *m = marr + 2u * pos;
                mn = (uint32_t)m[0] | ((uint32_t)m[1] << 8);
            }
        }
        d = d > 8u * PIX ? 8u * PIX : d;   // (a validated frame has none)
        // the tile's live pixels: columns [c0, c1) and rows [r0, r1) of it lie inside the patch and the frame (an edge
        // tile's padding beyond W or H does not: such a tile can overlap the patch and still hold no live pixel)
        const int X0 = 8 * tx, Y0 = 8 * ty;
        const int ic0 = fx0 > X0 ? fx0 - X0 : 0, ic1 = fx1 - X0 < 8 ? fx1 - X0 : 8;
        const int ir0 = fy0 > Y0 ? fy0 - Y0 : 0, ir1 = fy1 - Y0 < 8 ? fy1 - Y0 : 8;
        bool live = valid && !none && ic0 < ic1 && ir0 < ir1;
        if (live) {
            const uint32_t top = mn + (1u << d) - 1u;   // the tile's values lie in [mn, top] when top does not wrap
            if (top <= kPixMax && (top < lo || mn > hi)) live = false;
        }
        const uint64_t need = __ballot(live && d != 0u);   // the tiles that are cut
        const bool row_need = (need & row_lanes) != 0ull;

        uint32_t woff = 0, sh = 0;
        if (need) {   // (wave-uniform)
            // ---- 1. offsets ----
            uint32_t base = 0, pre = 0;
            if (row_need) {
                const uint32_t pos0 = (uint32_t)ty * p.w + (uint32_t)txs;
                const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
                base = p.chunk_off[(size_t)f * (p.geom.cpf + 1u) + c];
                const uint32_t npre = pos0 - cb;   // < 512 (roi_index_geometry)
                if (npre) {
                    // bytes [s, e) of the dwords at a0: the dwords lie inside the frame (24 header bytes in front, the
                    // row's own depth bytes and the minima behind)
                    const uintptr_t pa = reinterpret_cast<uintptr_t>(darr + cb);
                    const uint32_t *a0 = reinterpret_cast<const uint32_t *>(pa & ~(uintptr_t)3);
                    const uint32_t s = (uint32_t)(pa & 3u), e = s + npre, nd = (e + 3u) >> 2;   // nd <= 129
                    for (uint32_t i0 = lc; i0 < nd; i0 += kPrefixBatch * mtx) {
                        uint32_t v[kPrefixBatch];
#pragma unroll
                        for (uint32_t j = 0; j < kPrefixBatch; j++) {   // (a clamped index keeps the loads unconditional)
                            const uint32_t i = i0 + j * mtx;
                            v[j] = a0[i < nd ? i : nd - 1u];
                        }
#pragma unroll
                        for (uint32_t j = 0; j < kPrefixBatch; j++) {
                            const uint32_t i = i0 + j * mtx;
                            uint32_t m = i < nd ? 0xFFFFFFFFu : 0u;
                            if (4u * i < s) m &= 0xFFFFFFFFu << (8u * (s - 4u * i));
                            if (4u * i + 4u > e) m &= 4u * i < e ? 0xFFFFFFFFu >> (8u * (4u * i + 4u - e)) : 0u;
                            pre = __builtin_amdgcn_sad_u8(v[j] & m, 0u, pre);
                        }
                    }
                }
            }
            // one scan for both sums: a row's depths total at most 64 * 16, its prefix bytes 511 * 16
            uint32_t sc = d | (pre << 16);
            for (uint32_t o = 1; o < mtx; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)sc, o, 64);
                if (lc >= o) sc += t;
            }
            const uint32_t last = lr * mtx + mtx - 1u;
            const uint32_t tot = (uint32_t)__shfl((int)sc, (int)(last < 63u ? last : 63u), 64);
            const uint32_t S = tot & 0xFFFFu, PRE = tot >> 16;   // the row's payload words, and those in front of it
            woff = (sc & 0xFFFFu) - d;                           // payload words in front of this tile inside the row

            // ---- 2. the rows' payload ranges into LDS ----
            if (row_need) {
                const uint8_t *src0 = pay + 8ull * ((uint64_t)base + PRE);
                const uint8_t *a_lo = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(src0) & ~(uintptr_t)15);
                sh = (uint32_t)(src0 - a_lo);
                const uint32_t nblk = (sh + 8u * S + 15u) >> 4;   // <= 4 * PIX * mtx + 1: row_bytes less the over-read
                const uint8_t *end = p.stream + p.stream_bytes;
                for (uint32_t i = lc; i < nblk; i += mtx) {
                    const uint8_t *q = a_lo + 16u * i;
                    uint4 v;
                    if (q + 16 <= end) {
                        const u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(q));   // streamed once
                        v = make_uint4(t.x, t.y, t.z, t.w);
                    } else {   // the block that crosses the readable extent: only the bytes in front of it
                        uint32_t wq[4] = {0, 0, 0, 0};
                        for (uint32_t bb = 0; bb < 16u; bb++)
                            if (q + bb < end) wq[bb >> 2] |= (uint32_t)q[bb] << (8u * (bb & 3u));
                        v = make_uint4(wq[0], wq[1], wq[2], wq[3]);
                    }
                    *reinterpret_cast<uint4 *>(s_row + 4u * i) = v;
                }
            }
        }
        __syncthreads();

        // ---- 3. tile rows -> registers -> the tile's sums ----
        if (live) {
            const uint32_t c0 = (uint32_t)ic0, c1 = (uint32_t)ic1, r0 = (uint32_t)ir0, r1 = (uint32_t)ir1;   // 0 .. 8
            uint32_t n, s = 0, s_c = 0, s_r = 0, s_cc = 0, s_rc = 0, s_rr = 0;   // tile-local sums
            uint32_t cmin, cmax, rmin, rmax;
            Sq ww = 0;   // 64 * 255^2 fits 32 bits, 64 * 65535^2 does not
            if (d == 0u) {   // flat, and not skipped: every live pixel is selected with the weight of mn
                const uint32_t wv = (uint32_t)((int)mn * sa + sb), nc = c1 - c0, nr = r1 - r0;
                uint32_t c_1, c_2, r_1, r_2;
                span_sums(c0, c1, c_1, c_2);
                span_sums(r0, r1, r_1, r_2);
                n = nc * nr;
                s = wv * n;
                s_c = wv * nr * c_1;
                s_r = wv * nc * r_1;
                s_cc = wv * nr * c_2;
                s_rr = wv * nc * r_2;
                s_rc = wv * c_1 * r_1;
                ww = (Sq)((Sq)wv * wv * n);
                cmin = c0; cmax = c1 - 1u; rmin = r0; rmax = r1 - 1u;
            } else {
                const uint32_t colmask = ((1u << c1) - 1u) & ~((1u << c0) - 1u);
                const uint32_t byte0 = sh + 8u * woff;
                const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u;
                const uint32_t mm = PIX == 1u ? mn * 0x01010101u : mn * 0x00010001u;
                uint64_t sel = 0;   // the selection bits, a byte per row
#pragma unroll kRowUnroll
                for (uint32_t r = 0; r < 8u; r++) {
                    uint32_t q[8];   // the row's pixels
                    if constexpr (PIX == 1u) {
                        const uint32_t o = byte0 + r * d;   // byte of tile row r (8d bits)
                        const uint32_t w0 = o >> 2, sft = o & 3u;
                        const uint32_t a0 = s_row[w0], a1 = s_row[w0 + 1u], a2 = s_row[w0 + 2u];
                        const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(a1, a0, sft) |
                                              ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, sft) << 32);
                        uint32_t e0, e1;
                        expand_row(bits, d, e0, e1);
                        e0 = add_bytes(e0, mm);
                        e1 = add_bytes(e1, mm);
#pragma unroll
                        for (uint32_t c = 0; c < 4u; c++) {
                            q[c] = (e0 >> (8u * c)) & 0xFFu;
                            q[4u + c] = (e1 >> (8u * c)) & 0xFFu;
                        }
                    } else {
                        const uint32_t a = byte0 + r * d, ah = a + (d >> 1);   // the row's two 4-pixel halves
                        uint32_t e[4];
                        cut_row16(s_row + (a >> 2), s_row + (ah >> 2), a, ah, d, m32, mm, e[0], e[1], e[2], e[3]);
#pragma unroll
                        for (uint32_t c = 0; c < 4u; c++) {
                            q[2u * c] = e[c] & 0xFFFFu;
                            q[2u * c + 1u] = e[c] >> 16;
                        }
                    }
                    // the selection as bits first and as a mask per pixel after: a compare is used at once, so that no
                    // lane mask lives across the rows
                    uint32_t bits = 0;
#pragma unroll
                    for (uint32_t c = 0; c < 8u; c++) bits |= q[c] - lo <= span ? 1u << c : 0u;
                    bits &= (r >= r0 && r < r1) ? colmask : 0u;
                    uint32_t a_0 = 0, a_1 = 0, a_2 = 0;
#pragma unroll
                    for (uint32_t c = 0; c < 8u; c++) {
                        const uint32_t wv = (uint32_t)((int)q[c] * sa + sb) & (0u - ((bits >> c) & 1u));
                        a_0 += wv;
                        a_1 += c * wv;
                        a_2 += c * c * wv;
                        ww += (Sq)wv * wv;
                    }
                    sel |= (uint64_t)bits << (8u * r);
                    s += a_0;
                    s_c += a_1;
                    s_cc += a_2;
                    s_r += r * a_0;
                    s_rc += r * a_1;
                    s_rr += r * r * a_0;
                }
                const uint32_t sel_lo = (uint32_t)sel, sel_hi = (uint32_t)(sel >> 32);
                n = (uint32_t)__popc(sel_lo) + (uint32_t)__popc(sel_hi);
                uint32_t cols = sel_lo | sel_hi;   // the columns that hold a selected pixel
                cols |= cols >> 16;
                cols = (cols | (cols >> 8)) & 0xFFu;
                cmin = (uint32_t)__builtin_ctz(cols | 0x100u);
                cmax = 31u - (uint32_t)__builtin_clz(cols | 1u);
                rmin = sel_lo ? (uint32_t)__builtin_ctz(sel_lo) >> 3 : 4u + ((uint32_t)__builtin_ctz(sel_hi | 0x80000000u) >> 3);
                rmax = sel_hi ? 4u + ((31u - (uint32_t)__builtin_clz(sel_hi)) >> 3) : (31u - (uint32_t)__builtin_clz(sel_lo | 1u)) >> 3;
            }
            if (n) {
                // ---- 4. tile coordinates -> patch coordinates ----
                const int64_t dx = X0 - x, dy = Y0 - y;   // >= -7
                aN += n;
                aS += s;
                aSx += (uint64_t)((int64_t)s_c + dx * s);
                aSy += (uint64_t)((int64_t)s_r + dy * s);
                aSxx += (uint64_t)((int64_t)s_cc + 2 * dx * s_c + dx * dx * s);
                aSxy += (uint64_t)((int64_t)s_rc + dx * s_r + dy * s_c + dx * dy * s);
                aSyy += (uint64_t)((int64_t)s_rr + 2 * dy * s_r + dy * dy * s);
                aSww += ww;
                // a selected pixel lies inside the patch: 0 <= j < pw, 0 <= i < ph
                bmin = pk_min_u16(bmin, ((uint32_t)(dx + cmin) << 16) | (uint32_t)(dy + rmin));
                bmax = pk_max_u16(bmax, ((uint32_t)(dx + cmax + 1) << 16) | (uint32_t)(dy + rmax + 1));
            }
        }
        __syncthreads();   // every tile cut: the next group's payload may come
    }

    // ---- the wave's sums and box -> lane 63 -> the patch's entry ----
    const uint64_t tN = wave_total_u64(aN), tS = wave_total_u64(aS), tSx = wave_total_u64(aSx), tSy = wave_total_u64(aSy);
    const uint64_t tSxx = wave_total_u64(aSxx), tSxy = wave_total_u64(aSxy), tSyy = wave_total_u64(aSyy);
    const uint64_t tSww = wave_total_u64(aSww);
    bmin = wave_total_pk_u16<false>(bmin);
    bmax = wave_total_pk_u16<true>(bmax);
    if (lane == 63u) {
        uint64_t *m = p.moments + 8u * pi;
        m[0] = tN; m[1] = tS; m[2] = tSx; m[3] = tSy; m[4] = tSxx; m[5] = tSxy; m[6] = tSyy; m[7] = tSww;
        if (p.bbox) {
            int32_t *bx = p.bbox + 4u * pi;
            bx[0] = (int32_t)(bmin >> 16);
            bx[1] = (int32_t)(bmin & 0xFFFFu);
            bx[2] = (int32_t)(bmax >> 16) - 1;
            bx[3] = (int32_t)(bmax & 0xFFFFu) - 1;
        }
    }
}

hipError_t launch_patch_moments(const MomentParams &p0, uint32_t n_frames, uint32_t pix, hipStream_t s) {
    const uint32_t total = n_frames * p0.n_patches;   // (the host keeps it below 2^31)
    MomentParams p = p0;
    // a grid of 2^26 workgroups or more is 2^32 work-items or more, which one launch does not take
    for (p.block0 = 0; p.block0 < total; p.block0 += kMomentMaxGrid) {
        const uint32_t grid = total - p.block0 < kMomentMaxGrid ? total - p.block0 : kMomentMaxGrid;
        if (pix == 1u)
            hipLaunchKernelGGL((patch_moments_kernel<1>), dim3(grid), dim3(kMomentThreads), 0, s, p);
        else
            hipLaunchKernelGGL((patch_moments_kernel<2>), dim3(grid), dim3(kMomentThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dbde
