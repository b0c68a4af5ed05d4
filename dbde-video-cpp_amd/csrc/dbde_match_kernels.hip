// dbde_match_kernels.hip -- patch match for MI355X (gfx950, wave64): for each of K search patches per frame, the
// correlation surfaces of a tw x th template over the (2S + 1)^2 integer shifts of a search radius S, straight from the
// compressed bytes (no pixel is written): prod = sum T P, sum = sum P, sq = sum P^2 over the template's footprint.
//
// The index pass (decode_index_kernel on roi_index_geometry's chunks) gives a payload offset at the start of every tile
// row, so it runs once per call however many patches there are; match_patches_kernel<PIX> then visits only the search
// patches' tiles.
//
// match_patches_kernel<PIX>: PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  One 256-lane workgroup per (frame,
// patch); the LDS is sized per launch (MatchLayout, dbde_match_kernels.h).
//   Front half, decode_patches_kernel's steps 1-3 (dbde_patch_kernels.hip), repeated here so that the patch decoder's
//   listing stays as it is: a wave takes a group of G tile rows, one tile per lane (prefix bytes by v_sad_u8, one
//   segmented scan, the rows' payload ranges into LDS, each lane cuts its tile's 8 rows), and writes the tiles into the
//   band at their tile-aligned place, fill pixels included.  Up to four waves take a group each per step.  Meanwhile
//   all lanes copy the template into LDS, rows padded with zeros to whole dwords.
//   Back half: an item is (shift, slice); lane t takes items t, t + 256, ...; consecutive lanes have consecutive dx,
//   then dy, then slice.  For each template row i of its slice (i = slice, slice + slices, ...) the lane walks the row
//   four dwords at a time, their eight reads issued together: the template dword is one address for all lanes of a slice
//   (a broadcast read), the patch dword at byte offset (j + dx) comes from two aligned reads, one of them carried over
//   from the step before, and a v_alignbyte.  8-bit pixels: one v_dot4_u32_u8 each for prod, sq (p . p) and sum
//   (p . 0x01010101) into U32 (an entry is at most 128^2 * 255^2 < 2^32).  16-bit pixels: one product can pass 32 bits, so prod and sq are accumulated in
//   64 bits (v_mad_u64_u32).  The last dword of a row is masked to the template's width.  With slices == 1 a lane owns
//   its shift and stores the entries; otherwise the partial sums meet in U64 accumulators in LDS (ds_add_u64; integers:
//   the order is free) and lane s stores shift s.
// Every live entry is written once by plain stores; a rejected frame's and a dead patch's entries stay untouched.
#include "dbde_match_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));   // native vector for the nontemporal builtins

constexpr uint32_t kPrefixBatch = 8;   // prefix dwords a lane has in flight at once

// One dword of template (t) and of patch (p) pixels into the three sums.  PIX = 1: four pixels, U32 sums; PIX = 2: two
// pixels, prod and sq in 64 bits.
template <uint32_t PIX, uint32_t STATS, typename Acc>
__device__ __forceinline__ void match_step(uint32_t t, uint32_t p, Acc &prod, uint32_t &sum, Acc &sq) {
    if constexpr (PIX == 1u) {
        if constexpr ((STATS & kMatchProd) != 0u) prod = __builtin_amdgcn_udot4(t, p, prod, false);
        if constexpr ((STATS & kMatchSum) != 0u) sum = __builtin_amdgcn_udot4(p, 0x01010101u, sum, false);
        if constexpr ((STATS & kMatchSq) != 0u) sq = __builtin_amdgcn_udot4(p, p, sq, false);
    } else {
        const uint32_t p0 = p & 0xFFFFu, p1 = p >> 16;
        if constexpr ((STATS & kMatchProd) != 0u) prod += (uint64_t)(t & 0xFFFFu) * p0 + (uint64_t)(t >> 16) * p1;
        if constexpr ((STATS & kMatchSum) != 0u) sum += p0 + p1;   // at most 128^2 * 65535 < 2^31
        if constexpr ((STATS & kMatchSq) != 0u) sq += (uint64_t)p0 * p0 + (uint64_t)p1 * p1;
    }
}

// The template rows i0, i0 + slices, ... against the band at byte `at` (the patch pixel under the template's (0, 0)).
template <uint32_t PIX, uint32_t STATS>
__device__ __forceinline__ void match_rows(const uint32_t *s_band, const uint32_t *s_tmpl, uint32_t at, uint32_t pitch_bytes,
                                           uint32_t tw4, uint32_t th, uint32_t i0, uint32_t slices, uint32_t tail,
                                           uint64_t &o_prod, uint64_t &o_sum, uint64_t &o_sq) {
    typedef typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type Acc;
    Acc prod = 0, sq = 0;
    uint32_t sum = 0;
    const uint32_t sft = at & 3u;
    const uint32_t last = tw4 - 1u;
    for (uint32_t i = i0; i < th; i += slices) {
        const uint32_t *q = s_band + ((at + i * pitch_bytes) >> 2);   // (pitch_bytes is a multiple of 4: sft holds for every row)
        const uint32_t *t = s_tmpl + i * tw4;
        uint32_t lo = q[0];
        // kMatchBatch dwords at a time, all their reads issued before the first is used: one read per step, each waited
        // for, left the loop bound by the LDS latency.  A batch that reaches beyond the row reads the row's last dword
        // again (a clamped index keeps the reads unconditional) and masks what it read to nothing.
        for (uint32_t g0 = 0; g0 < tw4; g0 += kMatchBatch) {
            uint32_t hi[kMatchBatch], tv[kMatchBatch];
#pragma unroll
            for (uint32_t c = 0; c < kMatchBatch; c++) {
                const uint32_t g = g0 + c < last ? g0 + c : last;
                hi[c] = q[g + 1u];
                tv[c] = t[g];
            }
#pragma unroll
            for (uint32_t c = 0; c < kMatchBatch; c++) {
                const uint32_t keep = g0 + c < last ? 0xFFFFFFFFu : (g0 + c == last ? tail : 0u);
                const uint32_t p = __builtin_amdgcn_alignbyte(hi[c], c ? hi[c - 1u] : lo, sft) & keep;
                match_step<PIX, STATS, Acc>(tv[c], p, prod, sum, sq);
            }
            lo = hi[kMatchBatch - 1u];
        }
    }
    o_prod = prod;
    o_sum = sum;
    o_sq = sq;
}

}  // namespace

template <uint32_t PIX>
__global__ __launch_bounds__(kMatchThreads) void match_patches_kernel(MatchParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Pix;
    typedef typename std::conditional<PIX == 1u, uint2, uint4>::type Row;   // one tile row of 8 pixels
    extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
    uint32_t *s_band = s_lds;
    uint32_t *s_tmpl = s_lds + (p.lds.off_tmpl >> 2);
    uint32_t *s_work = s_lds + (p.lds.off_work >> 2);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t b = p.block0 + blockIdx.x;
    const uint32_t k = b % p.n_patches, f = b / p.n_patches;
    if (!p.frame_ok[f]) return;   // rejected frame: its entries stay untouched
    if (p.counts) {
        const uint32_t cnt = p.counts[f];
        if (k >= (cnt < p.n_patches ? cnt : p.n_patches)) return;   // not a live patch: untouched
    }
    const size_t pi = (size_t)f * p.n_patches + k;
    const int ox = p.origins[2u * pi], oy = p.origins[2u * pi + 1u];
    const bool fill_mode = p.mode == kMatchFill;
    int x, y;
    if (!fill_mode) {   // the window decoder's rule
        x = ox < 0 ? 0 : (ox > p.W - p.pw ? p.W - p.pw : ox);
        y = oy < 0 ? 0 : (oy > p.H - p.ph ? p.H - p.ph : oy);
    } else {   // any origin at or beyond these bounds gives the same patch, all fill
        x = ox < -p.pw ? -p.pw : (ox > p.W ? p.W : ox);
        y = oy < -p.ph ? -p.ph : (oy > p.H ? p.H : oy);
    }
    if (p.used && tid == 0u) {
        p.used[2u * pi] = fill_mode ? ox : x;
        p.used[2u * pi + 1u] = fill_mode ? oy : y;
    }
    // tile coordinates are signed (a fill-mode patch can start left of or above the frame); pw, ph <= 160
    const int tx_a = x >> 3, tx_b = (x + p.pw - 1) >> 3;
    const int ty_a = y >> 3, ty_b = (y + p.ph - 1) >> 3;

    // ---- the template -> LDS, rows padded with zeros to whole dwords ----
    const uint32_t tw = p.tw, th = p.th, tw4 = p.lds.tw4;
    {
        const Pix *tp = reinterpret_cast<const Pix *>(p.templates) + (p.per_patch ? (size_t)k * th * tw : (size_t)0);
        constexpr uint32_t kPer = 4u / PIX;
        for (uint32_t i = tid; i < th * tw4; i += kMatchThreads) {
            const uint32_t r = i / tw4, j0 = (i - r * tw4) * kPer;
            uint32_t v = 0;
#pragma unroll
            for (uint32_t c = 0; c < kPer; c++)
                if (j0 + c < tw) v |= (uint32_t)tp[r * tw + j0 + c] << (8u * PIX * c);
            s_tmpl[i] = v;
        }
    }

    // ---- front half: the search patch's tiles -> the band ----
    const uint32_t mtx = p.mtx;
    const uint32_t lr = lane / mtx, lc = lane - lr * mtx;
    const int tx = tx_a + (int)lc;
    const int txs = tx_a < 0 ? 0 : tx_a, txe = tx_b > (int)p.w - 1 ? (int)p.w - 1 : tx_b;
    const uint8_t *fb = p.stream + p.frame_offsets[f];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *darr = fb + 24;
    const uint8_t *marr = fb + 28 + p.T;
    const uint8_t *pay = fb + 32 + (PIX + 1ull) * p.T;
    const uint32_t row_bytes = kMatchRowBytesOf(mtx, PIX);
    uint32_t *s_row = s_work + wv * (p.lds.pay_wave >> 2) + lr * (row_bytes >> 2);   // (lanes of no row never use it)
    Row fillpx;
    if constexpr (PIX == 1u) {
        fillpx = make_uint2(p.fill * 0x01010101u, p.fill * 0x01010101u);
    } else {
        const uint32_t f2 = p.fill * 0x00010001u;
        fillpx = make_uint4(f2, f2, f2, f2);
    }

    for (uint32_t step = 0; step < p.steps; step++) {   // (the same count in every wave: the barriers are uniform)
        const int tyg = ty_a + (int)((step * p.dwaves + wv) * p.G);   // first tile row of this wave's group
        const int ty = tyg + (int)lr;
        const bool row_live = wv < p.dwaves && lr < p.G && ty <= ty_b;
        const bool row_has = row_live && ty >= 0 && ty < (int)p.h && txs <= txe;   // the row has tiles inside the frame
        const bool valid = row_has && tx >= txs && tx <= txe;

        // ---- 1. depth / minimum bytes, offsets ----
        uint32_t base = 0, pre = 0;
        if (row_has) {
            const uint32_t pos0 = (uint32_t)ty * p.w + (uint32_t)txs;
            const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
            base = p.chunk_off[(size_t)f * (p.geom.cpf + 1u) + c];
            const uint32_t npre = pos0 - cb;   // < 512 (roi_index_geometry)
            if (npre) {
                // bytes [s, e) of the dwords at a0: the dwords lie inside the frame (24 header bytes in front, the row's
                // own depth bytes and the minima behind)
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
        // one scan for both sums: a row's depths total at most 64 * 16, its prefix bytes 511 * 16
        uint32_t sc = d | (pre << 16);
        for (uint32_t o = 1; o < mtx; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)sc, o, 64);
            if (lc >= o) sc += t;
        }
        const uint32_t last = lr * mtx + mtx - 1u;
        const uint32_t tot = (uint32_t)__shfl((int)sc, (int)(last < 63u ? last : 63u), 64);
        const uint32_t S = tot & 0xFFFFu, PRE = tot >> 16;   // the row's payload words, and those in front of it
        const uint32_t woff = (sc & 0xFFFFu) - d;            // payload words in front of this tile inside the row

        // ---- 2. the rows' payload ranges into LDS ----
        uint32_t sh = 0;
        if (row_has) {
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
        __syncthreads();

        // ---- 3. tile rows -> registers -> the band, at the tile's own place ----
        Row px[8];
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) px[r] = fillpx;
        if (valid) {
            if constexpr (PIX == 1u) {
                const uint32_t mm = mn * 0x01010101u;
#pragma unroll
                for (uint32_t r = 0; r < 8u; r++) {
                    const uint32_t o = sh + 8u * woff + r * d;   // byte of tile row r (8d bits)
                    const uint32_t w0 = o >> 2, s = o & 3u;
                    const uint32_t a0 = s_row[w0], a1 = s_row[w0 + 1u], a2 = s_row[w0 + 2u];
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
                    cut_row16(s_row + (a >> 2), s_row + (ah >> 2), a, ah, d, m32, mn2, px[r].x, px[r].y, px[r].z, px[r].w);
                }
            }
            // fill mode: the encoder's padding beyond W or H is not part of the frame
            const uint32_t ncol = (uint32_t)(p.W - 8 * tx), nrow = (uint32_t)(p.H - 8 * ty);   // >= 1
            if (fill_mode && (ncol < 8u || nrow < 8u)) {
                // the dword holding pixels [a, a + 4 / PIX) of a tile row: which of its pixels lie left of column ncol
                auto keep = [&](uint32_t a) -> uint32_t {
                    const uint32_t n = ncol > a ? ncol - a : 0u;
                    return n >= 4u / PIX ? 0xFFFFFFFFu : (1u << (8u * PIX * n)) - 1u;
                };
#pragma unroll
                for (uint32_t r = 0; r < 8u; r++) {
                    if (r >= nrow) {
                        px[r] = fillpx;
                    } else if constexpr (PIX == 1u) {
                        const uint32_t m0 = keep(0u), m1 = keep(4u);
                        px[r].x = (px[r].x & m0) | (fillpx.x & ~m0);
                        px[r].y = (px[r].y & m1) | (fillpx.y & ~m1);
                    } else {
                        const uint32_t m0 = keep(0u), m1 = keep(2u), m2 = keep(4u), m3 = keep(6u);
                        px[r].x = (px[r].x & m0) | (fillpx.x & ~m0);
                        px[r].y = (px[r].y & m1) | (fillpx.x & ~m1);
                        px[r].z = (px[r].z & m2) | (fillpx.x & ~m2);
                        px[r].w = (px[r].w & m3) | (fillpx.x & ~m3);
                    }
                }
            }
        }
        if (row_live && (valid || fill_mode)) {   // (the band is apart from the payload: no barrier in between)
            uint32_t *dst = s_band + (uint32_t)(8 * (ty - ty_a)) * p.lds.pitch + 2u * PIX * lc;   // the pitch is odd: dwords
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                uint32_t *o = dst + r * p.lds.pitch;
                o[0] = px[r].x;
                o[1] = px[r].y;
                if constexpr (PIX == 2u) {
                    o[2] = px[r].z;
                    o[3] = px[r].w;
                }
            }
        }
        __syncthreads();   // every tile cut: the next step's payload may come
    }

    // ---- back half: the surfaces ----
    const uint32_t D = p.D, nsh = D * D, slices = p.slices, items = nsh * slices;
    uint64_t *s_acc = reinterpret_cast<uint64_t *>(s_work);   // [nsh][3], where slices > 1 (the payload is done with)
    if (slices > 1u) {
        for (uint32_t i = tid; i < 3u * nsh; i += kMatchThreads) s_acc[i] = 0ull;
        __syncthreads();
    }
    const uint32_t pitch_bytes = 4u * p.lds.pitch;
    const uint32_t bx = (uint32_t)(x - 8 * tx_a), by = (uint32_t)(y - 8 * ty_a);   // the patch's place in the band: 0 .. 7
    const uint32_t vb = ((tw * PIX - 1u) & 3u) + 1u;   // bytes of a template row's last dword
    const uint32_t tail = vb == 4u ? 0xFFFFFFFFu : (1u << (8u * vb)) - 1u;
    const uint32_t stats = p.stats;
    const size_t out0 = pi * nsh;
    for (uint32_t it = tid; it < items; it += kMatchThreads) {
        const uint32_t sl = it / nsh, s = it - sl * nsh;
        const uint32_t dy = s / D, dx = s - dy * D;   // (offset by S: the surface's row and column)
        const uint32_t at = (by + dy) * pitch_bytes + (bx + dx) * PIX;
        uint64_t v_prod, v_sum, v_sq;
        if (stats == (kMatchProd | kMatchSum | kMatchSq))
            match_rows<PIX, 7u>(s_band, s_tmpl, at, pitch_bytes, tw4, th, sl, slices, tail, v_prod, v_sum, v_sq);
        else if (stats == kMatchProd)
            match_rows<PIX, kMatchProd>(s_band, s_tmpl, at, pitch_bytes, tw4, th, sl, slices, tail, v_prod, v_sum, v_sq);
        else   // the other masks: all three sums, the requested ones leave
            match_rows<PIX, 7u>(s_band, s_tmpl, at, pitch_bytes, tw4, th, sl, slices, tail, v_prod, v_sum, v_sq);
        if (slices == 1u) {
            if (stats & kMatchProd) p.prod[out0 + s] = v_prod;
            if (stats & kMatchSum) p.sum[out0 + s] = v_sum;
            if (stats & kMatchSq) p.sq[out0 + s] = v_sq;
        } else {
            if (stats & kMatchProd) atomicAdd(reinterpret_cast<unsigned long long *>(s_acc + 3u * s), (unsigned long long)v_prod);
            if (stats & kMatchSum) atomicAdd(reinterpret_cast<unsigned long long *>(s_acc + 3u * s + 1u), (unsigned long long)v_sum);
            if (stats & kMatchSq) atomicAdd(reinterpret_cast<unsigned long long *>(s_acc + 3u * s + 2u), (unsigned long long)v_sq);
        }
    }
    if (slices > 1u) {
        __syncthreads();
        for (uint32_t s = tid; s < nsh; s += kMatchThreads) {
            if (stats & kMatchProd) p.prod[out0 + s] = s_acc[3u * s];
            if (stats & kMatchSum) p.sum[out0 + s] = s_acc[3u * s + 1u];
            if (stats & kMatchSq) p.sq[out0 + s] = s_acc[3u * s + 2u];
        }
    }
}

hipError_t launch_match_patches(const MatchParams &p0, uint32_t n_frames, uint32_t pix, hipStream_t s) {
    const uint32_t total = n_frames * p0.n_patches;   // (the host keeps it below 2^31)
    MatchParams p = p0;
    const void *fn = pix == 1u ? reinterpret_cast<const void *>(match_patches_kernel<1>)
                               : reinterpret_cast<const void *>(match_patches_kernel<2>);
    if (p.lds.bytes > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds.bytes);
        if (e != hipSuccess) return e;
    }
    // a grid of 2^24 workgroups or more is 2^32 work-items or more, which one launch does not take
    for (p.block0 = 0; p.block0 < total; p.block0 += kMatchMaxGrid) {
        const uint32_t grid = total - p.block0 < kMatchMaxGrid ? total - p.block0 : kMatchMaxGrid;
        if (pix == 1u)
            hipLaunchKernelGGL((match_patches_kernel<1>), dim3(grid), dim3(kMatchThreads), p.lds.bytes, s, p);
        else
            hipLaunchKernelGGL((match_patches_kernel<2>), dim3(grid), dim3(kMatchThreads), p.lds.bytes, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dbde
