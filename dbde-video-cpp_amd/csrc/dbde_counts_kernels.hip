// dbde_counts_kernels.hip -- count projections for MI355X (gfx950, wave64): K U32 planes of the rw x rh window,
// out[k][y][x] = number of accepted frames f with p_f[y][x] <= thr_k(y, x) (unsigned compare in the pixel type),
// straight from the compressed bytes (no image is written).  DESIGN.md 4.19.
//
// counts_kernel<K, PIX>: K = 1..8 levels, PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  The launch shape and the
// load pipeline are project_kernel's (dbde_project_kernels.hip), as wproject_kernel took them: one 256-lane workgroup
// per (frame segment, window tile row, piece of kProjTilesOf(PIX) tiles), one lane per tile row (PIX 2: per half row),
// the segment's frames walked in groups of kCountsGroup with the payload loads of group k + 1, the depth / minimum loads
// of group k + 2 and the per-frame words of group k + 3 in flight while group k is counted, one barrier per group.  The
// body is this file's own.
//
// The count.  Each lane keeps cnt[K][kNpx] U32 in registers, started at 0, and the thresholds of its kNpx pixels packed
// as the pixels arrive: thr[K][2] dwords, four U8 or two U16 each, loaded once in front of the frame loop.  Scalar
// thresholds are broadcast into the same registers, so one body serves both modes.  An accepted frame adds
// (p_i <= thr[k][i]) to cnt[k][i]; a rejected frame, or one past the segment, adds nothing.  A map element is read only
// where the lane's pixel lies inside the window (the maps are in window coordinates).
//
// The value.  The counts are integers modulo 2^32, so neither the segments nor the order of anything matters.  With one
// segment each lane writes its window pixels of the K planes (old + cnt when accumulating); with more, the per-segment
// partials [segments][K][rw * rh] go to the workspace and counts_combine_kernel (one thread per window pixel, looping
// over k) adds them onto the prior content (accumulate) or onto partial 0.
#include "dbde_counts_kernels.h"

#include <type_traits>

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

constexpr uint32_t kCountsWaves = kProjThreads / 64u;

__device__ __forceinline__ uint32_t readlane(uint32_t v, uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j); }

// Frames of [0, p.n_frames) that the index accepted -> *p.out_count (added to it when accumulating).  Whole workgroup.
__device__ void write_count(const CountsParams &p) {
    __shared__ uint32_t s_c[kCountsWaves];
    const uint32_t tid = threadIdx.x;
    uint32_t c = 0;
    for (uint32_t g = tid; g < p.n_frames; g += kProjThreads) c += p.frame_ok[g] != 0u ? 1u : 0u;
    c = wave_sum(c);
    if ((tid & 63u) == 0u) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint64_t total = 0;
        for (uint32_t k = 0; k < kCountsWaves; k++) total += s_c[k];
        *p.out_count = (p.accumulate ? *p.out_count : 0ull) + total;
    }
}

}  // namespace

template <uint32_t K, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void counts_kernel(CountsParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(K >= 1u && K <= kCountsMaxLevels, "1..8 levels");
    constexpr uint32_t G = kCountsGroup, kTiles = kProjTilesOf(PIX), kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    constexpr uint32_t kPerDw = 4u / PIX, kBits = 8u * PIX, kMask = (1u << kBits) - 1u;                    // pixels per dword
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Px;
    __shared__ uint32_t s_wsum[2][G][2][kCountsWaves];   // per group of frames (double-buffered): wave depth totals, sums in front

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // tile of the piece, row of the tile, half of the row (PIX 2)
    const uint32_t t = PIX == 1u ? tid >> 3 : tid >> 4, r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u, hh = PIX == 1u ? 0u : tid & 1u;
    const uint32_t per_seg = p.rows * p.pieces;
    const uint32_t seg = blockIdx.x / per_seg;
    const uint32_t rem = blockIdx.x - seg * per_seg;
    const uint32_t br = rem / p.pieces, pc = rem - br * p.pieces;
    const uint32_t ty = p.ty0 + br, txp = p.tx0 + pc * kTiles;
    const uint32_t tx_b = (uint32_t)(p.x0 + p.rw - 1) >> 3;
    const uint32_t nt = tx_b + 1u - txp < kTiles ? tx_b + 1u - txp : kTiles;
    const bool has_tile = t < nt;
    const uint32_t pos0 = ty * p.w + txp;              // the piece's first tile (stream order)
    const uint32_t c = dec_chunk_of(p.geom, pos0), cb = dec_chunk_begin(p.geom, c);
    const uint32_t npre = pos0 - cb;                   // < 512 (roi_index_geometry)
    const uint32_t cstride = p.geom.cpf + 1u;
    const uint32_t f_begin = seg * p.fps;
    const uint64_t f_last = (uint64_t)f_begin + p.fps;
    const uint32_t f_end = f_last < p.n_frames ? (uint32_t)f_last : p.n_frames;
    const uint8_t *const end = p.stream + p.stream_bytes;

    // ---- this lane's pixels in the window, the counters and the thresholds ----
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const int yy = 8 * (int)ty + (int)r;
    const int xx0 = 8 * (int)(txp + t) + 4 * (int)hh;                  // the lane's first pixel column
    const bool row_in = has_tile && yy >= p.y0 && yy < p.y0 + p.rh;
    const uint64_t row0 = row_in ? (uint64_t)(yy - p.y0) * (uint64_t)p.rw : 0u;

    uint32_t cnt[K][kNpx];
    uint32_t thr[K][2];   // level j's thresholds of pixels kPerDw * h + i, element i of dword h
#pragma unroll
    for (uint32_t j = 0; j < K; j++) {
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) cnt[j][i] = 0u;
        thr[j][0] = thr[j][1] = 0u;
    }
    {
        const Px *const th = static_cast<const Px *>(p.thresholds);
        if (!p.maps) {
#pragma unroll
            for (uint32_t j = 0; j < K; j++) thr[j][0] = thr[j][1] = (uint32_t)th[j] * (PIX == 1u ? 0x01010101u : 0x00010001u);
        } else if (row_in) {
#pragma unroll
            for (uint32_t i = 0; i < kNpx; i++) {
                const int xx = xx0 + (int)i;
                if (xx < p.x0 || xx >= p.x0 + p.rw) continue;   // only elements of window pixels are read
                const uint64_t o = row0 + (uint64_t)(xx - p.x0);
#pragma unroll
                for (uint32_t j = 0; j < K; j++)
                    thr[j][i / kPerDw] |= (uint32_t)th[(uint64_t)j * p.level_stride + o] << (kBits * (i % kPerDw));
            }
        }
    }

    // ---- the per-frame words of a group: lane k < G holds frame g0 + k ----
    struct Words {
        uint32_t ok, base;
        uint64_t fo;
    };
    auto issue_words = [&](Words &wd, uint32_t g0) __attribute__((always_inline)) {
        const uint32_t g = g0 + (lane < G ? lane : 0u);
        wd.ok = 0u; wd.base = 0u; wd.fo = 0u;
        if (lane < G && g < f_end) {
            wd.ok = p.frame_ok[g];
            wd.fo = p.frame_offsets[g];
            wd.base = p.chunk_off[(size_t)g * cstride + c];
        }
    };

    // ---- one group of frames in flight ----
    struct Meta {
        uint32_t ok[G];            // uniform: frame accepted (and inside the segment)
        uint32_t base[G];          // uniform: payload words of the frame in front of the piece's chunk
        const uint8_t *fb[G];      // uniform: the frame
        uint32_t d8[G], ml[G], mh[G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
        uint32_t pre[G];           // this lane's dword of the depth bytes in front of the piece (masked where used)
    };
    struct Pay {
        uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[G];                // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };

    // pre: depth bytes [cb, pos0) of the frame, as aligned dwords, lane tid < ndw holding dword tid.  Every load is
    // unconditional inside an accepted frame (lanes without a tile read tile 0, lanes past ndw dword 0) and nothing
    // consumes a loaded value here, so that the loads stay in flight while the group in front is counted.
    // The U16 minima start at 28 + T, possibly at an odd address: read byte by byte.
    auto issue_meta = [&](Meta &m, const Words &wd) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.ok[k] = 0u; m.base[k] = 0u; m.fb[k] = p.stream; m.d8[k] = 0u; m.ml[k] = 0u; m.pre[k] = 0u;
            if constexpr (PIX == 2u) m.mh[k] = 0u;
            m.ok[k] = readlane(wd.ok, k);   // 0 past the segment
            if (m.ok[k]) {
                const uint64_t fo = (uint64_t)readlane((uint32_t)wd.fo, k) | ((uint64_t)readlane((uint32_t)(wd.fo >> 32), k) << 32);
                m.fb[k] = p.stream + fo;   // validated: the whole frame lies inside stream_bytes
                m.base[k] = readlane(wd.base, k);
                const uint8_t *darr = m.fb[k] + 24;
                const uint32_t tt = has_tile ? t : 0u;
                m.d8[k] = darr[pos0 + tt];
                if constexpr (PIX == 1u) {
                    m.ml[k] = darr[4u + p.T + pos0 + tt];
                } else {
                    m.ml[k] = darr[4u + p.T + 2u * (pos0 + tt)];
                    m.mh[k] = darr[5u + p.T + 2u * (pos0 + tt)];
                }
                const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(darr + cb) & 3u), ndw = (head + npre + 3u) >> 2;
                const uint8_t *a_lo = darr + cb - head;   // (pointer arithmetic: the load stays a global one)
                m.pre[k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (tid < ndw ? tid : 0u));   // inside the frame
            }
        }
    };
    // the mask of the depth bytes [cb, pos0) in this lane's pre dword of frame fb
    auto pre_keep = [&](const uint8_t *fb) __attribute__((always_inline)) -> uint32_t {
        const uintptr_t a = reinterpret_cast<uintptr_t>(fb + 24 + cb);
        const uint32_t head = (uint32_t)(a & 3u), ndw = (head + npre + 3u) >> 2;
        if (tid >= ndw) return 0u;
        const uint32_t lo = 4u * tid < head ? head - 4u * tid : 0u;   // bytes in front of cb
        const uint32_t hi = head + npre - 4u * tid;                   // bytes before pos0
        return (hi >= 4u ? ~0u : (1u << (8u * hi)) - 1u) & ~((1u << (8u * lo)) - 1u);
    };

    // the group's tile offsets (one barrier) and its payload loads
    uint32_t buf = 0;
    auto issue_payload = [&](const Meta &m, Pay &q) __attribute__((always_inline)) {
        uint32_t any = 0;
#pragma unroll
        for (uint32_t k = 0; k < G; k++) any |= m.ok[k];
        if (!any) {
#pragma unroll
            for (uint32_t k = 0; k < G; k++) { q.a0[k] = q.a1[k] = q.a2[k] = 0u; q.dms[k] = 0u; }
            return;
        }
        uint32_t incl[G];
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t d = has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;   // (a validated frame has none above)
            incl[k] = wave_scan_incl((PIX == 1u ? r == 0u : (tid & 15u) == 0u) ? d : 0u);   // the tile's first lane
            const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[k] & pre_keep(m.fb[k]), 0u, 0u));
            if (lane == 63u) s_wsum[buf][k][0][wave] = incl[k];
            if (lane == 0u) s_wsum[buf][k][1][wave] = pw;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kCountsWaves; w++) {
                wbase += w < wave ? s_wsum[buf][k][0][w] : 0u;
                PRE += s_wsum[buf][k][1][w];
            }
            const uint32_t d = has_tile ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;
            const uint32_t woff = m.base[k] + PRE + wbase + incl[k] - d;   // payload words in front of the tile
            // PIX 2, the half row: byte r * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
            const uint8_t *src = m.fb[k] + 32 + (PIX + 1ull) * p.T + 8ull * woff + r * d + hh * (d >> 1);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
            const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
            const bool need = m.ok[k] && has_tile && d != 0u, tail = q8 + 12 > end;
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
            if (need && !tail) {
                const uint32_t *q32 = reinterpret_cast<const uint32_t *>(q8);
                w0 = q32[0]; w1 = q32[1]; w2 = q32[2];
            }
            if (need && tail) {   // the stream's last bytes: only those in front of stream_bytes (rare: its waits cost nothing)
                const uint32_t nb = PIX == 1u ? d : (4u * d + 4u * hh * (d & 1u) + 7u) >> 3;
                for (uint32_t b = sh; b < sh + nb; b++) {
                    if (q8 + b >= end) break;
                    const uint32_t v = (uint32_t)q8[b] << (8u * (b & 3u));
                    if (b < 4u) w0 |= v; else if (b < 8u) w1 |= v; else w2 |= v;
                }
            }
            q.a0[k] = w0; q.a1[k] = w1; q.a2[k] = w2;
            if constexpr (PIX == 1u) q.dms[k] = d | (m.ml[k] << 8) | (sh << 16);
            else q.dms[k] = d | (sh << 8) | (m.ml[k] << 16) | (m.mh[k] << 24);
        }
        buf ^= 1u;
    };

    // cnt[j][kPerDw * h + i] += element i of dword v <= element i of thr[j][h], for the kPerDw pixels of dword v
    auto tally = [&](uint32_t h, uint32_t v) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t i = 0; i < kPerDw; i++) {
            const uint32_t px = (v >> (kBits * i)) & kMask;
#pragma unroll
            for (uint32_t j = 0; j < K; j++)
                cnt[j][kPerDw * h + i] += px <= ((thr[j][h] >> (kBits * i)) & kMask) ? 1u : 0u;
        }
    };
    auto accumulate = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;   // rejected (or past the segment): counts nothing
            if constexpr (PIX == 1u) {
                const uint32_t d = q.dms[k] & 0xFFu, sh = q.dms[k] >> 16;
                const uint32_t mm = ((q.dms[k] >> 8) & 0xFFu) * 0x01010101u;
                const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh) |
                                      ((uint64_t)__builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh) << 32);
                uint32_t px[2];
                expand_row(bits, d, px[0], px[1]);
                tally(0u, add_bytes(px[0], mm));
                tally(1u, add_bytes(px[1], mm));
            } else {
                const uint32_t d = q.dms[k] & 0xFFu, sh = (q.dms[k] >> 8) & 0xFFu, so = 4u * hh * (d & 1u);
                const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = (q.dms[k] >> 16) * 0x00010001u;
                const bool c2 = 2u * d >= 32u, c3 = 3u * d >= 32u;
                const uint32_t x0 = __builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh);
                const uint32_t x1 = __builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh);
                uint32_t e[2];
                cut_four16(__builtin_amdgcn_alignbit(x1, x0, so), x1 >> so, d, m32, mn2, c2, c3, e[0], e[1]);
                tally(0u, e[0]);
                tally(1u, e[1]);
            }
        }
    };

    // ---- the pipeline: count group k while group k + 1's payload and group k + 2's depth bytes load ----
    Meta m_cur, m_nxt, m_nn;
    Pay q_cur, q_nxt;
    Words w_nn;
    issue_words(w_nn, f_begin);
    issue_meta(m_cur, w_nn);
    issue_payload(m_cur, q_cur);
    issue_words(w_nn, f_begin + G);
    issue_meta(m_nxt, w_nn);
    issue_words(w_nn, f_begin + 2u * G);
    for (uint32_t g0 = f_begin; g0 < f_end; g0 += G) {
        issue_payload(m_nxt, q_nxt);
        issue_meta(m_nn, w_nn);
        issue_words(w_nn, g0 + 3u * G);
        accumulate(m_cur, q_cur);
        m_cur = m_nxt;
        q_cur = q_nxt;
        m_nxt = m_nn;
    }

    // ---- the window's pixels of this lane -> the planes, or this segment's partials ----
    if (row_in) {
        const bool direct = p.segments == 1u;
        uint32_t *const dst = direct ? p.out : p.ws + (uint64_t)seg * K * P;
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) {
            const int xx = xx0 + (int)i;
            if (xx < p.x0 || xx >= p.x0 + p.rw) continue;
            const uint64_t o = row0 + (uint64_t)(xx - p.x0);
#pragma unroll
            for (uint32_t j = 0; j < K; j++) {
                uint32_t *const q = dst + (uint64_t)j * P + o;
                *q = direct && p.accumulate ? *q + cnt[j][i] : cnt[j][i];
            }
        }
    }
    if (p.segments == 1u && blockIdx.x == 0u) write_count(p);
}

// Segments > 1: prior (ACC: what the planes hold) + partial 0 + partial 1 + ..., U32 additions modulo 2^32.  One thread
// per window pixel, looping over the levels; the partials are [segments][K][rw * rh], so each read is coalesced.
template <bool ACC>
__global__ __launch_bounds__(kProjCombineThreads) void counts_combine_kernel(CountsParams p) {
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint64_t i = (uint64_t)blockIdx.x * kProjCombineThreads + threadIdx.x;
    if (i < P) {
        const uint64_t KP = (uint64_t)p.levels * P;
        for (uint32_t j = 0; j < p.levels; j++) {
            const uint32_t *const ws = p.ws + (uint64_t)j * P + i;
            uint32_t *const out = p.out + (uint64_t)j * P + i;
            uint32_t v = ACC ? *out : 0u;
            for (uint32_t s = 0; s < p.segments; s++) v += ws[(uint64_t)s * KP];
            *out = v;
        }
    }
    if (blockIdx.x == 0u) write_count(p);
}

uint64_t counts_workspace_bytes(uint32_t levels, uint32_t segments, uint64_t pixels) {
    if (segments <= 1u) return 0;
    return (4ull * segments * levels * pixels + 15u) & ~(uint64_t)15;
}

typedef void (*CountsKernel)(CountsParams);

hipError_t launch_counts(const CountsParams &p, uint32_t levels, uint32_t pix, hipStream_t s) {
    static const CountsKernel table[2][kCountsMaxLevels] = {
        {counts_kernel<1, 1>, counts_kernel<2, 1>, counts_kernel<3, 1>, counts_kernel<4, 1>,
         counts_kernel<5, 1>, counts_kernel<6, 1>, counts_kernel<7, 1>, counts_kernel<8, 1>},
        {counts_kernel<1, 2>, counts_kernel<2, 2>, counts_kernel<3, 2>, counts_kernel<4, 2>,
         counts_kernel<5, 2>, counts_kernel<6, 2>, counts_kernel<7, 2>, counts_kernel<8, 2>}};
    if (levels < 1u || levels > kCountsMaxLevels || levels != p.levels || (pix != 1u && pix != 2u))
        return hipErrorInvalidValue;
    const uint32_t grid = p.pieces * p.rows * p.segments;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(table[pix - 1u][levels - 1u], dim3(grid), dim3(kProjThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.segments == 1u) return e;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint32_t cgrid = (uint32_t)((P + kProjCombineThreads - 1u) / kProjCombineThreads);
    const CountsKernel combine = p.accumulate ? counts_combine_kernel<true> : counts_combine_kernel<false>;
    hipLaunchKernelGGL(combine, dim3(cgrid), dim3(kProjCombineThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
