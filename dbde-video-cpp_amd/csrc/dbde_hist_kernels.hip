// dbde_hist_kernels.hip -- per-frame intensity histograms for MI355X (gfx950, wave64): the counts of the rw x rh
// window's pixel values per frame, straight from the compressed bytes (no image is written).
//
// hist_kernel<PIX, NB>: PIX = 1 for DBDE frames (U8 pixels, depth 0..8, payload at 32 + 2T), PIX = 2 for DBDE16 frames
// (U16 pixels, depth 0..16, payload at 32 + 3T).  NB: bins of the LDS histogram, 256 (one copy per wave) or 4,096
// (DBDE16 only, one copy).  One workgroup per (frame, segment), a segment being a run of consecutive pieces of the
// frame's window, a piece kHistTilesOf(PIX) tiles of one window tile row.  Lanes, loads and the offsets scan are the
// projection kernel's (dbde_project_kernels.hip): PIX = 1 one lane per tile row (expand_row / add_bytes), PIX = 2 one
// lane per half tile row (cut_four16).  The pipeline is the projection's with pieces in place of frames: while the
// pieces of group k are counted, group k + 1's payload, group k + 2's depth / minimum bytes and group k + 3's chunk
// offsets are in flight.
//
// Counting.  A depth-d tile's pixels lie in [min, min + 2^d - 1] (modulo 2^(8 PIX)).  When that range does not wrap
// and falls into one bin (depth 0 always; bins == 1 always), the tile is whole: its first lane adds the tile's window
// pixel count to that bin with one LDS add, and no lane of it loads payload.  Every other tile's lanes cut their
// pixels, fold each run of equal bins along the row into one count, and add each run with one LDS add.
// At the end the workgroup adds its nonzero bins into the frame's row (U32) and the total (U64) with global atomics:
// at most segments * bins adds per frame and output.  The rows of the accepted frames are zeroed by hist_init_kernel
// first; a rejected frame's workgroups return at once, so its row is never touched.
#include "dbde_hist_kernels.h"

#include "dbde_bits.h"
#include "dbde_device.h"

namespace dbde {

namespace {

__device__ __forceinline__ uint32_t readlane(uint32_t v, uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j); }

// Bits i < n (n may be <= 0 or >= 32) and bits i >= n.
__device__ __forceinline__ uint32_t bits_below(int n) { return n <= 0 ? 0u : (n >= 32 ? ~0u : (1u << n) - 1u); }

}  // namespace

template <uint32_t PIX, uint32_t NB>
__global__ __launch_bounds__(kHistThreads) void hist_kernel(HistParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(NB == kHistSmallBins || (PIX == 2u && NB == kHistLargeBins), "an LDS histogram size of the plan");
    constexpr uint32_t G = kHistGroup, kTiles = kHistTilesOf(PIX), kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    constexpr uint32_t kCopies = kHistCopiesOf(NB), kPixMax = PIX == 1u ? 0xFFu : 0xFFFFu;
    __shared__ uint32_t s_hist[kCopies * NB];
    __shared__ uint32_t s_wsum[2][G][2][kHistWaves];   // per group of pieces (double-buffered): wave depth totals, sums in front

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // tile of the piece, row of the tile, half of the row (PIX 2)
    const uint32_t t = PIX == 1u ? tid >> 3 : tid >> 4, r = PIX == 1u ? tid & 7u : (tid >> 1) & 7u, hh = PIX == 1u ? 0u : tid & 1u;
    const bool leader = PIX == 1u ? r == 0u : (tid & 15u) == 0u;   // the tile's first lane
    const uint32_t g = blockIdx.x / p.segments, seg = blockIdx.x - g * p.segments;
    if (!p.frame_ok[g]) return;   // rejected: the whole workgroup leaves, its row is not touched
    const uint8_t *const fb = p.stream + p.frame_offsets[g];   // validated: the whole frame lies inside stream_bytes
    const uint8_t *const darr = fb + 24;
    const uint32_t n_pieces = p.rows * p.pieces;
    const uint32_t p_begin = seg * p.pps;
    const uint32_t p_end = n_pieces - p_begin < p.pps ? n_pieces : p_begin + p.pps;
    const uint32_t tx_b = (uint32_t)(p.x0 + p.rw - 1) >> 3;
    const uint32_t *const coff = p.chunk_off + (size_t)g * (p.geom.cpf + 1u);
    const uint8_t *const end = p.stream + p.stream_bytes;
    const uint32_t shift = p.shift, last = p.bins - 1u;
    uint32_t *const hist = s_hist + (kCopies > 1u ? wave * NB : 0u);

    for (uint32_t i = tid; i < kCopies * NB; i += kHistThreads) s_hist[i] = 0u;
    __syncthreads();

    auto binof = [&](uint32_t v) __attribute__((always_inline)) -> uint32_t {
        const uint32_t b = v >> shift;
        return b < last ? b : last;
    };
    // a depth-d tile of minimum mn falls into one bin
    auto whole = [&](uint32_t d, uint32_t mn) __attribute__((always_inline)) -> bool {
        const uint32_t hi = mn + (1u << d) - 1u;
        return d == 0u || last == 0u || (hi <= kPixMax && binof(mn) == binof(hi));
    };
    // piece pi of the window: its tile row and first tile column
    auto piece = [&](uint32_t pi, uint32_t &ty, uint32_t &txp) __attribute__((always_inline)) {
        const uint32_t br = pi / p.pieces;
        ty = p.ty0 + br;
        txp = p.tx0 + (pi - br * p.pieces) * kTiles;
    };
    // this lane's window pixels of a piece: bit i = pixel i (0 when the lane has no tile or its row is outside)
    auto lane_mask = [&](uint32_t ty, uint32_t txp) __attribute__((always_inline)) -> uint32_t {
        const uint32_t nt = tx_b + 1u - txp < kTiles ? tx_b + 1u - txp : kTiles;
        const int yy = 8 * (int)ty + (int)r;
        if (t >= nt || yy < p.y0 || yy >= p.y0 + p.rh) return 0u;
        const int xb = 8 * (int)(txp + t) + 4 * (int)hh;
        return bits_below(p.x0 + p.rw - xb) & ~bits_below(p.x0 - xb) & ((1u << kNpx) - 1u);
    };

    // ---- the chunk offsets of a group, one group ahead of their use: lane k < G holds piece p0 + k ----
    auto issue_words = [&](uint32_t &base, uint32_t p0) __attribute__((always_inline)) {
        base = 0u;
        const uint32_t pi = p0 + lane;
        if (lane < G && pi < p_end) {
            uint32_t ty, txp;
            piece(pi, ty, txp);
            base = coff[dec_chunk_of(p.geom, ty * p.w + txp)];
        }
    };

    // ---- one group of pieces in flight ----
    struct Meta {
        uint32_t ok[G];                 // uniform: the piece lies in the segment
        uint32_t ty[G], txp[G];         // uniform: the piece's tile row and first tile column
        uint32_t cb[G], npre[G];        // uniform: its chunk's first tile, depth bytes from there to the piece
        uint32_t base[G];               // uniform: payload words of the frame in front of the chunk
        uint32_t d8[G], ml[G], mh[G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
        uint32_t pre[G];                // this lane's dword of the depth bytes in front of the piece (masked where used)
    };
    struct Pay {
        uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[G];                // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };

    // As the projection's issue_meta: every load is unconditional inside the frame and nothing consumes a loaded value
    // here.  The U16 minima start at 28 + T, possibly at an odd address: read byte by byte.
    auto issue_meta = [&](Meta &m, uint32_t words, uint32_t p0) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            m.ok[k] = p0 + k < p_end ? 1u : 0u;
            m.ty[k] = 0u; m.txp[k] = 0u; m.cb[k] = 0u; m.npre[k] = 0u; m.base[k] = 0u;
            m.d8[k] = 0u; m.ml[k] = 0u; m.mh[k] = 0u; m.pre[k] = 0u;
            if (m.ok[k]) {
                piece(p0 + k, m.ty[k], m.txp[k]);
                const uint32_t pos0 = m.ty[k] * p.w + m.txp[k];
                m.cb[k] = dec_chunk_begin(p.geom, dec_chunk_of(p.geom, pos0));
                m.npre[k] = pos0 - m.cb[k];   // < 512 (roi_index_geometry)
                m.base[k] = readlane(words, k);
                const uint32_t nt = tx_b + 1u - m.txp[k] < kTiles ? tx_b + 1u - m.txp[k] : kTiles;
                const uint32_t tt = t < nt ? t : 0u;
                m.d8[k] = darr[pos0 + tt];
                if constexpr (PIX == 1u) {
                    m.ml[k] = darr[4u + p.T + pos0 + tt];
                } else {
                    m.ml[k] = darr[4u + p.T + 2u * (pos0 + tt)];
                    m.mh[k] = darr[5u + p.T + 2u * (pos0 + tt)];
                }
                const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(darr + m.cb[k]) & 3u);
                const uint32_t ndw = (head + m.npre[k] + 3u) >> 2;
                const uint8_t *a_lo = darr + m.cb[k] - head;   // (pointer arithmetic: the load stays a global one)
                m.pre[k] = *reinterpret_cast<const uint32_t *>(a_lo + 4u * (tid < ndw ? tid : 0u));   // inside the frame
            }
        }
    };
    // the mask of the depth bytes [cb, cb + npre) in this lane's pre dword
    auto pre_keep = [&](uint32_t cb, uint32_t npre) __attribute__((always_inline)) -> uint32_t {
        const uintptr_t a = reinterpret_cast<uintptr_t>(darr + cb);
        const uint32_t head = (uint32_t)(a & 3u), ndw = (head + npre + 3u) >> 2;
        if (tid >= ndw) return 0u;
        const uint32_t lo = 4u * tid < head ? head - 4u * tid : 0u;   // bytes in front of cb
        const uint32_t hi = head + npre - 4u * tid;                   // bytes before the piece
        return (hi >= 4u ? ~0u : (1u << (8u * hi)) - 1u) & ~((1u << (8u * lo)) - 1u);
    };

    // the group's tile offsets (one barrier) and its payload loads (only lanes of split tiles inside the window)
    uint32_t buf = 0;
    auto issue_payload = [&](const Meta &m, Pay &q) __attribute__((always_inline)) {
        uint32_t incl[G];
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t nt = tx_b + 1u - m.txp[k] < kTiles ? tx_b + 1u - m.txp[k] : kTiles;
            const uint32_t d = t < nt ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;   // (a validated frame has none above)
            incl[k] = wave_scan_incl(leader ? d : 0u);
            const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[k] & pre_keep(m.cb[k], m.npre[k]), 0u, 0u));
            if (lane == 63u) s_wsum[buf][k][0][wave] = incl[k];
            if (lane == 0u) s_wsum[buf][k][1][wave] = pw;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kHistWaves; w++) {
                wbase += w < wave ? s_wsum[buf][k][0][w] : 0u;
                PRE += s_wsum[buf][k][1][w];
            }
            const uint32_t nt = tx_b + 1u - m.txp[k] < kTiles ? tx_b + 1u - m.txp[k] : kTiles;
            const uint32_t d = t < nt ? (m.d8[k] > kDmax ? kDmax : m.d8[k]) : 0u;
            const uint32_t mn = PIX == 1u ? m.ml[k] : m.ml[k] | (m.mh[k] << 8);
            const uint32_t woff = m.base[k] + PRE + wbase + incl[k] - d;   // payload words in front of the tile
            // PIX 2, the half row: byte r * d + h * (d / 2), a nibble further when d is odd; 4d bits (+ 4) <= 8 bytes
            const uint8_t *src = fb + 32 + (PIX + 1ull) * p.T + 8ull * woff + r * d + hh * (d >> 1);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
            const uint8_t *q8 = src - sh;   // (pointer arithmetic: the loads stay global ones)
            const bool need = m.ok[k] && !whole(d, mn) && lane_mask(m.ty[k], m.txp[k]) != 0u, tail = q8 + 12 > end;
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
            if (need && !tail) {
                const uint32_t *q32 = reinterpret_cast<const uint32_t *>(q8);
                w0 = q32[0]; w1 = q32[1]; w2 = q32[2];
            }
            if (need && tail) {   // the stream's last bytes: only those in front of stream_bytes
                const uint32_t nb = PIX == 1u ? d : (4u * d + 4u * hh * (d & 1u) + 7u) >> 3;
                for (uint32_t b = sh; b < sh + nb; b++) {
                    if (q8 + b >= end) break;
                    const uint32_t v = (uint32_t)q8[b] << (8u * (b & 3u));
                    if (b < 4u) w0 |= v; else if (b < 8u) w1 |= v; else w2 |= v;
                }
            }
            q.a0[k] = w0; q.a1[k] = w1; q.a2[k] = w2;
            if constexpr (PIX == 1u) q.dms[k] = d | (mn << 8) | (sh << 16);
            else q.dms[k] = d | (sh << 8) | (mn << 16);
        }
        buf ^= 1u;
    };

    // ---- the counts of one group ----
    auto count = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;
            const uint32_t d = q.dms[k] & 0xFFu;
            const uint32_t mn = PIX == 1u ? (q.dms[k] >> 8) & 0xFFu : q.dms[k] >> 16;
            if (whole(d, mn)) {
                // one add per tile: the tile's window pixels (rows x columns inside the window)
                if (leader) {
                    const uint32_t nt = tx_b + 1u - m.txp[k] < kTiles ? tx_b + 1u - m.txp[k] : kTiles;
                    const int xt = 8 * (int)(m.txp[k] + t), yt = 8 * (int)m.ty[k];
                    const int cx = min(xt + 8, p.x0 + p.rw) - max(xt, p.x0), cy = min(yt + 8, p.y0 + p.rh) - max(yt, p.y0);
                    if (t < nt && cx > 0 && cy > 0) atomicAdd(hist + binof(mn), (uint32_t)(cx * cy));
                }
                continue;
            }
            const uint32_t cm = lane_mask(m.ty[k], m.txp[k]);
            if (cm == 0u) continue;
            // this lane's pixels
            uint32_t v[kNpx];
            if constexpr (PIX == 1u) {
                const uint32_t sh = q.dms[k] >> 16;
                const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh) |
                                      ((uint64_t)__builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh) << 32);
                uint32_t px[2];
                expand_row(bits, d, px[0], px[1]);
                px[0] = add_bytes(px[0], mn * 0x01010101u);
                px[1] = add_bytes(px[1], mn * 0x01010101u);
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++) v[i] = (px[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
            } else {
                const uint32_t sh = (q.dms[k] >> 8) & 0xFFu, so = 4u * hh * (d & 1u);
                const uint32_t m32 = d >= 16u ? 0xFFFFu : (1u << d) - 1u, mn2 = mn * 0x00010001u;
                const bool c2 = 2u * d >= 32u, c3 = 3u * d >= 32u;
                const uint32_t x0 = __builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh);
                const uint32_t x1 = __builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh);
                uint32_t e[2];
                cut_four16(__builtin_amdgcn_alignbit(x1, x0, so), x1 >> so, d, m32, mn2, c2, c3, e[0], e[1]);
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) v[i] = (e[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
            }
            // runs of equal bins along the row: one add each
            uint32_t b[kNpx];
#pragma unroll
            for (uint32_t i = 0; i < kNpx; i++) b[i] = binof(v[i]);
            uint32_t run = 0;
#pragma unroll
            for (uint32_t i = 0; i < kNpx; i++) {
                run += (cm >> i) & 1u;
                if (i + 1u == kNpx || b[i + 1u] != b[i]) {
                    if (run) atomicAdd(hist + b[i], run);
                    run = 0;
                }
            }
        }
    };

    // ---- the pipeline: count group k while group k + 1's payload and group k + 2's depth bytes load ----
    Meta m_cur, m_nxt, m_nn;
    Pay q_cur, q_nxt;
    uint32_t w_nn;
    issue_words(w_nn, p_begin);
    issue_meta(m_cur, w_nn, p_begin);
    issue_payload(m_cur, q_cur);
    issue_words(w_nn, p_begin + G);
    issue_meta(m_nxt, w_nn, p_begin + G);
    issue_words(w_nn, p_begin + 2u * G);
    for (uint32_t p0 = p_begin; p0 < p_end; p0 += G) {
        issue_payload(m_nxt, q_nxt);
        issue_meta(m_nn, w_nn, p0 + 2u * G);
        issue_words(w_nn, p0 + 3u * G);
        count(m_cur, q_cur);
        m_cur = m_nxt;
        q_cur = q_nxt;
        m_nxt = m_nn;
    }

    // ---- the segment's counts -> the frame's row and the total (nonzero bins only) ----
    __syncthreads();
    uint32_t *const row = p.out_hist ? p.out_hist + (size_t)g * p.bins : nullptr;
    for (uint32_t j = tid; j < p.bins; j += kHistThreads) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t c = 0; c < kCopies; c++) v += s_hist[c * NB + j];
        if (v == 0u) continue;
        if (row) atomicAdd(row + j, v);
        if (p.out_total) atomicAdd(reinterpret_cast<unsigned long long *>(p.out_total + j), (unsigned long long)v);
    }
    if (p.out_count && seg == 0u && tid == 0u) atomicAdd(reinterpret_cast<unsigned long long *>(p.out_count), 1ull);
}

// Before the histogram kernel: the accepted frames' rows to 0 and, with accumulate = 0, the total and the count to 0.
// One thread per output bin.
__global__ __launch_bounds__(kHistRowThreads) void hist_init_kernel(HistParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * kHistRowThreads + threadIdx.x;
    if (p.out_hist && i < (uint64_t)p.n_frames * p.bins && p.frame_ok[i / p.bins]) p.out_hist[i] = 0u;
    if (p.accumulate) return;
    if (p.out_total && i < p.bins) p.out_total[i] = 0ull;
    if (p.out_count && i == 0u) *p.out_count = 0ull;
}

hipError_t launch_histogram(const HistParams &p, uint32_t pix, hipStream_t s) {
    if ((pix != 1u && pix != 2u) || p.bins < 1u || p.bins > (pix == 1u ? kHistSmallBins : kHistLargeBins))
        return hipErrorInvalidValue;
    const uint64_t rows = (uint64_t)p.n_frames * p.bins > p.bins ? (uint64_t)p.n_frames * p.bins : p.bins;
    const uint32_t rgrid = (uint32_t)((rows + kHistRowThreads - 1u) / kHistRowThreads);   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(hist_init_kernel, dim3(rgrid), dim3(kHistRowThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.n_frames == 0u) return e;
    void (*k)(HistParams) = pix == 1u ? hist_kernel<1, kHistSmallBins>
                          : (p.bins <= kHistSmallBins ? hist_kernel<2, kHistSmallBins> : hist_kernel<2, kHistLargeBins>);
    const uint64_t grid = (uint64_t)p.n_frames * p.segments;
    hipLaunchKernelGGL(k, dim3((uint32_t)grid), dim3(kHistThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
