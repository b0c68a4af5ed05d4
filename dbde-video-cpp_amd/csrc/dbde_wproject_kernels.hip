// dbde_wproject_kernels.hip -- weighted temporal projections for MI355X (gfx950, wave64): R F32 planes of the rw x rh
// window, out[r][y][x] = sum over the accepted frames f of w[r][f] * p_f[y][x], straight from the compressed bytes (no
// image is written).  DESIGN.md 4.17.
//
// wproject_kernel<R, PIX>: R = 1..8 regressors, PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  The launch shape
// and the load pipeline are project_kernel's (dbde_proj_pipeline.h): one 256-lane workgroup per (frame segment,
// window tile row, piece of kProjTilesOf(PIX) tiles), one lane per tile row (PIX 2: per half row), the segment's frames
// walked in groups of kWProjGroup with the payload loads of group k + 1, the depth / minimum loads of group k + 2 and
// the per-frame words of group k + 3 in flight while group k is folded in, one barrier per group.  The body is this
// file's own.
//
// The fold.  Each lane keeps acc[R][kNpx] F32 in registers, started at +0.0f.  An accepted frame folds in as
//     acc[r][i] = fmaf(w[r][f], (float)p_i, acc[r][i])
// with an explicit fused multiply-add (one rounding, whatever the contraction setting), denormals kept.  A rejected
// frame, or one past the segment, executes no FMA: its weights are loaded with the group's words but never used.
// The weights travel with the per-frame words: where lanes k < G load frame g0 + k's words, lanes r * G + k < R * G
// (at most 32) load w[r][g0 + k]; the accumulate step reads them with readlane, three groups after the load.
//
// The value.  With one segment each lane writes its window pixels of the R planes (old + acc when accumulating); with
// more, the per-segment partials [segments][R][rw * rh] go to the workspace and wproject_combine_kernel (one thread per
// window pixel, looping over r) adds them in ascending segment order onto the prior content (accumulate) or onto
// partial 0.  That order is part of the contract (include/dbde_hip.h).
#include "dbde_wproject_kernels.h"

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

// Frames of [0, p.n_frames) that the index accepted -> *p.out_count (added to it when accumulating).  Whole workgroup.
__device__ void write_count(const WProjParams &p) {
    __shared__ uint32_t s_c[kProjWaves];
    const uint32_t tid = threadIdx.x;
    uint32_t c = 0;
    for (uint32_t g = tid; g < p.n_frames; g += kProjThreads) c += p.frame_ok[g] != 0u ? 1u : 0u;
    c = wave_sum(c);
    if ((tid & 63u) == 0u) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint64_t total = 0;
        for (uint32_t k = 0; k < kProjWaves; k++) total += s_c[k];
        *p.out_count = (p.accumulate ? *p.out_count : 0ull) + total;
    }
}

}  // namespace

template <uint32_t R, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void wproject_kernel(WProjParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(R >= 1u && R <= kWProjMaxRegressors && R * kWProjGroup <= 32u, "a group's weights fit lanes 0-31");
    constexpr uint32_t G = kWProjGroup, kTiles = kProjTilesOf(PIX), kDmax = 8u * PIX, kNpx = 8u / PIX;   // kNpx: pixels per lane
    __shared__ uint32_t s_wsum[2][G][2][kProjWaves];   // per group of frames (double-buffered): wave depth totals, sums in front

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

    // ---- accumulators: this lane's kNpx pixels of each plane ----
    float acc[R][kNpx];
#pragma unroll
    for (uint32_t j = 0; j < R; j++)
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) acc[j][i] = 0.0f;

    // ---- the per-frame words of a group: lane k < G holds frame g0 + k, lane j * G + k < R * G holds w[j][g0 + k] ----
    struct Words {
        uint32_t ok, base, wt;
        uint64_t fo;
    };
    const uint32_t wk = lane & (G - 1u);
    const uint32_t *const wrow = reinterpret_cast<const uint32_t *>(p.weights) + (uint64_t)(lane < R * G ? lane / G : 0u) * p.weight_stride;
    auto issue_words = [&](Words &wd, uint32_t g0) __attribute__((always_inline)) {
        const uint32_t g = g0 + (lane < G ? lane : 0u);
        wd.ok = 0u; wd.base = 0u; wd.fo = 0u; wd.wt = 0u;
        if (lane < G && g < f_end) {
            wd.ok = p.frame_ok[g];
            wd.fo = p.frame_offsets[g];
            wd.base = p.chunk_off[(size_t)g * cstride + c];
        }
        if (lane < R * G && g0 + wk < f_end) wd.wt = wrow[g0 + wk];   // only w[j][0 .. n_frames) is ever read
    };

    // ---- one group of frames in flight ----
    struct Meta {
        uint32_t ok[G];            // uniform: frame accepted (and inside the segment)
        uint32_t base[G];          // uniform: payload words of the frame in front of the piece's chunk
        const uint8_t *fb[G];      // uniform: the frame
        uint32_t d8[G], ml[G], mh[G];   // depth, minimum (PIX 2: its low / high byte) of this lane's tile (raw loads)
        uint32_t pre[G];           // this lane's dword of the depth bytes in front of the piece (masked where used)
        uint32_t wt;               // the group's weights, as the words hold them (lane j * G + k)
    };
    struct Pay {
        uint32_t a0[G], a1[G], a2[G];   // the aligned dwords around this lane's (half) row
        uint32_t dms[G];                // PIX 1: depth | minimum << 8 | byte shift << 16; PIX 2: depth | shift << 8 | minimum << 16
    };

    // pre: depth bytes [cb, pos0) of the frame, as aligned dwords, lane tid < ndw holding dword tid.  Every load is
    // unconditional inside an accepted frame (lanes without a tile read tile 0, lanes past ndw dword 0) and nothing
    // consumes a loaded value here, so that the loads stay in flight while the group in front is accumulated.
    // The U16 minima start at 28 + T, possibly at an odd address: read byte by byte.
    auto issue_meta = [&](Meta &m, const Words &wd) __attribute__((always_inline)) {
        m.wt = wd.wt;
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
            const uint32_t pw = wave_sum(__builtin_amdgcn_sad_u8(m.pre[k] & pre_keep(m.fb[k], cb, npre, tid), 0u, 0u));
            if (lane == 63u) s_wsum[buf][k][0][wave] = incl[k];
            if (lane == 0u) s_wsum[buf][k][1][wave] = pw;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            uint32_t wbase = 0, PRE = 0;
#pragma unroll
            for (uint32_t w = 0; w < kProjWaves; w++) {
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

    // acc[j][i] = fmaf(w[j][frame k of the group], pixel i, acc[j][i]); the weight is uniform (a readlane of m.wt)
    auto fold = [&](const Meta &m, uint32_t k, uint32_t i, uint32_t v) __attribute__((always_inline)) {
        const float pf = (float)v;   // exact: v < 2^16
#pragma unroll
        for (uint32_t j = 0; j < R; j++)
            acc[j][i] = __builtin_fmaf(__uint_as_float(readlane(m.wt, j * G + k)), pf, acc[j][i]);
    };
    auto accumulate = [&](const Meta &m, const Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;   // rejected (or past the segment): no FMA, its weights stay unused
            uint32_t px[2];
            cut_row<PIX>(q.a0[k], q.a1[k], q.a2[k], q.dms[k], hh, px[0], px[1]);
            if constexpr (PIX == 1u) {
#pragma unroll
                for (uint32_t h = 0; h < 2; h++)
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++) fold(m, k, 4u * h + i, (px[h] >> (8u * i)) & 0xFFu);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 2; j++)
#pragma unroll
                    for (uint32_t i = 0; i < 2; i++) fold(m, k, 2u * j + i, (px[j] >> (16u * i)) & 0xFFFFu);
            }
        }
    };

    // ---- the pipeline: accumulate group k while group k + 1's payload and group k + 2's depth bytes load ----
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
    const int yy = 8 * (int)ty + (int)r;
    if (has_tile && yy >= p.y0 && yy < p.y0 + p.rh) {
        const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
        const uint64_t row0 = (uint64_t)(yy - p.y0) * (uint64_t)p.rw;
        const bool direct = p.segments == 1u;
        float *const dst = direct ? p.out : p.ws + (uint64_t)seg * R * P;
#pragma unroll
        for (uint32_t i = 0; i < kNpx; i++) {
            const int xx = 8 * (int)(txp + t) + 4 * (int)hh + (int)i;
            if (xx < p.x0 || xx >= p.x0 + p.rw) continue;
            const uint64_t o = row0 + (uint64_t)(xx - p.x0);
#pragma unroll
            for (uint32_t j = 0; j < R; j++) {
                float *const q = dst + (uint64_t)j * P + o;
                *q = direct && p.accumulate ? *q + acc[j][i] : acc[j][i];
            }
        }
    }
    if (p.segments == 1u && blockIdx.x == 0u) write_count(p);
}

// Segments > 1: prior (ACC: what the planes hold) + partial 0 + partial 1 + ... in ascending segment order, one F32
// round-to-nearest-even addition each.  One thread per window pixel, looping over the regressors; the partials are
// [segments][R][rw * rh], so each read is coalesced.
template <bool ACC>
__global__ __launch_bounds__(kProjCombineThreads) void wproject_combine_kernel(WProjParams p) {
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint64_t i = (uint64_t)blockIdx.x * kProjCombineThreads + threadIdx.x;
    if (i < P) {
        const uint64_t RP = (uint64_t)p.regressors * P;
        for (uint32_t j = 0; j < p.regressors; j++) {
            const float *const ws = p.ws + (uint64_t)j * P + i;
            float *const out = p.out + (uint64_t)j * P + i;
            float v = ACC ? *out : ws[0];
            for (uint32_t s = ACC ? 0u : 1u; s < p.segments; s++) v = v + ws[(uint64_t)s * RP];
            *out = v;
        }
    }
    if (blockIdx.x == 0u) write_count(p);
}

uint64_t wproject_workspace_bytes(uint32_t regressors, uint32_t segments, uint64_t pixels) {
    if (segments <= 1u) return 0;
    return (4ull * segments * regressors * pixels + 15u) & ~(uint64_t)15;
}

typedef void (*WProjKernel)(WProjParams);

hipError_t launch_wproject(const WProjParams &p, uint32_t regressors, uint32_t pix, hipStream_t s) {
    static const WProjKernel table[2][kWProjMaxRegressors] = {
        {wproject_kernel<1, 1>, wproject_kernel<2, 1>, wproject_kernel<3, 1>, wproject_kernel<4, 1>,
         wproject_kernel<5, 1>, wproject_kernel<6, 1>, wproject_kernel<7, 1>, wproject_kernel<8, 1>},
        {wproject_kernel<1, 2>, wproject_kernel<2, 2>, wproject_kernel<3, 2>, wproject_kernel<4, 2>,
         wproject_kernel<5, 2>, wproject_kernel<6, 2>, wproject_kernel<7, 2>, wproject_kernel<8, 2>}};
    if (regressors < 1u || regressors > kWProjMaxRegressors || regressors != p.regressors || (pix != 1u && pix != 2u))
        return hipErrorInvalidValue;
    const uint32_t grid = p.pieces * p.rows * p.segments;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(table[pix - 1u][regressors - 1u], dim3(grid), dim3(kProjThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.segments == 1u) return e;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint32_t cgrid = (uint32_t)((P + kProjCombineThreads - 1u) / kProjCombineThreads);
    const WProjKernel combine = p.accumulate ? wproject_combine_kernel<true> : wproject_combine_kernel<false>;
    hipLaunchKernelGGL(combine, dim3(cgrid), dim3(kProjCombineThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
