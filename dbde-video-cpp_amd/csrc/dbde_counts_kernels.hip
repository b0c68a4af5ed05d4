// dbde_counts_kernels.hip -- count projections for MI355X (gfx950, wave64): K U32 planes of the rw x rh window,
// out[k][y][x] = number of accepted frames f with p_f[y][x] <= thr_k(y, x) (unsigned compare in the pixel type),
// straight from the compressed bytes (no image is written).  DESIGN.md 4.19.
//
// counts_kernel<K, PIX>: K = 1..8 levels, PIX = 1 for DBDE frames, PIX = 2 for DBDE16 frames.  The launch shape and the
// load pipeline are project_kernel's (dbde_proj_pipeline.h), as wproject_kernel took them: one 256-lane workgroup
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

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

// Frames of [0, p.n_frames) that the index accepted -> *p.out_count (added to it when accumulating).  Whole workgroup.
__device__ void write_count(const CountsParams &p) {
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

template <uint32_t K, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void counts_kernel(CountsParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    static_assert(K >= 1u && K <= kCountsMaxLevels, "1..8 levels");
    constexpr uint32_t G = kCountsGroup, kNpx = 8u / PIX;                                   // kNpx: pixels per lane
    constexpr uint32_t kPerDw = 4u / PIX, kBits = 8u * PIX, kMask = (1u << kBits) - 1u;    // pixels per dword
    typedef typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type Px;
    typedef ProjPipeline<PIX, G, CountsParams> Pipe;
    __shared__ uint32_t s_wsum[2][G][2][kProjWaves];

    const ProjPiece<PIX> pc = proj_piece<PIX>(p);
    const uint32_t t = pc.t, r = pc.r, hh = pc.hh, seg = pc.seg, ty = pc.ty, txp = pc.txp;
    const uint32_t f_begin = seg * p.fps;
    const uint64_t f_last = (uint64_t)f_begin + p.fps;
    const uint32_t f_end = f_last < p.n_frames ? (uint32_t)f_last : p.n_frames;

    // ---- this lane's pixels in the window, the counters and the thresholds ----
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const int yy = 8 * (int)ty + (int)r;
    const int xx0 = 8 * (int)(txp + t) + 4 * (int)hh;                  // the lane's first pixel column
    const bool row_in = pc.has_tile && yy >= p.y0 && yy < p.y0 + p.rh;
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
    auto accumulate = [&](const typename Pipe::Meta &m, const typename Pipe::Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;   // rejected (or past the segment): counts nothing
            if constexpr (PIX == 1u) {   // cut_row's statements, each half tallied as it is cut: cut_row's order costs
                                         // the K >= 5 instances six more instructions
                const uint32_t d = q.dms[k] & 0xFFu, sh = q.dms[k] >> 16;
                const uint32_t mm = ((q.dms[k] >> 8) & 0xFFu) * 0x01010101u;
                const uint64_t bits = (uint64_t)__builtin_amdgcn_alignbyte(q.a1[k], q.a0[k], sh) |
                                      ((uint64_t)__builtin_amdgcn_alignbyte(q.a2[k], q.a1[k], sh) << 32);
                uint32_t px[2];
                expand_row(bits, d, px[0], px[1]);
                tally(0u, add_bytes(px[0], mm));
                tally(1u, add_bytes(px[1], mm));
            } else {
                uint32_t e[2];
                cut_row<PIX>(q.a0[k], q.a1[k], q.a2[k], q.dms[k], hh, e[0], e[1]);
                tally(0u, e[0]);
                tally(1u, e[1]);
            }
        }
    };

    // ---- the pipeline: count group k while group k + 1's payload and group k + 2's depth bytes load ----
    uint32_t buf = 0;
    Pipe pl{p, pc, s_wsum, p.stream + p.stream_bytes, buf};
    typename Pipe::Meta m_cur, m_nxt, m_nn;
    typename Pipe::Pay q_cur, q_nxt;
    typename Pipe::Words w_nn;
    pl.issue_words(w_nn, f_begin, f_end);
    pl.issue_meta(m_cur, w_nn);
    pl.issue_payload(m_cur, q_cur);
    pl.issue_words(w_nn, f_begin + G, f_end);
    pl.issue_meta(m_nxt, w_nn);
    pl.issue_words(w_nn, f_begin + 2u * G, f_end);
    for (uint32_t g0 = f_begin; g0 < f_end; g0 += G) {
        pl.issue_payload(m_nxt, q_nxt);
        pl.issue_meta(m_nn, w_nn);
        pl.issue_words(w_nn, g0 + 3u * G, f_end);
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
