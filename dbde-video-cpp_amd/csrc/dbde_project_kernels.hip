// dbde_project_kernels.hip -- temporal projections for MI355X (gfx950, wave64): per-pixel maximum, minimum, sum and sum
// of squares of the rw x rh window over a batch of frames, straight from the compressed bytes (no image is written).
//
// What a frame's window needs is what the window decoder reads (dbde_roi_kernels.hip): the depth and minimum bytes of
// the window's tiles, the depth bytes in front of each window tile row's first tile within its chunk (fewer than 512:
// roi_index_geometry), the chunk's payload offset from the decode index kernel, and the window tiles' payload.
//
// project_kernel<STATS, PIX>: PIX = 1 for DBDE frames (U8 pixels and minima, depth 0..8, payload at 32 + 2T), PIX = 2
// for DBDE16 frames (U16 pixels and minima, depth 0..16, payload at 32 + 3T).  One workgroup per (frame segment, window
// tile row, piece of kProjTilesOf(PIX) tiles); 256 lanes, 8 * PIX lanes per tile:
//   PIX = 1  one lane per tile row.  Row r of a depth-d tile is bytes [r*d, r*d + d) of the tile's payload, at most 8
//            bytes; the lane loads the three aligned dwords around it straight from global memory and cuts its 8 pixels
//            with dbde_bits.h's expand_row / add_bytes.
//   PIX = 2  one lane per HALF tile row (lanes 2r and 2r + 1 of a tile).  Half h of row r is the 32d-bit integer at bit
//            (8r + 4h) * d of the tile's payload: at most 8 bytes plus a nibble, so the lane loads the same three dwords
//            and cuts its 4 pixels with dbde_device.h's cut_four16 (cut_row16's step).
// The pixels fold into register accumulators:
//   max / min  packed U16 pairs (v_pk_max_u16 / v_pk_min_u16).  PIX = 1: even bytes masked into 16-bit lanes, odd bytes
//              compared through the high byte of each 16-bit lane (3 operations per statistic per 4 pixels, as
//              tile_minmax);
//   sum        one U32 per pixel: exact for kProjMaxFramesPerSegment = 65,536 frames (65,536 * 65,535 < 2^32);
//   sumsq      PIX = 1: one U32 per pixel, exact for the same bound (65,536 * 255^2 < 2^32); PIX = 2: one U64 per pixel
//              (one square alone can fill a U32), a 32-bit add with carry per frame.
// STATS is a template parameter: an unrequested statistic has no accumulator and no instruction.
// The workgroup walks its segment's frames in groups of kProjGroup.  While group k is accumulated, the payload loads of
// group k + 1, the depth / minimum loads of group k + 2 and the per-frame words (frame_ok, offset, chunk offset) of
// group k + 3 are in flight (one barrier per group, for the offsets scan).
// At the end each lane writes its window pixels: into the outputs when the launch has one segment, else into the
// per-segment partials, which project_combine_kernel<PIX> (one thread per window pixel) folds into the outputs.
// The __global__ template is the body itself, with the pixel size's differences behind `if constexpr`: every instance
// compiles to the instructions the two kernels had as separate bodies.
#include "dbde_project_kernels.h"

#include <type_traits>
#include <utility>

#include "dbde_proj_pipeline.h"

namespace dbde {

namespace {

constexpr uint32_t kProjGroup = 4;                 // frames per pipeline step

// What the outputs and partials hold: U8 (PIX 1) or U16 (PIX 2) max / min, U32 or U64 partial sums of squares.
template <uint32_t PIX> using ProjPix = typename std::conditional<PIX == 1u, uint8_t, uint16_t>::type;
template <uint32_t PIX> using ProjSq = typename std::conditional<PIX == 1u, uint32_t, uint64_t>::type;

// Frames of [0, p.n_frames) that the index accepted -> *p.out_count (added to it when accumulating).  Whole workgroup.
__device__ void write_count(const ProjParams &p) {
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

template <uint32_t STATS, uint32_t PIX>
__global__ __launch_bounds__(kProjThreads) void project_kernel(ProjParams p) {
    static_assert(PIX == 1u || PIX == 2u, "U8 or U16 pixels");
    typedef ProjPix<PIX> Pix;
    constexpr bool kMax = (STATS & kProjMax) != 0u, kMin = (STATS & kProjMin) != 0u;
    constexpr bool kSum = (STATS & kProjSum) != 0u, kSq = (STATS & kProjSumSq) != 0u;
    constexpr uint32_t G = kProjGroup, kNpx = 8u / PIX;   // kNpx: pixels per lane
    constexpr uint32_t kPixMask = PIX == 1u ? 0xFFu : 0xFFFFu;
    typedef ProjPipeline<PIX, G, ProjParams> Pipe;
    __shared__ uint32_t s_wsum[2][G][2][kProjWaves];

    const ProjPiece<PIX> pc = proj_piece<PIX>(p);
    const uint32_t t = pc.t, r = pc.r, hh = pc.hh, seg = pc.seg, ty = pc.ty, txp = pc.txp;
    const uint32_t f_begin = seg * p.fps;
    const uint64_t f_last = (uint64_t)f_begin + p.fps;
    const uint32_t f_end = f_last < p.n_frames ? (uint32_t)f_last : p.n_frames;

    // ---- accumulators: this lane's kNpx pixels ----
    // max / min: PIX 1 even bytes (mx, mn) and odd bytes (mxo, mno) of pixels 0-3, 4-7; PIX 2 U16 pairs (mx, mn)
    uint32_t mx[2] = {0u, 0u}, mxo[2] = {0u, 0u};
    uint32_t mn[2] = {~0u, ~0u}, mno[2] = {~0u, ~0u};
    uint32_t sum[kNpx] = {};
    ProjSq<PIX> sq[kNpx] = {};

    auto accumulate = [&](const typename Pipe::Meta &m, const typename Pipe::Pay &q) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            if (!m.ok[k]) continue;   // rejected (or past the segment): contributes nothing
            uint32_t px[2];
            cut_row<PIX>(q.a0[k], q.a1[k], q.a2[k], q.dms[k], hh, px[0], px[1]);
            if constexpr (PIX == 1u) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t e = px[h] & 0x00FF00FFu;
                    if (kMax) { mx[h] = pk_max_u16(mx[h], e); mxo[h] = pk_max_u16(mxo[h], px[h]); }
                    if (kMin) { mn[h] = pk_min_u16(mn[h], e); mno[h] = pk_min_u16(mno[h], px[h]); }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t v = (px[h] >> (8 * i)) & 0xFFu;
                        if (kSum) sum[4 * h + i] += v;
                        if (kSq) sq[4 * h + i] += v * v;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    if (kMax) mx[j] = pk_max_u16(mx[j], px[j]);
                    if (kMin) mn[j] = pk_min_u16(mn[j], px[j]);
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const uint32_t v = (px[j] >> (16 * i)) & 0xFFFFu;
                        if (kSum) sum[2 * j + i] += v;
                        if (kSq) sq[2 * j + i] += (uint64_t)(v * v);   // v * v < 2^32; the add carries into the high dword
                    }
                }
            }
        }
    };

    // ---- the pipeline: accumulate group k while group k + 1's payload and group k + 2's depth bytes load ----
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

    // ---- the window's pixels of this lane -> the outputs, or this segment's partials ----
    Pix *const out_max = reinterpret_cast<Pix *>(p.out_max), *const out_min = reinterpret_cast<Pix *>(p.out_min);
    const int yy = 8 * (int)ty + (int)r;
    if (pc.has_tile && yy >= p.y0 && yy < p.y0 + p.rh) {
        const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
        const uint64_t row0 = (uint64_t)(yy - p.y0) * (uint64_t)p.rw;
        const bool direct = p.segments == 1u;
#pragma unroll
        for (int i = 0; i < (int)kNpx; i++) {
            const int xx = 8 * (int)(txp + t) + 4 * (int)hh + i;
            if (xx < p.x0 || xx >= p.x0 + p.rw) continue;
            const uint64_t o = row0 + (uint64_t)(xx - p.x0);
            // the partials' index: PIX 2 forms it once, PIX 1 at each store (listing of the separate bodies)
            const uint64_t ow = (uint64_t)seg * P + o;
            // pixel i of a packed max / min: PIX 1 byte i & 3 of the even / odd accumulator, PIX 2 U16 i & 1 of a pair
            const int h = PIX == 1u ? i >> 2 : i >> 1, sb = PIX == 1u ? 8 * (i & 3) : 16 * (i & 1);
            if (kMax) {
                uint32_t v = ((PIX == 1u && (i & 1)) ? mxo[h] : mx[h]) >> sb & kPixMask;
                if (direct) {
                    if (p.accumulate) { const uint32_t ov = out_max[o]; v = v > ov ? v : ov; }
                    out_max[o] = (Pix)v;
                } else {
                    reinterpret_cast<Pix *>(p.ws_max)[PIX == 1u ? (uint64_t)seg * P + o : ow] = (Pix)v;
                }
            }
            if (kMin) {
                uint32_t v = ((PIX == 1u && (i & 1)) ? mno[h] : mn[h]) >> sb & kPixMask;
                if (direct) {
                    if (p.accumulate) { const uint32_t ov = out_min[o]; v = v < ov ? v : ov; }
                    out_min[o] = (Pix)v;
                } else {
                    reinterpret_cast<Pix *>(p.ws_min)[PIX == 1u ? (uint64_t)seg * P + o : ow] = (Pix)v;
                }
            }
            if (kSum) {
                if (direct) p.out_sum[o] = (p.accumulate ? p.out_sum[o] : 0ull) + sum[i];
                else p.ws_sum[PIX == 1u ? (uint64_t)seg * P + o : ow] = sum[i];
            }
            if (kSq) {
                if (direct) p.out_sumsq[o] = (p.accumulate ? p.out_sumsq[o] : 0ull) + sq[i];
                else reinterpret_cast<ProjSq<PIX> *>(p.ws_sumsq)[PIX == 1u ? (uint64_t)seg * P + o : ow] = sq[i];
            }
        }
    }
    if (p.segments == 1u && blockIdx.x == 0u) write_count(p);
}

// Segments > 1: the partials of every segment (and the outputs' values when accumulating) -> the outputs.  One thread
// per window pixel; the partials are [segments][rw * rh], so each segment's read is coalesced.
template <uint32_t PIX>
__global__ __launch_bounds__(kProjCombineThreads) void project_combine_kernel(ProjParams p) {
    typedef ProjPix<PIX> Pix;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint64_t i = (uint64_t)blockIdx.x * kProjCombineThreads + threadIdx.x;
    if (i < P) {
        if (p.out_max) {
            Pix *const out = reinterpret_cast<Pix *>(p.out_max);
            const Pix *const ws = reinterpret_cast<const Pix *>(p.ws_max);
            uint32_t v = p.accumulate ? out[i] : 0u;
            for (uint32_t s = 0; s < p.segments; s++) { const uint32_t w = ws[(uint64_t)s * P + i]; v = w > v ? w : v; }
            out[i] = (Pix)v;
        }
        if (p.out_min) {
            Pix *const out = reinterpret_cast<Pix *>(p.out_min);
            const Pix *const ws = reinterpret_cast<const Pix *>(p.ws_min);
            uint32_t v = p.accumulate ? out[i] : (PIX == 1u ? 255u : 65535u);
            for (uint32_t s = 0; s < p.segments; s++) { const uint32_t w = ws[(uint64_t)s * P + i]; v = w < v ? w : v; }
            out[i] = (Pix)v;
        }
        if (p.out_sum) {
            uint64_t v = p.accumulate ? p.out_sum[i] : 0ull;
            for (uint32_t s = 0; s < p.segments; s++) v += p.ws_sum[(uint64_t)s * P + i];
            p.out_sum[i] = v;
        }
        if (p.out_sumsq) {
            const ProjSq<PIX> *const ws = reinterpret_cast<const ProjSq<PIX> *>(p.ws_sumsq);
            uint64_t v = p.accumulate ? p.out_sumsq[i] : 0ull;
            for (uint32_t s = 0; s < p.segments; s++) v += ws[(uint64_t)s * P + i];
            p.out_sumsq[i] = v;
        }
    }
    if (blockIdx.x == 0u) write_count(p);
}

uint64_t project_partial_bytes(uint32_t bit, uint32_t segments, uint64_t pixels, uint32_t pix) {
    if (segments <= 1u) return 0;
    const uint64_t n = (uint64_t)segments * pixels;
    const uint64_t width = bit == kProjSum ? 4u : bit == kProjSumSq ? 4u * pix : pix;   // DBDE16: U64 sums of squares
    return (width * n + 15u) & ~(uint64_t)15;
}

uint64_t project_workspace_bytes(uint32_t stats, uint32_t segments, uint64_t pixels, uint32_t pix) {
    uint64_t total = 0;
    for (uint32_t bit = 1u; bit <= kProjSumSq; bit <<= 1)
        if (stats & bit) total += project_partial_bytes(bit, segments, pixels, pix);
    return total;
}

typedef void (*ProjKernel)(ProjParams);
struct ProjTable {
    ProjKernel k[16];   // [stats]: project_kernel<stats, PIX>, 1..15
};

template <uint32_t PIX, uint32_t... S>
static constexpr ProjTable proj_table(std::integer_sequence<uint32_t, S...>) {
    return {{nullptr, project_kernel<S + 1u, PIX>...}};
}

hipError_t launch_project(const ProjParams &p, uint32_t stats, uint32_t pix, hipStream_t s) {
    static const ProjTable tables[2] = {proj_table<1>(std::make_integer_sequence<uint32_t, 15>()),
                                        proj_table<2>(std::make_integer_sequence<uint32_t, 15>())};
    if (stats < 1u || stats > kProjAll || (pix != 1u && pix != 2u)) return hipErrorInvalidValue;
    const uint32_t grid = p.pieces * p.rows * p.segments;   // (the host keeps it below 2^31)
    hipLaunchKernelGGL(tables[pix - 1u].k[stats], dim3(grid), dim3(kProjThreads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.segments == 1u) return e;
    return launch_project_combine(p, pix, s);
}

hipError_t launch_project_combine(const ProjParams &p, uint32_t pix, hipStream_t s) {
    if (pix != 1u && pix != 2u) return hipErrorInvalidValue;
    const uint64_t P = (uint64_t)p.rw * (uint64_t)p.rh;
    const uint32_t cgrid = (uint32_t)((P + kProjCombineThreads - 1u) / kProjCombineThreads);
    const ProjKernel combine = pix == 1u ? project_combine_kernel<1> : project_combine_kernel<2>;
    hipLaunchKernelGGL(combine, dim3(cgrid), dim3(kProjCombineThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace dbde
