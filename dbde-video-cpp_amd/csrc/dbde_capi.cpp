// dbde_capi.cpp -- implementation of include/dbde_hip.h (the C-ABI of libdbde_hip.so).
//
// Host side only: argument checking, workspace, launches, and the byte marshalling the
// host-pointer entry points need.  All tile arithmetic is in dbde_kernels.hip; nothing here
// (or anywhere in this library) computes DBDE on the CPU.
#include "../../include/dbde_hip.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dbde16_kernels.h"
#include "dbde_binned_kernels.h"
#include "dbde_counts_kernels.h"
#include "dbde_lag_kernels.h"
#include "dbde_pairs_kernels.h"
#include "dbde_crop_kernels.h"
#include "dbde_gproject_kernels.h"
#include "dbde_hist_kernels.h"
#include "dbde_kernels.h"
#include "dbde_mask_kernels.h"
#include "dbde_match_kernels.h"
#include "dbde_moment_kernels.h"
#include "dbde_patch_kernels.h"
#include "dbde_project_kernels.h"
#include "dbde_roi_kernels.h"
#include "dbde_rproject_kernels.h"
#include "dbde_scaled_kernels.h"
#include "dbde_trace_kernels.h"
#include "dbde_wenc_kernels.h"
#include "dbde_wproject_kernels.h"

using namespace dbde;

namespace {

struct TimedSpan {
    hipEvent_t a, b;
    int kind;
};

struct Geometry {
    uint32_t w, h, T;
    uint64_t pixels;
};

}  // namespace

struct dbde_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;         // dbde_hip_create_on_own_stream: destroyed with the context
    std::string err;
    std::string arch;

    // look-back workspace: [two sets of control words: 2 x 8 x u32][state: n_chunks x u64].  Zeroed when it is allocated
    // and after a failed launch; otherwise every launch leaves it as it found it (persistent encoder: each record is
    // cleared by its reader, the scanner clears the control words of the launch after it; small launches tag theirs)
    uint8_t *lb = nullptr;
    size_t lb_bytes = 0;
    uint32_t enc_parity = 0;         // which set of control words the next persistent launch uses
    // scan-ahead: a second stream so that the frame-to-frame walk of the NEXT batch runs beside the decode of this one
    hipStream_t scan_stream = nullptr;
    hipEvent_t scan_ev_main = nullptr, scan_ev_done = nullptr;
    // speculative stream walk: temporary position lists of the segments
    uint8_t *scan_ws = nullptr;
    size_t scan_ws_bytes = 0;
    // DBDE16 encode workspace (per-tile depth / minimum, chunk and frame totals, frame bases, arrival counter)
    uint8_t *w16 = nullptr;
    size_t w16_bytes = 0;
    bool lb_fresh = true;            // the block holds arbitrary bits (fresh allocation): a small launch zeroes it before its first use
    uint32_t enc_epoch = 0;          // tag of the last small encode launch's records (launch_encode_small)
    // decode workspace
    uint32_t *chunk_off = nullptr;
    size_t chunk_off_n = 0;
    uint32_t *frame_ok = nullptr;
    size_t frame_ok_n = 0;
    uint32_t *idx_ctr = nullptr;     // [2 * n]: arrival counters, then flags, of the split index kernel (kept zero)
    size_t idx_ctr_n = 0;
    unsigned long long *fuse_rec = nullptr;   // records of the fused index + decode launch (epoch-tagged, never cleared)
    uint8_t *proj_ws = nullptr;      // per-segment partials of dbde_hip_project
    size_t proj_ws_bytes = 0;
    uint8_t *trace_ws = nullptr;     // U32 max / min per (frame, label) of dbde_hip_traces
    size_t trace_ws_bytes = 0;
    uint8_t *crop_ws = nullptr;      // row and frame tables, records of re-packed tiles of dbde_hip_crop_frames
    size_t crop_ws_bytes = 0;
    size_t fuse_rec_n = 0;
    uint32_t fuse_epoch = 0;
    // sticky failure word (device) + scratch
    uint32_t *sticky = nullptr;
    uint64_t *scratch64 = nullptr;   // small device scratch: [0..3]
    // staging for the host-pointer entry points
    uint8_t *st_img = nullptr;
    size_t st_img_bytes = 0;
    uint8_t *st_pack = nullptr;
    size_t st_pack_bytes = 0;
    // ... and their pinned host twins (dbde_hip_set_host_staging): the caller's pageable bytes are copied through these
    // by the calling thread, so that the DMA never has to pin (and the runtime's pinning of pageable memory, which
    // serialises concurrent callers, is out of the way)
    uint64_t *h_words = nullptr;     // pinned, device-visible: [0] the encoder's byte count, [1..4] the decoder's frame result -- the kernels write them
                                     // straight into host memory, so a call has no small copies between its two big ones
    uint8_t *d_hdr = nullptr;        // a frame header {2, 0, 0} in device memory (dbde_hip_unpack_image puts it in front of the caller's frame data)
    int host_staging = 0;
    uint8_t *h_img = nullptr;
    size_t h_img_bytes = 0;
    uint8_t *h_pack = nullptr;
    size_t h_pack_bytes = 0;
    // timing
    uint32_t exp_flags = 0;          // $DBDE_HIP_EXPERIMENT (tuning experiments only)
    uint32_t enc_grid = 0;           // resident workgroups for the persistent encoder
    uint32_t enc16_grid = 0;         // the same for the DBDE16 encoder (queried at its first call)
    uint32_t wenc_grid[2] = {0, 0};  // the same for the window encoder, DBDE and DBDE16
    int n_cu = 0;
    int mid_dec_per_cu[2][3] = {};   // resident workgroups per CU of decode_mid_kernel (decode_mid_blocks_per_cu)
    uint64_t *diag = nullptr;        // [16] phase cycle sums of diagnostic launches
    bool timing = false;
    std::vector<TimedSpan> spans;
    double acc_ms[4] = {0, 0, 0, 0};     // encode, decode index, decode, stream scan
    uint64_t acc_n[4] = {0, 0, 0, 0};
};

namespace {

int fail(dbde_hip_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, DBDE_HIP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

bool geometry(int W, int H, Geometry &g) {
    if (W <= 0 || H <= 0) return false;
    uint64_t w = ((uint64_t)W + 7) / 8, h = ((uint64_t)H + 7) / 8;
    uint64_t T = w * h;
    if (T >= (1ull << 27)) return false;   // in-frame payload words must stay below 2^30
    g.w = (uint32_t)w;
    g.h = (uint32_t)h;
    g.T = (uint32_t)T;
    g.pixels = (uint64_t)W * (uint64_t)H;
    return true;
}

template <typename Ptr>
int grow(dbde_hip_ctx *ctx, Ptr &p, size_t &have, size_t want_elems, size_t elem_bytes, bool uncached = false) {
    if (want_elems <= have) return DBDE_HIP_OK;
    // everything queued may still be using the old block
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p) HIP_TRY(ctx, hipFree(p));
    p = nullptr;
    have = 0;
    size_t n = want_elems + want_elems / 4 + 64;
    void *q = nullptr;
    // chunk records are written by one CU and polled by others through sc1 atomics: keeping them out
    // of the (per-XCD, mutually incoherent) L2s measured 1.5-2.5 % faster; plain memory if refused
    if (uncached && hipExtMallocWithFlags(&q, n * elem_bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        q = nullptr;
    }
    if (!q) HIP_TRY(ctx, hipMalloc(&q, n * elem_bytes));
    p = reinterpret_cast<Ptr>(q);
    have = n;
    return DBDE_HIP_OK;
}

void span_begin(dbde_hip_ctx *ctx, int kind) {
    if (!ctx->timing) return;
    TimedSpan s;
    s.kind = kind;
    if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
    (void)hipEventRecord(s.a, ctx->stream);
    ctx->spans.push_back(s);
}
void span_end(dbde_hip_ctx *ctx) {
    if (!ctx->timing || ctx->spans.empty()) return;
    (void)hipEventRecord(ctx->spans.back().b, ctx->stream);
}

void put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
void put64(uint8_t *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
uint32_t get32(const uint8_t *p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
uint64_t get64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

int grow_pinned(dbde_hip_ctx *ctx, uint8_t *&p, size_t &have, size_t want) {
    if (want <= have) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p) HIP_TRY(ctx, hipHostFree(p));
    p = nullptr;
    have = 0;
    void *q = nullptr;
    HIP_TRY(ctx, hipHostMalloc(&q, want + want / 4 + 64, hipHostMallocDefault));
    p = reinterpret_cast<uint8_t *>(q);
    have = want + want / 4 + 64;
    return DBDE_HIP_OK;
}

int ensure_staging(dbde_hip_ctx *ctx, size_t img_bytes, size_t pack_bytes) {
    if (!ctx->h_words) {
        void *q = nullptr;
        HIP_TRY(ctx, hipHostMalloc(&q, 64, hipHostMallocDefault));
        ctx->h_words = reinterpret_cast<uint64_t *>(q);
        memset(ctx->h_words, 0, 64);
        HIP_TRY(ctx, hipMalloc(&q, 32));
        ctx->d_hdr = reinterpret_cast<uint8_t *>(q);
        uint8_t hdr[20];
        const dbde_hip_frame_header fh = {2, 0, 0};
        dbde_hip_pack_frame_header(&fh, hdr);
        HIP_TRY(ctx, hipMemcpy(ctx->d_hdr, hdr, 20, hipMemcpyHostToDevice));   // (once per context)
    }
    int rc = grow(ctx, ctx->st_img, ctx->st_img_bytes, img_bytes + 64, 1);
    if (rc) return rc;
    rc = grow(ctx, ctx->st_pack, ctx->st_pack_bytes, pack_bytes + 64, 1);
    if (rc || !ctx->host_staging) return rc;
    rc = grow_pinned(ctx, ctx->h_img, ctx->h_img_bytes, img_bytes + 64);
    if (rc) return rc;
    return grow_pinned(ctx, ctx->h_pack, ctx->h_pack_bytes, pack_bytes + 64);
}

// Host -> device / device -> host of the host-pointer entry points: straight from / to the caller's (pageable) memory, or
// through the context's pinned twin (host_staging).  `via`: the pinned buffer that shadows the device buffer.
bool h2d(dbde_hip_ctx *ctx, void *d_dst, const void *src, size_t n, uint8_t *via) {
    if (ctx->host_staging && via) { memcpy(via, src, n); src = via; }
    return hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
}

}  // namespace

extern "C" {

// ---- context ---------------------------------------------------------------------------------

int dbde_hip_create(int device, void *stream, dbde_hip_ctx **out) {
    if (!out) return DBDE_HIP_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return DBDE_HIP_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return DBDE_HIP_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DBDE_HIP_ERR_HIP;
    // kernels are built for gfx950 only; refuse anything else instead of failing at launch
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DBDE_HIP_ERR_HIP;
    dbde_hip_ctx *ctx = new dbde_hip_ctx;
    ctx->device = device;
    ctx->stream = reinterpret_cast<hipStream_t>(stream);
    ctx->arch = prop.gcnArchName;
    {
        int per_cu = encode_blocks_per_cu();
        if (const char *g = getenv("DBDE_HIP_ENC_BLOCKS_PER_CU")) per_cu = atoi(g) > 0 ? atoi(g) : per_cu;
        ctx->enc_grid = (uint32_t)(per_cu * prop.multiProcessorCount);
        if (ctx->enc_grid > kEncMaxGrid) ctx->enc_grid = kEncMaxGrid;   // one mode flag per workgroup (attach_lookback)
        ctx->n_cu = prop.multiProcessorCount;
        decode_mid_blocks_per_cu(ctx->mid_dec_per_cu);
    }
    if (const char *e = getenv("DBDE_HIP_EXPERIMENT")) ctx->exp_flags = (uint32_t)strtoul(e, nullptr, 0);
    void *p = nullptr;
#ifdef DBDE_DIAG
    const size_t small_block = 64 + 128 + 8 * 16 * 1024;   // + per-workgroup timeline of the persistent encoder ([1024][16] u64)
#else
    const size_t small_block = 64 + 128;
#endif
    if (hipMalloc(&p, small_block) != hipSuccess) { delete ctx; return DBDE_HIP_ERR_HIP; }
    ctx->sticky = reinterpret_cast<uint32_t *>(p);
    ctx->scratch64 = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(p) + 16);
    ctx->diag = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(p) + 64);
    if (hipMemsetAsync(p, 0, small_block, ctx->stream) != hipSuccess) { (void)hipFree(p); delete ctx; return DBDE_HIP_ERR_HIP; }
    *out = ctx;
    return DBDE_HIP_OK;
}

int dbde_hip_create_on_own_stream(int device, dbde_hip_ctx **out) {
    if (!out) return DBDE_HIP_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return DBDE_HIP_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return DBDE_HIP_ERR_HIP;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return DBDE_HIP_ERR_HIP;
    const int rc = dbde_hip_create(device, s, out);
    if (rc != DBDE_HIP_OK) { (void)hipStreamDestroy(s); return rc; }
    (*out)->own_stream = true;
    return DBDE_HIP_OK;
}

void dbde_hip_destroy(dbde_hip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &s : ctx->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    if (ctx->scan_stream) { (void)hipStreamSynchronize(ctx->scan_stream); (void)hipStreamDestroy(ctx->scan_stream); }
    if (ctx->scan_ev_main) (void)hipEventDestroy(ctx->scan_ev_main);
    if (ctx->scan_ev_done) (void)hipEventDestroy(ctx->scan_ev_done);
    if (ctx->scan_ws) (void)hipFree(ctx->scan_ws);
    if (ctx->w16) (void)hipFree(ctx->w16);
    if (ctx->lb) (void)hipFree(ctx->lb);
    if (ctx->chunk_off) (void)hipFree(ctx->chunk_off);
    if (ctx->frame_ok) (void)hipFree(ctx->frame_ok);
    if (ctx->idx_ctr) (void)hipFree(ctx->idx_ctr);
    if (ctx->fuse_rec) (void)hipFree(ctx->fuse_rec);
    if (ctx->proj_ws) (void)hipFree(ctx->proj_ws);
    if (ctx->trace_ws) (void)hipFree(ctx->trace_ws);
    if (ctx->crop_ws) (void)hipFree(ctx->crop_ws);
    if (ctx->sticky) (void)hipFree(ctx->sticky);
    if (ctx->st_img) (void)hipFree(ctx->st_img);
    if (ctx->st_pack) (void)hipFree(ctx->st_pack);
    if (ctx->h_words) (void)hipHostFree(ctx->h_words);
    if (ctx->d_hdr) (void)hipFree(ctx->d_hdr);
    if (ctx->h_img) (void)hipHostFree(ctx->h_img);
    if (ctx->h_pack) (void)hipHostFree(ctx->h_pack);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int dbde_hip_sync(dbde_hip_ctx *ctx) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, ctx->sticky, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) {
        ctx->lb_fresh = true;   // the failed launch left its records behind: the next encode clears the workspace first
        HIP_TRY(ctx, hipMemsetAsync(ctx->sticky, 0, 4, ctx->stream));
        return fail(ctx, DBDE_HIP_ERR_DEVICE, "encode kernel: chunk look-back timed out");
    }
    return DBDE_HIP_OK;
}

int dbde_hip_set_host_staging(dbde_hip_ctx *ctx, int pinned) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    ctx->host_staging = pinned ? 1 : 0;
    return DBDE_HIP_OK;
}

const char *dbde_hip_last_error(const dbde_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
const char *dbde_hip_device_arch(const dbde_hip_ctx *ctx) { return ctx ? ctx->arch.c_str() : ""; }
void *dbde_hip_stream_handle(const dbde_hip_ctx *ctx) { return ctx ? reinterpret_cast<void *>(ctx->stream) : nullptr; }
int dbde_hip_device_index(const dbde_hip_ctx *ctx) { return ctx ? ctx->device : -1; }

// ---- sizes -----------------------------------------------------------------------------------

size_t dbde_hip_max_frame_bytes(int W, int H) {
    Geometry g;
    if (!geometry(W, H, g)) return 0;
    return 20 + 12 + 66 * (size_t)g.T;
}

size_t dbde_hip_image_bytes(int W, int H, uint64_t n64) {
    Geometry g;
    if (!geometry(W, H, g)) return 0;
    return 12 + 2 * (size_t)g.T + 8 * (size_t)n64;
}

// What every launch of the persistent / small / tiny encoders is told about the batch (`pix` bytes per pixel: 1 = DBDE,
// 2 = DBDE16 through the same kernel; ctrl / state are attached by the caller once the workspace is known).
static EncParams enc_params(dbde_hip_ctx *ctx, const Geometry &g, int W, int H, int n_frames, uint32_t pix, uint32_t chunks_per_frame,
                            uint32_t lanes_per_row, const uint8_t *d_images, uint8_t *d_out, uint64_t slot_stride,
                            uint64_t first_index, uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    EncParams p;
    p.images = d_images;
    p.out = d_out;
    p.frame_offsets = d_frame_offsets;
    p.frame_bytes = d_frame_bytes;
    p.indices = nullptr;
    p.elapsed_ns = nullptr;
    p.first_index = first_index;
    p.state = nullptr;
    p.ctrl = nullptr;
    p.ctrl_next = nullptr;
    p.mode_flags = nullptr;
    p.arrive_flags = nullptr;
    p.launch_epoch = 0;
    p.sticky = ctx->sticky;
    p.slot_stride = slot_stride;
    p.frame_pixels = (uint64_t)pix * g.pixels;   // bytes of one frame's image
    p.W = W; p.H = H; p.w = g.w; p.h = g.h; p.T = g.T;
    p.chunks_per_frame = chunks_per_frame;
    p.n_chunks = (uint32_t)n_frames * chunks_per_frame;
    p.lanes_per_row = lanes_per_row;
    p.pairs_per_wave = 64u;
    p.seg_per_row = p.seg_q = p.seg_rem = p.magic_seg = 0u;
    p.magic_w = div_magic_of(g.w);
    p.magic_cpf = div_magic_of(chunks_per_frame);
    p.magic_lpr = div_magic_of(lanes_per_row);
    p.last_frame = (uint32_t)n_frames - 1u;
    p.flags = ctx->exp_flags;
    p.grid_blocks = ctx->enc_grid;
    p.diag = reinterpret_cast<unsigned long long *>(ctx->diag);
    p.small_epoch = 0;
    return p;
}

// The encoders' shared workspace: [control words, set 0: 8 x u32][set 1][records: n_chunks x u64].  NO memset in front
// of a launch (round 3 cleared it before every persistent launch: a fill kernel and its boundary, 8-10 us of each):
//   * a persistent launch finds zeros where it needs them and leaves zeros behind -- every AGG / INC record is cleared
//     by the workgroup that reads it (wait_inc), the control words it uses were cleared by the launch before it (the
//     scanner clears the OTHER set; launches alternate), and records of small launches (below) have bits 63:62 clear,
//     which no AGG / INC record has;
//   * a small launch tags its records with its epoch and clears nothing.
// The block is zeroed when it is (re)allocated, when the small launches' epoch wraps, and after a launch that failed
// (dbde_hip_sync saw the sticky word: until then the context's launches return at once, encode_kernel).
static int attach_lookback(dbde_hip_ctx *ctx, EncParams &p, uint32_t n_chunks, bool small) {
    // two sets of control words | the mode flags | the arrival flags | records
    constexpr size_t kFlagsAt = 2 * 4 * (size_t)kEncCtrlWords, kHeader = (kFlagsAt + 2 * 4 * (size_t)kEncMaxGrid + 4095) & ~(size_t)4095;
    const size_t lb_need = (kHeader + 8 * (size_t)n_chunks + 15) & ~(size_t)15;
    {   // grown in place: on failure ctx->lb is null and ctx->lb_bytes 0, never a freed pointer
        const size_t had = ctx->lb_bytes;
        int rc = grow(ctx, ctx->lb, ctx->lb_bytes, lb_need, 1, true);
        if (rc) return rc;
        if (ctx->lb_bytes != had) ctx->lb_fresh = true;
    }
    if (ctx->lb_fresh || ctx->enc_epoch >= (1u << 30) - 1u) {   // (small launches' record tags and persistent launches' mode flags share the epoch counter)
        HIP_TRY(ctx, hipMemsetAsync(ctx->lb, 0, ctx->lb_bytes, ctx->stream));
        ctx->lb_fresh = false;
        ctx->enc_epoch = 0;
        ctx->enc_parity = 0;
    }
    const uint32_t epoch = ++ctx->enc_epoch;
    p.small_epoch = small ? epoch : 0u;
    p.launch_epoch = epoch;
    p.ctrl = reinterpret_cast<uint32_t *>(ctx->lb) + kEncCtrlWords * ctx->enc_parity;
    p.ctrl_next = reinterpret_cast<uint32_t *>(ctx->lb) + kEncCtrlWords * (ctx->enc_parity ^ 1u);
    p.mode_flags = reinterpret_cast<uint32_t *>(ctx->lb + kFlagsAt);
    p.arrive_flags = p.mode_flags + kEncMaxGrid;
    p.state = reinterpret_cast<unsigned long long *>(ctx->lb + kHeader);
    if (!small) ctx->enc_parity ^= 1u;
    return DBDE_HIP_OK;
}

// ---- batch encode ----------------------------------------------------------------------------
#ifndef DBDE_MID_ENCODE_TILES
// Frames of 65 .. this many tiles, one slot each, encode with whole frames per workgroup (encode_mid_kernel, 0.46 of peak
// on mixed content whatever T, 0.37 on incompressible frames); the chunk-per-frame kernels overtake it as T grows --
// measured: T = 81 / 144 / 196 / 256 / 324 / 396 general path 0.12 / 0.19 / 0.25 / 0.32 / 0.36 / 0.40 mixed and
// 0.15 / 0.27 / 0.35 / 0.44 / 0.50 / 0.53 incompressible.
#define DBDE_MID_ENCODE_TILES 256
#endif

// Which kernel an encode call runs and on what chunk geometry: a pure function of the shape, the batch size, the
// buffers' alignment, the layout and the number of workgroups the device holds (dbde_hip_encode_plan).
struct EncPlan {
    bool fast_in, aligned_out;
    uint32_t enc_cpf, lanes_per_row, pairs_per_wave;
    uint32_t seg_per_row, seg_q, seg_rem;   // kInRow: segments of a tile row (0 = not taken)
    uint64_t n_chunks64;
    int kernel;            // 0 = persistent (encode_kernel), 1 = encode_small_kernel, 2 = encode_tiny_kernel, 3 = encode_mid_kernel, 4 = encode_frames_kernel
};
#ifndef DBDE_ROW_FILL
#define DBDE_ROW_FILL 90
#endif
#ifndef DBDE_FRAMES_ENCODE_TILES
// Frames of 65 .. this many tiles with 8-byte aligned rows encode with whole frames per workgroup and staged, coalesced
// traffic (encode_frames_kernel); above it the chunk kernels' 512 / 1024 tile slots are filled well enough by one frame.
// (Its decode-side twin measured equal at 81 tiles (0.39; incompressible 0.42 -> 0.49) and slower from 144 tiles on
// (0.43 -> 0.37; 300 tiles: 0.55 with its index kernel counted -> 0.44) -- six dependent phases per workgroup, each a
// memory or LDS round trip, where decode_mid_kernel and the chunk decoder have three -- and was removed.)
#define DBDE_FRAMES_ENCODE_TILES 640   // measured (mixed, encode): 81 tiles 0.39 -> 0.51, 144 0.44 -> 0.56, 256 0.49 -> 0.65, 300 0.32 -> 0.51, 396 0.39 -> 0.57, 625 0.47 -> 0.48
#endif
#ifndef DBDE_GROUP_ENCODE_TILES
#define DBDE_GROUP_ENCODE_TILES 85    // largest frame (tiles) of the persistent small-frame encoder where frames above 64 tiles fill 90 % of its lanes (77 .. 85 tiles: three frames)
#endif
// rows 8-byte aligned, frames and base whole 16-byte blocks: what the staged whole-frame encoder takes
static bool frames_geometry(const Geometry &g, int W, uintptr_t images) {
    return W % 8 == 0 && g.pixels % 16 == 0 && (images & 15u) == 0 && g.T > 64u;
}
static EncPlan plan_encode(const Geometry &g, int W, int n_frames, uintptr_t images, uintptr_t out, uint64_t slot_stride,
                           uint32_t enc_grid) {
    EncPlan pl;
    pl.fast_in = (W % 16 == 0) && ((images & 15u) == 0);
    // chunk geometry of the encoder (EncParams): plain runs of 1024 tiles, or -- any-geometry path, W >= 16 --
    // 512 tile PAIRS that never leave a tile row
    pl.enc_cpf = (g.T + kEncChunkTiles - 1) / kEncChunkTiles;
    pl.lanes_per_row = 0;
    pl.pairs_per_wave = 64;
    pl.seg_per_row = pl.seg_q = pl.seg_rem = 0;
    if (!pl.fast_in && W >= 16) {
        pl.lanes_per_row = (g.w + 1u) / 2u;
        // Dword-aligned fetches (kInRaw4: a 16-byte load at an odd address runs at 0.87 of the rate of one at any even
        // address): a wave owns 63 pairs, its 64th lane feeds the 63rd.  Taken when the last pair of a tile row holds at
        // most 13 pixel columns -- the up to 3 bytes its moved fetch is short of are then padding (dbde_kernels.hip).
        // Rows at even addresses (W and the base even) read at the full rate as they are and keep 64 pairs.
        const uint32_t last_cols = (uint32_t)W - 16u * (pl.lanes_per_row - 1u);
        // (32-bit offsets inside a frame: geometry() admits frames of up to 8 GiB)
        if (last_cols <= 13u && ((W | (int)(images & 1u)) & 1) && g.pixels < (1ull << 31)) pl.pairs_per_wave = 63;
        const uint32_t ppc = pl.pairs_per_wave * (kEncChunkTiles / 128u);
        pl.enc_cpf = (uint32_t)(((uint64_t)g.h * pl.lanes_per_row + ppc - 1u) / ppc);
        // kInRow: one wave per segment of a tile row (addresses and shifts in scalar registers) when that keeps at least
        // DBDE_ROW_FILL percent of the lanes busy -- 1921 wide: 121 pairs = 61 + 60 of 128 lanes
        if (pl.pairs_per_wave == 63u) {
            const uint32_t nseg = (pl.lanes_per_row + 62u) / 63u;
            if (100u * pl.lanes_per_row >= (unsigned)DBDE_ROW_FILL * 64u * nseg && pl.lanes_per_row / nseg >= 2u) {
                pl.seg_per_row = nseg;
                pl.seg_q = pl.lanes_per_row / nseg;
                pl.seg_rem = pl.lanes_per_row % nseg;
                const uint32_t spc = kEncChunkTiles / 128u;   // segments (waves) per chunk
                pl.enc_cpf = (uint32_t)(((uint64_t)g.h * nseg + spc - 1u) / spc);
            }
        }
    }
    pl.n_chunks64 = (uint64_t)n_frames * pl.enc_cpf;
    pl.aligned_out = ((out & 7u) == 0) && (g.T % 4 == 0) && (slot_stride % 8 == 0);
    pl.kernel = 0;
    const bool rows4 = W % 4 == 0 && (images & 3u) == 0 && (out & 15u) == 0 && slot_stride % 16 == 0;
    // Small frames in slots, 8-byte aligned rows, frames and buffers whole 16-byte blocks: persistent workgroups, the next
    // group's pixels in flight while a group is encoded (encode_group_kernel: one tile per lane, 256 / T frames per
    // workgroup).  Measured against what it replaces (mixed / incompressible): 64x64 0.40 -> 0.53 / 0.33 -> 0.56, 32x32 0.35
    // -> 0.49 / 0.32 -> 0.47, 40x24 0.31 -> 0.46 / 0.30 -> 0.41; 72x72 (81 tiles, three frames fill 95 % of the lanes) 0.49 ->
    // 0.50 / 0.49 -> 0.56.  Where whole frames leave lanes empty the two-tiles-per-lane kernel below keeps mixed content
    // (96x96, one frame of 144 tiles per workgroup: 0.51 -> 0.42; 128x128 at full fill 0.62 -> 0.56, incompressible 0.54 ->
    // 0.58), and single-tile frames keep the per-wave kernel (8x8: 0.17 -> 0.09, 256 frame images per workgroup).
    // (rows and image bases of 4-byte multiples suffice since the round's last hours: DESIGN 4.1)
    // Rows of 4 mod 8 bytes take it for every frame up to 256 tiles (against encode_mid_kernel there: 84x84 0.33 -> 0.44 /
    // 0.30 -> 0.50, 124x124 0.37 -> 0.53 / 0.32 -> 0.59, 100x75 0.325 -> 0.316 / 0.29 -> 0.37).
    if (slot_stride != 0 && rows4 && g.T >= 4u &&
        (g.T <= 64u || (g.T <= (unsigned)DBDE_GROUP_ENCODE_TILES && (256u / g.T) * g.T * 10u >= 256u * 9u) ||
         (W % 8 != 0 && g.T <= 256u))) pl.kernel = 5;
    else if (g.T <= 64u && slot_stride != 0) pl.kernel = 2;     // tiny frames in slots: several frames per wave, nothing shared
    else if (slot_stride != 0 && g.T <= (unsigned)DBDE_FRAMES_ENCODE_TILES && frames_geometry(g, W, images) && (out & 15u) == 0 &&
             slot_stride % 16 == 0) pl.kernel = 4;              // 65 .. 700 tiles, aligned rows: whole frames per workgroup, staged
    else if (g.T <= (unsigned)DBDE_MID_ENCODE_TILES && slot_stride != 0) pl.kernel = 3;   // 65 .. 256 tiles in slots: whole frames per workgroup
    else if (pl.n_chunks64 < enc_grid) pl.kernel = 1;           // fewer chunks than resident workgroups: one workgroup per chunk
    return pl;
}

int dbde_hip_encode_frames(dbde_hip_ctx *ctx, const uint8_t *d_images, int W, int H, int n_frames,
                           uint64_t first_index, const uint64_t *d_indices, const uint64_t *d_elapsed_ns,
                           uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                           uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    Geometry g;
    if (!d_images || !d_out || n_frames < 0 || !geometry(W, H, g))
        return fail(ctx, DBDE_HIP_ERR_ARG, "encode_frames: bad argument (W=%d H=%d n=%d)", W, H, n_frames);
    if (n_frames == 0) return DBDE_HIP_OK;
    const uint64_t maxf = 32ull + 66ull * g.T;
    const EncPlan pl = plan_encode(g, W, n_frames, reinterpret_cast<uintptr_t>(d_images), reinterpret_cast<uintptr_t>(d_out), slot_stride,
                                   ctx->enc_grid);
    const bool fast_in = pl.fast_in, aligned_out = pl.aligned_out;
    const uint32_t enc_cpf = pl.enc_cpf, lanes_per_row = pl.lanes_per_row;
    const uint64_t n_chunks64 = pl.n_chunks64;
    if (n_chunks64 >= (1ull << 31)) return fail(ctx, DBDE_HIP_ERR_ARG, "encode_frames: too many chunks in one call");
    if (slot_stride) {
        if (slot_stride < maxf) return fail(ctx, DBDE_HIP_ERR_ARG, "encode_frames: slot_stride below the worst case");
        if ((uint64_t)(n_frames - 1) * slot_stride + maxf > out_capacity)
            return fail(ctx, DBDE_HIP_ERR_CAPACITY, "encode_frames: out_capacity below the worst case");
    } else {
        if ((uint64_t)n_frames * maxf > out_capacity)
            return fail(ctx, DBDE_HIP_ERR_CAPACITY, "encode_frames: out_capacity below the worst case");
        // launch-wide running word count is carried in 32 bits
        if ((uint64_t)n_frames * 8ull * g.T >= (1ull << 32))
            return fail(ctx, DBDE_HIP_ERR_ARG, "encode_frames: more than 2^32 payload words possible; split the batch");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const uint32_t n_chunks = (uint32_t)n_chunks64;
    EncParams p = enc_params(ctx, g, W, H, n_frames, 1u, enc_cpf, lanes_per_row, d_images, d_out, slot_stride, first_index,
                             d_frame_offsets, d_frame_bytes);
    p.indices = d_indices;
    p.elapsed_ns = d_elapsed_ns;
    p.pairs_per_wave = pl.pairs_per_wave;
    p.seg_per_row = pl.seg_per_row;
    p.seg_q = pl.seg_q;
    p.seg_rem = pl.seg_rem;
    p.magic_seg = pl.seg_per_row ? div_magic_of(pl.seg_per_row) : 0u;

    if (pl.kernel == 5) {   // 1 .. 256 tiles in slots, aligned rows: persistent workgroups, pixels double-buffered (encode_group_kernel)
        span_begin(ctx, 0);
        HIP_TRY(ctx, launch_encode_group(p, (uint32_t)n_frames, (ctx->exp_flags & 1024u) ? 0u : (uint32_t)ctx->n_cu, ctx->stream));   // (experiment bit 10: three workgroups)
        span_end(ctx);
        return DBDE_HIP_OK;
    }

    if (pl.kernel == 2) {   // tiny frames in slots: several frames per wave, nothing shared (encode_tiny_kernel)
        span_begin(ctx, 0);
        HIP_TRY(ctx, launch_encode_tiny(p, (uint32_t)n_frames, ctx->stream));
        span_end(ctx);
        return DBDE_HIP_OK;
    }

    if (pl.kernel == 4) {   // frames of 65 .. 700 tiles in slots, 8-byte aligned rows: whole frames per workgroup, staged (encode_frames_kernel)
        span_begin(ctx, 0);
        HIP_TRY(ctx, launch_encode_frames(p, (uint32_t)n_frames, ctx->stream));
        span_end(ctx);
        return DBDE_HIP_OK;
    }

    if (pl.kernel == 3) {   // frames of 65 .. 256 tiles in slots: whole frames per workgroup (encode_mid_kernel)
        span_begin(ctx, 0);
        HIP_TRY(ctx, launch_encode_mid(p, (uint32_t)n_frames, ctx->stream));
        span_end(ctx);
        return DBDE_HIP_OK;
    }

    // small launches (one frame per call above all): one workgroup per chunk, epoch-tagged records
    const bool small = pl.kernel == 1;
    {
        int rc = attach_lookback(ctx, p, n_chunks, small);
        if (rc) return rc;
    }
    span_begin(ctx, 0);   // (after the workspace: a failed attach returns with no span left open)
    if (small) HIP_TRY(ctx, launch_encode_small(p, fast_in, aligned_out, ctx->stream));
    else HIP_TRY(ctx, launch_encode(p, fast_in, aligned_out, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

// ---- batch decode ----------------------------------------------------------------------------
#ifndef DBDE_MID_DECODE_TILES
// Frames of up to this many tiles decode with whole frames per workgroup (decode_mid_kernel: one tile per lane, from one-tile
// frames up; rounds 2-3 had a kernel of its own for T <= 64, whole frames per wave, which the persistent form beat at every
// size -- 64x64 0.49 -> 0.63, 32x32 0.33 -> 0.56, 8x8 0.19 -> 0.30): no index kernel, no chunk.  Measured wall time per step, mid against chunks + index kernel, round 3:
// T = 81 twice as fast, 144 +24 %, 196 equal (mixed) / -14 % (incompressible), 256 -7 %; with the round-4 form of the kernel
// (persistent 256-thread workgroups, software-pipelined, wide payload loads, pixels staged): 169 tiles 0.91 -> 0.60 ms,
// 225 0.48 -> 0.40 (incompressible 0.53 -> 0.475), 240 0.40 -> 0.315, 256 0.416 -> 0.344 (incompressible 0.414 -> 0.429).
#define DBDE_MID_DECODE_TILES 256
#endif
#ifndef DBDE_MID_DECODE_TILES_UNSTAGED
#define DBDE_MID_DECODE_TILES_UNSTAGED 768
#endif
#ifndef DBDE_STAGED_FILL
// Percent of a workgroup's 512 tile slots that whole tile rows must fill for the staged decode path.  A workgroup's time
// hardly depends on how many of its slots are used, so empty slots are lost throughput -- but tile-by-tile stores
// (partial cache lines) cost more.  Measured on mixed content (round 3): 88 % fill (720, 1200, 600 wide) staged +4..9 %,
// 84 % (3440) +3.5 %, 82 % (1680) equal, 79 % (1080 wide: portrait HD) equal and +26 % on incompressible frames,
// 78 % (1600) -6 %, 70 % (1440) -4 %.
#define DBDE_STAGED_FILL 79
#endif

// Which kernels a decode call runs: a pure function of the geometry, the batch size, the image base's alignment and the
// device's CU count, so that the choice can be inspected and tested without a GPU (dbde_hip_decode_plan).
struct DecPlan {
    int img_mode;          // kImgDirect / kImgLinear / kImgTiles (dbde_kernels.hip)
    uint32_t cap;          // tile slots of the workgroup that takes whole-tile-row chunks
    DecGeom dg;
    uint64_t n_chunks64;
    bool self_index, fused;
    int kernel;            // 0 = chunk kernels, 3 = decode_mid_kernel
};
static DecPlan plan_decode(const Geometry &g, int W, int n_frames, uintptr_t ib, int n_cu) {
    DecPlan pl;
    // How the pixels reach the image (decode_kernel<IMG>): direct register -> image stores are only FAST when a
    // wave's 1 KB covers whole cache lines (W, the frame size and the base multiples of 128).  Other widths get
    // chunks of whole tile rows where those fill enough of a 512-tile workgroup (DBDE_STAGED_FILL percent): the
    // workgroup stages its pixels in LDS and writes whole cache lines of the chunk's byte range.  Everything else
    // stores tile by tile from plain chunks.
    int img_mode = 2;
    uint32_t cap = kChunkTiles;   // tile slots of the workgroup that takes whole-tile-row chunks
    if (W % 128 == 0 && g.pixels % 128 == 0 && (ib & 127u) == 0) img_mode = 0;
    else if (g.w <= kChunkTiles && W >= 16) {
        // whole tile rows in 512 slots (256 threads) or in 384 (192 threads), whichever they fill better
        // (1366 wide: 2 x 171 tiles = 67 % of 512, 89 % of 384)
        const uint32_t used512 = (kChunkTiles / g.w) * g.w;
        const uint32_t used384 = g.w <= kChunkTilesSmall ? (kChunkTilesSmall / g.w) * g.w : 0u;
        // (16-byte aligned rows are left out: there plain chunks with direct 16-byte stores, below, beat the better-filled
        // small workgroup on mixed content -- 1440 / 2704 wide: 0.70 / 0.70 against 0.68 / 0.67)
        if (W % 16 != 0 && (uint64_t)used384 * kChunkTiles > (uint64_t)used512 * kChunkTilesSmall) cap = kChunkTilesSmall;
        const uint32_t used = cap == kChunkTiles ? used512 : used384, rows = cap / g.w;
        if (used * 100u >= cap * (unsigned)DBDE_STAGED_FILL) {
            // image rows that are not 8-byte aligned are staged tile-aligned at pitch 8 w + 16: that image must fit the
            // workgroup's LDS (narrow frames have many rows per chunk and do not); chunks of at most 384 tiles run on
            // the smaller workgroup whatever `cap` says (launch_decode)
            const bool a8 = W % 8 == 0 && (ib & 7u) == 0;
            const uint64_t lds = used <= kChunkTilesSmall ? 25600ull : 34048ull;
            if (a8 || 8ull * rows * (8ull * g.w + 16ull) <= lds) img_mode = 1;
        }
    }
    // 16-byte aligned rows that neither cover whole cache lines per wave nor fill staged chunks: still ONE 16-byte store
    // per lane and image row (the direct form) instead of two 8-byte ones (1440 / 1600 wide: 0.62 -> 0.69 / 0.73)
    if (img_mode == 2 && W % 16 == 0 && (ib & 15u) == 0) img_mode = 0;
    pl.img_mode = img_mode;
    pl.cap = cap;
    pl.dg = dec_geometry(g.w, g.h, img_mode == 1, kChunkTiles, cap);
    pl.n_chunks64 = (uint64_t)n_frames * pl.dg.cpf;
    // Small frames (the tile-level entry points, thumbnails): the decode workgroups index the frame themselves --
    // each reads the T depth bytes -- and the index kernel with its launch boundary is gone.  Only while T is a
    // couple of loads per thread: for a 4096x3072 frame (T = 196,608, 384 workgroups re-reading it) the same
    // idea took 38 us against 11 us for index + decode, measured.
    // (Large batches of one-chunk frames gain nothing from it although each frame's depth bytes would be read only once:
    // 262,144 frames of 128x128 took 1.75 ms self-indexed against 1.50 ms with the index kernel, measured.)
    pl.self_index = g.T <= 8192u && pl.n_chunks64 * (uint64_t)g.T <= (8ull << 20);
    // Few LARGE frames (one 4096x3072 frame per call: 384 chunks): the decode workgroups build the index among
    // themselves (decode_kernel<IMG, kIdxFused>) -- no index kernel, no launch boundary.  Taken when the launch fits the
    // device's workgroup slots (four per CU); correctness does not depend on that, only the latency does.
    pl.fused = !pl.self_index && pl.n_chunks64 <= 4ull * (uint64_t)n_cu;
    // tiny frames (the tile-level entry points, thumbnails) and those just above: whole frames per wave / per workgroup
    pl.kernel = g.T <= (unsigned)DBDE_MID_DECODE_TILES ? 3 : 0;
    // ... and larger frames whose chunks would store tile by tile (rows that are not 8-byte aligned and whole-tile-row chunks
    // that do not fit the staged image): one frame per 512- or 1024-thread workgroup of the same kernel beats two chunks per
    // frame + the index kernel -- 180x180 (529 tiles) 0.25 -> 0.33 mixed / 0.28 -> 0.37 incompressible, 130x121 0.37 -> 0.39 / 0.47,
    // 220x215 (756) 0.36 -> 0.39 / 0.39 -> 0.46; not at 1024 tiles (250x250: 0.51 -> 0.44), not where the chunks stage
    // (300x200: 0.59 -> 0.42) -- profiles/r04b_gain.sh
    if (img_mode == 2 && g.T <= (unsigned)DBDE_MID_DECODE_TILES_UNSTAGED) pl.kernel = 3;
    return pl;
}

// Index split of the decode index kernel: few frames are cut into pieces so that the index pass fills the device too
// (>= 4 chunks per piece, about 1024 workgroups in all); from 256 frames on, one workgroup per frame.
static uint32_t index_split_for(int n_frames, uint32_t cpf) {
    if (n_frames < 1 || n_frames >= 256 || cpf < 8u) return 1u;
    uint32_t sp = 1024u / (uint32_t)n_frames;
    const uint32_t most = (cpf + 3u) / 4u;
    return sp > most ? most : (sp < 1u ? 1u : sp);
}

// The decode index kernel in timing slot 1: validation, results and per-chunk payload offsets (ctx->chunk_off,
// ctx->frame_ok) of n_frames > 0 frames cut into the chunks of dg.  min_bytes: 1 = DBDE, 2 = DBDE16.  split: workgroups
// per frame (1, or the split form's index_split_for).  Shared by every decoder that runs the index as a launch of its own.
static int run_index(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                     int n_frames, dbde_hip_frame_result *d_results, const DecGeom &dg, uint32_t min_bytes,
                     uint32_t split) {
    int rc = grow(ctx, ctx->chunk_off, ctx->chunk_off_n, (size_t)n_frames * (dg.cpf + 1u), sizeof(uint32_t));
    if (rc) return rc;
    rc = grow(ctx, ctx->frame_ok, ctx->frame_ok_n, (size_t)n_frames, sizeof(uint32_t));
    if (rc) return rc;

    IdxParams ip;
    ip.stream = d_stream;
    ip.frame_offsets = d_frame_offsets;
    ip.stream_bytes = stream_bytes;
    ip.chunk_off = ctx->chunk_off;
    ip.frame_ok = ctx->frame_ok;
    ip.results = d_results;
    ip.T = dg.T;
    ip.chunks_per_frame = dg.cpf;
    ip.min_bytes = min_bytes;
    ip.geom = dg;
    ip.split = 1;
    ip.frame_ctr = nullptr;
    ip.frame_flag = nullptr;
    if (split > 1u) {
        const size_t before = ctx->idx_ctr_n;
        rc = grow(ctx, ctx->idx_ctr, ctx->idx_ctr_n, 2 * (size_t)n_frames, sizeof(uint32_t));
        if (rc) return rc;
        if (ctx->idx_ctr_n != before)   // fresh block: the kernel keeps it zero from here on
            HIP_TRY(ctx, hipMemsetAsync(ctx->idx_ctr, 0, ctx->idx_ctr_n * sizeof(uint32_t), ctx->stream));
        ip.split = split;
        ip.frame_ctr = ctx->idx_ctr;
        ip.frame_flag = ctx->idx_ctr + n_frames;
    }
    span_begin(ctx, 1);
    HIP_TRY(ctx, launch_decode_index(ip, n_frames, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, uint8_t *d_images,
                           dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    Geometry g;
    if (!d_stream || !d_frame_offsets || !d_images || n_frames < 0 || !geometry(W, H, g))
        return fail(ctx, DBDE_HIP_ERR_ARG, "decode_frames: bad argument (W=%d H=%d n=%d)", W, H, n_frames);
    if (n_frames == 0) return DBDE_HIP_OK;
    const DecPlan pl = plan_decode(g, W, n_frames, reinterpret_cast<uintptr_t>(d_images), ctx->n_cu);
    const int img_mode = pl.img_mode;
    const DecGeom dg = pl.dg;
    const uint32_t dcpf = dg.cpf;   // whole tile rows (or pieces of a wide one) per chunk, one decode workgroup each
    if (dcpf > kMaxChunksPerFrame) return fail(ctx, DBDE_HIP_ERR_ARG, "decode_frames: frame too large");
    const uint64_t n_chunks64 = pl.n_chunks64;
    if (n_chunks64 >= (1ull << 31)) return fail(ctx, DBDE_HIP_ERR_ARG, "decode_frames: too many chunks in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool self_index = pl.self_index;
    if (pl.kernel != 0) {   // tiny frames (the tile-level entry points, thumbnails) and those just above: whole frames per wave / per workgroup, nothing else needed
        DecParams tp;
        memset(&tp, 0, sizeof tp);
        tp.stream = d_stream; tp.frame_offsets = d_frame_offsets; tp.stream_bytes = stream_bytes;
        tp.images = d_images; tp.results = d_results; tp.frame_pixels = g.pixels;
        tp.W = W; tp.H = H; tp.w = g.w; tp.h = g.h; tp.T = g.T;
        span_begin(ctx, 2);
        HIP_TRY(ctx, launch_decode_mid(tp, (uint32_t)n_frames, (ctx->exp_flags & 1024u) ? 0u : (uint32_t)ctx->n_cu, ctx->mid_dec_per_cu, ctx->stream));   // (experiment bit 10: three workgroups)
        span_end(ctx);
        return DBDE_HIP_OK;
    }
    const bool fused = pl.fused;   // few large frames: the index is built inside the decode launch (plan_decode)
    if (fused) {
        const size_t had = ctx->fuse_rec_n;
        int rc = grow(ctx, ctx->fuse_rec, ctx->fuse_rec_n, (size_t)n_chunks64, sizeof(unsigned long long), true);
        if (rc) return rc;
        if (ctx->fuse_rec_n != had || ctx->fuse_epoch == 0xFFFFFFFFu) {   // a fresh block (or the epoch wrapping): epoch 0 everywhere
            HIP_TRY(ctx, hipMemsetAsync(ctx->fuse_rec, 0, ctx->fuse_rec_n * sizeof(unsigned long long), ctx->stream));
            ctx->fuse_epoch = 0;
        }
        ctx->fuse_epoch++;
    }
    if (!self_index && !fused) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, dg, 1u,
                           index_split_for(n_frames, dcpf));
        if (rc) return rc;
    }

    DecParams p;
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.images = d_images;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.results = d_results;
    p.frame_pixels = g.pixels;
    p.W = W;
    p.H = H;
    p.w = g.w;
    p.h = g.h;
    p.T = g.T;
    p.chunks_per_frame = dcpf;
    p.n_chunks = (uint32_t)n_chunks64;
    p.magic_W = div_magic_of((uint32_t)W);
    p.fuse_rec = ctx->fuse_rec;
    p.fuse_epoch = ctx->fuse_epoch;
    p.fuse_flags = (ctx->exp_flags & 16u) ? 1u : 0u;
    p.diag = reinterpret_cast<unsigned long long *>(ctx->diag);
    p.geom = dg;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode(p, img_mode, self_index ? 1 : (fused ? 2 : 0), ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

// ---- window decode ----------------------------------------------------------------------------------------
struct RoiPlan {
    Geometry g;
    DecGeom dg;                       // the index's chunks (roi_index_geometry)
    uint32_t tx0, ty0, ntx, nty;      // the window at (x0, y0)
    uint32_t max_tx, max_ty;          // the most any origin needs
    uint32_t split, threads, pieces, pieces_fixed;
    uint64_t grid, grid_origins;
};
// nullptr when the arguments are good, else what is wrong with them.  wide: tiles per workgroup of windows more than 64
// tiles across (kRoiWideThreads for DBDE, kRoi16WideThreads for DBDE16).
static const char *plan_roi(int W, int H, int n_frames, int x0, int y0, int rw, int rh, RoiPlan &pl,
                            uint32_t wide = kRoiWideThreads) {
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, pl.g)) return "bad frame size";
    if (rw < 1 || rh < 1 || rw > W || rh > H) return "window size outside [1, W] x [1, H]";
    if (x0 < 0 || y0 < 0 || x0 > W - rw || y0 > H - rh) return "window origin outside [0, W-rw] x [0, H-rh]";
    pl.dg = roi_index_geometry(pl.g.w, pl.g.h);
    if (pl.dg.cpf > kMaxChunksPerFrame) return "frame too large";
    pl.tx0 = (uint32_t)x0 >> 3;
    pl.ty0 = (uint32_t)y0 >> 3;
    pl.ntx = (uint32_t)(x0 + rw - 1) / 8u + 1u - pl.tx0;
    pl.nty = (uint32_t)(y0 + rh - 1) / 8u + 1u - pl.ty0;
    // x mod 8 reaches min(7, W - rw) over the origins a window of this width can have
    const uint32_t mx = (uint32_t)(W - rw) < 7u ? (uint32_t)(W - rw) : 7u, my = (uint32_t)(H - rh) < 7u ? (uint32_t)(H - rh) : 7u;
    pl.max_tx = (mx + (uint32_t)rw + 7u) / 8u;
    pl.max_ty = (my + (uint32_t)rh + 7u) / 8u;
    pl.split = index_split_for(n_frames, pl.dg.cpf);
    pl.threads = pl.max_tx <= kRoiNarrowThreads ? kRoiNarrowThreads : wide;
    pl.pieces = (pl.max_tx + pl.threads - 1u) / pl.threads;
    pl.pieces_fixed = (pl.ntx + pl.threads - 1u) / pl.threads;
    pl.grid = (uint64_t)n_frames * pl.nty * pl.pieces_fixed;
    pl.grid_origins = (uint64_t)n_frames * pl.max_ty * pl.pieces;
    if (pl.grid_origins >= (1ull << 31)) return "too many workgroups in one call";
    if ((uint64_t)n_frames * (pl.dg.cpf + 1u) >= (1ull << 31)) return "too many chunks in one call";
    return nullptr;
}

static void report_roi_plan(const RoiPlan &pl, dbde_hip_roi_plan_t *plan) {
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.tx0;
    plan->tile_y = (int32_t)pl.ty0;
    plan->tiles_x = (int32_t)pl.ntx;
    plan->tiles_y = (int32_t)pl.nty;
    plan->max_tiles_x = (int32_t)pl.max_tx;
    plan->max_tiles_y = (int32_t)pl.max_ty;
    plan->chunks_per_frame = pl.dg.cpf;
    plan->chunk_tiles = pl.dg.ct;
    plan->chunk_pieces = pl.dg.ct == pl.g.w || pl.dg.pieces > 1u ? pl.dg.pieces : 0u;
    plan->index_split = pl.split;
    plan->threads = pl.threads;
    plan->pieces_x = pl.pieces;
    plan->grid = pl.grid;
    plan->grid_origins = pl.grid_origins;
}

int dbde_hip_roi_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_roi_plan_t *plan) {
    RoiPlan pl;
    if (!plan || plan_roi(W, H, n_frames, x0, y0, rw, rh, pl)) return DBDE_HIP_ERR_ARG;
    report_roi_plan(pl, plan);
    return DBDE_HIP_OK;
}

int dbde16_hip_roi_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_roi_plan_t *plan) {
    RoiPlan pl;
    if (!plan || plan_roi(W, H, n_frames, x0, y0, rw, rh, pl, kRoi16WideThreads)) return DBDE_HIP_ERR_ARG;
    report_roi_plan(pl, plan);
    return DBDE_HIP_OK;
}

// Both window decoders: the index (min_bytes: 1 = DBDE, 2 = DBDE16) in timing slot 1, the window kernel in slot 2.
static int decode_roi_common(dbde_hip_ctx *ctx, const char *name, uint32_t min_bytes, const uint8_t *d_stream,
                             size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                             int y0, int rw, int rh, const int32_t *d_origins, void *d_out,
                             dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    RoiPlan pl;
    const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl, min_bytes == 2u ? kRoi16WideThreads : kRoiWideThreads);
    if (why)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames,
                    rw, rh, x0, y0);
    if (!d_stream || !d_frame_offsets || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, min_bytes, pl.split);
    if (rc) return rc;

    RoiParams p;
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.origins = d_origins;
    p.out = static_cast<uint8_t *>(d_out);
    p.W = W;
    p.H = H;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.w = pl.g.w;
    p.h = pl.g.h;
    p.T = pl.g.T;
    p.geom = pl.dg;
    p.rows = d_origins ? pl.max_ty : pl.nty;
    p.pieces = d_origins ? pl.pieces : pl.pieces_fixed;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_roi(p, (uint32_t)n_frames, pl.threads, min_bytes, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_roi(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                        int W, int H, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                        uint8_t *d_out, dbde_hip_frame_result *d_results) {
    return decode_roi_common(ctx, "decode_roi", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                             rh, d_origins, d_out, d_results);
}

int dbde16_hip_decode_roi(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                          const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                          const int32_t *d_origins, uint16_t *d_out, dbde_hip_frame_result *d_results) {
    return decode_roi_common(ctx, "decode_roi16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                             rw, rh, d_origins, d_out, d_results);
}

// ---- temporal projections ---------------------------------------------------------------------------------
struct ProjectPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t stats;
    uint32_t pieces, rows, segments, fps;
    uint64_t grid, combine_grid, workspace;
};
// Frames per segment: a segment is cut only to fill the device (about 4 workgroups per CU) and never below
// kProjMinFramesPerSegment frames, whose partials would cost more traffic than they save; never above the U32 bound.
// pix: 1 = DBDE (dbde_hip_project), 2 = DBDE16 (dbde16_hip_project: kProjTilesOf(2) tiles per workgroup, U16 / U64
// partials); the segment rule is the same for both.
static constexpr uint32_t kProjMinFramesPerSegment = 32;
static const char *plan_project_segments(int n_frames, int rw, int rh, int n_cu, uint32_t pix, ProjectPlan &pl);
static const char *plan_project(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                                uint32_t pix, ProjectPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    if (stats < 1u || stats > kProjAll) return "no statistic (or an unknown one) requested";
    pl.stats = stats;
    const uint32_t tiles = kProjTilesOf(pix);
    pl.pieces = (pl.roi.ntx + tiles - 1u) / tiles;
    return plan_project_segments(n_frames, rw, rh, n_cu, pix, pl);
}
// The rows, segments, grids and workspace of a projection whose pieces across a window tile row are set (pl.pieces).
static const char *plan_project_segments(int n_frames, int rw, int rh, int n_cu, uint32_t pix, ProjectPlan &pl) {
    pl.rows = pl.roi.nty;
    const uint64_t base = (uint64_t)pl.pieces * pl.rows, n = (uint64_t)n_frames;
    const uint64_t target = 4ull * (uint64_t)(n_cu > 0 ? n_cu : 1);
    uint64_t seg = base >= target ? 1u : (target + base - 1u) / base;
    const uint64_t by_len = (n + kProjMinFramesPerSegment - 1u) / kProjMinFramesPerSegment;
    if (seg > by_len) seg = by_len;
    const uint64_t by_bound = (n + kProjMaxFramesPerSegment - 1u) / kProjMaxFramesPerSegment;
    if (seg < by_bound) seg = by_bound;
    if (seg < 1u) seg = 1u;
    uint64_t fps = (n + seg - 1u) / seg;
    if (fps > 0u) seg = (n + fps - 1u) / fps;   // no empty segment
    if (seg >= (1ull << 31)) return "too many workgroups in one call";
    pl.segments = (uint32_t)seg;
    pl.fps = (uint32_t)fps;
    pl.grid = base * seg;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t pixels = (uint64_t)rw * (uint64_t)rh;
    pl.combine_grid = seg > 1u ? (pixels + kProjCombineThreads - 1u) / kProjCombineThreads : 0u;
    if (pl.combine_grid >= (1ull << 31)) return "too many workgroups in one call";
    pl.workspace = project_workspace_bytes(pl.stats, pl.segments, pixels, pix);
    return nullptr;
}

static int project_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                               uint32_t pix, dbde_hip_project_plan_t *plan) {
    ProjectPlan pl;
    if (!plan || plan_project(W, H, n_frames, x0, y0, rw, rh, stats, n_cu, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->threads = kProjThreads;   // (DBDE16: 16 lanes per tile, threads / 16 tiles)
    plan->pieces_x = pl.pieces;
    plan->segments = pl.segments;
    plan->frames_per_segment = pl.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->grid = pl.grid;
    plan->combine_grid = pl.combine_grid;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

int dbde_hip_project_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                          dbde_hip_project_plan_t *plan) {
    return project_plan_common(W, H, n_frames, x0, y0, rw, rh, stats, n_cu, 1u, plan);
}

int dbde16_hip_project_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats, int n_cu,
                            dbde_hip_project_plan_t *plan) {
    return project_plan_common(W, H, n_frames, x0, y0, rw, rh, stats, n_cu, 2u, plan);
}

// Both projections: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the projection
// kernels in slot 2.  d_max / d_min hold U8 (pix 1) or U16 (pix 2) pixels.
static int project_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                          size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                          int y0, int rw, int rh, int accumulate, void *d_max, void *d_min, uint64_t *d_sum,
                          uint64_t *d_sumsq, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_max ? kProjMax : 0u) | (d_min ? kProjMin : 0u) | (d_sum ? kProjSum : 0u) |
                           (d_sumsq ? kProjSumSq : 0u);
    ProjectPlan pl;
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, stats, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames,
                    rw, rh, x0, y0);
    if (!d_stream || !d_frame_offsets || !d_count) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if ((reinterpret_cast<uintptr_t>(d_sum) | reinterpret_cast<uintptr_t>(d_sumsq) |
         reinterpret_cast<uintptr_t>(d_count)) & 7u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_max) | reinterpret_cast<uintptr_t>(d_min)) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 outputs must be 2-byte aligned", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
        if (rc) return rc;
    }
    ProjParams p;
    memset(&p, 0, sizeof p);
    if (pl.workspace) {   // the partials in project_workspace_bytes' order: max, min, sum, sumsq, each 16-byte aligned
        int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.workspace, 1);
        if (rc) return rc;
        const uint64_t n = (uint64_t)pl.segments * (uint64_t)rw * (uint64_t)rh;
        const uint64_t mm = (pix * n + 15u) & ~(uint64_t)15, u32 = (4u * n + 15u) & ~(uint64_t)15;
        const uint64_t sq = pix == 1u ? u32 : (8u * n + 15u) & ~(uint64_t)15;
        uint8_t *w = ctx->proj_ws;
        if (d_max) { p.ws_max = w; w += mm; }
        if (d_min) { p.ws_min = w; w += mm; }
        if (d_sum) { p.ws_sum = reinterpret_cast<uint32_t *>(w); w += u32; }
        if (d_sumsq) { p.ws_sumsq = reinterpret_cast<uint32_t *>(w); w += sq; }
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.roi.g.T;
    p.w = pl.roi.g.w;
    p.geom = pl.roi.dg;
    p.tx0 = pl.roi.tx0;
    p.ty0 = pl.roi.ty0;
    p.rows = pl.rows;
    p.pieces = pl.pieces;
    p.segments = pl.segments;
    p.fps = pl.fps;
    p.accumulate = accumulate ? 1 : 0;
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_project(p, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                     int W, int H, int n_frames, int x0, int y0, int rw, int rh, int accumulate, uint8_t *d_max,
                     uint8_t *d_min, uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count,
                     dbde_hip_frame_result *d_results) {
    return project_common(ctx, "project", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                          accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_results);
}

int dbde16_hip_project(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                       const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                       int accumulate, uint16_t *d_max, uint16_t *d_min, uint64_t *d_sum, uint64_t *d_sumsq,
                       uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return project_common(ctx, "project16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                          rh, accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_results);
}

// ---- weighted temporal projections -------------------------------------------------------
// The window, the index geometry and the segment rule are plan_project's (any statistics set gives the same segments);
// ONE_SEGMENT forces one segment, whose F32 chain has no bound on its frames.
struct WProjectPlan {
    ProjectPlan proj;
    uint32_t regressors;
};
static const char *plan_wproject(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                 uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                 uint64_t count_address, int n_cu, uint32_t pix, WProjectPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (n_regressors < 1 || n_regressors > (int)kWProjMaxRegressors) return "n_regressors outside 1..8";
    if (flags & ~DBDE_HIP_WPROJ_ONE_SEGMENT) return "unknown flag bits";
    if (weight_stride < (uint64_t)n_frames) return "weight_stride < n_frames";
    if (!weights_address || !out_address || !count_address) return "null pointer";
    if ((weights_address | out_address) & 3u) return "F32 weights and output must be 4-byte aligned";
    if (count_address & 7u) return "the U64 count must be 8-byte aligned";
    pl.regressors = (uint32_t)n_regressors;
    if (flags & DBDE_HIP_WPROJ_ONE_SEGMENT) {
        pl.proj.segments = 1u;
        pl.proj.fps = (uint32_t)n_frames;
        pl.proj.grid = (uint64_t)pl.proj.pieces * pl.proj.rows;
        pl.proj.combine_grid = 0u;
    }
    pl.proj.workspace = wproject_workspace_bytes(pl.regressors, pl.proj.segments, (uint64_t)rw * (uint64_t)rh);
    return nullptr;
}

static int wproject_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_weighted_plan_t *plan) {
    WProjectPlan pl;
    if (!plan || plan_wproject(W, H, n_frames, x0, y0, rw, rh, n_regressors, weight_stride, flags, weights_address,
                               out_address, count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.proj.roi.tx0;
    plan->tile_y = (int32_t)pl.proj.roi.ty0;
    plan->tiles_x = (int32_t)pl.proj.roi.ntx;
    plan->tiles_y = (int32_t)pl.proj.roi.nty;
    plan->chunks_per_frame = pl.proj.roi.dg.cpf;
    plan->chunk_tiles = pl.proj.roi.dg.ct;
    plan->chunk_pieces = pl.proj.roi.dg.ct == pl.proj.roi.g.w || pl.proj.roi.dg.pieces > 1u ? pl.proj.roi.dg.pieces : 0u;
    plan->index_split = pl.proj.roi.split;
    plan->threads = kProjThreads;
    plan->pieces_x = pl.proj.pieces;
    plan->segments = pl.proj.segments;
    plan->frames_per_segment = pl.proj.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->regressors = pl.regressors;
    plan->grid = pl.proj.grid;
    plan->combine_grid = pl.proj.combine_grid;
    plan->workspace_bytes = pl.proj.workspace;
    plan->lds_bytes = kWProjLdsBytes;
    return DBDE_HIP_OK;
}

int dbde_hip_project_weighted_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                   uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                   uint64_t count_address, int n_cu, dbde_hip_project_weighted_plan_t *plan) {
    return wproject_plan_common(W, H, n_frames, x0, y0, rw, rh, n_regressors, weight_stride, flags, weights_address,
                                out_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_weighted_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_regressors,
                                     uint64_t weight_stride, int flags, uint64_t weights_address, uint64_t out_address,
                                     uint64_t count_address, int n_cu, dbde_hip_project_weighted_plan_t *plan) {
    return wproject_plan_common(W, H, n_frames, x0, y0, rw, rh, n_regressors, weight_stride, flags, weights_address,
                                out_address, count_address, n_cu, 2u, plan);
}

// Both weighted projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
static int wproject_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                           size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                           int y0, int rw, int rh, const float *d_weights, int n_regressors, size_t weight_stride,
                           int accumulate, int flags, float *d_out, uint64_t *d_count,
                           dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    WProjectPlan pl;
    if (const char *why = plan_wproject(W, H, n_frames, x0, y0, rw, rh, n_regressors, (uint64_t)weight_stride, flags,
                                        reinterpret_cast<uintptr_t>(d_weights), reinterpret_cast<uintptr_t>(d_out),
                                        reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, R=%d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, n_regressors);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                           pl.proj.roi.split);
        if (rc) return rc;
    }
    WProjParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the F32 partials [segments][R][rh * rw]
        int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        p.ws = reinterpret_cast<float *>(ctx->proj_ws);
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.proj.roi.g.T;
    p.w = pl.proj.roi.g.w;
    p.geom = pl.proj.roi.dg;
    p.tx0 = pl.proj.roi.tx0;
    p.ty0 = pl.proj.roi.ty0;
    p.rows = pl.proj.rows;
    p.pieces = pl.proj.pieces;
    p.segments = pl.proj.segments;
    p.fps = pl.proj.fps;
    p.accumulate = accumulate ? 1 : 0;
    p.regressors = pl.regressors;
    p.weights = d_weights;
    p.weight_stride = (uint64_t)weight_stride;
    p.out = d_out;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_wproject(p, pl.regressors, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_weighted(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw,
                              int rh, const float *d_weights, int n_regressors, size_t weight_stride, int accumulate,
                              int flags, float *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return wproject_common(ctx, "project_weighted", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                           rw, rh, d_weights, n_regressors, weight_stride, accumulate, flags, d_out, d_count, d_results);
}

int dbde16_hip_project_weighted(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw,
                                int rh, const float *d_weights, int n_regressors, size_t weight_stride, int accumulate,
                                int flags, float *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return wproject_common(ctx, "project_weighted16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                           y0, rw, rh, d_weights, n_regressors, weight_stride, accumulate, flags, d_out, d_count,
                           d_results);
}

// ---- count projections -------------------------------------------------------------------
// The window, the index geometry and the segment rule are plan_project's (any statistics set gives the same segments).
// The counts are integers, so the value does not depend on the segments.
struct CountsPlan {
    ProjectPlan proj;
    uint32_t levels;
};
static const char *plan_counts(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                               uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                               uint64_t count_address, int n_cu, uint32_t pix, CountsPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (n_levels < 1 || n_levels > (int)kCountsMaxLevels) return "n_levels outside 1..8";
    if (flags & ~DBDE_HIP_COUNTS_MAPS) return "unknown flag bits";
    if ((flags & DBDE_HIP_COUNTS_MAPS) && level_stride < (uint64_t)rw * (uint64_t)rh) return "level_stride < rw * rh";
    if (!thresholds_address || !out_address || !count_address) return "null pointer";
    if (thresholds_address & (pix - 1u)) return "U16 thresholds must be 2-byte aligned";
    if (out_address & 3u) return "the U32 output must be 4-byte aligned";
    if (count_address & 7u) return "the U64 count must be 8-byte aligned";
    pl.levels = (uint32_t)n_levels;
    pl.proj.workspace = counts_workspace_bytes(pl.levels, pl.proj.segments, (uint64_t)rw * (uint64_t)rh);
    return nullptr;
}

static int counts_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                              uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                              uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_counts_plan_t *plan) {
    CountsPlan pl;
    if (!plan || plan_counts(W, H, n_frames, x0, y0, rw, rh, n_levels, level_stride, flags, thresholds_address,
                             out_address, count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.proj.roi.tx0;
    plan->tile_y = (int32_t)pl.proj.roi.ty0;
    plan->tiles_x = (int32_t)pl.proj.roi.ntx;
    plan->tiles_y = (int32_t)pl.proj.roi.nty;
    plan->chunks_per_frame = pl.proj.roi.dg.cpf;
    plan->chunk_tiles = pl.proj.roi.dg.ct;
    plan->chunk_pieces = pl.proj.roi.dg.ct == pl.proj.roi.g.w || pl.proj.roi.dg.pieces > 1u ? pl.proj.roi.dg.pieces : 0u;
    plan->index_split = pl.proj.roi.split;
    plan->threads = kProjThreads;
    plan->pieces_x = pl.proj.pieces;
    plan->segments = pl.proj.segments;
    plan->frames_per_segment = pl.proj.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->levels = pl.levels;
    plan->grid = pl.proj.grid;
    plan->combine_grid = pl.proj.combine_grid;
    plan->workspace_bytes = pl.proj.workspace;
    plan->lds_bytes = kCountsLdsBytes;
    return DBDE_HIP_OK;
}

int dbde_hip_project_counts_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                                 uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                                 uint64_t count_address, int n_cu, dbde_hip_project_counts_plan_t *plan) {
    return counts_plan_common(W, H, n_frames, x0, y0, rw, rh, n_levels, level_stride, flags, thresholds_address,
                              out_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_counts_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int n_levels,
                                   uint64_t level_stride, int flags, uint64_t thresholds_address, uint64_t out_address,
                                   uint64_t count_address, int n_cu, dbde_hip_project_counts_plan_t *plan) {
    return counts_plan_common(W, H, n_frames, x0, y0, rw, rh, n_levels, level_stride, flags, thresholds_address,
                              out_address, count_address, n_cu, 2u, plan);
}

// Both count projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
static int counts_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         const void *d_thresholds, int n_levels, size_t level_stride, int accumulate, int flags,
                         uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    CountsPlan pl;
    if (const char *why = plan_counts(W, H, n_frames, x0, y0, rw, rh, n_levels, (uint64_t)level_stride, flags,
                                      reinterpret_cast<uintptr_t>(d_thresholds), reinterpret_cast<uintptr_t>(d_out),
                                      reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, K=%d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, n_levels);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                           pl.proj.roi.split);
        if (rc) return rc;
    }
    CountsParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the U32 partials [segments][K][rh * rw]
        int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        p.ws = reinterpret_cast<uint32_t *>(ctx->proj_ws);
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.proj.roi.g.T;
    p.w = pl.proj.roi.g.w;
    p.geom = pl.proj.roi.dg;
    p.tx0 = pl.proj.roi.tx0;
    p.ty0 = pl.proj.roi.ty0;
    p.rows = pl.proj.rows;
    p.pieces = pl.proj.pieces;
    p.segments = pl.proj.segments;
    p.fps = pl.proj.fps;
    p.accumulate = accumulate ? 1 : 0;
    p.levels = pl.levels;
    p.maps = (flags & DBDE_HIP_COUNTS_MAPS) ? 1 : 0;
    p.thresholds = d_thresholds;
    p.level_stride = (uint64_t)level_stride;
    p.out = d_out;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_counts(p, pl.levels, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_counts(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                            const uint8_t *d_thresholds, int n_levels, size_t level_stride, int accumulate, int flags,
                            uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return counts_common(ctx, "project_counts", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                         rh, d_thresholds, n_levels, level_stride, accumulate, flags, d_out, d_count, d_results);
}

int dbde16_hip_project_counts(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw,
                              int rh, const uint16_t *d_thresholds, int n_levels, size_t level_stride, int accumulate,
                              int flags, uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return counts_common(ctx, "project_counts16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                         rw, rh, d_thresholds, n_levels, level_stride, accumulate, flags, d_out, d_count, d_results);
}

// ---- neighbour-product projections -------------------------------------------------------
// The window and the index geometry are plan_project's.  The pieces across a window tile row overlap by the halo tiles
// of the instance that serves the mask (kPairsPiecesOf), and the segment rule is plan_project's applied to that grid.
// The sums are integers, so the value does not depend on the segments.
struct PairsPlan {
    ProjectPlan proj;
    uint32_t pairs, planes, instance;
};
static const char *plan_pairs(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs, uint64_t out_address,
                              uint64_t count_address, int n_cu, uint32_t pix, PairsPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (pairs < 1 || pairs > (int)kPairAll) return "pairs outside 1..15";
    if (!out_address || !count_address) return "null pointer";
    if ((out_address | count_address) & 7u) return "the U64 output and count must be 8-byte aligned";
    pl.pairs = (uint32_t)pairs;
    pl.planes = (uint32_t)__builtin_popcount(pl.pairs);
    pl.instance = kPairsInstanceOf(pl.pairs);
    pl.proj.pieces = kPairsPiecesOf(pl.proj.roi.ntx, pl.instance, pix);
    if (const char *why = plan_project_segments(n_frames, rw, rh, n_cu, pix, pl.proj)) return why;
    pl.proj.workspace = pairs_workspace_bytes(pl.planes, pl.proj.segments, (uint64_t)rw * (uint64_t)rh, pix);
    return nullptr;
}

static int pairs_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs, uint64_t out_address,
                             uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_pairs_plan_t *plan) {
    PairsPlan pl;
    if (!plan || plan_pairs(W, H, n_frames, x0, y0, rw, rh, pairs, out_address, count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.proj.roi.tx0;
    plan->tile_y = (int32_t)pl.proj.roi.ty0;
    plan->tiles_x = (int32_t)pl.proj.roi.ntx;
    plan->tiles_y = (int32_t)pl.proj.roi.nty;
    plan->chunks_per_frame = pl.proj.roi.dg.cpf;
    plan->chunk_tiles = pl.proj.roi.dg.ct;
    plan->chunk_pieces = pl.proj.roi.dg.ct == pl.proj.roi.g.w || pl.proj.roi.dg.pieces > 1u ? pl.proj.roi.dg.pieces : 0u;
    plan->index_split = pl.proj.roi.split;
    plan->threads = kProjThreads;
    plan->pieces_x = pl.proj.pieces;
    plan->segments = pl.proj.segments;
    plan->frames_per_segment = pl.proj.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->planes = pl.planes;
    plan->grid = pl.proj.grid;
    plan->combine_grid = pl.proj.combine_grid;
    plan->workspace_bytes = pl.proj.workspace;
    plan->lds_bytes = kPairsLdsBytesOf(pl.instance);
    plan->instance = pl.instance;
    plan->piece_tiles = kProjTilesOf(pix);
    plan->piece_stride = kPairsStrideOf(pl.instance, pix);
    plan->halo_left = kPairsHaloLeft(pl.instance);
    plan->halo_right = kPairsHaloRight(pl.instance);
    plan->rows_below = pl.instance != kPairRight ? pl.proj.roi.nty - 1u : 0u;
    return DBDE_HIP_OK;
}

int dbde_hip_project_pairs_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs,
                                uint64_t out_address, uint64_t count_address, int n_cu,
                                dbde_hip_project_pairs_plan_t *plan) {
    return pairs_plan_common(W, H, n_frames, x0, y0, rw, rh, pairs, out_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_pairs_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs,
                                  uint64_t out_address, uint64_t count_address, int n_cu,
                                  dbde_hip_project_pairs_plan_t *plan) {
    return pairs_plan_common(W, H, n_frames, x0, y0, rw, rh, pairs, out_address, count_address, n_cu, 2u, plan);
}

// Both pair projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
static int pairs_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                        const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                        int pairs, int accumulate, uint64_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    PairsPlan pl;
    if (const char *why = plan_pairs(W, H, n_frames, x0, y0, rw, rh, pairs, reinterpret_cast<uintptr_t>(d_out),
                                     reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, pairs=%d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, pairs);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                           pl.proj.roi.split);
        if (rc) return rc;
    }
    PairsParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the partials [segments][planes][rh * rw], U32 (pix 1) or U64 (pix 2)
        int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        p.ws = ctx->proj_ws;
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.proj.roi.g.T;
    p.w = pl.proj.roi.g.w;
    p.geom = pl.proj.roi.dg;
    p.tx0 = pl.proj.roi.tx0;
    p.ty0 = pl.proj.roi.ty0;
    p.rows = pl.proj.rows;
    p.pieces = pl.proj.pieces;
    p.segments = pl.proj.segments;
    p.fps = pl.proj.fps;
    p.accumulate = accumulate ? 1 : 0;
    p.pairs = pl.pairs;
    p.planes = pl.planes;
    p.out = d_out;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_pairs(p, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_pairs(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           int pairs, int accumulate, uint64_t *d_out, uint64_t *d_count,
                           dbde_hip_frame_result *d_results) {
    return pairs_common(ctx, "project_pairs", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                        pairs, accumulate, d_out, d_count, d_results);
}

int dbde16_hip_project_pairs(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                             int pairs, int accumulate, uint64_t *d_out, uint64_t *d_count,
                             dbde_hip_frame_result *d_results) {
    return pairs_common(ctx, "project_pairs16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                        rh, pairs, accumulate, d_out, d_count, d_results);
}

// ---- lag projections ---------------------------------------------------------------------
// The window, the index geometry, the pieces and the segment rule are plan_project's (any statistics set gives the same
// segments).  The values are integers, so they do not depend on the segments.
struct LagPlan {
    ProjectPlan proj;
    uint32_t stats, instance, lag, lead, first_pair, history;
};
static const char *plan_lag(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead, unsigned stats,
                            uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                            uint64_t count_address, int n_cu, uint32_t pix, LagPlan &pl) {
    if (const char *why = plan_project(W, H, n_frames, x0, y0, rw, rh, kProjSum, n_cu, pix, pl.proj)) return why;
    if (lag < 1 || lag > (int)kLagMax) return "lag outside 1..8";
    if (lead < 0 || lead > n_frames) return "lead outside 0..n_frames";
    if (stats < 1u || stats > kLagAll) return "no statistic (or an unknown one) requested";
    if (!pairs_address || !count_address) return "null pointer";
    if ((sums_address | pairs_address | count_address) & 7u) return "U64 outputs must be 8-byte aligned";
    if (maxdiff_address & (pix - 1u)) return "the U16 maxdiff plane must be 2-byte aligned";
    pl.stats = stats;
    pl.instance = kLagInstanceOf(stats);
    pl.lag = (uint32_t)lag;
    pl.lead = (uint32_t)lead;
    pl.first_pair = pl.lead > pl.lag ? pl.lead : pl.lag;
    // segments that count a pair: those reaching past first_pair; each but the first decodes lag history frames again
    const uint32_t active = pl.first_pair < (uint32_t)n_frames ? pl.proj.segments - pl.first_pair / pl.proj.fps : 0u;
    pl.history = active > 1u ? (active - 1u) * pl.lag : 0u;
    pl.proj.workspace = lag_workspace_bytes(stats, pl.proj.segments, (uint64_t)rw * (uint64_t)rh, pix);
    return nullptr;
}

static int lag_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead, unsigned stats,
                           uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                           uint64_t count_address, int n_cu, uint32_t pix, dbde_hip_project_lag_plan_t *plan) {
    LagPlan pl;
    if (!plan || plan_lag(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums_address, maxdiff_address, pairs_address,
                          count_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.proj.roi.tx0;
    plan->tile_y = (int32_t)pl.proj.roi.ty0;
    plan->tiles_x = (int32_t)pl.proj.roi.ntx;
    plan->tiles_y = (int32_t)pl.proj.roi.nty;
    plan->chunks_per_frame = pl.proj.roi.dg.cpf;
    plan->chunk_tiles = pl.proj.roi.dg.ct;
    plan->chunk_pieces = pl.proj.roi.dg.ct == pl.proj.roi.g.w || pl.proj.roi.dg.pieces > 1u ? pl.proj.roi.dg.pieces : 0u;
    plan->index_split = pl.proj.roi.split;
    plan->threads = kProjThreads;
    plan->pieces_x = pl.proj.pieces;
    plan->segments = pl.proj.segments;
    plan->frames_per_segment = pl.proj.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->planes = (uint32_t)__builtin_popcount(pl.stats);
    plan->grid = pl.proj.grid;
    plan->combine_grid = pl.proj.combine_grid;
    plan->workspace_bytes = pl.proj.workspace;
    plan->lds_bytes = kLagLdsBytes;
    plan->instance = pl.instance;
    plan->first_frame = pl.first_pair - pl.lag;
    plan->history_frames = pl.history;
    plan->first_pair = pl.first_pair;
    return DBDE_HIP_OK;
}

int dbde_hip_project_lag_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead,
                              unsigned stats, uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                              uint64_t count_address, int n_cu, dbde_hip_project_lag_plan_t *plan) {
    return lag_plan_common(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums_address, maxdiff_address,
                           pairs_address, count_address, n_cu, 1u, plan);
}

int dbde16_hip_project_lag_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead,
                                unsigned stats, uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                                uint64_t count_address, int n_cu, dbde_hip_project_lag_plan_t *plan) {
    return lag_plan_common(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums_address, maxdiff_address,
                           pairs_address, count_address, n_cu, 2u, plan);
}

// Both lag projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot 2.
// d_maxdiff holds U8 (pix 1) or U16 (pix 2) pixels.
static int lag_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                      const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                      int lag, int lead, int accumulate, uint64_t *d_product, uint64_t *d_pairsum, uint64_t *d_absdiff,
                      uint64_t *d_sqdiff, void *d_maxdiff, uint64_t *d_pairs, uint64_t *d_count,
                      dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_product ? kLagProduct : 0u) | (d_pairsum ? kLagPairSum : 0u) | (d_absdiff ? kLagAbsDiff : 0u) |
                           (d_sqdiff ? kLagSqDiff : 0u) | (d_maxdiff ? kLagMaxDiff : 0u);
    const uint64_t sums = reinterpret_cast<uintptr_t>(d_product) | reinterpret_cast<uintptr_t>(d_pairsum) |
                          reinterpret_cast<uintptr_t>(d_absdiff) | reinterpret_cast<uintptr_t>(d_sqdiff);
    LagPlan pl;
    if (const char *why = plan_lag(W, H, n_frames, x0, y0, rw, rh, lag, lead, stats, sums,
                                   reinterpret_cast<uintptr_t>(d_maxdiff), reinterpret_cast<uintptr_t>(d_pairs),
                                   reinterpret_cast<uintptr_t>(d_count), ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, lag=%d lead=%d)", name, why, W,
                    H, n_frames, rw, rh, x0, y0, lag, lead);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.proj.roi.dg, pix,
                           pl.proj.roi.split);
        if (rc) return rc;
    }
    LagParams p;
    memset(&p, 0, sizeof p);
    if (pl.proj.workspace) {   // the partials in lag_workspace_bytes' order, each 16-byte aligned
        int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.proj.workspace, 1);
        if (rc) return rc;
        const uint64_t pixels = (uint64_t)rw * (uint64_t)rh;
        uint8_t *w = ctx->proj_ws;
        if (d_product) { p.ws_product = w; w += lag_partial_bytes(kLagProduct, pl.proj.segments, pixels, pix); }
        if (d_pairsum) { p.ws_pairsum = w; w += lag_partial_bytes(kLagPairSum, pl.proj.segments, pixels, pix); }
        if (d_absdiff) { p.ws_absdiff = reinterpret_cast<uint32_t *>(w); w += lag_partial_bytes(kLagAbsDiff, pl.proj.segments, pixels, pix); }
        if (d_sqdiff) { p.ws_sqdiff = w; w += lag_partial_bytes(kLagSqDiff, pl.proj.segments, pixels, pix); }
        if (d_maxdiff) { p.ws_maxdiff = w; w += lag_partial_bytes(kLagMaxDiff, pl.proj.segments, pixels, pix); }
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.proj.roi.g.T;
    p.w = pl.proj.roi.g.w;
    p.geom = pl.proj.roi.dg;
    p.tx0 = pl.proj.roi.tx0;
    p.ty0 = pl.proj.roi.ty0;
    p.rows = pl.proj.rows;
    p.pieces = pl.proj.pieces;
    p.segments = pl.proj.segments;
    p.fps = pl.proj.fps;
    p.accumulate = accumulate ? 1 : 0;
    p.lag = pl.lag;
    p.lead = pl.lead;
    p.out_product = d_product;
    p.out_pairsum = d_pairsum;
    p.out_absdiff = d_absdiff;
    p.out_sqdiff = d_sqdiff;
    p.out_maxdiff = d_maxdiff;
    p.out_pairs = d_pairs;
    p.out_count = d_count;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_lag(p, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_lag(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         int lag, int lead, int accumulate, uint64_t *d_product, uint64_t *d_pairsum,
                         uint64_t *d_absdiff, uint64_t *d_sqdiff, uint8_t *d_maxdiff, uint64_t *d_pairs,
                         uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return lag_common(ctx, "project_lag", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh, lag,
                      lead, accumulate, d_product, d_pairsum, d_absdiff, d_sqdiff, d_maxdiff, d_pairs, d_count, d_results);
}

int dbde16_hip_project_lag(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           int lag, int lead, int accumulate, uint64_t *d_product, uint64_t *d_pairsum,
                           uint64_t *d_absdiff, uint64_t *d_sqdiff, uint16_t *d_maxdiff, uint64_t *d_pairs,
                           uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return lag_common(ctx, "project_lag16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                      lag, lead, accumulate, d_product, d_pairsum, d_absdiff, d_sqdiff, d_maxdiff, d_pairs, d_count,
                      d_results);
}

// ---- registered projections --------------------------------------------------------------
// The sizes and the index geometry are plan_roi's for the window at (0, 0), whose tile rows are the bands of 8 output
// rows; the pieces own kRProjColsOf(pix) output columns, and the segment rule is plan_project's applied to that grid.
static const char *plan_rproject(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu, uint32_t pix,
                                 ProjectPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, 0, 0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    if (stats < 1u || stats > kProjAll) return "no statistic (or an unknown one) requested";
    pl.stats = stats;
    pl.pieces = ((uint32_t)rw + kRProjColsOf(pix) - 1u) / kRProjColsOf(pix);
    return plan_project_segments(n_frames, rw, rh, n_cu, pix, pl);
}

static int rproject_plan_common(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu, uint32_t pix,
                                dbde_hip_project_registered_plan_t *plan) {
    ProjectPlan pl;
    if (!plan || plan_rproject(W, H, n_frames, rw, rh, stats, n_cu, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->threads = kProjThreads;
    plan->piece_cols = kRProjColsOf(pix);
    plan->pieces_x = pl.pieces;
    plan->band_rows = kRProjBandRows;
    plan->bands = pl.rows;
    plan->segments = pl.segments;
    plan->frames_per_segment = pl.fps;
    plan->max_frames_per_segment = kProjMaxFramesPerSegment;
    plan->grid = pl.grid;
    plan->combine_grid = pl.combine_grid;
    plan->workspace_bytes = pl.workspace;
    plan->lds_bytes = kRProjLdsBytes;
    plan->instance = kRProjInstanceOf(stats);
    return DBDE_HIP_OK;
}

int dbde_hip_project_registered_plan(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu,
                                     dbde_hip_project_registered_plan_t *plan) {
    return rproject_plan_common(W, H, n_frames, rw, rh, stats, n_cu, 1u, plan);
}

int dbde16_hip_project_registered_plan(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu,
                                       dbde_hip_project_registered_plan_t *plan) {
    return rproject_plan_common(W, H, n_frames, rw, rh, stats, n_cu, 2u, plan);
}

// Both registered projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the projection kernels in slot
// 2.  d_max / d_min hold U8 (pix 1) or U16 (pix 2) pixels.
static int rproject_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                           size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw,
                           int rh, const int32_t *d_origins, int accumulate, void *d_max, void *d_min, uint64_t *d_sum,
                           uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                           dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_max ? kProjMax : 0u) | (d_min ? kProjMin : 0u) | (d_sum ? kProjSum : 0u) |
                           (d_sumsq ? kProjSumSq : 0u);
    ProjectPlan pl;
    if (const char *why = plan_rproject(W, H, n_frames, rw, rh, stats, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d)", name, why, W, H, n_frames, rw, rh);
    if (!d_stream || !d_frame_offsets || !d_count || !d_origins)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if ((reinterpret_cast<uintptr_t>(d_sum) | reinterpret_cast<uintptr_t>(d_sumsq) |
         reinterpret_cast<uintptr_t>(d_count)) & 7u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_max) | reinterpret_cast<uintptr_t>(d_min)) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 outputs must be 2-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_origins) | reinterpret_cast<uintptr_t>(d_origins_used)) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins must be 4-byte aligned", name);
    if (n_frames == 0 && accumulate) return DBDE_HIP_OK;   // nothing to add
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
        if (rc) return rc;
    }
    RProjParams rp;
    memset(&rp, 0, sizeof rp);
    ProjParams &p = rp.pj;
    if (pl.workspace) {   // the partials in project_workspace_bytes' order: max, min, sum, sumsq, each 16-byte aligned
        int rc = grow(ctx, ctx->proj_ws, ctx->proj_ws_bytes, (size_t)pl.workspace, 1);
        if (rc) return rc;
        const uint64_t n = (uint64_t)pl.segments * (uint64_t)rw * (uint64_t)rh;
        const uint64_t mm = (pix * n + 15u) & ~(uint64_t)15, u32 = (4u * n + 15u) & ~(uint64_t)15;
        const uint64_t sq = pix == 1u ? u32 : (8u * n + 15u) & ~(uint64_t)15;
        uint8_t *w = ctx->proj_ws;
        if (d_max) { p.ws_max = w; w += mm; }
        if (d_min) { p.ws_min = w; w += mm; }
        if (d_sum) { p.ws_sum = reinterpret_cast<uint32_t *>(w); w += u32; }
        if (d_sumsq) { p.ws_sumsq = reinterpret_cast<uint32_t *>(w); w += sq; }
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.roi.g.T;
    p.w = pl.roi.g.w;
    p.geom = pl.roi.dg;
    p.rows = pl.rows;
    p.pieces = pl.pieces;
    p.segments = pl.segments;
    p.fps = pl.fps;
    p.accumulate = accumulate ? 1 : 0;
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    p.out_count = d_count;
    rp.origins = d_origins;
    rp.origins_used = d_origins_used;
    rp.W = W;
    rp.H = H;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_rproject(rp, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_registered(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw, int rh,
                                const int32_t *d_origins, int accumulate, uint8_t *d_max, uint8_t *d_min,
                                uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                                dbde_hip_frame_result *d_results) {
    return rproject_common(ctx, "project_registered", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, rw, rh,
                           d_origins, accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_origins_used, d_results);
}

int dbde16_hip_project_registered(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                  const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw, int rh,
                                  const int32_t *d_origins, int accumulate, uint16_t *d_max, uint16_t *d_min,
                                  uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                                  dbde_hip_frame_result *d_results) {
    return rproject_common(ctx, "project_registered16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, rw,
                           rh, d_origins, accumulate, d_max, d_min, d_sum, d_sumsq, d_count, d_origins_used, d_results);
}

// ---- grouped temporal projections --------------------------------------------------------
struct GroupsPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t stats;
    uint32_t pieces, rows, runs, gpr;
    uint64_t grid;
    uint64_t max_bytes, min_bytes, sum_bytes, sumsq_bytes, counts_bytes;
};
// Groups per run: a run is cut only to fill the device (about 4 workgroups per CU, project's segment rule with whole
// groups as the unit) and never below kGProjMinFramesPerRun frames, which would start a pipeline for a handful of
// frames.  The ragged form's groups live on the device: it counts n_frames / n_groups frames per group.
// The *_addr arguments are the call's output pointers (0 = NULL); only their alignment is looked at.
static constexpr uint32_t kGProjMinFramesPerRun = 32;
static const char *plan_groups(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                               bool has_starts, int n_groups, int sum_type, int accumulate, uint64_t max_addr,
                               uint64_t min_addr, uint64_t sum_addr, uint64_t sumsq_addr, uint64_t counts_addr,
                               int n_cu, uint32_t pix, GroupsPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    const unsigned stats = (max_addr ? kProjMax : 0u) | (min_addr ? kProjMin : 0u) | (sum_addr ? kProjSum : 0u) |
                           (sumsq_addr ? kProjSumSq : 0u);
    if (!stats) return "no plane requested";
    if (!counts_addr) return "d_counts is required";
    if (accumulate != 0 && accumulate != 1) return "accumulate must be 0 or 1";
    if (sum_type != DBDE_HIP_SUM_U32 && sum_type != DBDE_HIP_SUM_U16) return "unknown sum_type";
    if (has_starts == (group_frames != 0)) return "exactly one of group_frames and d_group_starts must be given";
    if (n_groups < 0) return "n_groups is negative";
    const uint64_t n = (uint64_t)n_frames;
    uint64_t max_group;   // frames the largest group can hold
    if (has_starts) {
        if (n_groups < 1) return "the ragged form needs n_groups >= 1";
        if (n > kGProjMaxGroupFrames) return "the ragged form needs n_frames <= 65,536";
        max_group = n;
    } else {
        if (group_frames < 1 || (uint32_t)group_frames > kGProjMaxGroupFrames) return "group_frames must be 1..65,536";
        if ((uint64_t)n_groups != (n + (uint64_t)group_frames - 1u) / (uint64_t)group_frames)
            return "n_groups must equal ceil(n_frames / group_frames)";
        max_group = (uint64_t)group_frames;
    }
    if (sum_type == DBDE_HIP_SUM_U16) {
        if (pix != 1u) return "DBDE16 sums are U32 only";
        if (max_group > kGProjMaxGroupFramesU16) return "a U16 sum needs groups of at most 257 frames";
        if (accumulate) return "a U16 sum cannot accumulate";
    }
    if ((max_addr | min_addr) & (pix - 1u)) return "U16 planes must be 2-byte aligned";
    if (sum_addr & (sum_type == DBDE_HIP_SUM_U16 ? 1u : 3u)) return "d_sum is misaligned";
    if (sumsq_addr & 7u) return "d_sumsq must be 8-byte aligned";
    if (counts_addr & 3u) return "d_counts must be 4-byte aligned";
    pl.stats = stats;
    const uint32_t tiles = kProjTilesOf(pix);
    pl.pieces = (pl.roi.ntx + tiles - 1u) / tiles;
    pl.rows = pl.roi.nty;
    const uint64_t base = (uint64_t)pl.pieces * pl.rows, ng = (uint64_t)n_groups;
    const uint64_t target = 4ull * (uint64_t)(n_cu > 0 ? n_cu : 1);
    uint64_t runs = base >= target ? 1u : (target + base - 1u) / base;
    uint64_t per_group = has_starts ? (ng ? n / ng : 0u) : (uint64_t)group_frames;   // frames of a group (ragged: the mean)
    if (per_group < 1u) per_group = 1u;
    const uint64_t min_gpr = (kGProjMinFramesPerRun + per_group - 1u) / per_group;
    uint64_t gpr = ng ? (ng + runs - 1u) / runs : 1u;
    if (gpr < min_gpr) gpr = min_gpr;
    if (gpr > ng && ng) gpr = ng;
    if (gpr < 1u) gpr = 1u;
    runs = ng ? (ng + gpr - 1u) / gpr : 0u;   // no empty run
    pl.runs = (uint32_t)runs;
    pl.gpr = (uint32_t)gpr;
    pl.grid = base * runs;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t plane = (uint64_t)rw * (uint64_t)rh * ng;
    pl.max_bytes = (stats & kProjMax) ? pix * plane : 0u;
    pl.min_bytes = (stats & kProjMin) ? pix * plane : 0u;
    pl.sum_bytes = (stats & kProjSum) ? (sum_type == DBDE_HIP_SUM_U16 ? 2u : 4u) * plane : 0u;
    pl.sumsq_bytes = (stats & kProjSumSq) ? 8u * plane : 0u;
    pl.counts_bytes = 4u * ng;
    return nullptr;
}

static int groups_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                              int has_group_starts, int n_groups, int sum_type, int accumulate, uint64_t max_address,
                              uint64_t min_address, uint64_t sum_address, uint64_t sumsq_address,
                              uint64_t counts_address, int n_cu, uint32_t pix, dbde_hip_project_groups_plan_t *plan) {
    GroupsPlan pl;
    if (!plan || (has_group_starts != 0 && has_group_starts != 1) ||
        plan_groups(W, H, n_frames, x0, y0, rw, rh, group_frames, has_group_starts != 0, n_groups, sum_type, accumulate,
                    max_address, min_address, sum_address, sumsq_address, counts_address, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->threads = kProjThreads;
    plan->pieces_x = pl.pieces;
    plan->runs = pl.runs;
    plan->groups_per_run = pl.gpr;
    plan->max_group_frames = kGProjMaxGroupFrames;
    plan->stats = pl.stats;
    plan->grid = pl.grid;
    plan->sum_bytes = pl.sum_bytes;
    plan->max_bytes = pl.max_bytes;
    plan->min_bytes = pl.min_bytes;
    plan->sumsq_bytes = pl.sumsq_bytes;
    plan->counts_bytes = pl.counts_bytes;
    plan->workspace_bytes = 0;
    return DBDE_HIP_OK;
}

int dbde_hip_project_groups_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                                 int has_group_starts, int n_groups, int sum_type, int accumulate, uint64_t max_address,
                                 uint64_t min_address, uint64_t sum_address, uint64_t sumsq_address,
                                 uint64_t counts_address, int n_cu, dbde_hip_project_groups_plan_t *plan) {
    return groups_plan_common(W, H, n_frames, x0, y0, rw, rh, group_frames, has_group_starts, n_groups, sum_type,
                              accumulate, max_address, min_address, sum_address, sumsq_address, counts_address, n_cu, 1u,
                              plan);
}

int dbde16_hip_project_groups_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int group_frames,
                                   int has_group_starts, int n_groups, int sum_type, int accumulate, uint64_t max_address,
                                   uint64_t min_address, uint64_t sum_address, uint64_t sumsq_address,
                                   uint64_t counts_address, int n_cu, dbde_hip_project_groups_plan_t *plan) {
    return groups_plan_common(W, H, n_frames, x0, y0, rw, rh, group_frames, has_group_starts, n_groups, sum_type,
                              accumulate, max_address, min_address, sum_address, sumsq_address, counts_address, n_cu, 2u,
                              plan);
}

// Both grouped projections: the index (pix: 1 = DBDE, 2 = DBDE16) in timing slot 1, the grouped kernel in slot 2.
static int project_groups_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                 size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                                 int x0, int y0, int rw, int rh, int group_frames, const uint32_t *d_group_starts,
                                 int n_groups, int sum_type, int accumulate, void *d_max, void *d_min, void *d_sum,
                                 uint64_t *d_sumsq, uint32_t *d_counts, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    GroupsPlan pl;
    if (const char *why = plan_groups(W, H, n_frames, x0, y0, rw, rh, group_frames, d_group_starts != nullptr, n_groups,
                                      sum_type, accumulate, reinterpret_cast<uintptr_t>(d_max),
                                      reinterpret_cast<uintptr_t>(d_min), reinterpret_cast<uintptr_t>(d_sum),
                                      reinterpret_cast<uintptr_t>(d_sumsq), reinterpret_cast<uintptr_t>(d_counts),
                                      ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d, g=%d groups=%d)", name, why, W,
                    H, n_frames, rw, rh, x0, y0, group_frames, n_groups);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_groups == 0) return DBDE_HIP_OK;   // (uniform form, n_frames == 0)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
        if (rc) return rc;
    }
    GProjParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.roi.g.T;
    p.w = pl.roi.g.w;
    p.geom = pl.roi.dg;
    p.tx0 = pl.roi.tx0;
    p.ty0 = pl.roi.ty0;
    p.rows = pl.rows;
    p.pieces = pl.pieces;
    p.runs = pl.runs;
    p.gpr = pl.gpr;
    p.n_groups = (uint32_t)n_groups;
    p.group_frames = (uint32_t)group_frames;
    p.group_starts = d_group_starts;
    p.accumulate = accumulate;
    p.sum16 = sum_type == DBDE_HIP_SUM_U16 ? 1u : 0u;
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    p.out_counts = d_counts;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_gproject(p, pl.stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_project_groups(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                            int group_frames, const uint32_t *d_group_starts, int n_groups, int sum_type, int accumulate,
                            uint8_t *d_max, uint8_t *d_min, void *d_sum, uint64_t *d_sumsq, uint32_t *d_counts,
                            dbde_hip_frame_result *d_results) {
    return project_groups_common(ctx, "project_groups", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                 y0, rw, rh, group_frames, d_group_starts, n_groups, sum_type, accumulate, d_max, d_min,
                                 d_sum, d_sumsq, d_counts, d_results);
}

int dbde16_hip_project_groups(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                              int group_frames, const uint32_t *d_group_starts, int n_groups, int sum_type, int accumulate,
                              uint16_t *d_max, uint16_t *d_min, uint32_t *d_sum, uint64_t *d_sumsq, uint32_t *d_counts,
                              dbde_hip_frame_result *d_results) {
    return project_groups_common(ctx, "project_groups16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames,
                                 x0, y0, rw, rh, group_frames, d_group_starts, n_groups, sum_type, accumulate, d_max,
                                 d_min, d_sum, d_sumsq, d_counts, d_results);
}

// ---- region traces ----------------------------------------------------------------------------------------
struct dbde_hip_trace_map {
    dbde_hip_ctx *ctx;
    dbde_hip_trace_map_info_t info;
    uint8_t *dev;                     // one allocation: the layout of trace_map_layout
    const uint32_t *span_first[2];    // [pix - 1]: first active tile of each span, [spans + 1]
    uint32_t spans_x[2], spans[2];
    const uint32_t *tile_pos, *tile_kind;
    const uint16_t *blocks;
    const uint64_t *pixels;
};

namespace {

// The host side of a trace map: the active tiles in tile order, their words (the label of a whole tile, kTraceMixed |
// block of a mixed one), the mixed tiles' label blocks, the per-label pixel counts and each pixel size's spans.
struct HostTraceMap {
    dbde_hip_trace_map_info_t info;
    std::vector<uint32_t> pos, kind, span_first[2];
    std::vector<uint16_t> blocks;
    std::vector<uint64_t> pixels;
    uint32_t spans_x[2];
};

// nullptr when the labels are good, else what is wrong.  full: also the tile lists, blocks and spans.
const char *trace_classify(const int32_t *labels, int W, int H, int n_labels, HostTraceMap &m, bool full) {
    Geometry g;
    if (!labels) return "null labels";
    if (!geometry(W, H, g)) return "bad frame size";
    if (n_labels < 1 || n_labels > 65535) return "n_labels outside [1, 65535]";
    memset(&m.info, 0, sizeof m.info);
    m.info.W = W;
    m.info.H = H;
    m.info.n_labels = (uint32_t)n_labels;
    m.info.tiles = g.T;
    m.pixels.assign((size_t)n_labels, 0);
    for (size_t i = 0; i < g.pixels; i++)
        if (labels[i] < 0 || labels[i] > n_labels) return "a label outside [0, n_labels]";
    uint16_t blk[64];
    for (uint32_t ty = 0; ty < g.h; ty++) {
        for (uint32_t tx = 0; tx < g.w; tx++) {
            const uint32_t x0 = 8u * tx, y0 = 8u * ty;
            const uint32_t vw = (uint32_t)W - x0 < 8u ? (uint32_t)W - x0 : 8u, vh = (uint32_t)H - y0 < 8u ? (uint32_t)H - y0 : 8u;
            bool any = false, same = true;
            const int32_t first = labels[(size_t)y0 * W + x0];
            for (uint32_t y = 0; y < 8; y++) {
                for (uint32_t x = 0; x < 8; x++) {
                    int32_t l = 0;
                    if (y < vh && x < vw) {
                        l = labels[(size_t)(y0 + y) * W + x0 + x];
                        if (l) m.pixels[l - 1]++;
                        same = same && l == first;
                    }
                    any = any || l != 0;
                    blk[8 * y + x] = (uint16_t)l;
                }
            }
            if (!any) continue;
            const bool whole = same && vw == 8u && vh == 8u;
            m.info.tiles_active++;
            if (whole) m.info.tiles_whole++;
            else m.info.tiles_mixed++;
            if (!full) continue;
            m.pos.push_back(ty * g.w + tx);
            if (whole) {
                m.kind.push_back((uint32_t)first);
            } else {
                m.kind.push_back(kTraceMixed | (uint32_t)(m.blocks.size() / 64u));
                m.blocks.insert(m.blocks.end(), blk, blk + 64);
            }
        }
    }
    if (!full) return nullptr;
    for (uint32_t pix = 1; pix <= 2u; pix++) {
        const uint32_t K = kTraceTilesOf(pix), sx = (g.w + K - 1u) / K;
        std::vector<uint32_t> &sf = m.span_first[pix - 1u];
        m.spans_x[pix - 1u] = sx;
        sf.resize((size_t)sx * g.h + 1u);
        size_t a = 0;
        for (uint32_t s = 0; s < sx * g.h; s++) {   // spans in stream order: tiles [ty * w + (s % sx) * K, + K) of row ty
            const uint32_t ty = s / sx, p0 = ty * g.w + (s - ty * sx) * K;
            while (a < m.pos.size() && m.pos[a] < p0) a++;
            sf[s] = (uint32_t)a;
        }
        sf[(size_t)sx * g.h] = (uint32_t)m.pos.size();
    }
    return nullptr;
}

// Byte offsets of the device map: [span_first pix 1][span_first pix 2][tile_pos][tile_kind][blocks][pixels], each
// 16-byte aligned.
struct TraceMapLayout {
    size_t sf1, sf2, pos, kind, blocks, pixels, total;
};
TraceMapLayout trace_map_layout(const HostTraceMap &m) {
    auto up = [](size_t v) { return (v + 15u) & ~(size_t)15; };
    TraceMapLayout l;
    l.sf1 = 0;
    l.sf2 = l.sf1 + up(4u * m.span_first[0].size());
    l.pos = l.sf2 + up(4u * m.span_first[1].size());
    l.kind = l.pos + up(4u * m.pos.size());
    l.blocks = l.kind + up(4u * m.kind.size());
    l.pixels = l.blocks + up(2u * m.blocks.size());
    l.total = l.pixels + up(8u * m.pixels.size());
    return l;
}

}  // namespace

int dbde_hip_trace_map_summary(const int32_t *labels, int W, int H, int n_labels, dbde_hip_trace_map_info_t *info,
                               uint64_t *pixels) {
    HostTraceMap m;
    if (trace_classify(labels, W, H, n_labels, m, true)) return DBDE_HIP_ERR_ARG;
    m.info.device_bytes = trace_map_layout(m).total;
    if (info) *info = m.info;
    if (pixels) memcpy(pixels, m.pixels.data(), 8u * m.pixels.size());
    return DBDE_HIP_OK;
}

int dbde_hip_trace_map_create(dbde_hip_ctx *ctx, const int32_t *labels, int W, int H, int n_labels,
                              dbde_hip_trace_map **out) {
    if (!ctx || !out) return fail(ctx, DBDE_HIP_ERR_ARG, "trace_map_create: null pointer");
    *out = nullptr;
    HostTraceMap m;
    if (const char *why = trace_classify(labels, W, H, n_labels, m, true))
        return fail(ctx, DBDE_HIP_ERR_ARG, "trace_map_create: %s (W=%d H=%d n_labels=%d)", why, W, H, n_labels);
    const TraceMapLayout l = trace_map_layout(m);
    m.info.device_bytes = l.total;
    std::vector<uint8_t> host(l.total, 0);
    auto put = [&](size_t at, const void *src, size_t n) { if (n) memcpy(host.data() + at, src, n); };
    put(l.sf1, m.span_first[0].data(), 4u * m.span_first[0].size());
    put(l.sf2, m.span_first[1].data(), 4u * m.span_first[1].size());
    put(l.pos, m.pos.data(), 4u * m.pos.size());
    put(l.kind, m.kind.data(), 4u * m.kind.size());
    put(l.blocks, m.blocks.data(), 2u * m.blocks.size());
    put(l.pixels, m.pixels.data(), 8u * m.pixels.size());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *dev = nullptr;
    HIP_TRY(ctx, hipMalloc(&dev, l.total));
    hipError_t e = hipMemcpyAsync(dev, host.data(), l.total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return fail(ctx, DBDE_HIP_ERR_HIP, "trace_map_create: copy failed: %s", hipGetErrorString(e));
    }
    dbde_hip_trace_map *tm = new dbde_hip_trace_map;
    uint8_t *d = static_cast<uint8_t *>(dev);
    tm->ctx = ctx;
    tm->info = m.info;
    tm->dev = d;
    tm->span_first[0] = reinterpret_cast<const uint32_t *>(d + l.sf1);
    tm->span_first[1] = reinterpret_cast<const uint32_t *>(d + l.sf2);
    for (int k = 0; k < 2; k++) {
        tm->spans_x[k] = m.spans_x[k];
        tm->spans[k] = (uint32_t)(m.span_first[k].size() - 1u);
    }
    tm->tile_pos = reinterpret_cast<const uint32_t *>(d + l.pos);
    tm->tile_kind = reinterpret_cast<const uint32_t *>(d + l.kind);
    tm->blocks = reinterpret_cast<const uint16_t *>(d + l.blocks);
    tm->pixels = reinterpret_cast<const uint64_t *>(d + l.pixels);
    *out = tm;
    return DBDE_HIP_OK;
}

void dbde_hip_trace_map_destroy(dbde_hip_trace_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);   // queued traces may still read it
    (void)hipFree(m->dev);
    delete m;
}

int dbde_hip_trace_map_info(const dbde_hip_trace_map *m, dbde_hip_trace_map_info_t *info) {
    if (!m || !info) return DBDE_HIP_ERR_ARG;
    *info = m->info;
    return DBDE_HIP_OK;
}

const uint64_t *dbde_hip_trace_map_pixels(const dbde_hip_trace_map *m) { return m ? m->pixels : nullptr; }

namespace {

struct TracePlan {
    Geometry g;
    DecGeom dg;                       // the index's chunks (roi_index_geometry)
    uint32_t split, tiles, spans_x, spans, segments, fps;
    uint64_t grid, row_grid, workspace;
};
// Frames per segment: segments only fill the device (about 4 busy workgroups per CU, the busy spans counted as the
// fewest that can hold the active tiles) and never hold fewer than kTraceMinFramesPerSegment frames.  Segments cost no
// extra traffic: each (frame, span) is traced by one workgroup.
constexpr uint32_t kTraceMinFramesPerSegment = 16;
const char *plan_trace(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                       uint32_t pix, TracePlan &pl) {
    if (!info) return "null map info";
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, pl.g)) return "bad frame size";
    if (info->W != W || info->H != H) return "W / H differ from the map's";
    if (info->n_labels < 1u || info->n_labels > 65535u || info->tiles != pl.g.T || info->tiles_active > pl.g.T)
        return "map info does not describe a map of this frame size";
    if (stats < 1u || stats > kProjAll) return "no statistic (or an unknown one) requested";
    if (n_cu < 1) return "n_cu < 1";
    pl.dg = roi_index_geometry(pl.g.w, pl.g.h);
    if (pl.dg.cpf > kMaxChunksPerFrame) return "frame too large";
    if ((uint64_t)n_frames * (pl.dg.cpf + 1u) >= (1ull << 31)) return "too many chunks in one call";
    pl.split = index_split_for(n_frames, pl.dg.cpf);
    pl.tiles = kTraceTilesOf(pix);
    pl.spans_x = (pl.g.w + pl.tiles - 1u) / pl.tiles;
    pl.spans = pl.spans_x * pl.g.h;
    const uint64_t n = (uint64_t)n_frames;
    const uint64_t busy = info->tiles_active ? (info->tiles_active + pl.tiles - 1u) / pl.tiles : 1u;
    const uint64_t target = 4ull * (uint64_t)n_cu;
    uint64_t seg = busy >= target ? 1u : (target + busy - 1u) / busy;
    const uint64_t by_len = (n + kTraceMinFramesPerSegment - 1u) / kTraceMinFramesPerSegment;
    if (seg > by_len) seg = by_len;
    if (seg < 1u) seg = 1u;
    uint64_t fps = (n + seg - 1u) / seg;
    if (fps > 0u) seg = (n + fps - 1u) / fps;   // no empty segment
    pl.segments = (uint32_t)seg;
    pl.fps = (uint32_t)fps;
    pl.grid = (uint64_t)pl.spans * seg;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t rows = n * info->n_labels;
    pl.row_grid = (rows + kTraceRowThreads - 1u) / kTraceRowThreads;
    if (pl.row_grid >= (1ull << 31)) return "too many outputs in one call";
    const uint64_t ws = (4u * rows + 15u) & ~(uint64_t)15;
    pl.workspace = ((stats & kProjMax) ? ws : 0u) + ((stats & kProjMin) ? ws : 0u);
    return nullptr;
}

int trace_plan_common(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                      uint32_t pix, dbde_hip_trace_plan_t *plan) {
    TracePlan pl;
    if (!plan || plan_trace(W, H, n_frames, info, stats, n_cu, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->chunks_per_frame = pl.dg.cpf;
    plan->chunk_tiles = pl.dg.ct;
    plan->chunk_pieces = pl.dg.ct == pl.g.w || pl.dg.pieces > 1u ? pl.dg.pieces : 0u;
    plan->index_split = pl.split;
    plan->threads = kTraceThreads;
    plan->tiles_per_workgroup = pl.tiles;
    plan->spans_x = pl.spans_x;
    plan->spans = pl.spans;
    plan->segments = pl.segments;
    plan->frames_per_segment = pl.fps;
    plan->grid = pl.grid;
    plan->row_grid = pl.row_grid;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

// Both trace entry points: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the trace
// kernels in slot 2.  d_max / d_min hold U8 (pix 1) or U16 (pix 2) values.
int traces_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                  const uint64_t *d_frame_offsets, int W, int H, int n_frames, const dbde_hip_trace_map *map,
                  void *d_max, void *d_min, uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    if (!map) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null map", name);
    if (map->ctx != ctx) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the map belongs to another context", name);
    const unsigned stats = (d_max ? kProjMax : 0u) | (d_min ? kProjMin : 0u) | (d_sum ? kProjSum : 0u) |
                           (d_sumsq ? kProjSumSq : 0u);
    TracePlan pl;
    if (const char *why = plan_trace(W, H, n_frames, &map->info, stats, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, map %dx%d)", name, why, W, H, n_frames,
                    map->info.W, map->info.H);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if ((reinterpret_cast<uintptr_t>(d_sum) | reinterpret_cast<uintptr_t>(d_sumsq)) & 7u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_max) | reinterpret_cast<uintptr_t>(d_min)) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 outputs must be 2-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, pix, pl.split);
    if (rc) return rc;
    TraceParams p;
    memset(&p, 0, sizeof p);
    if (pl.workspace) {   // U32 max, then U32 min, [n_frames][n_labels] each, 16-byte aligned
        rc = grow(ctx, ctx->trace_ws, ctx->trace_ws_bytes, (size_t)pl.workspace, 1);
        if (rc) return rc;
        const uint64_t ws = (4u * (uint64_t)n_frames * map->info.n_labels + 15u) & ~(uint64_t)15;
        uint8_t *w = ctx->trace_ws;
        if (d_max) { p.ws_max = reinterpret_cast<uint32_t *>(w); w += ws; }
        if (d_min) p.ws_min = reinterpret_cast<uint32_t *>(w);
    }
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.T = pl.g.T;
    p.w = pl.g.w;
    p.geom = pl.dg;
    p.spans_x = pl.spans_x;
    p.spans = pl.spans;
    p.segments = pl.segments;
    p.fps = pl.fps;
    p.n_labels = map->info.n_labels;
    p.pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    p.span_first = map->span_first[pix - 1u];
    p.tile_pos = map->tile_pos;
    p.tile_kind = map->tile_kind;
    p.blocks = map->blocks;
    p.out_max = static_cast<uint8_t *>(d_max);
    p.out_min = static_cast<uint8_t *>(d_min);
    p.out_sum = d_sum;
    p.out_sumsq = d_sumsq;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_traces(p, stats, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

}  // namespace

int dbde_hip_trace_plan(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                        dbde_hip_trace_plan_t *plan) {
    return trace_plan_common(W, H, n_frames, info, stats, n_cu, 1u, plan);
}

int dbde16_hip_trace_plan(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                          dbde_hip_trace_plan_t *plan) {
    return trace_plan_common(W, H, n_frames, info, stats, n_cu, 2u, plan);
}

int dbde_hip_traces(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                    int W, int H, int n_frames, const dbde_hip_trace_map *map, uint8_t *d_max, uint8_t *d_min,
                    uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results) {
    return traces_common(ctx, "traces", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, map, d_max, d_min,
                         d_sum, d_sumsq, d_results);
}

int dbde16_hip_traces(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                      int W, int H, int n_frames, const dbde_hip_trace_map *map, uint16_t *d_max, uint16_t *d_min,
                      uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results) {
    return traces_common(ctx, "traces16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, map, d_max,
                         d_min, d_sum, d_sumsq, d_results);
}

// ---- per-frame histograms ---------------------------------------------------------------------------------
struct HistPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t pieces_x, pieces, segments, pps, lds_bins;
    uint64_t grid, init_grid, atomics, workspace;
};
// A segment is cut only to fill the device (about 16 workgroups per CU) and never below the pieces whose pixels
// outnumber its flush 64 times (64 * bins pixels, and at least kHistMinPieces pieces).
static constexpr uint32_t kHistMinPieces = 16;
static const char *plan_histogram(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                                  unsigned outputs, int n_cu, uint32_t pix, HistPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, pix == 2u ? kRoi16WideThreads : kRoiWideThreads))
        return why;
    const int max_shift = pix == 1u ? 7 : 15;
    if (shift < 0 || shift > max_shift) return "shift outside [0, 7] (DBDE) / [0, 15] (DBDE16)";
    const uint32_t range = (pix == 1u ? 256u : 65536u) >> shift;
    const uint32_t most = pix == 1u ? range : (range < kHistLargeBins ? range : kHistLargeBins);
    if (bins < 1 || (uint32_t)bins > most) return "bins outside [1, 256 >> shift] (DBDE) / [1, min(4096, 65536 >> shift)] (DBDE16)";
    if (outputs < 1u || outputs > 3u) return "no output (or an unknown one) requested";
    const uint32_t tiles = kHistTilesOf(pix);
    pl.pieces_x = (pl.roi.ntx + tiles - 1u) / tiles;
    pl.pieces = pl.pieces_x * pl.roi.nty;
    pl.lds_bins = kHistLdsBinsOf((uint32_t)bins);
    const uint64_t n = (uint64_t)n_frames;
    const uint64_t px_piece = 64ull * tiles;
    uint64_t min_pieces = (64ull * (uint64_t)bins + px_piece - 1u) / px_piece;
    if (min_pieces < kHistMinPieces) min_pieces = kHistMinPieces;
    const uint64_t target = 16ull * (uint64_t)(n_cu > 0 ? n_cu : 1);
    uint64_t seg = (target + (n > 0 ? n : 1) - 1u) / (n > 0 ? n : 1);
    const uint64_t by_len = (pl.pieces + min_pieces - 1u) / min_pieces;
    if (seg > by_len) seg = by_len;
    if (seg < 1u) seg = 1u;
    const uint64_t pps = (pl.pieces + seg - 1u) / seg;
    seg = (pl.pieces + pps - 1u) / pps;   // no empty segment
    pl.segments = (uint32_t)seg;
    pl.pps = (uint32_t)pps;
    pl.grid = n * seg;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    const uint64_t rows = (n > 0 ? n : 1) * (uint64_t)bins;
    pl.init_grid = (rows + kHistRowThreads - 1u) / kHistRowThreads;
    if (pl.init_grid >= (1ull << 31)) return "too many workgroups in one call";
    pl.atomics = seg * (uint64_t)bins * (uint64_t)(((outputs & 1u) ? 1u : 0u) + ((outputs & 2u) ? 1u : 0u));
    pl.workspace = n * (pl.roi.dg.cpf + 1u) * 4u + n * 4u;
    return nullptr;
}

static int histogram_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                                 unsigned outputs, int n_cu, uint32_t pix, dbde_hip_histogram_plan_t *plan) {
    HistPlan pl;
    if (!plan || n_cu < 1 || plan_histogram(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, n_cu, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->threads = kHistThreads;
    plan->tiles_per_piece = kHistTilesOf(pix);
    plan->pieces_x = pl.pieces_x;
    plan->pieces = pl.pieces;
    plan->segments = pl.segments;
    plan->pieces_per_segment = pl.pps;
    plan->lds_bins = pl.lds_bins;
    plan->lds_copies = kHistCopiesOf(pl.lds_bins);
    plan->lds_bytes = kHistLdsBytesOf(pl.lds_bins);
    plan->grid = pl.grid;
    plan->init_grid = pl.init_grid;
    plan->global_atomics_per_frame = pl.atomics;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

int dbde_hip_histogram_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                            unsigned outputs, int n_cu, dbde_hip_histogram_plan_t *plan) {
    return histogram_plan_common(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, n_cu, 1u, plan);
}

int dbde16_hip_histogram_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                              unsigned outputs, int n_cu, dbde_hip_histogram_plan_t *plan) {
    return histogram_plan_common(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, n_cu, 2u, plan);
}

// Both histograms: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the histogram kernels
// in slot 2.
static int histogram_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                            size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                            int y0, int rw, int rh, int shift, int bins, int accumulate, uint32_t *d_hist,
                            uint64_t *d_total, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned outputs = (d_hist ? 1u : 0u) | (d_total ? 2u : 0u);
    HistPlan pl;
    if (const char *why = plan_histogram(W, H, n_frames, x0, y0, rw, rh, shift, bins, outputs, ctx->n_cu, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d shift %d bins %d)", name, why,
                    W, H, n_frames, rw, rh, x0, y0, shift, bins);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (d_total && !d_count) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: d_total needs d_count", name);
    if ((reinterpret_cast<uintptr_t>(d_total) | reinterpret_cast<uintptr_t>(d_count)) & 7u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U64 outputs must be 8-byte aligned", name);
    if (reinterpret_cast<uintptr_t>(d_hist) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U32 rows must be 4-byte aligned", name);
    if (n_frames == 0 && (accumulate || !d_total)) return DBDE_HIP_OK;   // nothing to add or to reset
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_frames > 0) {
        int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
        if (rc) return rc;
    }
    HistParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.n_frames = (uint32_t)n_frames;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.T = pl.roi.g.T;
    p.w = pl.roi.g.w;
    p.geom = pl.roi.dg;
    p.tx0 = pl.roi.tx0;
    p.ty0 = pl.roi.ty0;
    p.rows = pl.roi.nty;
    p.pieces = pl.pieces_x;
    p.segments = pl.segments;
    p.pps = pl.pps;
    p.shift = (uint32_t)shift;
    p.bins = (uint32_t)bins;
    p.accumulate = accumulate ? 1 : 0;
    p.out_hist = d_hist;
    p.out_total = d_total;
    p.out_count = d_total ? d_count : nullptr;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_histogram(p, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_histogram(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                       int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins, int accumulate,
                       uint32_t *d_hist, uint64_t *d_total, uint64_t *d_count, dbde_hip_frame_result *d_results) {
    return histogram_common(ctx, "histogram", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                            rh, shift, bins, accumulate, d_hist, d_total, d_count, d_results);
}

int dbde16_hip_histogram(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         int shift, int bins, int accumulate, uint32_t *d_hist, uint64_t *d_total, uint64_t *d_count,
                         dbde_hip_frame_result *d_results) {
    return histogram_common(ctx, "histogram16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw,
                            rh, shift, bins, accumulate, d_hist, d_total, d_count, d_results);
}

// ---- binned decode -----------------------------------------------------------------------------------------
struct BinnedPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t threads, pieces, ow, oh;
    uint64_t grid, sum_bytes, mm_bytes;
};
static const char *plan_binned(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                               uint32_t pix, BinnedPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, kBinWideThreadsOf(pix))) return why;
    if (bin != 2 && bin != 4 && bin != 8) return "bin other than 2, 4, 8";
    if (x0 % bin || y0 % bin) return "window origin not a multiple of the bin";
    if (stats < 1u || stats > 7u) return "no statistic (or an unknown one) requested";
    pl.threads = pl.roi.ntx <= kBinNarrowThreads ? kBinNarrowThreads : kBinWideThreadsOf(pix);
    pl.pieces = (pl.roi.ntx + pl.threads - 1u) / pl.threads;
    pl.ow = ((uint32_t)rw + (uint32_t)bin - 1u) / (uint32_t)bin;
    pl.oh = ((uint32_t)rh + (uint32_t)bin - 1u) / (uint32_t)bin;
    pl.grid = (uint64_t)n_frames * pl.roi.nty * pl.pieces;   // below 2^31: at most plan_roi's grid_origins
    const uint64_t elems = (uint64_t)n_frames * pl.oh * pl.ow;
    pl.sum_bytes = elems * 2u * pix;
    pl.mm_bytes = elems * pix;
    return nullptr;
}

static int binned_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                              uint32_t pix, dbde_hip_binned_plan_t *plan) {
    BinnedPlan pl;
    if (!plan || plan_binned(W, H, n_frames, x0, y0, rw, rh, bin, stats, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->out_w = pl.ow;
    plan->out_h = pl.oh;
    plan->threads = pl.threads;
    plan->pieces_x = pl.pieces;
    plan->lds_bytes = kBinLdsBytesOf(pl.threads, pix);
    plan->grid = pl.grid;
    plan->sum_bytes = (stats & DBDE_HIP_BINNED_SUM) ? pl.sum_bytes : 0u;
    plan->max_bytes = (stats & DBDE_HIP_BINNED_MAX) ? pl.mm_bytes : 0u;
    plan->min_bytes = (stats & DBDE_HIP_BINNED_MIN) ? pl.mm_bytes : 0u;
    return DBDE_HIP_OK;
}

int dbde_hip_binned_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                         dbde_hip_binned_plan_t *plan) {
    return binned_plan_common(W, H, n_frames, x0, y0, rw, rh, bin, stats, 1u, plan);
}

int dbde16_hip_binned_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                           dbde_hip_binned_plan_t *plan) {
    return binned_plan_common(W, H, n_frames, x0, y0, rw, rh, bin, stats, 2u, plan);
}

// Both binned decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the binning kernel
// in slot 2.
static int decode_binned_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                                int y0, int rw, int rh, int bin, void *d_sum, void *d_max, void *d_min,
                                dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    const unsigned stats = (d_sum ? DBDE_HIP_BINNED_SUM : 0u) | (d_max ? DBDE_HIP_BINNED_MAX : 0u) | (d_min ? DBDE_HIP_BINNED_MIN : 0u);
    BinnedPlan pl;
    if (const char *why = plan_binned(W, H, n_frames, x0, y0, rw, rh, bin, stats, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d bin %d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, bin);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (reinterpret_cast<uintptr_t>(d_sum) & (2u * pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the sum plane must be %u-byte aligned", name, 2u * pix);
    if ((reinterpret_cast<uintptr_t>(d_max) | reinterpret_cast<uintptr_t>(d_min)) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: U16 planes must be 2-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;
    BinnedParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.w = pl.roi.g.w;
    p.T = pl.roi.g.T;
    p.geom = pl.roi.dg;
    p.tx0 = pl.roi.tx0;
    p.ty0 = pl.roi.ty0;
    p.rows = pl.roi.nty;
    p.pieces = pl.pieces;
    p.ow = pl.ow;
    p.oh = pl.oh;
    p.out_sum = d_sum;
    p.out_max = d_max;
    p.out_min = d_min;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_binned(p, (uint32_t)n_frames, pl.threads, pix, (uint32_t)bin, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_binned(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           int bin, uint16_t *d_sum, uint8_t *d_max, uint8_t *d_min, dbde_hip_frame_result *d_results) {
    return decode_binned_common(ctx, "decode_binned", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                y0, rw, rh, bin, d_sum, d_max, d_min, d_results);
}

int dbde16_hip_decode_binned(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                             int bin, uint32_t *d_sum, uint16_t *d_max, uint16_t *d_min,
                             dbde_hip_frame_result *d_results) {
    return decode_binned_common(ctx, "decode_binned16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                y0, rw, rh, bin, d_sum, d_max, d_min, d_results);
}

// ---- scaled float decode -------------------------------------------------------------------------------------
struct ScaledPlan {
    RoiPlan roi;                      // arguments, tile window, index geometry and launch: the window decoder's (plan_roi)
    uint32_t elem;                    // bytes of an output element
    uint64_t out_bytes;
};
static const char *plan_scaled(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type, uint32_t pix,
                               ScaledPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, kScaledWideThreadsOf(pix))) return why;
    if (out_type != DBDE_HIP_OUT_F32 && out_type != DBDE_HIP_OUT_F16 && out_type != DBDE_HIP_OUT_BF16)
        return "output type other than F32, F16, BF16";
    pl.elem = kScaledElemBytesOf((uint32_t)out_type);
    pl.out_bytes = (uint64_t)n_frames * (uint64_t)rw * (uint64_t)rh * pl.elem;
    return nullptr;
}

static int scaled_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type, uint32_t pix,
                              dbde_hip_scaled_plan_t *plan) {
    ScaledPlan pl;
    if (!plan || plan_scaled(W, H, n_frames, x0, y0, rw, rh, out_type, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->max_tiles_x = (int32_t)pl.roi.max_tx;
    plan->max_tiles_y = (int32_t)pl.roi.max_ty;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->threads = pl.roi.threads;
    plan->pieces_x = pl.roi.pieces;
    plan->lds_bytes = kScaledLdsBytesOf(pl.roi.threads, pix);
    plan->elem_bytes = pl.elem;
    plan->grid = pl.roi.grid;
    plan->grid_origins = pl.roi.grid_origins;
    plan->out_bytes = pl.out_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_scaled_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type,
                         dbde_hip_scaled_plan_t *plan) {
    return scaled_plan_common(W, H, n_frames, x0, y0, rw, rh, out_type, 1u, plan);
}

int dbde16_hip_scaled_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type,
                           dbde_hip_scaled_plan_t *plan) {
    return scaled_plan_common(W, H, n_frames, x0, y0, rw, rh, out_type, 2u, plan);
}

// Both scaled decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the scaling kernel
// in slot 2.
static int decode_scaled_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                                int y0, int rw, int rh, const int32_t *d_origins, int out_type, const float *d_dark,
                                float dark0, const float *d_gain, float gain0, void *d_out,
                                dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    ScaledPlan pl;
    if (const char *why = plan_scaled(W, H, n_frames, x0, y0, rw, rh, out_type, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d type %d)", name, why, W, H,
                    n_frames, rw, rh, x0, y0, out_type);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames > 0 && !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null output", name);
    if (reinterpret_cast<uintptr_t>(d_out) & (pl.elem - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the output must be %u-byte aligned", name, pl.elem);
    if ((reinterpret_cast<uintptr_t>(d_dark) | reinterpret_cast<uintptr_t>(d_gain)) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the maps must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;

    ScaledParams p;
    memset(&p, 0, sizeof p);
    p.roi.stream = d_stream;
    p.roi.frame_offsets = d_frame_offsets;
    p.roi.stream_bytes = stream_bytes;
    p.roi.chunk_off = ctx->chunk_off;
    p.roi.frame_ok = ctx->frame_ok;
    p.roi.origins = d_origins;
    p.roi.out = static_cast<uint8_t *>(d_out);
    p.roi.W = W;
    p.roi.H = H;
    p.roi.x0 = x0;
    p.roi.y0 = y0;
    p.roi.rw = rw;
    p.roi.rh = rh;
    p.roi.w = pl.roi.g.w;
    p.roi.h = pl.roi.g.h;
    p.roi.T = pl.roi.g.T;
    p.roi.geom = pl.roi.dg;
    p.roi.rows = d_origins ? pl.roi.max_ty : pl.roi.nty;
    p.roi.pieces = d_origins ? pl.roi.pieces : pl.roi.pieces_fixed;
    p.dark = d_dark;
    p.gain = d_gain;
    p.dark0 = dark0;
    p.gain0 = gain0;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_scaled(p, (uint32_t)n_frames, pl.roi.threads, pix, (uint32_t)out_type, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_scaled(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           const int32_t *d_origins, int out_type, const float *d_dark, float dark0, const float *d_gain,
                           float gain0, void *d_out, dbde_hip_frame_result *d_results) {
    return decode_scaled_common(ctx, "decode_scaled", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0,
                                y0, rw, rh, d_origins, out_type, d_dark, dark0, d_gain, gain0, d_out, d_results);
}

int dbde16_hip_decode_scaled(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                             const int32_t *d_origins, int out_type, const float *d_dark, float dark0,
                             const float *d_gain, float gain0, void *d_out, dbde_hip_frame_result *d_results) {
    return decode_scaled_common(ctx, "decode_scaled16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames,
                                x0, y0, rw, rh, d_origins, out_type, d_dark, dark0, d_gain, gain0, d_out, d_results);
}

// ---- threshold mask decode ----------------------------------------------------------------------------------
struct MaskPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t words, threads;
    uint32_t piece_words, pieces;               // with per-frame origins: any x mod 8
    uint32_t piece_words_fixed, pieces_fixed;   // at (x0, y0): one more word per piece when x0 is a multiple of 8
    uint64_t grid, grid_origins, mask_bytes;
};
// Pieces are cut in window coordinates (whole mask words), so their number does not depend on the origin.
static const char *plan_mask(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint32_t pix, MaskPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi, kMaskWideThreadsOf(pix))) return why;
    pl.words = ((uint32_t)rw + 63u) / 64u;
    pl.threads = pl.words <= kMaskNarrowWords ? kMaskNarrowThreads : kMaskWideThreadsOf(pix);
    // as few pieces as the workgroup's tiles allow, the words spread evenly over them
    const uint32_t cap = kMaskPieceWordsOf(pl.threads), cap_fixed = x0 % 8 == 0 ? kMaskAlignedPieceWordsOf(pl.threads) : cap;
    pl.pieces = (pl.words + cap - 1u) / cap;
    pl.piece_words = (pl.words + pl.pieces - 1u) / pl.pieces;
    pl.pieces_fixed = (pl.words + cap_fixed - 1u) / cap_fixed;
    pl.piece_words_fixed = (pl.words + pl.pieces_fixed - 1u) / pl.pieces_fixed;
    pl.grid = (uint64_t)n_frames * pl.roi.nty * pl.pieces_fixed;
    pl.grid_origins = (uint64_t)n_frames * pl.roi.max_ty * pl.pieces;
    if (pl.grid_origins >= (1ull << 31)) return "too many workgroups in one call";
    pl.mask_bytes = (uint64_t)n_frames * (uint64_t)rh * pl.words * 8u;
    return nullptr;
}

static int mask_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint32_t pix,
                            dbde_hip_mask_plan_t *plan) {
    MaskPlan pl;
    if (!plan || plan_mask(W, H, n_frames, x0, y0, rw, rh, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->max_tiles_x = (int32_t)pl.roi.max_tx;
    plan->max_tiles_y = (int32_t)pl.roi.max_ty;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->threads = pl.threads;
    plan->pieces_x = pl.pieces;
    plan->piece_words = pl.piece_words;
    plan->lds_bytes = kMaskLdsBytesOf(pl.threads, pix);
    plan->words = pl.words;
    plan->pieces_x_fixed = pl.pieces_fixed;
    plan->piece_words_fixed = pl.piece_words_fixed;
    plan->grid = pl.grid;
    plan->grid_origins = pl.grid_origins;
    plan->mask_bytes = pl.mask_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_mask_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_mask_plan_t *plan) {
    return mask_plan_common(W, H, n_frames, x0, y0, rw, rh, 1u, plan);
}

int dbde16_hip_mask_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_mask_plan_t *plan) {
    return mask_plan_common(W, H, n_frames, x0, y0, rw, rh, 2u, plan);
}

// Both mask decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the counts' and boxes'
// initialisation and the mask kernel in slot 2.
static int decode_mask_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                              size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0,
                              int y0, int rw, int rh, const int32_t *d_origins, int mode, const void *d_lo_map,
                              uint32_t lo0, const void *d_hi_map, uint32_t hi0, uint64_t *d_mask, uint32_t *d_counts,
                              int32_t *d_boxes, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    MaskPlan pl;
    if (const char *why = plan_mask(W, H, n_frames, x0, y0, rw, rh, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames,
                    rw, rh, x0, y0);
    if (!d_stream || !d_frame_offsets) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (mode != DBDE_HIP_MASK_INSIDE && mode != DBDE_HIP_MASK_OUTSIDE)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: mode %d is neither INSIDE nor OUTSIDE", name, mode);
    const uint32_t pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    if (lo0 > pix_max || hi0 > pix_max)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: thresholds %u, %u above %u", name, lo0, hi0, pix_max);
    if (!d_mask && !d_counts && !d_boxes) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: no output requested", name);
    if (reinterpret_cast<uintptr_t>(d_mask) & 7u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the mask must be 8-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_counts) | reinterpret_cast<uintptr_t>(d_boxes)) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the counts and boxes must be 4-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_lo_map) | reinterpret_cast<uintptr_t>(d_hi_map)) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the maps must be %u-byte aligned", name, pix);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;

    MaskParams p;
    memset(&p, 0, sizeof p);
    p.roi.stream = d_stream;
    p.roi.frame_offsets = d_frame_offsets;
    p.roi.stream_bytes = stream_bytes;
    p.roi.chunk_off = ctx->chunk_off;
    p.roi.frame_ok = ctx->frame_ok;
    p.roi.origins = d_origins;
    p.roi.W = W;
    p.roi.H = H;
    p.roi.x0 = x0;
    p.roi.y0 = y0;
    p.roi.rw = rw;
    p.roi.rh = rh;
    p.roi.w = pl.roi.g.w;
    p.roi.h = pl.roi.g.h;
    p.roi.T = pl.roi.g.T;
    p.roi.geom = pl.roi.dg;
    p.roi.rows = d_origins ? pl.roi.max_ty : pl.roi.nty;
    p.roi.pieces = d_origins ? pl.pieces : pl.pieces_fixed;
    p.lo_map = d_lo_map;
    p.hi_map = d_hi_map;
    p.lo0 = lo0;
    p.hi0 = hi0;
    p.outside = mode == DBDE_HIP_MASK_OUTSIDE ? kMaskOutside : kMaskInside;
    p.words = pl.words;
    p.piece_words = d_origins ? pl.piece_words : pl.piece_words_fixed;
    p.mask = d_mask;
    p.counts = d_counts;
    p.boxes = d_boxes;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_mask_init(d_counts, d_boxes, (uint32_t)n_frames, rw, rh, ctx->stream));
    HIP_TRY(ctx, launch_decode_mask(p, (uint32_t)n_frames, pl.threads, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_mask(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                         const int32_t *d_origins, int mode, const uint8_t *d_lo_map, uint32_t lo0,
                         const uint8_t *d_hi_map, uint32_t hi0, uint64_t *d_mask, uint32_t *d_counts, int32_t *d_boxes,
                         dbde_hip_frame_result *d_results) {
    return decode_mask_common(ctx, "decode_mask", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                              rw, rh, d_origins, mode, d_lo_map, lo0, d_hi_map, hi0, d_mask, d_counts, d_boxes, d_results);
}

int dbde16_hip_decode_mask(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           const int32_t *d_origins, int mode, const uint16_t *d_lo_map, uint32_t lo0,
                           const uint16_t *d_hi_map, uint32_t hi0, uint64_t *d_mask, uint32_t *d_counts,
                           int32_t *d_boxes, dbde_hip_frame_result *d_results) {
    return decode_mask_common(ctx, "decode_mask16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0,
                              rw, rh, d_origins, mode, d_lo_map, lo0, d_hi_map, hi0, d_mask, d_counts, d_boxes, d_results);
}

// ---- patch decode -------------------------------------------------------------------------------------------
struct PatchPlan {
    Geometry g;
    DecGeom dg;                       // the index's chunks (roi_index_geometry)
    uint32_t mtx, mty;                // the most tiles any origin makes a patch span
    uint32_t G, groups, split;
    uint64_t grid, out_bytes;
};
// nullptr when the arguments are good, else what is wrong with them.
static const char *plan_patches(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                                PatchPlan &pl) {
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, pl.g)) return "bad frame size";
    if (edge_mode != DBDE_HIP_PATCH_CLAMP && edge_mode != DBDE_HIP_PATCH_FILL) return "edge mode is neither CLAMP nor FILL";
    if (n_patches < 1) return "n_patches < 1";
    if (pw < 1 || ph < 1) return "patch size below 1";
    if (((uint32_t)pw + 6u) / 8u + 1u > kPatchMaxTilesX) return "a patch could be more than 64 tiles across (pw > 505)";
    const bool clamp = edge_mode == DBDE_HIP_PATCH_CLAMP;
    if (clamp && (pw > W || ph > H)) return "CLAMP mode: patch size outside [1, W] x [1, H]";
    pl.dg = roi_index_geometry(pl.g.w, pl.g.h);
    if (pl.dg.cpf > kMaxChunksPerFrame) return "frame too large";
    // x mod 8 reaches 7 in general, min(7, W - pw) over the origins clamping leaves (plan_roi)
    const uint64_t mx = clamp && (uint32_t)(W - pw) < 7u ? (uint32_t)(W - pw) : 7u;
    const uint64_t my = clamp && (uint32_t)(H - ph) < 7u ? (uint32_t)(H - ph) : 7u;
    pl.mtx = (uint32_t)((mx + (uint64_t)pw + 7u) / 8u);
    pl.mty = (uint32_t)((my + (uint64_t)ph + 7u) / 8u);
    pl.G = kPatchThreads / pl.mtx < 1u ? 1u : kPatchThreads / pl.mtx;
    pl.groups = (pl.mty + pl.G - 1u) / pl.G;
    pl.split = index_split_for(n_frames, pl.dg.cpf);
    // (n_frames, n_patches < 2^31 and groups < 2^29: np is bounded before it is multiplied by groups, so nothing wraps)
    const uint64_t np = (uint64_t)n_frames * (uint64_t)n_patches;
    if (np >= (1ull << 31)) return "too many workgroups in one call";
    pl.grid = np * pl.groups;
    if (pl.grid >= (1ull << 31)) return "too many workgroups in one call";
    if ((uint64_t)n_frames * (pl.dg.cpf + 1u) >= (1ull << 31)) return "too many chunks in one call";
    pl.out_bytes = np * (uint64_t)ph * (uint64_t)pw * pix;   // (ph <= 512 groups: np * ph < 2^40)
    return nullptr;
}

static int patches_plan_common(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                               dbde_hip_patches_plan_t *plan) {
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (!plan || plan_patches(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->max_tiles_x = (int32_t)pl.mtx;
    plan->max_tiles_y = (int32_t)pl.mty;
    plan->rows_per_workgroup = pl.G;
    plan->groups_per_patch = pl.groups;
    plan->threads = kPatchThreads;
    plan->chunks_per_frame = pl.dg.cpf;
    plan->chunk_tiles = pl.dg.ct;
    plan->chunk_pieces = pl.dg.ct == pl.g.w || pl.dg.pieces > 1u ? pl.dg.pieces : 0u;
    plan->index_split = pl.split;
    plan->lds_bytes = kPatchPayBytesOf(pix);
    plan->grid = pl.grid;
    plan->out_bytes = pl.out_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_patches_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                          dbde_hip_patches_plan_t *plan) {
    return patches_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 1u, plan);
}

int dbde16_hip_patches_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                            dbde_hip_patches_plan_t *plan) {
    return patches_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 2u, plan);
}

// Both patch decoders: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the patch kernel in
// slot 2.
static int decode_patches_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                 size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw,
                                 int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode,
                                 uint32_t fill, void *d_out, int32_t *d_used, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (const char *why = plan_patches(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, %d patches of %dx%d, edge mode %d)", name, why, W, H,
                    n_frames, n_patches, pw, ph, edge_mode);
    if (!d_stream || !d_frame_offsets || !d_origins || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    const uint32_t pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    if (fill > pix_max) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: fill %u above %u", name, fill, pix_max);
    if (reinterpret_cast<uintptr_t>(d_out) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the output must be %u-byte aligned", name, pix);
    if ((reinterpret_cast<uintptr_t>(d_origins) | reinterpret_cast<uintptr_t>(d_counts) | reinterpret_cast<uintptr_t>(d_used)) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins, counts and used origins must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, pix, pl.split);
    if (rc) return rc;

    PatchParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.origins = d_origins;
    p.counts = d_counts;
    p.out = static_cast<uint8_t *>(d_out);
    p.used = d_used;
    p.W = W;
    p.H = H;
    p.pw = pw;
    p.ph = ph;
    p.n_patches = (uint32_t)n_patches;
    p.w = pl.g.w;
    p.h = pl.g.h;
    p.T = pl.g.T;
    p.geom = pl.dg;
    p.mtx = pl.mtx;
    p.G = pl.G;
    p.groups = pl.groups;
    p.mode = edge_mode == DBDE_HIP_PATCH_FILL ? kPatchFill : kPatchClamp;
    p.fill = fill;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_decode_patches(p, (uint32_t)n_frames, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_decode_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                            const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                            uint8_t *d_out, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return decode_patches_common(ctx, "decode_patches", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw,
                                 ph, n_patches, d_origins, d_counts, edge_mode, fill, d_out, d_used, d_results);
}

int dbde16_hip_decode_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                              const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                              uint16_t *d_out, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return decode_patches_common(ctx, "decode_patches16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw,
                                 ph, n_patches, d_origins, d_counts, edge_mode, fill, d_out, d_used, d_results);
}

// ---- patch moments ------------------------------------------------------------------------------------------
// The sizes and the edge mode are the patch decoder's (plan_patches); what is added is the height limit that keeps every
// sum inside 64 bits, and the launch: one workgroup per patch that walks the patch's groups of tile rows itself.
static const char *plan_moments(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                                PatchPlan &pl) {
    if (const char *why = plan_patches(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl)) return why;
    if (ph > kMomentMaxHeight) return "patch higher than 512 rows (the sums could pass 64 bits)";
    static_assert(kMomentMaxTilesX == kPatchMaxTilesX && kMomentThreads == kPatchThreads, "plan_patches' geometry is the kernel's");
    static_assert(kMomentClamp == DBDE_HIP_PATCH_CLAMP && kMomentFill == DBDE_HIP_PATCH_FILL, "edge modes");
    static_assert(kMomentCount == DBDE_HIP_MOMENT_COUNT && kMomentValue == DBDE_HIP_MOMENT_VALUE &&
                  kMomentAbove == DBDE_HIP_MOMENT_ABOVE && kMomentBelow == DBDE_HIP_MOMENT_BELOW, "weight modes");
    return nullptr;
}

static int moments_plan_common(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode, uint32_t pix,
                               dbde_hip_patch_moments_plan_t *plan) {
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (!plan || plan_moments(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->max_tiles_x = (int32_t)pl.mtx;
    plan->max_tiles_y = (int32_t)pl.mty;
    plan->rows_per_workgroup = pl.G;
    plan->steps_per_patch = pl.groups;
    plan->threads = kMomentThreads;
    plan->chunks_per_frame = pl.dg.cpf;
    plan->chunk_tiles = pl.dg.ct;
    plan->chunk_pieces = pl.dg.ct == pl.g.w || pl.dg.pieces > 1u ? pl.dg.pieces : 0u;
    plan->index_split = pl.split;
    plan->lds_bytes = kMomentPayBytesOf(pix);
    plan->grid = (uint64_t)n_frames * (uint64_t)n_patches;
    plan->moments_bytes = plan->grid * 64u;
    return DBDE_HIP_OK;
}

int dbde_hip_patch_moments_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                                dbde_hip_patch_moments_plan_t *plan) {
    return moments_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 1u, plan);
}

int dbde16_hip_patch_moments_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                                  dbde_hip_patch_moments_plan_t *plan) {
    return moments_plan_common(W, H, n_frames, pw, ph, n_patches, edge_mode, 2u, plan);
}

// Both calls: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the moments kernel in slot 2.
static int patch_moments_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw,
                                int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode,
                                uint32_t lo, uint32_t hi, int weight_mode, uint64_t *d_moments, int32_t *d_bbox,
                                int32_t *d_used, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    PatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (const char *why = plan_moments(W, H, n_frames, pw, ph, n_patches, edge_mode, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, %d patches of %dx%d, edge mode %d)", name, why, W, H,
                    n_frames, n_patches, pw, ph, edge_mode);
    if (!d_stream || !d_frame_offsets || !d_origins || !d_moments) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    const uint32_t pix_max = pix == 1u ? 0xFFu : 0xFFFFu;
    if (lo > pix_max || hi > pix_max)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: threshold %u above %u", name, lo > pix_max ? lo : hi, pix_max);
    if (weight_mode < DBDE_HIP_MOMENT_COUNT || weight_mode > DBDE_HIP_MOMENT_BELOW)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: unknown weight mode %d", name, weight_mode);
    if (reinterpret_cast<uintptr_t>(d_moments) & 7u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the moments must be 8-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_origins) | reinterpret_cast<uintptr_t>(d_counts) | reinterpret_cast<uintptr_t>(d_used) |
         reinterpret_cast<uintptr_t>(d_bbox)) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins, counts, boxes and used origins must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.dg, pix, pl.split);
    if (rc) return rc;

    MomentParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.origins = d_origins;
    p.counts = d_counts;
    p.moments = d_moments;
    p.bbox = d_bbox;
    p.used = d_used;
    p.W = W;
    p.H = H;
    p.pw = pw;
    p.ph = ph;
    p.n_patches = (uint32_t)n_patches;
    p.w = pl.g.w;
    p.h = pl.g.h;
    p.T = pl.g.T;
    p.geom = pl.dg;
    p.mtx = pl.mtx;
    p.G = pl.G;
    p.steps = pl.groups;
    p.mode = edge_mode == DBDE_HIP_PATCH_FILL ? kMomentFill : kMomentClamp;
    p.lo = lo;
    p.hi = hi;
    p.weight = (uint32_t)weight_mode;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_patch_moments(p, (uint32_t)n_frames, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_patch_moments(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                           const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t lo, uint32_t hi,
                           int weight_mode, uint64_t *d_moments, int32_t *d_bbox, int32_t *d_used,
                           dbde_hip_frame_result *d_results) {
    return patch_moments_common(ctx, "patch_moments", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw, ph,
                                n_patches, d_origins, d_counts, edge_mode, lo, hi, weight_mode, d_moments, d_bbox, d_used,
                                d_results);
}

int dbde16_hip_patch_moments(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int pw, int ph, int n_patches,
                             const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t lo, uint32_t hi,
                             int weight_mode, uint64_t *d_moments, int32_t *d_bbox, int32_t *d_used,
                             dbde_hip_frame_result *d_results) {
    return patch_moments_common(ctx, "patch_moments16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, pw,
                                ph, n_patches, d_origins, d_counts, edge_mode, lo, hi, weight_mode, d_moments, d_bbox,
                                d_used, d_results);
}

// ---- patch match --------------------------------------------------------------------------------------------
// The search patch's size and the edge mode go through the patch decoder's plan (plan_patches); what is added are the
// template and radius limits that keep an 8-bit entry inside 32 bits, the split of a shift's rows over lanes, and the LDS.
struct MatchPlan {
    PatchPlan pp;
    int pw, ph;
    uint32_t D, dwaves, steps, slices;
    MatchLayout lds;
    uint64_t surface_bytes;
};
static const char *plan_match(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                              int edge_mode, uint32_t fill, unsigned stats, uint32_t pix, MatchPlan &pl) {
    if (tw < 1 || th < 1 || tw > kMatchMaxTemplate || th > kMatchMaxTemplate) return "template size outside [1, 128]";
    if (S < 0 || S > kMatchMaxRadius) return "search radius outside [0, 16]";
    pl.pw = tw + 2 * S;
    pl.ph = th + 2 * S;
    if (const char *why = plan_patches(W, H, n_frames, pl.pw, pl.ph, n_patches, edge_mode, pix, pl.pp)) return why;
    if (fill > (pix == 1u ? 0xFFu : 0xFFFFu)) return "fill above the pixel type";
    if (n_templates != 1 && n_templates != n_patches) return "n_templates is neither 1 nor n_patches";
    if (stats == 0u || (stats & ~7u)) return "stats empty or with unknown bits";
    static_assert(kMatchClamp == DBDE_HIP_PATCH_CLAMP && kMatchFill == DBDE_HIP_PATCH_FILL, "edge modes");
    static_assert(kMatchProd == DBDE_HIP_MATCH_PROD && kMatchSum == DBDE_HIP_MATCH_SUM && kMatchSq == DBDE_HIP_MATCH_SQ, "surfaces");
    static_assert(kPatchThreads == 64u, "plan_patches' G is tile rows per wave");
    pl.D = 2u * (uint32_t)S + 1u;
    pl.dwaves = pl.pp.groups < kMatchWaves ? pl.pp.groups : kMatchWaves;
    pl.steps = (pl.pp.groups + pl.dwaves - 1u) / pl.dwaves;
    // the row slices: a lane's cost is its passes over the items times an item's cost, the batches of kMatchBatch dwords
    // in the rows of its slice plus a fixed part: ceil(nsh r / 256) * (ceil(th / r) * batches + kMatchItemCost).  The count
    // up to 16 (and th) with the least cost, the smallest on a tie
    const uint32_t nsh = pl.D * pl.D, rmax = (uint32_t)th < kMatchMaxSlices ? (uint32_t)th : kMatchMaxSlices;
    const uint32_t batches = (((uint32_t)tw * pix + 3u) / 4u + kMatchBatch - 1u) / kMatchBatch;
    uint32_t best = 0xFFFFFFFFu;
    pl.slices = 1u;
    for (uint32_t r = 1; r <= rmax; r++) {
        const uint32_t passes = (nsh * r + kMatchThreads - 1u) / kMatchThreads;
        const uint32_t cost = passes * ((((uint32_t)th + r - 1u) / r) * batches + kMatchItemCost);
        if (cost < best) {
            best = cost;
            pl.slices = r;
        }
    }
    pl.lds = match_layout(pix, (uint32_t)tw, (uint32_t)th, (uint32_t)S, pl.pp.mtx, pl.pp.mty, pl.pp.G, pl.dwaves, pl.slices);
    pl.surface_bytes = (uint64_t)n_frames * (uint64_t)n_patches * nsh * 8u;   // (below 2^31 * 1089 * 8)
    return nullptr;
}

static int match_plan_common(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                             int edge_mode, uint32_t fill, unsigned stats, uint32_t pix, dbde_hip_match_plan_t *plan) {
    MatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (!plan || plan_match(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, pix, pl))
        return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->pw = pl.pw;
    plan->ph = pl.ph;
    plan->D = (int32_t)pl.D;
    plan->max_tiles_x = (int32_t)pl.pp.mtx;
    plan->max_tiles_y = (int32_t)pl.pp.mty;
    plan->rows_per_wave = pl.pp.G;
    plan->decode_waves = pl.dwaves;
    plan->steps_per_patch = pl.steps;
    plan->row_slices = pl.slices;
    plan->threads = kMatchThreads;
    plan->chunks_per_frame = pl.pp.dg.cpf;
    plan->chunk_tiles = pl.pp.dg.ct;
    plan->chunk_pieces = pl.pp.dg.ct == pl.pp.g.w || pl.pp.dg.pieces > 1u ? pl.pp.dg.pieces : 0u;
    plan->index_split = pl.pp.split;
    plan->lds_bytes = pl.lds.bytes;
    plan->grid = (uint64_t)n_frames * (uint64_t)n_patches;
    plan->surface_bytes = pl.surface_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_match_plan(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                        int edge_mode, uint32_t fill, unsigned stats, dbde_hip_match_plan_t *plan) {
    return match_plan_common(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, 1u, plan);
}

int dbde16_hip_match_plan(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                          int edge_mode, uint32_t fill, unsigned stats, dbde_hip_match_plan_t *plan) {
    return match_plan_common(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, 2u, plan);
}

// Both calls: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the match kernel in slot 2.
static int match_patches_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream,
                                size_t stream_bytes, const uint64_t *d_frame_offsets, int W, int H, int n_frames, int tw,
                                int th, int S, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                                int edge_mode, uint32_t fill, const void *d_templates, int n_templates, unsigned stats,
                                uint64_t *d_prod, uint64_t *d_sum, uint64_t *d_sq, int32_t *d_used,
                                dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    MatchPlan pl;
    memset(&pl, 0, sizeof pl);
    if (const char *why = plan_match(W, H, n_frames, tw, th, S, n_patches, n_templates, edge_mode, fill, stats, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d, %d patches, %d templates of %dx%d, radius %d, edge mode %d, "
                    "fill %u, stats %u)", name, why, W, H, n_frames, n_patches, n_templates, tw, th, S, edge_mode, fill, stats);
    if (!d_stream || !d_frame_offsets || !d_origins || !d_templates) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (reinterpret_cast<uintptr_t>(d_templates) & (pix - 1u))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: the templates must be %u-byte aligned", name, pix);
    uint64_t *const surf[3] = {d_prod, d_sum, d_sq};
    for (int i = 0; i < 3; i++)
        if ((stats >> i & 1u) && (!surf[i] || (reinterpret_cast<uintptr_t>(surf[i]) & 7u)))
            return fail(ctx, DBDE_HIP_ERR_ARG, "%s: a requested surface is null or not 8-byte aligned", name);
    if ((reinterpret_cast<uintptr_t>(d_origins) | reinterpret_cast<uintptr_t>(d_counts) | reinterpret_cast<uintptr_t>(d_used)) & 3u)
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: origins, counts and used origins must be 4-byte aligned", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.pp.dg, pix, pl.pp.split);
    if (rc) return rc;

    MatchParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.origins = d_origins;
    p.counts = d_counts;
    p.templates = static_cast<const uint8_t *>(d_templates);
    p.prod = (stats & DBDE_HIP_MATCH_PROD) ? d_prod : nullptr;
    p.sum = (stats & DBDE_HIP_MATCH_SUM) ? d_sum : nullptr;
    p.sq = (stats & DBDE_HIP_MATCH_SQ) ? d_sq : nullptr;
    p.used = d_used;
    p.W = W;
    p.H = H;
    p.pw = pl.pw;
    p.ph = pl.ph;
    p.tw = (uint32_t)tw;
    p.th = (uint32_t)th;
    p.D = pl.D;
    p.n_patches = (uint32_t)n_patches;
    p.per_patch = n_templates == 1 ? 0u : 1u;
    p.w = pl.pp.g.w;
    p.h = pl.pp.g.h;
    p.T = pl.pp.g.T;
    p.geom = pl.pp.dg;
    p.mtx = pl.pp.mtx;
    p.G = pl.pp.G;
    p.dwaves = pl.dwaves;
    p.steps = pl.steps;
    p.slices = pl.slices;
    p.mode = edge_mode == DBDE_HIP_PATCH_FILL ? kMatchFill : kMatchClamp;
    p.fill = fill;
    p.stats = stats;
    p.lds = pl.lds;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_match_patches(p, (uint32_t)n_frames, pix, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_match_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int tw, int th, int S,
                           int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                           const uint8_t *d_templates, int n_templates, unsigned stats, uint64_t *d_prod, uint64_t *d_sum,
                           uint64_t *d_sq, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return match_patches_common(ctx, "match_patches", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, tw, th, S,
                                n_patches, d_origins, d_counts, edge_mode, fill, d_templates, n_templates, stats, d_prod,
                                d_sum, d_sq, d_used, d_results);
}

int dbde16_hip_match_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames, int tw, int th, int S,
                             int n_patches, const int32_t *d_origins, const uint32_t *d_counts, int edge_mode, uint32_t fill,
                             const uint16_t *d_templates, int n_templates, unsigned stats, uint64_t *d_prod, uint64_t *d_sum,
                             uint64_t *d_sq, int32_t *d_used, dbde_hip_frame_result *d_results) {
    return match_patches_common(ctx, "match_patches16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, tw, th,
                                S, n_patches, d_origins, d_counts, edge_mode, fill, d_templates, n_templates, stats, d_prod,
                                d_sum, d_sq, d_used, d_results);
}

// ---- compressed-domain crop ---------------------------------------------------------------------------------
struct CropPlan {
    RoiPlan roi;                      // arguments, tile window and index geometry: the window decoder's (plan_roi)
    uint32_t Tout, recoded;
    uint64_t max_frame, capacity, rows;
    uint64_t tables_bytes, rec_fixed_bytes, rec_origins_bytes;
};
static uint64_t crop_max_frame_bytes(uint64_t T, uint32_t pix) { return 20u + 12u + (pix == 2u ? 131u : 66u) * T; }
static uint64_t round16(uint64_t v) { return (v + 15u) & ~(uint64_t)15; }
static const char *plan_crop(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                             uint32_t pix, CropPlan &pl) {
    if (const char *why = plan_roi(W, H, n_frames, x0, y0, rw, rh, pl.roi)) return why;
    if ((x0 | y0) & 7) return "window origin not a multiple of 8";
    const RoiPlan &r = pl.roi;
    pl.Tout = r.ntx * r.nty;
    pl.max_frame = crop_max_frame_bytes(pl.Tout, pix);
    if (slot_stride && slot_stride < pl.max_frame) return "slot_stride below the cropped frame's worst case";
    pl.capacity = n_frames == 0 ? 0u : (slot_stride ? (uint64_t)(n_frames - 1) * slot_stride + pl.max_frame : (uint64_t)n_frames * pl.max_frame);
    pl.rows = (uint64_t)n_frames * r.nty;
    if (pl.rows >= (1ull << 31)) return "too many workgroups in one call";
    const uint32_t rm = (uint32_t)rw - 8u * (r.ntx - 1u), dm = (uint32_t)rh - 8u * (r.nty - 1u);
    const uint32_t srm = (uint32_t)W - 8u * (r.tx0 + r.ntx - 1u), sdm = (uint32_t)H - 8u * (r.ty0 + r.nty - 1u);
    const bool cut_col = rm != (srm < 8u ? srm : 8u), cut_row = dm != (sdm < 8u ? sdm : 8u);
    pl.recoded = cut_row ? (cut_col ? r.ntx + r.nty - 1u : r.ntx) : (cut_col ? r.nty : 0u);
    // three U32 per (frame, window tile row), two U64 per frame; the records behind them
    pl.tables_bytes = round16(3u * 4u * pl.rows) + 2u * 8u * (uint64_t)n_frames;
    pl.rec_origins_bytes = (uint64_t)n_frames * (r.ntx + r.nty - 1u) * kCropRecBytes;
    pl.rec_fixed_bytes = pl.recoded ? pl.rec_origins_bytes : 0u;
    return nullptr;
}

static int crop_plan_common(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride, uint32_t pix,
                            dbde_hip_crop_plan_t *plan) {
    CropPlan pl;
    if (!plan || plan_crop(W, H, n_frames, x0, y0, rw, rh, slot_stride, pix, pl)) return DBDE_HIP_ERR_ARG;
    memset(plan, 0, sizeof *plan);
    plan->tile_x = (int32_t)pl.roi.tx0;
    plan->tile_y = (int32_t)pl.roi.ty0;
    plan->tiles_x = (int32_t)pl.roi.ntx;
    plan->tiles_y = (int32_t)pl.roi.nty;
    plan->out_tiles = pl.Tout;
    plan->recoded_tiles = pl.recoded;
    plan->chunks_per_frame = pl.roi.dg.cpf;
    plan->chunk_tiles = pl.roi.dg.ct;
    plan->chunk_pieces = pl.roi.dg.ct == pl.roi.g.w || pl.roi.dg.pieces > 1u ? pl.roi.dg.pieces : 0u;
    plan->index_split = pl.roi.split;
    plan->size_threads = kCropThreads;
    plan->size_lds_bytes = kCropSizeLds;
    plan->rows_threads = kCropThreads;
    plan->rows_lds_bytes = kCropRowsLds;
    plan->place_threads = kCropPlaceThreads;
    plan->place_lds_bytes = kCropPlaceLds;
    plan->copy_threads = kCropThreads;
    plan->copy_lds_bytes = kCropCopyLds;
    plan->repack_threads = kCropThreads;
    plan->repack_lds_bytes = kCropRepackLds;
    plan->repack_grid = pl.recoded ? (uint64_t)n_frames * ((pl.roi.ntx + pl.roi.nty - 1u + kCropThreads - 1u) / kCropThreads) : 0u;
    plan->size_grid = pl.rows;
    plan->rows_grid = (uint64_t)n_frames;
    plan->place_grid = n_frames ? 1u : 0u;
    plan->copy_grid = pl.rows;
    plan->max_out_frame_bytes = pl.max_frame;
    plan->out_capacity = pl.capacity;
    plan->workspace_bytes = pl.tables_bytes + pl.rec_origins_bytes;
    return DBDE_HIP_OK;
}

int dbde_hip_crop_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                       dbde_hip_crop_plan_t *plan) {
    return crop_plan_common(W, H, n_frames, x0, y0, rw, rh, slot_stride, 1u, plan);
}

int dbde16_hip_crop_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                         dbde_hip_crop_plan_t *plan) {
    return crop_plan_common(W, H, n_frames, x0, y0, rw, rh, slot_stride, 2u, plan);
}

// Both crops: the index (pix: 1 = DBDE, 2 = DBDE16, also its min_bytes) in timing slot 1, the crop kernels in slot 2.
static int crop_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_stream, size_t stream_bytes,
                       const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                       const int32_t *d_origins, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                       uint64_t *d_out_offsets, uint64_t *d_out_bytes, int32_t *d_origins_used,
                       dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    CropPlan pl;
    if (const char *why = plan_crop(W, H, n_frames, x0, y0, rw, rh, slot_stride, pix, pl))
        return fail(ctx, DBDE_HIP_ERR_ARG, "%s: %s (W=%d H=%d n=%d window %dx%d at %d,%d)", name, why, W, H, n_frames, rw,
                    rh, x0, y0);
    if (!d_stream || !d_frame_offsets || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    if ((uint64_t)out_capacity < pl.capacity)
        return fail(ctx, DBDE_HIP_ERR_CAPACITY, "%s: out_capacity %zu below the worst case %llu", name, out_capacity,
                    (unsigned long long)pl.capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t rec_bytes = d_origins ? pl.rec_origins_bytes : pl.rec_fixed_bytes;
    int rc = grow(ctx, ctx->crop_ws, ctx->crop_ws_bytes, (size_t)(pl.tables_bytes + rec_bytes), 1);
    if (rc) return rc;
    rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, pl.roi.dg, pix, pl.roi.split);
    if (rc) return rc;

    CropParams p;
    memset(&p, 0, sizeof p);
    p.stream = d_stream;
    p.frame_offsets = d_frame_offsets;
    p.stream_bytes = stream_bytes;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.origins = d_origins;
    p.origins_used = d_origins_used;
    p.out = d_out;
    p.slot_stride = slot_stride;
    p.out_offsets = d_out_offsets;
    p.out_bytes = d_out_bytes;
    uint8_t *ws = ctx->crop_ws;
    p.frame_bytes = reinterpret_cast<uint64_t *>(ws);
    p.frame_off = p.frame_bytes + n_frames;
    p.row_src = reinterpret_cast<uint32_t *>(ws + 16u * (size_t)n_frames);
    p.row_copy = p.row_src + pl.rows;
    p.row_words = p.row_copy + pl.rows;
    p.rec = ws + pl.tables_bytes;
    p.W = W;
    p.H = H;
    p.x0 = x0;
    p.y0 = y0;
    p.rw = rw;
    p.rh = rh;
    p.w = pl.roi.g.w;
    p.T = pl.roi.g.T;
    p.geom = pl.roi.dg;
    p.ntx = pl.roi.ntx;
    p.nty = pl.roi.nty;
    p.Tout = pl.Tout;
    p.n_frames = (uint32_t)n_frames;
    span_begin(ctx, 2);
    HIP_TRY(ctx, launch_crop(p, pix, d_origins != nullptr || pl.recoded != 0u, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_crop_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                         int W, int H, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                         uint8_t *d_out, size_t out_capacity, uint64_t slot_stride, uint64_t *d_out_offsets,
                         uint64_t *d_out_bytes, int32_t *d_origins_used, dbde_hip_frame_result *d_results) {
    return crop_common(ctx, "crop_frames", 1u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                       d_origins, d_out, out_capacity, slot_stride, d_out_offsets, d_out_bytes, d_origins_used, d_results);
}

int dbde16_hip_crop_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                           const int32_t *d_origins, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                           uint64_t *d_out_offsets, uint64_t *d_out_bytes, int32_t *d_origins_used,
                           dbde_hip_frame_result *d_results) {
    return crop_common(ctx, "crop_frames16", 2u, d_stream, stream_bytes, d_frame_offsets, W, H, n_frames, x0, y0, rw, rh,
                       d_origins, d_out, out_capacity, slot_stride, d_out_offsets, d_out_bytes, d_origins_used, d_results);
}

int dbde_hip_index_stream_async(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, int W, int H,
                                int max_frames, uint64_t *d_frame_offsets, uint32_t *d_n_found) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    Geometry g;
    if (!d_stream || !d_frame_offsets || !d_n_found || max_frames < 0 || !geometry(W, H, g))
        return fail(ctx, DBDE_HIP_ERR_ARG, "index_stream: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // Long streams are walked speculatively in up to 16 segments at once (scan_spec_kernel: exact by construction,
    // the plain hop-by-hop walk is what it falls back to); short ones hop by hop.
    const uint64_t maxlen = 32ull + 66ull * g.T, meta = 32ull + 2ull * g.T;
    uint64_t n_seg = stream_bytes / (2 * maxlen);
    if (n_seg > 16) n_seg = 16;   // the signature searches (one maximal frame each, at worst) are the cost: few, wide segments (measured: 8-16)
    if (n_seg >= 2 && max_frames > 0) {
        ScanParams sp;
        sp.stream = d_stream;
        sp.stream_bytes = stream_bytes;
        sp.T = g.T;
        sp.gran = g.T % 4 == 0 ? 8u : (g.T % 2 == 0 ? 4u : 2u);   // frame lengths 32 + 2T + 8 n64 are multiples of this
        sp.seg_bytes = (stream_bytes + n_seg - 1) / n_seg;
        sp.seg_cap = (uint32_t)(sp.seg_bytes / meta + 3);
        if (sp.seg_cap > (uint32_t)max_frames + 3u) sp.seg_cap = (uint32_t)max_frames + 3u;   // no list needs more than the caller takes (tiny frames: T = 1, meta = 34)
        // workspace: [found 8 x 64][arrive 4 x 64] (kept zero by the kernel) | lists | start, end, count, ended
        const size_t fixed = 64 * 8 + 64 * 4, lists = (size_t)n_seg * sp.seg_cap * 8, need = fixed + lists + n_seg * 32 + 64;
        const size_t had = ctx->scan_ws_bytes;
        int rc = grow(ctx, ctx->scan_ws, ctx->scan_ws_bytes, need, 1);
        if (rc) return rc;
        if (ctx->scan_ws_bytes != had) HIP_TRY(ctx, hipMemsetAsync(ctx->scan_ws, 0, fixed, ctx->stream));
        sp.seg_found_inv = reinterpret_cast<unsigned long long *>(ctx->scan_ws);
        sp.seg_arrive = reinterpret_cast<uint32_t *>(ctx->scan_ws + 64 * 8);
        sp.seg_pos = reinterpret_cast<uint64_t *>(ctx->scan_ws + fixed);
        sp.seg_start = reinterpret_cast<uint64_t *>(ctx->scan_ws + fixed + lists);
        sp.seg_end = sp.seg_start + n_seg;
        sp.seg_count = reinterpret_cast<uint32_t *>(sp.seg_end + n_seg);
        sp.seg_ended = sp.seg_count + n_seg;
        sp.wg_per_seg = 4;                          // workgroups sharing a segment's signature search (measured: 1-4)
        span_begin(ctx, 3);
        HIP_TRY(ctx, launch_scan_spec(sp, (uint32_t)n_seg, max_frames, d_frame_offsets, d_n_found, ctx->stream));
    } else {
        span_begin(ctx, 3);
        HIP_TRY(ctx, launch_scan_stream(d_stream, stream_bytes, g.T, max_frames, d_frame_offsets, d_n_found, nullptr, ctx->stream));
    }
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_scan_ahead(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, int W, int H, int max_frames,
                        uint64_t *d_cursor, uint64_t *d_frame_offsets, uint32_t *d_n_found) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    Geometry g;
    if (!d_stream || !d_frame_offsets || !d_n_found || !d_cursor || max_frames < 0 || !geometry(W, H, g))
        return fail(ctx, DBDE_HIP_ERR_ARG, "scan_ahead: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->scan_stream) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->scan_stream, hipStreamNonBlocking, hi));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->scan_ev_main, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->scan_ev_done, hipEventDisableTiming));
    }
    // the walk may read what the main stream has produced so far (and the cursor a previous walk left)
    HIP_TRY(ctx, hipEventRecord(ctx->scan_ev_main, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->scan_stream, ctx->scan_ev_main, 0));
    // the walk is launched whether or not its timing bracket could be created (as span_begin / span_end)
    TimedSpan sp;
    sp.kind = 3;
    bool timed = false;
    if (ctx->timing && hipEventCreate(&sp.a) == hipSuccess) {
        if (hipEventCreate(&sp.b) == hipSuccess) timed = true;
        else (void)hipEventDestroy(sp.a);
    }
    if (timed) (void)hipEventRecord(sp.a, ctx->scan_stream);
    const hipError_t e_walk = launch_scan_stream(d_stream, stream_bytes, g.T, max_frames, d_frame_offsets, d_n_found, d_cursor, ctx->scan_stream);
    if (timed) {
        (void)hipEventRecord(sp.b, ctx->scan_stream);
        ctx->spans.push_back(sp);
    }
    HIP_TRY(ctx, e_walk);
    HIP_TRY(ctx, hipEventRecord(ctx->scan_ev_done, ctx->scan_stream));
    return DBDE_HIP_OK;
}

int dbde_hip_scan_join(dbde_hip_ctx *ctx) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    if (ctx->scan_stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->scan_ev_done, 0));
    return DBDE_HIP_OK;
}

int dbde_hip_index_stream(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, int W, int H,
                          int max_frames, uint64_t *d_frame_offsets, int *n_found) {
    if (!ctx || !n_found) return DBDE_HIP_ERR_ARG;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(ctx->scratch64);
    int rc = dbde_hip_index_stream_async(ctx, d_stream, stream_bytes, W, H, max_frames, d_frame_offsets, d_count);
    if (rc) return rc;
    uint32_t cnt = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&cnt, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_found = (int)cnt;
    return DBDE_HIP_OK;
}

int dbde_hip_synth_frames(dbde_hip_ctx *ctx, int mode, uint64_t seed, uint64_t first_frame, int n_frames,
                          int W, int H, uint8_t *d_images) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    if (!d_images || W <= 0 || H <= 0 || n_frames < 0 || mode < 0 || mode > 12)
        return fail(ctx, DBDE_HIP_ERR_ARG, "synth_frames: bad argument");
    if (n_frames == 0) return DBDE_HIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_synth(mode, seed, first_frame, n_frames, W, H, d_images, ctx->stream));
    return DBDE_HIP_OK;
}

// ---- launch plans (pure functions: no context, no device) ------------------------------------------------------

int dbde_hip_encode_plan(int W, int H, int n_frames, uint64_t image_address, uint64_t out_address, uint64_t slot_stride,
                         int resident_workgroups, dbde_hip_launch_plan *plan) {
    Geometry g;
    if (!plan || n_frames < 1 || resident_workgroups < 1 || !geometry(W, H, g)) return DBDE_HIP_ERR_ARG;
    const EncPlan pl = plan_encode(g, W, n_frames, (uintptr_t)image_address, (uintptr_t)out_address, slot_stride, (uint32_t)resident_workgroups);
    memset(plan, 0, sizeof *plan);
    plan->kernel = pl.kernel;
    plan->input_mode = pl.fast_in ? 0 : (pl.lanes_per_row ? (pl.seg_per_row ? 4 : pl.pairs_per_wave == 63u ? 3 : 1) : 2);
    plan->aligned_out = pl.aligned_out ? 1 : 0;
    plan->threads = (pl.kernel == 2 || pl.kernel == 5) ? 256 : (pl.kernel == 3 ? (int32_t)mid_encode_threads_for(g.T) : (pl.kernel == 4 ? (int32_t)frames_threads_for(g.T) : (int32_t)(kEncChunkTiles / 2u)));
    plan->chunks_per_frame = pl.kernel >= 2 ? 0u : pl.enc_cpf;
    plan->chunk_tiles = pl.kernel >= 2 ? 0u : (pl.seg_per_row ? 2u * (pl.seg_q + (pl.seg_rem ? 1u : 0u)) * (kEncChunkTiles / 128u) : pl.lanes_per_row ? 2u * pl.pairs_per_wave * (kEncChunkTiles / 128u) : kEncChunkTiles);
    plan->n_chunks = pl.kernel >= 2 ? 0ull : pl.n_chunks64;
    return DBDE_HIP_OK;
}

int dbde_hip_decode_plan(int W, int H, int n_frames, uint64_t image_address, int n_cu, dbde_hip_launch_plan *plan) {
    Geometry g;
    if (!plan || n_frames < 1 || n_cu < 1 || !geometry(W, H, g)) return DBDE_HIP_ERR_ARG;
    const DecPlan pl = plan_decode(g, W, n_frames, (uintptr_t)image_address, n_cu);
    memset(plan, 0, sizeof *plan);
    plan->kernel = pl.kernel;
    if (pl.kernel == 0) {
        plan->image_mode = pl.img_mode;
        plan->index_mode = pl.self_index ? 1 : (pl.fused ? 2 : 0);
        plan->threads = pl.img_mode == 1 && pl.dg.pieces == 1u && pl.dg.ct <= kChunkTilesSmall ? (int32_t)(kChunkTilesSmall / 2u) : (int32_t)(kChunkTiles / 2u);
        plan->chunks_per_frame = pl.dg.cpf;
        plan->chunk_tiles = pl.dg.ct;
        plan->n_chunks = pl.n_chunks64;
    } else {
        plan->threads = (int32_t)mid_decode_threads_for(g.T);
    }
    return DBDE_HIP_OK;
}

// ---- DBDE16: the higher-bit-depth extension (include/dbde_hip.h, oracle/dbde16_oracle.c) ----------------------

size_t dbde16_hip_max_frame_bytes(int W, int H) {
    Geometry g;
    if (!geometry(W, H, g)) return 0;
    return 20 + 12 + 131 * (size_t)g.T;
}

int dbde16_hip_encode_frames(dbde_hip_ctx *ctx, const uint16_t *d_images, int W, int H, int n_frames, uint64_t first_index,
                             uint8_t *d_out, size_t out_capacity, uint64_t slot_stride, uint64_t *d_frame_offsets,
                             uint64_t *d_frame_bytes) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    Geometry g;
    if (!d_images || !d_out || n_frames < 0 || !geometry(W, H, g))
        return fail(ctx, DBDE_HIP_ERR_ARG, "encode16: bad argument (W=%d H=%d n=%d)", W, H, n_frames);
    if (n_frames == 0) return DBDE_HIP_OK;
    const uint64_t maxf = 32ull + 131ull * g.T;
    if (slot_stride ? (slot_stride < maxf || (uint64_t)(n_frames - 1) * slot_stride + maxf > out_capacity)
                    : (uint64_t)n_frames * maxf > out_capacity)
        return fail(ctx, DBDE_HIP_ERR_CAPACITY, "encode16: out_capacity (or slot_stride) below the worst case");
    const uint32_t cpf = (g.T + dbde16::kChunkTiles16 - 1) / dbde16::kChunkTiles16;
    if ((uint64_t)n_frames * cpf >= (1ull << 31) || (uint64_t)g.T * 16ull >= (1ull << 32))
        return fail(ctx, DBDE_HIP_ERR_ARG, "encode16: launch too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // Large launches of 16-byte aligned rows go through the 8-bit path's persistent encoder (encode_kernel<.., PIX = 2>:
    // central scanner, register prefetch, wave-private payload images, one barrier per 512-tile chunk).  Its prefixes
    // are 32-bit word counts (30 bits inside a frame); everything else -- odd widths, launches the device is not
    // filled by, batches past those limits -- stays with enc16_kernel below.
    {
        const uint32_t cpf2 = (g.T + kEncChunkTiles / 2u - 1u) / (kEncChunkTiles / 2u);
        const uint64_t n_chunks64 = (uint64_t)n_frames * cpf2;
        const bool fits = 16ull * g.T < (1ull << 30) && (slot_stride != 0 || (uint64_t)n_frames * 16ull * g.T < (1ull << 32));
        const bool fast_in = W % 8 == 0 && (reinterpret_cast<uintptr_t>(d_images) & 15u) == 0;
        // (any other geometry from 8 pixels across on: the same kernel with its fetches where they lie -- U16 rows always
        // start at even addresses, which read at the full rate; a frame's bytes stay below 2^32 for its 32-bit offsets)
        const bool raw_in = !fast_in && W >= 8 && 2ull * g.pixels < (1ull << 32) && (reinterpret_cast<uintptr_t>(d_images) & 1u) == 0;
        if ((fast_in || raw_in) && fits && n_chunks64 >= ctx->enc_grid &&
            n_chunks64 < (1ull << 31) && !(ctx->exp_flags & 32u)) {
            EncParams q = enc_params(ctx, g, W, H, n_frames, 2u, cpf2, 0u, reinterpret_cast<const uint8_t *>(d_images), d_out,
                                     slot_stride, first_index, d_frame_offsets, d_frame_bytes);
            const bool aligned_out = (reinterpret_cast<uintptr_t>(d_out) & 7u) == 0 && g.T % 8 == 0 && slot_stride % 8 == 0;
            int rc = attach_lookback(ctx, q, q.n_chunks, false);
            if (rc) return rc;
            span_begin(ctx, 0);
            HIP_TRY(ctx, launch_encode16_fast(q, fast_in, aligned_out, ctx->stream));
            span_end(ctx);
            return DBDE_HIP_OK;
        }
    }
    // workspace, zeroed before the launch: [ticket 16 B][state 8 n cpf][gsum 8 n gpf][fsize 8 n][fgsum 8 ceil(n / 64)]
    const size_t n = (size_t)n_frames, gpf = (cpf + 63) / 64;
    const size_t need = 16 + 8 * (n * cpf + n * gpf + n + (n + 63) / 64);
    int rc = grow(ctx, ctx->w16, ctx->w16_bytes, need, 1, true);
    if (rc) return rc;
    dbde16::Params16 p;
    p.images = d_images;
    p.out = d_out;
    p.frame_offsets = d_frame_offsets;
    p.frame_bytes = d_frame_bytes;
    p.first_index = first_index;
    p.slot_stride = slot_stride;
    p.frame_pixels = g.pixels;
    p.W = W; p.H = H; p.w = g.w; p.h = g.h; p.T = g.T;
    p.chunks_per_frame = cpf;
    p.n_frames = (uint32_t)n_frames;
    p.ticket = reinterpret_cast<uint32_t *>(ctx->w16);
    p.state = reinterpret_cast<unsigned long long *>(ctx->w16 + 16);
    p.gsum = p.state + n * cpf;
    p.fsize = p.gsum + n * gpf;
    p.fgsum = p.fsize + n;
    p.sticky = ctx->sticky;
    p.diag = reinterpret_cast<unsigned long long *>(ctx->diag);
    if (!ctx->enc16_grid) ctx->enc16_grid = (uint32_t)(dbde16::encode16_blocks_per_cu() * ctx->n_cu);
    span_begin(ctx, 0);
    HIP_TRY(ctx, hipMemsetAsync(ctx->w16, 0, need, ctx->stream));
    p.force_tickets = (ctx->exp_flags & 1u) ? 1u : 0u;
    HIP_TRY(ctx, dbde16::launch_encode16(p, n_frames, ctx->enc16_grid, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

// ---- window encode (include/dbde_hip.h) ------------------------------------------------------------
struct WencPlan {
    Geometry g;                       // of the window
    uint64_t pitch, frame_stride, min_image_bytes, max_frame, capacity, workspace;
    uint32_t lanes_per_row, units, cpf;
    bool forwards;
    int code;                         // of the broken rule
};
// nullptr when the arguments are good, else what is wrong with them (pl.code: the error code).  pix: 1 = DBDE, 2 = DBDE16.
static const char *plan_wenc(uint64_t image_address, uint64_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                             int n_frames, int x0, int y0, int rw, int rh, bool has_origins, uint64_t out_capacity,
                             bool check_capacity, uint64_t slot_stride, uint32_t pix, WencPlan &pl) {
    pl.code = DBDE_HIP_ERR_ARG;
    Geometry src;
    if (n_frames < 0) return "n_frames < 0";
    if (!geometry(W, H, src)) return "bad source size";
    if (rw < 1 || rh < 1 || rw > W || rh > H) return "window size outside [1, W] x [1, H]";
    if (x0 < 0 || y0 < 0 || x0 > W - rw || y0 > H - rh) return "window origin outside [0, W-rw] x [0, H-rh]";
    if (!geometry(rw, rh, pl.g)) return "window too large";
    const uint64_t row_bytes = (uint64_t)W * pix;
    pl.pitch = pitch ? pitch : row_bytes;
    if (pl.pitch < row_bytes) return "pitch below W * PIX";
    if (pl.pitch >= (1ull << 40)) return "pitch too large";
    const uint64_t frame_extent = (uint64_t)(H - 1) * pl.pitch + row_bytes;
    pl.frame_stride = frame_stride ? frame_stride : (uint64_t)H * pl.pitch;
    if (pl.frame_stride < frame_extent) return "frame_stride below (H-1) * pitch + W * PIX";
    if (pl.frame_stride >= (1ull << 48)) return "frame_stride too large";
    if (pix == 2u && ((pl.pitch | pl.frame_stride | image_address) & 1u)) return "DBDE16: odd pitch, frame_stride or base address";
    pl.min_image_bytes = n_frames ? (uint64_t)(n_frames - 1) * pl.frame_stride + frame_extent : 0u;
    if (image_bytes < pl.min_image_bytes) return "image_bytes below (n-1) * frame_stride + (H-1) * pitch + W * PIX";
    pl.max_frame = 32ull + (pix == 2u ? 131ull : 66ull) * pl.g.T;
    pl.capacity = n_frames == 0 ? 0u : (slot_stride ? (uint64_t)(n_frames - 1) * slot_stride + pl.max_frame : (uint64_t)n_frames * pl.max_frame);
    if (slot_stride && slot_stride < pl.max_frame) {
        if (pix == 2u) pl.code = DBDE_HIP_ERR_CAPACITY;   // (each as its frame encoder reports it)
        return "slot_stride below the window's worst case";
    }
    if (check_capacity && out_capacity < pl.capacity) { pl.code = DBDE_HIP_ERR_CAPACITY; return "out_capacity below the worst case"; }
    pl.forwards = !has_origins && rw == W && rh == H && pl.pitch == row_bytes && pl.frame_stride == (uint64_t)H * row_bytes;
    pl.lanes_per_row = pix == 2u ? pl.g.w : (pl.g.w + 1u) / 2u;
    const uint64_t units = (uint64_t)pl.g.h * pl.lanes_per_row;
    pl.units = (uint32_t)units;
    pl.cpf = (uint32_t)((units + kWencThreads - 1u) / kWencThreads);
    if (!pl.forwards && (uint64_t)n_frames * pl.cpf >= (1ull << 31)) return "too many chunks in one call";
    const uint64_t n = (uint64_t)n_frames, gpf = (pl.cpf + kWencGroup - 1u) / kWencGroup;
    pl.workspace = 16u + 8u * (n * pl.cpf + n * gpf + n + (n + kWencGroup - 1u) / kWencGroup);
    return nullptr;
}

static int wenc_plan_common(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                            int n_frames, int x0, int y0, int rw, int rh, int has_origins, size_t out_capacity,
                            uint64_t slot_stride, int n_cu, uint32_t pix, dbde_hip_window_encode_plan_t *plan) {
    WencPlan pl;
    if (!plan || n_cu < 1) return DBDE_HIP_ERR_ARG;
    if (plan_wenc(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw, rh, has_origins != 0,
                  out_capacity, out_capacity != 0, slot_stride, pix, pl))
        return pl.code;
    memset(plan, 0, sizeof *plan);
    plan->forwards = pl.forwards ? 1u : 0u;
    plan->tiles_x = pl.g.w;
    plan->tiles_y = pl.g.h;
    plan->tiles = pl.g.T;
    plan->pitch = pl.pitch;
    plan->frame_stride = pl.frame_stride;
    plan->min_image_bytes = pl.min_image_bytes;
    plan->max_out_frame_bytes = pl.max_frame;
    plan->out_capacity = pl.capacity;
    if (pl.forwards) return DBDE_HIP_OK;
    plan->lanes_per_row = pl.lanes_per_row;
    plan->chunks_per_frame = pl.cpf;
    plan->chunk_tiles = wenc_chunk_tiles(pix);
    plan->record_group = kWencGroup;
    plan->threads = kWencThreads;
    plan->lds_bytes = kWencLdsBytes;
    const uint64_t chunks = (uint64_t)n_frames * pl.cpf, resident = (uint64_t)n_cu * kWencBlocksPerCu;
    plan->grid = chunks < resident ? chunks : resident;
    plan->workspace_bytes = pl.workspace;
    return DBDE_HIP_OK;
}

int dbde_hip_window_encode_plan(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                                int n_frames, int x0, int y0, int rw, int rh, int has_origins, size_t out_capacity,
                                uint64_t slot_stride, int n_cu, dbde_hip_window_encode_plan_t *plan) {
    return wenc_plan_common(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw, rh, has_origins,
                            out_capacity, slot_stride, n_cu, 1u, plan);
}

int dbde16_hip_window_encode_plan(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch, uint64_t frame_stride,
                                  int n_frames, int x0, int y0, int rw, int rh, int has_origins, size_t out_capacity,
                                  uint64_t slot_stride, int n_cu, dbde_hip_window_encode_plan_t *plan) {
    return wenc_plan_common(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw, rh, has_origins,
                            out_capacity, slot_stride, n_cu, 2u, plan);
}

// Both window encoders (pix: 1 = DBDE, 2 = DBDE16), timing slot 0.
static int encode_window_common(dbde_hip_ctx *ctx, const char *name, uint32_t pix, const uint8_t *d_images, size_t image_bytes,
                                int W, int H, uint64_t pitch, uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh,
                                const int32_t *d_origins, uint64_t first_index, const uint64_t *d_indices,
                                const uint64_t *d_elapsed_ns, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                                uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    WencPlan pl;
    if (const char *why = plan_wenc(reinterpret_cast<uintptr_t>(d_images), image_bytes, W, H, pitch, frame_stride, n_frames, x0,
                                    y0, rw, rh, d_origins != nullptr, out_capacity, true, slot_stride, pix, pl))
        return fail(ctx, pl.code, "%s: %s (W=%d H=%d pitch=%llu stride=%llu n=%d window %dx%d at %d,%d)", name, why, W, H,
                    (unsigned long long)pitch, (unsigned long long)frame_stride, n_frames, rw, rh, x0, y0);
    if (!d_images || !d_out) return fail(ctx, DBDE_HIP_ERR_ARG, "%s: null pointer", name);
    if (n_frames == 0) return DBDE_HIP_OK;
    if (pl.forwards)   // exactly the frame encoders' layout: the plain case stays on the persistent encoder
        return pix == 2u ? dbde16_hip_encode_frames(ctx, reinterpret_cast<const uint16_t *>(d_images), W, H, n_frames, first_index,
                                                    d_out, out_capacity, slot_stride, d_frame_offsets, d_frame_bytes)
                         : dbde_hip_encode_frames(ctx, d_images, W, H, n_frames, first_index, d_indices, d_elapsed_ns, d_out,
                                                  out_capacity, slot_stride, d_frame_offsets, d_frame_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = grow(ctx, ctx->w16, ctx->w16_bytes, (size_t)pl.workspace, 1, true);
    if (rc) return rc;
    WencParams p;
    memset(&p, 0, sizeof p);
    p.images = d_images;
    p.image_bytes = image_bytes;
    p.pitch = pl.pitch;
    p.frame_stride = pl.frame_stride;
    p.origins = d_origins;
    p.W = W; p.H = H; p.x0 = x0; p.y0 = y0; p.rw = rw; p.rh = rh;
    p.narrow = (uint32_t)rw * pix < 16u ? 1u : 0u;
    p.out = d_out;
    p.frame_offsets = d_frame_offsets;
    p.frame_bytes = d_frame_bytes;
    p.indices = d_indices;
    p.elapsed_ns = d_elapsed_ns;
    p.first_index = first_index;
    p.slot_stride = slot_stride;
    p.w = pl.g.w; p.h = pl.g.h; p.T = pl.g.T;
    p.lanes_per_row = pl.lanes_per_row;
    p.units = pl.units;
    p.chunks_per_frame = pl.cpf;
    p.n_frames = (uint32_t)n_frames;
    const size_t n = (size_t)n_frames, gpf = (pl.cpf + kWencGroup - 1u) / kWencGroup;
    p.ticket = reinterpret_cast<uint32_t *>(ctx->w16);
    p.state = reinterpret_cast<unsigned long long *>(ctx->w16 + 16);
    p.gsum = p.state + n * pl.cpf;
    p.fsize = p.gsum + n * gpf;
    p.fgsum = p.fsize + n;
    p.sticky = ctx->sticky;
    p.force_tickets = (ctx->exp_flags & 1u) ? 1u : 0u;
    uint32_t &resident = ctx->wenc_grid[pix - 1u];
    if (!resident) resident = (uint32_t)(wenc_blocks_per_cu(pix) * ctx->n_cu);
    span_begin(ctx, 0);
    HIP_TRY(ctx, hipMemsetAsync(ctx->w16, 0, (size_t)pl.workspace, ctx->stream));
    HIP_TRY(ctx, launch_encode_window(p, pix, (ctx->exp_flags & 1024u) ? 3u : resident, ctx->stream));   // (experiment bit 10: three workgroups)
    span_end(ctx);
    return DBDE_HIP_OK;
}

int dbde_hip_encode_window(dbde_hip_ctx *ctx, const uint8_t *d_images, size_t image_bytes, int W, int H, uint64_t pitch,
                           uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                           uint64_t first_index, const uint64_t *d_indices, const uint64_t *d_elapsed_ns, uint8_t *d_out,
                           size_t out_capacity, uint64_t slot_stride, uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    return encode_window_common(ctx, "encode_window", 1u, d_images, image_bytes, W, H, pitch, frame_stride, n_frames, x0, y0, rw,
                                rh, d_origins, first_index, d_indices, d_elapsed_ns, d_out, out_capacity, slot_stride,
                                d_frame_offsets, d_frame_bytes);
}

int dbde16_hip_encode_window(dbde_hip_ctx *ctx, const uint16_t *d_images, size_t image_bytes, int W, int H, uint64_t pitch,
                             uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh, const int32_t *d_origins,
                             uint64_t first_index, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                             uint64_t *d_frame_offsets, uint64_t *d_frame_bytes) {
    return encode_window_common(ctx, "encode_window16", 2u, reinterpret_cast<const uint8_t *>(d_images), image_bytes, W, H, pitch,
                                frame_stride, n_frames, x0, y0, rw, rh, d_origins, first_index, nullptr, nullptr, d_out,
                                out_capacity, slot_stride, d_frame_offsets, d_frame_bytes);
}

int dbde16_hip_decode_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                             int W, int H, int n_frames, uint16_t *d_images, dbde_hip_frame_result *d_results) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    Geometry g;
    if (!d_stream || !d_frame_offsets || !d_images || n_frames < 0 || !geometry(W, H, g))
        return fail(ctx, DBDE_HIP_ERR_ARG, "decode16: bad argument (W=%d H=%d n=%d)", W, H, n_frames);
    if (n_frames == 0) return DBDE_HIP_OK;
    const DecGeom dg = dec_geometry(g.w, g.h, false, dbde16::kChunkTiles16);   // plain runs of 256 tiles
    if (dg.cpf > kMaxChunksPerFrame) return fail(ctx, DBDE_HIP_ERR_ARG, "decode16: frame too large");
    const uint64_t n_chunks64 = (uint64_t)n_frames * dg.cpf;
    if (n_chunks64 >= (1ull << 31)) return fail(ctx, DBDE_HIP_ERR_ARG, "decode16: too many chunks in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // U16 minima, depth <= 16, nm = 2T; one index workgroup per frame (the split form is a latency tool of the 8-bit path)
    int rc = run_index(ctx, d_stream, stream_bytes, d_frame_offsets, n_frames, d_results, dg, 2u, 1u);
    if (rc) return rc;
    dbde16::DecParams16 p;
    p.stream = d_stream;
    p.stream_bytes = stream_bytes;
    p.frame_offsets = d_frame_offsets;
    p.images = d_images;
    p.chunk_off = ctx->chunk_off;
    p.frame_ok = ctx->frame_ok;
    p.frame_pixels = g.pixels;
    p.W = W; p.H = H; p.w = g.w; p.h = g.h; p.T = g.T;
    p.chunks_per_frame = dg.cpf;
    p.diag = reinterpret_cast<unsigned long long *>(ctx->diag);
    span_begin(ctx, 2);
    HIP_TRY(ctx, dbde16::launch_decode16(p, n_frames, ctx->stream));
    span_end(ctx);
    return DBDE_HIP_OK;
}

// ---- host-pointer entry points ---------------------------------------------------------------

// Device -> host on the context's OWN stream (hipMemcpy would go through the null stream, where the calls of every thread
// of a multi-threaded caller queue up behind each other).
static bool d2h(dbde_hip_ctx *ctx, void *dst, const void *src, size_t n, uint8_t *via = nullptr) {
    void *land = ctx->host_staging && via ? via : dst;
    if (hipMemcpyAsync(land, src, n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
    if (land != dst) memcpy(dst, land, n);
    return true;
}

// Encodes one host image through the GPU; returns the frame's byte count and leaves the
// packed frame (header + data) in ctx->st_pack.  0 on failure.
static size_t encode_one_host(dbde_hip_ctx *ctx, uint64_t index, const uint8_t *image, int W, int H) {
    Geometry g;
    if (!ctx || !image || !geometry(W, H, g)) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) return 0;   // (the calling thread may never have touched this device)
    const size_t maxf = 32 + 66 * (size_t)g.T;
    if (ensure_staging(ctx, (size_t)g.pixels, maxf)) return 0;
    if (!h2d(ctx, ctx->st_img, image, (size_t)g.pixels, ctx->h_img)) return 0;
    // the byte count lands in pinned host memory, written by the kernel itself: nothing small travels between the image
    // going in and the frame coming out (a copy of 8 bytes costs the link what a hundred kilobytes cost it)
    volatile uint64_t *h_bytes = ctx->h_words;
    *h_bytes = 0;
    if (dbde_hip_encode_frames(ctx, ctx->st_img, W, H, 1, index, nullptr, nullptr, ctx->st_pack, maxf, 0, nullptr,
                               const_cast<uint64_t *>(h_bytes)) != DBDE_HIP_OK)
        return 0;
    // One frame is a launch of the small, tiny or mid encoders, which cannot raise the sticky failure word (their waits
    // end in a fallback); only a frame of more chunks than the device holds workgroups runs the persistent encoder
    Geometry gg = g;
    const EncPlan pl = plan_encode(gg, W, 1, reinterpret_cast<uintptr_t>(ctx->st_img), reinterpret_cast<uintptr_t>(ctx->st_pack), 0, ctx->enc_grid);
    if (pl.kernel == 0) { if (dbde_hip_sync(ctx) != DBDE_HIP_OK) return 0; }
    else if (hipStreamSynchronize(ctx->stream) != hipSuccess) return 0;
    const uint64_t nbytes = *h_bytes;
    return nbytes <= maxf ? (size_t)nbytes : 0;
}

size_t dbde_hip_pack_frame(dbde_hip_ctx *ctx, uint64_t index, const uint8_t *image, int W, int H, uint8_t *target) {
    size_t n = encode_one_host(ctx, index, image, W, H);
    if (!n || !target) return 0;
    if (!d2h(ctx, target, ctx->st_pack, n, ctx->h_pack)) return 0;
    return n;
}

size_t dbde_hip_pack_image(dbde_hip_ctx *ctx, const uint8_t *image, int W, int H, uint8_t *target) {
    size_t n = encode_one_host(ctx, 0, image, W, H);
    if (n <= 20 || !target) return 0;
    if (!d2h(ctx, target, ctx->st_pack + 20, n - 20, ctx->h_pack)) return 0;
    return n - 20;
}

uint32_t dbde_hip_pack_8x8_partial(dbde_hip_ctx *ctx, const uint8_t *image, int stride, int rightmargin,
                                   int downmargin, uint8_t *target) {
    // A rm x dm image is exactly one constant-padded tile (dbde_util.cpp:105-135).
    if (!ctx || !image || rightmargin < 1 || downmargin < 1) return 0;
    const int rm = rightmargin > 8 ? 8 : rightmargin, dm = downmargin > 8 ? 8 : downmargin;
    uint8_t dense[64];
    for (int r = 0; r < dm; r++) memcpy(dense + r * rm, image + (ptrdiff_t)r * stride, (size_t)rm);   // gather only
    size_t n = encode_one_host(ctx, 0, dense, rm, dm);
    if (n < 34) return 0;
    uint8_t head[34 + 64];
    if (!d2h(ctx, head, ctx->st_pack, n)) return 0;
    // T = 1: header 20 | nb 4 | depth 1 | nm 4 | min 1 | n64 4 | payload
    const uint32_t depth = head[24], mn = head[29];
    if (target && depth) memcpy(target, head + 34, 8u * depth);
    return (depth << 8) | mn;
}

uint32_t dbde_hip_pack_8x8(dbde_hip_ctx *ctx, const uint8_t *image, int stride, uint8_t *target) {
    return dbde_hip_pack_8x8_partial(ctx, image, stride, 8, 8, target);
}

// Runs index + decode for one frame_data already resident at ctx->st_pack + 20 (a dummy
// frame header precedes it).  Returns bytes of frame data consumed (0 = rejected) and leaves
// the image in ctx->st_img.
static size_t decode_one_staged(dbde_hip_ctx *ctx, size_t staged_bytes, int W, int H) {
    Geometry g;
    if (!geometry(W, H, g)) return 0;
    uint64_t *d_off = ctx->scratch64 + 2;   // a zero that lives in device memory (cleared when the context was made, never written)
    // the frame's result record is written by the kernel straight into pinned host memory
    volatile dbde_hip_frame_result *h_res = reinterpret_cast<volatile dbde_hip_frame_result *>(ctx->h_words + 1);
    h_res->consumed = 0;
    if (dbde_hip_decode_frames(ctx, ctx->st_pack, staged_bytes, d_off, W, H, 1, ctx->st_img,
                               const_cast<dbde_hip_frame_result *>(h_res)) != DBDE_HIP_OK) return 0;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return 0;   // (decode kernels have no sticky failure)
    const uint64_t consumed = h_res->consumed;
    return consumed > 20 ? (size_t)(consumed - 20) : 0;
}

size_t dbde_hip_unpack_image(dbde_hip_ctx *ctx, const uint8_t *packed, int W, int H, uint8_t *image) {
    Geometry g;
    if (!ctx || !packed || !image || !geometry(W, H, g)) return 0;
    // Only to learn how many bytes to move: the first I32 and the word count
    // (validation proper happens on the device, dbde_util.cpp:295-303 order preserved).
    if ((int32_t)get32(packed) != (int32_t)g.T) return 0;
    if ((int32_t)get32(packed + 4 + g.T) != (int32_t)g.T) return 0;
    const int32_t n64 = (int32_t)get32(packed + 8 + 2 * (size_t)g.T);
    if (n64 < 0 || (uint64_t)n64 > 8ull * g.T) return 0;   // cannot equal sum(depth) with depth <= 8
    const size_t body = 12 + 2 * (size_t)g.T + 8 * (size_t)n64;
    if (hipSetDevice(ctx->device) != hipSuccess) return 0;
    if (ensure_staging(ctx, (size_t)g.pixels, 20 + body + 128)) return 0;
    // a frame header in front of the caller's frame data: device to device (a 20-byte copy from the stack was a trip over the link)
    if (hipMemcpyAsync(ctx->st_pack, ctx->d_hdr, 20, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return 0;
    if (!h2d(ctx, ctx->st_pack + 20, packed, body, ctx->h_pack)) return 0;
    const size_t used = decode_one_staged(ctx, 20 + body, W, H);
    if (!used) return 0;
    if (!d2h(ctx, image, ctx->st_img, (size_t)g.pixels, ctx->h_img)) return 0;
    return used;
}

size_t dbde_hip_unpack_image_roi(dbde_hip_ctx *ctx, const uint8_t *packed, int W, int H, int x0, int y0, int rw, int rh,
                                 uint8_t *image) {
    RoiPlan pl;
    if (!ctx || !packed || !image || plan_roi(W, H, 1, x0, y0, rw, rh, pl)) return 0;
    const Geometry &g = pl.g;
    // as dbde_hip_unpack_image: the host reads only what it needs to know how many bytes to move
    if ((int32_t)get32(packed) != (int32_t)g.T) return 0;
    if ((int32_t)get32(packed + 4 + g.T) != (int32_t)g.T) return 0;
    const int32_t n64 = (int32_t)get32(packed + 8 + 2 * (size_t)g.T);
    if (n64 < 0 || (uint64_t)n64 > 8ull * g.T) return 0;
    const size_t body = 12 + 2 * (size_t)g.T + 8 * (size_t)n64;
    const size_t win = (size_t)rw * (size_t)rh;
    if (hipSetDevice(ctx->device) != hipSuccess) return 0;
    if (ensure_staging(ctx, win, 20 + body + 128)) return 0;
    if (hipMemcpyAsync(ctx->st_pack, ctx->d_hdr, 20, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return 0;
    if (!h2d(ctx, ctx->st_pack + 20, packed, body, ctx->h_pack)) return 0;
    uint64_t *d_off = ctx->scratch64 + 2;   // a zero in device memory
    volatile dbde_hip_frame_result *h_res = reinterpret_cast<volatile dbde_hip_frame_result *>(ctx->h_words + 1);
    h_res->consumed = 0;
    if (dbde_hip_decode_roi(ctx, ctx->st_pack, 20 + body, d_off, W, H, 1, x0, y0, rw, rh, nullptr, ctx->st_img,
                            const_cast<dbde_hip_frame_result *>(h_res)) != DBDE_HIP_OK) return 0;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return 0;
    const uint64_t consumed = h_res->consumed;
    if (consumed <= 20) return 0;
    if (!d2h(ctx, image, ctx->st_img, win, ctx->h_img)) return 0;
    return (size_t)(consumed - 20);
}

dbde_hip_frame_header dbde_hip_unpack_frame(dbde_hip_ctx *ctx, uint8_t **packed, int W, int H, uint8_t *image) {
    dbde_hip_frame_header fh = dbde_hip_unpack_frame_header(packed);   // advances by 20 (dbde_util.cpp:340)
    const size_t n = dbde_hip_unpack_image(ctx, *packed, W, H, image);
    if (n == 0) fh.u64s = 0xFFFFFFFFu;   // dbde_util.cpp:342
    else *packed += n;
    return fh;
}

void dbde_hip_unpack_8x8_partial(dbde_hip_ctx *ctx, uint8_t depth, uint8_t minval, const uint8_t *packed,
                                 size_t stride, int rightmargin, int downmargin, uint8_t *image) {
    if (!ctx || !image || depth > 8 || rightmargin < 1 || downmargin < 1) return;
    const int rm = rightmargin > 8 ? 8 : rightmargin, dm = downmargin > 8 ? 8 : downmargin;
    // frame data of a one-tile rm x dm frame
    uint8_t body[14 + 64];
    put32(body, 1);
    body[4] = depth;
    put32(body + 5, 1);
    body[9] = minval;
    put32(body + 10, depth);
    if (depth) memcpy(body + 14, packed, 8u * depth);
    uint8_t dense[64];
    if (dbde_hip_unpack_image(ctx, body, rm, dm, dense) == 0) return;
    for (int r = 0; r < dm; r++) memcpy(image + r * stride, dense + r * rm, (size_t)rm);   // scatter only
}

void dbde_hip_unpack_8x8(dbde_hip_ctx *ctx, uint8_t depth, uint8_t minval, const uint8_t *packed, size_t stride,
                         uint8_t *image) {
    dbde_hip_unpack_8x8_partial(ctx, depth, minval, packed, stride, 8, 8, image);
}

// ---- header wire format ----------------------------------------------------------------------

size_t dbde_hip_pack_frame_header(const dbde_hip_frame_header *fh, uint8_t *target) {
    put32(target, fh->u64s);
    put64(target + 4, fh->index);
    const double el = (double)fh->elapsed_ns;   // the reference stores a double here (dbde_util.cpp:186)
    uint64_t bits;
    memcpy(&bits, &el, 8);
    put64(target + 12, bits);
    return 20;
}

size_t dbde_hip_pack_video_header(const dbde_hip_video_header *vh, uint8_t *target) {
    put32(target, vh->u64s);
    put64(target + 4, vh->height);
    put64(target + 12, vh->width);
    uint64_t bits;
    memcpy(&bits, &vh->frame_hz, 8);
    put64(target + 20, bits);
    return 28;
}

// The reference's `(uint64_t)el` (dbde_util.cpp:334) as g++ compiles it for x86-64, the host twin of the device
// f64_to_u64_x86: cvttsd2si below 2^63, else cvttsd2si(v - 2^63) ^ 2^63; out of range and NaN give the "integer
// indefinite" 2^63, so 2^64 and above (+inf included) read as 0.  A plain cast here does not do that: how a compiler
// converts an out-of-range double is its own choice (clang's branch-free form gives 2^63 from 2^64 on).
static uint64_t f64_to_u64_x86_host(double v) {
    const double two63 = 9223372036854775808.0;
    const bool high = v >= two63;       // false for NaN
    const double a = high ? v - two63 : v;
    uint64_t r = 0x8000000000000000ull;
    if (a >= -two63 && a < two63) r = (uint64_t)(long long)a;   // truncates toward zero
    return high ? (r ^ 0x8000000000000000ull) : r;
}

dbde_hip_frame_header dbde_hip_unpack_frame_header(uint8_t **packed) {
    dbde_hip_frame_header fh;
    const uint8_t *p = *packed;
    fh.u64s = get32(p);
    fh.index = get64(p + 4);
    const uint64_t bits = get64(p + 12);
    double el;
    memcpy(&el, &bits, 8);
    fh.elapsed_ns = f64_to_u64_x86_host(el);
    if (fh.u64s != 2) fh.u64s = 0xFFFFFFFFu;
    *packed += 20;
    return fh;
}

dbde_hip_video_header dbde_hip_unpack_video_header(uint8_t **packed) {
    dbde_hip_video_header vh;
    const uint8_t *p = *packed;
    vh.u64s = get32(p);
    vh.height = get64(p + 4);
    vh.width = get64(p + 12);
    const uint64_t bits = get64(p + 20);
    memcpy(&vh.frame_hz, &bits, 8);
    if (vh.u64s != 3) vh.u64s = 0xFFFFFFFFu;
    *packed += 28;
    return vh;
}

// ---- timing ----------------------------------------------------------------------------------

// Diagnostic builds (-DDBDE_DIAG) accumulate in-kernel cycle counters; this reads (and clears) them.
// Not part of include/dbde_hip.h: tuning tool (profiles/abbench.cpp) only.
int dbde_hip_diag_read(dbde_hip_ctx *ctx, uint64_t out[16]) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->diag, 128, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->diag, 0, 128, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DBDE_HIP_OK;
}
#ifdef DBDE_DIAG
// [1024][16] u64: wave 0's wall clock (10 ns) at the points of a persistent-encoder workgroup's life (encode_kernel).
int dbde_hip_diag_trace_read(dbde_hip_ctx *ctx, uint64_t *out, size_t n_u64) {
    if (!ctx || n_u64 > 16 * 1024) return DBDE_HIP_ERR_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->diag + 16, 8 * n_u64, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->diag + 16, 0, 8 * 16 * 1024, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DBDE_HIP_OK;
}
#endif

int dbde_hip_timing_enable(dbde_hip_ctx *ctx, int on) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    ctx->timing = on != 0;
    return DBDE_HIP_OK;
}

int dbde_hip_timing_read(dbde_hip_ctx *ctx, double ms[4], uint64_t launches[4], int reset) {
    if (!ctx) return DBDE_HIP_ERR_ARG;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->scan_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->scan_stream));
    for (auto &s : ctx->spans) {
        float t = 0;
        if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) {
            ctx->acc_ms[s.kind] += t;
            ctx->acc_n[s.kind] += 1;
        }
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
    }
    ctx->spans.clear();
    for (int k = 0; k < 4; k++) {
        if (ms) ms[k] = ctx->acc_ms[k];
        if (launches) launches[k] = ctx->acc_n[k];
        if (reset) { ctx->acc_ms[k] = 0; ctx->acc_n[k] = 0; }
    }
    return DBDE_HIP_OK;
}

}  // extern "C"
