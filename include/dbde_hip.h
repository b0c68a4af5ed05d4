/*
 * dbde_hip.h -- C-ABI of the MI355X (gfx950) DBDE frame codec: libdbde_hip.so.
 *
 * This is the drop-in boundary for the reference's hot path, dbde_util.h:21-37
 * (dbde_pack_* / dbde_unpack_*).  Plain C: pointers, sizes and fixed-width integers only.
 * Two layers live behind it:
 *
 *   1. the batch API on DEVICE-RESIDENT buffers (dbde_hip_encode_frames /
 *      dbde_hip_decode_frames): N frames per launch, what bench.py measures;
 *   2. host-pointer entry points with the argument meaning of the reference functions they
 *      replace (each cites its reference line); include/dbde_util.h re-exports them under
 *      the reference's own C++ names, so code written against the reference links unchanged.
 *
 * All compute runs in hand-written HIP kernels (csrc/dbde_kernels.hip).  There is no CPU
 * fallback: every entry point fails with DBDE_HIP_ERR_HIP when no gfx950 device is usable.
 *
 * Wire format (all little-endian; reference README.md:12-67, dbde_util.cpp:137-209):
 *   stream := video_header(28 B) { frame_header(20 B) frame_data }*
 *   frame_data := I32 T | U8 depth[T] | I32 T | U8 min[T] | I32 n64 | U64 data[n64]
 *   T = ceil(W/8)*ceil(H/8) 8x8 tiles, row-major; n64 = sum(depth)
 */
#ifndef DBDE_HIP_H
#define DBDE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dbde_hip_ctx dbde_hip_ctx;

enum {
    DBDE_HIP_OK = 0,
    DBDE_HIP_ERR_ARG = -1,       /* bad argument (null pointer, W/H out of range, ...) */
    DBDE_HIP_ERR_HIP = -2,       /* HIP runtime error or no usable gfx950 device */
    DBDE_HIP_ERR_CAPACITY = -3,  /* output buffer smaller than the worst case */
    DBDE_HIP_ERR_DEVICE = -4     /* a kernel reported failure (look-back time-out) */
};

/* In-memory headers, field-for-field the reference's structs (dbde_util.h:8-19). */
typedef struct {
    uint32_t u64s;
    uint64_t height;
    uint64_t width;
    double frame_hz;
} dbde_hip_video_header;

typedef struct {
    uint32_t u64s;       /* 2, or 0xFFFFFFFF when the frame failed to parse (dbde_util.cpp:335,342) */
    uint64_t index;
    uint64_t elapsed_ns;
} dbde_hip_frame_header;

/* Per-frame result of a batch decode (device memory, one per frame). */
typedef struct {
    dbde_hip_frame_header header;  /* as dbde_unpack_frame would return it */
    uint64_t consumed;             /* bytes the reference would advance *packed by (20 on failure) */
} dbde_hip_frame_result;

/* ---- context -------------------------------------------------------------------------- */

/* Creates a context on HIP device `device`.  `stream` is a hipStream_t (or NULL for the
 * default stream) on which every kernel and copy of this context is enqueued; the caller
 * keeps ownership of it.  Workspace (look-back state, decode index, staging buffers for the
 * host-pointer entry points) is owned by the context and grown on demand. */
int dbde_hip_create(int device, void *stream, dbde_hip_ctx **out);
/* The same with a stream of the context's OWN (non-blocking, destroyed with it): what a caller without the HIP headers
 * needs to run several contexts side by side -- the drop-in shim keeps a pool of these, one per calling thread at a
 * time, so that the reference's re-entrant API (dbde_util.h:21-37: no global state) scales with the caller's threads. */
int dbde_hip_create_on_own_stream(int device, dbde_hip_ctx **out);
/* How the host-pointer entry points (dbde_hip_pack_frame ...) move the caller's bytes: 0 (default) straight from / to
 * the caller's pageable memory (the runtime pins it per call: fastest for ONE caller, but that pinning serialises
 * concurrent callers), 1 through pinned buffers of the context (a memcpy by the calling thread each way, DMA that never
 * pins: scales with the number of calling threads).  The drop-in shim switches per call by how many calls are in flight. */
int dbde_hip_set_host_staging(dbde_hip_ctx *ctx, int pinned);
void dbde_hip_destroy(dbde_hip_ctx *ctx);
/* Blocks until everything enqueued by this context has finished; returns
 * DBDE_HIP_ERR_DEVICE if a kernel raised its failure flag since the last call. */
int dbde_hip_sync(dbde_hip_ctx *ctx);
const char *dbde_hip_last_error(const dbde_hip_ctx *ctx);
/* Name of the device the context runs on (e.g. "gfx950:sramecc+:xnack-"). */
const char *dbde_hip_device_arch(const dbde_hip_ctx *ctx);
/* The hipStream_t and HIP device index the context was created with. */
void *dbde_hip_stream_handle(const dbde_hip_ctx *ctx);
int dbde_hip_device_index(const dbde_hip_ctx *ctx);

/* ---- sizes ---------------------------------------------------------------------------- */

/* Worst-case bytes of one packed frame incl. its 20-byte header: 20 + 12 + 66*T
 * (the bound the reference's test allocates, dbde_util_test.cpp:78). */
size_t dbde_hip_max_frame_bytes(int W, int H);
/* Exact bytes of frame_data for a frame with n64 payload words: 12 + 2T + 8*n64. */
size_t dbde_hip_image_bytes(int W, int H, uint64_t n64);

/* ---- batch API, device pointers (the measured path) ----------------------------------- */

/* Encodes n_frames images (contiguous, W*H bytes each, row-major U8, pitch W) into DBDE
 * frames (frame header + frame data each), replacing n_frames calls of dbde_pack_frame
 * (dbde_util.cpp:190-196).
 *   d_indices    : optional frame numbers (device, n_frames); NULL -> first_index + f
 *   d_elapsed_ns : optional elapsed_ns per frame (device); NULL -> 0 as dbde_pack_frame writes
 *   d_out        : output bytes (device), capacity out_capacity
 *   slot_stride  : 0 -> frames are CONCATENATED from d_out (a ready-to-write .dbde body);
 *                  else frame f starts at d_out + f*slot_stride (>= dbde_hip_max_frame_bytes)
 *   d_frame_offsets / d_frame_bytes : optional outputs (device, n_frames each): byte offset of
 *                  each frame from d_out and its exact length.
 * Asynchronous on the context's stream.  out_capacity must cover the worst case
 * (n_frames * dbde_hip_max_frame_bytes, or (n_frames-1)*slot_stride + max). */
int dbde_hip_encode_frames(dbde_hip_ctx *ctx, const uint8_t *d_images, int W, int H, int n_frames,
                           uint64_t first_index, const uint64_t *d_indices,
                           const uint64_t *d_elapsed_ns, uint8_t *d_out, size_t out_capacity,
                           uint64_t slot_stride, uint64_t *d_frame_offsets,
                           uint64_t *d_frame_bytes);

/* Decodes n_frames frames, replacing n_frames calls of dbde_unpack_frame
 * (dbde_util.cpp:339-345).  Frame f starts at d_stream + d_frame_offsets[f] (any byte
 * alignment).  stream_bytes is the readable extent of d_stream.  A frame whose frame data
 * fails validation (nb != T, nm != T, n64 != sum(depth): dbde_util.cpp:295-303; or a depth
 * byte > 8, the one documented deviation) leaves its image untouched and reports
 * header.u64s = 0xFFFFFFFF, consumed = 20.  d_results may be NULL. */
int dbde_hip_decode_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           uint8_t *d_images, dbde_hip_frame_result *d_results);

/* Window (region-of-interest) decode: the rw x rh window at (x, y) of each of n_frames frames, decoding only the tiles
 * the window covers.  Frame f starts at d_stream + d_frame_offsets[f] (any byte alignment); its window
 * goes to d_out + f*rw*rh, row-major, pitch rw, any byte alignment, and equals rows [y, y+rh) x columns [x, x+rw) of
 * the image dbde_hip_decode_frames would write, byte for byte.
 *   d_origins: optional device int32 [n_frames][2] (x, y) per frame, CLAMPED into [0, W-rw] x [0, H-rh] (a tracker's
 *              moving window).  NULL -> (x0, y0) for every frame.  (x0, y0) must lie in [0, W-rw] x [0, H-rh] either way
 *              (pass 0, 0 with per-frame origins); a host origin outside the frame is DBDE_HIP_ERR_ARG.
 *   d_results: as in dbde_hip_decode_frames (header fields; consumed = the whole frame's length), may be NULL.
 * Validation is dbde_hip_decode_frames' own (the same index kernel): a rejected frame reports the same result entry
 * and leaves its window untouched.  No byte at or beyond stream_bytes is read; nothing outside the n_frames*rw*rh
 * output is written.  n_frames == 0 does nothing.  rw / rh below 1 or above W / H, or a frame too large for the
 * index (more than 32768 chunks), is DBDE_HIP_ERR_ARG.  Asynchronous on the context's stream; timing hook: the index
 * kernel in slot 1, the window kernel in slot 2. */
int dbde_hip_decode_roi(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                        const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                        int x0, int y0, int rw, int rh, const int32_t *d_origins,
                        uint8_t *d_out, dbde_hip_frame_result *d_results);

/* Temporal projection: the per-pixel maximum, minimum, sum and sum of squares over n_frames frames of
 * the rw x rh window at (x0, y0), reduced straight from the compressed bytes (no image is written).
 * Inputs and outputs:
 *   Frame f starts at d_stream + d_frame_offsets[f] (any byte alignment; concatenated and slot layouts alike).  No byte
 *   at or beyond stream_bytes is read.  The window and its argument rules are dbde_hip_decode_roi's (plan_roi); there
 *   are no per-frame origins.  The whole frame is 0, 0, W, H.
 *   Each output is rh x rw, row-major, pitch rw: d_max and d_min U8 at any byte alignment, d_sum and d_sumsq U64,
 *   8-byte aligned.  A NULL output is not computed and its buffer is never touched; at least one of the four must be
 *   non-NULL.  d_count (one U64, required) receives the number of frames that contributed.  d_results (optional) is
 *   filled exactly as dbde_hip_decode_frames fills it: same validation, same entries.
 * What is reduced: only frames dbde_hip_decode_frames accepts; a rejected frame reports its usual result entry and
 *   adds nothing.  The pixels reduced are exactly the bytes dbde_hip_decode_frames would write (minima that wrap modulo
 *   256 included).
 * accumulate = 0: the outputs and *d_count are overwritten with this call's projection, also for n_frames == 0 or when
 *   every frame is rejected (the empty projection: max 0, min 255, sums 0, count 0).  accumulate = 1: this call's
 *   projection is combined into what the buffers hold (max of maxima, min of minima, sums and count added;
 *   n_frames == 0 changes nothing).  Frames [0, n) in one call give the same result as any split into consecutive
 *   calls with accumulate = 1 after the first: every result is an exact integer.
 * Overflow: the U64 sums are exact for any count a user can reach; inside the kernel a workgroup sums at most 65,536
 *   frames in U32 (65,536 * 255^2 < 2^32), a bound the plan enforces.
 * Errors: DBDE_HIP_ERR_ARG as dbde_hip_decode_roi, and for no statistic, a NULL d_count or an unaligned U64 output.
 * Asynchronous on the context's stream; workspace as dbde_hip_decode_roi (the context's, grown on demand), plus the
 * per-segment partials the plan reports.  Timing hook: the index kernel in slot 1, the projection kernels in slot 2. */
int dbde_hip_project(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                     const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                     int x0, int y0, int rw, int rh, int accumulate,
                     uint8_t *d_max, uint8_t *d_min, uint64_t *d_sum, uint64_t *d_sumsq,
                     uint64_t *d_count, dbde_hip_frame_result *d_results);

/* Grouped temporal projection: dbde_hip_project's reduction done once per GROUP of frames -- every run
 * of frames becomes one set of planes (temporal binning, block maxima, per-trial sums).
 * Input, validation and results: the stream, stream_bytes, d_frame_offsets, the window and d_results are exactly
 *   dbde_hip_project's (no per-frame origins, no byte read at or beyond stream_bytes; a rejected frame reports its
 *   usual entry and adds nothing; the pixels reduced are the ones dbde_hip_decode_frames would write).
 * Groups: exactly one of two forms.
 *   uniform  group_frames = g, 1 <= g <= 65,536, d_group_starts == NULL: group k is frames [k*g, min((k+1)*g, n_frames));
 *            n_groups must equal ceil(n_frames / g).  n_frames == 0 (n_groups == 0) does nothing.
 *   ragged   group_frames == 0, d_group_starts a device U32 array of n_groups + 1 entries s[], n_groups >= 1: group k is
 *            frames [b, e), b = min(s[k], n_frames), e = min(max(s[k+1], s[k]), n_frames).  The array is clamped, never
 *            trusted: a decreasing entry gives an empty group, ranges may overlap, frames may belong to no group, and no
 *            value can cause a read outside the n_frames offsets.  Needs n_frames <= 65,536 (the kernel's U32 bound on
 *            the frames of one group).
 * Outputs: each plane is [n_groups][rh][rw], row-major with pitch rw (64-bit indexing).  A NULL plane is neither
 *   computed nor touched; at least one is required.  d_max / d_min hold U8 pixels at any address.  d_sum is U32 (4-byte
 *   aligned), or with sum_type = DBDE_HIP_SUM_U16 a U16 plane (2-byte aligned), allowed only where no group can exceed
 *   257 frames (257 * 255 = 65,535: uniform g <= 257, or the ragged form with n_frames <= 257) and accumulate == 0.
 *   d_sumsq is U64, 8-byte aligned.  d_counts (required, U32 [n_groups], 4-byte aligned) receives the accepted frames
 *   of each group.  An empty group, or one whose frames were all rejected, gets the empty projection: max 0, min 255,
 *   sums 0, count 0.  Nothing outside the requested planes and d_counts is written.
 * accumulate = 1 combines with what the planes and counts hold, by dbde_hip_project's rule applied per group (max of
 *   maxima, min of minima, sums and counts added, modulo the planes' widths).
 * Defining property: group k's planes equal what dbde_hip_project returns for frames [b_k, e_k) alone with
 *   accumulate = 0, and d_counts[k] equals that call's *d_count.  Every value is an exact integer, independent of the
 *   launch shape.
 * Errors: DBDE_HIP_ERR_ARG, before anything is launched, for every broken rule above and for misaligned outputs.
 * Asynchronous on the context's stream; workspace is the context's (the decode index's).  Timing hook: the index kernel
 * in slot 1, the grouped projection kernel in slot 2. */
enum { DBDE_HIP_SUM_U32 = 0, DBDE_HIP_SUM_U16 = 1 };
int dbde_hip_project_groups(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                            int x0, int y0, int rw, int rh,
                            int group_frames, const uint32_t *d_group_starts, int n_groups,
                            int sum_type, int accumulate,
                            uint8_t *d_max, uint8_t *d_min, void *d_sum, uint64_t *d_sumsq,
                            uint32_t *d_counts, dbde_hip_frame_result *d_results);

/* Builds the frame index of a concatenated frame sequence starting at d_stream (no video
 * header): hops 20 + 12 + 2T + 8*n64 from frame to frame (README.md:12-23) until max_frames
 * or the end of stream_bytes.  Writes offsets (device, max_frames) and returns the number of
 * whole frames found in *n_found (host).  Synchronous. */
int dbde_hip_index_stream(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, int W,
                          int H, int max_frames, uint64_t *d_frame_offsets, int *n_found);
/* The same walk, enqueued on the context's stream without waiting for it: the frame count lands in the
 * DEVICE word *d_n_found.  A dbde_hip_decode_frames call enqueued behind it may use d_frame_offsets
 * directly (a reader that knows how many frames it expects, or that bounds the decode by max_frames and
 * inspects the per-frame results: entries past the count are set to 0xFFFFFFFFFFFFFFFF, an offset every
 * extent check rejects -- those frames report header.u64s = 0xFFFFFFFF, consumed = 20, index = elapsed_ns = 0
 * and leave their image untouched; the same holds for any offset outside [0, stream_bytes), however large). */
int dbde_hip_index_stream_async(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, int W,
                                int H, int max_frames, uint64_t *d_frame_offsets, uint32_t *d_n_found);

/* Reading an un-indexed stream a batch at a time without the walk on the critical path: dbde_hip_scan_ahead
 * enqueues the walk of the next (up to) max_frames frames on a SECOND stream owned by the context -- behind
 * everything enqueued on the context's stream so far -- starting at the byte offset in the device word *d_cursor
 * and leaving the offset of the first unvisited byte there (zero it before the first call); frame offsets are
 * relative to d_stream.  dbde_hip_scan_join makes the context's stream wait for the walks enqueued so far.
 * A reader enqueues: scan_ahead(batch 0); then per batch b: scan_join, scan_ahead(batch b+1), decode_frames(batch b)
 * -- the dependent pointer chase of batch b+1 (about a microsecond per frame) then runs beside the decode of b. */
int dbde_hip_scan_ahead(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, int W, int H,
                        int max_frames, uint64_t *d_cursor, uint64_t *d_frame_offsets,
                        uint32_t *d_n_found);
int dbde_hip_scan_join(dbde_hip_ctx *ctx);

/* Counter-based synthetic frames (same bytes as oracle/synth.c): mode 0 noise8, 1 mixed,
 * 2 flat, 3 smooth; modes 4..12 (profiling only, no oracle twin): every tile of depth mode - 4.
 * Used by bench.py and the parity tests to build inputs in HBM. */
int dbde_hip_synth_frames(dbde_hip_ctx *ctx, int mode, uint64_t seed, uint64_t first_frame,
                          int n_frames, int W, int H, uint8_t *d_images);

/* ---- host-pointer entry points: the reference signatures, on the GPU -------------------- */
/* Each copies its operands to the device, runs the same kernels as the batch API, copies
 * the result back and synchronises.  Return values and written bytes are the reference's. */

/* dbde_pack_8x8 (dbde_util.h:21, dbde_util.cpp:22-103): returns (depth<<8)|min, writes
 * exactly 8*depth bytes at target. */
uint32_t dbde_hip_pack_8x8(dbde_hip_ctx *ctx, const uint8_t *image, int stride, uint8_t *target);
/* dbde_pack_8x8_partial (dbde_util.h:22, dbde_util.cpp:105-135). */
uint32_t dbde_hip_pack_8x8_partial(dbde_hip_ctx *ctx, const uint8_t *image, int stride,
                                   int rightmargin, int downmargin, uint8_t *target);
/* dbde_pack_image (dbde_util.h:24, dbde_util.cpp:137-180): returns 12 + 2T + 8*n64. */
size_t dbde_hip_pack_image(dbde_hip_ctx *ctx, const uint8_t *image, int W, int H, uint8_t *target);
/* dbde_pack_frame (dbde_util.h:26, dbde_util.cpp:190-196). */
size_t dbde_hip_pack_frame(dbde_hip_ctx *ctx, uint64_t index, const uint8_t *image, int W, int H,
                           uint8_t *target);
/* dbde_unpack_8x8 (dbde_util.h:30, dbde_util.cpp:216-279); depth > 8 is ignored (no write). */
void dbde_hip_unpack_8x8(dbde_hip_ctx *ctx, uint8_t depth, uint8_t minval, const uint8_t *packed,
                         size_t stride, uint8_t *image);
/* dbde_unpack_8x8_partial (dbde_util.h:31, dbde_util.cpp:281-289). */
void dbde_hip_unpack_8x8_partial(dbde_hip_ctx *ctx, uint8_t depth, uint8_t minval,
                                 const uint8_t *packed, size_t stride, int rightmargin,
                                 int downmargin, uint8_t *image);
/* dbde_unpack_image (dbde_util.h:33, dbde_util.cpp:291-328): bytes consumed, 0 on failure. */
size_t dbde_hip_unpack_image(dbde_hip_ctx *ctx, const uint8_t *packed, int W, int H,
                             uint8_t *image);
/* The window form of dbde_hip_unpack_image (no reference counterpart): one packed frame_data -> the rw x rh window at
 * (x0, y0), row-major at pitch rw.  Returns the bytes consumed, or 0 on failure (window untouched). */
size_t dbde_hip_unpack_image_roi(dbde_hip_ctx *ctx, const uint8_t *packed, int W, int H,
                                 int x0, int y0, int rw, int rh, uint8_t *image);
/* dbde_unpack_frame (dbde_util.h:35, dbde_util.cpp:339-345): *packed is advanced exactly as
 * the reference advances it (by 20 only when the frame data is rejected). */
dbde_hip_frame_header dbde_hip_unpack_frame(dbde_hip_ctx *ctx, uint8_t **packed, int W, int H,
                                            uint8_t *image);

/* ---- header wire format (host only; a few bytes, no kernel) ----------------------------- */
/* dbde_pack_frame_header (dbde_util.cpp:182-188): 20 bytes; elapsed_ns travels as an F64. */
size_t dbde_hip_pack_frame_header(const dbde_hip_frame_header *fh, uint8_t *target);
/* dbde_pack_video_header (dbde_util.cpp:198-209): 28 bytes, height before width. */
size_t dbde_hip_pack_video_header(const dbde_hip_video_header *vh, uint8_t *target);
/* dbde_unpack_frame_header (dbde_util.cpp:330-337): advances *packed by 20. */
dbde_hip_frame_header dbde_hip_unpack_frame_header(uint8_t **packed);
/* dbde_unpack_video_header (dbde_util.cpp:347-359): advances *packed by 28. */
dbde_hip_video_header dbde_hip_unpack_video_header(uint8_t **packed);

/* ---- file I/O: batched .dbde writer and reader -------------------------------------------- */
/* The other end of the path: the reference reads a file frame by frame
 * (dbde_start_file_walk / dbde_walk_a_file / dbde_end_file_walk, dbde_util.cpp:362-426; that
 * API itself is served by libdbde_util_hip.so) and has no writer, its test hand-rolls one
 * (dbde_util_test.cpp:204-211).  These move whole batches: images are DEVICE buffers, the
 * compressed bytes cross PCIe through two pinned windows so that file I/O of one batch
 * overlaps the kernels of the next.  Files are byte-identical to a video header followed by
 * dbde_pack_frame output for every frame. */
typedef struct dbde_hip_writer dbde_hip_writer;
typedef struct dbde_hip_reader dbde_hip_reader;

/* Creates `path` and writes the 28-byte video header {3, H, W, frame_hz}
 * (dbde_pack_video_header).  batch_frames = frames encoded per launch (window size). */
int dbde_hip_writer_open(dbde_hip_ctx *ctx, const char *path, int W, int H, double frame_hz,
                         int batch_frames, dbde_hip_writer **out);
/* Appends n_frames device-resident images (arguments as dbde_hip_encode_frames).  On return
 * d_images may be reused; the bytes reach the file by the next put or by close. */
int dbde_hip_writer_put(dbde_hip_writer *w, const uint8_t *d_images, int n_frames,
                        uint64_t first_index, const uint64_t *d_indices,
                        const uint64_t *d_elapsed_ns);
/* Appends the rw x rh = W x H (the writer's size) window at (x0, y0) of n_frames source images of src_W x src_H
 * pixels (source arguments as dbde_hip_encode_window): the same double-buffered path as dbde_hip_writer_put. */
int dbde_hip_writer_put_window(dbde_hip_writer *w, const uint8_t *d_images, size_t image_bytes, int src_W, int src_H,
                               uint64_t pitch, uint64_t frame_stride, int n_frames, int x0, int y0,
                               const int32_t *d_origins, uint64_t first_index, const uint64_t *d_indices,
                               const uint64_t *d_elapsed_ns);
const char *dbde_hip_writer_error(const dbde_hip_writer *w);
/* Flushes, closes the file and frees the writer; totals are optional outputs. */
int dbde_hip_writer_close(dbde_hip_writer *w, uint64_t *frames_written, uint64_t *bytes_written);

/* Opens `path`, parses and checks the video header with the walker's limits
 * (dbde_util.cpp:371-381: u64s == 3, 0 < H, W, H*W <= 0x37FFFFFF) and starts reading. */
int dbde_hip_reader_open(dbde_hip_ctx *ctx, const char *path, int batch_frames,
                         dbde_hip_video_header *vh, dbde_hip_reader **out);
/* Decodes the next up-to-max_frames frames (capped at batch_frames) into d_images (device,
 * W*H bytes each) and their headers into `headers` (host, optional).  *n_out = frames
 * delivered; 0 = end of file or, as dbde_walk_a_file returns false (dbde_util.cpp:412-420),
 * the first frame that is truncated or does not parse -- the walk ends there. */
int dbde_hip_reader_next(dbde_hip_reader *r, uint8_t *d_images, int max_frames,
                         dbde_hip_frame_header *headers, int *n_out);
void dbde_hip_reader_close(dbde_hip_reader *r);

/* ---- DBDE16: higher-bit-depth frames (extension; PARITY UNPINNED) ------------------------------------------- */
/* The reference's README notes that the minimum array "could expand size to handle higher bit depth images"
 * (README.md:65) and defines nothing further.  DBDE16 is that expansion and nothing else -- U16 pixels (pitch W
 * pixels), depth bytes 0..16, U16 little-endian minima, the second I32 = 2T (it is the BYTE count of the minimum
 * array, README.md:63), payload and tiling rules unchanged; an 8-bit reader rejects such a frame on nm != T.
 * Full specification: oracle/dbde16_oracle.c.  There is no reference behaviour to be bit-exact against: the kernels
 * are checked against that oracle, which agrees with the pinned 8-bit oracle on images that fit 8 bits.
 * Batch API on device buffers only, arguments as dbde_hip_encode_frames / dbde_hip_decode_frames (frame headers
 * carry index first_index + f, elapsed 0); worst case per frame 20 + 12 + 131*T bytes. */
size_t dbde16_hip_max_frame_bytes(int W, int H);
int dbde16_hip_encode_frames(dbde_hip_ctx *ctx, const uint16_t *d_images, int W, int H, int n_frames,
                             uint64_t first_index, uint8_t *d_out, size_t out_capacity,
                             uint64_t slot_stride, uint64_t *d_frame_offsets, uint64_t *d_frame_bytes);
int dbde16_hip_decode_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                             uint16_t *d_images, dbde_hip_frame_result *d_results);
/* Window (region-of-interest) decode of DBDE16 frames: dbde_hip_decode_roi's contract with U16 pixels.
 * Frame f's window goes to d_out + f*rw*rh pixels, row-major, pitch rw pixels; d_out may be any 2-byte aligned address.
 * Validation is dbde16_hip_decode_frames' own (the same index kernel, U16 minima): a rejected frame reports the same
 * result entry and leaves its window untouched.  d_origins (optional) as in dbde_hip_decode_roi, clamped into the
 * frame; NULL -> (x0, y0) for every frame.  No byte at or beyond stream_bytes is read; nothing outside the
 * n_frames*rw*rh output pixels is written.  n_frames == 0 does nothing.  A window size or origin outside the frame, a
 * null pointer, or a frame of more than 32768 index chunks is DBDE_HIP_ERR_ARG before anything is launched.
 * Asynchronous on the context's stream; timing hook: the index kernel in slot 1, the window kernel in slot 2. */
int dbde16_hip_decode_roi(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                          const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                          int x0, int y0, int rw, int rh, const int32_t *d_origins,
                          uint16_t *d_out, dbde_hip_frame_result *d_results);
/* Temporal projection of DBDE16 frames: dbde_hip_project's contract with U16 pixels.
 * Validation is dbde16_hip_decode_frames' own: a rejected frame reports the same d_results entry and adds nothing; the
 * pixels reduced are exactly the U16 values dbde16_hip_decode_frames writes (minima that wrap modulo 2^16 included).
 * d_max / d_min are U16 at any 2-byte aligned address; d_sum, d_sumsq and d_count U64, 8-byte aligned.  The empty
 * projection is max 0, min 65535, sums 0, count 0.  accumulate, n_frames == 0, NULL statistics, stream_bytes and the
 * timing slots are as in dbde_hip_project.
 * Overflow: a workgroup sums at most 65,536 frames per pixel in U32 (65,536 * 65,535 < 2^32) -- the bound the plan
 *   enforces -- and its sums of squares in U64 (one square alone, up to 65,535^2, fills a U32).
 * Errors: DBDE_HIP_ERR_ARG as dbde_hip_project, and for a U16 output that is not 2-byte aligned. */
int dbde16_hip_project(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                       const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                       int x0, int y0, int rw, int rh, int accumulate,
                       uint16_t *d_max, uint16_t *d_min, uint64_t *d_sum, uint64_t *d_sumsq,
                       uint64_t *d_count, dbde_hip_frame_result *d_results);
/* Grouped temporal projection of DBDE16 frames: dbde_hip_project_groups' contract with U16 pixels,
 * validated as dbde16_hip_project validates.  d_max / d_min are U16 planes (2-byte aligned), d_sum is U32 only
 * (65,536 * 65,535 < 2^32; sum_type must be DBDE_HIP_SUM_U32), d_sumsq U64.  The empty projection is max 0, min 65535,
 * sums 0, count 0. */
int dbde16_hip_project_groups(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                              int x0, int y0, int rw, int rh,
                              int group_frames, const uint32_t *d_group_starts, int n_groups,
                              int sum_type, int accumulate,
                              uint16_t *d_max, uint16_t *d_min, uint32_t *d_sum, uint64_t *d_sumsq,
                              uint32_t *d_counts, dbde_hip_frame_result *d_results);

/* Weighted temporal projection: R = n_regressors F32 planes of the rw x rh window,
 *   out[r][y][x] = sum over the accepted frames f of w[r][f] * p_f[y][x],   r = 0 .. R - 1,
 * reduced straight from the compressed bytes (no image is written).  One primitive for Fourier components at a
 * stimulus frequency, per-pixel trends, exponentially weighted backgrounds, GLM regressor maps and correlation maps.
 * Inputs and outputs:
 *   The stream, the window and its argument rules, the validation, d_results, the stream_bytes rule and the timing
 *   slots (index 1, projection kernels 2) are dbde_hip_project's; there are no per-frame origins.
 *   The weight of frame f for regressor r is d_weights[r * weight_stride + f]: a 4-byte aligned device array of F32,
 *   weight_stride >= n_frames (in elements).  Only the entries [r][0 .. n_frames) are read.  Weights are not inspected:
 *   infinities and NaNs propagate by IEEE rules.  1 <= n_regressors <= DBDE_HIP_WPROJ_MAX_REGRESSORS.
 *   d_out is [n_regressors][rh][rw] F32, row-major, 4-byte aligned, indexed in 64 bits.  d_count (one U64, 8-byte
 *   aligned, required) receives the number of frames that contributed, as in dbde_hip_project.
 * The defined value (checked bit for bit).  The frames are cut into S segments of fps frames (both reported by the
 *   plan; the last segment may hold fewer).  Partial P_s is the chain acc = fmaf(w[r][f], (float)p_f, acc) over the
 *   accepted frames f of segment s in ascending f, started at +0.0f: one fused multiply-add each, a single rounding to
 *   nearest even, denormal operands and results kept.  A rejected frame executes no multiply-add: its weight is never
 *   used, so a NaN weight at a rejected frame leaves the output finite.  The result is
 *       ((prior + P_0) + P_1) + ... + P_{S-1}
 *   with F32 round-to-nearest-even additions in ascending s.  prior is what d_out holds when accumulate = 1; when
 *   accumulate = 0 it is absent and the chain starts at P_0.
 *   accumulate = 0 with no accepted frame (n_frames == 0 included) writes +0.0 planes and count 0.  accumulate = 1
 *   with n_frames == 0 changes nothing.  Unlike the integer projections, splitting a run of frames into consecutive
 *   accumulating calls may change the last bits of the result: the additions round.
 * flags: DBDE_HIP_WPROJ_ONE_SEGMENT forces S = 1; the result is then the pure frame-order chain, independent of the
 *   device's compute unit count and of the plan.  Without it S is chosen by dbde_hip_project's rule for the same
 *   window, n_frames and compute units (65,536 frames per segment at most), so the two plans agree.
 * Errors: DBDE_HIP_ERR_ARG for everything dbde_hip_project rejects of its sizes, window and pointers, n_regressors
 *   outside 1..8, NULL d_weights / d_out / d_count, a misaligned d_weights / d_out / d_count, weight_stride < n_frames
 *   and unknown flag bits.
 * Asynchronous on the context's stream; workspace as dbde_hip_project, with the F32 partials the plan reports. */
enum { DBDE_HIP_WPROJ_MAX_REGRESSORS = 8 };
enum { DBDE_HIP_WPROJ_ONE_SEGMENT = 1 };   /* flags */
int dbde_hip_project_weighted(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                              int x0, int y0, int rw, int rh,
                              const float *d_weights, int n_regressors, size_t weight_stride,
                              int accumulate, int flags,
                              float *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results);
/* The same for DBDE16 frames: dbde_hip_project_weighted's contract with U16 pixels, validated as dbde16_hip_project
 * validates.  (float)p_f is exact for every U16 pixel. */
int dbde16_hip_project_weighted(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                                int x0, int y0, int rw, int rh,
                                const float *d_weights, int n_regressors, size_t weight_stride,
                                int accumulate, int flags,
                                float *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results);

/* Count projection: K = n_levels U32 planes of the rw x rh window,
 *   out[k][y][x] = number of accepted frames f with p_f[y0 + y][x0 + x] <= thr_k(y, x),   k = 0 .. K - 1,
 * reduced straight from the compressed bytes (no image is written).  The compare is unsigned in the pixel type.  One
 * primitive for exact per-pixel order statistics over time (a radix refinement on the counts: temporal median,
 * percentile baselines) and for dwell and occupancy maps.
 * Inputs and outputs:
 *   The stream, the window and its argument rules, the validation, d_results, the stream_bytes rule and the timing
 *   slots (index 1, projection kernels 2) are dbde_hip_project's; there are no per-frame origins.
 *   Thresholds always live on the device (U8 elements), so the call stays asynchronous.  Without DBDE_HIP_COUNTS_MAPS
 *   thr_k = d_thresholds[k]: K values, level_stride ignored.  With it thr_k(y, x) = d_thresholds[k * level_stride +
 *   y * rw + x]: K maps in window coordinates, level_stride >= rw * rh (in elements); only elements of window pixels
 *   are read.  The levels are independent: no ordering of the thresholds is required.  1 <= n_levels <=
 *   DBDE_HIP_COUNTS_MAX_LEVELS.
 *   d_out is [n_levels][rh][rw] U32, row-major, 4-byte aligned, indexed in 64 bits.  d_count (one U64, 8-byte aligned,
 *   required) receives the number of frames that contributed, as in dbde_hip_project.
 * The value.  Counts are exact integers modulo 2^32 (a pixel wraps only after 2^32 accepted frames at or below its
 *   threshold).  A rejected frame adds nothing.  accumulate = 1 adds this call's counts to what the planes hold and
 *   the accepted frames to *d_count, so a run of frames may be split into calls, batches or segments in any way with
 *   the same result; accumulate = 1 with n_frames == 0 changes nothing.  accumulate = 0 with no accepted frame
 *   (n_frames == 0 included) writes zero planes and count 0.  The result does not depend on the plan's segments.
 * Errors: DBDE_HIP_ERR_ARG for everything dbde_hip_project rejects of its sizes, window and pointers, n_levels
 *   outside 1..8, NULL d_thresholds / d_out / d_count, a misaligned d_out (4 bytes) or d_count (8 bytes), MAPS with
 *   level_stride < rw * rh, and unknown flag bits.
 * Asynchronous on the context's stream; workspace as dbde_hip_project, with the U32 partials the plan reports. */
enum { DBDE_HIP_COUNTS_MAX_LEVELS = 8 };
enum { DBDE_HIP_COUNTS_MAPS = 1 };   /* flags: thresholds are per-pixel maps; otherwise K scalars */
int dbde_hip_project_counts(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                            int x0, int y0, int rw, int rh,
                            const uint8_t *d_thresholds, int n_levels, size_t level_stride,
                            int accumulate, int flags,
                            uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results);
/* The same for DBDE16 frames: dbde_hip_project_counts' contract with U16 pixels and U16 thresholds (2-byte aligned),
 * validated as dbde16_hip_project validates. */
int dbde16_hip_project_counts(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                              int x0, int y0, int rw, int rh,
                              const uint16_t *d_thresholds, int n_levels, size_t level_stride,
                              int accumulate, int flags,
                              uint32_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results);

/* Neighbour-product projection: one U64 plane of the rw x rh window per requested forward offset,
 *   out[j][y][x] = sum over the accepted frames f of p_f[y0 + y][x0 + x] * p_f[y0 + y + dy][x0 + x + dx]
 *                  where 0 <= x + dx < rw and y + dy < rh (both pixels inside the window),
 * reduced straight from the compressed bytes (no image is written).  With dbde_hip_project's sum, sumsq and count it
 * gives the Pearson correlation of every pixel with its neighbours exactly: the local correlation image.
 * The offsets, one bit each: RIGHT (+1, 0), DOWN (0, +1), DOWN_RIGHT (+1, +1), DOWN_LEFT (-1, +1).  The four cover
 *   every unordered pair of an 8-neighbourhood once; mask 3 is the 4-neighbourhood, mask 15 the 8-neighbourhood.
 *   `pairs` is a mask in 1..15; plane j belongs to its j-th set bit in ascending bit order.
 * Inputs and outputs:
 *   The stream, the window and its argument rules, the validation, d_results, the stream_bytes rule and the timing
 *   slots (index 1, projection kernels 2) are dbde_hip_project's; there are no per-frame origins.
 *   d_out is [popcount(pairs)][rh][rw] U64, row-major, 8-byte aligned, indexed in 64 bits.  d_count (one U64, 8-byte
 *   aligned, required) receives the number of frames that contributed, as in dbde_hip_project.
 * The value.  The sums are exact integers, so a run of frames may be split into calls, batches or segments in any way
 *   with the same bits.  A product is at most 255^2 (DBDE) or 65,535^2 < 2^32 (DBDE16), so an element stays below 2^63
 *   while the accepted frames accumulated into it number fewer than 2^63 / 255^2 > 1.4e14 (DBDE) or 2^31 (DBDE16):
 *   more than one call's n_frames (an int) can hold, and the bound that matters only for accumulate = 1 over many calls.
 *   A rejected frame adds nothing.  Pixels outside the window never contribute, even where the frame has them.  An
 *   element whose partner lies outside the window holds 0 after accumulate = 0 and is left unchanged by accumulate = 1.
 *   accumulate = 1 adds this call's sums to what the planes hold and the accepted frames to *d_count; with
 *   n_frames == 0 it changes nothing.  accumulate = 0 with no accepted frame (n_frames == 0 included) writes zero
 *   planes and count 0.  The result does not depend on the plan's segments.
 * Errors: DBDE_HIP_ERR_ARG for everything dbde_hip_project rejects of its sizes, window and pointers, pairs outside
 *   1..15, NULL d_out / d_count, and a d_out or d_count that is not 8-byte aligned.
 * Asynchronous on the context's stream; workspace as dbde_hip_project, with the partials the plan reports. */
enum { DBDE_HIP_PAIR_RIGHT = 1, DBDE_HIP_PAIR_DOWN = 2, DBDE_HIP_PAIR_DOWN_RIGHT = 4, DBDE_HIP_PAIR_DOWN_LEFT = 8 };
int dbde_hip_project_pairs(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int x0, int y0, int rw, int rh, int pairs, int accumulate,
                           uint64_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results);
/* The same for DBDE16 frames: dbde_hip_project_pairs' contract with U16 pixels, validated as dbde16_hip_project
 * validates. */
int dbde16_hip_project_pairs(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                             int x0, int y0, int rw, int rh, int pairs, int accumulate,
                             uint64_t *d_out, uint64_t *d_count, dbde_hip_frame_result *d_results);

/* Lag projection: per pixel of the rw x rh window, statistics over the pairs of frames `lag` apart,
 * with the order of the frames kept.  A pair is (a, b) = (p_{f - lag}[y0 + y][x0 + x], p_f[y0 + y][x0 + x]); over the
 * counted pairs the planes hold
 *   product = sum a * b        pairsum = sum (a + b)        absdiff = sum |b - a|        sqdiff = sum (b - a)^2
 *   maxdiff = max |b - a| in the pixel type, 0 where no pair was counted,
 * reduced straight from the compressed bytes (no image is written).  sqdiff gives the noise level from successive
 * differences, sqrt(sqdiff / (2 pairs)); absdiff and maxdiff are motion maps; product and pairsum, with
 * dbde_hip_project's sum, sumsq and count, give the autocorrelation at the lag.
 * Which pairs count.  Positions are frame indices within the call.  Pair f is counted iff f >= max(lead, lag) and
 *   frames f and f - lag are both accepted.  A rejected frame is not skipped over: it only voids the up to two pairs it
 *   is a member of.  `lag` is a runtime value in 1..DBDE_HIP_LAG_MAX.  `lead`, 0..n_frames, is the number of leading
 *   frames of the call that serve as history only: they are partners a, never b.
 * Inputs and outputs:
 *   The stream, the window and its argument rules, the validation, d_results, the stream_bytes rule and the timing
 *   slots (index 1, projection kernels 2) are dbde_hip_project's; there are no per-frame origins.
 *   Each plane is [rh][rw], row-major, indexed in 64 bits: the four sums U64 and 8-byte aligned, d_maxdiff U8 (DBDE) or
 *   U16 and 2-byte aligned (DBDE16).  A NULL plane is not computed; at least one of the five must be given.
 *   *d_pairs (one U64, 8-byte aligned, required) receives the number of counted pairs, the same for every pixel;
 *   *d_count (likewise) the number of accepted frames with index >= lead.
 * The value.  All values are exact integers, so the result depends neither on the plan's segments nor on how a run of
 *   frames is split into calls.  The split rule: frames [0, N) in one call (lead 0, accumulate 0) equal, bit for bit,
 *   the calls on [0, B) with lead = 0, then accumulating on [B - lag, 2B) with lead = lag, on [2B - lag, 3B) with
 *   lead = lag and so on (B >= lag), maxdiff and *d_pairs included, and *d_count sums to the accepted frames of
 *   [0, N).  `lead` exists for this rule.
 *   Overflow: a product is at most 255^2 (DBDE) or 65,535^2 < 2^32 (DBDE16), a squared difference likewise, a + b at
 *   most 510 or 131,070, so an element stays below 2^63 while the pairs accumulated into it number fewer than
 *   2^63 / 255^2 > 1.4e14 (DBDE) or 2^31 (DBDE16): more than one call's n_frames (an int) can hold, and the bound
 *   that matters only for accumulate = 1 over many calls.
 *   accumulate = 1 adds to the sums, to *d_pairs and to *d_count and takes the maximum into maxdiff; with no counted
 *   pair it leaves the planes as they are.  accumulate = 0 with no counted pair (n_frames <= lag and lead == n_frames
 *   included) writes zero planes and *d_pairs = 0.
 * Errors: DBDE_HIP_ERR_ARG for everything dbde_hip_project rejects of its sizes, window and pointers, lag outside
 *   1..8, lead outside 0..n_frames, no plane requested, NULL d_pairs / d_count, and misaligned pointers.
 * Asynchronous on the context's stream; workspace as dbde_hip_project, with the partials the plan reports. */
enum { DBDE_HIP_LAG_MAX = 8 };
enum { DBDE_HIP_LAG_PRODUCT = 1, DBDE_HIP_LAG_PAIRSUM = 2, DBDE_HIP_LAG_ABSDIFF = 4, DBDE_HIP_LAG_SQDIFF = 8,
       DBDE_HIP_LAG_MAXDIFF = 16 };   /* the statistics as the plans name them */
int dbde_hip_project_lag(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                         int x0, int y0, int rw, int rh, int lag, int lead, int accumulate,
                         uint64_t *d_product, uint64_t *d_pairsum, uint64_t *d_absdiff, uint64_t *d_sqdiff,
                         uint8_t *d_maxdiff, uint64_t *d_pairs, uint64_t *d_count, dbde_hip_frame_result *d_results);
/* The same for DBDE16 frames: dbde_hip_project_lag's contract with U16 pixels and a U16 maxdiff plane, validated as
 * dbde16_hip_project validates. */
int dbde16_hip_project_lag(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int x0, int y0, int rw, int rh, int lag, int lead, int accumulate,
                           uint64_t *d_product, uint64_t *d_pairsum, uint64_t *d_absdiff, uint64_t *d_sqdiff,
                           uint16_t *d_maxdiff, uint64_t *d_pairs, uint64_t *d_count, dbde_hip_frame_result *d_results);

/* Registered projection: dbde_hip_project's reduction of an rw x rh window whose origin moves from
 * frame to frame, for recordings that drift under the sensor.  Frame f contributes the window at d_origins[f]; the
 * planes are indexed in window coordinates, so a feature that a registration tool or a tracker follows stays on one
 * output pixel.  Straight from the compressed bytes (no image is written).
 * Origins.  d_origins is a device int32 [n_frames][2] of (x, y), required (NULL is DBDE_HIP_ERR_ARG).  Each origin is
 *   clamped into [0, W - rw] x [0, H - rh], exactly as dbde_hip_decode_roi clamps its d_origins.  The array is never
 *   trusted: any int32 value, INT32_MIN and INT32_MAX included, is legal and causes no read outside the frame.  The
 *   origin of a rejected frame is never used.
 * The value.  The outputs equal what dbde_hip_project's reduction gives over the windows dbde_hip_decode_roi writes
 *   for the same stream, rw, rh and d_origins, taken over the accepted frames: bit for bit, every value an exact
 *   integer, wrapped minima included as dbde_hip_project includes them.  With all origins equal to (x0, y0) the
 *   result is dbde_hip_project's at that window.
 * Inputs and outputs:
 *   The stream, the validation, d_results, the planes (d_max / d_min U8 [rh][rw], d_sum / d_sumsq U64 and 8-byte
 *   aligned, a NULL plane neither computed nor touched, at least one given), *d_count (required), the empty
 *   projection, n_frames == 0, the stream_bytes rule (nothing is read at or beyond it) and the timing slots (index 1,
 *   projection kernels 2) are dbde_hip_project's.  1 <= rw <= W, 1 <= rh <= H.
 *   accumulate follows dbde_hip_project's rules; any split of the frames, with their origin rows, into consecutive
 *   accumulating calls gives the one-call result bit for bit.
 *   d_origins_used: optional device int32 [n_frames][2] that receives the clamped origin of every accepted frame; the
 *   row of a rejected frame stays untouched.  It shows that clamping happened instead of silently reducing a
 *   misregistered frame.
 * Errors: DBDE_HIP_ERR_ARG for everything dbde_hip_project rejects of its sizes and pointers, NULL d_origins, and
 *   d_origins / d_origins_used that are not 4-byte aligned.
 * Asynchronous on the context's stream; workspace as dbde_hip_project, with the partials the plan reports.  At most
 * 65,536 frames per segment, as dbde_hip_project. */
int dbde_hip_project_registered(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw, int rh,
                                const int32_t *d_origins, int accumulate, uint8_t *d_max, uint8_t *d_min,
                                uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                                dbde_hip_frame_result *d_results);
/* The same for DBDE16 frames: dbde_hip_project_registered's contract with U16 pixels (d_max / d_min U16 and 2-byte
 * aligned), validated as dbde16_hip_project validates. */
int dbde16_hip_project_registered(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                                  const uint64_t *d_frame_offsets, int W, int H, int n_frames, int rw, int rh,
                                  const int32_t *d_origins, int accumulate, uint16_t *d_max, uint16_t *d_min,
                                  uint64_t *d_sum, uint64_t *d_sumsq, uint64_t *d_count, int32_t *d_origins_used,
                                  dbde_hip_frame_result *d_results);

/* ---- multi-GPU: variable-length gather of the compressed stream to a root (RCCL over xGMI) ------------------- */
/* Frames are independent, so the path shards by contiguous frame blocks (rank g of G owns frames
 * [g*N/G, (g+1)*N/G)): every rank encodes its block with dbde_hip_encode_frames (slot_stride 0) and its output is
 * one in-order segment of the final stream (README.md:12-23: frames simply follow each other).  The only exchange
 * step is this gather (the reference is single-threaded and has no counterpart).  RCCL has no gatherv: byte counts
 * are all-gathered (ncclAllGather, 8 bytes per rank), every rank derives the same displacements, and the bytes
 * travel as grouped ncclSend / ncclRecv into the root's window at their displacement.  One process per GPU; the
 * library opens librccl itself (dlopen; a process that never calls these needs no RCCL).
 * Which RCCL: when the environment variable DBDE_HIP_RCCL_LIBRARY is set and non-empty, the library it names is opened
 * first (a path, or a name the dynamic loader can resolve); otherwise "librccl.so.1", "librccl.so" and
 * "/opt/rocm/lib/librccl.so.1" are tried in turn.  A named library that cannot be opened, or that lacks one of the eleven
 * entry points used (ncclGetUniqueId, ncclCommInitRank, ncclCommDestroy, ncclAllGather, ncclBroadcast, ncclSend, ncclRecv,
 * ncclGroupStart, ncclGroupEnd, ncclGetErrorString, ncclGetVersion), is an ERROR -- there is no fall-back to the default
 * names: dbde_hip_gather_rccl_version returns 0, the create / attach / unique_id calls return DBDE_HIP_ERR_HIP, and
 * dbde_hip_gather_error(NULL) / dbde_hip_scatter_error(NULL) give the reason.  The choice is made once per process, at
 * the first call that needs RCCL.  (The tests use it to run real peer ranks on one GPU through a stand-in transport,
 * tests/fake_rccl/; nothing in the library, the Python package or bench.py sets it.)
 *
 * Per batch, with two slots so that the gather of batch k overlaps the encode of batch k+1:
 *   dbde_hip_gather_join(g, slot)            codec stream waits until the slot's previous transfer has finished
 *   dbde_hip_encode_frames(... d_frame_offsets, d_frame_bytes)        (root 0: straight into its window)
 *   dbde_hip_gather_begin(g, slot, &d_frame_offsets[n-1], &d_frame_bytes[n-1])     returns at once
 *   ... enqueue more work (decode, the next batch's encode) ...
 *   dbde_hip_gather_post(g, slot, d_segment, d_window, window_bytes, sizes, 0)     host waits for the counts only
 * Collective: every rank of the communicator makes the same begin / post calls in the same order. */
typedef struct dbde_hip_gather dbde_hip_gather;
#define DBDE_HIP_GATHER_ID_BYTES 128
/* Rendezvous token (ncclGetUniqueId): one rank creates it, the caller hands it to every other rank by any means. */
int dbde_hip_gather_unique_id(uint8_t id[DBDE_HIP_GATHER_ID_BYTES]);
/* Rank `rank` of `nranks` on the context's device; `root` receives.  Collective (ncclCommInitRank). */
int dbde_hip_gather_create(dbde_hip_ctx *ctx, const uint8_t id[DBDE_HIP_GATHER_ID_BYTES], int nranks, int rank,
                           int root, dbde_hip_gather **out);
/* The same on a communicator the caller already owns (an ncclComm_t, passed as void*); it is not destroyed. */
int dbde_hip_gather_attach(dbde_hip_ctx *ctx, void *nccl_comm, int nranks, int rank, int root,
                           dbde_hip_gather **out);
void dbde_hip_gather_destroy(dbde_hip_gather *g);
/* The handle's last error; with g == NULL, why RCCL could not be opened (or "null gather"). */
const char *dbde_hip_gather_error(const dbde_hip_gather *g);
/* Messages are cut into pieces of at most this many bytes (default 1 GiB), all posted in one group. */
int dbde_hip_gather_set_max_message(dbde_hip_gather *g, uint64_t bytes);
/* Root: the bytes its window holds.  The value travels with every size exchange, so that "the batch does not fit" is a
 * verdict EVERY rank reaches from the same numbers (dbde_hip_gather_post then returns DBDE_HIP_ERR_CAPACITY on all ranks
 * and nothing has been posted anywhere; a root that found out alone used to leave its peers' sends unmatched).  Call it
 * once, before the first dbde_hip_gather_begin.  With nranks > 1 the declaration is REQUIRED: an undeclared window
 * travels as "none" (capacity 0), so every batch that carries a byte is DBDE_HIP_ERR_CAPACITY on every rank.  (nranks
 * == 1 has no peer to strand: an undeclared window there means "no limit declared" and only window_bytes is checked.)
 * The caller's contract that remains: the window_bytes the root later passes to dbde_hip_gather_post must be at least
 * what it declared here.  A root that breaks it gets DBDE_HIP_ERR_ARG ALONE, after its peers have posted their sends --
 * only the root knows window_bytes, so this cannot be a shared verdict without passing it through the exchange. */
int dbde_hip_gather_set_window(dbde_hip_gather *g, uint64_t window_bytes);
/* The verdict itself, pure arithmetic: pairs[2 r] = rank r's count, pairs[2 r + 1] = the window capacity rank r declared
 * (only the root's counts).  DBDE_HIP_OK or DBDE_HIP_ERR_CAPACITY; *total_out = sum of the counts. */
int dbde_hip_gather_check(int nranks, int root, const uint64_t *pairs, uint64_t *total_out);
/* Enqueues the size exchange of `slot` (0 or 1) behind everything on the context's stream: this rank's byte count
 * is the sum of the two DEVICE words (either may be NULL = 0; the encoder's offset and length of the batch's last
 * frame).  Does not wait for anything. */
int dbde_hip_gather_begin(dbde_hip_gather *g, int slot, const uint64_t *d_last_offset,
                          const uint64_t *d_last_bytes);
/* Blocks the HOST (not the codec's stream) until the slot's counts have arrived, then posts the transfers on the
 * gather's own stream: a non-root rank sends d_segment[0, its count) to the root; the root receives rank r's bytes
 * at d_window + sum(counts of ranks < r).  The root's own bytes are not moved when d_segment already is
 * d_window + its displacement (root 0 encoding straight into its window), else copied once device-to-device.
 * window_bytes (root) must hold the sum of all counts -- size it as nranks x the per-rank capacity and declare it
 * with dbde_hip_gather_set_window: DBDE_HIP_ERR_CAPACITY is then returned by EVERY rank, with nothing posted.  (A root
 * whose window_bytes is below what it declared gets DBDE_HIP_ERR_ARG: a caller's error, not the data's.)  sizes_out: optional host
 * array of nranks counts.  flags: DBDE_HIP_GATHER_LOOPBACK (tests and one-GPU rehearsals) sends the root's own
 * segment to itself through ncclSend / ncclRecv instead. */
#define DBDE_HIP_GATHER_LOOPBACK 1u
int dbde_hip_gather_post(dbde_hip_gather *g, int slot, const uint8_t *d_segment, uint8_t *d_window,
                         size_t window_bytes, uint64_t *sizes_out, uint32_t flags);
/* Makes the context's stream wait for the slot's posted transfers (before its segment / window is overwritten). */
int dbde_hip_gather_join(dbde_hip_gather *g, int slot);
/* Blocks the host until they have finished (before the root reads the window from the host side). */
int dbde_hip_gather_sync(dbde_hip_gather *g, int slot);
/* NCCL_VERSION_CODE of the RCCL in use; 0 when librccl cannot be opened. */
int dbde_hip_gather_rccl_version(void);
/* The transfer plan, exposed because it is the host logic both ends must agree on (pure arithmetic, no GPU):
 * for `rank`, the ordered list of operations given every rank's count.  Returns the number of operations
 * (filling at most max_ops of them) or a negative error; *total_out = sum of counts. */
enum { DBDE_HIP_GATHER_SEND = 1, DBDE_HIP_GATHER_RECV = 2, DBDE_HIP_GATHER_OWN = 3 };
typedef struct {
    int32_t peer;              /* rank at the other end (OWN: the root itself) */
    int32_t kind;              /* DBDE_HIP_GATHER_SEND / _RECV / _OWN */
    uint64_t segment_offset;   /* SEND: byte offset in this rank's segment */
    uint64_t window_offset;    /* byte offset in the root's window (displacement + piece offset) */
    uint64_t bytes;
} dbde_hip_gather_op;
int dbde_hip_gather_plan(int nranks, int rank, int root, const uint64_t *sizes, uint64_t max_piece,
                         dbde_hip_gather_op *ops, int max_ops, uint64_t *total_out);

/* ---- multi-GPU: scatter of a .dbde body to the ranks' frame blocks (the decode-side mirror of the gather) ------ */
/* A root holds a stream of frames following each other (README.md:12-23) and the frame starts the device scanner found
 * (dbde_hip_index_stream_async; the serial reader this replaces is dbde_util.cpp:408-421).  Rank r of G gets the bytes of
 * frames [r n / G, (r + 1) n / G) -- the gather's blocks -- and the offsets of those frames relative to its segment, and
 * decodes them with dbde_hip_decode_frames.  The block table is worked out on the device from the scanner's outputs and
 * broadcast (ncclBroadcast), every rank's buffer capacities are all-gathered beside it, the bytes and the offsets travel
 * as grouped ncclSend / ncclRecv; the root's own block is not moved.  Two slots, as for the gather.  Per batch:
 *   root:   dbde_hip_index_stream_async(ctx, d_stream, bytes, W, H, max, d_offsets, d_count)
 *   all:    dbde_hip_scatter_begin(s, slot, d_stream, bytes, d_offsets, d_count)      (non-root ranks pass NULL / 0)
 *   all:    dbde_hip_scatter_post(s, slot, d_segment, d_my_offsets, &mine, NULL, 0)   host waits for the table only
 *   all:    dbde_hip_scatter_join(s, slot)
 *   all:    dbde_hip_decode_frames(ctx, root ? d_stream + mine.byte_start : d_segment, mine.byte_count, d_my_offsets, W, H,
 *                                  (int)mine.n_frames, d_images, d_results)
 * Collective: every rank makes the same begin / post calls in the same order.  UNMEASURED on hardware beyond one rank:
 * worlds of 2-4 real processes have run every branch on one GPU through a stand-in transport (tests/fake_rccl/), which
 * checks bytes and verdicts and says nothing about time; RCCL itself has not carried rank-to-rank traffic. */
typedef struct dbde_hip_scatter dbde_hip_scatter;
typedef struct {
    uint64_t first_frame, n_frames;   /* the rank's frame block: global frame numbers [first_frame, first_frame + n_frames) */
    uint64_t byte_start, byte_count;  /* its bytes in the root's stream */
} dbde_hip_scatter_block;
int dbde_hip_scatter_create(dbde_hip_ctx *ctx, const uint8_t id[DBDE_HIP_GATHER_ID_BYTES], int nranks, int rank,
                            int root, dbde_hip_scatter **out);      /* collective (ncclCommInitRank); id: dbde_hip_gather_unique_id */
int dbde_hip_scatter_attach(dbde_hip_ctx *ctx, void *nccl_comm, int nranks, int rank, int root, dbde_hip_scatter **out);
void dbde_hip_scatter_destroy(dbde_hip_scatter *s);
const char *dbde_hip_scatter_error(const dbde_hip_scatter *s);   /* s == NULL: as dbde_hip_gather_error(NULL) */
int dbde_hip_scatter_set_max_message(dbde_hip_scatter *s, uint64_t bytes);
/* What this rank's receive buffers hold: segment bytes and frame offsets.  Travels with every table exchange, so that "a
 * block does not fit" is DBDE_HIP_ERR_CAPACITY on EVERY rank with nothing posted.  d_offsets_out (dbde_hip_scatter_post)
 * must hold max_frames entries on EVERY rank, the root included: the root's block is decoded in place, so its
 * segment_bytes is not looked at (unless DBDE_HIP_SCATTER_LOOPBACK), but the rebased offsets of its block ARE written to
 * its d_offsets_out, and their number comes from the scanner's reading of an untrusted stream.  A rank that never calls
 * this has declared room for nothing. */
int dbde_hip_scatter_set_capacity(dbde_hip_scatter *s, uint64_t segment_bytes, uint64_t max_frames);
/* Enqueues the table exchange of `slot` behind everything on the context's stream (the scanner).  Root: the stream, its
 * readable extent, the scanner's offsets and its count word (all device).  Other ranks: NULL, 0, NULL, NULL. */
int dbde_hip_scatter_begin(dbde_hip_scatter *s, int slot, const uint8_t *d_stream, uint64_t stream_bytes,
                           const uint64_t *d_frame_offsets, const uint32_t *d_n_frames);
/* Blocks the HOST until the table has arrived, then posts the transfers on the scatter's own stream.  d_segment: where a
 * non-root rank's bytes land (root: unused unless DBDE_HIP_SCATTER_LOOPBACK, which sends the root's own block to itself
 * through ncclSend / ncclRecv -- tests and one-GPU rehearsals); d_offsets_out: the block's frame offsets relative to its
 * first byte (every rank).  mine_out / table_out (nranks entries): optional host copies of the table. */
#define DBDE_HIP_SCATTER_LOOPBACK 1u
int dbde_hip_scatter_post(dbde_hip_scatter *s, int slot, uint8_t *d_segment, uint64_t *d_offsets_out,
                          dbde_hip_scatter_block *mine_out, dbde_hip_scatter_block *table_out, uint32_t flags);
int dbde_hip_scatter_join(dbde_hip_scatter *s, int slot);   /* the context's stream waits for the slot's transfers */
int dbde_hip_scatter_sync(dbde_hip_scatter *s, int slot);   /* the host does */
/* The host logic both ends must agree on, pure arithmetic (no GPU): the block table from a host-side frame index, the
 * capacity verdict (caps[2 r] = rank r's segment bytes, caps[2 r + 1] = its frame capacity), and the ordered transfers
 * of `rank` (returns their number, filling at most max_ops). */
enum { DBDE_HIP_SCATTER_SEND_BYTES = 1, DBDE_HIP_SCATTER_RECV_BYTES = 2, DBDE_HIP_SCATTER_SEND_OFFSETS = 3,
       DBDE_HIP_SCATTER_RECV_OFFSETS = 4, DBDE_HIP_SCATTER_OWN = 5 };
typedef struct {
    int32_t peer, kind;
    uint64_t source_offset;    /* bytes: offset in the root's stream; offsets: byte offset in the root's offset array */
    uint64_t dest_offset;      /* byte offset in the receiver's segment / offsets buffer */
    uint64_t bytes;
} dbde_hip_scatter_op;
int dbde_hip_scatter_blocks(int nranks, uint64_t n_frames, const uint64_t *frame_offsets, uint64_t stream_bytes,
                            dbde_hip_scatter_block *table);
int dbde_hip_scatter_check(int nranks, const dbde_hip_scatter_block *table, const uint64_t *caps);
int dbde_hip_scatter_plan(int nranks, int rank, int root, const dbde_hip_scatter_block *table, uint64_t max_piece,
                          dbde_hip_scatter_op *ops, int max_ops);

/* ---- launch plans: which kernels a batch call runs (pure host arithmetic: no context, no device) ------------
 * The batch calls choose among several kernel forms by shape, batch size and buffer alignment;
 * these two functions ARE that choice (dbde_hip_encode_frames / _decode_frames call the same code), exposed so that
 * an integrator can see -- and a CPU-only test can pin -- what a given geometry runs.  No reference counterpart. */
typedef struct dbde_hip_launch_plan {
    int32_t kernel;            /* 0 = chunk kernels (encode: persistent encoder), 1 = encode: one workgroup per chunk
                                  (small launches), 2 = whole frames per wave (encode, T <= 64 tiles), 3 = whole frames per workgroup
                                  (decode: 1 .. 256 tiles, and up to 768 where chunks would store tile by tile; persistent), 4 = encode: whole
                                  frames per workgroup, staged through LDS,
                                  5 = encode: 4 .. 64 (and 77 .. 85) tiles in 16-byte aligned slots, rows of 4-byte multiples: persistent
                                  workgroups, pixels double-buffered */
    int32_t input_mode;        /* encode: 0 = 16-byte aligned rows, 1 = any geometry (W >= 16), 2 = byte by byte (W < 16), 3 = any geometry with dword-aligned fetches (63 tile pairs per wave), 4 = the same with one wave per segment of a tile row */
    int32_t image_mode;        /* decode, kernel 0: 0 = one aligned 16-byte store per lane and image row, 1 = chunks of whole
                                  tile rows staged in LDS (16-byte rows: per chunk, only all-depth-8 chunks stage),
                                  2 = tile by tile */
    int32_t index_mode;        /* decode, kernel 0: 0 = index kernel + table, 1 = self-indexing workgroups, 2 = fused index + decode */
    int32_t threads;           /* workgroup size */
    int32_t aligned_out;       /* encode: 1 = 8-byte aligned frames and fields (wide stores) */
    uint32_t chunks_per_frame; /* kernels 0 / 1 */
    uint32_t chunk_tiles;      /* kernels 0 / 1: tile slots of a chunk (decode: whole tile rows, or 512) */
    uint64_t n_chunks;         /* kernels 0 / 1: chunks (= workgroups of the decoder) in the launch */
} dbde_hip_launch_plan;
/* resident_workgroups: what the device holds of the persistent encoder (2 per CU + 1 on MI355X: 513). */
int dbde_hip_encode_plan(int width, int height, int n_frames, uint64_t image_address, uint64_t out_address,
                         uint64_t slot_stride, int resident_workgroups, dbde_hip_launch_plan *plan);
int dbde_hip_decode_plan(int width, int height, int n_frames, uint64_t image_address, int n_cu,
                         dbde_hip_launch_plan *plan);

/* What a window decode with these arguments runs (pure host arithmetic, like dbde_hip_decode_plan): validates the
 * arguments as dbde_hip_decode_roi does (DBDE_HIP_ERR_ARG otherwise) and reports the tile window, the index geometry
 * and the window kernel's launch. */
typedef struct dbde_hip_roi_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window at (x0, y0) */
    int32_t tiles_x, tiles_y;         /* tiles across / down that window covers */
    int32_t max_tiles_x, max_tiles_y; /* the most any origin in [0, W-rw] x [0, H-rh] needs (per-frame origins) */
    uint32_t chunks_per_frame;        /* index: chunks per frame (each starts a tile row or a 512-tile piece of one) */
    uint32_t chunk_tiles;             /* index: tiles per chunk (the frame's width in tiles, or 512) */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks (frames too tall otherwise) */
    uint32_t index_split;             /* index: workgroups per frame (1 = one per frame) */
    uint32_t threads;                 /* window kernel: workgroup size = tiles per workgroup (64 or 256) */
    uint32_t pieces_x;                /* window kernel: workgroups per window tile row (per-frame origins: the most) */
    uint64_t grid;                    /* window kernel: workgroups with the origin (x0, y0) */
    uint64_t grid_origins;            /* ... with per-frame origins (the most any origin needs) */
} dbde_hip_roi_plan_t;
int dbde_hip_roi_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_roi_plan_t *plan);
/* The same for dbde16_hip_decode_roi: its arguments, its index geometry and the 16-bit window kernel's launch (windows
 * more than 64 tiles across take 128 tiles per workgroup there, not 256: a U16 tile needs twice the LDS). */
int dbde16_hip_roi_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_roi_plan_t *plan);

/* What dbde_hip_project runs (pure host arithmetic, like dbde_hip_roi_plan): validates exactly what dbde_hip_project
 * validates (DBDE_HIP_ERR_ARG otherwise) and reports the tile window, the index geometry, the projection launch and its
 * workspace.  stats: bitmask of the statistics, max 1, min 2, sum 4, sumsq 8 (dbde_hip_project: its non-NULL outputs).
 * n_cu: compute units of the device (dbde_hip_project uses its context's). */
enum { DBDE_HIP_PROJECT_MAX = 1, DBDE_HIP_PROJECT_MIN = 2, DBDE_HIP_PROJECT_SUM = 4, DBDE_HIP_PROJECT_SUMSQ = 8 };
typedef struct dbde_hip_project_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* projection kernel: workgroup size (8 lanes per tile: threads / 8 tiles) */
    uint32_t pieces_x;                /* projection kernel: workgroups across a window tile row */
    uint32_t segments;                /* frame segments, each reduced by its own workgroups */
    uint32_t frames_per_segment;      /* frames of every segment but the last (which may hold fewer) */
    uint32_t max_frames_per_segment;  /* the kernel's U32 bound on frames_per_segment */
    uint32_t reserved_;
    uint64_t grid;                    /* projection kernel: pieces_x * tiles_y * segments workgroups */
    uint64_t combine_grid;            /* combine kernel: workgroups (0 = one segment, no combine) */
    uint64_t workspace_bytes;         /* per-segment partials (0 for one segment) */
} dbde_hip_project_plan_t;
int dbde_hip_project_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats,
                          int n_cu, dbde_hip_project_plan_t *plan);
/* The same for dbde16_hip_project: the same window, index geometry and segment rule; the 16-bit kernel takes 16 lanes
 * per tile (threads / 16 tiles per workgroup, pieces_x accordingly), max_frames_per_segment is its U32 bound on the
 * sums (65,536 * 65,535 < 2^32), and workspace_bytes counts U16 max / min, U32 sum and U64 sumsq partials. */
int dbde16_hip_project_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, unsigned stats,
                            int n_cu, dbde_hip_project_plan_t *plan);

/* What dbde_hip_project_groups runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what the call
 * validates of its sizes, groups, sum_type, accumulate and output addresses (DBDE_HIP_ERR_ARG otherwise) and reports
 * the tile window, the index geometry, the launch and the bytes of each plane.  has_group_starts: 1 for the ragged form
 * (the call's d_group_starts != NULL).  The *_address arguments stand for the call's output pointers: 0 = NULL (the
 * statistic is not computed), otherwise only the alignment counts.  n_cu: compute units of the device.
 * The run rule: a workgroup takes one window tile row, one piece and a run of groups_per_run consecutive groups; runs
 * are cut only to bring the launch to about 4 workgroups per CU and never to fewer than 32 frames (the ragged form
 * counts n_frames / n_groups frames per group), so a large window has one run. */
typedef struct dbde_hip_project_groups_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* kernel: workgroup size (8 lanes per tile, DBDE16: 16) */
    uint32_t pieces_x;                /* kernel: workgroups across a window tile row */
    uint32_t runs;                    /* runs of consecutive groups, each walked by its own workgroups */
    uint32_t groups_per_run;          /* groups of every run but the last (which may hold fewer) */
    uint32_t max_group_frames;        /* the kernel's U32 bound on the frames of one group */
    uint32_t stats;                   /* the statistics computed: max 1, min 2, sum 4, sumsq 8 */
    uint64_t grid;                    /* kernel: pieces_x * tiles_y * runs workgroups */
    uint64_t sum_bytes, max_bytes, min_bytes, sumsq_bytes;   /* bytes of each plane set (0 = not computed) */
    uint64_t counts_bytes;            /* 4 * n_groups */
    uint64_t workspace_bytes;         /* beyond the decode index's: none (the planes are written directly) */
} dbde_hip_project_groups_plan_t;
int dbde_hip_project_groups_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                                 int group_frames, int has_group_starts, int n_groups, int sum_type, int accumulate,
                                 uint64_t max_address, uint64_t min_address, uint64_t sum_address,
                                 uint64_t sumsq_address, uint64_t counts_address, int n_cu,
                                 dbde_hip_project_groups_plan_t *plan);
int dbde16_hip_project_groups_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                                   int group_frames, int has_group_starts, int n_groups, int sum_type, int accumulate,
                                   uint64_t max_address, uint64_t min_address, uint64_t sum_address,
                                   uint64_t sumsq_address, uint64_t counts_address, int n_cu,
                                   dbde_hip_project_groups_plan_t *plan);

/* What dbde_hip_project_weighted runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what the
 * call validates of its sizes, window, n_regressors, weight_stride, flags and addresses (DBDE_HIP_ERR_ARG otherwise)
 * and reports the tile window, the index geometry, the launch and its workspace.  The fields are
 * dbde_hip_project_plan_t's, with regressors in place of a statistics set; segments and frames_per_segment are S and
 * fps of the defined value.  weights_address, out_address and count_address stand for the call's pointers (0 = NULL,
 * rejected); n_cu: compute units of the device (the call uses its context's). */
typedef struct dbde_hip_project_weighted_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* projection kernel: workgroup size */
    uint32_t pieces_x;                /* projection kernel: workgroups across a window tile row */
    uint32_t segments;                /* S: frame segments, each folded by its own workgroups (1 with ONE_SEGMENT) */
    uint32_t frames_per_segment;      /* fps: frames of every segment but the last (which may hold fewer) */
    uint32_t max_frames_per_segment;  /* dbde_hip_project's bound, kept so that the two plans agree */
    uint32_t regressors;              /* R */
    uint64_t grid;                    /* projection kernel: pieces_x * tiles_y * segments workgroups */
    uint64_t combine_grid;            /* combine kernel: workgroups (0 = one segment, no combine) */
    uint64_t workspace_bytes;         /* F32 partials: 4 * S * R * rw * rh rounded up to 16 (0 for one segment) */
    uint32_t lds_bytes;               /* projection kernel: LDS per workgroup */
    uint32_t reserved_;
} dbde_hip_project_weighted_plan_t;
int dbde_hip_project_weighted_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                                   int n_regressors, uint64_t weight_stride, int flags,
                                   uint64_t weights_address, uint64_t out_address, uint64_t count_address,
                                   int n_cu, dbde_hip_project_weighted_plan_t *plan);
int dbde16_hip_project_weighted_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                                     int n_regressors, uint64_t weight_stride, int flags,
                                     uint64_t weights_address, uint64_t out_address, uint64_t count_address,
                                     int n_cu, dbde_hip_project_weighted_plan_t *plan);

/* What dbde_hip_project_counts runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what the
 * call validates of its sizes, window, n_levels, level_stride, flags and addresses (DBDE_HIP_ERR_ARG otherwise) and
 * reports the tile window, the index geometry, the launch and its workspace.  The fields are
 * dbde_hip_project_weighted_plan_t's, with levels in place of regressors; segments and frames_per_segment follow
 * dbde_hip_project_plan's rule for the same window, n_frames and compute units (the counts do not depend on them).
 * All 8 level counts have a kernel instance of their own for both pixel sizes, so levels is also the instance used.
 * thresholds_address, out_address and count_address stand for the call's pointers (0 = NULL, rejected); n_cu: compute
 * units of the device (the call uses its context's). */
typedef struct dbde_hip_project_counts_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* projection kernel: workgroup size */
    uint32_t pieces_x;                /* projection kernel: workgroups across a window tile row */
    uint32_t segments;                /* S: frame segments, each counted by its own workgroups */
    uint32_t frames_per_segment;      /* fps: frames of every segment but the last (which may hold fewer) */
    uint32_t max_frames_per_segment;  /* dbde_hip_project's bound, kept so that the two plans agree */
    uint32_t levels;                  /* K */
    uint64_t grid;                    /* projection kernel: pieces_x * tiles_y * segments workgroups */
    uint64_t combine_grid;            /* combine kernel: workgroups (0 = one segment, no combine) */
    uint64_t workspace_bytes;         /* U32 partials: 4 * S * K * rw * rh rounded up to 16 (0 for one segment) */
    uint32_t lds_bytes;               /* projection kernel: LDS per workgroup */
    uint32_t reserved_;
} dbde_hip_project_counts_plan_t;
int dbde_hip_project_counts_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                                 int n_levels, uint64_t level_stride, int flags,
                                 uint64_t thresholds_address, uint64_t out_address, uint64_t count_address,
                                 int n_cu, dbde_hip_project_counts_plan_t *plan);
int dbde16_hip_project_counts_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh,
                                   int n_levels, uint64_t level_stride, int flags,
                                   uint64_t thresholds_address, uint64_t out_address, uint64_t count_address,
                                   int n_cu, dbde_hip_project_counts_plan_t *plan);

/* What dbde_hip_project_pairs runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what the call
 * validates of its sizes, window, pairs and addresses (DBDE_HIP_ERR_ARG otherwise) and reports the tile window, the
 * index geometry, the launch and its workspace.  out_address and count_address stand for the call's pointers (0 =
 * NULL, rejected); n_cu: compute units of the device (the call uses its context's).  The formulas:
 *   instance     1 for pairs == 1, 3 for pairs 2 and 3, 15 for every mask with a diagonal: the kernel instance that
 *                runs.  It accumulates all of its offsets and stores the requested planes.
 *   piece_tiles  P = threads / 8 (DBDE: 32) or threads / 16 (DBDE16: 16): tiles one workgroup decodes.
 *   halo_left    1 where the instance has DOWN_LEFT, halo_right 1 where it has RIGHT or DOWN_RIGHT, else 0: tiles at
 *                either end of a piece that are decoded as partners only.  The window's first piece owns its first
 *                tile and its last piece its last: their partners beyond lie outside the window.
 *   piece_stride s = P - halo_left - halo_right: tiles from one piece's first tile to the next one's.
 *   pieces_x     1 while tiles_x <= P, else 1 + ceil((tiles_x - P) / s): more than one from 264 pixels (DBDE) or 136
 *                pixels (DBDE16) of an aligned window.
 *   rows_below   tiles_y - 1 for instances 3 and 15 (every window tile row but the last also decodes row 0 of the tile
 *                row under it, through a second offset prefix), 0 for instance 1.
 *   segments, frames_per_segment: dbde_hip_project_plan's rule applied to pieces_x * tiles_y workgroups.
 *   grid         pieces_x * tiles_y * segments; combine_grid = ceil(rw * rh / 256) with more than one segment, else 0.
 *   workspace_bytes  (4 DBDE, 8 DBDE16) * segments * planes * rw * rh rounded up to 16; 0 for one segment.
 *   lds_bytes    2 * 4 * R * 288 + 2 * 4 * (R - 7) * 32 + 16 with R = 8 band rows for instance 1 and 9 otherwise: the
 *                double-buffered band of a group of 4 frames, the wave totals of the prefixes, the count's. */
typedef struct dbde_hip_project_pairs_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* projection kernel: workgroup size */
    uint32_t pieces_x;                /* projection kernel: workgroups across a window tile row */
    uint32_t segments;                /* S: frame segments, each summed by its own workgroups */
    uint32_t frames_per_segment;      /* fps: frames of every segment but the last (which may hold fewer) */
    uint32_t max_frames_per_segment;  /* 65,536: keeps the DBDE kernel's U32 partials exact (65,536 * 255^2 < 2^32) */
    uint32_t planes;                  /* popcount(pairs) */
    uint64_t grid;                    /* projection kernel: pieces_x * tiles_y * segments workgroups */
    uint64_t combine_grid;            /* combine kernel: workgroups (0 = one segment, no combine) */
    uint64_t workspace_bytes;         /* per-segment partials (0 for one segment) */
    uint32_t lds_bytes;               /* projection kernel: LDS per workgroup */
    uint32_t instance;                /* mask of the kernel instance that runs: 1, 3 or 15 */
    uint32_t piece_tiles;             /* tiles a workgroup decodes */
    uint32_t piece_stride;            /* tiles between the first tiles of neighbouring pieces */
    uint32_t halo_left, halo_right;   /* partner-only tiles at the ends of an inner piece */
    uint32_t rows_below;              /* window tile rows that also decode row 0 of the tile row under them */
    uint32_t reserved_;
} dbde_hip_project_pairs_plan_t;
int dbde_hip_project_pairs_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs,
                                uint64_t out_address, uint64_t count_address, int n_cu,
                                dbde_hip_project_pairs_plan_t *plan);
int dbde16_hip_project_pairs_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int pairs,
                                  uint64_t out_address, uint64_t count_address, int n_cu,
                                  dbde_hip_project_pairs_plan_t *plan);

/* What dbde_hip_project_lag runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what the call
 * validates of its sizes, window, lag, lead, statistics and addresses (DBDE_HIP_ERR_ARG otherwise) and reports the tile
 * window, the index geometry, the launch and its workspace.  `stats` is the mask of DBDE_HIP_LAG_* bits standing for
 * the non-NULL planes.  sums_address (the OR of the addresses of the requested U64 planes: only its alignment is
 * looked at), maxdiff_address, pairs_address and count_address stand for the call's pointers (pairs / count 0 = NULL,
 * rejected); n_cu: compute units of the device (the call uses its context's).  The formulas:
 *   instance     3 where stats has only product / pairsum, 28 where it has only absdiff / sqdiff / maxdiff, else 31:
 *                the kernel instance that runs.  It accumulates all of its statistics and stores the requested planes.
 *   pieces_x, segments, frames_per_segment: dbde_hip_project_plan's for the same window, n_frames and n_cu.
 *   first_frame  max(lead - lag, 0): the first frame any workgroup decodes (the index still validates every frame).
 *   history_frames  frames decoded a second time as history only: lag per segment that counts a pair, less the first
 *                of them (a segment counts one iff it reaches past max(lead, lag)); 0 where no pair is counted.
 *   grid         pieces_x * tiles_y * segments; combine_grid = ceil(rw * rh / 256) with more than one segment, else 0.
 *   workspace_bytes  per requested statistic segments * rw * rh elements rounded up to 16 bytes: product, pairsum and
 *                sqdiff 4 bytes (DBDE) or 8 (DBDE16), absdiff 4, maxdiff 1 or 2; 0 for one segment.
 *   lds_bytes    8 * 256 * 8 (the history ring) + 2 * 4 * 2 * 16 (the wave totals of a group) + 32 (the scalars'). */
typedef struct dbde_hip_project_lag_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* projection kernel: workgroup size */
    uint32_t pieces_x;                /* projection kernel: workgroups across a window tile row */
    uint32_t segments;                /* S: frame segments, each summed by its own workgroups */
    uint32_t frames_per_segment;      /* fps: frames of every segment but the last (which may hold fewer) */
    uint32_t max_frames_per_segment;  /* 65,536: keeps the kernel's per-lane sums exact */
    uint32_t planes;                  /* popcount(stats) */
    uint64_t grid;                    /* projection kernel: pieces_x * tiles_y * segments workgroups */
    uint64_t combine_grid;            /* combine kernel: workgroups (0 = one segment, no combine) */
    uint64_t workspace_bytes;         /* per-segment partials (0 for one segment) */
    uint32_t lds_bytes;               /* projection kernel: LDS per workgroup */
    uint32_t instance;                /* statistics of the kernel instance that runs: 3, 28 or 31 */
    uint32_t first_frame;             /* first frame decoded: max(lead - lag, 0) */
    uint32_t history_frames;          /* frames decoded twice (history of the segments after the first) */
    uint32_t first_pair;              /* max(lead, lag): the first frame that can be the later member of a pair */
    uint32_t reserved_;
} dbde_hip_project_lag_plan_t;
int dbde_hip_project_lag_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead,
                              unsigned stats, uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                              uint64_t count_address, int n_cu, dbde_hip_project_lag_plan_t *plan);
int dbde16_hip_project_lag_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int lag, int lead,
                                unsigned stats, uint64_t sums_address, uint64_t maxdiff_address, uint64_t pairs_address,
                                uint64_t count_address, int n_cu, dbde_hip_project_lag_plan_t *plan);

/* What dbde_hip_project_registered runs (pure host arithmetic, like dbde_hip_project_plan): validates what the call
 * validates of its sizes and statistics (DBDE_HIP_ERR_ARG otherwise; `stats` is the mask of the non-NULL planes, max 1,
 * min 2, sum 4, sumsq 8) and reports the index geometry, the launch and its workspace.  n_cu: compute units of the
 * device (the call uses its context's).  The formulas:
 *   piece_cols   output columns one workgroup owns: 8 * (256 / 8 - 1) = 248 (DBDE), 8 * (256 / 16 - 1) = 120 (DBDE16).
 *   pieces_x     ceil(rw / piece_cols); band_rows = 8; bands = ceil(rh / 8).
 *   segments, frames_per_segment: dbde_hip_project_plan's rule applied to pieces_x * bands workgroups.
 *   instance     3 where stats has only max / min, 12 where it has only sum / sumsq, else 15: the kernel instance that
 *                runs.  It accumulates all of its statistics and stores the requested planes.
 *   grid         pieces_x * bands * segments; combine_grid = ceil(rw * rh / 256) with more than one segment, else 0.
 *   workspace_bytes  dbde_hip_project_plan's for the requested statistics; 0 for one segment.
 *   lds_bytes    2 * 4 * 8 * 68 * 4 (the band: two groups of four frames, 8 rows of 68 dwords) + 2 * 4 * 2 * 32 (the wave
 *                totals of a group, two tile rows) + 16 (the count's). */
typedef struct dbde_hip_project_registered_plan_t {
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* projection kernel: workgroup size */
    uint32_t piece_cols;              /* output columns per workgroup */
    uint32_t pieces_x;                /* workgroups across the window */
    uint32_t band_rows;               /* output rows per workgroup: 8 */
    uint32_t bands;                   /* workgroups down the window */
    uint32_t segments;                /* S: frame segments, each reduced by its own workgroups */
    uint32_t frames_per_segment;      /* fps: frames of every segment but the last (which may hold fewer) */
    uint32_t max_frames_per_segment;  /* 65,536: keeps the kernel's per-lane sums exact */
    uint64_t grid;                    /* projection kernel: pieces_x * bands * segments workgroups */
    uint64_t combine_grid;            /* combine kernel: workgroups (0 = one segment, no combine) */
    uint64_t workspace_bytes;         /* per-segment partials (0 for one segment) */
    uint32_t lds_bytes;               /* projection kernel: LDS per workgroup */
    uint32_t instance;                /* statistics of the kernel instance that runs: 3, 12 or 15 */
} dbde_hip_project_registered_plan_t;
int dbde_hip_project_registered_plan(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu,
                                     dbde_hip_project_registered_plan_t *plan);
int dbde16_hip_project_registered_plan(int W, int H, int n_frames, int rw, int rh, unsigned stats, int n_cu,
                                       dbde_hip_project_registered_plan_t *plan);

/* ---- region traces: per frame and per labelled region, max / min / sum / sum of squares ---------- */
/* A trace map is a label image (H x W int32, row-major, pitch W: 0 = no region, 1..n_labels = region id) classified
 * once per 8x8 tile, counting only the tile's valid pixels (an edge tile's padding beyond W / H belongs to no region):
 *   empty  no pixel has a label > 0: the traces read none of its minimum or payload bytes;
 *   whole  every valid pixel has the same label l > 0 and the tile has no padding: its 64 pixels go to l;
 *   mixed  everything else (edge tiles with padding included): the map keeps its 64 labels as U16, padding 0.
 * Rules: 1 <= n_labels <= 65535 and every label in [0, n_labels], else DBDE_HIP_ERR_ARG.  W and H as the codec's. */
typedef struct dbde_hip_trace_map dbde_hip_trace_map;
typedef struct dbde_hip_trace_map_info_t {
    int32_t W, H;
    uint32_t n_labels;
    uint32_t tiles, tiles_active, tiles_whole, tiles_mixed, reserved_;  /* active = whole + mixed */
    uint64_t device_bytes;                                              /* the map's device memory */
} dbde_hip_trace_map_info_t;
/* Pure host: validates and classifies labels (host memory) without a context.  info (optional) gets the counts;
 * pixels (optional, host, n_labels U64) gets the number of pixels of each label 1..n_labels. */
int dbde_hip_trace_map_summary(const int32_t *labels, int W, int H, int n_labels, dbde_hip_trace_map_info_t *info,
                               uint64_t *pixels);
/* Builds the map in the context's device memory from labels (host memory).  Synchronous.  The map belongs to ctx: it
 * may be used only with ctx, and it must be destroyed before ctx is. */
int dbde_hip_trace_map_create(dbde_hip_ctx *ctx, const int32_t *labels, int W, int H, int n_labels,
                              dbde_hip_trace_map **out);
/* Waits for the map's context's stream, then frees the map.  NULL is allowed. */
void dbde_hip_trace_map_destroy(dbde_hip_trace_map *m);
int dbde_hip_trace_map_info(const dbde_hip_trace_map *m, dbde_hip_trace_map_info_t *info);
/* Device, n_labels U64: the pixels of each label 1..n_labels. */
const uint64_t *dbde_hip_trace_map_pixels(const dbde_hip_trace_map *m);

/* Region traces: for each frame f of n_frames and each label l = j + 1 of the map, the maximum, minimum, sum and sum of
 * squares of frame f's pixels that carry label l, reduced straight from the compressed bytes (no image is written).
 * Inputs and outputs:
 *   Frame f starts at d_stream + d_frame_offsets[f] (any byte alignment; concatenated and slot layouts alike).  No byte
 *   at or beyond stream_bytes is read.  W / H must be the map's, and the map must be ctx's.
 *   Each output is n_frames x n_labels, row-major (column j = label j + 1; label 0 is never reported): d_max and d_min
 *   U8 at any address, d_sum and d_sumsq U64, 8-byte aligned.  A NULL output is neither computed nor touched; at least
 *   one of the four must be non-NULL.  Nothing outside the n_frames x n_labels outputs is written.  d_results
 *   (optional) is filled exactly as dbde_hip_decode_frames fills it.
 * What is reduced: exactly the bytes dbde_hip_decode_frames would write (minima that wrap modulo 256 included), for
 *   the frames it accepts.  A rejected frame reports its usual result entry and its output rows are left untouched.
 *   For an accepted frame, a label without pixels gets the empty reduction: max 0, min 255, sums 0.
 * Every result is an exact integer, independent of the launch shape and of workgroup order (integer atomics).  The U64
 *   sums are exact for any frame the index accepts (at most 2^30 pixels * 65535^2 < 2^64); inside the kernel a
 *   workgroup's run holds at most 2,048 pixels in U32 (2,048 * 255^2 < 2^32).
 * n_frames == 0 does nothing.  Errors: DBDE_HIP_ERR_ARG for a NULL context, map, stream or offsets, a map of another
 *   context or of another W / H, no statistic, or an unaligned U64 output.
 * Asynchronous on the context's stream; workspace (the decode index, and U32 max / min per (frame, label) when max or
 * min is requested) is the context's, grown on demand.  Timing hook: the index kernel in slot 1, the trace kernels in
 * slot 2. */
int dbde_hip_traces(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                    int W, int H, int n_frames, const dbde_hip_trace_map *map, uint8_t *d_max, uint8_t *d_min,
                    uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results);
/* Region traces of DBDE16 frames: dbde_hip_traces' contract with U16 pixels.  Validation is dbde16_hip_decode_frames'
 * own; the values reduced are exactly the U16 values it writes (minima that wrap modulo 2^16 included).  d_max / d_min
 * are U16, 2-byte aligned; the empty minimum is 65535.  Inside the kernel a run holds at most 1,024 pixels, its sum in
 * U32 (1,024 * 65535 < 2^32) and its sum of squares in U64.  Errors: as dbde_hip_traces, and for an unaligned U16
 * output. */
int dbde16_hip_traces(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes, const uint64_t *d_frame_offsets,
                      int W, int H, int n_frames, const dbde_hip_trace_map *map, uint16_t *d_max, uint16_t *d_min,
                      uint64_t *d_sum, uint64_t *d_sumsq, dbde_hip_frame_result *d_results);

/* What dbde_hip_traces runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what dbde_hip_traces
 * validates of its sizes (DBDE_HIP_ERR_ARG otherwise: W / H other than info's, bad n_frames, no statistic, n_cu < 1)
 * and reports the index geometry, the trace kernel's launch and the workspace.  info: the map's
 * (dbde_hip_trace_map_info or dbde_hip_trace_map_summary).  stats: DBDE_HIP_PROJECT_* bitmask. */
typedef struct dbde_hip_trace_plan_t {
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* trace kernel: workgroup size */
    uint32_t tiles_per_workgroup;     /* trace kernel: tile columns of one span (8 lanes per tile; DBDE16: 16) */
    uint32_t spans_x;                 /* spans across a tile row */
    uint32_t spans;                   /* spans of the frame (a workgroup of a span without active tiles returns) */
    uint32_t segments;                /* frame segments, each traced by its own workgroups */
    uint32_t frames_per_segment;      /* frames of every segment but the last (which may hold fewer) */
    uint64_t grid;                    /* trace kernel: spans * segments workgroups */
    uint64_t row_grid;                /* init / finish kernels: workgroups over n_frames * n_labels */
    uint64_t workspace_bytes;         /* U32 max / min per (frame, label) */
} dbde_hip_trace_plan_t;
int dbde_hip_trace_plan(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                        dbde_hip_trace_plan_t *plan);
/* The same for dbde16_hip_traces: 16 lanes per tile, so half the tiles per workgroup and twice the spans. */
int dbde16_hip_trace_plan(int W, int H, int n_frames, const dbde_hip_trace_map_info_t *info, unsigned stats, int n_cu,
                          dbde_hip_trace_plan_t *plan);

/* ---- per-frame intensity histograms ------------------------------------------------------------- */
/* Histograms: for each frame f of n_frames, the counts of the values of the rw x rh window at (x0, y0), counted
 * straight from the compressed bytes (no image is written).
 * Inputs:
 *   Frame f starts at d_stream + d_frame_offsets[f] (any byte alignment; concatenated and slot layouts alike).  No byte
 *   at or beyond stream_bytes is read.  The window and its argument rules are dbde_hip_decode_roi's (plan_roi); there
 *   are no per-frame origins.  The whole frame is 0, 0, W, H.
 * Binning: a pixel value v goes to bin min(v >> shift, bins - 1); the last bin also collects every value above the
 *   range (the saturation bin).  DBDE: 0 <= shift <= 7 and 1 <= bins <= 256 >> shift.  The values binned are exactly
 *   the bytes dbde_hip_decode_frames writes (minima that wrap modulo 256 included), for the frames it accepts.
 * Outputs (at least one of d_hist / d_total; a NULL output is neither computed nor touched):
 *   d_hist   U32 [n_frames][bins], 4-byte aligned.  An accepted frame's row is overwritten with its counts, which sum
 *            to rw * rh (at most 2^30 by the index limit, so U32 is exact).  A rejected frame reports its usual
 *            d_results entry and its row is left untouched.
 *   d_total  U64 [bins], 8-byte aligned, with d_count (one U64, 8-byte aligned, required with d_total): the sum of the
 *            accepted frames' rows and the number of those frames.  accumulate = 0 overwrites them (all zeros for
 *            n_frames == 0 or an all-rejected batch); accumulate = 1 adds to them (n_frames == 0 changes nothing).
 *            Frames [0, n) in one call give the same as any split into consecutive calls with accumulate = 1.
 *   d_results (optional) is filled exactly as dbde_hip_decode_frames fills it.  Nothing outside the outputs is written.
 * Every count is an exact integer, independent of the launch shape and of workgroup order (integer atomics).
 * Errors: DBDE_HIP_ERR_ARG as dbde_hip_project (window, sizes, null stream / offsets), and for shift / bins outside
 *   the rules, no output, a d_total without d_count, or an unaligned output.
 * Asynchronous on the context's stream; workspace (the decode index) is the context's, grown on demand.  Timing hook:
 *   the index kernel in slot 1, the histogram kernels in slot 2. */
int dbde_hip_histogram(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                       const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                       int x0, int y0, int rw, int rh, int shift, int bins, int accumulate,
                       uint32_t *d_hist, uint64_t *d_total, uint64_t *d_count,
                       dbde_hip_frame_result *d_results);
/* Histograms of DBDE16 frames: dbde_hip_histogram's contract with U16 values.  Validation is dbde16_hip_decode_frames'
 * own; the values binned are exactly the U16 values it writes (minima that wrap modulo 2^16 included).  Binning:
 * 0 <= shift <= 15 and 1 <= bins <= min(4096, 65536 >> shift): shift 0 with 4096 bins bins 12-bit data exactly,
 * shift 4 with 4096 bins covers the whole 16-bit range. */
int dbde16_hip_histogram(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                         int x0, int y0, int rw, int rh, int shift, int bins, int accumulate,
                         uint32_t *d_hist, uint64_t *d_total, uint64_t *d_count,
                         dbde_hip_frame_result *d_results);
/* What dbde_hip_histogram runs (pure host arithmetic, like dbde_hip_project_plan): validates exactly what
 * dbde_hip_histogram validates of its arguments (DBDE_HIP_ERR_ARG otherwise) and reports the tile window and index
 * geometry (dbde_hip_roi_plan's), the histogram launch, its LDS and the workspace.  outputs: bitmask, per-frame rows 1,
 * total 2 (dbde_hip_histogram: its non-NULL d_hist / d_total).  n_cu: compute units of the device (dbde_hip_histogram
 * uses its context's). */
enum { DBDE_HIP_HISTOGRAM_ROWS = 1, DBDE_HIP_HISTOGRAM_TOTAL = 2 };
typedef struct dbde_hip_histogram_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* histogram kernel: workgroup size */
    uint32_t tiles_per_piece;         /* histogram kernel: tiles of one piece (8 lanes per tile; DBDE16: 16) */
    uint32_t pieces_x;                /* pieces across a window tile row */
    uint32_t pieces;                  /* pieces of one frame's window: pieces_x * tiles_y */
    uint32_t segments;                /* workgroups per frame, each counting a run of consecutive pieces */
    uint32_t pieces_per_segment;      /* pieces of every segment but the last (which may hold fewer) */
    uint32_t lds_bins;                /* bins of the kernel instance's LDS histogram (256, or 4096 for DBDE16) */
    uint32_t lds_copies;              /* copies of it per workgroup (one per wave, or one shared) */
    uint32_t lds_bytes;               /* LDS per workgroup (histogram copies and the offsets scan) */
    uint32_t reserved_;
    uint64_t grid;                    /* histogram kernel: n_frames * segments workgroups */
    uint64_t init_grid;               /* init kernel: workgroups over max(n_frames, 1) * bins */
    uint64_t global_atomics_per_frame;/* at most: segments * bins per requested output */
    uint64_t workspace_bytes;         /* the decode index: chunk offsets and frame verdicts */
} dbde_hip_histogram_plan_t;
int dbde_hip_histogram_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                            unsigned outputs, int n_cu, dbde_hip_histogram_plan_t *plan);
/* The same for dbde16_hip_histogram: 16 lanes per tile (half the tiles per piece), its bins / shift rules, and the
 * 4096-bin LDS instance (one shared copy) for more than 256 bins. */
int dbde16_hip_histogram_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int shift, int bins,
                              unsigned outputs, int n_cu, dbde_hip_histogram_plan_t *plan);

/* ---- binned decode: b x b block sum, max and min per frame ------------------------------------- */
/* Binned decode: for each frame f of n_frames, the rw x rh window at (x0, y0) reduced in bins of bin x bin pixels,
 * straight from the compressed bytes (no image is written).
 * Inputs:
 *   Frame f starts at d_stream + d_frame_offsets[f] (any byte alignment; concatenated and slot layouts alike).  No byte
 *   at or beyond stream_bytes is read.  bin is 2, 4 or 8.  The window and its argument rules are dbde_hip_decode_roi's
 *   (plan_roi), and x0 and y0 must be multiples of bin, which keeps every bin inside one 8 x 8 tile; rw and rh are
 *   free.  There are no per-frame origins.  The whole frame is 0, 0, W, H.
 * Bins: the planes have oh = ceil(rh / bin) rows and ow = ceil(rw / bin) columns per frame.  Element (i, j) of frame f
 *   reduces the pixels of rows [y0 + i bin, min(y0 + i bin + bin, y0 + rh)) and columns [x0 + j bin,
 *   min(x0 + j bin + bin, x0 + rw)) of the image dbde_hip_decode_frames writes for that frame: exactly the bytes it
 *   writes (minima that wrap modulo 256 included), for the frames it accepts.  Bins on the window's right and bottom
 *   edge are partial: they reduce only the pixels inside the window, never the padding of an edge tile.
 * Outputs (at least one; a NULL plane is neither computed nor touched), each [n_frames][oh][ow], row-major, pitch ow:
 *   d_sum  U16, 2-byte aligned: the bin's sum, at most 64 * 255 = 16,320: exact.
 *   d_max  U8: the bin's largest pixel.      d_min  U8: its smallest.
 *   There is no mean plane: the mean is sum / pixels, and a bin's pixel count follows from the geometry alone.
 *   A rejected frame reports its usual d_results entry and its planes are left untouched.  d_results (optional) is
 *   filled exactly as dbde_hip_decode_frames fills it.  Nothing outside the planes is written.  n_frames == 0 does
 *   nothing.
 * Errors: DBDE_HIP_ERR_ARG as dbde_hip_decode_roi (window, sizes, null stream / offsets), and for a bin other than
 *   2 / 4 / 8, an origin that is not a multiple of bin, no plane, or an unaligned d_sum.
 * Asynchronous on the context's stream; workspace (the decode index) is the context's, grown on demand.  Timing hook:
 *   the index kernel in slot 1, the binning kernel in slot 2. */
int dbde_hip_decode_binned(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int x0, int y0, int rw, int rh, int bin,
                           uint16_t *d_sum, uint8_t *d_max, uint8_t *d_min,
                           dbde_hip_frame_result *d_results);
/* Binned decode of DBDE16 frames: dbde_hip_decode_binned's contract with U16 pixels.  Validation is
 * dbde16_hip_decode_frames' own; the values reduced are exactly the U16 values it writes (minima that wrap modulo 2^16
 * included).  d_sum is U32, 4-byte aligned (at most 64 * 65,535 = 4,194,240: exact); d_max / d_min are U16, 2-byte
 * aligned. */
int dbde16_hip_decode_binned(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                             int x0, int y0, int rw, int rh, int bin,
                             uint32_t *d_sum, uint16_t *d_max, uint16_t *d_min,
                             dbde_hip_frame_result *d_results);
/* What dbde_hip_decode_binned runs (pure host arithmetic, like dbde_hip_roi_plan): validates exactly what
 * dbde_hip_decode_binned validates of its sizes (DBDE_HIP_ERR_ARG otherwise) and reports the tile window and index
 * geometry (dbde_hip_roi_plan's), the planes' shape and bytes, and the binning kernel's launch.  stats: bitmask of the
 * planes asked for (dbde_hip_decode_binned: its non-NULL d_sum / d_max / d_min). */
enum { DBDE_HIP_BINNED_SUM = 1, DBDE_HIP_BINNED_MAX = 2, DBDE_HIP_BINNED_MIN = 4 };
typedef struct dbde_hip_binned_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window covers */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t out_w, out_h;            /* columns and rows of each plane per frame: ceil(rw / bin), ceil(rh / bin) */
    uint32_t threads;                 /* binning kernel: workgroup size = tiles per workgroup (64, or 256; DBDE16: 128) */
    uint32_t pieces_x;                /* binning kernel: workgroups per window tile row */
    uint32_t lds_bytes;               /* LDS per workgroup (the piece's payload, reused as the output band; the scan) */
    uint32_t reserved_;
    uint64_t grid;                    /* binning kernel: n_frames * tiles_y * pieces_x workgroups */
    uint64_t sum_bytes, max_bytes, min_bytes;   /* bytes of each plane asked for (0: not asked for), n_frames frames */
} dbde_hip_binned_plan_t;
int dbde_hip_binned_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                         dbde_hip_binned_plan_t *plan);
/* The same for dbde16_hip_decode_binned: its index, 128 tiles per workgroup for windows more than 64 tiles across, U32
 * sums and U16 maxima / minima. */
int dbde16_hip_binned_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int bin, unsigned stats,
                           dbde_hip_binned_plan_t *plan);

/* ---- scaled float decode: dark-subtracted, gain-corrected F32 / F16 / BF16 ----------------------- */
/* Scaled decode: the rw x rh window of each of n_frames frames as floating point, v = ((float)p - D) * G per pixel,
 * straight from the compressed bytes (no integer image is written).
 * Input and validation: the stream, the window, d_origins and d_results are exactly dbde_hip_decode_roi's -- the same
 *   index kernel, the same clamping of per-frame origins into [0, W-rw] x [0, H-rh], the same result entries.  A
 *   rejected frame leaves its window untouched.  No byte at or beyond stream_bytes is read; nothing outside the
 *   n_frames*rw*rh output elements is written.  n_frames == 0 does nothing.
 * Value: for the pixel at FRAME coordinates (X, Y) with decoded value p -- exactly the byte dbde_hip_decode_frames
 *   writes, wrapping minima included -- the value is v = ((float)p - D) * G with
 *     D = d_dark ? d_dark[Y*W + X] : dark0        G = d_gain ? d_gain[Y*W + X] : gain0.
 *   The maps are F32, [H][W], pitch W, 4-byte aligned, in frame coordinates: a moving window (d_origins) keeps each
 *   sensor pixel's own correction, taken at the clamped origin.
 * Arithmetic: the subtraction and the multiplication are two IEEE binary32 operations, each rounded to nearest even
 *   (never p*G - D*G, never fused); v is then rounded once, to nearest even, to the output type.  F16 overflow goes to
 *   +-inf; F16 and BF16 subnormal results are produced, not flushed; the sign of a zero product is IEEE's (x - x is +0, the
 *   product's sign is the XOR of its operands').  Binary32 subnormals are never flushed: a subnormal D or G is read at
 *   its value, a subnormal difference or product is produced with IEEE gradual underflow (rounded to nearest even),
 *   a product below half the smallest subnormal is +-0, and a subnormal v converts to the BF16 subnormal (or F16 zero)
 *   nearest to it.  A product beyond the largest binary32 value is +-inf.  NaN / Inf in a map propagate; NaN payload
 *   bits are unspecified.
 * Output: out_type is DBDE_HIP_OUT_F32, _F16 or _BF16; d_out is [n_frames][rh][rw] of that type, row-major, pitch rw,
 *   aligned to its element size only (not assumed 16-byte aligned).
 * Errors: DBDE_HIP_ERR_ARG as dbde_hip_decode_roi, and for an unknown out_type, a NULL d_out with n_frames > 0, or a
 *   misaligned d_out or map.
 * Asynchronous on the context's stream; workspace (the decode index) is the context's, grown on demand.  Timing hook:
 *   the index kernel in slot 1, the scaling kernel in slot 2. */
enum { DBDE_HIP_OUT_F32 = 0, DBDE_HIP_OUT_F16 = 1, DBDE_HIP_OUT_BF16 = 2 };
int dbde_hip_decode_scaled(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int x0, int y0, int rw, int rh, const int32_t *d_origins,
                           int out_type, const float *d_dark, float dark0,
                           const float *d_gain, float gain0,
                           void *d_out, dbde_hip_frame_result *d_results);
/* Scaled decode of DBDE16 frames: dbde_hip_decode_scaled's contract with U16 pixels.  Validation is
 * dbde16_hip_decode_frames' own; p is exactly the U16 value it writes (minima that wrap modulo 2^16 included). */
int dbde16_hip_decode_scaled(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                             int x0, int y0, int rw, int rh, const int32_t *d_origins,
                             int out_type, const float *d_dark, float dark0,
                             const float *d_gain, float gain0,
                             void *d_out, dbde_hip_frame_result *d_results);
/* What dbde_hip_decode_scaled runs (pure host arithmetic, like dbde_hip_binned_plan): validates exactly what
 * dbde_hip_decode_scaled validates of its sizes, window and type (DBDE_HIP_ERR_ARG otherwise) and reports
 * dbde_hip_roi_plan's tile window and index geometry, the scaling kernel's launch and LDS, and the output bytes. */
typedef struct dbde_hip_scaled_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window at (x0, y0) */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window at (x0, y0) covers */
    int32_t max_tiles_x, max_tiles_y; /* the most any per-frame origin needs */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* scaling kernel: workgroup size = tiles per workgroup (64, or 256; DBDE16: 128) */
    uint32_t pieces_x;                /* scaling kernel: workgroups per window tile row (the most any origin needs) */
    uint32_t lds_bytes;               /* LDS per workgroup (the piece's payload, reused as the band of pixels; the scan) */
    uint32_t elem_bytes;              /* bytes of an output element: 4, 2, 2 */
    uint64_t grid;                    /* workgroups without per-frame origins */
    uint64_t grid_origins;            /* workgroups with per-frame origins */
    uint64_t out_bytes;               /* n_frames * rw * rh * elem_bytes */
} dbde_hip_scaled_plan_t;
int dbde_hip_scaled_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type,
                         dbde_hip_scaled_plan_t *plan);
/* The same for dbde16_hip_decode_scaled: its index and 128 tiles per workgroup for windows more than 64 tiles across. */
int dbde16_hip_scaled_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, int out_type,
                           dbde_hip_scaled_plan_t *plan);

/* ---- threshold mask decode: a bit per pixel straight from the stream ---------------------------- */
/* Mask decode: for the rw x rh window of each of n_frames frames, one bit per pixel -- whether the decoded value lies
 * inside (or outside) a band -- plus, optionally, the number of set bits per frame and their bounding box, straight from
 * the compressed bytes (no integer image is written).
 * Input and validation: the stream, the window, d_origins and d_results are exactly dbde_hip_decode_roi's -- the same
 *   index kernel, the same clamping of per-frame origins into [0, W-rw] x [0, H-rh], the same result entries.  No byte
 *   at or beyond stream_bytes is read.  n_frames == 0 does nothing.
 * Predicate: for the pixel at FRAME coordinates (X, Y) with decoded value p -- exactly the byte dbde_hip_decode_frames
 *   writes, wrapping minima included --
 *     L = d_lo_map ? d_lo_map[Y*W + X] : lo0        Hh = d_hi_map ? d_hi_map[Y*W + X] : hi0
 *   and the bit is set iff L <= p <= Hh (DBDE_HIP_MASK_INSIDE) or iff p < L or p > Hh (DBDE_HIP_MASK_OUTSIDE).  L > Hh
 *   is legal: the band is empty.  The maps are [H][W] in the pixel type, pitch W, in frame coordinates: a moving window
 *   (d_origins) keeps each sensor pixel's own thresholds, taken at the clamped origin.  Bright objects are lo = t,
 *   hi = 255; dark objects lo = 0, hi = t; |p - bg| > delta is lo = clamp(bg - delta), hi = clamp(bg + delta), OUTSIDE.
 * Mask: d_mask is U64 [n_frames][rh][words], words = ceil(rw / 64), 8-byte aligned; bit (c & 63) of word (c >> 6) of
 *   row r is window pixel (r, c); the bits at and beyond rw of a row's last word are written as 0 (on a little-endian
 *   host: numpy.packbits(bitorder="little") of rows padded to a multiple of 64).  Every word of an accepted frame is
 *   written, by one plain store; nothing outside the n_frames*rh*words words is written.
 * Optional outputs: d_counts is U32 [n_frames], the set bits of each frame; d_boxes is I32 [n_frames][4], x_min, y_min,
 *   x_max, y_max of the set bits in window coordinates, inclusive, (rw, rh, -1, -1) for a frame with none.  Either may
 *   be NULL, and so may d_mask; at least one of the three is required.
 * A rejected frame leaves its mask words untouched; its count is 0 and its box the empty box; d_results has the verdict.
 * Errors: DBDE_HIP_ERR_ARG as dbde_hip_decode_roi, and for an unknown mode, lo0 or hi0 above 255, no output requested,
 *   or a misaligned d_mask (8), d_counts or d_boxes (4).
 * Asynchronous on the context's stream; workspace (the decode index) is the context's, grown on demand.  Timing hook:
 *   the index kernel in slot 1, the mask kernel (with the counts' and boxes' initialisation) in slot 2. */
enum { DBDE_HIP_MASK_INSIDE = 0, DBDE_HIP_MASK_OUTSIDE = 1 };
int dbde_hip_decode_mask(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                         int x0, int y0, int rw, int rh, const int32_t *d_origins,
                         int mode, const uint8_t *d_lo_map, uint32_t lo0,
                         const uint8_t *d_hi_map, uint32_t hi0,
                         uint64_t *d_mask, uint32_t *d_counts, int32_t *d_boxes,
                         dbde_hip_frame_result *d_results);
/* Mask decode of DBDE16 frames: dbde_hip_decode_mask's contract with U16 pixels, U16 maps (2-byte aligned) and
 * thresholds up to 65535.  Validation is dbde16_hip_decode_frames' own; p is exactly the U16 value it writes. */
int dbde16_hip_decode_mask(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int x0, int y0, int rw, int rh, const int32_t *d_origins,
                           int mode, const uint16_t *d_lo_map, uint32_t lo0,
                           const uint16_t *d_hi_map, uint32_t hi0,
                           uint64_t *d_mask, uint32_t *d_counts, int32_t *d_boxes,
                           dbde_hip_frame_result *d_results);
/* What dbde_hip_decode_mask runs (pure host arithmetic, like dbde_hip_scaled_plan): validates exactly what
 * dbde_hip_decode_mask validates of its sizes and window (DBDE_HIP_ERR_ARG otherwise) and reports dbde_hip_roi_plan's
 * tile window and index geometry, the mask kernel's launch and LDS, and the mask's size.  A workgroup owns piece_words
 * whole mask words of one window tile row (pieces are cut in window coordinates, so no word is shared) and decodes the
 * at most 8 * piece_words + 1 <= threads tiles that overlap them at any x mod 8.  Without per-frame origins and with x0
 * a multiple of 8, threads / 8 words are exactly threads tiles: the _fixed fields. */
typedef struct dbde_hip_mask_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window at (x0, y0) */
    int32_t tiles_x, tiles_y;         /* tiles across / down the window at (x0, y0) covers */
    int32_t max_tiles_x, max_tiles_y; /* the most any per-frame origin needs */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t threads;                 /* mask kernel: workgroup size (64 for windows of at most 7 words, else 256; DBDE16: 128) */
    uint32_t pieces_x;                /* with origins: workgroups per window tile row = ceil(words / (threads / 8 - 1)) */
    uint32_t piece_words;             /* with origins: mask words of a row per workgroup = ceil(words / pieces_x) */
    uint32_t lds_bytes;               /* LDS per workgroup (payload reused as the band; the scan; block bits; wave results) */
    uint32_t words;                   /* U64 words per mask row = ceil(rw / 64) */
    uint32_t pieces_x_fixed;          /* at (x0, y0): pieces_x, with threads / 8 words at most when x0 % 8 == 0 */
    uint32_t piece_words_fixed;       /* at (x0, y0): ceil(words / pieces_x_fixed) */
    uint32_t reserved;
    uint64_t grid;                    /* workgroups without per-frame origins */
    uint64_t grid_origins;            /* workgroups with per-frame origins */
    uint64_t mask_bytes;              /* n_frames * rh * words * 8 */
} dbde_hip_mask_plan_t;
int dbde_hip_mask_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_mask_plan_t *plan);
/* The same for dbde16_hip_decode_mask: its index and 128 threads (15 words) per workgroup for windows wider than 7 words. */
int dbde16_hip_mask_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, dbde_hip_mask_plan_t *plan);

/* ---- patch decode: many small windows per frame in one call -------------------------------------- */
/* Patch decode: n_patches windows of one size pw x ph per frame, each with its own origin per frame (one cut-out per
 * tracked object), decoded straight from the compressed stream by ONE index pass and one kernel.  Frame f starts at
 * d_stream + d_frame_offsets[f] (any byte alignment); patch (f, k) goes to d_out + (f*n_patches + k)*ph*pw pixels,
 * row-major, pitch pw; d_out may have any alignment of the pixel size.  Patches may overlap or coincide.
 *   d_origins: device int32 [n_frames][n_patches][2] (x, y), required.
 *   edge_mode: DBDE_HIP_PATCH_CLAMP -- the origin is clamped into [0, W-pw] x [0, H-ph], and patch (f, k) equals, byte
 *              for byte, what dbde_hip_decode_roi writes for frame f with that origin; requires pw <= W and ph <= H.
 *              DBDE_HIP_PATCH_FILL -- the patch sits exactly where the origin says: its pixels inside the frame equal
 *              the full decode, its pixels outside the frame are `fill` (only the low 8 bits may be set; DBDE16: 16),
 *              a patch wholly outside the frame is all fill.  Any int32 origin is legal, INT32_MIN and INT32_MAX
 *              included (nothing overflows: x is first clamped into [-pw, W], y into [-ph, H], which gives the same
 *              patch); pw > W or ph > H is allowed.
 *   d_counts:  optional device uint32 [n_frames]; min(d_counts[f], n_patches) is the number of live patches of frame f,
 *              NULL means all of them.  Patches k >= count and their d_used entries stay untouched.
 *   d_used:    optional device int32 [n_frames][n_patches][2]: the origin actually used -- the clamped one in CLAMP
 *              mode, the given one in FILL mode.
 *   d_results: as in dbde_hip_decode_frames (header fields; consumed = the whole frame's length), may be NULL.
 * Validation is dbde_hip_decode_frames' own (the same index kernel on dbde_hip_roi_plan's geometry): a rejected frame
 * reports the same result entry and leaves all its patches and d_used entries untouched.  No byte at or beyond
 * stream_bytes is read; nothing outside the n_frames*n_patches*ph*pw pixels (and d_used) is written.  n_frames == 0
 * does nothing.  DBDE_HIP_ERR_ARG: n_patches < 1; pw or ph < 1; a patch that could be more than 64 tiles across,
 * (pw + 6)/8 + 1 > 64, so pw <= 505 (ph has no limit); in CLAMP mode pw > W or ph > H; a frame too large for the index
 * (more than 32768 chunks); n_frames * n_patches * groups_per_patch >= 2^31; a null stream, offsets, origins or output;
 * an unknown edge mode; fill above the pixel type.  Asynchronous on the context's stream; timing hook: the index kernel
 * in slot 1, the patch kernel in slot 2. */
enum { DBDE_HIP_PATCH_CLAMP = 0, DBDE_HIP_PATCH_FILL = 1 };
int dbde_hip_decode_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                            const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                            int pw, int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                            int edge_mode, uint32_t fill, uint8_t *d_out, int32_t *d_used,
                            dbde_hip_frame_result *d_results);
/* Patch decode of DBDE16 frames: dbde_hip_decode_patches' contract with U16 pixels (d_out 2-byte aligned, fill up to
 * 65535).  Validation is dbde16_hip_decode_frames' own; CLAMP-mode patches equal dbde16_hip_decode_roi's windows. */
int dbde16_hip_decode_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                              const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                              int pw, int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                              int edge_mode, uint32_t fill, uint16_t *d_out, int32_t *d_used,
                              dbde_hip_frame_result *d_results);
/* What dbde_hip_decode_patches runs (pure host arithmetic, like dbde_hip_roi_plan): refuses exactly the arguments the
 * call refuses, pointers and fill aside (DBDE_HIP_ERR_ARG), and reports the launch.  A 64-lane workgroup takes
 * rows_per_workgroup = max(1, 64 / max_tiles_x) tile rows of one patch, one tile per lane. */
typedef struct dbde_hip_patches_plan_t {
    int32_t max_tiles_x, max_tiles_y; /* the most tiles any origin makes a patch span: (pw + 6)/8 + 1 across, (ph + 6)/8 + 1
                                         down; in CLAMP mode (min(7, W - pw) + pw + 7)/8, as dbde_hip_roi_plan */
    uint32_t rows_per_workgroup;      /* tile rows of one patch per workgroup */
    uint32_t groups_per_patch;        /* workgroups per patch = ceil(max_tiles_y / rows_per_workgroup) */
    uint32_t threads;                 /* workgroup size: 64 */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t lds_bytes;               /* LDS per workgroup (the rows' payload ranges, reused as the band) */
    uint64_t grid;                    /* workgroups: n_frames * n_patches * groups_per_patch */
    uint64_t out_bytes;               /* n_frames * n_patches * ph * pw * pixel size */
} dbde_hip_patches_plan_t;
int dbde_hip_patches_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                          dbde_hip_patches_plan_t *plan);
/* The same for dbde16_hip_decode_patches: its index, LDS and output size. */
int dbde16_hip_patches_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                            dbde_hip_patches_plan_t *plan);

/* ---- patch moments: centroid and shape sums per tracked window ----------------------------------- */
/* Patch moments: for each of n_patches windows of one size pw x ph per frame, each with its own origin per frame (as in
 * dbde_hip_decode_patches), the thresholded image moments up to second order, straight from the compressed stream by
 * ONE index pass and one kernel; no pixel is written.  Stream, offsets, d_origins, d_counts, d_used, d_results,
 * validation and the two edge modes are dbde_hip_decode_patches' own, with one difference: there is no fill value.  A
 * patch pixel outside the frame (the encoder's padding beyond W or H included) is not part of any sum; a FILL-mode
 * patch wholly outside the frame gives all zeros and an empty box.
 *   Selection: pixel p at patch row i (0 <= i < ph), column j (0 <= j < pw), inside the frame, is selected when
 *     lo <= p <= hi.  lo > hi is legal and selects nothing.
 *   Weight w of a selected pixel, by weight_mode: DBDE_HIP_MOMENT_COUNT w = 1; _VALUE w = p; _ABOVE w = p - lo (a bright
 *     object over a dark level); _BELOW w = hi - p (a dark object under a bright level).
 *   d_moments: device uint64 [n_frames][n_patches][8], 8-byte aligned, required.  Over the selected pixels of patch
 *     (f, k): [0] N = sum 1, [1] S = sum w, [2] Sx = sum w j, [3] Sy = sum w i, [4] Sxx = sum w j^2, [5] Sxy = sum w i j,
 *     [6] Syy = sum w i^2, [7] Sww = sum w^2.  Coordinates are relative to the patch, so with pw <= 505 and ph <= 512
 *     every sum stays below 2^63: 65535 * 511^2 * 505 * 512 < 2^63 bounds Syy, the largest, with 511^2 taken for every
 *     row (a DBDE16 patch of all 65535 gives 65535 * 505 * sum i^2, about 2^50.4), and Sww is at most 65535^2 * 505 * 512
 *     < 2^50.  All arithmetic is integer: the sums are exact and do not depend on the launch.
 *   d_bbox: optional device int32 [n_frames][n_patches][4], 4-byte aligned: (j_min, i_min, j_max, i_max) of the
 *     selected pixels, (pw, ph, -1, -1) when none is selected.
 * A rejected frame, and a patch k >= min(d_counts[f], n_patches), leave their moments, box and used entries untouched;
 * the caller zeroes nothing beforehand, every live entry is written once by plain stores.  No byte at or beyond
 * stream_bytes is read; nothing outside the three outputs is written.  n_frames == 0 does nothing.
 * DBDE_HIP_ERR_ARG: whatever dbde_hip_decode_patches refuses for the same sizes and edge mode; ph > 512; lo or hi above
 * the pixel maximum (255; DBDE16: 65535); an unknown weight mode; a null stream, offsets, origins or d_moments; d_moments
 * not 8-byte aligned, d_bbox (or origins, counts, used) not 4-byte aligned.  Asynchronous on the context's stream; timing
 * hook: the index kernel in slot 1, the moments kernel in slot 2. */
enum { DBDE_HIP_MOMENT_COUNT = 0, DBDE_HIP_MOMENT_VALUE = 1, DBDE_HIP_MOMENT_ABOVE = 2, DBDE_HIP_MOMENT_BELOW = 3 };
int dbde_hip_patch_moments(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int pw, int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                           int edge_mode, uint32_t lo, uint32_t hi, int weight_mode,
                           uint64_t *d_moments, int32_t *d_bbox, int32_t *d_used,
                           dbde_hip_frame_result *d_results);
/* Patch moments of DBDE16 frames: the same contract over U16 pixels (lo, hi up to 65535).  Validation is
 * dbde16_hip_decode_frames' own. */
int dbde16_hip_patch_moments(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                             int pw, int ph, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                             int edge_mode, uint32_t lo, uint32_t hi, int weight_mode,
                             uint64_t *d_moments, int32_t *d_bbox, int32_t *d_used,
                             dbde_hip_frame_result *d_results);
/* What dbde_hip_patch_moments runs (pure host arithmetic, shared with the call): refuses exactly the arguments the call
 * refuses, pointers and thresholds aside (DBDE_HIP_ERR_ARG), and reports the launch.  ONE 64-lane workgroup takes a
 * whole patch: it walks steps_per_patch groups of rows_per_workgroup = max(1, 64 / max_tiles_x) tile rows, one tile per
 * lane, and keeps the sums in registers (a 505 x 512 patch is 65 steps of one wave). */
typedef struct dbde_hip_patch_moments_plan_t {
    int32_t max_tiles_x, max_tiles_y; /* the most tiles any origin makes a patch span, as dbde_hip_patches_plan */
    uint32_t rows_per_workgroup;      /* tile rows of one patch per step */
    uint32_t steps_per_patch;         /* groups of tile rows one workgroup walks = ceil(max_tiles_y / rows_per_workgroup) */
    uint32_t threads;                 /* workgroup size: 64 */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t lds_bytes;               /* LDS per workgroup (the rows' payload ranges) */
    uint64_t grid;                    /* workgroups: n_frames * n_patches */
    uint64_t moments_bytes;           /* n_frames * n_patches * 64 */
} dbde_hip_patch_moments_plan_t;
int dbde_hip_patch_moments_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                                dbde_hip_patch_moments_plan_t *plan);
/* The same for dbde16_hip_patch_moments: its index and LDS. */
int dbde16_hip_patch_moments_plan(int W, int H, int n_frames, int pw, int ph, int n_patches, int edge_mode,
                                  dbde_hip_patch_moments_plan_t *plan);

/* ---- patch match: correlation surfaces of templates over a shift search ------------------------- */
/* Patch match: for each of n_patches search patches per frame, each with its own origin per frame (as in
 * dbde_hip_decode_patches), the correlation surfaces of a tw x th template over every integer shift of a search radius
 * S, straight from the compressed stream by ONE index pass and one kernel; no pixel is written.  The search patch is
 * pw = tw + 2S wide and ph = th + 2S high; d_origins are the SEARCH PATCH's origins, so a template at zero shift sits at
 * origin + (S, S).  Stream, offsets, d_origins, d_counts, edge_mode, fill, d_used (the search patch's used origin),
 * d_results and validation are dbde_hip_decode_patches' own.
 *   d_templates: device pixels [n_templates][th][tw], contiguous, aligned to the pixel size, required; n_templates is 1
 *     (every patch uses template 0) or n_patches (patch k uses template k).
 *   stats: a mask of DBDE_HIP_MATCH_PROD, _SUM, _SQ: the surfaces to write.
 *   d_prod, d_sum, d_sq: device uint64 [n_frames][n_patches][D][D], D = 2S + 1, 8-byte aligned; a surface not in stats
 *     may be NULL and is not written.  With P the ph x pw patch dbde_hip_decode_patches writes for the same stream,
 *     origins, edge mode, fill, pw and ph, the entry at row dy + S, column dx + S (-S <= dy, dx <= S) is, over
 *     0 <= i < th, 0 <= j < tw:
 *         prod = sum T[i][j] * P[i + dy + S][j + dx + S]
 *         sum  = sum           P[i + dy + S][j + dx + S]
 *         sq   = sum           P[i + dy + S][j + dx + S]^2
 *     In FILL mode the pixels outside the frame are `fill` and take part like any other pixel (decode_patches' rule, not
 *     patch_moments').  All values are exact integers: an 8-bit entry is at most 128^2 * 255^2 < 2^32, a 16-bit entry
 *     at most 128^2 * 65535^2 < 2^46.
 * A rejected frame, and a patch k >= min(d_counts[f], n_patches), leave their surfaces and used entries untouched; the
 * caller zeroes nothing beforehand, every live entry is written once by plain stores.  No byte at or beyond
 * stream_bytes is read; nothing outside the requested surfaces and d_used is written.  n_frames == 0 does nothing.
 * DBDE_HIP_ERR_ARG: tw or th outside [1, 128]; S outside [0, 16]; whatever dbde_hip_decode_patches refuses for that pw,
 * ph, edge mode and fill; n_templates neither 1 nor n_patches; stats empty or with unknown bits; a requested surface
 * that is NULL or not 8-byte aligned; a null stream, offsets, origins or templates; templates not aligned to the pixel
 * size.  Asynchronous on the context's stream; timing hook: the index kernel in slot 1, the match kernel in slot 2. */
enum { DBDE_HIP_MATCH_PROD = 1, DBDE_HIP_MATCH_SUM = 2, DBDE_HIP_MATCH_SQ = 4 };
int dbde_hip_match_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int tw, int th, int S, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                           int edge_mode, uint32_t fill, const uint8_t *d_templates, int n_templates, unsigned stats,
                           uint64_t *d_prod, uint64_t *d_sum, uint64_t *d_sq, int32_t *d_used,
                           dbde_hip_frame_result *d_results);
/* Patch match of DBDE16 frames: the same contract over U16 pixels (templates U16, 2-byte aligned; fill up to 65535).
 * Validation is dbde16_hip_decode_frames' own. */
int dbde16_hip_match_patches(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                             const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                             int tw, int th, int S, int n_patches, const int32_t *d_origins, const uint32_t *d_counts,
                             int edge_mode, uint32_t fill, const uint16_t *d_templates, int n_templates, unsigned stats,
                             uint64_t *d_prod, uint64_t *d_sum, uint64_t *d_sq, int32_t *d_used,
                             dbde_hip_frame_result *d_results);
/* What dbde_hip_match_patches runs (pure host arithmetic, shared with the call): refuses exactly the arguments the call
 * refuses, pointers aside (DBDE_HIP_ERR_ARG), and reports the launch.  ONE 256-lane workgroup takes a whole search
 * patch: up to four of its waves decode a group of rows_per_wave = max(1, 64 / max_tiles_x) tile rows each per step,
 * one tile per lane, into LDS; then lane t takes the items t, t + 256, ... of the D * D * row_slices (shift, slice)
 * pairs, a slice being every row_slices-th template row. */
typedef struct dbde_hip_match_plan_t {
    int32_t pw, ph;                   /* the search patch: tw + 2S, th + 2S */
    int32_t D;                        /* 2S + 1: a surface is D x D */
    int32_t max_tiles_x, max_tiles_y; /* the most tiles any origin makes the search patch span, as dbde_hip_patches_plan */
    uint32_t rows_per_wave;           /* tile rows a decoding wave takes per step */
    uint32_t decode_waves;            /* waves that decode: min(4, ceil(max_tiles_y / rows_per_wave)) */
    uint32_t steps_per_patch;         /* steps of the decode loop */
    uint32_t row_slices;              /* lanes that share a shift (1: a lane owns its shift, no LDS accumulators) */
    uint32_t threads;                 /* workgroup size: 256 */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t lds_bytes;               /* LDS per workgroup: the band, the template, the payload ranges / accumulators */
    uint64_t grid;                    /* workgroups: n_frames * n_patches */
    uint64_t surface_bytes;           /* n_frames * n_patches * D * D * 8, of ONE surface */
} dbde_hip_match_plan_t;
int dbde_hip_match_plan(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                        int edge_mode, uint32_t fill, unsigned stats, dbde_hip_match_plan_t *plan);
/* The same for dbde16_hip_match_patches: its index, LDS and fill limit. */
int dbde16_hip_match_plan(int W, int H, int n_frames, int tw, int th, int S, int n_patches, int n_templates,
                          int edge_mode, uint32_t fill, unsigned stats, dbde_hip_match_plan_t *plan);

/* ---- compressed-domain crop: a window of each frame as a new stream ------------------------------ */
/* Crops the rw x rh window at (x0, y0) out of each of n_frames DBDE frames and writes it as a complete DBDE frame of an
 * rw x rh image, without decoding the window: tiles whose valid pixels are unchanged are COPIED (depth byte, minimum,
 * payload bytes), only tiles that the window's right or bottom edge cuts are decoded, padded and packed again.
 * Input: exactly as dbde_hip_decode_roi -- frame f at d_stream + d_frame_offsets[f], any byte alignment, concatenated or
 *   slot layout; no byte at or beyond stream_bytes is read.  Validation is dbde_hip_decode_frames' own (the same index
 *   kernel); d_results (optional) is filled exactly as that call fills it, consumed being the SOURCE frame's length.
 * Window: inside the frame as dbde_hip_decode_roi requires, and x0, y0 multiples of 8 (DBDE_HIP_ERR_ARG otherwise); rw
 *   and rh are free.  d_origins (optional, device int32 [n_frames][2]): per-frame (x, y), clamped into
 *   [0, W-rw] x [0, H-rh] as dbde_hip_decode_roi clamps them, then rounded DOWN to a multiple of 8; the origin actually
 *   used goes to d_origins_used (optional, same shape; written for rejected frames too).
 * Output: for every accepted frame the source's 20 header bytes unchanged (index and elapsed_ns bits kept), then
 *   nb = T', depths, nm, minima, n64, payload with T' = ceil(rw/8) * ceil(rh/8).  Layout as dbde_hip_encode_frames:
 *   slot_stride == 0 concatenates from d_out (a ready .dbde body for a video header of rw x rh), otherwise frame f
 *   starts at d_out + f*slot_stride, slot_stride >= dbde_hip_max_frame_bytes(rw, rh).  d_out may have any alignment.
 *   d_out_offsets / d_out_bytes (optional) as the encoder returns them.  out_capacity must cover the worst case
 *   (n_frames * max_frame_bytes(rw, rh), or (n_frames-1)*slot_stride + max): less is DBDE_HIP_ERR_CAPACITY before
 *   anything is launched.
 * Which tiles are copied: window tile (i, j) has valid margins rm = min(8, rw - 8i), dm = min(8, rh - 8j); its source
 *   tile has srm = min(8, W - 8(tx+i)), sdm = min(8, H - 8(ty+j)).  With rm == srm and dm == sdm the tile is copied
 *   verbatim; otherwise it is decoded (wrapping add), its rm x dm valid pixels are constant-padded as
 *   dbde_pack_8x8_partial pads them, and it is packed again.  With per-frame origins the test is per frame.
 * Guarantees: (a) decoding an output frame as an rw x rh frame gives rows [y, y+rh) x columns [x, x+rw) of what
 *   dbde_hip_decode_frames gives for the source, byte for byte.  (b) If the source frame is what an encoder writes,
 *   the output frame is byte-identical to the reference's dbde_pack_frame of the cropped image with the header's 16
 *   index / elapsed bytes carried over.  (c) x0 = y0 = 0, rw = W, rh = H reproduces every accepted source frame byte
 *   for byte.  For valid but NON-CANONICAL streams (a stored minimum that makes the add wrap, a depth larger than the
 *   range needs) copied tiles stay as stored, so only (a) and (c) hold.
 * Rejected frames write nothing: d_out_bytes[f] = 0; d_out_offsets[f] is the slot start in the slot layout and,
 *   concatenated, the position the next accepted frame takes (the body holds the accepted frames only, in order).
 * Nothing outside [offsets[f], offsets[f] + bytes[f]) of the accepted frames is written.  n_frames == 0 does nothing.
 * Asynchronous on the context's stream; workspace is the context's, grown on demand.  Timing hook: the index kernel
 * in slot 1, the crop kernels in slot 2. */
int dbde_hip_crop_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                         const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                         int x0, int y0, int rw, int rh, const int32_t *d_origins,
                         uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                         uint64_t *d_out_offsets, uint64_t *d_out_bytes,
                         int32_t *d_origins_used, dbde_hip_frame_result *d_results);
/* The same for DBDE16 frames in, DBDE16 frames out: U16 minima, depth <= 16, nm = 2T', sizes by
 * dbde16_hip_max_frame_bytes; validation is dbde16_hip_decode_frames' own.  (That format's parity is unpinned.) */
int dbde16_hip_crop_frames(dbde_hip_ctx *ctx, const uint8_t *d_stream, size_t stream_bytes,
                           const uint64_t *d_frame_offsets, int W, int H, int n_frames,
                           int x0, int y0, int rw, int rh, const int32_t *d_origins,
                           uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                           uint64_t *d_out_offsets, uint64_t *d_out_bytes,
                           int32_t *d_origins_used, dbde_hip_frame_result *d_results);
/* What dbde_hip_crop_frames runs (pure host arithmetic, like dbde_hip_roi_plan): validates exactly what it validates
 * of its sizes (DBDE_HIP_ERR_ARG otherwise) and reports the tile window, the output's size, the index geometry and
 * the crop kernels' launches.  The workspace is reported for per-frame origins (records for every tile that any
 * origin could cut); with the fixed origin only recoded_tiles records per frame are kept. */
typedef struct dbde_hip_crop_plan_t {
    int32_t tile_x, tile_y;           /* first tile column / row of the window at (x0, y0) */
    int32_t tiles_x, tiles_y;         /* tiles across / down of the cropped frame */
    uint32_t out_tiles;               /* T' = tiles_x * tiles_y */
    uint32_t recoded_tiles;           /* tiles re-packed per frame at (x0, y0): 0 when both extents end on a tile
                                         boundary or on the frame's own edge */
    uint32_t chunks_per_frame;        /* index: chunks per frame (dbde_hip_roi_plan's geometry) */
    uint32_t chunk_tiles;             /* index: tiles per chunk */
    uint32_t chunk_pieces;            /* index: chunks per tile row, 0 = plain 512-tile chunks */
    uint32_t index_split;             /* index: workgroups per frame */
    uint32_t size_threads, size_lds_bytes;     /* sizing kernel: one workgroup per (frame, window tile row) */
    uint32_t repack_threads, repack_lds_bytes; /* re-pack kernel: one thread per record slot (tiles_x + tiles_y - 1 a frame) */
    uint32_t rows_threads, rows_lds_bytes;     /* row scan: one workgroup per frame */
    uint32_t place_threads, place_lds_bytes;   /* frame scan: one workgroup */
    uint32_t copy_threads, copy_lds_bytes;     /* copy: one workgroup per (frame, window tile row) */
    uint64_t size_grid, rows_grid, place_grid, copy_grid;
    uint64_t repack_grid;             /* 0 when nothing is cut at (x0, y0); with per-frame origins it always runs */
    uint64_t max_out_frame_bytes;     /* worst case of one cropped frame: max_frame_bytes(rw, rh) */
    uint64_t out_capacity;            /* the least out_capacity for n_frames and slot_stride */
    uint64_t workspace_bytes;         /* row and frame tables, records of re-packed tiles (the index's own aside) */
} dbde_hip_crop_plan_t;
int dbde_hip_crop_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                       dbde_hip_crop_plan_t *plan);
int dbde16_hip_crop_plan(int W, int H, int n_frames, int x0, int y0, int rw, int rh, uint64_t slot_stride,
                         dbde_hip_crop_plan_t *plan);

/* ---- window encode: a pitched window of each source image as a frame ---------------------------- */
/* Encodes the rw x rh window at (x0, y0) of each of n_frames source images into DBDE frames, reading the window where
 * it lies: the mirror of dbde_hip_decode_roi, and dbde_hip_encode_frames for sources that are not n contiguous
 * pitch-W images (a padded pitch, a ring buffer's frame stride, a region of a sensor, a tracker's moving window).
 * Source: pixel (x, y) of image f is the byte at d_images + f*frame_stride + y*pitch + x*PIX, PIX = 1 (DBDE16: 2).
 *   pitch and frame_stride are in BYTES; 0 means the compact value (W*PIX, H*pitch).  Otherwise pitch >= W*PIX and
 *   frame_stride >= (H-1)*pitch + W*PIX.  DBDE: base, pitch and stride may have any byte alignment.  DBDE16: pitch and
 *   stride are even and the base is 2-byte aligned.  image_bytes is the readable extent of d_images, as stream_bytes
 *   is for the decoders: it must cover (n_frames-1)*frame_stride + (H-1)*pitch + W*PIX, and no byte at or beyond it
 *   is read.
 * Window: 1 <= rw <= W, 1 <= rh <= H, at any pixel position; tiles are counted from the window's own corner.
 *   d_origins: optional device int32 [n_frames][2] (x, y) per frame, CLAMPED into [0, W-rw] x [0, H-rh] exactly as
 *   dbde_hip_decode_roi clamps.  (x0, y0) must lie in that range either way.
 * Output: frame f is byte for byte what dbde_hip_encode_frames writes for the contiguous rw x rh copy of that window
 *   (the reference's dbde_pack_frame of it): headers, both layouts (slot_stride 0, or >= the worst case of an rw x rh
 *   frame), d_frame_offsets, d_frame_bytes, d_indices / d_elapsed_ns, capacity rules and their error codes are that
 *   call's own, taken for (rw, rh).  d_out may have any alignment.  Only the frames' bytes are written, and the output
 *   does not depend on any source byte outside the window.  n_frames == 0 does nothing.
 * Errors: any broken rule above is DBDE_HIP_ERR_ARG (DBDE_HIP_ERR_CAPACITY for out_capacity; for DBDE16 also for a
 *   slot_stride below the worst case), with nothing launched and nothing written.  The kernel's own limits, also
 *   DBDE_HIP_ERR_ARG: fewer than 2^27 tiles in the window and fewer than 2^31 chunks (256 lanes of 16 window bytes by
 *   8 rows each) in one call; offsets inside the source are 64-bit, so a window's bytes are not limited (4096 x 3072
 *   is 384 chunks a frame).
 * A call that describes exactly dbde_hip_encode_frames' layout (whole frame, compact pitch and stride, no origins)
 * is forwarded to it.  Small windows are not a separate form: a window of a few tiles occupies one mostly idle chunk
 * and is bound by the launch.  Asynchronous on the context's stream; timing hook: slot 0. */
int dbde_hip_encode_window(dbde_hip_ctx *ctx, const uint8_t *d_images, size_t image_bytes,
                           int W, int H, uint64_t pitch, uint64_t frame_stride, int n_frames,
                           int x0, int y0, int rw, int rh, const int32_t *d_origins,
                           uint64_t first_index, const uint64_t *d_indices, const uint64_t *d_elapsed_ns,
                           uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                           uint64_t *d_frame_offsets, uint64_t *d_frame_bytes);
/* The same for U16 pixels in, DBDE16 frames out (what dbde16_hip_encode_frames writes for the window's copy; it has no
 * d_indices / d_elapsed_ns, so neither has this). */
int dbde16_hip_encode_window(dbde_hip_ctx *ctx, const uint16_t *d_images, size_t image_bytes,
                             int W, int H, uint64_t pitch, uint64_t frame_stride, int n_frames,
                             int x0, int y0, int rw, int rh, const int32_t *d_origins,
                             uint64_t first_index, uint8_t *d_out, size_t out_capacity, uint64_t slot_stride,
                             uint64_t *d_frame_offsets, uint64_t *d_frame_bytes);
/* What the window encoders run (pure host arithmetic, like dbde_hip_crop_plan): validates exactly what they validate
 * of sizes, strides and alignment and returns their error code.  image_address: the source's base address (only its
 * alignment matters; 0 = aligned).  out_capacity: 0 = not checked.  has_origins: per-frame origins will be passed (such a call never forwards).
 * n_cu: compute units of the device (the grid is min(chunks, 4 workgroups per CU)). */
typedef struct dbde_hip_window_encode_plan_t {
    uint32_t forwards;                /* 1: the call is dbde_hip_encode_frames' layout and goes there; the kernel fields are 0 */
    uint32_t tiles_x, tiles_y, tiles; /* of the window */
    uint32_t lanes_per_row;           /* lanes a tile row takes: ceil(tiles_x / 2) tile pairs (DBDE16: tiles_x tiles) */
    uint32_t chunks_per_frame;        /* ceil(tiles_y * lanes_per_row / threads) */
    uint32_t chunk_tiles;             /* tiles of a full chunk: 512 (DBDE16: 256) */
    uint32_t record_group;            /* chunk (and frame) records per group of the two-level sums: 64 */
    uint32_t threads, lds_bytes;      /* workgroup size and its LDS */
    uint64_t grid;                    /* persistent workgroups */
    uint64_t pitch, frame_stride;     /* as used: the compact values where 0 was passed */
    uint64_t min_image_bytes;         /* the least image_bytes */
    uint64_t max_out_frame_bytes;     /* worst case of one frame: max_frame_bytes(rw, rh) */
    uint64_t out_capacity;            /* the least out_capacity for n_frames and slot_stride */
    uint64_t workspace_bytes;         /* records, zeroed before each launch */
} dbde_hip_window_encode_plan_t;
int dbde_hip_window_encode_plan(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch,
                                uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh, int has_origins,
                                size_t out_capacity, uint64_t slot_stride, int n_cu,
                                dbde_hip_window_encode_plan_t *plan);
int dbde16_hip_window_encode_plan(uint64_t image_address, size_t image_bytes, int W, int H, uint64_t pitch,
                                  uint64_t frame_stride, int n_frames, int x0, int y0, int rw, int rh, int has_origins,
                                  size_t out_capacity, uint64_t slot_stride, int n_cu,
                                  dbde_hip_window_encode_plan_t *plan);

/* ---- kernel timing hook for bench.py ---------------------------------------------------- */
/* When enabled, every encode / decode call brackets its kernels with HIP events on the
 * context's stream; dbde_hip_timing_read returns accumulated milliseconds and launch counts
 * ([0]=encode kernel, [1]=decode index kernel, [2]=decode kernel, [3]=stream scanner) after synchronising. */
int dbde_hip_timing_enable(dbde_hip_ctx *ctx, int on);
int dbde_hip_timing_read(dbde_hip_ctx *ctx, double ms[4], uint64_t launches[4], int reset);

#ifdef __cplusplus
}
#endif
#endif
