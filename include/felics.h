/*
 * felics.h -- C ABI of libfelics: MI355X-native FELICS lossless image codec.
 *
 * Drop-in boundary for the encode hot path of visanalexandru/felics.  The
 * reference has no FFI layer of its own: its boundary is the public Rust
 * surface in src/compression.rs / src/compression/traits.rs and the
 * cfelics/dfelics command lines.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference repository); the Rust
 * `extern "C"` block a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; no exceptions or aborts cross this boundary;
 *   - pixels are row-major, native-endian u8 (depth 0) or u16 (depth 1),
 *     interleaved RGBRGB... when color == FELICS_COLOR_RGB -- the layout of
 *     `ImageBuffer::as_raw()` (compression.rs:276, :338);
 *   - the caller owns every buffer; the library keeps no pointer after return;
 *   - a context is bound to one GPU (it owns a few HIP streams) and is not thread-safe:
 *     use one context per host thread / per GPU (the reference is single
 *     threaded and re-entrant on distinct images);
 *   - ENCODE RUNS ON THE GPU ONLY.  There is no CPU encode fallback: without a
 *     usable HIP device felics_ctx_create() returns FELICS_E_HIP.
 *   - every function returning int returns FELICS_OK (0) or a negative code.
 */
#ifndef FELICS_H
#define FELICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error.rs:4-19 DecompressionError variants, then the codes this ABI adds */
#define FELICS_OK 0
#define FELICS_E_IO (-1)                  /* DecompressionError::IoError (truncated stream) */
#define FELICS_E_INVALID_VALUE (-2)       /* ::InvalidValue   */
#define FELICS_E_VALUE_OVERFLOW (-3)      /* ::ValueOverflow  */
#define FELICS_E_INVALID_DIMENSIONS (-4)  /* ::InvalidDimensions */
#define FELICS_E_INVALID_COLOR_TYPE (-5)  /* ::InvalidColorType  */
#define FELICS_E_INVALID_PIXEL_DEPTH (-6) /* ::InvalidPixelDepth */
#define FELICS_E_INVALID_SIGNATURE (-7)   /* ::InvalidSignature  */
#define FELICS_E_BUFFER_TOO_SMALL (-8)    /* caller's output buffer cannot hold the result */
#define FELICS_E_HIP (-9)                 /* no device / HIP runtime error (see felics_last_error) */
#define FELICS_E_UNSUPPORTED (-10)        /* valid request this build cannot run on the GPU (one image of >= 3.7 G samples; a 16-bit image of > 2^29 pixels) */
#define FELICS_E_INVALID_ARGUMENT (-11)   /* NULL pointer, bad enum value */
#define FELICS_E_INVALID_INDEX (-12)      /* a restart index is malformed or does not fit the stream it came with */

/* format.rs:8-12 ColorType, format.rs:27-31 PixelDepth (wire values) */
#define FELICS_COLOR_GRAY 0
#define FELICS_COLOR_RGB 1
#define FELICS_DEPTH_8 0
#define FELICS_DEPTH_16 1

/* format.rs:44-49 `pub struct Header` */
typedef struct felics_header {
    uint8_t color_type;
    uint8_t pixel_depth;
    uint32_t width;
    uint32_t height;
} felics_header;

#define FELICS_HEADER_BYTES 14 /* "FLCS", u8 colour, u8 depth, u32 BE width, u32 BE height */

typedef struct felics_ctx felics_ctx;

/* Binds a context to HIP device `device` (>= 0).  Replaces nothing in the
 * reference (it has no device); it is the handle the Rust wrapper would keep
 * in a `struct Encoder`. */
int felics_ctx_create(int device, felics_ctx **out);
void felics_ctx_destroy(felics_ctx *ctx);

/* Upper bound of the .felics size of a w x h image (worst case of the code:
 * 2 flag bits + unary(emax) + terminator at k = 0 for every pixel). */
size_t felics_max_compressed_size(uint32_t w, uint32_t h, int color, int depth);

/* Replaces `<ImageBuffer<Luma<T>|Rgb<T>, Vec<T>> as CompressDecompress>::compress`
 * (compression.rs:255-282, :322-371) and `compress_image` (:412-418): writes the
 * WHOLE file (14-byte header + bit stream, zero padded to a byte) to `out`.
 * A Rust `compress<W: Write>(&self, to: W)` is: call this into a Vec<u8>, then
 * `to.write_all(&buf[..out_len])`.  On FELICS_E_BUFFER_TOO_SMALL *out_len holds
 * the size needed. */
int felics_compress(felics_ctx *ctx, const void *pixels, uint32_t w, uint32_t h, int color,
                    int depth, uint8_t *out, size_t cap, size_t *out_len);

/* n images of one shape in one submission (BASELINE config 3/5: a batch of
 * frames on one GPU).  pixels[i], outs[i], caps[i], lens[i] per image.  Images
 * are independent streams, exactly n calls of felics_compress. */
int felics_compress_batch(felics_ctx *ctx, size_t n, const void *const *pixels, uint32_t w,
                          uint32_t h, int color, int depth, uint8_t *const *outs,
                          const size_t *caps, size_t *lens);

/* Same, with input frames and output already in DEVICE memory (what a capture
 * or decode pipeline that lives on the GPU calls; what bench.py times).
 *   d_pixels : n frames back to back (w*h*channels samples each)
 *   d_out    : device buffer of d_out_cap bytes; stream i is written at
 *              offsets[i] (16-byte aligned, ascending) with lens[i] bytes
 *   offsets, lens : HOST arrays of n entries, filled on return
 * On FELICS_E_BUFFER_TOO_SMALL lens[0] holds the capacity needed.
 * The library works on HIP streams of its own (created non-blocking): the frames must be COMPLETE in memory when the
 * call is made -- synchronise the stream that produced them first (hipStreamSynchronize / an event the host has
 * waited for); the same holds for felics_submit_batch_device (felics_submit_surfaces_device takes a producer event instead) and for the streams handed to
 * felics_decompress_batch_device.  What the library wrote is complete when the blocking call / felics_wait_batch returns. */
int felics_compress_batch_device(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w,
                                 uint32_t h, int color, int depth, void *d_out,
                                 size_t d_out_cap, uint64_t *offsets, uint64_t *lens);

/* The same submission in two halves, for callers that encode batch after batch: felics_submit_batch_device
 * queues the work and returns, felics_wait_batch(ticket) blocks until that batch is complete and fills
 * offsets / lens.  Up to felics_lane_count() submissions can be in flight, each with its own d_out;
 * tickets must be waited for in the order they were handed out.  While the GPU is finishing one batch (its
 * last pack slices) it already classifies, scatters and replays the estimator of the next one, which hides
 * the latency-bound head and tail of a batch.  The synchronous entry points refuse to run
 * (FELICS_E_INVALID_ARGUMENT) while a ticket is outstanding.  The reference has no counterpart (it is one
 * blocking call per image); a Rust wrapper would expose this as a two-deep pipeline over `compress`. */
int felics_submit_batch_device(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w,
                               uint32_t h, int color, int depth, void *d_out, size_t d_out_cap,
                               int *ticket);
/* (also serves the tickets of felics_submit_surfaces_device) */
int felics_wait_batch(felics_ctx *ctx, int ticket, uint64_t *offsets, uint64_t *lens);

/* One image of a mixed-shape batch: its own size, colour and depth. */
typedef struct felics_image {
    const void *pixels;      /* host pointer (felics_compress_images) or device pointer (felics_compress_images_device) */
    uint32_t width, height;
    int color, depth;        /* FELICS_COLOR_*, FELICS_DEPTH_* -- per image */
} felics_image;

/* n images of ANY shapes and types in one call: what felics_compress_batch is for one shape.  Every stream is byte-identical to
 * what felics_compress writes for that image alone.  Every image is checked before anything is launched (the first error in
 * image order is returned; NULL pixels only for a zero-sized image).  Images of one depth and colour and of similar size share a
 * submission (their tile counts padded to the largest of the group, at most 25 %), 8-bit and 16-bit alike; 16-bit images of one
 * shape keep the same-shape path.  outs[i], caps[i], lens[i] per image; on FELICS_E_BUFFER_TOO_SMALL every lens[i] holds the size stream i needs and
 * nothing is written to a buffer that is too small.  The reference has no counterpart (it is one call per image). */
int felics_compress_images(felics_ctx *ctx, size_t n, const felics_image *images, uint8_t *const *outs, const size_t *caps,
                           size_t *lens);

/* Same, with the frames (images[i].pixels) and the output in DEVICE memory.  Stream i is written at offsets[i] of d_out
 * (16-byte aligned, ascending in image order, non-overlapping) with lens[i] bytes; offsets / lens are HOST arrays of n entries.
 * If d_out_cap holds a slot of felics_compress_batch_device's size for every stream, the streams are encoded into those slots;
 * otherwise they are placed exactly, back to back.  On FELICS_E_BUFFER_TOO_SMALL lens[0] holds the capacity needed.  The stream
 * contract of felics_compress_batch_device holds: the frames must be complete in memory when the call is made.  Like the other
 * synchronous entry points it refuses to run (FELICS_E_INVALID_ARGUMENT) while a felics_submit_batch_device ticket is outstanding. */
int felics_compress_images_device(felics_ctx *ctx, size_t n, const felics_image *images, void *d_out, size_t d_out_cap,
                                  uint64_t *offsets, uint64_t *lens);

/* A frame where it lies in DEVICE memory, in any layout strides can describe: the address of sample (x, y, c) is
 *     data + y * row_stride + x * pixel_stride + c * channel_stride        (bytes; c = 0, 1, 2 = R, G, B)
 * All strides are signed, and since a view is only read, zero and negative strides are legal: BGR is data + 2 with
 * channel_stride = -1, a bottom-up image has a negative row_stride, row_stride = 0 repeats one row.  A pitched surface
 * (hipMallocPitch), a sub-rectangle of one, RGBA / BGRA pixels and planar C x H x W tensors are all views.  For depth 16, data and
 * every stride must be multiples of 2.  The reference has no counterpart for strides: its images are `ImageBuffer::as_raw()`. */
typedef struct felics_view {
    const void *data;          /* DEVICE address of sample (x=0, y=0, channel 0) */
    uint32_t width, height;
    int color, depth;          /* FELICS_COLOR_*, FELICS_DEPTH_* */
    int64_t row_stride;        /* bytes from (x, y, c) to (x, y+1, c) */
    int64_t pixel_stride;      /* bytes from (x, y, c) to (x+1, y, c) */
    int64_t channel_stride;    /* bytes from (x, y, c) to (x, y, c+1); ignored for gray */
} felics_view;

/* felics_compress_images_device for views: stream i is byte-identical to what felics_compress writes for the dense copy of view i
 * (still n x `compress`, compression.rs:255-282 / :322-371), and no dense copy is made where the kernels can read the view itself.
 * Everything felics_compress_images_device says holds unless named here: placement and alignment of the streams, slots if
 * d_out_cap holds them and exact placement otherwise, FELICS_E_BUFFER_TOO_SMALL with lens[0], every view checked before anything
 * is launched (the first error in view order; NULL data only for a zero-sized view; FELICS_E_INVALID_ARGUMENT for an odd address
 * or stride at depth 16 and for strides whose extent does not fit 64 bits; the size limits of felics_compress_images), refused
 * while a ticket is outstanding, FELICS_E_HIP on a failed context, n = 0 returns FELICS_OK.
 *   ready_event : a hipEvent_t the caller has recorded behind whatever produces the views and last used d_out, or NULL.  If given,
 *                 every stream of the library waits for it (hipStreamWaitEvent) before it first reads a view or writes d_out in
 *                 this call, and the caller need not synchronise the host.  NULL keeps the contract of
 *                 felics_compress_batch_device: the frames are complete in memory when the call is made.
 * How a view is read (felics_get_view_stats counts them):
 *   dense     : the view is the layout felics_image describes; it takes felics_compress_images_device's path as it is;
 *   in place  : gray8 with pixel_stride = 1 and row_stride >= width (the kernels take the row pitch), and RGB8 of ANY strides
 *               (the plane transform reads the view; the Y / Co / Cg planes it writes exist for dense frames as well);
 *   gathered  : everything else -- gray8 with another pixel stride or a row stride below the width, every 16-bit view -- is copied
 *               to a dense frame in a staging buffer of the context first (one kernel; felics_submit_surfaces_device reads 16-bit
 *               surfaces in place).  So is a view of a sub-batch that has to
 *               be redone (a remedy of felics_stats).
 * The call is blocking: the streams are complete when it returns. */
int felics_compress_views_device(felics_ctx *ctx, size_t n, const felics_view *views, void *ready_event, void *d_out,
                                 size_t d_out_cap, uint64_t *offsets, uint64_t *lens);

/* Host only, no context: checks a view exactly as felics_compress_views_device does and returns the half-open byte range
 * [*lo, *hi) relative to `data` that an encode of the view may read -- the hull of its samples; both 0 for a zero-sized view.
 * The caller's bounds check: the view is safe to encode if data + lo .. data + hi lies inside its allocation. */
int felics_view_extent(const felics_view *v, int64_t *lo, int64_t *hi);

/* How the views of a context's calls were read so far (cumulative). */
typedef struct felics_view_stats {
    uint64_t views;         /* views handed to felics_compress_views_device (calls that passed the checks) */
    uint64_t dense;         /* ... that were the dense layout */
    uint64_t in_place;      /* ... read where they lay */
    uint64_t gathered;      /* ... copied to a dense frame first */
    uint64_t bytes_staged;  /* bytes written by such copies, those of redone sub-batches included */
} felics_view_stats;
/* Writes min(out_size, sizeof(felics_view_stats)) bytes, never more: a caller built against a shorter struct stays valid. */
int felics_get_view_stats(const felics_ctx *ctx, felics_view_stats *out, size_t out_size);

/* n frames of ONE shape, a fixed stride apart, in any layout a view can describe: the ring of pitched surfaces a capture or decode
 * pipeline on the GPU holds, the windows of an N x H x W tensor, the images of an N x C x H x W batch.  Frame i is the view frame0
 * with data + i * frame_stride. */
typedef struct felics_surfaces {
    felics_view frame0;    /* frame 0, with the meaning felics_view has */
    int64_t frame_stride;  /* bytes from sample (x, y, c) of frame i to the same sample of frame i + 1; signed, 0 legal (the frames are only
                              read); a multiple of 2 at depth 16 */
    uint64_t count;        /* n frames */
} felics_surfaces;

/* Host only, no context: felics_view_extent's checks on frame0, then the frame axis (an even frame_stride at depth 16, an extent
 * that fits 64 bits: FELICS_E_INVALID_ARGUMENT), and the half-open byte range [*lo, *hi) relative to frame0.data that an encode of the
 * n frames may read -- the hull of all their samples; both 0 for count == 0 or a zero-sized frame.  Where the kernels read such
 * surfaces in place they load samples only, one at a time or as aligned 16-byte words made of samples and pad bytes of ONE row
 * (8-bit surfaces: the words of felics_compress_views_device's in-place class, which lie inside the hull or are aligned 16-byte words
 * that also hold a byte of it); pad bytes may be read and are never interpreted. */
int felics_surfaces_extent(const felics_surfaces *s, int64_t *lo, int64_t *hi);

/* felics_submit_batch_device for surfaces, behind a producer event: queues the batch and returns; felics_wait_batch(ticket) fills
 * offsets / lens (s->count entries each).  Stream i is byte-identical to felics_compress of the dense copy of frame i.  The descriptor
 * is copied at the call; the surfaces, d_out and the event must stay valid and untouched until the ticket has been waited for.
 * Every argument is checked before anything is launched (felics_surfaces_extent's checks and the size limits of
 * felics_compress_images; NULL pointers and count == 0: FELICS_E_INVALID_ARGUMENT; count > 2^24: FELICS_E_UNSUPPORTED; FELICS_E_HIP on a
 * failed context); with every lane
 * holding a ticket it returns FELICS_E_INVALID_ARGUMENT.  Tickets of felics_submit_batch_device and of this call share the lanes
 * (felics_ctx_lane_count) and the waiting order, and the synchronous entry points refuse to run while either kind is outstanding.
 *   ready_event : as in felics_compress_views_device -- a hipEvent_t recorded behind whatever produces the surfaces and last used
 *                 d_out, or NULL.  Every stream of the library waits for it before its first read of a surface or write of d_out;
 *                 the caller does not synchronise the host.  NULL: the surfaces are complete in memory when the call is made.
 * The call creates no HIP stream.
 * QUEUED (the kernels read the surfaces where they lie, nothing is staged) when all of these hold:
 *   - the layout can be read in place: gray8 with pixel_stride = 1 and row_stride >= width; RGB8 of any strides; gray16 with
 *     pixel_stride = 2 and row_stride >= 2 * width; RGB16 of any (even) strides;
 *   - the frames are not zero-sized and count fits one sub-batch (8192 frames, fewer for large frames: the pass bound of
 *     felics_compress_images);
 *   - d_out_cap holds count slots of felics_compress_images_device's size (frame bytes * 1.25 + 64, rounded up to 16): stream i is
 *     then at i * slot;
 *   - the context is not on the two-pass kernels (felics_stats).
 *   A descriptor that is exactly the dense back-to-back layout of felics_submit_batch_device takes that call's path as it is (its
 *   slots: (d_out_cap / count) & ~15), with the event in front of its first kernel: the event-ordered form of that call.
 *   A queued sub-batch that needs a remedy of felics_stats is redone at the wait from gathered frames (counted in bytes_staged);
 *   after a slot overflow the streams are placed exactly, back to back, in d_out; if d_out cannot hold them the wait returns
 *   FELICS_E_BUFFER_TOO_SMALL and lens[0] holds the capacity needed.
 * IMMEDIATE: everything else is encoded during the call and handed over at the wait, with the result felics_compress_views_device
 *   gives for the n views -- its classes, its exact placement, FELICS_E_BUFFER_TOO_SMALL with lens[0] -- counted in
 *   felics_surface_stats and not in felics_view_stats. */
int felics_submit_surfaces_device(felics_ctx *ctx, const felics_surfaces *s, void *ready_event, void *d_out, size_t d_out_cap, int *ticket);

/* Submit and wait in one blocking call; offsets / lens are HOST arrays of s->count entries.  Refused (FELICS_E_INVALID_ARGUMENT) while
 * a ticket is outstanding; count == 0 returns FELICS_OK. */
int felics_compress_surfaces_device(felics_ctx *ctx, const felics_surfaces *s, void *ready_event, void *d_out, size_t d_out_cap,
                                    uint64_t *offsets, uint64_t *lens);

/* What became of a context's surface submissions so far (cumulative). */
typedef struct felics_surface_stats {
    uint64_t submissions;      /* calls of the two functions above that passed the checks (count > 0) */
    uint64_t queued;           /* ... that were queued */
    uint64_t immediate;        /* ... that were encoded during the call */
    uint64_t frames_in_place;  /* frames read where they lay (dense descriptors included) */
    uint64_t frames_gathered;  /* frames of immediate submissions that were copied to a dense frame first */
    uint64_t bytes_staged;     /* bytes written by such copies, those of redone sub-batches included */
} felics_surface_stats;
/* Writes min(out_size, sizeof(felics_surface_stats)) bytes, never more. */
int felics_get_surface_stats(const felics_ctx *ctx, felics_surface_stats *out, size_t out_size);

/* Replaces `read_header` (format.rs:63-84). */
int felics_read_header(const uint8_t *in, size_t len, felics_header *hdr);
/* Replaces `write_header` (format.rs:51-61): writes FELICS_HEADER_BYTES bytes. */
int felics_write_header(const felics_header *hdr, uint8_t *out, size_t cap);

/* Replaces `decompress_image` / `CompressDecompress::decompress`
 * (compression.rs:420-441, traits.rs:57-64).  Host (CPU) implementation: the
 * entropy decoder is bit-serial per plane.  `pixels` receives
 * width*height*channels samples of the depth the header states. */
int felics_decompress(const uint8_t *in, size_t len, void *pixels, size_t pixels_cap,
                      felics_header *hdr);

/* Replaces `CompressDecompress::decompress_with_header(from, &Header)` (traits.rs:53-56; compression.rs:284-314,
 * :373-409): the caller has read (or knows) the header; `in` points at the bit stream BEHIND the 14 header bytes.
 * The header's claims are checked against pixels_cap and against the stream length before anything is allocated. */
int felics_decompress_with_header(const uint8_t *in, size_t len, const felics_header *hdr, void *pixels,
                                  size_t pixels_cap);

/* GPU decoder: n streams of ONE shape resident in device memory (stream i at d_streams + offsets[i], lens[i] bytes:
 * exactly what felics_compress_batch_device leaves behind) decoded into d_pixels (n frames back to back, the layout
 * the encoder takes).  offsets / lens / status are HOST arrays of n entries; status[i] is FELICS_OK or the
 * DecompressionError code of stream i; the function returns the first non-zero status (or a HIP / argument
 * error).  *hdr (optional) receives the header all streams must share; it is read from stream 0.
 * Replaces n calls of `decompress_image` (compression.rs:420-441).  The format is bit-serial per stream (and the
 * planes of an RGB image share one bit stream), so the only parallelism is across streams: one wave per stream, or, in large
 * batches of streams at least 8 pixels wide, 64 streams per wave with a stream per lane.  16-bit data: k_decode16 (a wave per
 * stream, a 8.4 MB estimator table per stream in device memory, rows tagged with an epoch) or k_decode16_lanes (a lane per stream,
 * a hashed table sized by the stream's pixel count: 512 KB per plane of a 64 x 64 stream), the latter from
 * felics_decode_lanes_min_streams(1, color) streams on; felics_get_decode_stats says which form a call's streams took.
 * status[] is written for all n streams on every return (a call that ends before decoding -- bad header of stream 0, buffer too
 * small, a HIP error -- puts its own code in every entry).  The kernel loads a stream as whole ALIGNED 32-bit words: it may
 * touch up to three bytes on either side of a stream, always inside an aligned word that also holds a byte of the stream,
 * hence never outside the page the stream lies in; those bytes are never interpreted. */
int felics_decompress_batch_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets,
                                   const uint64_t *lens, void *d_pixels, size_t d_pixels_cap, felics_header *hdr,
                                   int *status);

/* The headers of n streams resident in device memory (stream i at d_streams + offsets[i], lens[i] bytes), read on the device in
 * one launch and copied back once.  offsets / lens / hdrs / status are HOST arrays of n entries.  status[i] is exactly what
 * felics_read_header returns for stream i's first min(lens[i], FELICS_HEADER_BYTES) bytes; hdrs[i] is that header, zeroed where
 * status[i] != FELICS_OK.  Returns the first non-zero status; a HIP error or a refusal puts its own code in every status[i]
 * (NULL pointers: FELICS_E_INVALID_ARGUMENT, nothing written).  No byte outside [offsets[i], offsets[i] + lens[i]) is read.
 * Like the other synchronous entry points it refuses to run (FELICS_E_INVALID_ARGUMENT) while a felics_submit_batch_device
 * ticket is outstanding; n = 0 returns FELICS_OK. */
int felics_read_headers_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                               felics_header *hdrs, int *status);

/* n streams of ANY shapes, colours and depths, resident in device memory (stream i at d_streams + offsets[i], lens[i] bytes),
 * decoded in one call: what felics_decompress_batch_device is for one shape.  offsets / lens / pix_offsets / hdrs / status are
 * HOST arrays of n entries; hdrs is optional.
 *   - Output placement: frame i is written at d_pixels + pix_offsets[i], w * h * channels * bytes_per_sample bytes in the layout
 *     the encoder takes.  Offsets are 16-byte aligned, ascending in stream order, and frames do not overlap.  A stream whose
 *     header is invalid, or whose frame is empty, gets 0 bytes.  Bytes of d_pixels outside the frames are never written.
 *   - Per-stream status: every stream has its own header and its own status; one bad stream does not fail the others (unlike
 *     the same-shape call, where stream 0 names the shape).  Codes: the header codes of felics_read_header, then
 *     FELICS_E_IO / _INVALID_VALUE / _INVALID_DIMENSIONS as for the same-shape call.  status[] is filled on every return.
 *     hdrs[i] receives the header where felics_read_header would accept it, zeros otherwise.
 *   - A header that claims more than the stream can hold is rejected before anything is sized: a valid stream of C planes has
 *     at least C * (64 + max(0, w * h - 2)) bits behind its header.  A shorter stream gets FELICS_E_IO and no output space; a
 *     header with w * h >= 2^32 gets FELICS_E_INVALID_DIMENSIONS.
 *   - Buffer too small: if d_pixels_cap cannot hold the layout the call returns FELICS_E_BUFFER_TOO_SMALL, pix_offsets[0] holds
 *     the capacity needed, hdrs is filled, nothing is written to d_pixels, the streams that would have been decoded get
 *     FELICS_E_BUFFER_TOO_SMALL and the others keep their header status.
 *   - Refusals as for the other synchronous entry points: FELICS_E_INVALID_ARGUMENT for NULL pointers or while a
 *     felics_submit_batch_device ticket is outstanding, FELICS_E_HIP on a failed context; n = 0 returns FELICS_OK.
 *   - The stream contract of felics_decompress_batch_device holds (complete in memory when the call is made; the kernels load
 *     whole aligned words).  The same stream may be referenced several times.
 * Returns the first non-zero status.  8-bit streams decode one wave per stream, or 64 streams of one shape per wave in calls of
 * many 8-bit streams; 16-bit streams likewise: one wave per stream, or, in calls of at least
 * felics_decode_lanes_min_streams(1, color) 16-bit streams, whole waves of 64 streams of one shape and colour (the rest of such a
 * group a wave per stream); streams whose rows do not fit the LDS on the host.  felics_get_decode_stats counts the forms. */
int felics_decompress_images_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                    void *d_pixels, size_t d_pixels_cap, uint64_t *pix_offsets, felics_header *hdrs, int *status);

/* Which form the streams of a context's device decode calls took so far. */
typedef struct felics_decode_stats {   /* cumulative per context */
    uint64_t streams;       /* streams handed to the two device decode calls (calls that passed the checks) */
    uint64_t wave8, lanes8; /* 8-bit streams decoded a wave per stream / a lane per stream */
    uint64_t wave16, lanes16;
    uint64_t host;          /* streams that went to the host decoder (rows too wide for the LDS) */
    uint64_t undecoded;     /* streams that got a status without being decoded (bad header, too short, buffer too small) */
    uint64_t lanes16_table_bytes; /* table memory the last call's 16-bit lane launches used (its largest pass) */
} felics_decode_stats;
/* Writes min(out_size, sizeof(felics_decode_stats)) bytes, never more: a caller built against a shorter struct stays valid. */
int felics_get_decode_stats(const felics_ctx *ctx, felics_decode_stats *out, size_t out_size);
/* Streams of a depth (0: 8 bits, 1: 16) a device decode call must hold for them to go 64 to a wave (color: 0 gray, 1 RGB);
 * 0xFFFFFFFF: no call does.  FELICS_TEST_DECODE16_LANES=1 / =0 in the environment (read per call) forces / forbids that form for
 * 16-bit streams whatever the count. */
uint32_t felics_decode_lanes_min_streams(int depth, int color);

/* ---- Restart index: one large 8-bit stream decoded on many waves ----
 * A FELICS stream is bit-serial: the context and the Rice parameter of a pixel depend on everything decoded before it, so a stream
 * decodes on one wave however large it is.  The restart index is a SIDECAR beside the unchanged .felics stream (the reference has no
 * counterpart; a stream without one decodes as ever): for every `segment_pixels` pixels of every plane it holds what a decoder
 * needs to start at that pixel -- the bit position, the estimator's counters, and the 2 W samples in front of it.  With it
 * felics_decompress_batch_device_indexed gives every segment of every plane a wave of its own.
 *
 * Format (one blob per stream, little-endian).  segment_pixels is the caller's choice, a multiple of
 * FELICS_INDEX_GRANULE and at least that; K = ceil(W * H / segment_pixels) segments per plane (K = 0 for an empty image).
 *   header, 64 bytes : "FLCX" | u16 version = 1 | u8 colour | u8 depth (0) | u32 width | u32 height | u32 segment_pixels | u32 K |
 *                      u64 plane_end_bit[3] (the bit behind plane c's last code, counted from the stream's first byte, header
 *                      included; unused entries 0) | 16 reserved zero bytes
 *   checkpoints      : for plane c = 0 .. C - 1, segment j = 0 .. K - 1, at 64 + (c * K + j) * S, S = the fields below rounded up to
 *                      a multiple of 16 (zero padded).  With p0 = j * segment_pixels:
 *       u64 bit_offset      : bits from the stream's first byte to the first bit of pixel p0's code; for j = 0 the plane's start, in
 *                             front of its two raw 32-bit samples
 *       u16 state[nctx][6]  : the KEstimator counters (parameter_selection.rs:24-85) of every context as they stand before pixel
 *                             p0; nctx = 256 for gray, 512 for Y / Co / Cg (row 511 is zero); all zero for j = 0.  CANONICAL FORM:
 *                             a context with no out-of-range pixel at or behind p0 in this plane is stored as zeros (its state is
 *                             never read again).  Counters of planes that decode to 8-bit samples stay below 2^16 (e <= 510: a
 *                             counter grows at most 511 / 21 times as fast as the one that triggers the halving at 1024)
 *       window[2 W]         : the plane's samples p0 - 2 W .. p0 - 1 in raster order, zero where the index is negative; u8 for
 *                             gray, i16 for Y / Co / Cg.  Two rows, not one: a segment that starts mid-row at (x0, y0) needs
 *                             (0, y0 - 1) for the first pixel of row y0 + 1, one that starts at x0 = 0 needs (0, y0 - 2)
 *                             (misc.rs:14-23)
 * Checks, the same on the host and on the GPU; any failure is FELICS_E_INVALID_INDEX: magic, version, size = felics_index_size;
 * colour, depth, width, height equal the stream header's; every bit_offset is >= 112 and <= 8 * len and ascends in (plane, segment)
 * order, a plane's first one standing on the end of the plane before it; ceil(plane_end_bit[C - 1] / 8) = len; window samples are in
 * the plane's range (Y 0..255, Co / Cg -255..255); and the END CHECK: a segment that has decoded its pixels stands exactly on the
 * next checkpoint's bit_offset (plane_end_bit[c] for a plane's last segment).
 * WHAT THE CHECKS DO NOT PROVE: an index that passes all of this but was built from another stream can still yield wrong pixels,
 * as a corrupt stream can.  Pairing index and stream is the caller's contract.  No index makes the decoder read or write out of
 * bounds.  The REGION calls (below) prove less still: they make the checks of the segments a region needs and of no other, and
 * no end check where a walk stops early.  16-bit streams have none in these calls; see "Restart index: 16-bit streams" below: every call here
 * returns FELICS_E_UNSUPPORTED for them. */
#define FELICS_INDEX_GRANULE 4096u

/* Host only: the size of the index of a w x h 8-bit image; 0 for depth 16, a bad colour, w * h >= 2^32 or a segment_pixels that
 * is not a positive multiple of FELICS_INDEX_GRANULE. */
size_t felics_index_size(uint32_t w, uint32_t h, int color, int depth, uint32_t segment_pixels);

/* Host only: builds the index of ANY 8-bit stream (files written by the reference included) by decoding it once on the CPU.
 * `len` is the stream's exact length (bytes behind the last code: FELICS_E_INVALID_ARGUMENT).  Returns the stream's own decode
 * error if the stream is bad, FELICS_E_INVALID_ARGUMENT for a bad segment_pixels, FELICS_E_BUFFER_TOO_SMALL with *index_len = the
 * size needed if cap is short, FELICS_E_UNSUPPORTED for a 16-bit stream or a counter that does not fit 16 bits (never truncated). */
int felics_index_build(const uint8_t *in, size_t len, uint32_t segment_pixels, uint8_t *index, size_t cap, size_t *index_len);

/* Host only: felics_decompress through the index -- segment by segment, each from its checkpoint alone (bit position, table and
 * window are re-initialised from the index, nothing is carried over from the segment before).  The pixels are those of
 * felics_decompress; the first failing check or segment in (plane, segment) order gives the code. */
int felics_decompress_indexed(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, void *pixels, size_t pixels_cap,
                              felics_header *hdr);

/* GPU, the index for free: felics_compress_batch_device (blocking, one shape, 8-bit) plus the restart index of stream i at
 * d_index + i * felics_index_size(w, h, color, depth, segment_pixels) (d_index 16-byte aligned).  The streams are byte-identical to
 * felics_compress_batch_device's and the indexes to felics_index_build's of those streams: the encoder already computes the
 * estimator's state at every 16-event record, every tile's bit offset and, for RGB, the Y / Co / Cg planes, and a small kernel per
 * pass collects them (felics_index.hip) -- on both placements of the streams, after every remedy of felics_stats (a pass that is
 * redone rewrites its indexes) and for batches of several passes.  FELICS_E_BUFFER_TOO_SMALL for a short d_index_cap and
 * FELICS_E_INVALID_ARGUMENT for a bad segment_pixels, before anything is launched; FELICS_E_UNSUPPORTED for depth 16; refused like
 * the other synchronous entry points while a ticket is outstanding. */
int felics_compress_batch_device_indexed(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, int depth,
                                         void *d_out, size_t d_out_cap, uint32_t segment_pixels, void *d_index, size_t d_index_cap,
                                         uint64_t *offsets, uint64_t *lens);

/* GPU: n 8-bit streams of ONE shape, each with its index (index i at d_index + i * index_stride; d_index and index_stride multiples
 * of 16, index_stride >= the index's size), decoded a wave per (stream, plane, segment): k_decode8_seg.  Output layout and status
 * conventions of felics_decompress_batch_device; stream 0's header names the shape, index 0's header names segment_pixels and K,
 * and a stream whose own index header differs gets FELICS_E_INVALID_INDEX.  All checks above are made on the device; status[i] is
 * the code of stream i's first failing segment in (plane, segment) order; a failing segment leaves only its own pixels undefined
 * (for RGB: the frame is not converted).  Rows too wide for the LDS and 16-bit streams: FELICS_E_UNSUPPORTED in every status (no
 * host fallback in this call).  Refused like the other synchronous entry points while a ticket is outstanding.
 * WHICH FORM A CALL TAKES.  A wave per segment is the form for a few frames; once the segments fill the chip, 63 of such a wave's 64
 * lanes idle.  Segment j of 64 frames of one shape starts at the same pixel, so a large call decodes 64 segments per wave, a lane
 * per stream (k_decode8_seg_lanes): with W >= 8, K >= 1 and n >= 64, the first n / 64 * 64 streams take that form if they make
 * felics_index_lanes_min_items(color) items (n / 64 * 64 * C * K) or more, and the other n % 64 streams a wave per segment beside
 * them in the same call.  Checks, statuses and pixels are the same in both forms; felics_index_stats says which ran.
 * FELICS_TEST_INDEX_LANES=1 / =0 in the environment (read per call) forces / forbids the lane form for calls with W >= 8, K >= 1 and
 * n >= 64, whatever the item count; FELICS_TEST_INDEX_LANES_PASS=k caps one pass of that form at k items (rounded down to whole
 * waves of 64, at least one wave; tests).  The lane form runs in passes of whole waves, each within the table memory the context
 * may take (6 KB per RGB item, 3 KB per gray one; at most a quarter of the free device memory).  The region call, 16-bit streams,
 * W < 8 and n < 64 keep a wave per segment. */
int felics_decompress_batch_device_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                           const void *d_index, size_t index_stride, void *d_pixels, size_t d_pixels_cap, felics_header *hdr,
                                           int *status);

/* What a context's indexed decode calls did so far (cumulative).  (felics_decode_stats keeps its eight fields: these are counted here.) */
typedef struct felics_index_stats {
    uint64_t streams;    /* streams handed to felics_decompress_batch_device_indexed (calls that passed the checks) */
    uint64_t segments8;  /* segments that got a wave each */
    uint64_t lane_segments8;  /* segments walked by a lane each, 64 to a wave; segments8 + lane_segments8 = n * C * K per call */
    uint64_t lane_passes;     /* lane-form passes launched */
} felics_index_stats;
/* Writes min(out_size, sizeof(felics_index_stats)) bytes, never more: a caller built against the two-field struct stays valid. */
int felics_get_index_stats(const felics_ctx *ctx, felics_index_stats *out, size_t out_size);
/* Lane-form items (n / 64 * 64 * C * K) from which felics_decompress_batch_device_indexed takes the lane form by itself (color: 0
 * gray, 1 RGB); 0xFFFFFFFF: no call does, the form is reachable through FELICS_TEST_INDEX_LANES=1 only. */
uint32_t felics_index_lanes_min_items(int color);

/* ---- Restart index: regions ----
 * Random access through the index: the w x h window at (x, y) of a frame, from the segments that hold a pixel of it and from no
 * other.  A plane's segment j covers its pixels [j * segment_pixels, min(W * H, (j + 1) * segment_pixels)) in raster order; it is
 * NEEDED iff that range meets [yy * W + x, yy * W + x + w) for some row yy of the region.  The needed segments are not always one
 * range: where a row is wider than a segment, those wholly between two rows' column spans are skipped.  The stream is serial, so a
 * needed segment is walked from its first pixel, and up to stop = min(its end, (y + h - 1) * W + x + w) -- not to its end.
 * WHAT A REGION'S CHECKS COVER: the stream header and the index header in full; of the NEEDED segments the bit range
 * (bit_offset rules above) and the window samples; the end check of a segment that is walked to its end; of a walk that stops
 * early only that the reader did not run off the stream.  WHAT THEY LEAVE OUT: every check of a segment the region does not need,
 * and the end check of a walk that stops early -- a region call can succeed on a pair felics_decompress_indexed refuses, and it
 * proves no more about the rest of the index than the paragraph above says of the whole. */
typedef struct felics_region {
    uint32_t stream;      /* which stream of the call (device call only) */
    uint32_t x, y, w, h;  /* the window: x + w <= W, y + h <= H; w = 0 or h = 0 is an empty region */
} felics_region;

/* Host only, the planner: the needed segments of a plane of a W x H image cut every segment_pixels pixels, ascending, worked out
 * per segment in closed form.  *count = how many there are (0 for an empty region); FELICS_E_BUFFER_TOO_SMALL if cap is short (segs
 * may be NULL then), FELICS_E_INVALID_ARGUMENT for x + w > W or y + h > H (64-bit sums), W * H >= 2^32 or a bad segment_pixels.
 * r->stream is ignored. */
int felics_region_segments(uint32_t W, uint32_t H, uint32_t segment_pixels, const felics_region *r, uint32_t *segs, size_t cap,
                           size_t *count);

/* Host only: the dense w x h x C crop of the stream's image (every sample that of felics_decompress at its place), decoded from the
 * checkpoints of the needed segments alone, in (plane, segment) order; the first failure gives the code.  The host model of
 * k_decode8_region: the same checks in the same order (above).  FELICS_E_INVALID_ARGUMENT for a region outside the image,
 * FELICS_E_BUFFER_TOO_SMALL for w * h * C > pixels_cap.  r->stream is ignored. */
int felics_decompress_region_indexed(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *r,
                                     void *pixels, size_t pixels_cap, felics_header *hdr);

/* GPU: n_regions windows of n_streams 8-bit streams of ONE shape with their indexes, all in device memory as for
 * felics_decompress_batch_device_indexed (same alignment rules; stream 0's header names the shape, index 0's segment_pixels and K).
 * Region r is a window of stream regions[r].stream (`regions` is host memory; several may name one stream); its crop is written
 * dense at d_pixels + out_offsets[r], the crops back to back in request order (out_offsets: host, optional).  One wave per
 * (region, plane, needed segment): k_decode8_region, the indexed call's walk stopped at `stop`; RGB scratch is crop-sized.  status[r]
 * (n_regions of them) is the code of region r's first failing item in (plane, segment) order, after the header checks of its stream
 * and index (made for an empty region too).  A failing region leaves only its own crop undefined.
 * Before anything is launched: FELICS_E_INVALID_ARGUMENT for a region outside the image or a stream number >= n_streams,
 * FELICS_E_BUFFER_TOO_SMALL if the crops do not fit d_pixels_cap; rows too wide for the LDS and 16-bit streams: FELICS_E_UNSUPPORTED
 * (a call that ends so puts its code into every status).  Refused like the other synchronous entry points while a ticket is
 * outstanding.  Dense output only: no views, no ready event, no queued form. */
int felics_decompress_regions_device_indexed(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                             const uint64_t *lens, const void *d_index, size_t index_stride, size_t n_regions,
                                             const felics_region *regions, void *d_pixels, size_t d_pixels_cap, uint64_t *out_offsets,
                                             felics_header *hdr, int *status);

/* What a context's region calls did so far (cumulative; calls that passed the checks before the launch). */
typedef struct felics_region_stats {
    uint64_t regions;           /* regions handed in */
    uint64_t segments_walked;   /* (region, plane, segment) waves launched */
    uint64_t segments_skipped;  /* C * K per region minus what was walked */
    uint64_t pixels_walked;     /* pixels those waves were asked to decode: stop - first pixel, summed */
} felics_region_stats;
/* Writes min(out_size, sizeof(felics_region_stats)) bytes, never more. */
int felics_get_region_stats(const felics_ctx *ctx, felics_region_stats *out, size_t out_size);

/* felics_decompress_images_device into views: stream i (at d_streams + offsets[i], lens[i] bytes) is decoded straight into views[i]
 * -- sample (x, y, c) of the decoded image lands at data + y * row_stride + x * pixel_stride + c * channel_stride, sample for sample
 * what felics_decompress yields for that stream.  felics_view is the encoder's, unchanged; its `data` is `const void *`, and THIS CALL
 * WRITES THROUGH IT.  The tiles of a loader go where they are wanted -- the images of an N x C x H x W batch tensor, the cells of a
 * mosaic, a pitched or RGBA surface the next kernel or a display owns -- with no second buffer and no re-layout pass.  The reference
 * has no counterpart (its decoder returns a fresh `ImageBuffer`, compression.rs:420-441).
 * Everything felics_decompress_images_device says holds unless named here: per-stream headers (hdrs, optional) and status[] filled on
 * every return, one bad stream does not fail the others, the device header check and its "header claims more than the stream
 * holds" rule, the same stream may be referenced several times, refused while a ticket is outstanding, FELICS_E_HIP on a failed
 * context, n = 0 returns FELICS_OK, the first non-zero status is returned.  offsets / lens / views / hdrs / status are HOST arrays.
 *   Checked before anything is launched (the first error in view order is returned and put in every status[i]):
 *     - every view as felics_view_extent checks it (enums, NULL data only for a zero-sized view, even addresses and strides at
 *       depth 16, an extent that fits 64 bits) -- without the encoder's size limits: the decoder's are those of the mixed call;
 *     - a written view must not alias itself.  Of the axes whose extent exceeds 1 (x: width, y: height, c: 3 for RGB), sorted by
 *       |stride| into a1 <= a2 <= a3, |stride(a1)| >= the sample size and |stride(a(k+1))| >= |stride(ak)| * extent(ak) must hold;
 *       anything else, zero strides included, is FELICS_E_INVALID_ARGUMENT (felics_view_writable gives the code without a context).
 *       The rule admits interleaved, BGR, RGBA, planar, bottom-up, crops and every-other-column views.  It is SUFFICIENT, NOT
 *       NECESSARY: some layouts whose samples do not share bytes (interleaved strides that are not nested) are refused.
 *   NOT checked, the caller's contract: the views of one call share no sample with each other, nor with the streams (the cells of a
 *   mosaic have interleaved hulls, so hulls cannot be compared).
 *   Per stream, after the headers are read: a valid header whose colour, depth, width or height differs from views[i] gets
 *   FELICS_E_INVALID_DIMENSIONS; nothing is written for that stream; hdrs[i] still receives the header the stream has.
 *   The write guarantee: the call stores SAMPLE BYTES ONLY.  It never writes the alpha byte of an RGBA pixel, the bytes between a
 *   row's end and the pitch, anything between the cells of a mosaic, or anything outside felics_view_extent's hull; no wide store
 *   covers a byte that is not a sample (unlike the encoder, which may READ pad bytes).  A stream that fails while decoding may leave
 *   any of its own view's samples written or unwritten, and nothing else.
 *   ready_event : a hipEvent_t the caller has recorded behind whatever produces the streams and last used the views, or NULL.  If
 *                 given, every stream of the library waits for it (hipStreamWaitEvent) before it first reads a stream byte or
 *                 writes a view in this call, the header kernel included, and the caller need not synchronise the host.  NULL keeps
 *                 the contract of felics_decompress_batch_device: the streams are complete in memory when the call is made.
 * How a view is written (felics_get_decode_view_stats counts them; the streams are counted in felics_decode_stats by form as well):
 *   dense     : the view is the layout the mixed call writes (a zero-sized view counts here); it takes that call's path as it is;
 *   in place  : nothing is staged -- RGB8 and RGB16 of ANY strides in every form (the decode kernels write Y / Co / Cg planes as
 *               for dense frames; the conversion kernel writes the view, sample by sample), and gray8 / gray16 with pixel_stride =
 *               the sample size and row_stride >= width * sample size (pitched surfaces, crops, mosaic cells: the kernels of both
 *               forms take the pitch);
 *   scattered : every other gray view (another pixel stride, a negative or short row stride) and every stream that goes to the host
 *               decoder (rows too wide for the LDS) is decoded to a dense frame in a staging buffer of the context; one kernel then
 *               writes its samples through the strides.  The staging is bounded: streams are taken in passes of consecutive
 *               streams whose frames fit a quarter of the free device memory (a single larger frame is a pass of its own).
 * The call is blocking: the views are complete when it returns.  It creates no HIP stream. */
int felics_decompress_views_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                   const felics_view *views, void *ready_event, felics_header *hdrs /* optional */, int *status);

/* Host only, no context: the code felics_decompress_views_device's checks give this view before anything is launched --
 * FELICS_OK, felics_view_extent's error, or FELICS_E_INVALID_ARGUMENT for strides that fail the nested rule above. */
int felics_view_writable(const felics_view *v);

/* How the views of a context's decode calls were written so far (cumulative). */
typedef struct felics_decode_view_stats {
    uint64_t views;         /* views handed to felics_decompress_views_device (calls that passed the checks) */
    uint64_t dense;         /* ... that were the dense layout (zero-sized ones included) */
    uint64_t in_place;      /* ... written where they lie */
    uint64_t scattered;     /* ... decoded to a staged dense frame and written by the scatter kernel */
    uint64_t bytes_staged;  /* bytes of the frames staged for scattered views whose stream was decoded */
} felics_decode_view_stats;
/* Writes min(out_size, sizeof(felics_decode_view_stats)) bytes, never more. */
int felics_get_decode_view_stats(const felics_ctx *ctx, felics_decode_view_stats *out, size_t out_size);

/* ---- Restart index: views and mixed shapes ----
 * felics_decompress_views_device through restart indexes: stream i (at d_streams + offsets[i], lens[i] bytes; any 8-bit stream, with
 * its own shape, colour, segment_pixels and K) has its index at d_index + idx_offsets[i], idx_lens[i] bytes long, and is decoded one
 * wave per (stream, plane, segment) straight into views[i]: k_decode8_seg_views, the walk of felics_decompress_batch_device_indexed
 * with a sink that writes through the view.  Every sample equals what felics_decompress yields for that stream.  A small image takes
 * part with the K = 1 index felics_index_build gives it; a stream without an index does not.
 * Everything felics_decompress_views_device says holds unless named here: per-stream headers (hdrs, optional: hdrs[i] gets the
 * stream's header where felics_read_header accepts it, zeros otherwise) and status[] filled on every return, one bad stream does not
 * fail the others, the same stream (and index) may be referenced several times, refused while a ticket is outstanding, FELICS_E_HIP on
 * a failed context, n = 0 returns FELICS_OK, the first non-zero status is returned.  offsets / lens / idx_offsets / idx_lens / views /
 * hdrs / status are HOST arrays.
 *   Checked before anything is launched (the first error in view order is returned and put in every status[i]): NULL pointers
 *   (FELICS_E_INVALID_ARGUMENT); every view as felics_view_writable checks it; d_index + idx_offsets[i] a multiple of 16
 *   (FELICS_E_INVALID_ARGUMENT: the kernel loads a checkpoint as aligned words); a call of 2^31 work items or more (the sum of
 *   C * max(K, 1) cannot be known yet: it is refused with FELICS_E_UNSUPPORTED in every status once the headers are read, before a
 *   stream is decoded).
 *   Per stream, in this order: the header codes of felics_read_header; the mixed call's "header claims more than the stream holds"
 *   rule (FELICS_E_IO; w * h >= 2^32: FELICS_E_INVALID_DIMENSIONS); FELICS_E_UNSUPPORTED for a 16-bit stream; FELICS_E_UNSUPPORTED for
 *   a row too wide for the wave form's LDS (no host fallback, as in the other indexed calls); FELICS_E_INVALID_DIMENSIONS for a header
 *   whose colour, depth, width or height differs from views[i] (nothing is written for that stream); FELICS_E_INVALID_INDEX if
 *   idx_lens[i] < 64, if the index header fails the checks above against the stream's header and length, or if idx_lens[i] is not the
 *   index's exact size (felics_index_size); then whatever the walk reports for the first failing segment in (plane, segment) order,
 *   all checks of "Restart index" made on the device.  A failing stream may leave any of its own view's samples written or unwritten,
 *   and nothing else.
 *   The write guarantee is felics_decompress_views_device's: SAMPLE BYTES ONLY.  Gray is stored sample by sample, one byte through all
 *   three strides -- negative strides and pixel strides other than 1 included, so NO gray view is staged, whatever its layout.  RGB is
 *   decoded as int16 Y / Co / Cg planes into the context's plane scratch (6 bytes per pixel) and the strided conversion of the
 *   unindexed call writes the view.  The scratch is bounded: streams are taken in passes of consecutive streams whose planes fit a
 *   quarter of the free device memory (what the context already holds counted as free); a single larger stream is a pass of its own.
 *   FELICS_TEST_INDEX_VIEWS_PASS=<bytes> in the environment (read per call) caps a pass's planes (tests).
 *   ready_event : as for felics_decompress_views_device.  If given, every stream of the library waits for it before the first byte of
 *                 a stream, an index or a view is touched in this call, the two header kernels included.
 * The stream headers and the first 64 bytes of every index are read by two kernels and come back in one synchronise; no header is
 * fetched with a blocking copy.  The call is blocking: the views are complete when it returns.  It creates no HIP stream.
 * NOT HERE: a lane-per-segment form, a queued form, streams without an index in the same call; 16-bit streams
 * (they have a call of their own: "Restart index: 16-bit streams into views and mixed shapes", below).
 * (Regions into views: "Restart index: regions into views and mixed shapes", below.)
 * (The encode side of this call is felics_compress_views_device_indexed, below.) */
int felics_decompress_views_device_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                           const void *d_index, const uint64_t *idx_offsets, const uint64_t *idx_lens,
                                           const felics_view *views, void *ready_event, felics_header *hdrs /* optional */, int *status);

/* Host only, the model of k_decode8_seg_views as felics_decompress_indexed is k_decode8_seg's: the same checks in the same order
 * (the per-stream list above), decoded segment by segment from the checkpoints alone, written through the view's strides into HOST
 * memory by the offset function the kernel's sink compiles (sample bytes only).  A view that is not felics_view_writable
 * (its code) or whose shape differs from the stream's (FELICS_E_INVALID_DIMENSIONS) is refused before a byte is written; an RGB
 * stream that fails leaves the view untouched, a gray one may have written the segments in front of the failing one.  hdr (optional)
 * gets the stream's header where felics_read_header accepts it. */
int felics_decompress_indexed_view(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_view *view,
                                   felics_header *hdr);

/* What a context's felics_decompress_views_device_indexed calls did so far (cumulative; calls that passed the checks before the
 * launch). */
typedef struct felics_index_view_stats {
    uint64_t streams;      /* streams handed in */
    uint64_t undecoded;    /* ... that got a code before a wave was launched for them */
    uint64_t items;        /* waves launched: C * max(K, 1) for every decoded stream */
    uint64_t launches;     /* k_decode8_seg_views launches (one per LDS class of a pass) */
    uint64_t passes;       /* passes (consecutive streams whose RGB planes share the scratch) */
    uint64_t plane_bytes;  /* NOT cumulative: the RGB scratch of the last call's largest pass */
} felics_index_view_stats;
/* Writes min(out_size, sizeof(felics_index_view_stats)) bytes, never more. */
int felics_get_index_view_stats(const felics_ctx *ctx, felics_index_view_stats *out, size_t out_size);

/* ---- Restart index: written while encoding views and mixed shapes ----
 * Host only, no device: where the indexes of n views go in one buffer.  segment_pixels[i] is view i's segment (a positive multiple of
 * FELICS_INDEX_GRANULE), or 0: no index for view i.  idx_lens[i] = felics_index_size of view i's shape and segment (0 for segment 0),
 * idx_offsets[i] = the running sum of the lengths before it, each rounded up to 16 (a view without an index gets the offset the next
 * index will get and does not advance it), *total = the end: the capacity felics_compress_views_device_indexed needs.  The first error
 * in view order: the view's own code where felics_view_extent refuses it, FELICS_E_INVALID_ARGUMENT for a non-zero segment that is
 * not a positive multiple of FELICS_INDEX_GRANULE (and for NULL arrays with n > 0), FELICS_E_UNSUPPORTED for a 16-bit view with a
 * non-zero segment (16-bit streams have no index). */
int felics_index_plan(size_t n, const felics_view *views, const uint32_t *segment_pixels, uint64_t *idx_offsets, uint64_t *idx_lens,
                      uint64_t *total);

/* felics_compress_views_device plus, for every view with segment_pixels[i] != 0, the restart index of stream i at
 * d_index + idx_offsets[i] (felics_index_size bytes): views of any shapes, colours, layouts and segments in one call.  The streams
 * are byte-identical to felics_compress_views_device's and every index to felics_index_build(stream i, segment_pixels[i]).
 * Everything felics_compress_views_device says holds: the classes of the views, slots and the exact second run (the indexes of the
 * run that places the streams are the ones that remain), the remedies of felics_stats, ready_event (d_index counts as d_out does:
 * nothing of it is touched before the event), refusal while a ticket is outstanding, zero-sized views (which get the 64-byte index
 * of an empty image, built on the host).  16-bit views and 8-bit views with segment_pixels[i] == 0 take part and get their streams
 * as ever.  segment_pixels and idx_offsets are HOST arrays of n entries (felics_index_plan fills idx_offsets; any other placement
 * that passes the checks will do); d_index may be NULL if no view asks for an index.
 * Checked before anything is launched, beside felics_compress_views_device's checks: segment_pixels by felics_index_plan's rules
 * (16-bit views included); d_index + idx_offsets[i] a multiple of 16 (FELICS_E_INVALID_ARGUMENT); every index inside d_index_cap
 * (FELICS_E_BUFFER_TOO_SMALL); no two indexes overlapping (FELICS_E_INVALID_ARGUMENT).  No byte of d_index outside the indexes' own
 * ranges is written.
 * How the indexes are written (felics_get_index_emit_stats counts them): the mixed sub-batches of the call compute everything an
 * index holds, and two kernels per sub-batch collect it for all its images (k_index_states_mixed, k_index_windows_mixed:
 * felics_index.hip), reading the windows where the views lie; a sub-batch that is redone by a remedy gets its indexes from the
 * writer of felics_compress_batch_device_indexed, one shape and segment at a time. */
int felics_compress_views_device_indexed(felics_ctx *ctx, size_t n, const felics_view *views, const uint32_t *segment_pixels,
                                         void *ready_event, void *d_out, size_t d_out_cap, void *d_index, size_t d_index_cap,
                                         const uint64_t *idx_offsets, uint64_t *offsets, uint64_t *lens);

/* What a context's felics_compress_views_device_indexed calls wrote so far (cumulative). */
typedef struct felics_index_emit_stats {
    uint64_t indexes;      /* indexes written by kernels (an index written again by a second run or a remedy counts again; the
                              host-built ones of zero-sized views do not count) */
    uint64_t checkpoints;  /* their checkpoints: the sum of C * K */
    uint64_t in_mixed;     /* indexes written by the mixed kernels */
    uint64_t redone;       /* indexes written by the uniform writer inside a remedy */
} felics_index_emit_stats;
/* Writes min(out_size, sizeof(felics_index_emit_stats)) bytes, never more. */
int felics_get_index_emit_stats(const felics_ctx *ctx, felics_index_emit_stats *out, size_t out_size);

/* ---- Restart index: 16-bit streams ----
 * The same idea for streams of 16-bit samples, in a format of its own (version 2) and through calls of their own; the calls above
 * keep refusing 16-bit input.  A 16-bit plane has up to 131 071 contexts of fifteen 32-bit counters: a dense state per checkpoint
 * would be 7.9 MB, and how many contexts are live depends on the content.  So a checkpoint's state is SPARSE -- one 64-byte row per
 * live context -- and the size of an index is not a function of the shape (felics_index16_size_max bounds it).
 *
 * Format (one blob per stream, little-endian, 64-byte aligned where a device call reads it).  segment_pixels and K as above; C planes.
 *   header, 64 bytes : "FLCX" | u16 version = 2 | u8 colour | u8 depth = 1 | u32 width | u32 height | u32 segment_pixels | u32 K |
 *                      u64 plane_end_bit[3] (as in version 1) | u64 total_bytes (of the whole index) | 8 reserved zero bytes
 *   directory, at 64 : C * K entries of 32 bytes in (plane, segment) order:
 *                      u64 bit_offset (as in version 1) | u64 rows_off | u32 n_rows | 12 reserved zero bytes
 *   windows          : from win_base = round_up(64 + 32 * C * K, 64); window (c, j) at win_base + (c * K + j) * win_bytes,
 *                      win_bytes = round_up(2 W * sb, 16): the plane's samples p0 - 2 W .. p0 - 1, zero in front of the plane;
 *                      sb = 2 (u16) for gray, 4 (i32) for Y / Co / Cg
 *   state rows       : from rows_base = round_up(win_base + C * K * win_bytes, 64); a row is u32 counter[15] | u32 context.
 *                      Checkpoint (c, j)'s rows are the n_rows rows at rows_off, contexts strictly ascending.  CANONICAL FORM: a
 *                      context has a row if and only if it has an out-of-range pixel in front of p0 (its counters are not zero)
 *                      and one at or behind p0 in that plane (its state is read again); segment 0 has none.  Rows are CHAINED in
 *                      (plane, segment) order: rows_off(0, 0) = rows_base, every other rows_off = the one before + 64 * n_rows,
 *                      and the last chain ends at total_bytes.  An empty image: K = 0, the header alone, total_bytes = 64.
 * Checks, the same on the host and on the GPU, in this order; any failure is FELICS_E_INVALID_INDEX: version 1's header checks
 * (version 2, depth 1); total_bytes = the length the caller gave (and >= rows_base); the reserved bytes are zero; version 1's
 * bit-offset rules; rows_off >= rows_base, a multiple of 64, rows_off + 64 * n_rows <= total_bytes and equal to its successor's
 * rows_off (total_bytes for the last entry); n_rows = 0 for j = 0; every context below 65 536 (gray, Y) or 131 071 (Co / Cg) and
 * above the one in front of it; every window sample in the plane's range (0..65535, Co / Cg -65535..65535); and the END CHECK.
 * WHAT THE CHECKS DO NOT PROVE: as above, and COUNTERS ARE NOT JUDGED: a forged counter gives a wrong Rice parameter in a segment
 * whose end check then fails (or whose pixels are wrong, as with an index of another stream); no address depends on a counter.
 * The encoder writes this index beside the streams of a blocking same-shape batch (felics_compress_batch_device_indexed16 below) and
 * of views and mixed shapes ("Restart index: 16-bit streams, written while encoding views and mixed shapes").
 * NOT HERE: the encoder's index in queued and host-buffer calls; a lane form and a queued form of the decoder;
 * a hashed table for small segments; cfelics / dfelics flags (--index keeps refusing 16-bit images).  (Regions are built: "Restart
 * index: regions of 16-bit streams", below; so are views and mixed shapes in the decoder: "Restart index: 16-bit streams into views
 * and mixed shapes".)
 * NAMES: the library's symbols hold no digit, like every other symbol of this ABI (its symbol check reads names as letters and
 * underscores), so the five functions are exported as felics_index_wide_size_max, felics_index_wide_build,
 * felics_decompress_indexed_wide, felics_decompress_batch_device_indexed_wide and felics_get_index_wide_stats ("wide" as in the 16-bit
 * encoder).  C and C++ callers may use the names felics_index16_size_max, felics_index16_build, felics_decompress_indexed16,
 * felics_decompress_batch_device_indexed16 and felics_get_index16_stats, inline aliases defined behind the declarations; a binding
 * that looks symbols up by name (ctypes, a Rust extern block) uses the exported ones.  The encoder's call and its counts follow the
 * same rule: felics_compress_batch_device_indexed_wide and felics_get_index_wide_emit_stats, with the aliases
 * felics_compress_batch_device_indexed16 and felics_get_index16_emit_stats. */

/* Host only: an upper bound of the size of the version-2 index of a w x h 16-bit image, for sizing buffers (checkpoint (c, j) has at
 * most min(p0 - 2, w * h - p0, contexts of plane c) rows); 0 for a bad colour, w * h >= 2^32 or a bad segment_pixels. */
size_t felics_index_wide_size_max(uint32_t w, uint32_t h, int color, uint32_t segment_pixels);

/* Host only: builds the version-2 index of ANY 16-bit stream by decoding it once on the CPU.  The two-call pattern of
 * felics_index_build: FELICS_E_BUFFER_TOO_SMALL with *index_len = the exact size.  FELICS_E_UNSUPPORTED for an 8-bit stream, the
 * stream's own decode error for a bad stream, FELICS_E_INVALID_ARGUMENT for a bad segment_pixels or bytes behind the last code. */
int felics_index_wide_build(const uint8_t *in, size_t len, uint32_t segment_pixels, uint8_t *index, size_t cap, size_t *index_len);

/* Host only: felics_decompress of a 16-bit stream through its index -- segment by segment, each from its checkpoint alone (the table
 * is exactly the checkpoint's rows, nothing is carried over).  The host model of k_decode16_seg.  pixels: uint16 samples,
 * pixels_cap in bytes.  FELICS_E_UNSUPPORTED for an 8-bit stream. */
int felics_decompress_indexed_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, void *pixels, size_t pixels_cap,
                                felics_header *hdr);

/* GPU: n 16-bit streams of ONE shape, colour, segment_pixels and K, each with its version-2 index (index i at
 * d_index + idx_offsets[i], idx_lens[i] bytes: the indexes differ in length; HOST arrays; d_index and every offset a multiple of 64,
 * else FELICS_E_INVALID_ARGUMENT), decoded a wave per (stream, plane, segment): k_decode16_seg.  Output layout and status conventions
 * of felics_decompress_batch_device; stream 0's header names the shape, index 0's header segment_pixels and K, and a stream whose own
 * headers differ gets FELICS_E_INVALID_DIMENSIONS or FELICS_E_INVALID_INDEX.  All checks above are made on the device; status[i] is
 * the code of stream i's first failing segment in (plane, segment) order.  A failing segment leaves only its own samples undefined;
 * an RGB frame with a failing segment is not converted.  Before anything is launched: FELICS_E_UNSUPPORTED in every status for an
 * 8-bit batch and for a row too wide for the kernel's LDS (no host fallback), FELICS_E_BUFFER_TOO_SMALL for a short d_pixels_cap;
 * refused while a ticket is outstanding.  Blocking; creates no HIP stream.
 * Every wave of a pass owns a dense estimator table (8.4 MB) in the buffer the unindexed 16-bit decoder uses, bounded as there (a
 * quarter of the free memory); a call whose waves do not fit runs in passes of consecutive (stream, plane, segment) items.
 * FELICS_TEST_INDEX16_PASS=k in the environment (read per call) caps a pass at k waves (tests). */
int felics_decompress_batch_device_indexed_wide(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                             const void *d_index, const uint64_t *idx_offsets, const uint64_t *idx_lens, void *d_pixels,
                                             size_t d_pixels_cap, felics_header *hdr, int *status);

/* What a context's felics_decompress_batch_device_indexed16 calls did so far (cumulative but table_bytes: the last call's). */
typedef struct felics_index16_stats {
    uint64_t streams;      /* streams handed to the call (calls that passed the checks made before a launch) */
    uint64_t segments16;   /* waves: the sum of n * C * max(K, 1) */
    uint64_t passes;       /* launches of k_decode16_seg */
    uint64_t rows_loaded;  /* state rows copied into tables */
    uint64_t table_bytes;  /* estimator tables of one pass of the last call */
} felics_index16_stats;
/* Writes min(out_size, sizeof(felics_index16_stats)) bytes, never more. */
int felics_get_index_wide_stats(const felics_ctx *ctx, felics_index16_stats *out, size_t out_size);

/* GPU: felics_compress_batch_device for depth = 16 (blocking, one shape, gray16 or RGB16; the call has no depth argument: 8-bit
 * frames go to felics_compress_batch_device_indexed, which keeps refusing 16-bit ones) that also WRITES THE VERSION-2 INDEX of every
 * stream, from what the encoder has in device memory anyway.  The streams are byte for byte felics_compress_batch_device's, placed as
 * that call places them (fixed slots, or back to back after a slot overflow); offsets / lens as there.
 * The indexes follow each other in stream order: index i at d_index + idx_offsets[i], idx_lens[i] bytes, idx_offsets[i] a multiple of 64
 * (d_index 64-byte aligned, else FELICS_E_INVALID_ARGUMENT), each byte for byte what felics_index16_build makes of stream i with the
 * same segment_pixels.  idx_offsets / idx_lens are HOST arrays, exactly what felics_decompress_batch_device_indexed16 takes.
 * The size of an index depends on the content (felics_index16_size_max is a bound far above it), so *idx_total (may be NULL) receives
 * the bytes all indexes need, and a d_index_cap below that is FELICS_E_BUFFER_TOO_SMALL: the streams, offsets and lens are then complete
 * and valid as after felics_compress_batch_device, idx_offsets / idx_lens / *idx_total say what is needed, the indexes whose end lies
 * inside d_index_cap are written and nothing is written behind d_index_cap; call again with *idx_total bytes.  (An error of the stream
 * part -- FELICS_E_BUFFER_TOO_SMALL for d_out among them, lens[0] = the bytes needed -- comes back as from felics_compress_batch_device,
 * with *idx_total = 0.)
 * Before anything is launched: FELICS_E_INVALID_ARGUMENT for a bad segment_pixels, a misaligned or NULL d_index, NULL arrays with
 * n > 0; refused while a ticket is outstanding; FELICS_E_UNSUPPORTED for an image whose per-checkpoint workspace (a bit per context
 * and checkpoint and the bits' prefix counts: 16 KB per gray checkpoint, 32 KB per RGB plane's) does not fit a quarter of the free
 * device memory.  That workspace also bounds the images of a pass; FELICS_TEST_PASS_IMAGES applies as in the unindexed call.
 * An empty image gets the 64-byte header alone (K = 0).
 * NOT HERE: a queued form of this call; host-buffer entry points; cfelics / dfelics --index for 16-bit files.  (Views and mixed shapes
 * have a call of their own: felics_compress_views_device_indexed16, below.) */
int felics_compress_batch_device_indexed_wide(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, void *d_out,
                                              size_t d_out_cap, uint32_t segment_pixels, void *d_index, size_t d_index_cap, uint64_t *offsets,
                                              uint64_t *lens, uint64_t *idx_offsets, uint64_t *idx_lens, uint64_t *idx_total);

/* What a context's felics_compress_batch_device_indexed16 calls wrote so far (cumulative; calls that returned FELICS_OK or
 * FELICS_E_BUFFER_TOO_SMALL for the index buffer). */
typedef struct felics_index16_emit_stats {
    uint64_t streams;       /* streams of those calls */
    uint64_t rows_written;  /* state rows of the indexes written: the sum of their directories' n_rows */
    uint64_t index_bytes;   /* bytes of the indexes written */
    uint64_t passes;        /* passes that wrote an index (a batch that is redone counts its last run) */
} felics_index16_emit_stats;
/* Writes min(out_size, sizeof(felics_index16_emit_stats)) bytes, never more. */
int felics_get_index_wide_emit_stats(const felics_ctx *ctx, felics_index16_emit_stats *out, size_t out_size);

/* The same under the names with "16" (see NAMES above): aliases, not symbols. */
static inline int felics_compress_batch_device_indexed16(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color,
                                                         void *d_out, size_t d_out_cap, uint32_t segment_pixels, void *d_index,
                                                         size_t d_index_cap, uint64_t *offsets, uint64_t *lens, uint64_t *idx_offsets,
                                                         uint64_t *idx_lens, uint64_t *idx_total) {
    return felics_compress_batch_device_indexed_wide(ctx, n, d_pixels, w, h, color, d_out, d_out_cap, segment_pixels, d_index, d_index_cap, offsets,
                                                     lens, idx_offsets, idx_lens, idx_total);
}
static inline int felics_get_index16_emit_stats(const felics_ctx *ctx, felics_index16_emit_stats *out, size_t out_size) {
    return felics_get_index_wide_emit_stats(ctx, out, out_size);
}
/* ... and the five above. */
static inline size_t felics_index16_size_max(uint32_t w, uint32_t h, int color, uint32_t segment_pixels) {
    return felics_index_wide_size_max(w, h, color, segment_pixels);
}
static inline int felics_index16_build(const uint8_t *in, size_t len, uint32_t segment_pixels, uint8_t *index, size_t cap, size_t *index_len) {
    return felics_index_wide_build(in, len, segment_pixels, index, cap, index_len);
}
static inline int felics_decompress_indexed16(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, void *pixels,
                                              size_t pixels_cap, felics_header *hdr) {
    return felics_decompress_indexed_wide(in, len, index, index_len, pixels, pixels_cap, hdr);
}
static inline int felics_decompress_batch_device_indexed16(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets,
                                                           const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                           const uint64_t *idx_lens, void *d_pixels, size_t d_pixels_cap, felics_header *hdr,
                                                           int *status) {
    return felics_decompress_batch_device_indexed_wide(ctx, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, d_pixels, d_pixels_cap, hdr,
                                                       status);
}
static inline int felics_get_index16_stats(const felics_ctx *ctx, felics_index16_stats *out, size_t out_size) {
    return felics_get_index_wide_stats(ctx, out, out_size);
}

/* ---- Restart index: regions of 16-bit streams ----
 * "Restart index: regions" for version-2 indexes: a window of a 16-bit stream decoded from the checkpoints of the segments that hold
 * its pixels and from nothing else.  The planner is felics_region_segments (its arithmetic knows no depth).  The 8-bit region calls
 * keep refusing 16-bit streams; these refuse 8-bit ones (FELICS_E_UNSUPPORTED).
 * NAMES: exported as felics_decompress_region_indexed_wide, felics_decompress_regions_device_indexed_wide and
 * felics_get_region_wide_stats; the aliases felics_decompress_region_indexed16, felics_decompress_regions_device_indexed16 and
 * felics_get_region16_stats follow the declarations.
 * NOT HERE: a lane form, a queued form; dfelics --region for 16-bit files.  (Regions into views and regions of mixed shapes:
 * "Restart index: regions into views and mixed shapes", below.) */

/* Host only: the w x h window *r of a 16-bit stream through its version-2 index, as dense uint16 samples (w * h * C of them;
 * pixels_cap in bytes).  The host model of k_decode16_region: every needed segment, in (plane, segment) order, from its checkpoint
 * alone -- the table is exactly the checkpoint's rows, nothing is carried from one segment to the next -- with the checks of
 * "Restart index: 16-bit streams" in that section's order: the stream header, the index header (for an empty region too), then per
 * needed segment its directory entry, its state rows, its window samples, the two raw samples (j = 0), the walk up to
 * min(segment end, the pixel behind the region's last one), every decoded sample in range, and the end check where the walk reaches
 * the segment's end.  The first failure is the code.  FELICS_E_UNSUPPORTED for an 8-bit stream, FELICS_E_INVALID_ARGUMENT for a
 * region outside the image, FELICS_E_BUFFER_TOO_SMALL for 2 * w * h * C > pixels_cap.  r->stream is ignored. */
int felics_decompress_region_indexed_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *r,
                                          void *pixels, size_t pixels_cap, felics_header *hdr);

/* GPU: felics_decompress_regions_device_indexed for 16-bit streams.  Streams, indexes and their alignment rules are
 * felics_decompress_batch_device_indexed_wide's (one shape, colour, segment_pixels and K; stream 0's header names the shape, index
 * 0's header the cut; d_index and every idx_offsets[i] multiples of 64); regions, crops, out_offsets (bytes, optional) and status
 * (n_regions words) are felics_decompress_regions_device_indexed's, the crops dense uint16 back to back in request order.  One wave
 * per (region, plane, needed segment): k_decode16_region, the walk of k_decode16_seg with a sink that stops behind the region's last
 * pixel and stores the samples inside the window.  status[r] is the code of region r's first failing item in (plane, segment) order,
 * after the header checks, which are made for empty regions too; a failing region leaves only its own crop undefined; an RGB crop
 * with a failing item is not converted.
 * Before anything is launched: FELICS_E_INVALID_ARGUMENT for a region outside the image, a stream number >= n_streams, a misaligned
 * index or a d_pixels that is not 2-byte aligned; FELICS_E_BUFFER_TOO_SMALL if the crops do not fit d_pixels_cap;
 * FELICS_E_UNSUPPORTED in every status for 8-bit streams and for rows too wide for the kernel's LDS (no host fallback); refused while
 * a ticket is outstanding.  Blocking; creates no HIP stream.
 * Every wave of a pass owns a dense estimator table as in felics_decompress_batch_device_indexed_wide, so the items run in passes
 * bounded the same way (FELICS_TEST_INDEX16_PASS applies); a pass boundary may fall inside a region.  RGB crops go through crop-sized
 * int32 planes (12 bytes per crop pixel), not frame-sized ones. */
int felics_decompress_regions_device_indexed_wide(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                  const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                  const uint64_t *idx_lens, size_t n_regions, const felics_region *regions, void *d_pixels,
                                                  size_t d_pixels_cap, uint64_t *out_offsets /* optional */, felics_header *hdr, int *status);

/* What a context's felics_decompress_regions_device_indexed16 calls did so far (cumulative; calls that passed the checks made before
 * a launch).  felics_region_stats and felics_index16_stats do not count these calls. */
typedef struct felics_region16_stats {
    uint64_t regions;           /* regions handed in */
    uint64_t segments_walked;   /* waves that walked a segment: C per needed segment */
    uint64_t segments_skipped;  /* C * K per region minus the walked */
    uint64_t pixels_walked;     /* pixels those walks cover */
    uint64_t rows_loaded;       /* state rows copied into tables */
    uint64_t passes;            /* launches of k_decode16_region */
} felics_region16_stats;
/* Writes min(out_size, sizeof(felics_region16_stats)) bytes, never more. */
int felics_get_region_wide_stats(const felics_ctx *ctx, felics_region16_stats *out, size_t out_size);

static inline int felics_decompress_region_indexed16(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len,
                                                     const felics_region *r, void *pixels, size_t pixels_cap, felics_header *hdr) {
    return felics_decompress_region_indexed_wide(in, len, index, index_len, r, pixels, pixels_cap, hdr);
}
static inline int felics_decompress_regions_device_indexed16(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                             const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                             const uint64_t *idx_lens, size_t n_regions, const felics_region *regions,
                                                             void *d_pixels, size_t d_pixels_cap, uint64_t *out_offsets, felics_header *hdr,
                                                             int *status) {
    return felics_decompress_regions_device_indexed_wide(ctx, n_streams, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, n_regions, regions,
                                                         d_pixels, d_pixels_cap, out_offsets, hdr, status);
}
static inline int felics_get_region16_stats(const felics_ctx *ctx, felics_region16_stats *out, size_t out_size) {
    return felics_get_region_wide_stats(ctx, out, out_size);
}

/* ---- Restart index: 16-bit streams into views and mixed shapes ----
 * "Restart index: views and mixed shapes" for version-2 indexes: stream i (at d_streams + offsets[i], lens[i] bytes; any 16-bit stream,
 * with its own shape, colour, segment_pixels and K) has its version-2 index at d_index + idx_offsets[i], idx_lens[i] bytes long, and is
 * decoded one wave per (stream, plane, segment) straight into views[i]: k_decode16_seg_views, the walk of
 * felics_decompress_batch_device_indexed16 with a sink that writes through the view.  Every sample equals what felics_decompress yields
 * for that stream.  A small image takes part with the K = 1 index felics_index16_build gives it.
 * The contract is felics_decompress_views_device_indexed's, word for word -- hdrs and status[] filled on every return, one bad stream
 * does not fail the others, the same stream (and index) may be referenced several times, refused while a ticket is outstanding,
 * FELICS_E_HIP on a failed context, n = 0 returns FELICS_OK, the first non-zero status is returned, the checks made before anything is
 * launched, ready_event, one synchronise for both kinds of headers, blocking, no HIP stream created -- except where a version-2 index
 * forces a difference:
 *   - d_index + idx_offsets[i] must be a multiple of 64, not 16 (FELICS_E_INVALID_ARGUMENT before anything is launched): the kernel
 *     loads a state row as one aligned 64-byte line.
 *   - views are 16-bit: felics_view_writable wants an even address and even strides.  A view of depth 8 passes that check and is then
 *     FELICS_E_INVALID_DIMENSIONS for its stream, nothing written.
 *   - FELICS_E_UNSUPPORTED is for an 8-BIT stream, and for a row whose 16-bit wave form does not fit the LDS (wider than 16 128).
 *   - FELICS_E_INVALID_INDEX: idx_lens[i] < 64, or the version-2 header fails its checks against the stream's own header, its length
 *     and idx_lens[i] (total_bytes must equal idx_lens[i]; the size of a version-2 index is no function of the shape).  Then whatever
 *     the walk reports for the first failing segment in (plane, segment) order: all checks of "Restart index: 16-bit streams" are
 *     made on the device.
 *   - The write guarantee, SAMPLE BYTES ONLY: gray is one aligned 2-byte store per sample through all strides -- negative strides and
 *     pixel strides other than 2 included, so no gray view is staged; RGB is decoded as int32 Y / Co / Cg planes (12 bytes per pixel)
 *     into the context's plane scratch and the strided conversion of the unindexed call writes the view.  A stream that fails leaves
 *     its RGB view unconverted; a failing gray stream may have written its own samples and nothing else.
 *   - TWO bounds, both met by running in passes on the one stream.  The RGB plane scratch, as in the 8-bit call: consecutive streams
 *     whose planes fit a quarter of the free device memory make a pass, a single larger stream is a pass of its own,
 *     FELICS_TEST_INDEX_VIEWS_PASS=<bytes> caps it.  And the estimator tables: every wave of a launch owns a dense table (8.4 MB) in
 *     the buffer the other 16-bit decoders use, every launch takes a fresh epoch, and a launch holds at most as many items as there
 *     are tables (bounded as in felics_decompress_batch_device_indexed16; FELICS_TEST_INDEX16_PASS=k caps it).  A table cut may fall
 *     inside a stream or a plane: an item needs its own table and nothing of its neighbours'.  The conversion of a stream pass runs
 *     behind its last launch.
 * NAMES: exported as felics_decompress_views_device_indexed_wide, felics_decompress_indexed_view_wide and
 * felics_get_index_view_wide_stats; the aliases felics_decompress_views_device_indexed16, felics_decompress_indexed16_view and
 * felics_get_index16_view_stats follow the declarations.
 * NOT HERE: a lane form, a queued form, 8-bit and 16-bit streams in one call, cfelics / dfelics flags.  (Regions into views:
 * "Restart index: regions into views and mixed shapes", below.) */
int felics_decompress_views_device_indexed_wide(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                                const void *d_index, const uint64_t *idx_offsets, const uint64_t *idx_lens,
                                                const felics_view *views, void *ready_event, felics_header *hdrs /* optional */, int *status);

/* Host only, the model of k_decode16_seg_views as felics_decompress_indexed_view is k_decode8_seg_views': the per-stream checks above
 * in the same order, decoded segment by segment from the checkpoints alone (felics_decompress_indexed16's walk), written through the
 * view's strides into HOST memory by the offset function the kernel's sink compiles (sample bytes only).  A view that is not
 * felics_view_writable (its code) or whose shape differs from the stream's (FELICS_E_INVALID_DIMENSIONS) is refused before a byte is
 * written; an RGB stream that fails leaves the view untouched, a gray one may have written the segments in front of the failing one.
 * hdr (optional) gets the stream's header where felics_read_header accepts it. */
int felics_decompress_indexed_view_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_view *view,
                                        felics_header *hdr);

/* What a context's felics_decompress_views_device_indexed16 calls did so far (calls that passed the checks before the launch).
 * felics_index_view_stats and felics_index16_stats do not count these calls. */
typedef struct felics_index16_view_stats {
    uint64_t streams;      /* streams handed in */
    uint64_t undecoded;    /* ... that got a code before a wave was launched for them */
    uint64_t items;        /* waves launched: C * max(K, 1) for every decoded stream */
    uint64_t launches;     /* k_decode16_seg_views launches (per pass and LDS class, cut by the tables) */
    uint64_t passes;       /* stream passes (consecutive streams whose RGB planes share the scratch) */
    uint64_t rows_loaded;  /* state rows copied into tables */
    uint64_t plane_bytes;  /* NOT cumulative: the RGB scratch of the last call's largest pass */
    uint64_t table_bytes;  /* NOT cumulative: the estimator tables of the last call */
} felics_index16_view_stats;
/* Writes min(out_size, sizeof(felics_index16_view_stats)) bytes, never more. */
int felics_get_index_view_wide_stats(const felics_ctx *ctx, felics_index16_view_stats *out, size_t out_size);

static inline int felics_decompress_views_device_indexed16(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets,
                                                           const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                           const uint64_t *idx_lens, const felics_view *views, void *ready_event,
                                                           felics_header *hdrs, int *status) {
    return felics_decompress_views_device_indexed_wide(ctx, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, ready_event, hdrs,
                                                       status);
}
static inline int felics_decompress_indexed16_view(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_view *view,
                                                   felics_header *hdr) {
    return felics_decompress_indexed_view_wide(in, len, index, index_len, view, hdr);
}
static inline int felics_get_index16_view_stats(const felics_ctx *ctx, felics_index16_view_stats *out, size_t out_size) {
    return felics_get_index_view_wide_stats(ctx, out, out_size);
}

/* ---- Restart index: regions into views and mixed shapes ----
 * The region calls and the views calls in one: a window of every stream, the streams of any shapes, decoded straight into views.
 * Stream s (at d_streams + offsets[s], lens[s] bytes) is any 8-bit stream (_wide: any 16-bit stream) with its own shape, colour,
 * segment_pixels and K; its index is addressed as in felics_decompress_views_device_indexed (_wide: _indexed16): d_index +
 * idx_offsets[s], idx_lens[s] bytes, the address a multiple of 16 (_wide: of 64).  Region r is the window regions[r].{x, y, w, h} of
 * stream regions[r].stream; several regions may name one stream, a stream may go unnamed.  The window is decoded straight into
 * views[r]: window sample (i, j, c), that is image pixel (x + i, y + j), lands at data + j * row_stride + i * pixel_stride +
 * c * channel_stride.  Every sample is the one felics_decompress yields at its place.
 * One wave per (region, plane, needed segment): k_decode8_region_views / k_decode16_region_views, the walk of the region kernels with
 * a sink that writes through the view.  The needed segments are those felics_region_segments names for the stream's own W, H and
 * segment_pixels; each is walked up to `stop` as "Restart index: regions" defines it.
 * WHAT THE CHECKS COVER is exactly what "Restart index: regions" says: the checks of "Restart index" (_wide: of "Restart index: 16-bit
 * streams") for the NEEDED segments only, with no end check where a walk stops early.  A segment no region needs is not looked at: a
 * forged entry there goes unnoticed, as in the region calls.
 * offsets / lens / idx_offsets / idx_lens / regions / views / hdrs / status are HOST arrays; status has n_regions words, hdrs
 * (optional) n_streams headers.  status[] is filled on every return and the first non-zero status in region order is returned.
 *   Checked before anything is launched (the first error in region order is returned and put in every status[r]): NULL pointers;
 *   n_regions > 2^31 - 1, or n_streams == 0 with regions (FELICS_E_INVALID_ARGUMENT); regions[r].stream >= n_streams
 *   (FELICS_E_INVALID_ARGUMENT); views[r] refused by felics_view_writable (its code); views[r].width != regions[r].w or
 *   views[r].height != regions[r].h (FELICS_E_INVALID_ARGUMENT); then the index alignment rule for every stream
 *   (FELICS_E_INVALID_ARGUMENT).  Refused while a ticket is outstanding (FELICS_E_INVALID_ARGUMENT); FELICS_E_HIP on a failed
 *   context; n_regions == 0 returns FELICS_OK.
 *   Per stream, after the headers are read (the stream headers and the first 64 bytes of every index come back from the two header
 *   kernels of the views calls in one synchronise): the per-stream codes of felics_decompress_views_device_indexed (_wide: of
 *   _indexed16) in that call's order, except that a header is compared with a view per region (below).  hdrs[s] is filled as there.
 *   Per region, in this order: its stream's code; FELICS_E_INVALID_ARGUMENT for a window outside that stream's image (x + w and y + h
 *   as 64-bit sums); FELICS_E_INVALID_DIMENSIONS if views[r]'s colour or depth differs from the stream's; the code of its first
 *   failing item in (plane, segment) order; FELICS_E_INVALID_VALUE from the RGB conversion.
 *   A region that gets a code before the launch writes nothing.  A region that fails while decoding may leave any of its own view's
 *   samples written or unwritten, and nothing else; an RGB region with a failing item is not converted.  One bad stream or region
 *   does not fail the others.  An empty region (w = 0 or h = 0, with a zero-sized view) gets its stream's header and index-header
 *   code, then the two per-region checks above like any other region (an empty window must still lie inside the image, its view
 *   must still have the stream's colour and depth), and launches no walk.  FELICS_E_UNSUPPORTED in every status for 2^31 work items or more, once the headers are known.
 *   The write guarantee is the views calls', word for word: SAMPLE BYTES ONLY.  Gray is one aligned store of one sample through all
 *   strides, so NO gray view is staged, whatever its layout.  RGB goes through CROP-SIZED Y / Co / Cg planes in the context's plane
 *   scratch (6 bytes per crop pixel; _wide: 12) and the strided conversion of the unindexed call writes the view.
 *   ready_event: as in the views calls.  Nothing of a stream, an index or a view is touched before it, the header kernels included.
 *   The call is blocking and creates no HIP stream.  The views of one call share no sample with each other or with the streams: the
 *   caller's contract.
 *   Passes: consecutive regions whose RGB planes fit a quarter of the free device memory make a pass, a single larger region is a
 *   pass of its own; FELICS_TEST_INDEX_VIEWS_PASS=<bytes> caps it.  Within a pass the items run in the LDS classes of the views
 *   calls, a launch per class.  _wide: a launch holds at most as many items as there are estimator tables, with a fresh epoch per
 *   launch (FELICS_TEST_INDEX16_PASS=k caps it); a table cut may fall inside a region or a plane.
 * NAMES: the 16-bit forms are exported as felics_decompress_region_views_device_indexed_wide,
 * felics_decompress_region_indexed_view_wide and felics_get_region_view_wide_stats; the aliases
 * felics_decompress_region_views_device_indexed16, felics_decompress_region_indexed16_view and felics_get_region16_view_stats follow
 * the declarations.
 * NOT HERE: a lane form, a queued form, regions of streams without an index, 8-bit and 16-bit streams in one call, dfelics flags. */
int felics_decompress_region_views_device_indexed(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                  const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                  const uint64_t *idx_lens, size_t n_regions, const felics_region *regions,
                                                  const felics_view *views, void *ready_event, felics_header *hdrs /* optional, n_streams */,
                                                  int *status /* n_regions */);
int felics_decompress_region_views_device_indexed_wide(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                       const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                       const uint64_t *idx_lens, size_t n_regions, const felics_region *regions,
                                                       const felics_view *views, void *ready_event,
                                                       felics_header *hdrs /* optional, n_streams */, int *status /* n_regions */);

/* Host only, the models of k_decode8_region_views and k_decode16_region_views: the checks of the device call for one stream and one
 * region in its order -- the view writable (its code), the view w x h (FELICS_E_INVALID_ARGUMENT), the per-stream codes, the window
 * inside the image (FELICS_E_INVALID_ARGUMENT), the view's colour and depth the stream's (FELICS_E_INVALID_DIMENSIONS), all before a
 * byte is written --, then the needed segments from their checkpoints alone (the walk of felics_decompress_region_indexed /
 * _indexed16), written through the view's strides into HOST memory by the offset function the kernel's sink compiles (sample bytes
 * only).  A failing RGB region leaves the view untouched; a failing gray one may have written samples of its own window.
 * r->stream is ignored.  hdr (optional) gets the stream's header where felics_read_header accepts it. */
int felics_decompress_region_indexed_view(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *r,
                                          const felics_view *view, felics_header *hdr);
int felics_decompress_region_indexed_view_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *r,
                                               const felics_view *view, felics_header *hdr);

/* What a context's felics_decompress_region_views_device_indexed calls did so far (cumulative; calls that passed the checks made
 * before a launch).  The other region and view counters do not count these calls. */
typedef struct felics_region_view_stats {
    uint64_t regions;           /* regions handed in */
    uint64_t undecoded;         /* ... that got a code before a wave was launched for them */
    uint64_t segments_walked;   /* waves launched: C per needed segment of a decoded region */
    uint64_t segments_skipped;  /* C * K per decoded region minus the walked */
    uint64_t pixels_walked;     /* pixels those walks cover */
    uint64_t launches;          /* k_decode8_region_views launches (one per LDS class of a pass) */
    uint64_t passes;            /* passes (consecutive regions whose RGB planes share the scratch) */
    uint64_t plane_bytes;       /* NOT cumulative: the RGB scratch of the last call's largest pass */
} felics_region_view_stats;
/* Writes min(out_size, sizeof(felics_region_view_stats)) bytes, never more. */
int felics_get_region_view_stats(const felics_ctx *ctx, felics_region_view_stats *out, size_t out_size);

/* The same for felics_decompress_region_views_device_indexed16 (launches: per pass and LDS class, cut by the tables). */
typedef struct felics_region16_view_stats {
    uint64_t regions;
    uint64_t undecoded;
    uint64_t segments_walked;
    uint64_t segments_skipped;
    uint64_t pixels_walked;
    uint64_t launches;
    uint64_t passes;
    uint64_t plane_bytes;  /* NOT cumulative */
    uint64_t rows_loaded;  /* state rows copied into tables */
    uint64_t table_bytes;  /* NOT cumulative: the estimator tables of the last call */
} felics_region16_view_stats;
/* Writes min(out_size, sizeof(felics_region16_view_stats)) bytes, never more. */
int felics_get_region_view_wide_stats(const felics_ctx *ctx, felics_region16_view_stats *out, size_t out_size);

static inline int felics_decompress_region_views_device_indexed16(felics_ctx *ctx, size_t n_streams, const void *d_streams,
                                                                  const uint64_t *offsets, const uint64_t *lens, const void *d_index,
                                                                  const uint64_t *idx_offsets, const uint64_t *idx_lens, size_t n_regions,
                                                                  const felics_region *regions, const felics_view *views, void *ready_event,
                                                                  felics_header *hdrs, int *status) {
    return felics_decompress_region_views_device_indexed_wide(ctx, n_streams, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, n_regions,
                                                              regions, views, ready_event, hdrs, status);
}
static inline int felics_decompress_region_indexed16_view(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len,
                                                          const felics_region *r, const felics_view *view, felics_header *hdr) {
    return felics_decompress_region_indexed_view_wide(in, len, index, index_len, r, view, hdr);
}
static inline int felics_get_region16_view_stats(const felics_ctx *ctx, felics_region16_view_stats *out, size_t out_size) {
    return felics_get_region_view_wide_stats(ctx, out, out_size);
}

/* ---- Restart index: 16-bit streams, written while encoding views and mixed shapes ----
 * felics_compress_views_device that also WRITES THE VERSION-2 INDEX of every 16-bit view i with segment_pixels[i] != 0 -- the encode
 * side of felics_decompress_views_device_indexed16, which takes this call's buffers and arrays as they come back.  Views of any mix
 * of shapes, colours and segments in one call; the streams are byte for byte felics_compress_views_device's and placed as that call
 * places them, every index is byte for byte what felics_index16_build makes of stream i with segment_pixels[i].
 * Everything felics_compress_views_device says holds unless named here: the view checks and the first error in view order before
 * anything is launched, the classes (every 16-bit view is gathered), slots or the exact second run, FELICS_E_BUFFER_TOO_SMALL with
 * lens[0] for d_out, ready_event (d_index counts as d_out does), refused while a ticket is outstanding, n = 0 returns FELICS_OK,
 * FELICS_E_HIP on a failed context.
 *   PLACEMENT: the size of a version-2 index depends on the content, so the LIBRARY places the indexes and there is no host planner:
 *   idx_offsets / idx_lens are HOST arrays the call fills, *idx_total (may be NULL) the bytes all indexes need.  Every offset is a
 *   multiple of 64 (d_index must be 64-byte aligned, else FELICS_E_INVALID_ARGUMENT); the ranges are disjoint and tile
 *   [0, *idx_total) without gaps; their ORDER IS UNSPECIFIED (it is the order in which the call's sub-batches land, not view order).
 *   A view without an index gets idx_lens[i] = idx_offsets[i] = 0.  A zero-sized view that asks for one gets the 64-byte version-2
 *   header, built on the host and placed like the others.  d_index may be NULL if no view asks for an index.
 *   A SHORT d_index_cap is FELICS_E_BUFFER_TOO_SMALL as in felics_compress_batch_device_indexed16: the streams, offsets and lens are
 *   complete and valid, idx_offsets / idx_lens / *idx_total say what is needed, the indexes whose end lies inside d_index_cap are
 *   written, the others are not begun and nothing behind d_index_cap is written; a second call with *idx_total bytes succeeds.  An
 *   error of the stream part comes back as from felics_compress_views_device, with *idx_total = 0.
 *   Checked before anything is launched, per view in view order behind the view's own checks: segment_pixels[i] != 0 that is not a
 *   multiple of FELICS_INDEX_GRANULE (FELICS_E_INVALID_ARGUMENT); an 8-bit view with a segment (FELICS_E_UNSUPPORTED: its call is
 *   felics_compress_views_device_indexed; 8-bit views with segment 0 take part and get their streams).  Then NULL arrays with n > 0,
 *   a NULL d_index with an index asked for, a misaligned d_index (FELICS_E_INVALID_ARGUMENT), and an image whose own checkpoints do
 *   not fit the workspace budget of felics_compress_batch_device_indexed16 (FELICS_E_UNSUPPORTED): a quarter of the free device memory
 *   plus what the context already holds for this.
 * The per-checkpoint workspace (16 KB per gray checkpoint, 32 KB per RGB plane's, in the workspace of the lane the sub-batch ran on)
 * also bounds a sub-batch: when indexes are asked for, a pass of a bucket is cut so that its checkpoints fit the budget; a call
 * without indexes is cut exactly as felics_compress_views_device cuts it.  FELICS_TEST_INDEX16_EMIT_CPS=k in the environment (read
 * per call) caps a sub-batch at k checkpoints, at least one image per sub-batch (tests).
 * A sub-batch's indexes are written where it lands, by the table-driven kernels (k_wide_index_*_t: K, segment, shape and samples per
 * plane); a group redone after a slot overflow gets them from the uniform writer of felics_compress_batch_device_indexed16.  A run
 * for the sizes alone (d_out cannot hold the slots) writes no index: the run that places the streams writes them.
 * NAMES: exported as felics_compress_views_device_indexed_wide and felics_get_index_view_wide_emit_stats; the aliases
 * felics_compress_views_device_indexed16 and felics_get_index16_view_emit_stats follow the declarations.
 * NOT HERE: a queued (ticketed) form; felics_submit_surfaces_device with an index; host-buffer entry points; cfelics / dfelics flags;
 * 8-bit and 16-bit indexes from one call. */
int felics_compress_views_device_indexed_wide(felics_ctx *ctx, size_t n, const felics_view *views, const uint32_t *segment_pixels,
                                              void *ready_event, void *d_out, size_t d_out_cap, void *d_index, size_t d_index_cap,
                                              uint64_t *offsets, uint64_t *lens, uint64_t *idx_offsets, uint64_t *idx_lens, uint64_t *idx_total);

/* What a context's felics_compress_views_device_indexed16 calls wrote so far (cumulative but shapes_max; calls that returned FELICS_OK
 * or FELICS_E_BUFFER_TOO_SMALL for the index buffer).  felics_index16_emit_stats does not count these calls. */
typedef struct felics_index16_view_emit_stats {
    uint64_t views;         /* views of those calls */
    uint64_t indexes;       /* indexes written by a kernel (one that is written again counts again; host-built empty ones do not) */
    uint64_t rows_written;  /* state rows of those indexes: the sum of their directories' n_rows */
    uint64_t index_bytes;   /* bytes of the indexes written, the empty ones' headers included */
    uint64_t sub_batches;   /* sub-batches whose indexes the table-driven writer wrote */
    uint64_t shapes_max;    /* NOT cumulative: the distinct shapes of the last call's most mixed such sub-batch */
    uint64_t redone;        /* indexes written by the uniform writer inside a remedy */
} felics_index16_view_emit_stats;
/* Writes min(out_size, sizeof(felics_index16_view_emit_stats)) bytes, never more. */
int felics_get_index_view_wide_emit_stats(const felics_ctx *ctx, felics_index16_view_emit_stats *out, size_t out_size);

static inline int felics_compress_views_device_indexed16(felics_ctx *ctx, size_t n, const felics_view *views, const uint32_t *segment_pixels,
                                                         void *ready_event, void *d_out, size_t d_out_cap, void *d_index, size_t d_index_cap,
                                                         uint64_t *offsets, uint64_t *lens, uint64_t *idx_offsets, uint64_t *idx_lens,
                                                         uint64_t *idx_total) {
    return felics_compress_views_device_indexed_wide(ctx, n, views, segment_pixels, ready_event, d_out, d_out_cap, d_index, d_index_cap, offsets,
                                                     lens, idx_offsets, idx_lens, idx_total);
}
static inline int felics_get_index16_view_emit_stats(const felics_ctx *ctx, felics_index16_view_emit_stats *out, size_t out_size) {
    return felics_get_index_view_wide_emit_stats(ctx, out, out_size);
}

/* Text for a code above; for FELICS_E_HIP felics_last_error(ctx) has the HIP message. */
const char *felics_strerror(int code);
const char *felics_last_error(const felics_ctx *ctx);

/* What has happened to a context that the return codes do not say: how often it had to redo a batch, and
 * whether it is on a slower path or unusable.  (A look-back / hand-off that gives up -- e.g. another process
 * holding the GPU for a second -- moves the context to the two-pass kernels for good; felics_last_error says so.) */
typedef struct felics_stats {
    uint64_t submissions;        /* sub-batches queued so far */
    uint64_t ticket_retries;     /* 0 or 1: a look-back gave up and the context now hands its pack tiles out by ticket (first remedy) */
    uint64_t slot_overflows;     /* batches redone with exact placement: a stream outgrew its fixed slot */
    uint64_t lookback_fallbacks; /* batches redone because a tile gave up waiting for its predecessors */
    int two_pass;                /* 1: a ticketed look-back gave up as well: the context packs with the two-pass kernels from now on (slower) */
    int failed;                  /* 1: a wait for the GPU timed out; every further call returns FELICS_E_HIP */
    uint64_t scatter_fallbacks;  /* sub-batches redone because the front kernel's check of its own event order failed (with submissions in flight each
                                    reports its own, so 0 .. lanes); the context ranks events with ballots from then on (slower, no assumption about the LDS) */
    uint64_t sorted_event_sorts; /* sub-batches of 8-bit samples whose events were ranked with returning LDS atomics (the default), not with ballots */
    uint64_t tile_overflows;     /* sub-batches redone because a tile's events outgrew the slots a tile gets by default; the context sizes its tiles for the
                                    worst case from then on (more memory, same kernels) */
} felics_stats;
int felics_get_stats(const felics_ctx *ctx, felics_stats *out);

/* ---- measurement hooks (bench.py) ----
 * With profiling on, every kernel launch of the next submission gets a start / stop HIP event on the
 * stream it runs on (the kernel's own begin / end for single-kernel stages, event records around the
 * launches of the few stages that are several small kernels).  A submission launches most kernels once per slice of the image (the stages
 * follow each other slice by slice on several streams); felics_get_stage_ms gives, per stage, the SUM
 * of its launches' durations in milliseconds (launches of different stages overlap, so the stages add
 * up to more than the wall time), felics_get_stage_launches how many launches that was. */
#define FELICS_MAX_STAGES 16
int felics_set_profiling(felics_ctx *ctx, int enabled);
int felics_stage_count(void);
const char *felics_stage_name(int stage);
int felics_get_stage_ms(const felics_ctx *ctx, float *ms, int cap);
int felics_get_stage_launches(const felics_ctx *ctx, int *launches, int cap);
/* The same submission from its first kernel to its last byte (stream sizes on the host): one HIP event in front of the first
 * launch, one behind the size copy, on the streams they run on -- BASELINE.md section 2's per-step span. */
int felics_get_span_ms(const felics_ctx *ctx, float *ms);
/* Submissions that can be in flight at a time (felics_submit_batch_device): felics_ctx_lane_count for an existing context
 * (fixed when it was created), felics_lane_count for a context created now (2 unless FELICS_LANES says otherwise). */
int felics_lane_count(void);
int felics_ctx_lane_count(const felics_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* FELICS_H */
