/*
 * brotli_amd -- MI355X (gfx950) Brotli encode/decode engine: the C ABI.
 *
 * This is the drop-in boundary for countertype/brotli-lib's public surface
 * (package.json:7-23 exports `.`, `./encode`, `./decode`):
 *
 *   brotliEncode(input, {quality, lgwin, mode, sizeHint})  src/encode/encode.ts:22-27,50-90  -> mib_encode
 *   new BrotliEncoder(opts).update(chunk) / .finish()      src/encode/encode.ts:290-409      -> mib_encoder_*
 *   brotliDecode(data, {maxOutputSize, customDictionary} | outputSize)
 *                                                          src/decode/decode.ts:13-65        -> mib_decode
 *   brotliDecodedSize(data)                                src/decode/decode.ts:9-11         -> mib_decoded_size
 *   new BrotliDecoder(opts).update(chunk) / .finish()      (extension: streaming decode)     -> mib_decoder_*
 *   brotliDecoderUpdateBatch(decoders, chunks) / brotliDecoderFinishBatch(decoders)
 *                                                          (extension: many sessions a launch) -> mib_decoder_*_batch
 *   (C and Python only: the same with chunks and output in device memory)                        -> mib_decoder_*_batch_device
 *   EncoderMode {GENERIC 0, TEXT 1, FONT 2}                src/encode/enc-constants.ts:56-60 -> MIB_MODE_*
 *
 * plus batch entry points (host or device-resident buffers) that shard independent buffers
 * over the GPU.  Every call is synchronous.  The host-buffer entry points
 * share one default context and are serialised internally (safe from several threads); a
 * mib_ctx / mib_encoder / mib_decoder handle must not be used by two threads at once.
 * All compute runs on the GPU: there is no CPU fallback, a missing device is an error.
 *
 * Return codes: 0 = success; the reference decoder's own negative codes (-1..-30,
 * engine.ts makeError sites) so a host shim can throw the identical
 * "Brotli error code: N"; MIB_E_* (<= -100) for conditions of this engine.
 */
#ifndef BROTLI_AMD_H_
#define BROTLI_AMD_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MIB_MODE_GENERIC 0
#define MIB_MODE_TEXT 1
#define MIB_MODE_FONT 2

#define MIB_E_NO_DEVICE (-100)      /* no usable gfx950 device / HIP runtime error */
#define MIB_E_INVALID_ARG (-101)
#define MIB_E_OUT_OF_MEMORY (-102)
#define MIB_E_OUTPUT_LIMIT (-103)   /* decoded size exceeds maxOutputSize (decode.ts:46-62) */
#define MIB_E_NEED_SPACE (-104)     /* device buffer too small (batch/device APIs) */
#define MIB_E_JS_RANGE_ERROR (-105) /* the reference would throw a JS RangeError here */
#define MIB_E_JS_TYPE_ERROR (-106)  /* the reference would throw a JS TypeError here */
#define MIB_E_NO_PROGRESS (-107)    /* decoder iteration guard tripped (never on valid input) */

typedef struct {
  int quality;        /* 0..11, default 11 (clamped like encode.ts:57-62) */
  int lgwin;          /* 10..24, default 22 */
  int mode;           /* MIB_MODE_* */
  uint64_t size_hint; /* accepted, no effect (as in the reference) */
  /* customDictionary (extension: the reference's BrotliEncodeOptions, encode.ts:22-27, has
   * none; this is the encoder side of brotliDecode's customDictionary, decode.ts:13-35).
   * Copies into it are addressed the way the reference decoder resolves a compound
   * dictionary (engine.ts:142-159,903-1011): distance > max distance.  That decoder only
   * accepts a copy that ends exactly at the dictionary's last byte, so the encoder only
   * emits such copies; the stream then decodes with the same dictionary, and only with it.
   * Host memory, borrowed for the call (BrotliEncoder keeps its own copy). NULL: none. */
  const uint8_t *dict;
  uint64_t dict_len;
  /* BrotliEncoder only (extension): 0 = the reference's cadence (encode.ts:366-374: every
   * update() encodes each complete 2^lgblock block it has and returns its bytes); N > 0 =
   * throughput mode: input gathers until at least N bytes (whole blocks) are pending, and the
   * device encode then grows with the stream (up to 256 MiB) -- update() may return nothing
   * for a while and finish() returns the rest. */
  uint64_t stream_chunk;
} mib_enc_opts;

typedef struct { uint8_t *data; size_t size; } mib_buf;          /* library-allocated result */
typedef struct { const uint8_t *data; size_t size; } mib_span;   /* borrowed input */

/* defaults of createDefaultParams (enc-constants.ts:209-233) */
void mib_enc_opts_default(mib_enc_opts *o);

/* Select the device (default 0) and warm the engine up; optional. */
int mib_init(int device);
/* Human-readable message for a return code ("Brotli error code: N" for the reference's codes). */
const char *mib_strerror(int code);

/* brotliEncode (encode.ts:50-90). */
int mib_encode(const uint8_t *in, size_t n, const mib_enc_opts *o, mib_buf *out);

/* brotliDecode (decode.ts:18-65).  exact_out >= 0: the legacy numeric `outputSize`
 * signature (truncate / zero-pad to it); -1: none.  max_out: `maxOutputSize`, -1 = none.
 * dict: `customDictionary` (compound-dictionary semantics, engine.ts:142-159), may be NULL.
 * On MIB_E_OUTPUT_LIMIT no data is returned and out->size holds the size that exceeded
 * the limit (the header's size before decoding, the decoded length after). */
int mib_decode(const uint8_t *in, size_t n, const uint8_t *dict, size_t dict_n, int64_t max_out,
               int64_t exact_out, mib_buf *out);

/* brotliDecodedSize (decode.ts:9-11 -> engine.ts:2155-2192): -1 when unknown. */
int64_t mib_decoded_size(const uint8_t *in, size_t n);

/* BrotliEncoder (encode.ts:290-490): update() returns the newly completed bytes.  The
 * encoder keeps its 2^lgwin window of history in HBM, so matches reach across update()
 * calls; input is encoded in whole 2^lgblock blocks: by default each update() encodes the
 * complete blocks it has (the reference's cadence), with mib_enc_opts.stream_chunk several
 * MiB per device pass (throughput mode). */
typedef struct mib_encoder mib_encoder;
mib_encoder *mib_encoder_new(const mib_enc_opts *o);
int mib_encoder_update(mib_encoder *e, const uint8_t *in, size_t n, mib_buf *out);
int mib_encoder_finish(mib_encoder *e, mib_buf *out);
void mib_encoder_free(mib_encoder *e);
/* k independent encoders (distinct handles) advance by one chunk each in one launch sequence
 * (encoders with equal options share it); out[i] is encoder i's update() result. */
int mib_encoder_update_batch(mib_encoder *const *e, const mib_span *in, size_t k, mib_buf *out);

/* BrotliDecoder (extension: the reference decodes in one shot only, decode.ts:18-65; this is
 * the decode side of BrotliEncoder, in the shape of Node's zlib.BrotliDecompress and of
 * google/brotli's BrotliDecoderDecompressStream).  update() takes the next bytes of one
 * stream, cut anywhere, and returns the bytes they complete (the last few KiB of them may
 * come with the next call; the update() that brings the stream's last byte returns all that
 * is left); finish() declares the input ended and returns the rest, or the reference
 * decoder's error for an incomplete stream (-13, -16, -17 ...).  The decoder keeps the last 2^lgwin bytes of output, the input it may read
 * again and its state at the last command boundary in HBM, so neither the
 * compressed nor the decoded stream is ever held whole and its length has no limit.
 * Bytes behind the stream's end are an error (-17), in the update() that brings them or in
 * any later one; after an error every call returns that code again.  Output is that of
 * brotliDecode without a size (no truncation or padding to a header's size).
 *   dict / dict_len  customDictionary (host memory, copied by mib_decoder_new); NULL: none
 *   max_out          limit on the total output, -1 none: MIB_E_OUTPUT_LIMIT once passed
 *                    (no data; out->size holds the total decoded by then)
 *   out_window       output bytes per device pass, 0 = default (16 MiB); clamped to
 *                    64 KiB .. 512 MiB.  Smaller: less memory, more passes. */
typedef struct {
  const uint8_t *dict;
  uint64_t dict_len;
  int64_t max_out;
  uint64_t out_window;
} mib_dec_opts;
void mib_dec_opts_default(mib_dec_opts *o);   /* no dictionary, max_out -1, out_window 0 */
typedef struct mib_decoder mib_decoder;
mib_decoder *mib_decoder_new(const mib_dec_opts *o);   /* o NULL: the defaults */
int mib_decoder_update(mib_decoder *d, const uint8_t *in, size_t n, mib_buf *out);
int mib_decoder_finish(mib_decoder *d, mib_buf *out);
int mib_decoder_is_finished(const mib_decoder *d);   /* the last metablock has been decoded */
void mib_decoder_free(mib_decoder *d);
/* Diagnostic (tests, scripts/stream_decode_rate.py): device passes (decode launches) the
 * session has made, and the output bytes it decoded more than once (a launch that runs out of
 * input goes back to its last checkpoint).  Either pointer may be NULL. */
void mib_decoder_stats(const mib_decoder *d, uint64_t *passes, uint64_t *redecoded);
/* Diagnostic (tests): a call over no more sessions than the device has compute units runs the
 * decode kernel's one-stream-per-CU build (65,536 LDS table entries); non-zero makes every
 * launch of the session entry points use the four-per-CU build instead (12,224 entries,
 * block-type trees in scratch), the one a batch of more sessions gets; 0 restores. */
void mib_force_decoder_build(int four_per_cu);
/* Many sessions at once (a service holding many connections): k distinct sessions advance by
 * one chunk each; a round is ONE decode launch over every session that still has work, and a
 * call makes as many rounds as its neediest session makes passes.  status[i] / out[i] are what
 * mib_decoder_update(d[i], ...) / mib_decoder_finish(d[i], ...) alone would have returned, byte
 * for byte: everything about one stream (a corrupt stream, bytes behind its end, its output
 * limit, a failed allocation, an earlier error) is that session's status and leaves the others
 * running.  The sessions may be in any state and have any options; batch and solo calls may be
 * mixed on one session.  The call itself returns 0, MIB_E_NO_DEVICE, or MIB_E_INVALID_ARG (a NULL
 * array with k > 0, a NULL handle, NULL data with a size, the same handle twice: checked before
 * any session is touched).  A call whose chunks are all empty needs no device. */
int mib_decoder_update_batch(mib_decoder *const *d, const mib_span *in, size_t k, mib_buf *out, int *status);
int mib_decoder_finish_batch(mib_decoder *const *d, size_t k, mib_buf *out, int *status);
/* The same batches with the chunks and the decoded bytes in device memory (DESIGN.md 4d
 * "Device-resident batches"): nothing of either passes through host memory.  d_in / d_out are
 * device pointers on the default context's device (where the sessions live); in_offsets,
 * out_offsets (k + 1 entries), out_sizes and status (k entries) are host arrays, in the shape
 * of mib_ctx_decode.  Session i's chunk is d_in[in_offsets[i], in_offsets[i+1]); its bytes go
 * to d_out + out_offsets[i], room out_offsets[i+1] - out_offsets[i].  Offsets have any
 * alignment and room may be 0; the ranges must not overlap each other or a session's memory
 * (the 16-byte granules that hold a chunk's first and last byte are read whole).  Synchronous on
 * the default context's stream: the caller's writes to d_in are complete before the call, d_out
 * is complete on return.  Returns as mib_decoder_update_batch (also MIB_E_INVALID_ARG for a
 * decreasing offset, or a NULL buffer whose offsets span bytes).  Per slot:
 *   status 0                   out_sizes[i] bytes were written, all that the input so far
 *                              determines; while no slot runs out of room, byte for byte what
 *                              the host call returns for the same chunks
 *   MIB_DEC_MORE_OUTPUT        the range was filled (out_sizes[i] == room) and the session has
 *                              more: decoded bytes it holds (mib_decoder_held_output) or a launch
 *                              it still has to make.  Call again; an empty chunk will do
 *   < 0                        the host call's code; out_sizes[i] 0 (MIB_E_OUTPUT_LIMIT: the total)
 * Bytes of a range behind out_sizes[i] are unspecified; none outside the range is written.
 * Host and device calls may be mixed on a session: a host call first returns what is held. */
#define MIB_DEC_MORE_OUTPUT 1
int mib_decoder_update_batch_device(mib_decoder *const *d, const uint8_t *d_in, const uint64_t *in_offsets, size_t k,
                                    uint8_t *d_out, const uint64_t *out_offsets, uint64_t *out_sizes, int *status);
int mib_decoder_finish_batch_device(mib_decoder *const *d, size_t k, uint8_t *d_out, const uint64_t *out_offsets,
                                    uint64_t *out_sizes, int *status);
uint64_t mib_decoder_held_output(const mib_decoder *d);   /* decoded bytes not yet handed out (0 for NULL) */
/* Diagnostic (tests): the device calls' copy kernel alone, one call over k copies
 * d_dst[i][0, n[i]) <- d_src[i][0, n[i]); host arrays of device pointers of any alignment. */
int mib_debug_copy_batch(const uint8_t *const *d_src, uint8_t *const *d_dst, const uint64_t *n, size_t k);
/* Diagnostic (tests): decode launches made by the session entry points (mib_decoder_update /
 * finish and their batch forms) since process start. */
void mib_decoder_batch_stats(uint64_t *launches);
/* Diagnostic (scripts/stream_decode_rate.py): host wall time the rounds of the decode launches
 * made by the session entry points have spent since process start, ms[0..4] = upload (jobs,
 * heads, move descriptors; the move launch), the decode launch until it is done, the read-back of
 * jobs and heads, the delivery (copy descriptors and copy launch: into the staging span, or for a
 * device-resident call into the callers' ranges), the download of the span and its cutting into
 * results (a device-resident call adds nothing here). */
void mib_decoder_batch_times(double *ms, int n);
/* Diagnostic (tests): at most this many blocks per batch launch (0: the default), so a small
 * batch runs the kernel's job loop more than once per block. */
void mib_force_decoder_grid(int max_blocks);

/* Batches of independent buffers in host memory; one result (and status) per buffer. */
int mib_encode_batch(const mib_span *in, size_t k, const mib_enc_opts *o, mib_buf *out, int *status);
int mib_decode_batch(const mib_span *in, size_t k, mib_buf *out, int *status);
/* The same batches sharded over GPUs (SURVEY.md §8(b),(e)): n_gpus shards (<= 0: one per
 * visible device), size-balanced, one host thread and context per shard, shard s on device
 * s % device count; results in input order.  Safe from several threads (calls serialise). */
int mib_encode_batch_n(const mib_span *in, size_t k, const mib_enc_opts *o, int n_gpus, mib_buf *out, int *status);
int mib_decode_batch_n(const mib_span *in, size_t k, int n_gpus, mib_buf *out, int *status);
/* A prepared dictionary (extension; DESIGN.md 3d "A prepared dictionary"): shared bytes that many
 * small, similar buffers are compressed against, uploaded once.  The handle lives on the default
 * context's device: the bytes and, built there once by a kernel, an index of their positions
 * (two tables of 4 MiB: 4-byte keys for FONT mode, 6-byte keys for GENERIC / TEXT; a table is
 * left out where the dictionary is shorter than its key).  It is immutable, may be used by any
 * number of calls and threads (the calls serialise on the default context, as every host entry
 * point does) and must outlive the calls that use it (a session made with it holds a reference
 * of its own, below).  n may be 0 .. 2^31 - 1; a dictionary of
 * fewer than 4 bytes is attached (it shifts the addresses of the static dictionary's words, as
 * any custom dictionary does) but offers no copies.
 *   mib_dictionary_new   0; MIB_E_INVALID_ARG (NULL out, NULL data with n > 0, n >= 2^31: before
 *                        any device work), MIB_E_NO_DEVICE, MIB_E_OUT_OF_MEMORY; on every error
 *                        *out is NULL
 *   mib_dictionary_free  NULL is harmless;  mib_dictionary_size: n, 0 for NULL
 * Lifetime: the handle is reference counted.  mib_dictionary_new holds one reference, which
 * mib_dictionary_free drops; every session made with the handle (below) holds one, which
 * mib_encoder_free / mib_decoder_free drop.  The device memory goes with the last reference, under
 * the default context's lock.  After mib_dictionary_free the handle may not be given to any new
 * call; the sessions that already hold it keep working.
 * Addressing ("standard"): the decoder's arithmetic is that of mib_decode's customDictionary,
 * address = distance - max distance - 1 - n, a negative value a copy from dictionary offset
 * a = -address - 1; but with a handle the copy is valid whenever a + length <= n (else -9), where
 * mib_enc_opts.dict / customDictionary accept only the copy that ends at the dictionary's last
 * byte.  So the encoder may copy from anywhere in the dictionary.  A stream written by the
 * mib_enc_opts.dict path is valid under this rule too, and mib_decode_batch_dictionary reads it;
 * a stream written with a handle generally decodes only through mib_decode_batch_dictionary
 * (mib_decode answers -9 to its first copy from the middle of the dictionary).  To the author's
 * knowledge this is how google/brotli's C decoder bounds a copy from an attached raw dictionary;
 * no copy of that library was at hand, so interoperability with it is NOT verified.  One risk is
 * known by name: this decoder (as the reference's) pushes the distance of a copy from the
 * dictionary on its ring of last distances even when the distance came with code 0 or as a
 * command's implicit last distance, and with a handle the encoder often writes such commands (a run
 * of the dictionary cut into several copies repeats one distance) and codes what follows against
 * that ring.  A decoder that leaves its ring unchanged on code 0 would read a later short distance
 * code of such a stream differently.
 * Encoder limits: a copy from the dictionary is at most 200 bytes (a longer run becomes several
 * copies), and a match record holds a distance below 2^24 - 1 (below 2^23 where the stream also
 * uses static-dictionary words: quality >= 10, lgwin <= 22, n < 2^22, where it always fits).  A
 * copy from offset a at stream position p has the distance min(p, 2^lgwin - 16) + (n - a), so the
 * encoder uses at least the last MIB_DICTIONARY_MATCH_SPAN(lgwin) bytes of the dictionary at every
 * position, and at a position p below 2^lgwin - 16 that many more as p is below it; what lies in
 * front of that is never copied from (the data still round-trips, as literals or window copies).
 * The index keeps the 8 highest addresses of each of its 2^17 buckets, so of a dictionary of more
 * than about a million bytes the front is found only where its keys are rare.  The decoder has no
 * such limits.
 * The batch calls return as mib_encode_batch / mib_decode_batch do, and MIB_E_INVALID_ARG also for
 * a NULL handle, an o->dict set together with the handle, a NULL array with k > 0, NULL data with
 * a size, max_out < -1 (before any device work); k == 0 needs no device.  status[i] / out[i] as
 * mib_woff2_decode_batch's: everything about one stream is that slot's code and leaves the others
 * running, a failed slot is {NULL, 0}.  max_out (-1: none) applies to every slot as mib_decode's
 * does: MIB_E_OUTPUT_LIMIT, no data, the offending size in out[i].size.  Streams of fewer than 64
 * bytes and quality 0 are stored, as without a dictionary.  The mib_ctx_* and the _n calls take no
 * handle.
 * Sessions (BrotliEncoder / BrotliDecoder with options.dictionary):
 *   mib_encoder_new_dictionary(o, d), mib_decoder_new_dictionary(o, d)
 * return NULL for a NULL handle and for o->dict set together with a handle (both before any device
 * work), else what mib_encoder_new / mib_decoder_new return: an ordinary session, which every entry
 * point takes unchanged and may mix with other sessions in one call -- sessions with other
 * handles, with a customDictionary or with none (mib_encoder_update / _finish / _update_batch,
 * mib_decoder_update / _finish / _update_batch / _finish_batch and the _device forms).  The session
 * uses the handle's device bytes and index in place: no copy of its own, on the host or the device.
 * A handle on another device than the default context's: MIB_E_INVALID_ARG from the first call
 * that needs the device.
 * The addressing is that of the one-shot calls, with p the position in the whole stream: a stream
 * a session writes decodes through mib_decode_batch_dictionary and through a decoder session made
 * with the same bytes; a customDictionary session (mib_dec_opts.dict) answers -9 to its first copy
 * from the middle, as mib_decode does.
 * The encoder limits hold per chunk position.  Past stream position 2^lgwin - 16 the window term
 * of a distance is constant, so from there on the usable span is exactly
 * MIB_DICTIONARY_MATCH_SPAN(lgwin) bytes at the dictionary's end: about 12 MiB at the default
 * lgwin 22, 8 MiB at lgwin 23 and 14 bytes at lgwin 24 -- in a long lgwin-24 stream the handle is
 * all but inert (the data still round-trips).  A streaming chunk gets no static-dictionary words,
 * so the record's distance limit is 2^24 - 1 throughout, at every quality.  A run of the
 * dictionary is cut where a chunk ends, as it is at every 64 KiB parse segment. */
typedef struct mib_dictionary mib_dictionary;
#define MIB_DICTIONARY_MATCH_SPAN(lgwin) (0xFFFFFEu - ((1u << (lgwin)) - 16u))
int mib_dictionary_new(const uint8_t *data, size_t n, mib_dictionary **out);
void mib_dictionary_free(mib_dictionary *d);
uint64_t mib_dictionary_size(const mib_dictionary *d);
int mib_encode_batch_dictionary(const mib_span *in, size_t k, const mib_enc_opts *o, const mib_dictionary *d, mib_buf *out,
                                int *status);
int mib_decode_batch_dictionary(const mib_span *in, size_t k, const mib_dictionary *d, int64_t max_out, mib_buf *out,
                                int *status);
mib_encoder *mib_encoder_new_dictionary(const mib_enc_opts *o, const mib_dictionary *d);
mib_decoder *mib_decoder_new_dictionary(const mib_dec_opts *o, const mib_dictionary *d);
/* Visible HIP devices (0 without a GPU). */
int mib_device_count(void);
/* Diagnostics: the hardware property the match finder's bucket sort relies on for its
 * stability (the lanes of one wave's returning LDS atomic on one address are served in lane
 * order): lanes that broke it over `trials` random collision patterns (0 expected), < 0 on a
 * HIP error. */
int64_t mib_selftest_lds_atomic_order(int trials);
/* The library runs that self-test once per device and, where it fails, ranks the sort's
 * items by wave ballots instead (same stream bytes, slower).  Test hook: force = 1 makes
 * every device take the ballot ranking, 0 restores the self-test's choice. */
void mib_force_ballot_rank(int force);
/* Diagnostic (tests): non-zero makes mib_encode_batch_n / mib_decode_batch_n shard even when one
 * device is visible (by default a single device runs them as mib_encode_batch / mib_decode_batch,
 * one launch sequence). */
void mib_force_shards(int force);
/* Diagnostic (tests): non-zero turns the q10+ parse's distance-cache candidates off (the
 * parse then prices only last-distance copies, short codes 1-15 arise only where codes_kernel
 * finds a chosen distance in the ring), so a test can show what the candidates change; 0
 * restores them. */
void mib_force_no_dp_cache(int off);
/* Diagnostic (tests): how many launches of the parse's kernel this process has made so far with
 * one, two, four and eight pieces (or segments) a wave: out[0..3].  A test reads it before and
 * after a call to see which build of the parse the call took. */
void mib_debug_dp_launches(uint64_t out[4]);
/* Diagnostic (tests): the match finder's candidate walk alone.  The k host buffers are laid
 * out as one encode call lays them out and only that call's bucket sort and find_matches run
 * (no near scan, no dictionary passes, no history); `o` gives quality (depth), lgwin (window)
 * and mode (key bytes).  out[i] receives stream i's records: per position MIB_MAX_MATCHES (4 in
 * the product build) little-endian u32, each length << 24 | distance with stream-relative
 * positions, valid entries first, longest last, zeros after. */
int mib_debug_match_records(const mib_span *in, size_t k, const mib_enc_opts *o, mib_buf *out);
/* Diagnostic (tests): the match search pass by pass, as an encode call with the options `o`
 * runs it.  mib_debug_match_records is this entry with passes = 0 and history = 0.  After the
 * bucket sort and the candidate walk the passes of the bit set `passes` run, in the encoder's
 * order and each only where the encoder runs it for these options and streams (the encoder's
 * own conditions and launch sequence, shared code):
 *   2  static-dictionary words (one-shot streams at quality >= 10 and lgwin <= 22, the first
 *      64 KiB of a stream), through the encoder's device word table;
 *   4  the custom dictionary's tail copies, the dictionary being o->dict / o->dict_len (streams
 *      that are not stored; a dictionary of fewer than four bytes gives none);
 *   1  the near scan (quality >= 10, not in FONT mode), last: it merges into the records.
 * Any other bit is MIB_E_INVALID_ARG.  The prepared dictionary's lookup (mib_dictionary) and the
 * part index are not run.  history: the first `history` bytes of every buffer lie before its
 * stream, as the window lies before a BrotliEncoder chunk (there is no history table: the walk
 * sees the stream's own positions, the near scan reaches back into the history bytes; a chunk
 * gets no static words); every buffer must hold at least that many bytes.  out[i] receives the
 * records of the size - history positions after the history, in mib_debug_match_records' layout.
 * Beside the walk's entries (length << 24 | distance) a record can hold:
 *   a near entry   length << 24 | d, 1 <= d <= 63, length 2 .. 32, in front of the walk's
 *                  entries longer than the longest near entry (a full record drops from the front);
 *   a word         length << 24 | 1 << 23 | index, the identity transform of word `index` of
 *                  that length in the RFC 7932 dictionary: the record's only entry;
 *   a custom tail  length << 24 | 0xFFFFFF, the last `length` bytes of the custom dictionary:
 *                  the record's only entry. */
int mib_debug_match_passes(const mib_span *in, size_t k, const mib_enc_opts *o, int passes, uint32_t history, mib_buf *out);
/* Diagnostic (tests): the encoder's Huffman kernel alone on chosen histograms.  alphabet[i] is
 * 256 (a literal code), 704 (a command code) or 64 (a distance code, NPOSTFIX 0 and NDIRECT 0);
 * hist holds the k histograms back to back, histogram i as alphabet[i] u32 counts.  They are
 * placed in fabricated metablocks -- per metablock as many literal codes as the encoder's launch
 * has literal blocks, spread over eight block types, eight command types, eight distance types
 * of four codes -- and the kernel runs once, with the encoder's own launch arithmetic.  *out
 * receives k records of MIB_PREFIX_CODE_RECORD bytes, histogram i's at i * that: u32 bit count of
 * the serialised code, u8 depth[704], u16 code[704] (both zero past the alphabet), then the
 * 1024 bytes the kernel serialised the code into (LSB first, zero after the last bit). */
#define MIB_PREFIX_CODE_RECORD (4 + 704 + 2 * 704 + 1024)
int mib_debug_prefix_codes(const uint32_t *hist, const uint32_t *alphabet, size_t k, mib_buf *out);

void mib_buf_free(mib_buf *b);
/* The allocator behind every mib_buf the library returns (default malloc / free), in the
 * convention of brotli's own C API (brotli_alloc_func / brotli_free_func with an opaque
 * pointer, c/include/brotli/types.h): a binding can hand results over without a copy (the
 * Python mirror allocates its bytes objects this way).  Process-wide; set it before any
 * other call and free every buffer with the allocator that made it.  NULL, NULL: malloc /
 * free again.  alloc may return NULL (MIB_E_OUT_OF_MEMORY). */
typedef void *(*mib_alloc_func)(void *opaque, size_t size);
typedef void (*mib_free_func)(void *opaque, void *address);
void mib_set_allocator(mib_alloc_func alloc_func, mib_free_func free_func, void *opaque);

/* ---- device-resident batches (inputs already in HBM; used by bench.py and the
 *      multi-GPU driver).  d_* are device pointers on the context's device; offsets are
 *      host arrays of k+1 entries; `stream` is a hipStream_t (NULL = the context's own). */
typedef struct mib_ctx mib_ctx;
mib_ctx *mib_ctx_new(int device);
void mib_ctx_free(mib_ctx *c);
/* Packs the k compressed streams back to back into d_out (capacity out_cap) and fills
 * out_offsets[0..k].  Returns 0, or MIB_E_NEED_SPACE. */
int mib_ctx_encode(mib_ctx *c, const mib_enc_opts *o, const uint8_t *d_in, const uint64_t *in_offsets,
                   size_t k, uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets, void *stream);
/* Decodes k streams; stream i's output goes to d_out + out_offsets[i] with capacity
 * out_offsets[i+1] - out_offsets[i].  out_sizes[i] / status[i] filled (host arrays). */
int mib_ctx_decode(mib_ctx *c, const uint8_t *d_in, const uint64_t *in_offsets, size_t k, uint8_t *d_out,
                   const uint64_t *out_offsets, int64_t *out_sizes, int *status, void *stream);
/* Per-kernel device time of the last mib_ctx_* call (ms, HIP events on the launch stream). */
typedef struct { char name[32]; double ms; uint32_t launches; } mib_kernel_time;
int mib_ctx_kernel_times(mib_ctx *c, mib_kernel_time *out, int max);
/* on: 0 off, 1 every kernel, 2 the decoder's kernels only (one event pair a decode call; the
 * encoder's ~25 event pairs a call are overhead a small call notices). */
void mib_ctx_set_profiling(mib_ctx *c, int on);
/* The context behind the host-buffer entry points (mib_encode, mib_decode, the batches,
 * BrotliEncoder), created on first use (NULL without a device): for profiling them.  Its
 * kernel times accumulate over those calls until mib_ctx_clear_times. */
mib_ctx *mib_default_ctx(void);
void mib_ctx_clear_times(mib_ctx *c);
/* WOFF2 'glyf' transform (the FONT-mode caller, reference README.md:63;
 * W3C WOFF2 section 5.1): the glyf + loca tables of the TrueType font `ttf` become the
 * transformed glyf table (header, the seven streams, the overlap-simple bitmap), byte for
 * byte what fontTools' WOFF2GlyfTable.transform produces.  MIB_E_INVALID_ARG for a font
 * without glyf / loca / head / maxp or with a malformed glyph. */
int mib_woff2_transform_glyf(const uint8_t *ttf, size_t n, mib_buf *out);
/* WOFF2 'hmtx' transform (W3C WOFF2 section 5.4; fontTools WOFF2HmtxTable.transform): flags,
 * the advance widths and whichever left-side-bearing array does not equal the glyphs' xMin.
 * Returns 0 with out->size = 0 when both arrays differ (no transform: the table is stored
 * as is).  The transformed loca table is empty (WOFF2 section 5.3): nothing to compute. */
int mib_woff2_transform_hmtx(const uint8_t *ttf, size_t n, mib_buf *out);
/* Inverse of mib_woff2_transform_glyf (W3C WOFF2 section 5.1, 5.3): the transformed glyf table
 * becomes a TrueType glyf table and its loca table (format = the header's indexFormat), byte
 * for byte what fontTools' WOFF2GlyfTable.reconstruct + compile (4-byte padding, boxes kept)
 * and WOFF2LocaTable.compile produce.  The bytes are untrusted: MIB_E_INVALID_ARG for a header
 * that does not add up, a glyph that runs past a stream, streams not used up exactly, a
 * composite without its box, or offsets that loca format 0 cannot hold. */
int mib_woff2_reconstruct_glyf(const uint8_t *tglyf, size_t n, mib_buf *glyf, mib_buf *loca);
/* Inverse of mib_woff2_transform_hmtx (section 5.4): advance widths plus the side bearings, the
 * dropped array(s) taken from the glyphs' xMin in `glyf` / `loca` (0 for an empty glyph).
 * loca's format follows from loca_n.  MIB_E_INVALID_ARG for reserved flag bits, flags that
 * drop neither array, and a size that is not exactly what the flags imply. */
int mib_woff2_reconstruct_hmtx(const uint8_t *thmtx, size_t n, const uint8_t *glyf, size_t glyf_n,
                               const uint8_t *loca, size_t loca_n, uint32_t num_glyphs,
                               uint32_t num_hmetrics, mib_buf *out);
/* A .woff2 file (W3C WOFF2) -> the sfnt it stands for; of a font collection (flavor ttcf), the
 * OpenType collection (TTC; below).  The Brotli stream is decoded
 * and glyf, loca and hmtx are reconstructed (as the two functions above do) on the device, where
 * the sfnt is assembled as well: offset table, table records sorted by tag, then
 * the tables in the order of the file's directory, each at a 4-byte boundary and zero-padded;
 * table checksums computed, head's checkSumAdjustment set (the rest of head, flags bit 11
 * included, as in the file).  The file is untrusted: MIB_E_INVALID_ARG for a header or directory
 * that does not parse (a repeated tag in one font, an undefined transform version, a malformed
 * UIntBase128, lengths above 256 MiB ...), a stream that does not decode to exactly the
 * directory's total, and whatever the reconstruct functions reject; the decoder's own negative
 * code for a corrupt Brotli stream.  Metadata and private blocks are ignored.  On any error
 * sfnt is {NULL, 0}.
 * A collection (DESIGN.md 4c "A font collection") gives a TTC: 'ttcf', the CollectionHeader's
 * version, numFonts and the offsets of the fonts' offset tables (version 2.0: three zero words
 * more, no DSIG); the fonts' directories back to back, each with its member's flavor and its
 * records sorted by tag, offsets file-relative; then every directory entry that a font lists,
 * once, in the directory's order.  A table shared by several fonts has one checksum; per font,
 * its head's checkSumAdjustment is taken from that font's own directory and tables, and a head
 * shared by several fonts carries the last font's.  Every transformed glyf / loca pair and hmtx
 * is reconstructed.  MIB_E_INVALID_ARG also for a CollectionHeader that does not parse: a version
 * other than 1.0 or 2.0, no fonts, a font without tables, an index past the directory, a tag
 * twice in one font, a glyf entry without its loca right behind it (or a font that lists one of
 * the two alone), a transformed hmtx whose fonts do not agree on its glyf and hhea, directories
 * above 16 MiB together. */
int mib_woff2_decode(const uint8_t *woff2, size_t n, mib_buf *sfnt);
/* Diagnostic (tests): the assembly kernels alone.  k tables (tag, bytes) in host memory are laid
 * out as mib_woff2_decode lays a font out; d_src_misalign[i] in 0..15 is the misalignment table
 * i's bytes get in the device source buffer (NULL: packed back to back, as in a decompressed
 * WOFF2 stream). */
int mib_debug_sfnt_assemble(uint32_t flavor, const uint32_t *tags, const mib_span *tables,
                            const uint8_t *d_src_misalign, size_t k, mib_buf *sfnt);
/* k .woff2 files (single fonts and collections, in any slots) -> their sfnts or TTCs, in shared
 * launches (DESIGN.md 4c "A batch of files"): the Brotli streams of a group of files decode in
 * one launch, the sfnts and TTCs of a group are assembled in one launch of each assembly kernel;
 * glyf and loca are reconstructed pair after pair.  sfnt[i] / status[i] are what mib_woff2_decode(files[i]) alone would have produced, byte
 * for byte and code for code: everything about one file (a container that does not parse, a
 * corrupt stream, a table the reconstruct functions reject) is that slot's status -- 0,
 * MIB_E_INVALID_ARG, the decoder's own negative code, or MIB_E_OUT_OF_MEMORY when the slot's host
 * buffer could not be allocated -- and leaves the others running; a slot with a non-zero status
 * has sfnt[i] = {NULL, 0}.  The same file may stand in several slots.  Returns 0, or
 * MIB_E_INVALID_ARG (a NULL array with k > 0, NULL data with a size: checked before anything
 * else), MIB_E_NO_DEVICE, MIB_E_OUT_OF_MEMORY (a group's device buffers); then every sfnt[i] is
 * {NULL, 0}.  k == 0, and a call none of whose files parses, need no device.  Holds the default
 * context's lock for its duration.  Profiling: every group's decode starts the context's kernel
 * times afresh, so after a call of more than one group the times are the last group's. */
int mib_woff2_decode_batch(const mib_span *files, size_t k, mib_buf *sfnt, int *status);
/* Diagnostic (tests): the files of a call are worked in groups whose decompressed streams sum to
 * at most this many bytes (0: the default, 512 MiB); a file larger than that is a group alone. */
void mib_force_woff2_group_bytes(uint64_t bytes);
/* Diagnostic (tests): the batch's assembly kernels alone over k fonts; font f has counts[f]
 * tables, taken in order from tags / tables / d_src_misalign (as mib_debug_sfnt_assemble). */
int mib_debug_sfnt_assemble_batch(const uint32_t *flavors, const uint32_t *counts, const uint32_t *tags,
                                  const mib_span *tables, const uint8_t *d_src_misalign, size_t k, mib_buf *sfnt);
/* Diagnostic (tests): the assembly kernels alone over a collection.  The k tables are its
 * directory (tags may repeat; taken as mib_debug_sfnt_assemble takes them); member f of n_fonts
 * has font_counts[f] tables, their indices in order from font_indices.  MIB_E_INVALID_ARG for a
 * version other than 1.0 or 2.0, no fonts or more than 65,535, a font without tables, an index at
 * or past k, a tag twice in one font. */
int mib_debug_ttc_assemble(uint32_t version, const uint32_t *tags, const mib_span *tables,
                           const uint8_t *d_src_misalign, size_t k, const uint32_t *font_flavors,
                           const uint32_t *font_counts, const uint32_t *font_indices, size_t n_fonts, mib_buf *ttc);

/* An sfnt (TrueType or CFF flavoured, single font) -> a .woff2 file (W3C WOFF2), written on the
 * device (DESIGN.md 4c "Writing a file"): the font is uploaded once, glyf and hmtx are transformed
 * there (as mib_woff2_transform_glyf / _hmtx do), the other tables are copied into the stream
 * beside them, the stream is compressed in FONT mode, and the compressed bytes land behind the
 * header and directory in the result.  Every byte of the file but the Brotli stream is fixed:
 * tables in ascending tag order, DSIG dropped, origLength the table's length in the input font
 * (for glyf and loca too, where the specification makes it a hint: for a font that is not
 * already normalised the reconstructed tables, and with them totalSfntSize, may differ), head's
 * checkSumAdjustment stored as zero and its flags bit 11 set when glyf / loca are transformed, the
 * header's version head's fontRevision, the file zero-padded to a 4-byte boundary (counted in its
 * length), no metadata, no private block: what fontTools writes for the same font.
 *   transforms  MIB_WOFF2_GLYF: glyf + loca are transformed where the font has them (a font the
 *               transform rejects -- head shorter than 54 bytes, no maxp, a short loca, numGlyphs
 *               0, a malformed glyph -- is MIB_E_INVALID_ARG: no silent fallback);
 *               MIB_WOFF2_HMTX: hmtx is transformed where glyf is, hhea has 36 bytes,
 *               1 <= numberOfHMetrics <= numGlyphs, hmtx is exactly 4 nhm + 2 (ng - nhm) bytes and
 *               a side-bearing array equals the glyphs' xMin; otherwise it is stored as it is.
 *               Unknown bits: MIB_E_INVALID_ARG.
 *   quality, lgwin  clamped as mib_enc_opts'.  o NULL: quality 11, lgwin 22, both transforms.
 * MIB_E_INVALID_ARG, before any device work, for: fewer than 12 bytes; a first tag of wOF2 or
 * wOFF; numTables 0 or a directory past the input; a record whose offset + length runs past the
 * input; a tag twice; table lengths above 256 MiB in sum; exactly one of glyf and loca; nothing
 * left after dropping DSIG.  Checksums, searchRange fields, record order, alignment and overlap
 * of the input's tables are not checked.  mib_woff2_decode accepts every file written.  On any
 * error woff2 is {NULL, 0}.  mib_woff2_encode is the batch with k = 1.
 * An OpenType collection (first tag ttcf, version 1.0 or 2.0) becomes the .woff2 file of flavor
 * ttcf (DESIGN.md 4c "Writing a collection"): one directory over all members, each table in it
 * once, and the CollectionHeader with each member's flavor and indices.  Two records are one
 * table when they have the same tag, offset and length, or the same tag and length and equal
 * bytes (compared on the device; the records' checkSum fields only choose what is compared).
 * glyf and loca are shared as a pair (the same glyf with another loca, numGlyphs or
 * indexToLocFormat is written twice).  Members in the collection's order, each one's tables in
 * ascending tag order with loca directly behind glyf; an entry is appended the first time a
 * member lists it.  DSIG is dropped from every member.  The transforms apply to every pair; to
 * an hmtx entry where every member that lists it lists the same pair and the same hhea and the
 * single-font conditions hold.  Every head of at least 18 bytes is stored with bytes 8..11 zero,
 * and with flags bit 11 set when a member that lists it has a transformed pair.  The header's
 * version is the first member's head's that has one; totalSfntSize counts the TTC header, the
 * members' directories and each entry's origLength padded to 4.
 * MIB_E_INVALID_ARG for a collection, before any device work: the header, an offset table or a
 * directory past the input; a version other than 1.0 or 2.0; numFonts 0 or above 65,535, or a
 * member's numTables 0; a record whose offset + length runs past the input; a tag twice in one
 * member; directories (12 + 16 numTables per member) above 16 MiB in sum; lengths, summed once
 * per distinct (offset, length), above 256 MiB; a member with exactly one of glyf and loca; a
 * member with nothing left after dropping DSIG; more than 65,535 directory entries; with
 * MIB_WOFF2_GLYF, a member with glyf that the transform rejects. */
typedef struct { int quality; int lgwin; uint32_t transforms; } mib_woff2_enc_opts;
#define MIB_WOFF2_GLYF 1u   /* glyf + loca */
#define MIB_WOFF2_HMTX 2u
int mib_woff2_encode(const uint8_t *sfnt, size_t n, const mib_woff2_enc_opts *o, mib_buf *woff2);
/* k fonts (single fonts and collections, in any slots) in shared launches: per group of fonts
 * (mib_force_woff2_group_bytes, counting input bytes) one upload, one compare launch over every
 * candidate of every collection (none where there is no candidate), one copy launch over every
 * untransformed table, one encode call over every stream (a collection is one stream), one
 * synchronisation for the downloads; the transforms run font after font.  woff2[i] /
 * status[i] as mib_woff2_decode_batch's: everything about one font is that slot's status (0,
 * MIB_E_INVALID_ARG, MIB_E_OUT_OF_MEMORY for the slot's host buffer) and leaves the others
 * running; the same font may stand in several slots.  Returns 0, or MIB_E_INVALID_ARG (a NULL
 * array with k > 0, NULL data with a size, unknown transforms bits), MIB_E_NO_DEVICE,
 * MIB_E_OUT_OF_MEMORY (a group's device buffers); then every woff2[i] is {NULL, 0}.  k == 0, and a
 * call in which no font parses, need no device.  Holds the default context's lock. */
int mib_woff2_encode_batch(const mib_span *sfnts, size_t k, const mib_woff2_enc_opts *o, mib_buf *woff2, int *status);
/* Diagnostic (tests): the collection writer's compare kernel alone over k pairs of byte ranges,
 * a[i] and b[i] of one size; misalign_a[i] / misalign_b[i] in 0..15 are the misalignments the
 * ranges get in the device buffer (NULL: 0).  differ[i] becomes 1 where the ranges differ, else 0.
 * MIB_E_INVALID_ARG for sizes that are not equal. */
int mib_debug_tables_equal(const mib_span *a, const mib_span *b, const uint8_t *misalign_a, const uint8_t *misalign_b,
                           size_t k, uint8_t *differ);

/* Part-parallel decoding (streams this encoder marked with a part index):
 * how many streams a context (NULL: the default one) decoded part-parallel, and how many of
 * those it sent back to the serial decoder because a part did not check out. Diagnostic. */
void mib_part_stats(mib_ctx *c, uint64_t *parallel, uint64_t *fallback);

/* A stream that is one final metablock decodes in its output slot, with no pass through the
 * decoder's scratch ring, when the slot holds its decoded size and this many bytes more (no
 * custom dictionary).  Smaller slots decode to the same bytes through the ring. */
#define MIB_IN_PLACE_SLACK 101
/* Diagnostic: of the streams of a context's (NULL: the default one's) last serial decode launch,
 * how many finished in their slots (status 0) and how many began there and went back to the
 * ring, whatever they ended in. */
void mib_debug_in_place(mib_ctx *c, uint64_t *finished, uint64_t *left);

#ifdef __cplusplus
}
#endif
#endif
