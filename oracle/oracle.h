/*
 * ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle_decode.c / oracle_encode.c headers).
 * CPU restatement of countertype/brotli-lib's encode/decode algorithms, used as the
 * checker for the HIP path and as bench.py's cpu_baseline.  Never linked by the product.
 */
#ifndef BROTLI_ORACLE_H_
#define BROTLI_ORACLE_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* engine.ts:2155 peekDecodedSize: decoded size of a single-ISLAST-metablock stream, else -1/0 */
int64_t oracle_peek_decoded_size(const uint8_t *in, size_t n);

/* engine.ts:2197 brotliDecode.  out_size > 0: decode into an exact buffer of that size
 * (truncate / zero-pad, trailing checks skipped, as the reference).  Returns 0 or the
 * reference's negative error code; *out is malloc'ed (free with oracle_free). */
int oracle_decode(const uint8_t *in, size_t n, const uint8_t *dict, size_t dict_n,
                  int64_t out_size, uint8_t **out, size_t *out_n);
/* decode and record the decoder state (parts.h PartEntry layout, 72 bytes each) at the
 * command boundaries / metablock headers at the ascending output positions pos[0..npos) */
int oracle_decode_probe(const uint8_t *in, size_t n, const uint64_t *pos, size_t npos, void *states);
/* static-dictionary word references decoded so far by this process (test instrumentation) */
uint64_t oracle_word_refs(void);
uint64_t oracle_compound_refs(void);
/* out[4]: the copies decoded on this thread since the last call, by distance code: implicit
 * (command code < 128), explicit code 0, short codes 1-15, explicit distances (>= 16) */
void oracle_dist_code_counts(uint64_t *out);
void oracle_max_block_types(int *out);   /* largest (literal, command, distance) block type counts decoded (clears) */
/* largest per-metablock total of the literal, command and distance tree groups, roots included,
 * in table entries, decoded on this thread since the last call (clears) */
int oracle_max_table_total(void);

/* Trace of the prefix codes and context maps a decode reads (tests/_entropy_audit.py).  Per
 * thread, off by default; off, oracle_decode does exactly what it did without it.
 * oracle_trace(1) clears the thread's trace and turns it on: every oracle_decode on the thread
 * then appends records; oracle_trace(0) frees them and turns it off.  The arrays returned stay
 * valid until the thread's next oracle_trace call.  Bit positions count from the stream's
 * first bit (LSB of byte 0 first). */
struct OracleTraceCode {
  int32_t kind;      /* 0 literal, 1 command, 2 distance; 3 + c block type code and 6 + c block count
                      * code of category c (0 literal, 1 command, 2 distance); 9 literal and 10
                      * distance context map code */
  int32_t index;     /* tree index within its kind (0 for the others) */
  int32_t alphabet;  /* symbols of its alphabet */
  int32_t mb;        /* its metablock: headers read before this one's, metadata and stored ones included */
  int64_t begin, end;   /* its serialisation: stream bits [begin, end) */
  uint32_t *hist;    /* [alphabet] symbols decoded with it afterwards; a block count code's
                      * includes the first count in the header, a block type code's the switches only */
};
struct OracleTraceMap {
  int32_t kind;      /* 0 literal, 1 distance */
  int32_t mb;
  int32_t size;      /* entries: 64 per literal block type, 4 per distance block type */
  int32_t ntrees;
  int64_t begin, end;   /* the coded map, NTREES through the IMTF bit (NTREES alone when it is 1) */
  uint8_t *values;   /* [size] the decoded map */
};
void oracle_trace(int on);
size_t oracle_trace_codes(const struct OracleTraceCode **out);
size_t oracle_trace_maps(const struct OracleTraceMap **out);
void oracle_trace_metablocks(int32_t out[4]);   /* compressed, stored, metadata, empty-last metablocks read */

/* The reference's own serialisers, for one histogram / one context map (oracle_encode.c).
 * createHuffmanTree: fills depths[len]; returns how many count limits it tried (1: the first tree
 * was within `limit`; 0: fewer than two used symbols, no tree).
 * buildAndStoreHuffmanTree: fills depths / bits [asize], writes the code into out (LSB first);
 * returns its bit count, -1 when cap bytes are too few.
 * encodeContextMap (RLEMAX cap 6, move-to-front on): the coded map of cmap[size] over nclusters
 * trees, NTREES through the IMTF bit; returns its bit count or -1. */
int oracle_create_huffman_tree(const uint32_t *h, int len, int limit, uint8_t *depths);
int64_t oracle_build_store_tree(const uint32_t *h, int asize, uint8_t *depths, uint16_t *bits, uint8_t *out, size_t cap);
int64_t oracle_encode_context_map(const uint32_t *cmap, int size, int nclusters, uint8_t *out, size_t cap);

/* encode.ts:50 brotliEncode (bugs A,B fixed = the survey's "ref-fixed"; C,E fixed too).
 * quality 0..11, lgwin 10..24, mode 0 GENERIC / 1 TEXT / 2 FONT. */
int oracle_encode(const uint8_t *in, size_t n, int quality, int lgwin, int mode,
                  uint8_t **out, size_t *out_n);

/* createHqZopfliBackwardReferences pass 1: every position's findAllMatches list (ref-fixed
 * binary tree, hash-binary-tree.ts:57-227), flat: i, count, (distance, length) x count. */
int64_t oracle_bt_matches(const uint8_t *in, size_t n, int lgwin, uint32_t *out, size_t cap);

void oracle_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
