/* The oracle decoder's trace on malformed input, as a stand-alone program for AddressSanitizer and
 * UBSan (tests/test_entropy_audit_host.py compiles it with oracle/oracle_decode.c and
 * oracle/oracle_encode.c).  argv[1]: a file of streams, each a little-endian u32 length and
 * that many bytes.  Every stream is decoded with the trace on and every record is read in full:
 * each histogram over its alphabet, each map over its size, each bit range against the stream. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oracle.h"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  size_t streams = 0, failed = 0, codes = 0, maps = 0, bad = 0;
  uint64_t sum = 0;
  for (;;) {
    uint8_t lenb[4];
    if (fread(lenb, 1, 4, f) != 4) break;
    const size_t n = (size_t)lenb[0] | ((size_t)lenb[1] << 8) | ((size_t)lenb[2] << 16) | ((size_t)lenb[3] << 24);
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);   /* exactly n bytes: a read past the stream is an ASan error */
    if (!in || fread(in, 1, n, f) != n) return 2;
    oracle_trace(1);
    uint8_t *out = NULL;
    size_t out_n = 0;
    const int rc = oracle_decode(in, n, NULL, 0, -1, &out, &out_n);
    if (rc) failed++;
    else oracle_free(out);
    const struct OracleTraceCode *c;
    const struct OracleTraceMap *m;
    const size_t nc = oracle_trace_codes(&c), nm = oracle_trace_maps(&m);
    for (size_t i = 0; i < nc; i++) {
      if (c[i].kind < 0 || c[i].kind > 10 || c[i].alphabet <= 0 || c[i].alphabet > 1128 || c[i].begin < 0 || c[i].end < c[i].begin) bad++;
      for (int k = 0; k < c[i].alphabet; k++) sum += c[i].hist[k];
    }
    for (size_t i = 0; i < nm; i++) {
      if (m[i].kind < 0 || m[i].kind > 1 || m[i].size <= 0 || m[i].size > 256 * 64 || m[i].ntrees < 1 || m[i].ntrees > 256 ||
          m[i].begin < 0 || m[i].end < m[i].begin)
        bad++;
      for (int k = 0; k < m[i].size; k++) {
        if (m[i].values[k] >= m[i].ntrees) bad++;
        sum += m[i].values[k];
      }
    }
    int32_t mbs[4];
    oracle_trace_metablocks(mbs);
    for (int k = 0; k < 4; k++) sum += (uint64_t)mbs[k];
    codes += nc;
    maps += nm;
    streams++;
    oracle_trace(0);
    /* off again: the same decode, untraced, gives the same result */
    uint8_t *out2 = NULL;
    size_t out2_n = 0;
    const int rc2 = oracle_decode(in, n, NULL, 0, -1, &out2, &out2_n);
    if (rc2 != rc) bad++;
    if (!rc2) oracle_free(out2);
    free(in);
  }
  fclose(f);
  printf("streams %zu failed %zu codes %zu maps %zu bad %zu sum %llu\n", streams, failed, codes, maps, bad,
         (unsigned long long)sum);
  return bad ? 1 : 0;
}
