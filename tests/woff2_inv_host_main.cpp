// Stand-alone host build of the WOFF2 inverse walker (brotli-lib_amd/csrc/woff2_inv.h): the
// same text the GPU kernels compile, driven serially and meant to be built with
// -fsanitize=address,undefined (tests/test_woff2_reconstruct_golden.py).
//
//   woff2_inv_host check FILE        every fixture reconstructs to its stored bytes
//   woff2_inv_host fuzz FILE SEED N  damaged copies of the fixtures' tables: each is rejected,
//                                    or reconstructs within the size the sizing pass announced
//   woff2_inv_host reject FILE       every table in FILE is rejected (the GPU test's bad inputs)
// FILE: records of u32 little-endian length + bytes.  check / fuzz: seven per fixture
// (tglyf, glyf, loca, thmtx, hmtx, num_glyphs as 4 bytes, num_hmetrics as 4 bytes);
// reject: six per case (kind: "glyf" or "hmtx", table, and for hmtx the glyf, the loca,
// num_glyphs and num_hmetrics it goes with; empty for glyf).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "woff2_inv.h"

using namespace mib::woff2inv;
typedef std::vector<uint8_t> Bytes;

static std::vector<Bytes> read_records(const char *path) {
  std::vector<Bytes> r;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t h[4];
  while (fread(h, 1, 4, f) == 4) {
    const uint32_t n = h[0] | (h[1] << 8) | (h[2] << 16) | ((uint32_t)h[3] << 24);
    Bytes b(n);
    if (n && fread(b.data(), 1, n, f) != n) {
      fprintf(stderr, "short record in %s\n", path);
      exit(2);
    }
    r.push_back(b);
  }
  fclose(f);
  return r;
}
static uint32_t le32(const Bytes &b) { return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24); }

// The table in a heap block of exactly its size, so that a read past it is a sanitizer report.
static int run_glyf(const Bytes &t, Bytes *glyf, Bytes *loca) {
  uint8_t *exact = (uint8_t *)malloc(t.size() ? t.size() : 1);
  if (!t.empty()) memcpy(exact, t.data(), t.size());
  uint64_t announced = 0;
  const int rc = host_reconstruct(t.empty() ? nullptr : exact, t.size(), glyf, loca, &announced);
  free(exact);
  if (rc == 0 && glyf->size() != (announced ? announced : 1)) {
    fprintf(stderr, "output %zu bytes, announced %llu\n", glyf->size(), (unsigned long long)announced);
    exit(1);
  }
  return rc;
}
static int run_hmtx(const Bytes &t, const Bytes &glyf, const Bytes &loca, uint32_t ng, uint32_t nhm, Bytes *out) {
  uint8_t *exact = (uint8_t *)malloc(t.size() ? t.size() : 1);
  if (!t.empty()) memcpy(exact, t.data(), t.size());
  const int rc = host_reconstruct_hmtx(t.empty() ? nullptr : exact, t.size(), glyf.data(), glyf.size(), loca.data(),
                                       loca.size(), ng, nhm, out);
  free(exact);
  return rc;
}

static uint64_t g_rng;
static uint32_t rnd() {   // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 2685821657736338717ull) >> 32);
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  const std::vector<Bytes> rec = read_records(argv[2]);
  if (mode == "reject") {
    if (rec.size() % 6) return 2;
    for (size_t i = 0; i < rec.size(); i += 6) {
      const std::string kind(rec[i].begin(), rec[i].end());
      Bytes a, b;
      const int rc = kind == "glyf" ? run_glyf(rec[i + 1], &a, &b)
                                    : run_hmtx(rec[i + 1], rec[i + 2], rec[i + 3], le32(rec[i + 4]), le32(rec[i + 5]), &a);
      if (rc == 0) {
        fprintf(stderr, "case %zu (%s) was accepted\n", i / 6, kind.c_str());
        return 1;
      }
    }
    printf("rejected %zu\n", rec.size() / 6);
    return 0;
  }
  if (rec.size() % 7) return 2;
  if (mode == "check") {
    for (size_t i = 0; i < rec.size(); i += 7) {
      Bytes glyf, loca, hmtx;
      if (run_glyf(rec[i], &glyf, &loca) != 0 || glyf != rec[i + 1] || loca != rec[i + 2]) {
        size_t d = 0;
        while (d < glyf.size() && d < rec[i + 1].size() && glyf[d] == rec[i + 1][d]) d++;
        fprintf(stderr, "fixture %zu: glyf / loca differ (glyf %zu vs %zu bytes, first difference at %zu)\n", i / 7,
                glyf.size(), rec[i + 1].size(), d);
        return 1;
      }
      const uint32_t ng = le32(rec[i + 5]), nhm = le32(rec[i + 6]);
      if (!rec[i + 3].empty() && (run_hmtx(rec[i + 3], glyf, loca, ng, nhm, &hmtx) != 0 || hmtx != rec[i + 4])) {
        fprintf(stderr, "fixture %zu: hmtx differs\n", i / 7);
        return 1;
      }
    }
    printf("checked %zu\n", rec.size() / 7);
    return 0;
  }
  if (mode != "fuzz" || argc < 5) return 2;
  g_rng = strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
  const size_t edits = strtoull(argv[4], nullptr, 10);
  size_t total = 0, accepted = 0;
  auto one = [&](const Bytes &t) {
    Bytes glyf, loca;
    total++;
    if (run_glyf(t, &glyf, &loca) == 0) accepted++;
  };
  for (size_t i = 0; i < rec.size(); i += 7) {
    const Bytes &t = rec[i];
    // truncations: every length below 64, and at and around every stream boundary
    for (size_t len = 0; len < 64 && len < t.size(); len++) one(Bytes(t.begin(), t.begin() + len));
    size_t at = kHeaderBytes;
    for (int s = 0; s < kStreams; s++) {
      const size_t sz = ((size_t)t[8 + 4 * s] << 24) | (t[9 + 4 * s] << 16) | (t[10 + 4 * s] << 8) | t[11 + 4 * s];
      at += sz;
      for (int d = -1; d <= 1; d++)
        if (at + d <= t.size()) one(Bytes(t.begin(), t.begin() + at + d));
    }
    // header size fields (and the glyph count) moved by 1 and by 255
    static const int kDeltas[4] = {1, -1, 255, -255};
    for (int f = 0; f < kStreams + 1; f++)
      for (int d = 0; d < 4; d++) {
        Bytes u = t;
        if (f == kStreams) {
          const uint32_t v = (((uint32_t)u[4] << 8) | u[5]) + (uint32_t)kDeltas[d];
          u[4] = (uint8_t)(v >> 8), u[5] = (uint8_t)v;
        } else {
          uint32_t v = ((uint32_t)u[8 + 4 * f] << 24) | (u[9 + 4 * f] << 16) | (u[10 + 4 * f] << 8) | u[11 + 4 * f];
          v += (uint32_t)kDeltas[d];
          u[8 + 4 * f] = (uint8_t)(v >> 24), u[9 + 4 * f] = (uint8_t)(v >> 16), u[10 + 4 * f] = (uint8_t)(v >> 8),
                    u[11 + 4 * f] = (uint8_t)v;
        }
        one(u);
        // ... and with the table grown or cut by as much, so that the sizes still add up
        const long nl = (long)u.size() + kDeltas[d];
        if (f < kStreams && nl >= 0) {
          u.resize((size_t)nl, 0);
          one(u);
        }
      }
    // single-byte edits: a random place, a random or an off-by-one / extreme value
    for (size_t e = 0; e < edits; e++) {
      Bytes u = t;
      const size_t p = rnd() % u.size();
      const uint32_t how = rnd() % 6;
      const uint8_t old = u[p];
      u[p] = how == 0 ? old + 1 : how == 1 ? old - 1 : how == 2 ? 0xFF : how == 3 ? 0 : how == 4 ? (old ^ (1u << (rnd() & 7))) : (uint8_t)rnd();
      one(u);
    }
    // hmtx: every flag value, every length up to a little past the right one
    const Bytes &h = rec[i + 3];
    if (!h.empty()) {
      Bytes glyf, loca, out;
      if (run_glyf(t, &glyf, &loca) != 0) return 1;
      const uint32_t ng = le32(rec[i + 5]), nhm = le32(rec[i + 6]);
      for (int fl = 0; fl < 256; fl++) {
        Bytes u = h;
        u[0] = (uint8_t)fl;
        for (size_t len = 0; len <= h.size() + 4 * ng + 8; len += (len < 8 ? 1 : 2 * ng - 1)) {
          u.resize(len, 0);
          total++;
          if (run_hmtx(u, glyf, loca, ng, nhm, &out) == 0) accepted++;
        }
      }
      // damaged loca under an hmtx that takes every side bearing from glyf
      for (size_t e = 0; e < 2000; e++) {
        Bytes l = loca, u(1 + 2 * (size_t)nhm, 0);
        u[0] = 3;
        l[rnd() % l.size()] = (uint8_t)rnd();
        total++;
        if (run_hmtx(u, glyf, l, ng, nhm, &out) == 0) accepted++;
      }
    }
  }
  printf("damaged %zu accepted %zu rejected %zu\n", total, accepted, total - accepted);
  return 0;
}
