// A prepared dictionary's arithmetic (brotli-lib_amd/csrc/shared_dict.h) as host code, built with
// AddressSanitizer and UBSan by tests/test_shared_dict_host.py.  The dictionaries and documents
// live in heap blocks of their exact sizes, so a read past either end -- a candidate whose bytes
// go on matching into the zero padding behind the device copy, for one -- is the sanitizer's report.
//
//   shared_dict_host measure SEED   random dictionaries (4 B .. 8 KiB), documents cut from them:
//                                   every (position, address) measured and checked
//   shared_dict_host roundtrip      distance <-> address, both sides of p = max backward (lgwin 10)
//   shared_dict_host edges          address 0, the last byte, bytes that go on matching into padding
// Prints "ok <checks>" and returns 0, or a line saying what failed and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "shared_dict.h"

using namespace mib;

static long g_checks = 0;
#define CHECK(c, ...)                \
  do {                               \
    g_checks++;                      \
    if (!(c)) {                      \
      printf("FAILED %s: ", #c);     \
      printf(__VA_ARGS__);           \
      printf("\n");                  \
      exit(1);                       \
    }                                \
  } while (0)

// exact-size heap copies: ASan guards both ends
struct Block {
  uint8_t *p;
  size_t n;
  explicit Block(const std::vector<uint8_t> &v) : p((uint8_t *)malloc(v.size() ? v.size() : 1)), n(v.size()) {
    if (n) memcpy(p, v.data(), n);
  }
  ~Block() { free(p); }
};

static void check_copy(const Block &doc, uint32_t p, uint32_t seg_end, const Block &dict, uint32_t a, uint32_t len) {
  const uint32_t limit = seg_end - p;
  CHECK(len <= sd::kMaxCopy, "length %u above the cap", len);
  CHECK(len <= limit, "p %u len %u leaves the segment (end %u)", p, len, seg_end);
  CHECK((uint64_t)a + len <= dict.n, "a %u len %u leaves the dictionary (%zu)", a, len, dict.n);
  CHECK(sd::copy_valid(a, len, (int64_t)dict.n) && sd::copy_valid_u32(a, len, (uint32_t)dict.n), "rule rejects a %u len %u", a, len);
  CHECK(memcmp(doc.p + p, dict.p + a, len) == 0, "p %u a %u len %u: bytes differ", p, a, len);
  // maximal: stopped by a cap or by a differing byte
  const bool capped = len == sd::kMaxCopy || len == limit || a + len == dict.n;
  CHECK(capped || doc.p[p + len] != dict.p[a + len], "p %u a %u: stopped early at %u", p, a, len);
}

static int run_measure(unsigned seed) {
  std::mt19937 rng(seed);
  const size_t sizes[] = {4, 5, 6, 7, 64, 255, 1000, 4096, 8192};
  for (size_t dn : sizes) {
    std::vector<uint8_t> dv(dn);
    // few symbols: long accidental matches, runs, matches that reach the dictionary's end
    const int alpha = 2 + (int)(rng() % 3);
    for (auto &b : dv) b = (uint8_t)(rng() % alpha);
    Block dict(dv);
    for (int rep = 0; rep < 6; rep++) {
      // a document of slices of the dictionary with a few other bytes between them
      std::vector<uint8_t> doc;
      const size_t want = 50 + rng() % 1200;
      while (doc.size() < want) {
        const size_t a = rng() % dn, k = 1 + rng() % (dn - a);
        doc.insert(doc.end(), dv.begin() + a, dv.begin() + a + std::min<size_t>(k, 700));
        for (unsigned q = rng() % 3; q; q--) doc.push_back((uint8_t)(rng() % alpha));
      }
      Block d(doc);
      // parse segments: the document cut at a random place (a copy may not cross it)
      const uint32_t cut = 1 + (uint32_t)(rng() % d.n);
      for (uint32_t p = 0; p < d.n; p++) {
        const uint32_t seg_end = p < cut ? cut : (uint32_t)d.n;
        // every address for small dictionaries, a sample for large ones (and always the ends)
        const uint32_t step = dn <= 255 ? 1 : 1 + (uint32_t)(rng() % 97);
        for (uint32_t a = 0; a < dn; a += step) {
          const uint32_t len = sd::measure(d.p + p, seg_end - p, dict.p, (uint32_t)dn, a);
          check_copy(d, p, seg_end, dict, a, len);
        }
        const uint32_t a_last = (uint32_t)dn - 1;
        check_copy(d, p, seg_end, dict, a_last, sd::measure(d.p + p, seg_end - p, dict.p, (uint32_t)dn, a_last));
        CHECK(sd::measure(d.p + p, seg_end - p, dict.p, (uint32_t)dn, (uint32_t)dn) == 0, "an address at the end measures 0");
      }
    }
  }
  return 0;
}

static int run_roundtrip() {
  const int lgwin = 10;
  const uint32_t maxback = (1u << lgwin) - 16;   // 1008
  const uint32_t dict_len = 5000;
  for (uint32_t p = 0; p < 3000; p += (p > 990 && p < 1030) ? 1 : 7) {
    const uint32_t window = p < maxback ? p : maxback;
    for (uint32_t a : {0u, 1u, 17u, 2499u, 4998u, 4999u}) {
      const uint64_t d = sd::distance_of(window, dict_len, a);
      CHECK(d > window, "p %u a %u: distance %llu inside the window", p, a, (unsigned long long)d);
      // the decoder: max distance = min(position, max backward)
      const int64_t address = sd::address_of((int64_t)d, window, dict_len);
      CHECK(address < 0, "p %u a %u: address %lld is not in the dictionary", p, a, (long long)address);
      CHECK(sd::offset_of(address) == (int64_t)a, "p %u: a %u came back as %lld", p, a, (long long)sd::offset_of(address));
      // the other direction: an address in the dictionary has one distance at a position
      CHECK(sd::distance_of(window, dict_len, (uint32_t)sd::offset_of(address)) == d, "p %u a %u", p, a);
      CHECK(sd::copy_valid(a, dict_len - a, dict_len) && !sd::copy_valid(a, dict_len - a + 1, dict_len), "rule at a %u", a);
      CHECK(sd::copy_valid_tail(a, dict_len - a, dict_len) && (a == 0 || !sd::copy_valid_tail(a, dict_len - a - 1, dict_len)),
            "tail rule at a %u", a);
    }
    // one step further than the dictionary's first byte is a static word's address (>= 0)
    CHECK(sd::address_of((int64_t)sd::distance_of(window, dict_len, 0) + 1, window, dict_len) == 0, "p %u: first word", p);
  }
  // the record's field
  CHECK(sd::record_holds(0xFFFFFEu, false) && !sd::record_holds(0xFFFFFFu, false), "24-bit limit");
  CHECK(sd::record_holds((1u << 23) - 1, true) && !sd::record_holds(1u << 23, true), "word flag");
  return 0;
}

static int run_edges() {
  std::vector<uint8_t> dv(300);
  for (size_t i = 0; i < dv.size(); i++) dv[i] = (uint8_t)(i * 7 + 1);
  dv[296] = dv[297] = dv[298] = dv[299] = 0;   // the dictionary ends in zeros ...
  Block dict(dv);
  {   // address 0, the whole dictionary's head
    std::vector<uint8_t> doc(dv.begin(), dv.begin() + 120);
    doc.push_back(0xEE);
    Block d(doc);
    CHECK(sd::measure(d.p, (uint32_t)d.n, dict.p, 300, 0) == 120, "address 0");
  }
  {   // a copy that ends at the last byte, with the document going on in zeros: the padding trap
    std::vector<uint8_t> doc(dv.begin() + 250, dv.end());
    doc.insert(doc.end(), 64, 0);   // ... and so does what follows the slice in the document
    Block d(doc);
    CHECK(sd::measure(d.p, (uint32_t)d.n, dict.p, 300, 250) == 50, "stops at the dictionary's last byte");
    CHECK(sd::measure(d.p + 46, (uint32_t)d.n - 46, dict.p, 300, 296) == 4, "the zeros at the end, and no further");
    CHECK(sd::measure(d.p + 49, (uint32_t)d.n - 49, dict.p, 300, 299) == 1, "the last byte alone");
  }
  {   // caps: the segment's end, then kMaxCopy
    std::vector<uint8_t> doc(dv.begin(), dv.begin() + 290);
    Block d(doc);
    CHECK(sd::measure(d.p, 10, dict.p, 300, 0) == 10, "segment cap");
    CHECK(sd::measure(d.p, (uint32_t)d.n, dict.p, 300, 0) == sd::kMaxCopy, "length cap");
    CHECK(sd::measure(d.p, 0, dict.p, 300, 0) == 0, "no room");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  int rc = 2;
  if (!strcmp(argv[1], "measure") && argc == 3) rc = run_measure((unsigned)atoi(argv[2]));
  else if (!strcmp(argv[1], "roundtrip")) rc = run_roundtrip();
  else if (!strcmp(argv[1], "edges")) rc = run_edges();
  if (rc == 0) printf("ok %ld\n", g_checks);
  return rc;
}
