// A prepared dictionary (mib_dictionary, DESIGN.md 3d "A prepared dictionary"): the arithmetic
// of its copies, shared by the match finder's lookup (enc_match.hip), the decoder
// (decode_core.inc use_dictionary) and a host program (tests/shared_dict_host_main.cpp, built
// with the sanitizers).  Plain C++: no HIP types.
//
// A copy of `length` bytes from dictionary address a (0 = the dictionary's first byte) written
// at a stream position whose window reaches `window` = min(position, max backward) bytes back
// has the distance window + (dict_len - a): the dictionary lies directly in front of the stream,
// its last byte one step beyond the window.  The decoder turns a distance beyond its max
// distance back into the address and accepts the copy when it stays inside the dictionary.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MIB_SD_FN __host__ __device__ inline
#else
#define MIB_SD_FN inline
#endif

namespace mib {
namespace sd {

// the longest copy the lookup offers (enc_common.h kLongCopy: the parse measures longer matches
// itself, by reading the stream at cur - distance, which a dictionary distance is not)
constexpr uint32_t kMaxCopy = 200;
// a match record's distance field: 24 bits, all ones taken (enc_common.h kCDictMark); with static
// words on, bit 23 as well (kDictFlag)
constexpr uint32_t kRecordDistLimit = 0xFFFFFFu;
constexpr uint32_t kRecordWordFlag = 1u << 23;

// the distance of a copy from address a at a position whose window is `window` bytes
MIB_SD_FN uint64_t distance_of(uint32_t window, uint32_t dict_len, uint32_t a) { return (uint64_t)window + (dict_len - a); }

// the decoder's side: distance > max_distance -> address; negative: inside the custom dictionary
// (at offset -address - 1), else a static-dictionary word's address
MIB_SD_FN int64_t address_of(int64_t distance, int64_t max_distance, int64_t dict_len) {
  return distance - max_distance - 1 - dict_len;
}
MIB_SD_FN int64_t offset_of(int64_t address) { return -address - 1; }

// the standard rule: the copy stays inside the dictionary
MIB_SD_FN bool copy_valid(int64_t a, int64_t length, int64_t dict_len) { return a >= 0 && length >= 0 && a + length <= dict_len; }
// (the decoder's form: 0 <= a < dict_len < 2^31 and a copy is shorter than 2^25 bytes, so the sum
// does not wrap)
MIB_SD_FN bool copy_valid_u32(uint32_t a, uint32_t length, uint32_t dict_len) { return a + length <= dict_len; }
// the reference decoder's rule (engine.ts:972-992): it ends at the dictionary's last byte
MIB_SD_FN bool copy_valid_tail(int64_t a, int64_t length, int64_t dict_len) { return a + length == dict_len; }

// whether a record may carry this distance (words: the stream also uses static-dictionary words)
MIB_SD_FN bool record_holds(uint64_t distance, bool words) {
  return distance < (words ? kRecordWordFlag : kRecordDistLimit);
}

// One candidate of the lookup, measured and capped: the length of the common prefix of cur[0,
// limit) and the dictionary from address a, at most dict_len - a (the bytes behind the
// dictionary are never compared: whatever they hold, a copy ends at its last byte), `limit` (the
// bytes left in the position's parse segment and stream) and kMaxCopy.
MIB_SD_FN uint32_t measure(const uint8_t *cur, uint32_t limit, const uint8_t *dict, uint32_t dict_len, uint32_t a) {
  if (a >= dict_len) return 0;
  uint32_t cap = dict_len - a;
  cap = cap < limit ? cap : limit;
  cap = cap < kMaxCopy ? cap : kMaxCopy;
  const uint8_t *s = dict + a;
  uint32_t m = 0;
  while (m < cap && cur[m] == s[m]) m++;
  return m;
}

}  // namespace sd
}  // namespace mib
