// mib_dictionary (brotli_amd.h): a prepared dictionary on the default context's device.  Made
// and freed in encode.hip (the index kernel is the match finder's), read by encode.hip's and
// runtime.cpp's batch calls.  Immutable once mib_dictionary_new has returned.
#pragma once
#include <stdint.h>

struct mib_dictionary {
  uint8_t *d_data = nullptr;   // the bytes, kPad zero bytes behind them
  uint64_t n = 0;
  // the index per key length (enc_common.h kCDictWays): 4-byte keys (FONT mode), 6-byte keys
  // (GENERIC / TEXT); null where the dictionary is shorter than the key
  uint32_t *tab4 = nullptr, *tab6 = nullptr;
  int device = 0;
  static constexpr uint64_t kPad = 64;
};
