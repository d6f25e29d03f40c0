// mib_dictionary (brotli_amd.h): a prepared dictionary on the default context's device.  Made
// and freed in encode.hip (the index kernel is the match finder's), read by encode.hip's and
// runtime.cpp's batch calls and by the sessions made with it (mib_encoder_new_dictionary,
// mib_decoder_new_dictionary).  Immutable once mib_dictionary_new has returned, but for its
// reference count.
#pragma once
#include <stdint.h>

#include <atomic>

struct mib_dictionary {
  uint8_t *d_data = nullptr;   // the bytes, kPad zero bytes behind them
  uint64_t n = 0;
  // the index per key length (enc_common.h kCDictWays): 4-byte keys (FONT mode), 6-byte keys
  // (GENERIC / TEXT); null where the dictionary is shorter than the key
  uint32_t *tab4 = nullptr, *tab6 = nullptr;
  int device = 0;
  // mib_dictionary_new's reference (dropped by mib_dictionary_free) and one per session made with
  // the handle (dropped by mib_encoder_free / mib_decoder_free); the device memory goes with the last
  std::atomic<int> refs{1};
  static constexpr uint64_t kPad = 64;
};

// internal (encode.hip): a session takes / drops its reference.  The last drop frees the device
// memory under the default context's lock, so the caller must not be inside a device call of its
// own that still reads the handle.
extern "C" void mib_dictionary_ref(const mib_dictionary *d);
extern "C" void mib_dictionary_unref(const mib_dictionary *d);
