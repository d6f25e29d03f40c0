/*
 * brotli_amd.node -- Node-API binding of the brotli_amd C ABI (include/brotli_amd.h).
 *
 * This is the native half of the drop-in for countertype/brotli-lib's public surface
 * (package.json:7-23); index.js is the JavaScript half that keeps the reference's argument
 * handling and error messages.  Every function is synchronous on the JS thread, like the
 * reference's.  Result bytes are copied into a fresh Node Buffer and the library buffer
 * is released at once (mib_buf_free).
 */
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/brotli_amd.h"

#define CHECK(env, call)                                   \
  do {                                                     \
    if ((call) != napi_ok) {                               \
      napi_throw_error((env), NULL, "brotli_amd: N-API"); \
      return NULL;                                         \
    }                                                      \
  } while (0)

static int get_bytes(napi_env env, napi_value v, const uint8_t **p, size_t *n) {
  bool is_typed = false, is_buf = false;
  napi_is_typedarray(env, v, &is_typed);
  if (is_typed) {
    napi_typedarray_type t;
    size_t len, off;
    void *data;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off) != napi_ok) return -1;
    size_t el = (t == napi_uint8_array || t == napi_int8_array || t == napi_uint8_clamped_array) ? 1 : 0;
    if (!el) return -1;
    *p = (const uint8_t *)data;
    *n = len;
    return 0;
  }
  napi_is_buffer(env, v, &is_buf);
  if (is_buf) {
    void *data;
    if (napi_get_buffer_info(env, v, &data, n) != napi_ok) return -1;
    *p = (const uint8_t *)data;
    return 0;
  }
  return -1;
}

static napi_value throw_code(napi_env env, int code) {
  /* the reference's JS engine errors keep their type and message (engine.ts:998 subarray of
     a missing dictionary chunk; Uint8Array.set out of range) */
  if (code == MIB_E_JS_TYPE_ERROR) napi_throw_type_error(env, NULL, "Cannot read property 'subarray' of undefined");
  else if (code == MIB_E_JS_RANGE_ERROR) napi_throw_range_error(env, NULL, "offset is out of bounds");
  else napi_throw_error(env, NULL, mib_strerror(code));
  return NULL;
}

static napi_value take(napi_env env, mib_buf *b) {
  napi_value out;
  void *dst;
  if (napi_create_buffer_copy(env, b->size, b->size ? (const void *)b->data : (const void *)"", &dst, &out) != napi_ok) {
    mib_buf_free(b);
    napi_throw_error(env, NULL, "brotli_amd: out of host memory");
    return NULL;
  }
  mib_buf_free(b);
  return out;
}

static int get_int(napi_env env, napi_value v, int dflt) {
  napi_valuetype t;
  int32_t r;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return dflt;
  if (napi_get_value_int32(env, v, &r) != napi_ok) return dflt;
  return r;
}
static int64_t get_i64(napi_env env, napi_value v, int64_t dflt) {
  napi_valuetype t;
  int64_t r;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return dflt;
  if (napi_get_value_int64(env, v, &r) != napi_ok) return dflt;
  return r;
}

/* encode(bytes, quality, lgwin, mode, dictionary|null) -> Buffer */
static napi_value js_encode(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  mib_enc_opts o;
  mib_enc_opts_default(&o);
  o.quality = get_int(env, argc > 1 ? argv[1] : NULL, o.quality);
  o.lgwin = get_int(env, argc > 2 ? argv[2] : NULL, o.lgwin);
  o.mode = get_int(env, argc > 3 ? argv[3] : NULL, o.mode);
  size_t dn = 0;
  if (argc > 4 && get_bytes(env, argv[4], &o.dict, &dn) == 0) o.dict_len = dn;
  else o.dict = NULL;
  mib_buf b = {0, 0};
  int rc = mib_encode(p, n, &o, &b);
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}

/* decode(bytes, maxOutputSize|-1, exactSize|-1, dictionary|null) -> Buffer
 * throws Error("Brotli error code: N") or, for the size limit, an Error whose message
 * index.js rewrites; err.size carries the offending size. */
static napi_value js_decode(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p, *d = NULL;
  size_t n, dn = 0;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  int64_t max_out = argc > 1 ? get_i64(env, argv[1], -1) : -1;
  int64_t exact = argc > 2 ? get_i64(env, argv[2], -1) : -1;
  if (argc > 3 && get_bytes(env, argv[3], &d, &dn)) d = NULL;
  mib_buf b = {0, 0};
  int rc = mib_decode(p, n, d, d ? dn : 0, max_out, exact, &b);
  if (rc == MIB_E_OUTPUT_LIMIT) {
    napi_value err, msg, sz;
    napi_create_string_utf8(env, "Decompressed size exceeds limit", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int64(env, (int64_t)b.size, &sz);
    napi_set_named_property(env, err, "size", sz);
    napi_throw(env, err);
    return NULL;
  }
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}

static napi_value js_decoded_size(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  CHECK(env, napi_create_int64(env, mib_decoded_size(p, n), &out));
  return out;
}

static void encoder_finalize(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  mib_encoder_free((mib_encoder *)data);
}

static int get_dictionary(napi_env env, napi_value v, mib_dictionary **d);

/* encoderNew(quality, lgwin, mode, customDictionary|null, streamChunk, dictionary|null) -> external
 * handle (the encoder copies a customDictionary; of a BrotliDictionary it takes a reference of its
 * own, mib_encoder_new_dictionary, so the session outlives the dictionary's close()) */
static napi_value js_encoder_new(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  mib_enc_opts o;
  mib_enc_opts_default(&o);
  o.quality = get_int(env, argc > 0 ? argv[0] : NULL, o.quality);
  o.lgwin = get_int(env, argc > 1 ? argv[1] : NULL, o.lgwin);
  o.mode = get_int(env, argc > 2 ? argv[2] : NULL, o.mode);
  size_t dn = 0;
  if (argc > 3 && get_bytes(env, argv[3], &o.dict, &dn) == 0) o.dict_len = dn;
  else o.dict = NULL;
  const int64_t sc = argc > 4 ? get_i64(env, argv[4], 0) : 0;
  o.stream_chunk = sc > 0 ? (uint64_t)sc : 0;
  mib_dictionary *hd = NULL;
  if (argc > 5 && get_dictionary(env, argv[5], &hd)) return NULL;
  if (hd && o.dict) return throw_code(env, MIB_E_INVALID_ARG);
  mib_encoder *e = hd ? mib_encoder_new_dictionary(&o, hd) : mib_encoder_new(&o);
  if (!e) return throw_code(env, MIB_E_OUT_OF_MEMORY);
  CHECK(env, napi_create_external(env, e, encoder_finalize, NULL, &out));
  return out;
}

static napi_value js_encoder_update(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  const uint8_t *p;
  size_t n;
  if (argc < 2 || napi_get_value_external(env, argv[0], &h) != napi_ok || get_bytes(env, argv[1], &p, &n)) {
    napi_throw_type_error(env, NULL, "update(chunk: Uint8Array)");
    return NULL;
  }
  mib_buf b = {0, 0};
  int rc = mib_encoder_update((mib_encoder *)h, p, n, &b);
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}

static napi_value js_encoder_finish(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  if (argc < 1 || napi_get_value_external(env, argv[0], &h) != napi_ok) {
    napi_throw_type_error(env, NULL, "finish()");
    return NULL;
  }
  mib_buf b = {0, 0};
  int rc = mib_encoder_finish((mib_encoder *)h, &b);
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}

static void decoder_finalize(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  mib_decoder_free((mib_decoder *)data);
}

static napi_value throw_decoder(napi_env env, int rc, mib_buf *b) {
  if (rc == MIB_E_OUTPUT_LIMIT) {   /* as js_decode: index.js rewrites the message */
    napi_value err, msg, sz;
    napi_create_string_utf8(env, "Decompressed size exceeds limit", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int64(env, (int64_t)b->size, &sz);
    napi_set_named_property(env, err, "size", sz);
    napi_throw(env, err);
    return NULL;
  }
  return throw_code(env, rc);
}

/* decoderNew(customDictionary|null, maxOutputSize|-1, outWindow|0, dictionary|null) -> external
 * handle (the decoder copies a customDictionary; of a BrotliDictionary it takes a reference of its
 * own, mib_decoder_new_dictionary) */
static napi_value js_decoder_new(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  mib_dec_opts o;
  mib_dec_opts_default(&o);
  size_t dn = 0;
  if (argc > 0 && get_bytes(env, argv[0], &o.dict, &dn) == 0) o.dict_len = dn;
  else o.dict = NULL;
  const int64_t mo = argc > 1 ? get_i64(env, argv[1], -1) : -1;
  o.max_out = mo < 0 ? -1 : mo;
  const int64_t ow = argc > 2 ? get_i64(env, argv[2], 0) : 0;
  o.out_window = ow > 0 ? (uint64_t)ow : 0;
  mib_dictionary *hd = NULL;
  if (argc > 3 && get_dictionary(env, argv[3], &hd)) return NULL;
  if (hd && o.dict) return throw_code(env, MIB_E_INVALID_ARG);
  mib_decoder *d = hd ? mib_decoder_new_dictionary(&o, hd) : mib_decoder_new(&o);
  if (!d) return throw_code(env, MIB_E_OUT_OF_MEMORY);
  CHECK(env, napi_create_external(env, d, decoder_finalize, NULL, &out));
  return out;
}

static napi_value js_decoder_update(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  const uint8_t *p;
  size_t n;
  if (argc < 2 || napi_get_value_external(env, argv[0], &h) != napi_ok || get_bytes(env, argv[1], &p, &n)) {
    napi_throw_type_error(env, NULL, "update(chunk: Uint8Array)");
    return NULL;
  }
  mib_buf b = {0, 0};
  int rc = mib_decoder_update((mib_decoder *)h, p, n, &b);
  if (rc) return throw_decoder(env, rc, &b);
  return take(env, &b);
}

static napi_value js_decoder_finish(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  if (argc < 1 || napi_get_value_external(env, argv[0], &h) != napi_ok) {
    napi_throw_type_error(env, NULL, "finish()");
    return NULL;
  }
  mib_buf b = {0, 0};
  int rc = mib_decoder_finish((mib_decoder *)h, &b);
  if (rc) return throw_decoder(env, rc, &b);
  return take(env, &b);
}

static napi_value js_decoder_finished(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  if (argc < 1 || napi_get_value_external(env, argv[0], &h) != napi_ok) {
    napi_throw_type_error(env, NULL, "finished");
    return NULL;
  }
  CHECK(env, napi_get_boolean(env, mib_decoder_is_finished((const mib_decoder *)h) != 0, &out));
  return out;
}

/* a session's error as the BrotliDecoder methods throw it, as a value (the slot of a batch) */
static napi_value decoder_error(napi_env env, int rc, const mib_buf *b) {
  napi_value err = NULL, msg;
  if (rc == MIB_E_OUTPUT_LIMIT) {   /* index.js rewrites the message, as for update() */
    napi_value sz;
    napi_create_string_utf8(env, "Decompressed size exceeds limit", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int64(env, (int64_t)b->size, &sz);
    napi_set_named_property(env, err, "size", sz);
  } else if (rc == MIB_E_JS_TYPE_ERROR) {
    napi_create_string_utf8(env, "Cannot read property 'subarray' of undefined", NAPI_AUTO_LENGTH, &msg);
    napi_create_type_error(env, NULL, msg, &err);
  } else if (rc == MIB_E_JS_RANGE_ERROR) {
    napi_create_string_utf8(env, "offset is out of bounds", NAPI_AUTO_LENGTH, &msg);
    napi_create_range_error(env, NULL, msg, &err);
  } else {
    napi_create_string_utf8(env, mib_strerror(rc), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
  }
  return err;
}

/* decoderUpdateBatch([handle...], [bytes...]) / decoderFinishBatch([handle...]) -> one Buffer or
 * Error per session: the sessions advance in shared launches (mib_decoder_update_batch) */
static napi_value decoder_batch(napi_env env, napi_callback_info info, int finish) {
  size_t argc = 2;
  napi_value argv[2], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t k = 0, kc = 0;
  bool is_arr = false, is_arr2 = finish != 0;
  if (argc < (finish ? 1u : 2u) || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr ||
      (!finish && (napi_is_array(env, argv[1], &is_arr2) != napi_ok || !is_arr2))) {
    napi_throw_type_error(env, NULL, finish ? "decoderFinishBatch(decoders: BrotliDecoder[])"
                                            : "decoderUpdateBatch(decoders: BrotliDecoder[], chunks: Uint8Array[])");
    return NULL;
  }
  CHECK(env, napi_get_array_length(env, argv[0], &k));
  if (!finish) {
    CHECK(env, napi_get_array_length(env, argv[1], &kc));
    if (kc != k) {
      napi_throw_type_error(env, NULL, "decoderUpdateBatch: one chunk per decoder");
      return NULL;
    }
  }
  mib_decoder **hs = (mib_decoder **)calloc(k ? k : 1, sizeof(mib_decoder *));
  mib_span *in = (mib_span *)calloc(k ? k : 1, sizeof(mib_span));
  mib_buf *res = (mib_buf *)calloc(k ? k : 1, sizeof(mib_buf));
  int *st = (int *)calloc(k ? k : 1, sizeof(int));
  for (uint32_t i = 0; i < k; i++) {
    napi_value e;
    void *h = NULL;
    napi_get_element(env, argv[0], i, &e);
    int bad = napi_get_value_external(env, e, &h) != napi_ok || !h;
    if (!bad && !finish) {
      napi_get_element(env, argv[1], i, &e);
      bad = get_bytes(env, e, &in[i].data, &in[i].size);
    }
    if (bad) {
      free(hs), free(in), free(res), free(st);
      napi_throw_type_error(env, NULL, "decoder batch: BrotliDecoder handles and Uint8Array chunks");
      return NULL;
    }
    hs[i] = (mib_decoder *)h;
  }
  int rc = finish ? mib_decoder_finish_batch(hs, k, res, st) : mib_decoder_update_batch(hs, in, k, res, st);
  free(hs), free(in);
  if (rc) {
    free(res), free(st);
    return throw_code(env, rc);
  }
  napi_create_array_with_length(env, k, &out);
  for (uint32_t i = 0; i < k; i++) {
    napi_value v;
    if (st[i]) {
      v = decoder_error(env, st[i], &res[i]);
      mib_buf_free(&res[i]);
    } else {
      v = take(env, &res[i]);
    }
    if (!v) {
      for (uint32_t j = i + 1; j < k; j++) mib_buf_free(&res[j]);
      out = NULL;
      break;
    }
    napi_set_element(env, out, i, v);
  }
  free(res), free(st);
  return out;
}
static napi_value js_decoder_update_batch(napi_env env, napi_callback_info info) { return decoder_batch(env, info, 0); }
static napi_value js_decoder_finish_batch(napi_env env, napi_callback_info info) { return decoder_batch(env, info, 1); }

/* ---- a prepared dictionary (mib_dictionary): dictionaryNew(bytes) -> external handle, freed by
   dictionaryClose or, at the latest, when the handle is collected.  The box outlives the
   mib_dictionary so that a closed handle is refused instead of read. */
typedef struct { mib_dictionary *d; } DictBox;

static void dictionary_finalize(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  DictBox *b = (DictBox *)data;
  if (b->d) mib_dictionary_free(b->d);
  free(b);
}

/* the handle of an argument: 0 and *d = NULL for null / undefined, 0 and the handle, or -1 with
   an exception pending (not a handle, or closed) */
static int get_dictionary(napi_env env, napi_value v, mib_dictionary **d) {
  napi_valuetype t;
  *d = NULL;
  if (!v || napi_typeof(env, v, &t) != napi_ok || t == napi_null || t == napi_undefined) return 0;
  void *h;
  if (t != napi_external || napi_get_value_external(env, v, &h) != napi_ok) {
    napi_throw_type_error(env, NULL, "dictionary must be a BrotliDictionary");
    return -1;
  }
  if (!((DictBox *)h)->d) {
    napi_throw_error(env, NULL, "the BrotliDictionary is closed");
    return -1;
  }
  *d = ((DictBox *)h)->d;
  return 0;
}

static napi_value js_dictionary_new(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "new BrotliDictionary(data: Uint8Array)");
    return NULL;
  }
  DictBox *b = (DictBox *)calloc(1, sizeof(DictBox));
  if (!b) return throw_code(env, MIB_E_OUT_OF_MEMORY);
  int rc = mib_dictionary_new(p, n, &b->d);
  if (rc) {
    free(b);
    return throw_code(env, rc);
  }
  if (napi_create_external(env, b, dictionary_finalize, NULL, &out) != napi_ok) {
    dictionary_finalize(env, b, NULL);
    napi_throw_error(env, NULL, "brotli_amd: N-API");
    return NULL;
  }
  return out;
}

static napi_value js_dictionary_close(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  if (argc < 1 || napi_get_value_external(env, argv[0], &h) != napi_ok) {
    napi_throw_type_error(env, NULL, "close()");
    return NULL;
  }
  DictBox *b = (DictBox *)h;
  if (b->d) mib_dictionary_free(b->d);
  b->d = NULL;
  return NULL;
}

static napi_value js_dictionary_size(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *h;
  if (argc < 1 || napi_get_value_external(env, argv[0], &h) != napi_ok) {
    napi_throw_type_error(env, NULL, "size");
    return NULL;
  }
  CHECK(env, napi_create_int64(env, (int64_t)mib_dictionary_size(((DictBox *)h)->d), &out));
  return out;
}

/* a slot that failed: its Error (MIB_E_OUTPUT_LIMIT: err.size carries the offending size) */
static napi_value slot_error(napi_env env, int code, size_t size) {
  napi_value msg, err;
  napi_create_string_utf8(env, code == MIB_E_OUTPUT_LIMIT ? "Decompressed size exceeds limit" : mib_strerror(code), NAPI_AUTO_LENGTH,
                          &msg);
  napi_create_error(env, NULL, msg, &err);
  if (code == MIB_E_OUTPUT_LIMIT) {
    napi_value sz;
    napi_create_int64(env, (int64_t)size, &sz);
    napi_set_named_property(env, err, "size", sz);
  }
  return err;
}

/* decodeBatchDictionary([bytes...], dictionary, maxOutputSize|-1) -> [Buffer | Error ...]:
 * mib_decode_batch_dictionary, one result per slot */
static napi_value js_decode_batch_dictionary(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t k = 0;
  bool is_arr = false;
  mib_dictionary *d = NULL;
  if (argc < 2 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "decodeBatchDictionary(inputs: Uint8Array[], dictionary)");
    return NULL;
  }
  if (get_dictionary(env, argv[1], &d)) return NULL;
  CHECK(env, napi_get_array_length(env, argv[0], &k));
  const int64_t max_out = argc > 2 ? get_i64(env, argv[2], -1) : -1;
  mib_span *in = (mib_span *)calloc(k ? k : 1, sizeof(mib_span));
  mib_buf *res = (mib_buf *)calloc(k ? k : 1, sizeof(mib_buf));
  int *st = (int *)calloc(k ? k : 1, sizeof(int));
  if (!in || !res || !st) {
    free(in), free(res), free(st);
    return throw_code(env, MIB_E_OUT_OF_MEMORY);
  }
  for (uint32_t i = 0; i < k; i++) {
    napi_value e;
    napi_get_element(env, argv[0], i, &e);
    if (get_bytes(env, e, &in[i].data, &in[i].size)) {
      free(in), free(res), free(st);
      napi_throw_type_error(env, NULL, "every input must be a Uint8Array");
      return NULL;
    }
  }
  int rc = mib_decode_batch_dictionary(in, k, d, max_out, res, st);
  free(in);
  if (rc) {
    free(res), free(st);
    return throw_code(env, rc);
  }
  napi_create_array_with_length(env, k, &out);
  for (uint32_t i = 0; i < k; i++) {
    napi_value v;
    if (st[i]) {
      v = slot_error(env, st[i], res[i].size);
      res[i].data = NULL;
    } else {
      v = take(env, &res[i]);
      if (!v) break;
    }
    napi_set_element(env, out, i, v);
  }
  free(res);
  free(st);
  return out;
}

/* encodeBatch([bytes...], quality, lgwin, mode, gpus, customDictionary|null, dictionary|null) -> [Buffer...]: one GPU
 * launch sequence (gpus >= 0: sharded over that many GPUs, 0 = all; -1 / absent: the default
 * device) */
static napi_value js_encode_batch(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t k = 0;
  bool is_arr = false;
  if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "encodeBatch(inputs: Uint8Array[])");
    return NULL;
  }
  CHECK(env, napi_get_array_length(env, argv[0], &k));
  mib_enc_opts o;
  mib_enc_opts_default(&o);
  o.quality = get_int(env, argc > 1 ? argv[1] : NULL, o.quality);
  o.lgwin = get_int(env, argc > 2 ? argv[2] : NULL, o.lgwin);
  o.mode = get_int(env, argc > 3 ? argv[3] : NULL, o.mode);
  size_t dn = 0;
  if (argc > 5 && get_bytes(env, argv[5], &o.dict, &dn) == 0) o.dict_len = dn;
  else o.dict = NULL;
  mib_dictionary *hd = NULL;   /* a BrotliDictionary: mib_encode_batch_dictionary */
  if (argc > 6 && get_dictionary(env, argv[6], &hd)) return NULL;
  mib_span *in = (mib_span *)calloc(k ? k : 1, sizeof(mib_span));
  mib_buf *res = (mib_buf *)calloc(k ? k : 1, sizeof(mib_buf));
  int *st = (int *)calloc(k ? k : 1, sizeof(int));
  for (uint32_t i = 0; i < k; i++) {
    napi_value e;
    napi_get_element(env, argv[0], i, &e);
    if (get_bytes(env, e, &in[i].data, &in[i].size)) {
      free(in), free(res), free(st);
      napi_throw_type_error(env, NULL, "encodeBatch: every input must be a Uint8Array");
      return NULL;
    }
  }
  const int gpus = argc > 4 ? get_int(env, argv[4], -1) : -1;
  int rc = hd ? mib_encode_batch_dictionary(in, k, &o, hd, res, st)
              : gpus >= 0 ? mib_encode_batch_n(in, k, &o, gpus, res, st) : mib_encode_batch(in, k, &o, res, st);
  free(in);
  if (rc) {
    free(res), free(st);
    return throw_code(env, rc);
  }
  napi_create_array_with_length(env, k, &out);
  for (uint32_t i = 0; i < k; i++) {
    napi_value v = take(env, &res[i]);
    if (!v) break;
    napi_set_element(env, out, i, v);
  }
  free(res);
  free(st);
  return out;
}

/* ---- asynchronous batches: the GPU work runs on a libuv worker thread (napi_async_work),
   the JS thread gets a Promise.  The inputs are COPIED into memory the addon owns before the
   work is queued: JS may transfer or detach an ArrayBuffer while the Promise is pending, and
   the worker must never read a buffer the JS heap has let go of. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  uint32_t k;
  int decode;       /* 0: encode batch, 1: decode batch */
  int gpus;         /* >= 0: sharded over that many GPUs (0 = all), else the default device */
  mib_enc_opts o;
  uint8_t *blob;    /* the inputs, back to back (owned) */
  uint8_t *dict;    /* encode: the customDictionary (owned copy), or NULL */
  mib_dictionary *hd;   /* a BrotliDictionary's handle, or NULL: the *_dictionary calls */
  napi_ref hd_ref;      /* ... kept alive until the work has settled */
  int64_t max_out;      /* decode with a handle: maxOutputSize, -1 none */
  mib_span *in;
  mib_buf *res;
  int *st;
  int rc;
} AsyncBatch;

static void async_free(AsyncBatch *a) {
  free(a->blob), free(a->dict), free(a->in), free(a->res), free(a->st), free(a);
}

static void async_execute(napi_env env, void *data) {
  AsyncBatch *a = (AsyncBatch *)data;
  if (a->hd)
    a->rc = a->decode ? mib_decode_batch_dictionary(a->in, a->k, a->hd, a->max_out, a->res, a->st)
                      : mib_encode_batch_dictionary(a->in, a->k, &a->o, a->hd, a->res, a->st);
  else if (a->gpus >= 0)
    a->rc = a->decode ? mib_decode_batch_n(a->in, a->k, a->gpus, a->res, a->st)
                      : mib_encode_batch_n(a->in, a->k, &a->o, a->gpus, a->res, a->st);
  else
    a->rc = a->decode ? mib_decode_batch(a->in, a->k, a->res, a->st) : mib_encode_batch(a->in, a->k, &a->o, a->res, a->st);
}

static void async_complete(napi_env env, napi_status status, void *data) {
  AsyncBatch *a = (AsyncBatch *)data;
  napi_value out, err;
  if (a->rc == 0 && status == napi_ok) {
    napi_create_array_with_length(env, a->k, &out);
    for (uint32_t i = 0; i < a->k; i++) {
      napi_value v;
      if (a->st[i]) {   /* a stream that failed to decode: its Error, in its slot */
        v = slot_error(env, a->st[i], a->res[i].size);
        if (a->st[i] == MIB_E_OUTPUT_LIMIT) a->res[i].data = NULL;   /* (no data: the size alone) */
        mib_buf_free(&a->res[i]);
      } else {
        void *dst;
        napi_create_buffer_copy(env, a->res[i].size, a->res[i].size ? (const void *)a->res[i].data : (const void *)"", &dst, &v);
        mib_buf_free(&a->res[i]);
      }
      napi_set_element(env, out, i, v);
    }
    napi_resolve_deferred(env, a->deferred, out);
  } else {
    napi_value msg;
    napi_create_string_utf8(env, mib_strerror(a->rc ? a->rc : MIB_E_NO_DEVICE), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, a->deferred, err);
    for (uint32_t i = 0; i < a->k; i++) mib_buf_free(&a->res[i]);
  }
  if (a->hd_ref) napi_delete_reference(env, a->hd_ref);
  napi_delete_async_work(env, a->work);
  async_free(a);
}

/* encodeBatchAsync(inputs, quality, lgwin, mode, gpus, customDictionary|null, dictionary|null) /
 * decodeBatchAsync(inputs, gpus, dictionary|null, maxOutputSize|-1) -> Promise */
static napi_value start_async(napi_env env, napi_callback_info info, int decode) {
  size_t argc = 7;
  napi_value argv[7], promise, name;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool is_arr = false;
  uint32_t k = 0;
  if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "inputs: Uint8Array[]");
    return NULL;
  }
  CHECK(env, napi_get_array_length(env, argv[0], &k));
  const size_t hd_arg = decode ? 2 : 6;
  mib_dictionary *hd = NULL;
  if (argc > hd_arg && get_dictionary(env, argv[hd_arg], &hd)) return NULL;
  AsyncBatch *a = (AsyncBatch *)calloc(1, sizeof(AsyncBatch));
  a->k = k;
  a->decode = decode;
  a->hd = hd;
  a->max_out = decode && argc > 3 ? get_i64(env, argv[3], -1) : -1;
  a->gpus = decode ? (argc > 1 ? get_int(env, argv[1], -1) : -1) : (argc > 4 ? get_int(env, argv[4], -1) : -1);
  mib_enc_opts_default(&a->o);
  if (!decode) {
    a->o.quality = get_int(env, argc > 1 ? argv[1] : NULL, a->o.quality);
    a->o.lgwin = get_int(env, argc > 2 ? argv[2] : NULL, a->o.lgwin);
    a->o.mode = get_int(env, argc > 3 ? argv[3] : NULL, a->o.mode);
    const uint8_t *d;
    size_t dn;
    if (argc > 5 && get_bytes(env, argv[5], &d, &dn) == 0 && dn) {   /* (copied: JS may detach it) */
      a->dict = (uint8_t *)malloc(dn);
      if (!a->dict) {
        free(a);
        return throw_code(env, MIB_E_OUT_OF_MEMORY);
      }
      memcpy(a->dict, d, dn);
      a->o.dict = a->dict;
      a->o.dict_len = dn;
    }
  }
  a->in = (mib_span *)calloc(k ? k : 1, sizeof(mib_span));
  a->res = (mib_buf *)calloc(k ? k : 1, sizeof(mib_buf));
  a->st = (int *)calloc(k ? k : 1, sizeof(int));
  if (!a->in || !a->res || !a->st) {
    async_free(a);
    return throw_code(env, MIB_E_OUT_OF_MEMORY);
  }
  size_t total = 0;
  for (int pass = 0; pass < 2; pass++) {   /* sizes, then the copies */
    size_t at = 0;
    for (uint32_t i = 0; i < k; i++) {
      napi_value e;
      const uint8_t *p;
      size_t n;
      napi_get_element(env, argv[0], i, &e);
      if (get_bytes(env, e, &p, &n)) {
        async_free(a);
        napi_throw_type_error(env, NULL, "every input must be a Uint8Array");
        return NULL;
      }
      if (pass) {
        if (n) memcpy(a->blob + at, p, n);
        a->in[i].data = a->blob + at;
        a->in[i].size = n;
      }
      at += n;
    }
    if (!pass) {
      total = at;
      a->blob = (uint8_t *)malloc(total ? total : 1);
      if (!a->blob) {
        async_free(a);
        return throw_code(env, MIB_E_OUT_OF_MEMORY);
      }
    }
  }
  /* the handle's external stays referenced while the worker uses it (index.js also defers a
     close() asked for meanwhile) */
  if (hd && napi_create_reference(env, argv[hd_arg], 1, &a->hd_ref) != napi_ok) {
    async_free(a);
    napi_throw_error(env, NULL, "brotli_amd: N-API");
    return NULL;
  }
  CHECK(env, napi_create_promise(env, &a->deferred, &promise));
  napi_create_string_utf8(env, decode ? "brotli_amd.decodeBatch" : "brotli_amd.encodeBatch", NAPI_AUTO_LENGTH, &name);
  CHECK(env, napi_create_async_work(env, NULL, name, async_execute, async_complete, a, &a->work));
  CHECK(env, napi_queue_async_work(env, a->work));
  return promise;
}
/* woff2Glyf(ttf) / woff2Hmtx(ttf) -> Buffer: the WOFF2-transformed glyf / hmtx table computed on
 * the GPU (the FONT-mode input of encode for a WOFF2 writer, reference README.md:63); hmtx
 * gives null when no transform applies */
static napi_value js_woff2(napi_env env, napi_callback_info info, int hmtx) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  mib_buf b = {0, 0};
  const int rc = hmtx ? mib_woff2_transform_hmtx(p, n, &b) : mib_woff2_transform_glyf(p, n, &b);
  if (rc) return throw_code(env, rc);
  if (hmtx && !b.size) {
    napi_value nul;
    CHECK(env, napi_get_null(env, &nul));
    return nul;
  }
  return take(env, &b);
}
static napi_value js_woff2_glyf(napi_env env, napi_callback_info info) { return js_woff2(env, info, 0); }
static napi_value js_woff2_hmtx(napi_env env, napi_callback_info info) { return js_woff2(env, info, 1); }
/* woff2File(data) -> Buffer: the sfnt a .woff2 file stands for, decoded, reconstructed and
 * assembled on the GPU; a file that does not parse throws (MIB_E_INVALID_ARG, or the decoder's
 * code for its Brotli stream) */
static napi_value js_woff2_file(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  mib_buf b = {0, 0};
  const int rc = mib_woff2_decode(p, n, &b);
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}
/* woff2FileBatch([bytes...]) -> one Buffer or Error per file: the files' Brotli streams decode
 * in shared launches and their sfnts are assembled in shared launches (mib_woff2_decode_batch) */
static napi_value js_woff2_file_batch(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t k = 0;
  bool is_arr = false;
  if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "woff2DecodeBatch(files: Uint8Array[])");
    return NULL;
  }
  CHECK(env, napi_get_array_length(env, argv[0], &k));
  mib_span *in = (mib_span *)calloc(k ? k : 1, sizeof(mib_span));
  mib_buf *res = (mib_buf *)calloc(k ? k : 1, sizeof(mib_buf));
  int *st = (int *)calloc(k ? k : 1, sizeof(int));
  for (uint32_t i = 0; i < k; i++) {
    napi_value e;
    napi_get_element(env, argv[0], i, &e);
    if (get_bytes(env, e, &in[i].data, &in[i].size)) {
      free(in), free(res), free(st);
      napi_throw_type_error(env, NULL, "every file must be a Uint8Array");
      return NULL;
    }
    if (!in[i].size) in[i].data = NULL;
  }
  const int rc = mib_woff2_decode_batch(in, k, res, st);
  free(in);
  if (rc) {
    free(res), free(st);
    return throw_code(env, rc);
  }
  napi_create_array_with_length(env, k, &out);
  for (uint32_t i = 0; i < k; i++) {
    napi_value v = st[i] ? decoder_error(env, st[i], &res[i]) : take(env, &res[i]);
    if (!v) {
      for (uint32_t j = i + 1; j < k; j++) mib_buf_free(&res[j]);
      out = NULL;
      break;
    }
    napi_set_element(env, out, i, v);
  }
  free(res), free(st);
  return out;
}
/* woff2Write(sfnt, quality, lgwin, transforms) -> Buffer: the .woff2 file of a single-font sfnt,
 * written on the GPU (mib_woff2_encode); a font that does not parse throws (MIB_E_INVALID_ARG) */
static void woff2_enc_opts(napi_env env, size_t argc, napi_value *argv, mib_woff2_enc_opts *o) {
  o->quality = get_int(env, argc > 1 ? argv[1] : NULL, 11);
  o->lgwin = get_int(env, argc > 2 ? argv[2] : NULL, 22);
  o->transforms = (uint32_t)get_i64(env, argc > 3 ? argv[3] : NULL, MIB_WOFF2_GLYF | MIB_WOFF2_HMTX);
}
static napi_value js_woff2_write(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  mib_woff2_enc_opts o;
  woff2_enc_opts(env, argc, argv, &o);
  mib_buf b = {0, 0};
  const int rc = mib_woff2_encode(n ? p : NULL, n, &o, &b);
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}
/* woff2WriteBatch([bytes...], quality, lgwin, transforms) -> one Buffer or Error per font: the
 * fonts are uploaded, copied and compressed in shared launches (mib_woff2_encode_batch) */
static napi_value js_woff2_write_batch(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t k = 0;
  bool is_arr = false;
  if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "woff2EncodeBatch(sfnts: Uint8Array[], options?)");
    return NULL;
  }
  CHECK(env, napi_get_array_length(env, argv[0], &k));
  mib_woff2_enc_opts o;
  woff2_enc_opts(env, argc, argv, &o);
  mib_span *in = (mib_span *)calloc(k ? k : 1, sizeof(mib_span));
  mib_buf *res = (mib_buf *)calloc(k ? k : 1, sizeof(mib_buf));
  int *st = (int *)calloc(k ? k : 1, sizeof(int));
  for (uint32_t i = 0; i < k; i++) {
    napi_value e;
    napi_get_element(env, argv[0], i, &e);
    if (get_bytes(env, e, &in[i].data, &in[i].size)) {
      free(in), free(res), free(st);
      napi_throw_type_error(env, NULL, "every font must be a Uint8Array");
      return NULL;
    }
    if (!in[i].size) in[i].data = NULL;
  }
  const int rc = mib_woff2_encode_batch(in, k, &o, res, st);
  free(in);
  if (rc) {
    free(res), free(st);
    return throw_code(env, rc);
  }
  napi_create_array_with_length(env, k, &out);
  for (uint32_t i = 0; i < k; i++) {
    napi_value v = st[i] ? decoder_error(env, st[i], &res[i]) : take(env, &res[i]);
    if (!v) {
      for (uint32_t j = i + 1; j < k; j++) mib_buf_free(&res[j]);
      out = NULL;
      break;
    }
    napi_set_element(env, out, i, v);
  }
  free(res), free(st);
  return out;
}
/* woff2InvGlyf(data) -> [glyf, loca] (Buffers): the TrueType tables of a WOFF2-transformed glyf
 * table, computed on the GPU; a table that does not parse throws (MIB_E_INVALID_ARG) */
static napi_value js_woff2_inv_glyf(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p;
  size_t n;
  if (argc < 1 || get_bytes(env, argv[0], &p, &n)) {
    napi_throw_type_error(env, NULL, "input must be a Uint8Array");
    return NULL;
  }
  mib_buf glyf = {0, 0}, loca = {0, 0};
  const int rc = mib_woff2_reconstruct_glyf(p, n, &glyf, &loca);
  if (rc) return throw_code(env, rc);
  napi_value arr, g, l;
  g = take(env, &glyf);
  if (!g) {
    mib_buf_free(&loca);
    return NULL;
  }
  l = take(env, &loca);
  if (!l) return NULL;
  CHECK(env, napi_create_array_with_length(env, 2, &arr));
  CHECK(env, napi_set_element(env, arr, 0, g));
  CHECK(env, napi_set_element(env, arr, 1, l));
  return arr;
}
/* woff2InvHmtx(data, glyf, loca, numGlyphs, numHMetrics) -> Buffer: the hmtx table of a
 * WOFF2-transformed one, the dropped side bearings from the glyphs' xMin */
static napi_value js_woff2_inv_hmtx(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const uint8_t *p[3];
  size_t n[3];
  if (argc < 5 || get_bytes(env, argv[0], &p[0], &n[0]) || get_bytes(env, argv[1], &p[1], &n[1]) ||
      get_bytes(env, argv[2], &p[2], &n[2])) {
    napi_throw_type_error(env, NULL, "data, glyf and loca must be Uint8Arrays");
    return NULL;
  }
  const int64_t ng = get_i64(env, argv[3], -1), nhm = get_i64(env, argv[4], -1);
  if (ng < 0 || nhm < 0 || ng > 0xFFFFFFFFll || nhm > 0xFFFFFFFFll) return throw_code(env, MIB_E_INVALID_ARG);
  mib_buf b = {0, 0};
  const int rc = mib_woff2_reconstruct_hmtx(p[0], n[0], p[1], n[1], p[2], n[2], (uint32_t)ng, (uint32_t)nhm, &b);
  if (rc) return throw_code(env, rc);
  return take(env, &b);
}
static napi_value js_encode_batch_async(napi_env env, napi_callback_info info) { return start_async(env, info, 0); }
static napi_value js_decode_batch_async(napi_env env, napi_callback_info info) { return start_async(env, info, 1); }

static napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"encode", 0, js_encode, 0, 0, 0, napi_default, 0},
      {"decode", 0, js_decode, 0, 0, 0, napi_default, 0},
      {"decodedSize", 0, js_decoded_size, 0, 0, 0, napi_default, 0},
      {"encoderNew", 0, js_encoder_new, 0, 0, 0, napi_default, 0},
      {"encoderUpdate", 0, js_encoder_update, 0, 0, 0, napi_default, 0},
      {"encoderFinish", 0, js_encoder_finish, 0, 0, 0, napi_default, 0},
      {"decoderNew", 0, js_decoder_new, 0, 0, 0, napi_default, 0},
      {"decoderUpdate", 0, js_decoder_update, 0, 0, 0, napi_default, 0},
      {"decoderFinish", 0, js_decoder_finish, 0, 0, 0, napi_default, 0},
      {"decoderFinished", 0, js_decoder_finished, 0, 0, 0, napi_default, 0},
      {"decoderUpdateBatch", 0, js_decoder_update_batch, 0, 0, 0, napi_default, 0},
      {"decoderFinishBatch", 0, js_decoder_finish_batch, 0, 0, 0, napi_default, 0},
      {"dictionaryNew", 0, js_dictionary_new, 0, 0, 0, napi_default, 0},
      {"dictionaryClose", 0, js_dictionary_close, 0, 0, 0, napi_default, 0},
      {"dictionarySize", 0, js_dictionary_size, 0, 0, 0, napi_default, 0},
      {"decodeBatchDictionary", 0, js_decode_batch_dictionary, 0, 0, 0, napi_default, 0},
      {"encodeBatch", 0, js_encode_batch, 0, 0, 0, napi_default, 0},
      {"encodeBatchAsync", 0, js_encode_batch_async, 0, 0, 0, napi_default, 0},
      {"decodeBatchAsync", 0, js_decode_batch_async, 0, 0, 0, napi_default, 0},
      {"woff2Glyf", 0, js_woff2_glyf, 0, 0, 0, napi_default, 0},
      {"woff2Hmtx", 0, js_woff2_hmtx, 0, 0, 0, napi_default, 0},
      {"woff2InvGlyf", 0, js_woff2_inv_glyf, 0, 0, 0, napi_default, 0},
      {"woff2InvHmtx", 0, js_woff2_inv_hmtx, 0, 0, 0, napi_default, 0},
      {"woff2File", 0, js_woff2_file, 0, 0, 0, napi_default, 0},
      {"woff2FileBatch", 0, js_woff2_file_batch, 0, 0, 0, napi_default, 0},
      {"woff2Write", 0, js_woff2_write, 0, 0, 0, napi_default, 0},
      {"woff2WriteBatch", 0, js_woff2_write_batch, 0, 0, 0, napi_default, 0},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
