'use strict'
// brotli_amd for Node: the public surface of countertype/brotli-lib (package.json:7-23)
// over the MI355X engine.  Argument handling and error messages follow the reference:
//   brotliEncode(input, {quality, lgwin, mode, sizeHint})    src/encode/encode.ts:50-90
//   new BrotliEncoder(options).update(chunk) / .finish()     src/encode/encode.ts:290-409
//   brotliDecode(data, {maxOutputSize, customDictionary} | outputSize)
//                                                            src/decode/decode.ts:18-65
//   brotliDecodedSize(data)                                  src/decode/decode.ts:9-11
//   new BrotliDecoder(options).update(chunk) / .finish() / .finished
//                                                            extension: streaming decode
//   EncoderMode                                              src/encode/enc-constants.ts:56-60
// The addon (brotli_amd.node) is built by __graft_entry__.build(); there is no JavaScript
// fallback, a missing GPU throws.
const path = require('path')
const native = require(path.join(__dirname, 'brotli_amd.node'))

const EncoderMode = Object.freeze({ GENERIC: 0, TEXT: 1, FONT: 2 })

function clampOptions(options) {
  const o = options || {}
  let quality = 11
  let lgwin = 22
  let mode = EncoderMode.GENERIC
  if (o.quality !== undefined) quality = Math.max(0, Math.min(11, o.quality))
  if (o.lgwin !== undefined) lgwin = Math.max(10, Math.min(24, o.lgwin))
  if (o.mode !== undefined) mode = o.mode
  return [quality | 0, lgwin | 0, mode | 0]
}

// customDictionary (extension, the encoder side of brotliDecode's option): Uint8Array / Int8Array
function dictOf(options) {
  const d = options && options.customDictionary
  if (!d) return null
  return d instanceof Uint8Array ? d : new Uint8Array(d.buffer, d.byteOffset, d.byteLength)
}

function toU8(b) {
  return new Uint8Array(b.buffer, b.byteOffset, b.byteLength)
}

// BrotliDictionary (extension; brotli_amd.h mib_dictionary): shared bytes uploaded to the GPU and
// indexed there once.  Pass it as options.dictionary to brotliEncode, brotliEncodeBatch,
// brotliEncodeBatchAsync, brotliDecode and brotliDecodeBatchAsync, and to new BrotliEncoder /
// new BrotliDecoder.  Copies may come from anywhere in it, so a stream written with one decodes
// with one of the same bytes (not with customDictionary).  close() drops this object's reference
// to the device memory; while an async call that uses the dictionary is pending, close() waits
// for it to settle.  A BrotliEncoder / BrotliDecoder made with the dictionary holds a reference
// of its own: it keeps working after close(), and the memory goes with the last of them.
// size: the dictionary's length.
class BrotliDictionary {
  constructor(data) {
    const d = data instanceof Uint8Array ? data : new Uint8Array(data.buffer, data.byteOffset, data.byteLength)
    this._h = native.dictionaryNew(d)
    this._size = d.length
    this._pending = 0
    this._closing = false
  }
  get size() {
    return this._size
  }
  get closed() {
    return this._h === null
  }
  close() {
    if (this._h === null) return
    if (this._pending > 0) {
      this._closing = true
      return
    }
    native.dictionaryClose(this._h)
    this._h = null
  }
}
// options.dictionary's handle (null: none); both kinds of dictionary at once is an error
function handleOf(options) {
  const d = options && options.dictionary
  if (d === undefined || d === null) return null
  if (!(d instanceof BrotliDictionary)) throw new TypeError('dictionary must be a BrotliDictionary')
  if (options.customDictionary) throw new Error('dictionary and customDictionary exclude each other')
  if (d._h === null || d._closing) throw new Error('the BrotliDictionary is closed')
  return d
}
// an async call holds the dictionary until it settles
function holding(d, promise) {
  if (!d) return promise
  d._pending++
  const release = () => {
    if (--d._pending === 0 && d._closing) {
      d._closing = false
      d.close()
    }
  }
  return promise.then((v) => { release(); return v }, (e) => { release(); throw e })
}
function limitError(o, maxOutputSize) {
  return o.size !== undefined ? new Error(`Decompressed size ${o.size} exceeds limit ${maxOutputSize}`) : o
}

function brotliEncode(input, options) {
  const [q, lg, m] = clampOptions(options)
  const hd = handleOf(options)
  if (hd) return toU8(native.encodeBatch([input], q, lg, m, -1, null, hd._h)[0])   // the batch with k = 1
  return toU8(native.encode(input, q, lg, m, dictOf(options)))
}

class BrotliEncoder {
  constructor(options) {
    const [q, lg, m] = clampOptions(options)
    // options.streamChunk (extension): throughput mode, see brotli_amd.h mib_enc_opts.stream_chunk
    const sc = options && options.streamChunk ? Math.max(0, options.streamChunk) : 0
    // options.dictionary (extension): a BrotliDictionary, errors as brotliEncode's; the session
    // copies from anywhere in it and its stream decodes with new BrotliDecoder({dictionary})
    const hd = handleOf(options)
    this._dictionary = hd
    this._h = native.encoderNew(q, lg, m, hd ? null : dictOf(options), sc, hd ? hd._h : null)
  }
  update(input) {
    return toU8(native.encoderUpdate(this._h, input))
  }
  finish() {
    return toU8(native.encoderFinish(this._h))
  }
}

function brotliDecodedSize(buffer) {
  return native.decodedSize(buffer)
}

function brotliDecode(buffer, options) {
  let exact = -1
  let maxOutputSize
  let dict = null
  if (typeof options === 'number') {
    exact = options
  } else if (options) {
    const hd = handleOf(options)
    if (hd) {   // the batch with k = 1
      const max = options.maxOutputSize
      const r = native.decodeBatchDictionary([buffer], hd._h, max === undefined ? -1 : max)[0]
      if (r instanceof Error) throw limitError(r, max)
      return toU8(r)
    }
    maxOutputSize = options.maxOutputSize
    const d = options.customDictionary
    if (d) dict = d instanceof Uint8Array ? d : new Uint8Array(d.buffer, d.byteOffset, d.byteLength)
  }
  try {
    return toU8(native.decode(buffer, maxOutputSize === undefined ? -1 : maxOutputSize, exact, dict))
  } catch (e) {
    if (e && e.size !== undefined) throw new Error(`Decompressed size ${e.size} exceeds limit ${maxOutputSize}`)
    throw e
  }
}

// BrotliDecoder (extension: the reference decodes in one shot only): the decode side of
// BrotliEncoder.  update(chunk) takes the next bytes of one stream, cut anywhere, and returns
// the bytes they complete; finish() declares the input ended and returns the rest, or throws
// the decoder's error for an incomplete stream; finished: the last metablock is decoded.
// options: customDictionary, maxOutputSize (total), outWindow (output bytes per device pass),
// dictionary (a BrotliDictionary, not with customDictionary: copies from anywhere in it).
class BrotliDecoder {
  constructor(options) {
    const o = options || {}
    const hd = handleOf(o)
    this._dictionary = hd
    const d = o.customDictionary
    const dict = d ? (d instanceof Uint8Array ? d : new Uint8Array(d.buffer, d.byteOffset, d.byteLength)) : null
    this._max = o.maxOutputSize
    this._h = native.decoderNew(dict, o.maxOutputSize === undefined ? -1 : o.maxOutputSize, o.outWindow ? Math.max(0, o.outWindow) : 0,
      hd ? hd._h : null)
  }
  _call(f, ...args) {
    try {
      return toU8(f(this._h, ...args))
    } catch (e) {
      if (e && e.size !== undefined) throw new Error(`Decompressed size ${e.size} exceeds limit ${this._max}`)
      throw e
    }
  }
  update(input) {
    return this._call(native.decoderUpdate, input)
  }
  finish() {
    return this._call(native.decoderFinish)
  }
  get finished() {
    return native.decoderFinished(this._h)
  }
}

// Many BrotliDecoder sessions advanced by one chunk each in shared launches (a round is one
// decode launch over every session that still has work).  One result per slot: the bytes
// decoder.update(chunk) / decoder.finish() alone would have returned, or the Error it would have
// thrown (not thrown here: the other sessions go on).  The decoders must be distinct.
function decoderSlots(decoders, outs) {
  return outs.map((o, i) => {
    if (!(o instanceof Error)) return toU8(o)
    return o.size !== undefined ? new Error(`Decompressed size ${o.size} exceeds limit ${decoders[i]._max}`) : o
  })
}
function brotliDecoderUpdateBatch(decoders, chunks) {
  return decoderSlots(decoders, native.decoderUpdateBatch(decoders.map((d) => d._h), chunks))
}
function brotliDecoderFinishBatch(decoders) {
  return decoderSlots(decoders, native.decoderFinishBatch(decoders.map((d) => d._h)))
}

// options.gpus: shard the batch over that many GPUs (0: every visible one); absent: one GPU
function gpusOf(options) {
  const g = options && options.gpus
  return g === undefined || g === null ? -1 : Math.max(0, g | 0)
}

// batch entry point of this engine: independent buffers in one GPU launch sequence
function brotliEncodeBatch(inputs, options) {
  const [q, lg, m] = clampOptions(options)
  const hd = handleOf(options)
  return native.encodeBatch(inputs, q, lg, m, gpusOf(options), dictOf(options), hd ? hd._h : null).map(toU8)
}

// the same, off the JS thread: the GPU work runs on a worker (napi_async_work), a Promise
// resolves to the outputs (decode: a stream that fails gives its Error in its slot)
function brotliEncodeBatchAsync(inputs, options) {
  const [q, lg, m] = clampOptions(options)
  const hd = handleOf(options)
  return holding(hd, native.encodeBatchAsync(inputs, q, lg, m, gpusOf(options), dictOf(options), hd ? hd._h : null))
    .then((outs) => outs.map(toU8))
}
// options.dictionary: the streams were written with that BrotliDictionary; options.maxOutputSize
// then applies to every stream (its slot gets the Error)
function brotliDecodeBatchAsync(inputs, options) {
  const hd = handleOf(options)
  const max = hd && options.maxOutputSize !== undefined ? options.maxOutputSize : -1
  return holding(hd, native.decodeBatchAsync(inputs, gpusOf(options), hd ? hd._h : null, max))
    .then((outs) => outs.map((o) => (o instanceof Error ? limitError(o, max) : toU8(o))))
}

// the FONT-mode caller's step before brotliEncode (reference README.md:63): the WOFF2
// transformed 'glyf' / 'hmtx' tables of a TrueType font, computed on the GPU
function woff2TransformGlyf(ttf) {
  return toU8(native.woff2Glyf(ttf))
}
function woff2TransformHmtx(ttf) {
  const r = native.woff2Hmtx(ttf)
  return r === null ? null : toU8(r)
}
// the WOFF2 reader's step after brotliDecode: the TrueType glyf / loca / hmtx tables of the
// transformed ones, computed on the GPU (the bytes fontTools reconstructs)
function woff2ReconstructGlyf(data) {
  const [glyf, loca] = native.woff2InvGlyf(data)
  return { glyf: toU8(glyf), loca: toU8(loca) }
}
function woff2ReconstructHmtx(data, glyf, loca, numGlyphs, numHMetrics) {
  return toU8(native.woff2InvHmtx(data, glyf, loca, numGlyphs, numHMetrics))
}
// a whole .woff2 file (single font) -> its sfnt: Brotli decode, reconstruction and assembly
// (records by tag, checksums, head's checkSumAdjustment) on the GPU; throws on a file that
// does not parse
function woff2Decode(data) {
  return toU8(native.woff2File(data))
}
// many .woff2 files in shared launches: per slot the sfnt woff2Decode(file) alone would have
// returned, or the Error it would have thrown (not thrown here: the other files go on)
function woff2DecodeBatch(files) {
  return native.woff2FileBatch(files).map((o) => (o instanceof Error ? o : toU8(o)))
}
// a single-font sfnt -> its .woff2 file, written on the GPU: glyf, loca and hmtx transformed, the
// other tables copied beside them, the stream compressed in FONT mode; every byte but the Brotli
// stream is fixed (tables in tag order, DSIG dropped) and woff2Decode reads every file written.
// options: { quality, lgwin, transformGlyf, transformHmtx } (both transforms default to true)
function woff2EncodeArgs(options) {
  const o = options || {}
  const q = o.quality === undefined || o.quality === null ? 11 : Math.max(0, Math.min(11, o.quality | 0))
  const w = o.lgwin === undefined || o.lgwin === null ? 22 : Math.max(10, Math.min(24, o.lgwin | 0))
  const t = (o.transformGlyf === false ? 0 : 1) | (o.transformHmtx === false ? 0 : 2)
  return [q, w, t]
}
function woff2Encode(sfnt, options) {
  return toU8(native.woff2Write(sfnt, ...woff2EncodeArgs(options)))
}
// many fonts in shared launches: per slot the file woff2Encode(font) alone would have returned,
// or the Error it would have thrown (not thrown here: the other fonts go on)
function woff2EncodeBatch(sfnts, options) {
  return native.woff2WriteBatch(sfnts, ...woff2EncodeArgs(options)).map((o) => (o instanceof Error ? o : toU8(o)))
}

module.exports = {
  brotliEncode, BrotliEncoder, brotliDecode, BrotliDecoder, brotliDecodedSize, EncoderMode,
  brotliEncodeBatch, brotliEncodeBatchAsync, brotliDecodeBatchAsync, BrotliDictionary,
  brotliDecoderUpdateBatch, brotliDecoderFinishBatch,
  woff2TransformGlyf, woff2TransformHmtx, woff2ReconstructGlyf, woff2ReconstructHmtx, woff2Decode, woff2DecodeBatch,
  woff2Encode, woff2EncodeBatch,
}
