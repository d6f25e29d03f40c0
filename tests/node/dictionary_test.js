'use strict'
// The Node mirror of the prepared dictionary (BrotliDictionary, options.dictionary) on the GPU,
// run by tests/test_gpu_dictionary_handle.py with a JSON file of its own making: the
// dictionary, documents, the streams the Python mirror wrote for them with a handle (quality 9)
// and a hand-written stream with a copy from the middle of the dictionary.  Prints one line per
// group and exits non-zero on the first mismatch.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))

const fx = JSON.parse(fs.readFileSync(process.argv[2]))
const u8 = (s) => new Uint8Array(Buffer.from(s, 'base64'))
const D = u8(fx.dictionary)
const docs = fx.docs.map(u8)
const streams = fx.streams.map(u8)
const opts = { quality: fx.quality }
function eq(a, b, what) {
  assert.strictEqual(Buffer.compare(Buffer.from(a), Buffer.from(b)), 0, what)
}
function throws(f, re, what) {
  let err = null
  try { f() } catch (e) { err = e }
  assert.ok(err && re.test(err.message), `${what}: ${err && err.message}`)
}

async function main() {
  const d = new lib.BrotliDictionary(D)
  assert.strictEqual(d.size, D.length)
  assert.strictEqual(d.closed, false)

  // the batch equals the other mirror's bytes, and the k = 1 call equals the batch
  const enc = lib.brotliEncodeBatch(docs, { ...opts, dictionary: d })
  enc.forEach((e, i) => eq(e, streams[i], `batch stream ${i}`))
  docs.forEach((doc, i) => eq(lib.brotliEncode(doc, { ...opts, dictionary: d }), streams[i], `solo stream ${i}`))
  console.log('encode', docs.length)

  // decode: solo, and the async batch with a corrupt stream and a limit that trips in one slot
  streams.forEach((s, i) => eq(lib.brotliDecode(s, { dictionary: d }), docs[i], `decode ${i}`))
  const bad = Uint8Array.from(streams[0], (b, i) => (i ? b ^ 0xff : b))
  const outs = await lib.brotliDecodeBatchAsync([streams[0], bad, streams[1], new Uint8Array(0)], { dictionary: d })
  eq(outs[0], docs[0], 'async slot 0')
  eq(outs[2], docs[1], 'async slot 2')
  assert.ok(outs[1] instanceof Error && /Brotli error code/.test(outs[1].message), 'corrupt slot')
  assert.ok(outs[3] instanceof Error, 'empty slot')
  const big = docs.reduce((m, x) => Math.max(m, x.length), 0)
  const lim = await lib.brotliDecodeBatchAsync(streams, { dictionary: d, maxOutputSize: big - 1 })
  lim.forEach((o, i) => {
    if (docs[i].length >= big) assert.ok(o instanceof Error && o.message === `Decompressed size ${docs[i].length} exceeds limit ${big - 1}`, `limit ${i}: ${o.message}`)
    else eq(o, docs[i], `under the limit ${i}`)
  })
  throws(() => lib.brotliDecode(streams[0], { dictionary: d, maxOutputSize: 1 }), /exceeds limit 1$/, 'solo limit')
  console.log('decode', streams.length)

  // the hand-written mid-dictionary stream: the handle reads it, customDictionary keeps -9
  const small = new lib.BrotliDictionary(u8(fx.mid_dictionary))
  eq(lib.brotliDecode(u8(fx.mid_stream), { dictionary: small }), u8(fx.mid_output), 'mid-dictionary copy')
  throws(() => lib.brotliDecode(u8(fx.mid_stream), { customDictionary: u8(fx.mid_dictionary) }), /Brotli error code: -9/, 'reference rule')
  throws(() => lib.brotliDecode(u8(fx.past_stream), { dictionary: small }), /Brotli error code: -9/, 'one past the end')
  small.close()
  console.log('rule ok')

  // async encode; a close() asked for while it is pending waits for it
  const p = lib.brotliEncodeBatchAsync(docs, { ...opts, dictionary: d })
  d.close()
  assert.strictEqual(d.closed, false, 'close() must wait for the pending call')
  throws(() => lib.brotliEncode(docs[0], { dictionary: d }), /closed/, 'no new call on a closing dictionary')
  const aenc = await p
  aenc.forEach((e, i) => eq(e, streams[i], `async stream ${i}`))
  assert.strictEqual(d.closed, true, 'closed once the call settled')
  d.close()
  console.log('async ok')

  // argument checks
  const e = new lib.BrotliDictionary(new Uint8Array(0))
  assert.strictEqual(e.size, 0)
  throws(() => lib.brotliEncode(docs[0], { dictionary: e, customDictionary: D }), /exclude each other/, 'both dictionaries')
  throws(() => lib.brotliDecode(streams[0], { dictionary: e, customDictionary: D }), /exclude each other/, 'both dictionaries (decode)')
  throws(() => lib.brotliEncode(docs[0], { dictionary: D }), /must be a BrotliDictionary/, 'bytes are no handle')
  throws(() => lib.brotliEncode(docs[0], { dictionary: d }), /closed/, 'closed handle')
  eq(lib.brotliDecode(lib.brotliEncode(docs[0], { dictionary: e }), { dictionary: e }), docs[0], 'empty dictionary')
  e.close()
  assert.deepStrictEqual(lib.brotliEncodeBatch([], { dictionary: new lib.BrotliDictionary(D) }), [])
  console.log('ALL OK')
}
main().catch((e) => {
  console.error(e)
  process.exit(1)
})
