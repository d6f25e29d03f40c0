'use strict'
// The Node mirror of sessions with a prepared dictionary (new BrotliEncoder({dictionary}),
// new BrotliDecoder({dictionary})) on the GPU, run by tests/test_gpu_dictionary_sessions.py with a
// JSON file of its own making: the dictionary, a document of slices and noise, and the stream the
// Python mirror's session wrote for it.  Prints one line per group and exits non-zero on the first
// mismatch.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))

const fx = JSON.parse(fs.readFileSync(process.argv[2]))
const u8 = (s) => new Uint8Array(Buffer.from(s, 'base64'))
const D = u8(fx.dictionary)
const doc = u8(fx.doc)
const stream = u8(fx.stream)
const opts = { quality: fx.quality, lgwin: fx.lgwin }
function eq(a, b, what) {
  assert.strictEqual(Buffer.compare(Buffer.from(a), Buffer.from(b)), 0, what)
}
function throws(f, re, what) {
  let err = null
  try { f() } catch (e) { err = e }
  assert.ok(err && re.test(err.message), `${what}: ${err && err.message}`)
}
function feed(session, data, step) {
  const parts = []
  for (let at = 0; at < data.length; at += step) parts.push(Buffer.from(session.update(data.subarray(at, Math.min(data.length, at + step)))))
  parts.push(Buffer.from(session.finish()))
  return new Uint8Array(Buffer.concat(parts))
}

function main() {
  const d = new lib.BrotliDictionary(D)

  // the session's stream is the other mirror's, byte for byte, and decodes through the one-shot
  // call and through a decoder session
  const enc = feed(new lib.BrotliEncoder({ ...opts, dictionary: d }), doc, fx.step)
  eq(enc, stream, 'encoder session stream')
  eq(lib.brotliDecode(enc, { dictionary: d }), doc, 'one-shot decode')
  const dec = new lib.BrotliDecoder({ dictionary: d, outWindow: 65536 })
  eq(feed(dec, enc, 10000), doc, 'decoder session')
  assert.strictEqual(dec.finished, true)
  throws(() => feed(new lib.BrotliDecoder({ customDictionary: D }), enc, 10000), /Brotli error code: -9/, 'reference rule')
  console.log('round trip', enc.length)

  // close() with sessions open: they hold references of their own
  const e2 = new lib.BrotliEncoder({ ...opts, dictionary: d })
  const d2 = new lib.BrotliDecoder({ dictionary: d })
  const head = Buffer.from(e2.update(doc.subarray(0, fx.step)))
  d.close()
  assert.strictEqual(d.closed, true)
  const parts = [head]
  for (let at = fx.step; at < doc.length; at += fx.step) parts.push(Buffer.from(e2.update(doc.subarray(at, Math.min(doc.length, at + fx.step)))))
  parts.push(Buffer.from(e2.finish()))
  const enc2 = new Uint8Array(Buffer.concat(parts))
  eq(enc2, stream, 'encoder session across close()')
  eq(feed(d2, enc2, 10000), doc, 'decoder session across close()')
  console.log('lifetime ok')

  // the three option errors, as brotliEncode's options.dictionary
  const live = new lib.BrotliDictionary(D.subarray(0, 100))
  for (const C of [lib.BrotliEncoder, lib.BrotliDecoder]) {
    throws(() => new C({ dictionary: D }), /must be a BrotliDictionary/, 'bytes are no handle')
    throws(() => new C({ dictionary: live, customDictionary: D }), /exclude each other/, 'both dictionaries')
    throws(() => new C({ dictionary: d }), /closed/, 'closed handle')
  }
  live.close()
  console.log('ALL OK')
}
try {
  main()
} catch (e) {
  console.error(e)
  process.exit(1)
}
