'use strict'
// Interoperability of the prepared dictionary with the Brotli of node's own zlib, where that
// takes a dictionary (it is google/brotli's library; the option does not exist in every node).
// Prints SKIP and exits 0 where zlib ignores the option.  Otherwise: zlib decodes what this engine
// wrote with a BrotliDictionary, and this engine decodes what zlib wrote with the same bytes.
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const fx = JSON.parse(fs.readFileSync(process.argv[2]))
const u8 = (s) => new Uint8Array(Buffer.from(s, 'base64'))
const D = Buffer.from(fx.dictionary, 'base64')
const docs = fx.docs.map(u8)

// a document made of dictionary slices shrinks only if zlib uses the dictionary
const probe = Buffer.from(docs.reduce((a, b) => (b.length > a.length ? b : a)))
let plain, withDict
try {
  plain = zlib.brotliCompressSync(probe)
  withDict = zlib.brotliCompressSync(probe, { dictionary: D })
} catch (e) {
  console.log('SKIP', e.message)
  process.exit(0)
}
if (withDict.length * 2 > plain.length) {
  console.log('SKIP node', process.version, 'zlib takes no dictionary for Brotli')
  process.exit(0)
}
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const d = new lib.BrotliDictionary(new Uint8Array(D))
for (const q of [5, 11]) {
  const enc = lib.brotliEncodeBatch(docs, { quality: q, dictionary: d })
  enc.forEach((e, i) => {
    assert.strictEqual(Buffer.compare(zlib.brotliDecompressSync(Buffer.from(e), { dictionary: D }), Buffer.from(docs[i])), 0, `zlib reads ours, q${q} doc ${i}`)
  })
}
docs.forEach((doc, i) => {
  const z = zlib.brotliCompressSync(Buffer.from(doc), { dictionary: D })
  assert.strictEqual(Buffer.compare(Buffer.from(lib.brotliDecode(new Uint8Array(z), { dictionary: d })), Buffer.from(doc)), 0, `we read zlib's, doc ${i}`)
})
d.close()
console.log('ALL OK')
