'use strict'
// Node-API check of woff2Encode / woff2EncodeBatch over an OpenType collection (run on the GPU by
// tests/test_gpu_woff2_encode_collection.py): the golden TTC ttc-shared-glyf of
// tests/golden/woff2/collection_golden.json becomes a .woff2 file of flavor ttcf with the golden
// file's number of directory entries, woff2Decode gives a TTC of the golden's size back (its
// tables stand in the writer's directory order, not the golden's), and writing that TTC again
// gives the same TTC; in a batch beside a single font and a rejected slot the collection's slot says what
// woff2Encode alone says.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const W = path.join(root, 'tests', 'golden', 'woff2')
const u8 = (b64) => new Uint8Array(Buffer.from(b64, 'base64'))
const same = (a, b) => Buffer.compare(Buffer.from(a), Buffer.from(b)) === 0

const gold = JSON.parse(fs.readFileSync(path.join(W, 'collection_golden.json'))).files['ttc-shared-glyf']
const single = JSON.parse(fs.readFileSync(path.join(W, 'file_golden.json'))).synthetic['synthetic-hmtx']
const ttc = u8(gold.ttc), goldFile = Buffer.from(u8(gold.woff2))

const file = Buffer.from(lib.woff2Encode(ttc))
assert.strictEqual(file.toString('latin1', 0, 8), 'wOF2ttcf')
assert.strictEqual(file.readUInt32BE(8), file.length)
assert.strictEqual(file.length % 4, 0)
assert.strictEqual(file.readUInt16BE(12), goldFile.readUInt16BE(12))   // each shared table once
const back = Buffer.from(lib.woff2Decode(file))
assert.strictEqual(back.length, ttc.length)
assert.ok(same(back.subarray(0, 12), ttc.subarray(0, 12)))   // 'ttcf', the version, numFonts
const again = lib.woff2Decode(lib.woff2Encode(back))
assert.ok(same(again, back))
console.log('solo ok')

const bad = ttc.slice()
bad.set([0, 3, 0, 0], 4)   // version 3.0
const out = lib.woff2EncodeBatch([ttc, bad, u8(single.sfnt), ttc])
assert.strictEqual(out.length, 4)
assert.ok(out[1] instanceof Error)
assert.ok(same(lib.woff2Decode(out[2]), u8(single.sfnt)))
for (const i of [0, 3]) {
  assert.ok(out[i] instanceof Uint8Array, String(i))
  const f = Buffer.from(out[i])
  for (const [lo, hi] of [[0, 8], [12, 20], [24, 48]]) assert.ok(same(f.subarray(lo, hi), file.subarray(lo, hi)), `header ${lo}`)
  assert.ok(same(lib.woff2Decode(out[i]), back), String(i))
}
assert.throws(() => lib.woff2Encode(bad), Error)
console.log('batch ok')
console.log('ALL OK')
