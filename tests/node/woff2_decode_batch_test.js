'use strict'
// Node-API check of woff2DecodeBatch (runs on the GPU box through tests/test_gpu_woff2_batch.py):
// the two synthetic golden .woff2 files of tests/golden/woff2/file_golden.json and a file that
// does not parse, in one call: the good slots are their golden sfnts as Uint8Arrays, the bad
// slot is an Error (returned, not thrown), and each slot is what woff2Decode alone gives.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const W = path.join(root, 'tests', 'golden', 'woff2')
const u8 = (b64) => new Uint8Array(Buffer.from(b64, 'base64'))

const gold = JSON.parse(fs.readFileSync(path.join(W, 'file_golden.json')))
const a = gold.synthetic['synthetic'], b = gold.synthetic['synthetic-hmtx']
const bad = u8(b.woff2)
bad[0] = 0x57   // 'WOF2'
const out = lib.woff2DecodeBatch([u8(a.woff2), bad, u8(b.woff2), new Uint8Array(0), u8(a.woff2)])
assert.strictEqual(out.length, 5)
for (const [i, fx] of [[0, a], [2, b], [4, a]]) {
  assert.ok(out[i] instanceof Uint8Array, String(i))
  assert.strictEqual(Buffer.compare(Buffer.from(out[i]), Buffer.from(fx.sfnt, 'base64')), 0, String(i))
  assert.strictEqual(Buffer.compare(Buffer.from(out[i]), Buffer.from(lib.woff2Decode(u8(fx.woff2)))), 0, String(i))
}
console.log('good slots ok')
for (const i of [1, 3]) assert.ok(out[i] instanceof Error, String(i))
let thrown = null
try {
  lib.woff2Decode(bad)
} catch (e) {
  thrown = e
}
assert.ok(thrown instanceof Error)
assert.strictEqual(out[1].message, thrown.message)
console.log('bad slots ok')
assert.deepStrictEqual(lib.woff2DecodeBatch([]), [])
assert.throws(() => lib.woff2DecodeBatch('not an array'), TypeError)
assert.throws(() => lib.woff2DecodeBatch(['not bytes']), TypeError)
console.log('ALL OK')
