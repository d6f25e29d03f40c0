'use strict'
// Node-API check of woff2Decode (runs on the GPU box through tests/test_gpu_woff2_file.py):
// every golden .woff2 file of tests/golden/woff2/file_golden.json becomes its golden sfnt
// (bytes for the synthetic files, size and sha256 for the bench fonts), the result is a
// Uint8Array, and a file that does not parse throws.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const crypto = require('crypto')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const W = path.join(root, 'tests', 'golden', 'woff2')
const sha = (u) => crypto.createHash('sha256').update(Buffer.from(u)).digest('hex')
const u8 = (b64) => new Uint8Array(Buffer.from(b64, 'base64'))

const gold = JSON.parse(fs.readFileSync(path.join(W, 'file_golden.json')))
let good = null
for (const name of Object.keys(gold.synthetic).sort()) {
  const fx = gold.synthetic[name]
  const out = lib.woff2Decode(u8(fx.woff2))
  assert.ok(out instanceof Uint8Array)
  assert.strictEqual(Buffer.compare(Buffer.from(out), Buffer.from(fx.sfnt, 'base64')), 0, name)
  good = u8(fx.woff2)
}
console.log('synthetic ok')

for (const name of Object.keys(gold.bench).sort()) {
  const fx = gold.bench[name]
  const out = lib.woff2Decode(new Uint8Array(fs.readFileSync(path.join(W, fx.file))))
  assert.strictEqual(out.length, fx.sfnt_size, name)
  assert.strictEqual(sha(out), fx.sfnt_sha256, name)
}
console.log('bench ok')

const bad = new Uint8Array(good)
bad[0] = 0x57   // 'WOF2'
assert.throws(() => lib.woff2Decode(bad), Error)
assert.throws(() => lib.woff2Decode(good.subarray(0, 47)), Error)
assert.throws(() => lib.woff2Decode(good.subarray(0, good.length - 1)), Error)
assert.throws(() => lib.woff2Decode('not bytes'), TypeError)
assert.strictEqual(lib.woff2Decode(good).length, gold.synthetic['synthetic-hmtx'].sfnt_size)
console.log('errors ok')
console.log('ALL OK')
