'use strict'
// Node-API check of woff2Encode / woff2EncodeBatch (run on the GPU by
// tests/test_gpu_woff2_encode.py): the synthetic golden font of tests/golden/woff2/file_golden.json
// is written with and without the hmtx transform, the files carry the golden files' header fields
// and directory and decode to the golden sfnt; in a batch a font that does not parse is an Error
// (returned, not thrown) and each good slot says what woff2Encode alone says.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const W = path.join(root, 'tests', 'golden', 'woff2')
const u8 = (b64) => new Uint8Array(Buffer.from(b64, 'base64'))
const same = (a, b) => Buffer.compare(Buffer.from(a), Buffer.from(b)) === 0

const gold = JSON.parse(fs.readFileSync(path.join(W, 'file_golden.json')))
const a = gold.synthetic['synthetic'], b = gold.synthetic['synthetic-hmtx']
// where the directory ends (the known-tag indices of glyf, loca and hmtx are 10, 11 and 3)
const dirEnd = (v) => {
  let at = 48
  const base128 = () => {
    while (v[at++] & 0x80);
  }
  for (let i = 0; i < v.readUInt16BE(12); i++) {
    const flags = v[at++], idx = flags & 63, ver = flags >> 6
    if (idx === 63) at += 4
    base128()
    if (((idx === 10 || idx === 11) && ver === 0) || (idx === 3 && ver === 1)) base128()
  }
  return at
}
// every byte but the Brotli stream's: the header (but its length and totalCompressedSize), the
// directory, and zero padding to a 4-byte boundary
const fixed = (file, golden) => {
  const f = Buffer.from(file), g = Buffer.from(golden)
  for (const [lo, hi] of [[0, 8], [12, 20], [24, 48]]) assert.ok(same(f.subarray(lo, hi), g.subarray(lo, hi)), `header ${lo}`)
  const at = dirEnd(g)
  assert.strictEqual(dirEnd(f), at)
  assert.ok(same(f.subarray(48, at), g.subarray(48, at)), 'directory')
  const comp = f.readUInt32BE(20)
  assert.strictEqual(f.readUInt32BE(8), f.length)
  assert.strictEqual(f.length, (at + comp + 3) & ~3)
  for (let i = at + comp; i < f.length; i++) assert.strictEqual(f[i], 0)
}

const plain = lib.woff2Encode(u8(a.sfnt), { transformHmtx: false })
const hm = lib.woff2Encode(u8(b.sfnt))
assert.ok(plain instanceof Uint8Array && hm instanceof Uint8Array)
fixed(plain, u8(a.woff2))
fixed(hm, u8(b.woff2))
assert.ok(same(lib.woff2Decode(plain), u8(a.sfnt)))
assert.ok(same(lib.woff2Decode(hm), u8(b.sfnt)))
console.log('solo ok')

const bad = u8(a.sfnt)
bad.set([0x74, 0x74, 0x63, 0x66])   // 'ttcf'
const out = lib.woff2EncodeBatch([u8(b.sfnt), bad, u8(a.sfnt), new Uint8Array(0), u8(b.sfnt)], { quality: 5, lgwin: 18 })
assert.strictEqual(out.length, 5)
for (const i of [0, 2, 4]) {
  assert.ok(out[i] instanceof Uint8Array, String(i))
  fixed(out[i], u8(b.woff2))
  assert.ok(same(lib.woff2Decode(out[i]), u8(b.sfnt)), String(i))
}
for (const i of [1, 3]) assert.ok(out[i] instanceof Error, String(i))
let thrown = null
try {
  lib.woff2Encode(bad)
} catch (e) {
  thrown = e
}
assert.ok(thrown instanceof Error)
assert.strictEqual(out[1].message, thrown.message)
console.log('batch ok')
assert.deepStrictEqual(lib.woff2EncodeBatch([]), [])
assert.throws(() => lib.woff2EncodeBatch('not an array'), TypeError)
assert.throws(() => lib.woff2EncodeBatch(['not bytes']), TypeError)
assert.throws(() => lib.woff2Encode('not bytes'), TypeError)
console.log('ALL OK')
