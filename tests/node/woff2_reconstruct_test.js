'use strict'
// Node-API check of the inverse WOFF2 transforms (runs on the GPU box through
// tests/test_gpu_woff2_reconstruct.py): woff2ReconstructGlyf on the reference's TrueType bench
// font against the fontTools golden, the shape of what it returns, the synthetic fixture's
// hmtx, and the error a table that does not parse raises.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const crypto = require('crypto')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const G = path.join(root, 'tests', 'golden')
const sha = (u) => crypto.createHash('sha256').update(Buffer.from(u)).digest('hex')
const u8 = (b64) => new Uint8Array(Buffer.from(b64, 'base64'))

const gold = JSON.parse(fs.readFileSync(path.join(G, 'woff2', 'reconstruct_golden.json')))
const ttf = new Uint8Array(fs.readFileSync(path.join(G, 'bench', 'enc-ttf.bin')))
const t = lib.woff2TransformGlyf(ttf)
const r = lib.woff2ReconstructGlyf(t)
assert.deepStrictEqual(Object.keys(r).sort(), ['glyf', 'loca'])
assert.ok(r.glyf instanceof Uint8Array && r.loca instanceof Uint8Array)
const want = gold.bench['enc-ttf']
assert.strictEqual(r.glyf.length, want.glyf_size)
assert.strictEqual(r.loca.length, want.loca_size)
assert.strictEqual(sha(r.glyf), want.glyf_sha256, 'reconstructed glyf')
assert.strictEqual(sha(r.loca), want.loca_sha256, 'reconstructed loca')
console.log('glyf ok')

for (const name of Object.keys(gold.synthetic).sort()) {
  const fx = gold.synthetic[name]
  const s = lib.woff2ReconstructGlyf(u8(fx.tglyf))
  assert.strictEqual(Buffer.compare(Buffer.from(s.glyf), Buffer.from(fx.glyf, 'base64')), 0, name + ' glyf')
  assert.strictEqual(Buffer.compare(Buffer.from(s.loca), Buffer.from(fx.loca, 'base64')), 0, name + ' loca')
  const h = lib.woff2ReconstructHmtx(u8(fx.thmtx), s.glyf, s.loca, fx.num_glyphs, fx.num_hmetrics)
  assert.ok(h instanceof Uint8Array)
  assert.strictEqual(Buffer.compare(Buffer.from(h), Buffer.from(fx.hmtx, 'base64')), 0, name + ' hmtx')
}
console.log('synthetic ok')

assert.throws(() => lib.woff2ReconstructGlyf(t.subarray(0, 35)), Error)
assert.throws(() => lib.woff2ReconstructGlyf(t.subarray(0, t.length - 1)), Error)
assert.throws(() => lib.woff2ReconstructGlyf('not bytes'), TypeError)
console.log('errors ok')
console.log('ALL OK')
