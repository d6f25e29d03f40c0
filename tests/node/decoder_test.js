'use strict'
// BrotliDecoder of the Node drop-in (runs on the GPU box through tests/test_gpu_node_decoder.py):
// two streams in 4,096-byte updates against brotliDecode, `finished`, finish(), the error
// after the stream's end.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const G = path.join(root, 'tests', 'golden')

for (const name of ['vectors/alice29.txt.compressed', 'parts/parts_enwik300k.br']) {
  const comp = new Uint8Array(fs.readFileSync(path.join(G, name)))
  const exp = Buffer.from(lib.brotliDecode(comp))
  const d = new lib.BrotliDecoder()
  const parts = []
  assert.strictEqual(d.finished, false)
  for (let at = 0; at < comp.length; at += 4096) parts.push(Buffer.from(d.update(comp.subarray(at, at + 4096))))
  assert.strictEqual(d.finished, true, name)
  parts.push(Buffer.from(d.finish()))
  assert.strictEqual(Buffer.compare(Buffer.concat(parts), exp), 0, name)
  assert.throws(() => d.update(new Uint8Array([1])), /Brotli error code: -17/)
  assert.throws(() => d.finish(), /Brotli error code: -17/)
  console.log(name, comp.length, '->', exp.length)
}
{
  const comp = new Uint8Array(fs.readFileSync(path.join(G, 'vectors/alice29.txt.compressed')))
  const d = new lib.BrotliDecoder({ maxOutputSize: 1000, outWindow: 65536 })
  assert.throws(() => d.update(comp), /Decompressed size \d+ exceeds limit 1000/)
  const t = new lib.BrotliDecoder()
  t.update(comp.subarray(0, 5000))
  assert.throws(() => t.finish(), /Brotli error code: -\d+/)
}
console.log('ALL OK')
