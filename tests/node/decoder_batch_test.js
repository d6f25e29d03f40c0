'use strict'
// brotliDecoderUpdateBatch / brotliDecoderFinishBatch of the Node drop-in (runs on the GPU box
// through tests/test_gpu_node_decoder_batch.py): a handful of golden vectors in lock-step
// 1,024-byte chunks against their plain files, a corrupt stream in one slot (argv: its base64
// and the oracle's error code for it), a session over its output limit in another.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const CHUNK = 1024
const V = path.join(root, 'tests', 'golden', 'vectors')

const corrupt = new Uint8Array(Buffer.from(process.argv[2], 'base64'))
const code = parseInt(process.argv[3], 10)
assert.ok(corrupt.length > 0 && code < 0)

const names = ['alice29.txt', '10x10y', '64x', 'monkey', 'mapsdatazrh']
const comps = names.map((n) => new Uint8Array(fs.readFileSync(path.join(V, n + '.compressed'))))
const exps = names.map((n) => fs.readFileSync(path.join(V, n)))
// slots: the vectors, then the corruption, then alice29 with a limit one byte short
const streams = comps.concat([corrupt, comps[0]])
const decoders = streams.map((_, i) => new lib.BrotliDecoder(i === streams.length - 1 ? { maxOutputSize: exps[0].length - 1 } : {}))
const bad = names.length, limited = names.length + 1
const got = streams.map(() => [])
const errors = streams.map(() => null)
const steps = Math.max(...streams.map((s) => Math.ceil(s.length / CHUNK)))
function collect(outs) {
  assert.strictEqual(outs.length, streams.length)
  outs.forEach((o, i) => {
    if (o instanceof Error) {
      // reported again in every later call (the size in the limit's message is the first report's only)
      if (errors[i]) assert.strictEqual(o.message.replace(/size \d+/, ''), errors[i].message.replace(/size \d+/, ''))
      else errors[i] = o
    } else {
      assert.ok(o instanceof Uint8Array)
      assert.strictEqual(errors[i], null, 'bytes after an error in slot ' + i)
      got[i].push(Buffer.from(o))
    }
  })
}
for (let t = 0; t < steps; t++) collect(lib.brotliDecoderUpdateBatch(decoders, streams.map((s) => s.subarray(CHUNK * t, CHUNK * (t + 1)))))
names.forEach((n, i) => assert.strictEqual(decoders[i].finished, true, n))
collect(lib.brotliDecoderFinishBatch(decoders))
names.forEach((n, i) => {
  assert.strictEqual(errors[i], null, n)
  assert.strictEqual(Buffer.compare(Buffer.concat(got[i]), exps[i]), 0, n)
  console.log(n, comps[i].length, '->', exps[i].length)
})
// the corrupt slot: the decoder's error, of the type and with the message update() throws
assert.ok(errors[bad] instanceof Error && !(errors[bad] instanceof TypeError) && !(errors[bad] instanceof RangeError))
assert.strictEqual(errors[bad].message, 'Brotli error code: ' + code)
{
  const solo = new lib.BrotliDecoder()
  let thrown = null
  try {
    for (let at = 0; at < corrupt.length; at += CHUNK) solo.update(corrupt.subarray(at, at + CHUNK))
    solo.finish()
  } catch (e) {
    thrown = e
  }
  assert.ok(thrown && thrown.constructor === errors[bad].constructor && thrown.message === errors[bad].message)
}
assert.strictEqual(errors[limited].message, `Decompressed size ${exps[0].length} exceeds limit ${exps[0].length - 1}`)
console.log('corrupt slot:', errors[bad].message, '| limited slot:', errors[limited].message)
// call-level errors throw
assert.throws(() => lib.brotliDecoderUpdateBatch([decoders[0], decoders[0]], [new Uint8Array(0), new Uint8Array(0)]), /brotli_amd|invalid/i)
assert.throws(() => lib.brotliDecoderUpdateBatch([decoders[0]], []), TypeError)
assert.deepStrictEqual(lib.brotliDecoderUpdateBatch([], []), [])
assert.deepStrictEqual(lib.brotliDecoderFinishBatch([]), [])
console.log('ALL OK')
