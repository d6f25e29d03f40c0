'use strict'
// Node-API check of woff2Decode / woff2DecodeBatch on a font collection (runs on the GPU box
// through tests/test_gpu_woff2_collection.py): the golden ttc-shared-glyf of
// tests/golden/woff2/collection_golden.json decodes to its golden TTC alone, and in a batch
// beside a single font and a collection that does not parse.
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const root = path.join(__dirname, '..', '..')
const lib = require(path.join(root, 'brotli-lib_amd', 'node', 'index.js'))
const W = path.join(root, 'tests', 'golden', 'woff2')
const u8 = (b64) => new Uint8Array(Buffer.from(b64, 'base64'))
const same = (a, b64) => Buffer.compare(Buffer.from(a), Buffer.from(b64, 'base64')) === 0

const fx = JSON.parse(fs.readFileSync(path.join(W, 'collection_golden.json'))).files['ttc-shared-glyf']
const single = JSON.parse(fs.readFileSync(path.join(W, 'file_golden.json'))).synthetic['synthetic-hmtx']
const solo = lib.woff2Decode(u8(fx.woff2))
assert.ok(solo instanceof Uint8Array)
assert.strictEqual(solo.length, fx.ttc_size)
assert.ok(same(solo, fx.ttc))
assert.strictEqual(Buffer.from(solo.subarray(0, 4)).toString('latin1'), 'ttcf')
console.log('solo ok')
const bad = u8(fx.woff2)
// the CollectionHeader sits behind the directory: version 1.0, two fonts.  Version 3.0 is none.
const v = Buffer.from(bad).indexOf(Buffer.from([0, 1, 0, 0, 2]), 48)
assert.ok(v > 48 && Buffer.from(bad).indexOf(Buffer.from([0, 1, 0, 0, 2]), v + 1) < 0)
bad[v + 1] = 3
const out = lib.woff2DecodeBatch([u8(single.woff2), u8(fx.woff2), bad, u8(fx.woff2)])
assert.strictEqual(out.length, 4)
assert.ok(same(out[0], single.sfnt))
assert.ok(same(out[1], fx.ttc) && same(out[3], fx.ttc))
assert.ok(out[2] instanceof Error)
assert.throws(() => lib.woff2Decode(bad), Error)
console.log('batch ok')
console.log('ALL OK')
