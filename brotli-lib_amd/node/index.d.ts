// Type declarations of the brotli_amd Node drop-in: the public surface of countertype/brotli-lib
// (src/encode/encode.ts:22-27,50-90,290-409; src/decode/decode.ts:9-16,18-65;
// src/encode/enc-constants.ts:56-60), plus this engine's batch entry points.

export declare const EncoderMode: {
  readonly GENERIC: 0
  readonly TEXT: 1
  readonly FONT: 2
}
export type EncoderMode = (typeof EncoderMode)[keyof typeof EncoderMode]

/** extension (brotli_amd.h mib_dictionary): shared bytes uploaded to the GPU and indexed there
 *  once. Copies may come from anywhere in it (customDictionary: its tail only), so a stream
 *  written with one decodes with one of the same bytes. A BrotliEncoder / BrotliDecoder made with
 *  it (options.dictionary) holds a reference of its own and keeps working after close(). */
export declare class BrotliDictionary {
  constructor(data: Uint8Array | Int8Array)
  /** the dictionary's length in bytes */
  readonly size: number
  readonly closed: boolean
  /** drops this object's reference to the device memory (it goes once no session holds the
   *  dictionary either); waits for pending async calls that use the dictionary */
  close(): void
}

export interface BrotliEncodeOptions {
  /** 0..11, default 11 (clamped) */
  quality?: number
  /** 10..24, default 22 (clamped) */
  lgwin?: number
  mode?: EncoderMode
  /** accepted, no effect (as in the reference) */
  sizeHint?: number
  /** extension: the encoder side of BrotliDecodeOptions.customDictionary; the stream decodes
   *  with (and only with) the same dictionary */
  customDictionary?: Uint8Array | Int8Array
  /** extension: a prepared dictionary (not together with customDictionary, not with gpus);
   *  new BrotliEncoder({dictionary}) takes it too, with the same errors */
  dictionary?: BrotliDictionary
}

export declare function brotliEncode(input: Uint8Array, options?: BrotliEncodeOptions): Uint8Array

export declare class BrotliEncoder {
  constructor(options?: BrotliEncodeOptions)
  /** the newly completed bytes (may be empty until enough input has arrived) */
  update(chunk: Uint8Array): Uint8Array
  finish(): Uint8Array
}

export interface BrotliDecodeOptions {
  maxOutputSize?: number
  /** compound dictionary (engine.ts:142-159) */
  customDictionary?: Uint8Array | Int8Array
  /** extension: the BrotliDictionary the stream was written with (not together with customDictionary) */
  dictionary?: BrotliDictionary
}

/** options as a number: the legacy exact output size (truncate / zero-pad) */
export declare function brotliDecode(buffer: Uint8Array, options?: BrotliDecodeOptions | number): Uint8Array

export interface BrotliDecoderOptions {
  /** limit on the total output; passing it throws "Decompressed size X exceeds limit Y" */
  maxOutputSize?: number
  /** compound dictionary (engine.ts:142-159), copied by the decoder */
  customDictionary?: Uint8Array | Int8Array
  /** output bytes per device pass, default 16 MiB, clamped to 64 KiB .. 512 MiB */
  outWindow?: number
  /** extension: the BrotliDictionary the stream was written with (not together with
   *  customDictionary): copies from anywhere in it are valid, as in brotliDecode */
  dictionary?: BrotliDictionary
}

/** extension (the reference decodes in one shot only): the decode side of BrotliEncoder. The
 *  last 2^lgwin bytes of output, the input still needed and the decoder's state stay on the GPU
 *  between calls, so a stream of any length decodes as it arrives. Bytes behind the stream's end
 *  throw "Brotli error code: -17"; after an error every call throws it again. */
export declare class BrotliDecoder {
  constructor(options?: BrotliDecoderOptions)
  /** the next bytes of the stream, cut anywhere; returns the bytes they complete (may be empty) */
  update(chunk: Uint8Array): Uint8Array
  /** the input has ended: the remaining bytes, or the decoder's error for an incomplete stream */
  finish(): Uint8Array
  /** the stream's last metablock has been decoded */
  readonly finished: boolean
}

/** decoded size from the first metablock header, -1 when unknown */
export declare function brotliDecodedSize(buffer: Uint8Array): number

export interface BatchOptions {
  /** shard the batch over this many GPUs (0: every visible one); absent: one GPU */
  gpus?: number
}
/** independent buffers in one GPU launch sequence (or one per GPU, options.gpus) */
export declare function brotliEncodeBatch(inputs: Uint8Array[], options?: BrotliEncodeOptions & BatchOptions): Uint8Array[]
export declare function brotliEncodeBatchAsync(inputs: Uint8Array[], options?: BrotliEncodeOptions & BatchOptions): Promise<Uint8Array[]>
/** a stream that fails to decode resolves to its Error in its slot */
export declare function brotliDecodeBatchAsync(
  inputs: Uint8Array[],
  /** dictionary: the BrotliDictionary the streams were written with; maxOutputSize then applies to every stream */
  options?: BatchOptions & { dictionary?: BrotliDictionary; maxOutputSize?: number },
): Promise<(Uint8Array | Error)[]>
/** many distinct BrotliDecoder sessions advance by one chunk each in shared GPU launches; per slot what decoder.update(chunk) alone would have returned, or the Error it would have thrown */
export declare function brotliDecoderUpdateBatch(decoders: BrotliDecoder[], chunks: Uint8Array[]): (Uint8Array | Error)[]
/** finish() of many BrotliDecoder sessions in shared launches; per slot the rest of the output, or the Error of an incomplete stream */
export declare function brotliDecoderFinishBatch(decoders: BrotliDecoder[]): (Uint8Array | Error)[]
/** WOFF2 'glyf' transform (W3C WOFF2 section 5.1) of a TrueType font, on the GPU: FONT-mode input for brotliEncode */
export declare function woff2TransformGlyf(ttf: Uint8Array): Uint8Array
/** WOFF2 'hmtx' transform (section 5.4), or null when the table must stay untransformed */
export declare function woff2TransformHmtx(ttf: Uint8Array): Uint8Array | null
/** inverse of woff2TransformGlyf: the TrueType glyf table and its loca (the header's indexFormat), on the GPU; throws on a table that does not parse */
export declare function woff2ReconstructGlyf(data: Uint8Array): { glyf: Uint8Array, loca: Uint8Array }
/** inverse of woff2TransformHmtx: the dropped side bearings are the glyphs' xMin in glyf / loca */
export declare function woff2ReconstructHmtx(data: Uint8Array, glyf: Uint8Array, loca: Uint8Array, numGlyphs: number, numHMetrics: number): Uint8Array
/** a .woff2 file -> the sfnt it stands for, decoded, reconstructed and assembled on the GPU (records sorted by tag, tables in the file's order, checksums computed); a font collection (flavor ttcf) -> its TTC (the members' directories behind the TTC header, each shared table once); throws on a file that does not parse */
export declare function woff2Decode(data: Uint8Array): Uint8Array
/** woff2Decode of many files, single fonts and collections in any slots, in shared GPU launches (one Brotli decode launch and one assembly launch per group of files): per slot the sfnt or TTC, or the Error woff2Decode(file) alone would have thrown */
export declare function woff2DecodeBatch(files: Uint8Array[]): (Uint8Array | Error)[]
export interface Woff2EncodeOptions {
  /** 0..11, default 11 */
  quality?: number
  /** 10..24, default 22 */
  lgwin?: number
  /** transform glyf + loca where the font has them (default true); a font the transform rejects throws */
  transformGlyf?: boolean
  /** transform hmtx where glyf is transformed and a side-bearing array equals the glyphs' xMin (default true) */
  transformHmtx?: boolean
}
/** an sfnt -> its .woff2 file, written on the GPU (FONT-mode Brotli; tables in tag order, DSIG dropped; every byte but the Brotli stream is fixed); an OpenType collection (TTC) -> the .woff2 file of flavor ttcf (every table once in one directory: tables of one tag, offset and length, or of one tag and length and equal bytes, are one entry; glyf and loca are shared as a pair; each member lists its entries in the CollectionHeader); woff2Decode reads every file written; throws on a font or collection that does not parse */
export declare function woff2Encode(sfnt: Uint8Array, options?: Woff2EncodeOptions): Uint8Array
/** woff2Encode of many fonts, single fonts and collections in any slots, in shared GPU launches (one upload, one compare launch where collections have tables to compare, one copy launch and one encode call per group of fonts): per slot the file, or the Error woff2Encode(font) alone would have thrown */
export declare function woff2EncodeBatch(sfnts: Uint8Array[], options?: Woff2EncodeOptions): (Uint8Array | Error)[]
