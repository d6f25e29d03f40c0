"""The stream writer of tests/_streams.py is right: what it writes, the oracle (and native
brotli, where node is installed) decodes to the model's bytes; its placement constructors hit
the table totals they claim, by the oracle decoder's own count; and the seeded set keeps
covering the header features it is there for.  CPU only: these runs are why the GPU tests of
test_gpu_decode_synthetic.py may trust the writer's streams."""
import hashlib
import shutil
import struct
import subprocess

import pytest

import _oracle
import _streams as S


def _expected(st, built):
    """the model's bytes; for word references the oracle's (the writer knows only their length)"""
    exp = S.model(st)
    if exp is None:
        exp = _oracle.decode(built.data)
        assert isinstance(exp, bytes) and len(exp) == len(built.sim_out), st.name
    return exp


def test_oracle_decodes_every_stream_to_the_model():
    words = 0
    for st, b in S.corpus():
        got = _oracle.decode(b.data)
        exp = _expected(st, b)
        assert got == exp, st.name
        if S.model(st) is None:
            assert b.words and b.stats['words'] > 0
            words += 1
        else:
            assert b.sim_out == exp, st.name   # the writer's own running output is the model's
        assert len(b.sim_out) <= (1 << 20) + 16 and len(b.data) <= 140000, st.name
    assert words >= 10
    assert len(S.corpus()) >= 230


def test_peek_size_agrees_where_the_header_gives_one():
    for st, b in S.corpus():
        first = st.mbs[0]
        if first.kind == 'empty':
            want = 0
        elif first.kind == 'cmds' and len(st.mbs) == 1:
            want = len(b.sim_out)
        else:
            want = -1
        assert _oracle.peek_size(b.data) == want, st.name


@pytest.mark.skipif(shutil.which('node') is None, reason='node not installed')
def test_native_brotli_agrees(tmp_path):
    """zlib.brotliDecompressSync on every stream, one child process for all of them"""
    p = tmp_path / 'streams.bin'
    with open(p, 'wb') as f:
        for _, b in S.corpus():
            f.write(struct.pack('<I', len(b.data)) + b.data)
    js = ("const z=require('zlib'),fs=require('fs'),c=require('crypto');const d=fs.readFileSync(process.argv[1]);"
          "let o=0,r=[];while(o<d.length){const n=d.readUInt32LE(o);o+=4;try{r.push(c.createHash('sha256')"
          ".update(z.brotliDecompressSync(d.subarray(o,o+n))).digest('hex'))}catch(e){r.push('ERR '+e.code)}o+=n}"
          "process.stdout.write(r.join('\\n'))")
    out = subprocess.run(['node', '-e', js, str(p)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split('\n')
    assert len(got) == len(S.corpus())
    for (st, b), h in zip(S.corpus(), got):
        assert h == hashlib.sha256(_expected(st, b)).hexdigest(), st.name


def _oracle_total(data):
    _oracle.max_table_total()
    assert isinstance(_oracle.decode(data), bytes)
    return _oracle.max_table_total()


def test_placement_totals_by_the_oracles_count():
    """both sides of 12,224 (the batch build's LDS cap), 65,536 (16-bit roots) and 68,096 (the
    one-per-CU build's cap): the exact value; parity never forbids it, since the number of trees
    (one root each) is free"""
    by_name = {st.name: b for st, b in S.corpus()}
    for t in S.BOUNDARIES:
        b = by_name['placed_%d' % t]
        assert _oracle_total(b.data) == t
        assert b.stats['totals'] == [t]
    assert _oracle_total(by_name['lit256'].data) == 66306
    assert _oracle_total(by_name['placed_90000'].data) == 90000
    # the transitions stream: small, beyond every cap, small, between the caps, small
    tr = by_name['transitions']
    assert tr.stats['totals'] == [2500, 70000, 9000, 13000, 1100] and _oracle_total(tr.data) == 70000
    # every stream: the writer's arithmetic is the oracle's count
    for st, b in S.corpus():
        assert _oracle_total(b.data) == max(b.stats['totals'], default=0), st.name


def test_placed_streams_use_their_last_trees():
    """a wrapped or misplaced root must change the output: the last literal, command and distance
    tree of a placed metablock each decode symbols, with explicit distances among them"""
    for st, b in S.corpus():
        for mb in st.mbs:
            if mb.kind == 'cmds' and hasattr(mb, 'want_total'):
                used = b.stats['trees_used']
                assert ('L', mb.ntrees_l - 1) in used and ('I', mb.ntypes[1] - 1) in used, st.name
                assert ('D', mb.ntrees_d - 1) in used, st.name
                assert b.stats['postfix'] + b.stats['direct'] > 0
    lit = next(st for st, _ in S.corpus() if st.name == 'lit256')
    assert lit.mbs[0].ntrees_l == 256 and lit.mbs[0].ntypes[1] == 1 and lit.mbs[0].ntrees_d == 1


def test_named_edges_are_what_their_names_say():
    by_name = {st.name: b.stats for st, b in S.corpus()}
    assert by_name['meta_sizes']['skipbytes'] == {0, 1, 2, 3}
    assert by_name['long_run_65606']['mnibbles'] == {5} and by_name['long_run_1048581']['mnibbles'] == {6}
    assert by_name['many_types']['type_wrap'] >= 2 and by_name['many_types']['switch'] == {0, 1, 2}
    assert by_name['ring_wrap']['ring_cross'] >= 3
    assert by_name['simple_codes']['tree_select'] == {(1, 0), (2, 0), (3, 0), (4, 0), (4, 1)}
    assert by_name['word_refs']['words'] >= 42
    assert by_name['transitions']['raw_mid'] == 2 and by_name['transitions']['meta_mid'] == 2


def test_seeded_set_keeps_its_coverage():
    agg = S.new_stats()
    lgwin10_cross = 0
    n = 0
    for st, b in S.corpus():
        if not st.name.startswith('random_'):
            continue
        n += 1
        for k, v in b.stats.items():
            if isinstance(v, set):
                agg[k] |= v
            elif isinstance(v, list):
                agg[k] += v
            elif k == 'maxlen':
                agg[k] = max(agg[k], v)
            else:
                agg[k] += v
        if st.lgwin == 10:
            lgwin10_cross += b.stats['ring_cross']
    assert n == 200
    assert agg['npostfix'] == {0, 1, 2, 3}
    assert agg['ndirect'] == set(range(16))
    assert agg['modes_used'] == {0, 1, 2, 3}
    assert agg['map_rle'] and agg['map_plain'] and agg['map_imtf'] and agg['map_no_imtf']
    assert agg['nsym'] == {1, 2, 3, 4} and {(4, 0), (4, 1)} <= agg['tree_select']
    assert agg['hskip'] == {0, 2, 3}
    assert agg['rep16'] and agg['rep17'] and agg['rep_chained']
    assert agg['maxlen'] >= 12
    assert agg['switch'] == {0, 1, 2} and agg['type_wrap']
    assert agg['raw_mid'] and agg['meta_mid']
    assert agg['long_copy']
    assert {1, 2, 3, 63} <= agg['overlap']
    assert lgwin10_cross
    assert agg['short'] == set(range(16)) and agg['implicit'] and agg['direct'] and agg['postfix'] and agg['words']
    assert agg['cells'] == {0, 64, 128, 192, 256, 320, 384, 448, 512, 576, 640}
