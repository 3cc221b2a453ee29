"""The id codec's checker (tests/idcodec_model.py) against the reference: the recorded files of the real
compress_id_block (tests/golden/ref_idcodec_*.npz) always; the live real codec and the real decompress_id_block where
oracle/_ref is built.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import idcodec_cases as ic
import idcodec_model as m
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_qualid = pytest.mark.skipif(po.ref_qualid_lib() is None, reason="oracle/_ref/libref_qualid.so not built (needs the reference sources)")


@pytest.mark.parametrize("name", ic.ALL)
def test_model_equals_recorded_reference(name):
    ids, B, want = ic.load(name)
    assert len(want) == (len(ids) + B - 1) // B
    assert m.compress_blocks(ids, B) == want


def test_recorded_fixtures_are_the_cases():
    for name, (ids, B) in ic.FIXTURES.items():
        got_ids, got_B, _ = ic.load(name)
        assert got_ids == ids and got_B == B, name
    ids, B, blocks = ic.load("rescale")
    assert ids == [ic.RESCALE_ID] * ic.RESCALE_COUNT and B == ic.RESCALE_COUNT and len(blocks[0]) == 13


def test_rescale_case_reaches_the_rescale():
    # token 0 of every id is coded in the type model of context 0: n = 10 + 10 k reaches 2^20 inside the block
    assert 10 + 10 * ic.RESCALE_COUNT >= 1 << 20
    # ... and every id of the counter case (the first after an empty id, value 0) codes a delta of 1 in the delta model of
    # context 0: n = 256 + 10 k
    ids, B, _ = ic.load("rescale256")
    words, _ = m.block_symbols(ids)
    assert ids[:3] == [b"1", b"2", b"3"] and B == len(ids) == ic.COUNTER_COUNT
    assert words.count(m.word(m.K_DELTA, 0, 1)) == ic.COUNTER_COUNT and 256 + 10 * ic.COUNTER_COUNT >= 1 << 20


def test_symbols_of_a_few_ids():
    sym, starts = m.tokenize(b"@AB.12", b"", [])
    assert starts == [0, 1, 3, 4]
    assert sym == [(m.K_TYPE, 0, m.CHAR), (m.K_CHAR, 0, 64), (m.K_TYPE, 1, m.ALPHA), (m.K_ALEN, 1, 2), (m.K_ABYTE, 1, 65),
                   (m.K_ABYTE, 1, 66), (m.K_TYPE, 2, m.CHAR), (m.K_CHAR, 2, 46), (m.K_TYPE, 3, m.DELTA), (m.K_DELTA, 3, 12),
                   (m.K_TYPE, 4, m.END)]
    sym, _ = m.tokenize(b"@AB.13", b"@AB.12", starts)
    assert [s[2] for s in sym if s[0] == m.K_TYPE] == [m.MATCH, m.MATCH, m.MATCH, m.DELTA, m.END]
    # 2^28 split: the value stops taking digits once it reaches 2^28, and the next piece may start with '0'
    _, starts = m.tokenize(b"268435456123", b"", [])
    assert starts == [0, 9]
    _, starts = m.tokenize(b"2684354560123", b"", [])
    assert starts == [0, 9, 10]


@pytest.mark.parametrize("bad", [b"@" + b"a" * 1023, b"@" + b"a" * 256, b"@" + b"0" * 256, b"@a\x80", b"@a\x00b"])
def test_model_refuses_what_the_stage_refuses(bad):
    with pytest.raises(ValueError):
        m.compress_block([bad])


@needs_qualid
@pytest.mark.parametrize("name", sorted(ic.FIXTURES))
def test_model_equals_live_reference(name):
    ids, B = ic.FIXTURES[name]
    assert m.compress_blocks(ids, B) == ic.ref_blocks(ids, B, num_thr=2)


@needs_qualid
@pytest.mark.parametrize("name", sorted(ic.FIXTURES))
def test_reference_decoder_reads_the_model(name, tmp_path):
    ids, B = ic.FIXTURES[name]
    for b, data in enumerate(m.compress_blocks(ids, B)):
        path = tmp_path / ("id_1.%d" % b)
        path.write_bytes(data)
        assert po.ref_read_ids(str(path), len(ids[b * B:(b + 1) * B])) == ids[b * B:(b + 1) * B]


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib, build
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_idcodec.h")).read()
    declared = set(re.findall(r"\b(spring_idcodec_\w+)\s*\(", hdr))
    assert declared == set(_lib.IDCODEC_EXPORTS) and len(_lib.IDCODEC_EXPORTS) == len(declared)
    for k in dir(_lib):
        if k.endswith("EXPORTS") and k != "IDCODEC_EXPORTS":
            assert not declared & set(getattr(_lib, k))
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert spring_amd.IdCodecStage is not None
    assert "idcodec.hip" in build.SOURCES and "spring_idcodec.h" in build.PUBLIC_HEADERS


def test_info_struct_matches_the_header():
    from spring_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spring_idcodec.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} spring_idcodec_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    assert [f for _, f in fields] == [k for k, _ in _lib.IdCodecInfo._fields_]
    assert all((t == "double") == (c is C.c_double) for (t, _), (_, c) in zip(fields, _lib.IdCodecInfo._fields_))
    assert C.sizeof(_lib.IdCodecInfo) == 8 * len(fields)
    kinds = dict((k, int(v)) for k, v in re.findall(r"#define SPRING_IDCODEC_K_(\w+) (\d+)", hdr))
    assert kinds == dict(TYPE=m.K_TYPE, ALEN=m.K_ALEN, ABYTE=m.K_ABYTE, CHAR=m.K_CHAR, DELTA=m.K_DELTA, ZEROS=m.K_ZEROS, INT=m.K_INT)
    assert np.uint32(m.word(m.K_INT, 4 * 1023 + 3, 255)) == 255 | (6 << 8) | (4095 << 11)
