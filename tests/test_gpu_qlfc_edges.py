"""GPU tests of the QLFC stage (include/spring_qlfc.h) on the branches and batch layouts that tests/test_gpu_qlfc.py
does not reach: the range coder's pending units with and without a carry, the escape path below
256 symbols, symbol tables of 4 to 255 symbols, the chunk rule one byte either side of its thresholds, raw chunks
beside coded ones, the rollback of a segment whose later chunk can be neither coded nor stored, CheckEOB one unit either
side of its bound, more than 1024 chunks in a batch, chunk boundaries on the 256-run tiles and 64-run loads of the
kernels, multi-chunk segments in later sub-batches, a two-chunk segment read from the block-sort stage, and batches
with nothing to code.  As there, every segment is compared byte for byte, return value included, with the plain-Python
model (tests/qlfc_model.py) and, where oracle/_ref/libref_units.so is built, with the real function;
tests/test_qlfc_cpu.py shows from the model's counters that every case reaches what it is here for."""
import functools

import numpy as np
import pytest

import qlfc_model as qm

pytestmark = pytest.mark.gpu

REF = qm.ref_lib()
TABLES = qm.state_tables()
needs_ref = pytest.mark.skipif(REF is None or TABLES is None, reason="oracle/_ref/libref_units.so not built (needs the reference sources)")
ANY = "real" if TABLES is not None else 101      # for the tests that are about the batch, not about the tables


@functools.lru_cache(maxsize=None)
def _tables(which):
    return TABLES if which == "real" else qm.random_tables(which)


@functools.lru_cache(maxsize=None)
def _model(data, which):
    """-> ((bytes, return value), chunks, chunks stored raw) as the model has them; a segment without bytes stores none."""
    stats = {}
    res = qm.compress(data, _tables(which), stats) if data else (b"", qm.NOT_COMPRESSIBLE)
    return res, qm.num_chunks(len(data)) if data else 0, stats.get("raw", 0) if res[1] > 0 else 0


def _batch(segs):
    return b"".join(segs), np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)


def _stage(which):
    from spring_amd.qlfc import QlfcStage
    st = QlfcStage()
    st.set_state_tables(*_tables(which))
    return st


def _code(st, segs):
    data, off = _batch(segs)
    info = st.code(data, off)
    assert info["num_segments"] == len(segs) and info["bytes_in"] == len(data)
    got = st.segments()
    assert info["bytes_out"] == sum(len(b) for b, _ in got)
    assert info["not_compressible"] == sum(rc < 0 for _, rc in got)
    return got, info


def _check(got, want, names):
    assert len(got) == len(want)
    for name, (gb, grc), (wb, wrc) in zip(names, got, want):
        print(name, "device", grc, "expected", wrc)
        assert grc == wrc, (name, "return value")
        assert gb == wb, (name, "bytes")


def _check_model(got, info, segs, which, names=None):
    want = [_model(s, which) for s in segs]
    _check(got, [w[0] for w in want], names or range(len(segs)))
    assert info["chunks"] == sum(w[1] for w in want) and info["chunks_raw"] == sum(w[2] for w in want)


@pytest.mark.parametrize("which", [pytest.param("real", marks=pytest.mark.skipif(TABLES is None, reason="the state tables cannot be read: oracle/_ref/libref_units.so not built")),
                                   101, 202])
def test_edge_cases_equal_the_model(which):
    names = qm.EDGE_CASES + qm.table_cases(which)
    segs = [qm.case(n) for n in names]
    with _stage(which) as st:
        got, info = _code(st, segs)
    _check_model(got, info, segs, which, names)
    assert info["not_compressible"] == 1 and got[names.index("eob_0_%s" % which)] == (b"", qm.NOT_COMPRESSIBLE)
    assert info["chunks_raw"] == 4
    if which == "real" and REF is not None:
        _check(got, [qm.ref_compress(s) for s in segs], names)


@needs_ref
def test_rollback_of_a_segment_that_can_be_neither_coded_nor_stored():
    names = (qm.ROLLBACK_CASE, "raw_coded", "empty", "a40")
    segs = [qm.case(qm.ROLLBACK_CASE), qm.case("raw_coded"), b"", qm.case("a40")]
    with _stage("real") as st:
        got, info = _code(st, segs)
        assert got[0] == (b"", qm.NOT_COMPRESSIBLE) and got[2] == (b"", qm.NOT_COMPRESSIBLE)
        _check(got, [qm.ref_compress(s) if s else (b"", qm.NOT_COMPRESSIBLE) for s in segs], names)
        assert info["chunks"] == 5 and info["chunks_raw"] == 1      # a segment without bytes stores no chunk
        assert info["not_compressible"] == 2
        assert st.compress(segs[0]) == (b"", qm.NOT_COMPRESSIBLE)


def test_many_segments():
    segs = qm.many_segments()
    want = [_model(s, 101)[0] for s in segs]
    filled = [rc for s, (_, rc) in zip(segs, want) if s]
    assert len(segs) == 1500 and 10 * sum(rc > 0 for rc in filled) >= 9 * len(filled)
    with _stage(101) as st:
        got, info = _code(st, list(segs))
    _check_model(got, info, segs, 101)
    assert info["chunks"] == len(filled) > 1024 and info["sub_batches"] == 1


@pytest.mark.parametrize("counts", qm.RUN_ORDERS, ids=["tiles", "loads"])
def test_chunk_boundaries_on_tile_and_load_boundaries(counts):
    segs = qm.run_batch(counts)
    assert [len(qm.chunk_ranks(s)[0]) for s in segs] == list(counts)
    with _stage(ANY) as st:
        got, info = _code(st, segs)
    _check_model(got, info, segs, ANY, counts)
    assert info["runs"] == sum(counts) and info["chunks"] == len(counts) and info["not_compressible"] == 0


def test_multi_chunk_segments_in_later_sub_batches():
    from spring_amd.qlfc import workspace_need
    names = ("letters5", "all256runs", "bwt5000", "exp16", "raw4", "raw_coded", "coded_raw")
    segs = [qm.case(n) for n in names]
    with _stage(ANY) as st:
        whole, info = _code(st, segs)
        _check_model(whole, info, segs, ANY, names)
        assert info["sub_batches"] == 1 and info["chunks_raw"] == 4
        alone, info4 = _code(st, [qm.case("raw4")])
        assert alone == [whole[names.index("raw4")]]
        # what the four-chunk case needs alone: it shares a sub-batch with nothing, so the small cases are one
        # sub-batch (or more), it is the next, and the other two raw-chunk cases come after it
        budget = workspace_need(len(qm.case("raw4")), 1) + info4["events"] * 160
        st.set_workspace_bytes(budget)
        split, info2 = _code(st, segs)
    assert info2["sub_batches"] >= 3 and info2["workspace_bytes"] == budget
    assert split == whole
    assert (info2["runs"], info2["events"], info2["chunks"], info2["chunks_raw"]) == (info["runs"], info["events"], info["chunks"], 4)


def test_from_bwt_with_a_two_chunk_segment():
    from spring_amd.bwt import BwtStage
    text = qm._mers(300000)
    with BwtStage() as bw, _stage(ANY) as st:
        binfo = bw.transform(text)
        assert binfo["num_segments"] == 1          # a host buffer without offsets is one segment, whatever the block cut
        res = bw.download()
        assert len(res["bwt"]) == len(text) >= 300000
        info = st.code(bw)
        got = st.segments()
        assert bw.download()["bwt"] == res["bwt"]
    _check_model(got, info, [res["bwt"]], ANY, ["bwt of 300000"])
    assert info["chunks"] == 2 and got[0][1] > 0 and got[0][0][0] == 2


def test_batches_with_nothing_to_code():
    with _stage(101) as st:
        info = st.code(b"", [0, 0, 0])
        assert st.segments() == [(b"", qm.NOT_COMPRESSIBLE)] * 2
        assert (info["num_segments"], info["sub_batches"], info["chunks"], info["events"], info["bytes_out"]) == (2, 1, 0, 0, 0)
        assert info["not_compressible"] == 2
        info = st.code(b"", [0])                     # offsets that start at 0 and end at the 0 bytes: no segments
        assert (info["num_segments"], info["chunks"], info["events"], info["bytes_out"]) == (0, 0, 0, 0)
        res = st.download()
        assert res["coded"] == b"" and list(res["coded_off"]) == [0] and len(res["status"]) == 0 and st.segments() == []
        assert st.compress(b"") == (b"", qm.NOT_COMPRESSIBLE)
        got, _ = _code(st, [qm.case("a40")])         # and the context goes on working
        assert got == [_model(qm.case("a40"), 101)[0]]
