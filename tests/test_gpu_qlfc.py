"""GPU tests of the QLFC stage (include/spring_qlfc.h).  Every segment is compared byte for byte, return value included,
with the plain-Python model of bsc_coder_compress (tests/qlfc_model.py) and, where oracle/_ref/libref_units.so is
built, with the real function.  The state tables are read out of that library; two seeded random pairs of tables
stand in where it is missing and show that the tables are the caller's."""
import functools
import os
import struct
import zlib

import numpy as np
import pytest

import qlfc_model as qm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = qm.ref_lib()
TABLES = qm.state_tables()
needs_tables = pytest.mark.skipif(TABLES is None, reason="the state tables cannot be read: oracle/_ref/libref_units.so not built")
needs_ref = pytest.mark.skipif(REF is None or TABLES is None, reason="oracle/_ref/libref_units.so not built (needs the reference sources)")
LARGE = tuple(n for n in qm.MODEL_CASES if n not in qm.SMALL)


@functools.lru_cache(maxsize=None)
def _tables(which):
    return TABLES if which == "real" else qm.random_tables(which)


@functools.lru_cache(maxsize=None)
def _model(name, which):
    return qm.compress(qm.case(name), _tables(which))


@functools.lru_cache(maxsize=None)
def _real(data):
    return qm.ref_compress(data)


def _batch(segs):
    return b"".join(segs), np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)


def _stage(which="real"):
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


@needs_tables
def test_small_cases_equal_the_model_with_the_real_tables():
    with _stage() as st:
        got, info = _code(st, [qm.case(n) for n in qm.SMALL])
    _check(got, [_model(n, "real") for n in qm.SMALL], qm.SMALL)
    assert info["sub_batches"] == 1 and info["chunks"] == len(qm.SMALL) and info["chunks_raw"] == 0
    stats = {}
    for n in qm.SMALL:   # the model counts runs and events of the chunks it codes to the end
        if _model(n, "real")[1] > 0:
            qm.compress(qm.case(n), TABLES, stats)
    assert info["runs"] >= stats["runs"] and info["events"] >= stats["events"]
    assert len(info["ms_pass"]) == 6 and info["ms_device"] > 0


@needs_tables
@pytest.mark.parametrize("name", LARGE)
def test_large_cases_equal_the_model_with_the_real_tables(name):
    with _stage() as st:
        got, info = _code(st, [qm.case(name)])
    _check(got, [_model(name, "real")], [name])
    assert info["chunks"] == qm.num_chunks(len(qm.case(name)))


@pytest.mark.parametrize("seed", [101, 202])
def test_cases_equal_the_model_with_random_tables(seed):
    names = qm.SMALL + ("a300000", "cycle4s")
    with _stage(seed) as st:
        got, _ = _code(st, [qm.case(n) for n in names])
    _check(got, [_model(n, seed) for n in names], names)
    if TABLES is not None:   # and the tables matter: some case comes out differently with the real ones
        assert any(_model(n, seed) != _model(n, "real") for n in names)


@needs_ref
@pytest.mark.parametrize("names", [qm.SMALL, LARGE, qm.REF_ONLY_CASES], ids=["small", "large", "half_random"])
def test_cases_equal_the_real_function(names):
    with _stage() as st:
        got, info = _code(st, [qm.case(n) for n in names])
        _check(got, [_real(qm.case(n)) for n in names], names)
        if names is qm.REF_ONLY_CASES:
            assert info["chunks_raw"] == 2 and info["chunks"] == 4
            for n in names:   # the one-segment entry point, return value and all
                assert st.compress(qm.case(n)) == _real(qm.case(n))
        else:
            for n in ("len17", "a40", "random4096"):
                assert st.compress(qm.case(n)) == _real(qm.case(n))


def test_one_batch_with_empty_segments_equals_one_by_one_and_two_sub_batches():
    from spring_amd.qlfc import workspace_need
    which = "real" if TABLES is not None else 101
    segs = []
    for n in qm.SMALL:
        segs += [qm.case(n), b""]
    segs = [b"", b""] + segs
    with _stage(which) as st:
        together, info = _code(st, segs)
        assert info["sub_batches"] == 1
        for seg, got in zip(segs, together):
            if not seg:
                assert got == (b"", -3)      # status 1 and no bytes
            else:
                assert _code(st, [seg])[0] == [got]
        _check(together[2::2], [_model(n, which) for n in qm.SMALL], qm.SMALL)
        # a budget that holds every segment alone but not the events of all of them together
        budget = workspace_need(sum(len(s) for s in segs), len(segs)) + info["events"] * 160 // 2
        st.set_workspace_bytes(budget)
        split, info2 = _code(st, segs)
        assert info2["sub_batches"] >= 2 and info2["workspace_bytes"] == budget
        assert split == together
        assert (info2["runs"], info2["events"], info2["chunks"]) == (info["runs"], info["events"], info["chunks"])
        st.set_workspace_bytes(workspace_need(len(qm.case("exp16")), 1) - 1)
        from spring_amd._stage import ReorderError
        with pytest.raises(ReorderError, match="code -1"):
            st.code(*_batch(segs))
        with pytest.raises(ReorderError, match="code -4"):
            st.download()


def test_the_same_call_twice_gives_the_same_bytes():
    which = "real" if TABLES is not None else 202
    segs = [qm.case(n) for n in ("bwt5000", "all256", "a300000", "letters9")]
    with _stage(which) as st:
        a, _ = _code(st, segs)
        b, _ = _code(st, segs)
    assert a == b


def _streams_run(ss, name, pe, preserve_order, B):
    z = np.load(os.path.join(GOLDEN, "enc_%s.npz" % name))
    N = len(z["rlen"])
    return ss.from_host(z["pos"], z["rc"], z["noise"], z["noisepos"], z["order"], z["rlen"], z["unaligned"], N, pe,
                        preserve_order, B)


@needs_ref
def test_from_bwt_on_the_streams_of_a_fixture_and_whole_bsc_blocks():
    """StreamsStage -> BwtStage -> QlfcStage without the host in between: every segment equals the real coder on the
    downloaded transform; with the 28-byte header (libbsc.cpp:270-301) in front, a block equals the real bsc_compress
    and the real bsc_decompress returns the slice."""
    from spring_amd.bwt import BwtStage
    from spring_amd.streams import StreamsStage
    adler = lambda b: zlib.adler32(b) & 0xffffffff
    with StreamsStage() as ss, BwtStage() as bw, _stage() as st:
        _streams_run(ss, "var2k", False, False, 2120)
        bw.transform(ss)
        res = bw.download()
        info = st.code(bw)
        got = st.segments()
        after = bw.download()
        assert after["bwt"] == res["bwt"]      # the block-sort context is left as it was
        stream, _, _ = bw.segments()
        off = res["seg_off"]
        assert info["num_segments"] == len(off) - 1 >= 7
        for j in range(len(off) - 1):
            assert got[j] == _real(res["bwt"][int(off[j]):int(off[j + 1])]), j
        slices = {int(s): ss.download(int(s))[0] for s in stream}
    picked = [j for j in range(len(off) - 1) if int(off[j + 1] - off[j]) >= 2048 and got[j][1] > 0][:4]
    assert len(picked) >= 3
    for j in picked:
        seg, n = slices[int(stream[j])], int(off[j + 1] - off[j])
        assert len(seg) == n                   # one block, one cut: the slice is the segment
        body = got[j][0] + bytes([0])          # below 64 KiB bsc_compress drops the secondary indexes
        assert len(body) < n
        head = struct.pack("<iiiiII", len(body) + 28, n, 1 | (1 << 5), int(res["primary"][j]), adler(seg), adler(body))
        block = head + struct.pack("<I", adler(head)) + body
        src = np.frombuffer(seg, np.uint8).copy()
        want = np.zeros(n + 28 + 4096, np.uint8)
        size = REF.bsc_compress(src.ctypes.data, want.ctypes.data, n, 0, 0, 1, 1, 3)
        assert size > 28 and want[:size].tobytes() == block, j
        blk = np.frombuffer(block, np.uint8).copy()
        back = np.zeros(n, np.uint8)
        assert REF.bsc_decompress(blk.ctypes.data, len(blk), back.ctypes.data, n, 3) == 0
        assert back.tobytes() == seg


def test_refusals():
    from spring_amd._stage import ReorderError
    from spring_amd.bwt import BwtStage
    from spring_amd.qlfc import QlfcStage
    data = qm.case("ab32") + qm.case("a40")
    with QlfcStage() as st:
        with pytest.raises(ReorderError, match="code -4"):      # no state tables yet
            st.code(data)
        with pytest.raises(ReorderError, match="code -4"):
            st.compress(data)
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        with pytest.raises(ValueError):
            st.set_state_tables(bytes(100), bytes(8192))
        st.set_state_tables(*_tables(101))
        with pytest.raises(ReorderError, match="code -4"):      # tables, but nothing coded
            st.download()
        for off in ([0, 60, 40, 104], [0, 50, 90], [0, 50, 105], [1, 50, 104]):
            with pytest.raises(ReorderError, match="code -1"):
                st.code(data, off)
            with pytest.raises(ReorderError, match="code -4"):  # a refused call leaves no result
                st.download()
        big = np.zeros((1 << 30) + 1, np.uint8)                 # never touched: refused before any copy
        with pytest.raises(ReorderError, match="code -1"):
            st.code(big)
        del big
        with BwtStage() as bw:                                  # no result yet
            with pytest.raises(ReorderError, match="code -4"):
                st.code(bw)
        try:
            other = BwtStage(device=1)
        except ReorderError:
            other = None                                        # one device: nothing to tell apart
        if other is not None:
            with other:
                other.transform(data)
                with pytest.raises(ReorderError, match="code -1"):
                    st.code(other)
        got, _ = _code(st, [data[:64], b"", data[64:]])
        assert got == [_model("ab32", 101), (b"", -3), _model("a40", 101)]
