"""GPU tests of the block-sort stage (include/spring_bwt.h).  Every segment is compared with the numpy model of
bsc_bwt_encode (tests/bwt_model.py; never skipped) and, where oracle/_ref/libref_units.so is built, with the real
function as well: bytes, primary index, num_indexes and every index."""
import functools
import os
import struct
import zlib

import numpy as np
import pytest

import bwt_model as bm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = bm.ref_lib()
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref/libref_units.so not built (needs /root/reference)")
KINDS = ("acgt", "bytes", "const", "cac", "tail00", "tailff")


@functools.lru_cache(maxsize=None)
def _want(seg):
    out, primary, idx = bm.bwt(seg)
    if REF is not None:
        r = bm.ref_bwt(seg, bm.FASTMODE | bm.MULTITHREADING) if seg else (b"", 0, np.zeros(0, np.int32))
        assert r[0] == out and r[1] == primary and np.array_equal(r[2], idx), "model and bsc_bwt_encode differ"
    return out, primary, idx


def _batch(segs):
    return b"".join(segs), np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)


def _same(res, segs, what=""):
    off = res["seg_off"]
    assert np.array_equal(off, _batch(segs)[1]), (what, "offsets")
    assert len(res["primary"]) == len(res["num_indexes"]) == len(res["indexes"]) == len(segs)
    for s, seg in enumerate(segs):
        out, primary, idx = _want(seg)
        assert res["bwt"][int(off[s]):int(off[s + 1])] == out, (what, s, len(seg), "bytes")
        assert res["primary"][s] == primary, (what, s, len(seg), "primary index")
        assert res["num_indexes"][s] == len(idx), (what, s, len(seg), "num_indexes")
        assert np.array_equal(res["indexes"][s][:len(idx)], idx), (what, s, len(seg), "indexes")
        assert not res["indexes"][s][len(idx):].any(), (what, s, "indexes behind num_indexes")


def _run(segs, workspace=None):
    from spring_amd.bwt import BwtStage
    data, off = _batch(segs)
    with BwtStage() as st:
        if workspace is not None:
            st.set_workspace_bytes(workspace)
        info = st.transform(data, off)
        assert info["num_segments"] == len(segs) and info["bytes"] == len(data)
        assert info["max_segment"] == max([len(s) for s in segs] + [0])
        return st.download(), info


def _lengths_batch():
    return [bm.contents(KINDS[i % 4], n, seed=i) for i, n in enumerate(bm.LENGTHS)]


def test_every_length_in_one_batch():
    segs = _lengths_batch()
    res, info = _run(segs)
    _same(res, segs, "lengths")
    assert info["sub_batches"] == 1 and 1 <= info["rounds"] <= 15


@pytest.mark.parametrize("kind", KINDS)
def test_contents(kind):
    lens = {"const": [1, 2, 9, 64, 257, 5000], "cac": [3, 7, 65, 1025, 4097], "tail00": [3, 9, 64, 257, 4097],
            "tailff": [3, 9, 64, 257, 4097]}.get(kind, [1, 8, 17, 255, 1024, 4097])
    segs = [bm.contents(kind, n, seed=7) for n in lens]
    res, info = _run(segs)
    _same(res, segs, kind)
    if kind == "const":   # every suffix of A^5000 ties until its end: the doubling runs to the segment's length
        assert info["rounds"] >= 10


def test_dna_of_one_mebibyte_with_planted_repeats():
    seg = bm.dna_with_repeats((1 << 20) + 3)
    res, info = _run([seg])
    _same(res, [seg], "1 MiB + 3")
    assert info["rounds"] >= 9   # the 5000-byte repeats


def test_segments_are_isolated():
    a = bm.contents("acgt", 700, seed=1)
    b = bm.contents("bytes", 300, seed=2)
    segs = [b"", b"", a, a, b"", a[:333], a, b, b"", b + a, b"\x00" * 40, b"\x00" * 41, b""]
    res, _ = _run(segs)
    _same(res, segs, "isolation")
    perm = [7, 2, 12, 9, 0, 3, 5, 11, 10, 1, 6, 4, 8]
    res2, _ = _run([segs[i] for i in perm])
    _same(res2, [segs[i] for i in perm], "isolation, permuted")
    for j, i in enumerate(perm):   # a segment's result does not depend on its neighbours
        assert (res2["bwt"][int(res2["seg_off"][j]):int(res2["seg_off"][j + 1])]
                == res["bwt"][int(res["seg_off"][i]):int(res["seg_off"][i + 1])])
        assert res2["primary"][j] == res["primary"][i] and np.array_equal(res2["indexes"][j], res["indexes"][i])


def test_secondary_indexes_around_64_kib():
    segs = [bm.contents("acgt", 70000, seed=4), bm.contents("bytes", 65536, seed=5)]
    res, _ = _run(segs)
    _same(res, segs, "secondary indexes")
    assert list(res["num_indexes"]) == [(70000 - 1) // bm.index_step(70000), (65536 - 1) // bm.index_step(65536)]
    assert min(res["num_indexes"]) >= 7


def test_sub_batches_give_the_same_result():
    from spring_amd.bwt import BwtStage, workspace_need
    from spring_amd.reorder import ReorderError
    segs = _lengths_batch()
    one, info1 = _run(segs)
    many, info = _run(segs, workspace=workspace_need(4097, 1))
    assert info1["sub_batches"] == 1 and info["sub_batches"] >= 3
    _same(many, segs, "sub-batches")
    assert many["bwt"] == one["bwt"]
    for k in ("seg_off", "primary", "num_indexes", "indexes"):
        assert np.array_equal(many[k], one[k]), k
    data, off = _batch(segs)
    with BwtStage() as st:
        st.set_workspace_bytes(workspace_need(4097, 1) - 1)
        with pytest.raises(ReorderError, match="code -1"):
            st.transform(data, off)
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        st.set_workspace_bytes(0)
        st.transform(data, off)
        _same(st.download(), segs, "after a refusal")


# ------------------------------------------------------------------ the classes of the first key
# The first sort key holds as many text bytes as the segment number leaves room for (bwt_plan.h::key_layout): 7 up to
# 32 segments in a sub-batch, 6 up to 8192, 5 up to 2^21, 4 above; the doubling starts at that width.

def key_bytes(sub_segments):
    """bwt_plan.h::key_layout restated: text bytes in the first key of a sub-batch of this many segments."""
    seg_bits = (max(sub_segments, 1) - 1).bit_length()
    return min(7, (64 - 3 - seg_bits) // 8)


def plan(segs, budget):
    """bwt_plan.h::plan_sub_batches restated (72 bytes a position, 16 a segment) -> segments of every sub-batch."""
    counts, m, k = [], 0, 0
    for seg in segs:
        if k and (m + len(seg)) * 72 + (k + 1) * 16 > budget:
            counts.append(k)
            m = k = 0
        m, k = m + len(seg), k + 1
    return counts + ([k] if k else [])


CLASSES = ((32, 7), (33, 6), (8192, 6), (8193, 5))


@functools.lru_cache(maxsize=None)
def _pool_run(S):
    segs = bm.pool_batch(S)
    return (segs,) + _run(segs)


@pytest.mark.parametrize("S,width", CLASSES)
def test_segment_count_classes(S, width):
    assert key_bytes(S) == width and [key_bytes(x) for x in (1, 1 << 21, (1 << 21) + 1)] == [7, 5, 4]
    segs, res, info = _pool_run(S)
    assert len(segs) == S and len(set(segs)) > 10 and b"" in segs and max(len(s) for s in segs) == 300
    assert any(a == b != b"" for a, b in zip(segs, segs[1:]))   # equal neighbours
    assert info["sub_batches"] == 1   # all S segments share one first key
    _same(res, segs, "%d segments" % S)


def test_the_5_byte_class_cut_into_7_byte_sub_batches():
    from spring_amd.bwt import workspace_need
    segs, one, info1 = _pool_run(8193)
    budget = workspace_need(1200, 32)
    counts = plan(segs, budget)
    assert sum(counts) == 8193 and 2 <= max(counts) <= 32 and key_bytes(max(counts)) == 7 and key_bytes(8193) == 5
    many, info = _run(segs, workspace=budget)
    assert info1["sub_batches"] == 1 and info["sub_batches"] == len(counts) > 256
    assert many["bwt"] == one["bwt"]
    for k in ("seg_off", "primary", "num_indexes", "indexes"):
        assert np.array_equal(many[k], one[k]), k


def test_two_runs_give_identical_bytes():
    segs = _lengths_batch()
    a, _ = _run(segs)
    b, _ = _run(segs)
    assert a["bwt"] == b["bwt"] and np.array_equal(a["primary"], b["primary"]) and np.array_equal(a["indexes"], b["indexes"])


def test_encode_inplace_follows_the_libbsc_contract():
    from spring_amd import _lib
    from spring_amd.bwt import BwtStage
    cases = [bm.contents("acgt", 4097, seed=1), bm.contents("const", 257), bm.contents("tail00", 1025, seed=2),
             bm.contents("bytes", 70000, seed=3)]
    with BwtStage() as st:
        for seg in cases:
            out, primary, idx = _want(seg)
            T = np.frombuffer(seg, np.uint8).copy()
            p, got_idx = st.encode_inplace(T)
            assert p == primary and T.tobytes() == out and np.array_equal(got_idx, idx), len(seg)
            batch = st.download()   # the batch path's result of the same call
            assert batch["bwt"] == out and batch["primary"][0] == primary and batch["num_indexes"][0] == len(idx)
        p, got_idx = st.encode_inplace(None)   # n = 0
        assert p == 0 and len(got_idx) == 0
        T = np.frombuffer(cases[0], np.uint8).copy()   # NULL index pointers
        assert _lib.lib().spring_bwt_encode_inplace(st._h, T.ctypes.data, len(T), None, None) == _want(cases[0])[1]
        assert T.tobytes() == _want(cases[0])[0]


def test_refusals():
    from spring_amd.bwt import BwtStage
    from spring_amd.reorder import ReorderError
    from spring_amd.streams import StreamsStage
    data = bm.contents("acgt", 100)
    with BwtStage() as st:
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        for off in ([0, 60, 40, 100], [0, 50, 90], [0, 50, 101], [1, 50, 100]):
            with pytest.raises(ReorderError, match="code -1"):
                st.transform(data, off)
            with pytest.raises(ReorderError, match="code -4"):   # a refused call leaves no result
                st.download()
        with pytest.raises(ReorderError, match="code -4"):
            st.segments()
        with StreamsStage() as ss:   # no run yet
            with pytest.raises(ReorderError, match="code -4"):
                st.transform(ss)
        with pytest.raises(ReorderError, match="code -1"):
            st.set_block_bytes(0)
        with pytest.raises(ReorderError, match="code -1"):
            st.set_block_bytes((1 << 30) + 1)
        st.transform(data, [0, 40, 40, 100])
        _same(st.download(), [data[:40], b"", data[40:]], "after refusals")


# ------------------------------------------------------------------ from a streams context

def _streams_run(ss, name, pe, preserve_order, B):
    """The stream stage on the encoder streams of a committed fixture (tests/golden/enc_<name>.npz)."""
    z = np.load(os.path.join(GOLDEN, "enc_%s.npz" % name))
    N = len(z["rlen"])
    return ss.from_host(z["pos"], z["rc"], z["noise"], z["noisepos"], z["order"], z["rlen"], z["unaligned"], N, pe,
                        preserve_order, B)


def _slices(ss, block_bytes, streams=range(9)):
    """The host path's view: (stream, block, cut, bytes) of every non-empty slice, cut every block_bytes."""
    out = []
    for s in streams:
        data, off = ss.download(s)
        for b in range(len(off) - 1):
            lo, hi = int(off[b]), int(off[b + 1])
            for c, x in enumerate(range(lo, hi, block_bytes)):
                out.append((s, b, c, data[x:min(x + block_bytes, hi)]))
    return out


@pytest.mark.parametrize("name,pe,preserve_order,B", [("var2k", False, False, 700), ("syn2k_100", True, True, 800)])
def test_from_a_streams_context(name, pe, preserve_order, B):
    from spring_amd.bwt import BwtStage
    from spring_amd.streams import StreamsStage
    with StreamsStage() as ss, BwtStage() as st, BwtStage() as host:
        _streams_run(ss, name, pe, preserve_order, B)
        before = [ss.download(s) for s in range(9)]
        want = _slices(ss, 4096)
        assert max(c for _, _, c, _ in want) >= 1 and len({s for s, _, _, _ in want}) >= 7   # slices are cut
        st.set_block_bytes(4096)
        info = st.transform(ss)
        assert info["num_segments"] == len(want) and info["max_segment"] == 4096
        stream, block, cut = st.segments()
        assert [(int(a), int(b), int(c)) for a, b, c in zip(stream, block, cut)] == [w[:3] for w in want]
        res = st.download()
        segs = [w[3] for w in want]
        _same(res, segs, name)
        hres = (host.transform(*_batch(segs)), host.download())[1]
        assert res["bwt"] == hres["bwt"]
        for k in ("seg_off", "primary", "num_indexes", "indexes"):
            assert np.array_equal(res[k], hres[k]), k
        assert list(host.segments()[0]) == [-1] * len(segs)
        # a mask takes some of the streams
        st.transform(ss, streams=["noise", 5])
        part = [w for w in want if w[0] in (2, 5)]
        assert [int(x) for x in st.segments()[0]] == [w[0] for w in part]
        _same(st.download(), [w[3] for w in part], name + ", two streams")
        after = [ss.download(s) for s in range(9)]
        for (a, ao), (b, bo) in zip(before, after):   # the streams context is left as it was
            assert a == b and np.array_equal(ao, bo)


def test_from_a_streams_context_in_more_than_8192_segments():
    """One read a block and slices cut every 16 bytes: the 5-byte class of the first key from a streams context."""
    from spring_amd.bwt import BwtStage
    from spring_amd.streams import StreamsStage
    with StreamsStage() as ss, BwtStage() as st, BwtStage() as host:
        _streams_run(ss, "var2k", False, False, 1)
        want = _slices(ss, 16)
        assert len(want) > 8192 and key_bytes(len(want)) == 5
        assert max(c for _, _, c, _ in want) >= 1 and len({s for s, _, _, _ in want}) >= 7   # slices are cut
        st.set_block_bytes(16)
        info = st.transform(ss)
        assert info["num_segments"] == len(want) and info["max_segment"] == 16 and info["sub_batches"] == 1
        stream, block, cut = st.segments()
        assert [(int(a), int(b), int(c)) for a, b, c in zip(stream, block, cut)] == [w[:3] for w in want]
        res = st.download()
        segs = [w[3] for w in want]
        _same(res, segs, "var2k, 16 bytes")
        hres = (host.transform(*_batch(segs)), host.download())[1]
        assert host.info["sub_batches"] == 1 and res["bwt"] == hres["bwt"]
        for k in ("seg_off", "primary", "num_indexes", "indexes"):
            assert np.array_equal(res[k], hres[k]), k


def _bsc_block(seg, out, primary, idx, adler):
    """The block bsc_compress writes for LZP off (libbsc.cpp:270-301), from a transform computed elsewhere."""
    n = len(seg)
    buf = np.frombuffer(out, np.uint8).copy()
    coded = np.zeros(n + 4096, np.uint8)
    size = REF.bsc_coder_compress(buf.ctypes.data, coded.ctypes.data, n, 1, 3)   # LIBBSC_CODER_QLFC_STATIC, features 3
    assert size >= 0
    if n < 64 * 1024:
        idx = idx[:0]
    body = coded[:size].tobytes() + np.asarray(idx, "<i4").tobytes() + bytes([len(idx)])
    assert len(body) < n, "not compressible: bsc_compress would store this block"
    head = struct.pack("<iiiiII", len(body) + 28, n, 1 | (1 << 5), primary, adler(seg), adler(body))
    return head + struct.pack("<I", adler(head)) + body


@needs_ref
def test_blocks_equal_bsc_compress_without_lzp_and_decompress():
    """Device transform + the real bsc_coder_compress + the 28-byte header equals the real bsc_compress(lzpHashSize 0,
    lzpMinLen 0) byte for byte, and the real bsc_decompress gives the slice back.  The Adler-32 fields are
    zlib.adler32: the blocks built with it equal the library's own, so bsc_adler32 is the same function."""
    from spring_amd.bwt import BwtStage
    from spring_amd.streams import StreamsStage
    with StreamsStage() as ss, BwtStage() as st:
        _streams_run(ss, "var2k", False, False, 2120)
        st.transform(ss)
        res = st.download()
        stream, _, _ = st.segments()
        off = res["seg_off"]
        segs = {int(s): ss.download(int(s))[0] for s in stream}
        picked = [j for j in range(len(stream)) if int(off[j + 1] - off[j]) >= 2048][:4]
        assert len(picked) >= 3
        cases = [(segs[int(stream[j])], res["bwt"][int(off[j]):int(off[j + 1])], int(res["primary"][j]),
                  res["indexes"][j][:res["num_indexes"][j]]) for j in picked]
        big = bm.contents("acgt", 70000, seed=4)   # one block with secondary indexes in it
        T = np.frombuffer(big, np.uint8).copy()
        p, idx = st.encode_inplace(T)
        cases.append((big, T.tobytes(), p, idx))
    for seg, out, primary, idx in cases:
        n = len(seg)
        block = _bsc_block(seg, out, primary, idx, lambda b: zlib.adler32(b) & 0xffffffff)
        src = np.frombuffer(seg, np.uint8).copy()
        want = np.zeros(n + 28 + 4096, np.uint8)
        size = REF.bsc_compress(src.ctypes.data, want.ctypes.data, n, 0, 0, 1, 1, 3)
        assert size > 28 and want[:size].tobytes() == block, n
        blk = np.frombuffer(block, np.uint8).copy()
        back = np.zeros(n, np.uint8)
        assert REF.bsc_decompress(blk.ctypes.data, len(blk), back.ctypes.data, n, 3) == 0
        assert back.tobytes() == seg
        assert REF.bsc_adler32(src.ctypes.data, n, 3) == zlib.adler32(seg) & 0xffffffff
