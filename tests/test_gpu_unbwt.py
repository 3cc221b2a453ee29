"""GPU tests of the inverse block-sort stage (include/spring_unbwt.h).  Every segment is compared with the numpy model of
bsc_bwt_decode (tests/unbwt_model.py; never skipped) and, where oracle/_ref/libref_units.so is built, with the real
function as well.  The inputs are transforms made by the forward model, so every result is also the text it came from."""
import functools

import numpy as np
import pytest

import bwt_model as bm
import unbwt_model as um

pytestmark = pytest.mark.gpu

REF = um.ref_lib()
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref/libref_units.so not built (needs /root/reference)")
KINDS = ("acgt", "bytes", "const", "cac", "tail00", "tailff")


@functools.lru_cache(maxsize=None)
def _fwd(text):
    """text -> (transform, primary index, secondary indexes as a tuple) by the forward model."""
    out, primary, idx = bm.bwt(text)
    return out, primary, tuple(int(x) for x in idx)


@functools.lru_cache(maxsize=None)
def _want(L, primary):
    """(transform, primary) -> the text by the model, pinned to the real function where that is built."""
    T = um.unbwt(L, primary)
    if REF is not None and len(L):
        rc, r = um.ref_unbwt(L, primary, bm.MULTITHREADING)
        assert rc == 0 and r == T, "model and bsc_bwt_decode differ"
    return T


def _batch(segs):
    return b"".join(segs), np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)


def _same(res, pairs, what=""):
    """pairs: (transform, primary) per segment."""
    off = res["seg_off"]
    assert np.array_equal(off, _batch([p[0] for p in pairs])[1]), (what, "offsets")
    for s, (L, primary) in enumerate(pairs):
        assert res["text"][int(off[s]):int(off[s + 1])] == _want(L, primary), (what, s, len(L), primary)


def _run(pairs, workspace=None, head_spacing=None):
    from spring_amd.unbwt import UnbwtStage
    data, off = _batch([p[0] for p in pairs])
    with UnbwtStage() as st:
        if workspace is not None:
            st.set_workspace_bytes(workspace)
        if head_spacing is not None:
            st.set_head_spacing(head_spacing)
        info = st.invert(data, off, [p[1] for p in pairs])
        assert info["num_segments"] == len(pairs) and info["bytes"] == len(data)
        assert info["max_segment"] == max([len(p[0]) for p in pairs] + [0])
        assert info == st.get_info()
        return st.download(), info


def _texts(texts, what, **kw):
    """Transforms the texts with the forward model, inverts them on the device: model, real function and the texts."""
    pairs = [_fwd(t)[:2] for t in texts]
    res, info = _run(pairs, **kw)
    _same(res, pairs, what)
    assert res["text"] == b"".join(texts), (what, "not the texts the transforms came from")
    return res, info


def _lengths_batch():
    return [bm.contents(KINDS[i % len(KINDS)], n, seed=i) for i, n in enumerate(bm.LENGTHS)]


def test_every_length_in_one_batch():
    res, info = _texts(_lengths_batch(), "lengths")
    assert info["sub_batches"] == 1 and info["head_spacing"] == 64 and 1 <= info["max_walk"] <= 4097
    assert info["heads"] >= 2 * len(bm.LENGTHS) + sum(bm.LENGTHS) // 64


@pytest.mark.parametrize("kind", KINDS)
def test_contents(kind):
    _texts([bm.contents(kind, 4097, seed=7)], kind)


PERIODIC = {"AB": b"AB" * 8192, "ACGT": (b"ACGT" * 4097)[:16385], "AAB": b"AAB" * 4096,
            "unit64": (np.random.default_rng(11).integers(0, 256, 64, dtype=np.uint8).tobytes() * 313)[:20000],
            "constant": b"G" * 10000}


@pytest.mark.parametrize("what", sorted(PERIODIC))
def test_periodic_texts(what):
    text = PERIODIC[what]
    for K in (16, 64):
        res, info = _texts([text], what, head_spacing=K)
        assert info["head_spacing"] == K
        assert info["max_walk"] <= len(text), (what, K, info["max_walk"])   # the bound of the walk is never reached


def test_segments_are_isolated():
    a = bm.contents("acgt", 700, seed=1)
    b = bm.contents("bytes", 300, seed=2)
    segs = [b"", b"", a, a, b"", a[:333], a, b, b"", b + a, b"\x00" * 40, b"\x00" * 41, b""]
    res, _ = _texts(segs, "isolation")
    perm = [7, 2, 12, 9, 0, 3, 5, 11, 10, 1, 6, 4, 8]
    res2, _ = _texts([segs[i] for i in perm], "isolation, permuted")
    for j, i in enumerate(perm):   # a segment's result does not depend on its neighbours
        assert (res2["text"][int(res2["seg_off"][j]):int(res2["seg_off"][j + 1])]
                == res["text"][int(res["seg_off"][i]):int(res["seg_off"][i + 1])])


def test_sizes_where_bsc_compress_keeps_indexes():
    _texts([bm.contents("acgt", 70000, seed=4), bm.contents("bytes", 65536, seed=5)], "index sizes")


def test_dna_of_one_mebibyte_with_planted_repeats():
    seg = bm.dna_with_repeats((1 << 20) + 3)
    _, info = _texts([seg], "1 MiB + 3")
    assert info["rank_rounds"] >= 14 and info["max_walk"] < 4096


def test_a_wrong_primary_with_a_complete_path_gives_the_models_text():
    assert um.path_length(b"annbaa", 6) == 6
    res, _ = _run([(b"annbaa", 6), (b"annbaa", 4)])
    _same(res, [(b"annbaa", 6), (b"annbaa", 4)], "annbaa")
    assert res["text"][6:] == b"banana" and res["text"][:6] != b"banana"


def test_sub_batches_give_the_same_result():
    from spring_amd.reorder import ReorderError
    from spring_amd.unbwt import UnbwtStage, workspace_need
    segs = _lengths_batch()
    one, info1 = _texts(segs, "one sub-batch")
    many, info = _texts(segs, "sub-batches", workspace=workspace_need(4097, 1))
    assert info1["sub_batches"] == 1 and info["sub_batches"] >= 3
    assert many["text"] == one["text"] and np.array_equal(many["seg_off"], one["seg_off"])
    pairs = [_fwd(t)[:2] for t in segs]
    data, off = _batch([p[0] for p in pairs])
    with UnbwtStage() as st:
        st.set_workspace_bytes(workspace_need(4097, 1) - 1)   # a segment beyond the budget
        with pytest.raises(ReorderError, match="code -1"):
            st.invert(data, off, [p[1] for p in pairs])
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        st.set_workspace_bytes(0)
        st.invert(data, off, [p[1] for p in pairs])
        _same(st.download(), pairs, "after a refusal")


def test_from_a_block_sort_context():
    from spring_amd.bwt import BwtStage
    from spring_amd.reorder import ReorderError
    from spring_amd.unbwt import UnbwtStage
    segs = _lengths_batch() + [bm.contents("acgt", 70000, seed=4)]
    data, off = _batch(segs)
    with BwtStage() as fw, UnbwtStage() as st:
        with pytest.raises(ReorderError, match="code -4"):   # no result yet
            st.invert(fw)
        fw.transform(data, off)
        before = fw.download()
        info = st.invert(fw)
        assert info["num_segments"] == len(segs) and info["bytes"] == len(data)
        res = st.download()
        assert res["text"] == data and np.array_equal(res["seg_off"], off)
        pairs = [(before["bwt"][int(off[s]):int(off[s + 1])], int(before["primary"][s])) for s in range(len(segs))]
        _same(res, pairs, "from_bwt")
        after = fw.download()   # the forward result is left as it was
        assert after["bwt"] == before["bwt"]
        for k in ("seg_off", "primary", "num_indexes", "indexes"):
            assert np.array_equal(after[k], before[k]), k


def _inplace_cases():
    return [bm.contents("acgt", 4097, seed=1), bm.contents("const", 257), bm.contents("tail00", 1025, seed=2),
            bm.contents("bytes", 70000, seed=3), b"x"]


def test_decode_inplace_on_a_model_transform():
    from spring_amd import _lib
    from spring_amd.reorder import ReorderError
    from spring_amd.unbwt import UnbwtStage
    with UnbwtStage() as st:
        for text in _inplace_cases():
            out, primary, idx = _fwd(text)
            for indexes in (None, idx):
                T = np.frombuffer(out, np.uint8).copy()
                st.decode_inplace(T, primary, indexes)
                assert T.tobytes() == text == _want(out, primary), len(text)
                assert st.download()["text"] == text   # the batch path's result of the same call
        st.decode_inplace(None, 0)   # n = 0
        assert st.info["bytes"] == 0
        with pytest.raises(ReorderError, match="code -1"):
            st.decode_inplace(None, 1)
        T = np.frombuffer(b"annbaa", np.uint8).copy()
        for bad in (0, 7, -3, 5):   # out of range, and a short path: refused, T untouched
            with pytest.raises(ReorderError, match="code -1"):
                st.decode_inplace(T, bad)
            assert T.tobytes() == b"annbaa"
        assert _lib.lib().spring_unbwt_decode_inplace(st._h, T.ctypes.data, 6, 4, 0, None) == 0
        assert T.tobytes() == b"banana"


@needs_ref
def test_decode_inplace_on_a_real_bsc_bwt_encode_output():
    from spring_amd.unbwt import UnbwtStage
    with UnbwtStage() as st:
        for text in _inplace_cases():
            out, primary, idx = bm.ref_bwt(text, bm.FASTMODE | bm.MULTITHREADING)
            T = np.frombuffer(out, np.uint8).copy()
            st.decode_inplace(T, primary, idx)
            assert T.tobytes() == text, len(text)


def test_short_paths_are_refused():
    from spring_amd.reorder import ReorderError
    from spring_amd.unbwt import UnbwtStage
    good = [_fwd(bm.contents("acgt", 300, seed=s))[:2] for s in (1, 2)]
    with UnbwtStage() as st:
        for p, steps in ((1, 1), (2, 3), (3, 5), (5, 2)):
            assert um.path_length(b"annbaa", p) == steps < 6
            with pytest.raises(ReorderError, match=r"segment 0.*\(code -1\)"):
                st.invert(b"annbaa", None, p)
            with pytest.raises(ReorderError, match="code -4"):
                st.download()
            with pytest.raises(ReorderError, match="code -4"):
                st.get_info()
            pairs = [good[0], (b"annbaa", p), good[1]]   # ... and as the middle one of three
            data, off = _batch([x[0] for x in pairs])
            with pytest.raises(ReorderError, match=r"segment 1.*\(code -1\)"):
                st.invert(data, off, [x[1] for x in pairs])
            with pytest.raises(ReorderError, match="code -4"):
                st.download()
        # one byte of a transform changed
        text = bm.contents("acgt", 4097)
        out, primary = _fwd(text)[:2]
        broken = bytearray(out)
        broken[100] ^= 1
        broken = bytes(broken)
        steps = um.path_length(broken, primary)
        assert steps == 2656 < 4097
        with pytest.raises(ReorderError, match="code -1"):
            st.invert(broken, None, primary)
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        # three sub-batches, the broken segment alone in the second: the result is dropped as a whole
        from spring_amd.unbwt import workspace_need
        pairs = [good[0], good[1], (broken, primary), (b"annbaa", 4)]
        data, off = _batch([x[0] for x in pairs])
        st.set_workspace_bytes(workspace_need(4097, 1))
        with pytest.raises(ReorderError, match=r"segment 2.*\(code -1\)"):
            st.invert(data, off, [x[1] for x in pairs])
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        st.set_workspace_bytes(0)
        st.invert(out, None, primary)   # the context works on
        assert st.download()["text"] == text


# ------------------------------------------------------------------ segment counts and head spacings
# The stable sort runs over 40 + bits_for(segments) bits and the heads are laid out by the spacing K: the batches of
# tests/test_gpu_bwt.py (32, 33, 8192 and 8193 segments) and every K the library takes.

CLASSES = (32, 33, 8192, 8193)
SPACINGS = (16, 32, 64, 128, 256, 512, 1024)


@pytest.mark.parametrize("S", CLASSES)
def test_segment_count_classes(S):
    texts = bm.pool_batch(S)
    assert len(texts) == S
    _, info = _texts(texts, "%d segments" % S)
    assert info["sub_batches"] == 1 and info["max_walk"] <= 300
    assert info["heads"] == -(-(sum(len(t) for t in texts) + S) // 64) + 2 * S


def test_from_a_block_sort_context_of_8193_segments():
    from spring_amd.bwt import BwtStage
    from spring_amd.unbwt import UnbwtStage
    texts = bm.pool_batch(8193)
    data, off = _batch(texts)
    with BwtStage() as fw, UnbwtStage() as st:
        assert fw.transform(data, off)["sub_batches"] == 1
        info = st.invert(fw)
        assert info["num_segments"] == 8193 and info["bytes"] == len(data) and info["sub_batches"] == 1
        res = st.download()
        assert res["text"] == data and np.array_equal(res["seg_off"], off)


SPACING_INPUTS = {"lengths": _lengths_batch, "periodic": lambda: [PERIODIC[k] for k in sorted(PERIODIC)],
                  "8193 segments": lambda: bm.pool_batch(8193), "70000 bytes": lambda: [bm.contents("acgt", 70000, seed=4)]}


@pytest.mark.parametrize("what", sorted(SPACING_INPUTS))
def test_every_head_spacing(what):
    texts = SPACING_INPUTS[what]()
    S, nbytes, longest = len(texts), sum(len(t) for t in texts), max(len(t) for t in texts)
    first = None
    for K in SPACINGS:
        res, info = _texts(texts, (what, K), head_spacing=K)   # the model's text, and the texts themselves
        assert info["head_spacing"] == K, (what, K)
        assert 1 <= info["max_walk"] <= longest, (what, K, info["max_walk"])   # the bound of the walk is never reached
        assert info["sub_batches"] == 1 and info["heads"] == -(-(nbytes + S) // K) + 2 * S, (what, K, info["heads"])
        first = first or res
        assert res["text"] == first["text"] and np.array_equal(res["seg_off"], first["seg_off"]), (what, K)


def _short_primary(L, primary):
    """A primary index whose path from row 0 is short (as test_short_paths_are_refused picks them)."""
    for p in range(1, len(L) + 1):
        if p != primary and um.path_length(L, p) < len(L):
            return p
    raise AssertionError("every primary index of this transform has a complete path")


def test_short_paths_among_8193_segments_are_refused():
    from spring_amd.reorder import ReorderError
    from spring_amd.unbwt import UnbwtStage
    pairs = [_fwd(t)[:2] for t in bm.pool_batch(8193)]
    good = list(pairs)
    for s in (8000, 40):
        assert len(pairs[s][0]) >= 255
        pairs[s] = (pairs[s][0], _short_primary(*pairs[s]))
    data, off = _batch([p[0] for p in pairs])
    with UnbwtStage() as st:
        for K in (16, 64, 1024):
            st.set_head_spacing(K)
            with pytest.raises(ReorderError, match=r"segment 40\b.*\(code -1\)"):
                st.invert(data, off, [p[1] for p in pairs])
            with pytest.raises(ReorderError, match="code -4"):
                st.download()
        pairs[40] = good[40]   # the later one alone
        with pytest.raises(ReorderError, match=r"segment 8000\b.*\(code -1\)"):
            st.invert(data, off, [p[1] for p in pairs])
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        st.invert(data, off, [p[1] for p in good])   # the context works on
        _same(st.download(), good, "after the refusals")


def test_refusals():
    from spring_amd import _lib
    from spring_amd.bwt import BwtStage
    from spring_amd.reorder import ReorderError
    from spring_amd.unbwt import UnbwtStage
    text = bm.contents("acgt", 100)
    out, primary = _fwd(text)[:2]
    with UnbwtStage() as st:
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        with pytest.raises(ReorderError, match="code -4"):
            st.get_info()
        for p in (0, 101, -1):   # primary index out of range
            with pytest.raises(ReorderError, match="primary index.*code -1"):
                st.invert(out, None, p)
            with pytest.raises(ReorderError, match="code -4"):
                st.download()
        with pytest.raises(ReorderError, match="primary index.*code -1"):   # an empty segment's is 0
            st.invert(out, [0, 100, 100], [primary, 1])
        for off in ([0, 60, 40, 100], [0, 50, 90], [0, 50, 101], [1, 50, 100]):   # bad offsets
            with pytest.raises(ReorderError, match="code -1"):
                st.invert(out, off, [1] * (len(off) - 1))
            with pytest.raises(ReorderError, match="code -4"):   # a refused call leaves no result
                st.download()
        L = _lib.lib()
        one = np.array([1], np.int32)
        assert L.spring_unbwt_from_host(st._h, None, 5, None, one.ctypes.data, 0, None) == -1   # NULL buffer with bytes
        buf = np.frombuffer(out, np.uint8)
        assert L.spring_unbwt_from_host(st._h, buf.ctypes.data, 100, None, None, 0, None) == -1   # NULL primary indexes
        with pytest.raises(ReorderError, match="code -1"):
            st.set_head_spacing(48)
        with pytest.raises(ReorderError, match="code -1"):
            st.set_head_spacing(8)
        with BwtStage() as fw:   # nothing transformed
            with pytest.raises(ReorderError, match="code -4"):
                st.invert(fw)
        st.invert(out + b"" + out, [0, 100, 100, 200], [primary, 0, primary])
        assert st.download()["text"] == text + text


def test_two_runs_give_identical_bytes():
    from spring_amd.unbwt import UnbwtStage
    pairs = [_fwd(t)[:2] for t in _lengths_batch()]
    data, off = _batch([p[0] for p in pairs])
    with UnbwtStage() as st:
        st.invert(data, off, [p[1] for p in pairs])
        a = st.download()
        st.invert(data, off, [p[1] for p in pairs])
        b = st.download()
    assert a["text"] == b["text"] and np.array_equal(a["seg_off"], b["seg_off"])
    _same(a, pairs, "two runs")
