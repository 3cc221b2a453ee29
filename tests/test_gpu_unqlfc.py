"""GPU tests of the QLFC decoder stage (include/spring_unqlfc.h).  Every decoded segment is compared byte for byte with
the plain-Python model of bsc_coder_decompress (tests/unqlfc_model.py) and, where oracle/_ref/libref_units.so is built,
with the real function on what the real coder wrote.  The state tables are read out of that library; two seeded random
pairs stand in where it is missing.  The malformed inputs are refusals to check: each one is a rule of the header."""
import functools
import os

import numpy as np
import pytest

import qlfc_model as qm
import unqlfc_model as um

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = qm.ref_lib()
TABLES = qm.state_tables()
needs_ref = pytest.mark.skipif(REF is None or TABLES is None, reason="oracle/_ref/libref_units.so not built (needs the reference sources)")
ANY = "real" if TABLES is not None else 101

# one chunk, coded to its end whatever CheckEOB says: lengths the coder refuses, symbol tables of 1, 2, 3, 255 and 256
# symbols, the escape path, run exponents up to 16, runs at every alignment, payloads that end on a load's edge
ONE_CHUNK = ("len1", "len2", "len16", "len17", "a40", "letters2", "letters3", "no255", "all256", "desc256", "esc100",
             "esc128", "ring100", "exp16", "odd41", "aligned", "units_last", "units_first")
# two, four and eight chunks by the equal split and by the sampled cut
CHUNKED = ("a300000", "cycle4e", "cycle4s", "cycle16e", "cycle16s", "eq262145", "smp4194305")


@functools.lru_cache(maxsize=None)
def _tables(which):
    return TABLES if which == "real" else qm.random_tables(which)


@functools.lru_cache(maxsize=None)
def _text(name, which):
    if name == "odd41":
        return b"Q" * 41
    if name == "aligned":
        return um.aligned_runs()[0]
    if name.startswith("units_"):
        n, seed = um.UNIT_CASES[which][name[6:]]
        return qm._letters(n, 9, seed)
    return qm.case(name)


@functools.lru_cache(maxsize=None)
def _coded(name, which):
    data = _text(name, which)
    if name in CHUNKED:
        coded, rc = qm.compress(data, _tables(which))
        assert rc > 1 and coded[0] == qm.num_chunks(len(data)) > 1
        return coded
    return um.payload(data, _tables(which))


@functools.lru_cache(maxsize=None)
def _model(name, which):
    stats = {}
    out, violation = um.decompress(_coded(name, which), len(_text(name, which)), _tables(which), stats)
    assert violation is None
    return out, stats


def _stage(which):
    from spring_amd.unqlfc import UnqlfcStage
    st = UnqlfcStage()
    st.set_state_tables(*_tables(which))
    return st


def _coder(which):
    from spring_amd.qlfc import QlfcStage
    st = QlfcStage()
    st.set_state_tables(*_tables(which))
    return st


def _batch(segs):
    return b"".join(segs), np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)


def _decode(st, coded, sizes):
    data, off = _batch(coded)
    info = st.decode(data, off, sizes)
    assert info["num_segments"] == len(coded) and info["bytes_in"] == len(data) and info["bytes_out"] == sum(sizes)
    return st.segments(), info


@pytest.mark.parametrize("which", [101, 202])
def test_device_equals_the_model(which):
    names = ONE_CHUNK + CHUNKED
    want = [_model(n, which) for n in names]
    with _stage(which) as st:
        got, info = _decode(st, [_coded(n, which) for n in names], [len(_text(n, which)) for n in names])
    for name, g, (w, _) in zip(names, got, want):
        assert g == w == _text(name, which), name
    assert info["chunks"] == len(ONE_CHUNK) + sum(qm.num_chunks(len(_text(n, which))) for n in CHUNKED)
    assert info["runs"] == sum(s["runs"] for _, s in want) and info["events"] == sum(s["events"] for _, s in want)
    assert info["chunks_raw"] == 0 and info["skipped"] == 0 and info["sub_batches"] == 1
    assert len(info["ms_pass"]) == 3 and info["ms_device"] > 0
    # what the cases are for, read off the model's counters
    assert _model("a40", which)[1]["max_exp"] == 5 and _model("exp16", which)[1]["max_exp"] == 16
    assert _model("a300000", which)[1]["max_exp"] == 17 and _model("aligned", which)[1]["max_exp"] == 7
    assert _model("units_last", which)[1]["payload_units"] == [256] and _model("units_first", which)[1]["payload_units"] == [257]
    assert all(2 * _model(n, which)[1]["escaped"] > _model(n, which)[1]["runs"] for n in ("esc100", "esc128", "ring100"))
    assert names.index("aligned") == names.index("odd41") + 1      # the runs start at odd addresses of the output too


@needs_ref
def test_device_equals_the_real_function():
    """What the real bsc_coder_compress wrote, raw chunks in front of, behind and between coded ones included."""
    names = tuple(n for n in qm.SMALL + qm.ESCAPE_CASES + qm.SYMBOL_CASES + qm.RAW_CASES + ("a300000", "cycle4s", "eq262145")
                  + qm.REF_ONLY_CASES if qm.ref_compress(qm.case(n))[1] > 0)
    coded = [qm.ref_compress(qm.case(n))[0] for n in names]
    sizes = [len(qm.case(n)) for n in names]
    with _stage("real") as st:
        got, info = _decode(st, coded, sizes)
        for name, g, c, n in zip(names, got, coded, sizes):
            want, rc = qm.ref_decompress(c, n)
            assert rc == n and g == want == qm.case(name), name
        assert info["chunks_raw"] == 1 + 1 + 2 + 1 + 1
        for n in ("a40", "raw4", "random_a"):
            assert st.decompress(qm.ref_compress(qm.case(n))[0], len(qm.case(n))) == qm.case(n)


def test_from_a_qlfc_context_in_hbm_and_in_sub_batches():
    from spring_amd.unqlfc import workspace_need
    segs = list(qm.many_segments())
    data, off = _batch(segs)
    with _coder(ANY) as ql, _stage(ANY) as st:
        cinfo = ql.code(data, off)
        status = ql.download()["status"]
        before = ql.download()["coded"]
        info = st.decode(ql)
        want = [s if status[j] == 0 else b"" for j, s in enumerate(segs)]
        assert st.segments() == want
        assert ql.download()["coded"] == before                    # the coder's context is left as it was
        assert info["skipped"] == cinfo["not_compressible"] >= 15
        assert info["chunks"] == int((status == 0).sum()) == cinfo["chunks"] - (cinfo["not_compressible"] - 15)
        assert info["bytes_in"] == cinfo["bytes_out"] and info["sub_batches"] == 1
        assert (info["runs"], info["events"]) == (cinfo["runs"], cinfo["events"]) or cinfo["not_compressible"] > 15
        budget = workspace_need(0, info["chunks"] // 3)
        st.set_workspace_bytes(budget)
        info2 = st.decode(ql)
        assert info2["sub_batches"] >= 3 and info2["workspace_bytes"] == budget
        assert st.segments() == want
        assert (info2["runs"], info2["events"], info2["chunks"]) == (info["runs"], info["events"], info["chunks"])
        # a batch with empty segments, host side
        st.set_workspace_bytes(0)
        few = [b"", segs[0], b"", b"", segs[1], b""]
        ql.code(*_batch(few))
        assert st.decode(ql)["skipped"] == 4 and st.segments() == few


def _streams_run(ss, name, pe, preserve_order, B):
    z = np.load(os.path.join(GOLDEN, "enc_%s.npz" % name))
    N = len(z["rlen"])
    return ss.from_host(z["pos"], z["rc"], z["noise"], z["noisepos"], z["order"], z["rlen"], z["unaligned"], N, pe,
                        preserve_order, B)


def test_block_sort_coder_decoder_inverse_without_the_host_in_between():
    """StreamsStage -> BwtStage -> QlfcStage -> UnqlfcStage -> UnbwtStage: only the primary indexes and the status, which
    a block header holds, pass through the host."""
    from spring_amd.bwt import BwtStage
    from spring_amd.streams import StreamsStage
    from spring_amd.unbwt import UnbwtStage
    with StreamsStage() as ss, BwtStage() as bw, _coder(ANY) as ql, _stage(ANY) as uq, UnbwtStage() as ub, UnbwtStage() as direct:
        _streams_run(ss, "var2k", False, False, 2120)
        bw.transform(ss)
        ql.code(bw)
        uq.decode(ql)
        fwd = bw.download()
        status = ql.download()["status"]
        off = fwd["seg_off"]
        S = len(off) - 1
        assert S >= 7 and int((status == 0).sum()) >= 5
        primary = np.where(status == 0, fwd["primary"], 0).astype(np.int32)
        info = ub.invert(uq, primary=primary)
        res = ub.download()
        direct.invert(bw)
        text = direct.download()["text"]
        stream, _, _ = bw.segments()
        slices = {int(s): ss.download(int(s))[0] for s in stream}
        assert info["num_segments"] == S
        checked = 0
        for j in range(S):
            got = res["text"][int(res["seg_off"][j]):int(res["seg_off"][j + 1])]
            want = text[int(off[j]):int(off[j + 1])] if status[j] == 0 else b""
            assert got == want, j
            if status[j] == 0 and len(slices[int(stream[j])]) == len(want):   # one block, one cut: the slice is the segment
                assert got == slices[int(stream[j])], j
                checked += 1
        assert checked >= 3
        with pytest.raises(ValueError):
            ub.invert(uq, primary=primary[:-1])


def test_decompress_on_host_buffers_and_the_same_call_twice():
    names = ("letters3", "esc100", "a300000", "aligned")
    with _stage(ANY) as st:
        for n in names:
            assert st.decompress(_coded(n, ANY), len(_text(n, ANY))) == _text(n, ANY), n
            assert st.info["num_segments"] == 1
        assert st.decompress(b"", 0) == b"" and st.info["skipped"] == 1
        coded, sizes = [_coded(n, ANY) for n in names], [len(_text(n, ANY)) for n in names]
        a, _ = _decode(st, coded, sizes)
        b, _ = _decode(st, coded, sizes)
    assert a == b == [_text(n, ANY) for n in names]


@functools.lru_cache(maxsize=None)
def _malformed(which):
    return um.malformed(_tables(which))


@pytest.mark.parametrize("name", sorted(um.malformed(qm.random_tables(101))))
def test_a_malformed_segment_refuses_the_call(name):
    from spring_amd._stage import ReorderError
    coded, n, violation = _malformed(ANY)[name]
    assert um.decompress(coded, n, _tables(ANY))[1] == violation
    good, size = _coded("letters3", ANY), len(_text("letters3", ANY))
    with _stage(ANY) as st:
        with pytest.raises(ReorderError, match=r"segment 0: .*\(%s.*code -1" % violation):
            st.decode(coded, None, n)
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        with pytest.raises(ReorderError, match=r"segment 2: .*\(%s.*code -1" % violation):
            st.decode(*_batch([good, good, coded, coded]), [size, size, n, n])
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        assert _decode(st, [good, good], [size, size])[0] == [_text("letters3", ANY)] * 2   # and the context goes on


def test_a_flipped_bit_gives_what_the_model_gives():
    from spring_amd._stage import ReorderError
    data = _text("letters3", ANY)
    good = _coded("letters3", ANY)
    outcomes = set()
    with _stage(ANY) as st:
        for bit in (0, 3, 7):
            coded = bytearray(good)
            coded[len(good) // 2] ^= 1 << bit
            want, violation = um.decompress(bytes(coded), len(data), _tables(ANY))
            outcomes.add(violation)
            if violation is None:
                assert len(want) == len(data) and want != data
                assert st.decompress(bytes(coded), len(data)) == want
            else:
                with pytest.raises(ReorderError, match=r"segment 0: .*\(%s.*code -1" % violation):
                    st.decode(bytes(coded), None, len(data))
    print(outcomes)


def test_refusals():
    from spring_amd._stage import ReorderError
    from spring_amd.qlfc import QlfcStage
    from spring_amd.unqlfc import UnqlfcStage, workspace_need
    good, size = _coded("letters3", 101), len(_text("letters3", 101))
    with UnqlfcStage() as st:
        with pytest.raises(ReorderError, match="code -4"):      # no state tables yet
            st.decode(good, None, size)
        with pytest.raises(ReorderError, match="code -4"):
            st.decompress(good, size)
        with pytest.raises(ValueError):
            st.set_state_tables(bytes(100), bytes(8192))
        st.set_state_tables(*_tables(101))
        with pytest.raises(ReorderError, match="code -4"):      # tables, but nothing decoded
            st.download()
        two = good + good
        for off in ([0, 60, 40, len(two)], [0, 50, 90], [0, 50, len(two) + 1], [1, 50, len(two)]):
            with pytest.raises(ReorderError, match="code -1"):
                st.decode(two, off, [size] * (len(off) - 1))
            with pytest.raises(ReorderError, match="code -4"):  # a refused call leaves no result
                st.download()
        with pytest.raises(ValueError):
            st.decode(two, [0, len(good), len(two)], [size])
        with pytest.raises(ReorderError, match="code -1"):      # more than 1 GiB to decode: refused before any copy
            st.decode(good, None, (1 << 30) + 1)
        with QlfcStage() as ql:                                 # no result yet
            ql.set_state_tables(*_tables(101))
            with pytest.raises(ReorderError, match="code -4"):
                st.decode(ql)
        st.set_workspace_bytes(workspace_need(size, 1) - 1)     # one chunk does not fit
        with pytest.raises(ReorderError, match="code -1"):
            st.decode(good, None, size)
        st.set_workspace_bytes(workspace_need(size, 1))
        assert _decode(st, [good, b"", good], [size, 0, size])[0] == [_text("letters3", 101), b"", _text("letters3", 101)]
        assert st.info["sub_batches"] == 2 and st.info["skipped"] == 1
        try:
            other = QlfcStage(device=1)
        except ReorderError:
            other = None                                        # one device: nothing to tell apart
        if other is not None:
            with other:
                other.set_state_tables(*_tables(101))
                other.code(_text("letters3", 101))
                with pytest.raises(ReorderError, match="code -1"):
                    st.decode(other)
