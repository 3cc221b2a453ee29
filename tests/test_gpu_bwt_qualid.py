"""GPU tests of the block sort over the quality / id blocks of a QualIdStage (spring_bwt_from_qualid) and of the
run-aware first keys (spring_bwt_set_run_keys).  Every segment is compared with the numpy model of bsc_bwt_encode
(tests/bwt_model.py; never skipped) and, where oracle/_ref/libref_units.so is built, with the real function as well:
bytes, primary index, num_indexes and every index."""
import collections
import functools
import os

import numpy as np
import pytest

import bwt_model as bm
import bwt_runs_model as rm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = bm.ref_lib()
KINDS = ("acgt", "bytes", "const", "cac", "tail00", "tailff")
HARD = b"A" * 3000 + b"C" + b"A" * 2000 + b"B"


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


def _equal(a, b, what=""):
    assert a["bwt"] == b["bwt"], (what, "bytes")
    for k in ("seg_off", "primary", "num_indexes", "indexes"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _run(segs, run_keys=None, workspace=None):
    """run_keys: None (off) or the cap_bits to switch them on with."""
    from spring_amd.bwt import BwtStage
    data, off = _batch(segs)
    with BwtStage() as st:
        if workspace is not None:
            st.set_workspace_bytes(workspace)
        if run_keys is not None:
            st.set_run_keys(True, run_keys)
        info = st.transform(data, off)
        assert info["num_segments"] == len(segs) and info["bytes"] == len(data)
        if run_keys is None:
            assert info["run_positions"] == 0
        return st.download(), info


# ------------------------------------------------------------------ from a quality / id context

def _fastq(j):
    return open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb").read()


def _cuts(qs, kind, block_bytes):
    """The host restatement of the cut: (block, cut, bytes) of every non-empty block of the context, cut every
    block_bytes bytes regardless of line ends."""
    data, _, off = qs.download(kind)
    out = []
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        for c, x in enumerate(range(lo, hi, block_bytes)):
            out.append((b, c, data[x:min(x + block_bytes, hi)]))
    return out


def _check_qualid(qs, st, host, kind, block_bytes, src_id, what):
    """transform(qs) against the restated cut, the model, and transform(host bytes, offsets); qs is left as it was."""
    before = qs.download(kind)
    want = _cuts(qs, kind, block_bytes or 64 << 20)
    info = st.transform(qs, kind=kind, block_bytes=block_bytes)
    assert info["num_segments"] == len(want) and info["bytes"] == len(before[0])
    stream, block, cut = st.segments()
    assert [(int(a), int(b), int(c)) for a, b, c in zip(stream, block, cut)] == [(src_id, b, c) for b, c, _ in want], what
    res = st.download()
    segs = [w[2] for w in want]
    _same(res, segs, what)
    host.transform(*_batch(segs))
    _equal(res, host.download(), what)
    after = qs.download(kind)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]), what
    return want, res


@pytest.mark.parametrize("run_keys", [None, 3, 0])
def test_from_a_quality_context(run_keys):
    """test_1.fastq single-end under a fixed permutation and the Illumina table, 7 reads a block, cut every 256 bytes;
    both files paired-end; the id blocks; block_bytes = 0; and back through the inverse.  With run keys off, with
    cap_bits = 3 and with the layout's own cap: the results do not depend on them."""
    from spring_amd import BwtStage, QualIdStage, UnbwtStage
    from spring_amd import _lib
    f1, f2 = _fastq(1), _fastq(2)
    n = f1.count(b"\n") // 4
    table = QualIdStage.quality_table("illumina")
    with QualIdStage() as qs, BwtStage() as st, BwtStage() as host, UnbwtStage() as inv:
        if run_keys is not None:
            st.set_run_keys(True, run_keys)
        qs.set_order(np.random.default_rng(5).permutation(n).astype(np.uint32), n)
        qi = qs.from_fastq(f1, table=table, num_reads_per_block=7)
        assert qi["num_blocks"] == (n + 6) // 7 and qi["bytes_changed"] > 0
        want, res = _check_qualid(qs, st, host, "quality", 256, _lib.BWT_SRC_QUALITY, "single-end")
        assert max(c for _, c, _ in want) >= 2 and min(len(s) for _, _, s in want) < 256   # cut, and a short last cut
        assert st.info["max_segment"] == 256
        assert (st.info["run_positions"] > 0) == (run_keys is not None)
        inv.invert(st)   # the inverse takes the result in HBM and gives the quality bytes back
        back = inv.download()
        assert back["text"] == qs.download("quality")[0] and np.array_equal(back["seg_off"], res["seg_off"])
        _check_qualid(qs, st, host, "id", 256, _lib.BWT_SRC_ID, "ids")
        want0, _ = _check_qualid(qs, st, host, "quality", 0, _lib.BWT_SRC_QUALITY, "block_bytes = 0")
        assert [(b, c) for b, c, _ in want0] == [(b, 0) for b in range(qi["num_blocks"])]   # one cut per block
        qs.set_order(np.random.default_rng(6).permutation(2 * n).astype(np.uint32), 2 * n, True)
        for j, f in enumerate((f1, f2)):
            qs.from_fastq(f, table=table, num_reads_per_block=7)
            _check_qualid(qs, st, host, "quality", 256, _lib.BWT_SRC_QUALITY, "paired-end, file %d" % (j + 1))


# ------------------------------------------------------------------ run keys over host batches

def _lengths_batch():
    return [bm.contents(KINDS[i % 6], n, seed=i) for i, n in enumerate(bm.LENGTHS)]


def _run_cases():
    """bm.LENGTHS x all six kinds; the quality-like pool; runs of CAP - 1, CAP, CAP + 1 bytes for cap_bits = 3 (CAP = 7),
    on both sides and at a segment's end; runs that end a segment; equal neighbouring segments."""
    segs = [bm.contents(kind, n, seed=2) for kind in KINDS for n in bm.LENGTHS if n >= 3 or kind == "acgt"]
    segs += rm.quality_like_pool()
    for r in (6, 7, 8):
        segs += [b"G" * r, b"AC" + b"G" * r, b"G" * r + b"A" + b"G" * r + b"T" + b"G" * r,
                 b"T" + b"G" * r + b"A" + b"G" * (r + 1) + b"T" + b"G" * (r - 1) + b"C" + b"G" * r,
                 b"\x00" * r + b"\xff" * r + b"\x00" * r, b"\xff" * r + b"\x00" * r + b"\xff" * r + b"\x01"]
    pool = rm.quality_like_pool(seed=12, count=4)
    segs += [pool[0], pool[0], b"", pool[1], pool[1], pool[1], b"G" * 40, b"G" * 40, b"G" * 41]
    return segs


@functools.lru_cache(maxsize=None)
def _plain(which):
    return _run({"cases": _run_cases, "lengths": _lengths_batch}[which]())


@pytest.mark.parametrize("cap_bits", [3, 0])
def test_run_keys_over_a_host_batch(cap_bits):
    segs = _run_cases()
    assert len(segs) > 400 and any(a == b != b"" for a, b in zip(segs, segs[1:]))
    res, info = _run(segs, run_keys=cap_bits)
    _same(res, segs, "run keys, cap_bits %d" % cap_bits)
    _equal(res, _plain("cases")[0], "run keys on against off")
    _, k, R, _ = rm.run_key_layout(len(segs))
    want = sum(rm.first_keys(np.frombuffer(s, np.uint8), k, R, cap_bits)[2] for s in segs if s)
    assert info["run_positions"] == want > 0 and info["sub_batches"] == 1


def test_rounds_on_two_long_runs():
    """A^3000 C A^2000 B.  The run key leaves 1 997 pairs tied (the positions with 4 .. 2000 bytes of their run left,
    once in front of C and once in front of B) and the hop splits them in the next round; the plain key needs the
    doubling to reach the runs' length."""
    from spring_amd.bwt import BwtStage
    from spring_amd.reorder import ReorderError
    res, info = _run([HARD])
    _same(res, [HARD], "run keys off")
    assert info["rounds"] >= 9 and info["run_positions"] == 0
    assert rm.ranks(HARD, 7, 0, runs=False)[1] == info["rounds"]
    res_on, info_on = _run([HARD], run_keys=0)
    _same(res_on, [HARD], "run keys on")
    assert info_on["rounds"] <= 3 and info_on["run_positions"] > 0
    in_runs = rm.first_keys(np.frombuffer(HARD, np.uint8), 4, 20)[2]
    assert in_runs == 2997 + 1997   # all of both runs but their last three positions
    assert info_on["rounds"] == rm.ranks(HARD, 4, 20)[1] == 2 and info_on["run_positions"] == in_runs
    with BwtStage() as st:   # the entries each round sorted
        st.transform(HARD)
        assert list(st.round_entries()) == rm.ranks(HARD, 7, 0, runs=False)[2]
        st.set_run_keys(True)
        st.transform(HARD)
        assert list(st.round_entries()) == rm.ranks(HARD, 4, 20)[2] == [5002, 2 * 1997]
        with pytest.raises(ReorderError, match="code -1"):
            st.transform(HARD, [0, 1])
        with pytest.raises(ReorderError, match="code -4"):
            st.round_entries()
    _, info_cap = _run([HARD], run_keys=3)   # runs above the cap tie and take the doubling rounds
    assert info_on["rounds"] < info_cap["rounds"] == rm.ranks(HARD, 4, 20, 3)[1]
    with BwtStage() as st:   # encode_inplace takes the option as well
        st.set_run_keys(True)
        T = np.frombuffer(HARD, np.uint8).copy()
        p, idx = st.encode_inplace(T)
        assert (T.tobytes(), p) == _want(HARD)[:2] and np.array_equal(idx, _want(HARD)[2])
        assert st.info["rounds"] == 2 and st.info["run_positions"] == in_runs
        st.set_run_keys(False)
        st.transform(HARD)
        assert st.info["rounds"] == info["rounds"] and st.info["run_positions"] == 0


# The run-key layout (bwt_plan.h::run_key_layout): a 20-bit run field and four text bytes up to 256 segments in a
# sub-batch; a 16-bit field above, with four text bytes up to 4096 segments, three up to 2^20, two up to 2^24.
CLASSES = ((256, 4, 20), (257, 4, 16), (4096, 4, 16), (4097, 3, 16))


def _layout(sub_segments):
    """bwt_plan.h::run_key_layout restated -> (text bytes, bits of the run field, bits of the key)."""
    seg_bits = (max(sub_segments, 1) - 1).bit_length()
    run_bits = 20 if seg_bits <= 8 else 16
    k = min(4, (60 - run_bits - seg_bits) // 8)
    return k, run_bits, seg_bits + 8 * k + 4 + run_bits


@pytest.mark.parametrize("S,k,R", CLASSES)
def test_segment_count_classes_with_run_keys(S, k, R):
    assert _layout(S)[:2] == (k, R) == rm.run_key_layout(S)[1:3]
    assert [_layout(x)[:2] for x in (1, 1 << 20, (1 << 20) + 1, 1 << 24)] == [(4, 20), (3, 16), (2, 16), (2, 16)]
    assert all(_layout(x)[2] <= 64 for x in (1, 256, 257, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 24))
    segs = bm.pool_batch(S)
    assert len(segs) == S and b"" in segs and any(a == b != b"" for a, b in zip(segs, segs[1:]))
    res, info = _run(segs, run_keys=0)
    assert info["sub_batches"] == 1   # all S segments share one first key
    _same(res, segs, "%d segments" % S)
    want = sum(c * rm.first_keys(np.frombuffer(s, np.uint8), k, R)[2] for s, c in collections.Counter(segs).items() if s)
    assert info["run_positions"] == want > 0


def test_the_two_byte_class_with_run_keys():
    """2^20 + 1 short segments in one sub-batch: two text bytes in the first key.  The index table of that many segments
    is a gibibyte, so bytes and primary indexes are fetched without it."""
    from spring_amd import _lib
    from spring_amd.bwt import BwtStage
    S = (1 << 20) + 1
    assert _layout(S)[:2] == (2, 16)
    pool = [b"", b"G", b"GG", b"GGG", b"GGGA", b"GGGT", b"AGGGGGGT", b"TGGGGGGA", b"GGGGGGGGGGGG", b"ACGT", b"\x00\x00\xff\xff\x00",
            b"##########II", b"I##########", b"CACAC", b"\xff\xff\xff", b"FF:FF,,,F"]
    idx = np.random.default_rng(3).integers(0, len(pool), S)
    idx[1:S:5] = idx[0:S - 1:5]   # equal neighbours
    segs = [pool[i] for i in idx]
    data, off = _batch(segs)
    with BwtStage() as st:
        st.set_run_keys(True)
        info = st.transform(data, off)
        assert info["sub_batches"] == 1 and info["num_segments"] == S and info["run_positions"] > 0
        buf, primary = np.zeros(len(data), np.uint8), np.zeros(S, np.int32)
        rc = _lib.lib().spring_bwt_download(st._h, buf.ctypes.data, None, primary.ctypes.data, None, None)
        assert rc == 0
    assert buf.tobytes() == b"".join([_want(p)[0] for p in pool][i] for i in idx)
    assert np.array_equal(primary, np.array([_want(p)[1] for p in pool], np.int32)[idx])


def test_sub_batches_with_run_keys_give_the_same_result():
    from spring_amd.bwt import BwtStage
    from spring_amd.reorder import ReorderError
    segs = _lengths_batch()
    budget = 76 * 4097 + 16   # the planner charges 76 bytes a position with run keys on
    first = rm.plan([len(s) for s in segs], budget)
    assert len(first) - 1 == 3
    one, info1 = _run(segs, run_keys=0)
    many, info = _run(segs, run_keys=0, workspace=budget)
    assert info1["sub_batches"] == 1 and info["sub_batches"] == 3
    _same(many, segs, "sub-batches")
    _equal(many, one, "three sub-batches against one")
    _equal(many, _plain("lengths")[0], "against run keys off")
    assert info["run_positions"] == info1["run_positions"] > 0
    data, off = _batch(segs)
    with BwtStage() as st:
        st.set_run_keys(True)
        st.set_workspace_bytes(budget - 1)   # 72 bytes a position would fit
        with pytest.raises(ReorderError, match="code -1"):
            st.transform(data, off)
        with pytest.raises(ReorderError, match="code -4"):
            st.download()
        st.set_run_keys(False)
        st.transform(data, off)
        _same(st.download(), segs, "the same budget with run keys off")


def test_two_runs_give_identical_bytes():
    segs = _run_cases()
    a, ia = _run(segs, run_keys=0)
    b, ib = _run(segs, run_keys=0)
    _equal(a, b, "two runs")
    assert ia["rounds"] == ib["rounds"] and ia["run_positions"] == ib["run_positions"]


def test_refusals():
    from spring_amd import BwtStage, QualIdStage
    from spring_amd import _lib
    from spring_amd.reorder import ReorderError
    f1 = _fastq(1)
    n = f1.count(b"\n") // 4

    def refused(st, code, call):
        with pytest.raises(ReorderError, match="code %d" % code):
            call()
        with pytest.raises(ReorderError, match="code -4"):   # a refused call leaves no result
            st.download()
        assert st.info is None

    with QualIdStage() as qs, BwtStage() as st:
        refused(st, -4, lambda: st.transform(qs))   # no result yet
        qs.set_order(None, n)
        qs.from_fastq(f1, want="quality", num_reads_per_block=7)
        st.transform(qs, block_bytes=256)
        refused(st, -1, lambda: st.transform(qs, kind=2))
        st.transform(qs, block_bytes=1 << 30)
        refused(st, -1, lambda: st.transform(qs, block_bytes=(1 << 30) + 1))
        st.transform(qs, block_bytes=256)
        refused(st, -4, lambda: st.transform(qs, kind="id"))   # only the quality blocks were built
        try:   # a block-sort context on a second device, where the machine has one
            other = BwtStage(1)
        except ReorderError:
            other = None
        if other is not None:
            with other:
                refused(other, -1, lambda: other.transform(qs))
        # cap_bits: 1, and above any layout's run field
        st.transform(qs, block_bytes=256)
        for bad in (1, 21, 64):
            with pytest.raises(ReorderError, match="code -1"):
                st.set_run_keys(True, bad)
        info = st.transform(qs, block_bytes=256)   # a refused setting changes nothing
        assert info["run_positions"] == 0
        # ... and above the run field of this batch's layout: more than 256 segments have 16 bits
        segs = [b"GGGGGGAT"] * 300
        st.set_run_keys(True, 17)
        refused(st, -1, lambda: st.transform(*_batch(segs)))
        st.set_run_keys(True, 16)
        st.transform(*_batch(segs))
        _same(st.download(), segs, "after refusals")
        st.set_run_keys(True, 20)
        st.transform(*_batch(segs[:256]))
        _same(st.download(), segs[:256], "20 bits at 256 segments")
        assert _lib.lib().spring_bwt_set_run_keys(None, 1, 0) == -1
