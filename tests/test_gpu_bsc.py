"""GPU tests of the BSC framing stage (include/spring_bsc.h).  Every block and file is compared byte for byte with the
plain-Python model (tests/bsc_frame_model.py) fed with what the block-sort and QLFC contexts themselves hold, and, where
oracle/_ref is built, with the real bsc_compress / bsc_store, the ref_bsc program (BSC_compress) and the quality files
the real reorder_compress_quality_id writes (BSC_str_array_compress); the real bsc_decompress and
BSC_str_array_decompress read the device's bytes back.  Byte equality: no tolerance anywhere."""
import functools
import os
import struct
import tempfile
import zlib

import numpy as np
import pytest

import bsc_frame_model as fm
import qlfc_model as qm
import qualid_model as qd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = fm.ref_lib()
TABLES = qm.state_tables()
REAL = REF is not None and TABLES is not None
needs_ref = pytest.mark.skipif(not REAL, reason="oracle/_ref/libref_units.so not built (needs the reference sources)")

NAMES = tuple(qm.SMALL) + ("a300000", "bwt300000", "random4096")
TEXTS = (1, 28, 29, 65535, 65536)
RUNS = (fm.NO_GAIN_RUN, fm.NO_GAIN_EQ_RUN, fm.GAIN_RUN)


@functools.lru_cache(maxsize=None)
def _segments():
    return tuple([qm.case(n) for n in NAMES] + [fm.text(n) for n in TEXTS] + [fm.no_gain_case(r) for r in RUNS])


def _labels():
    return list(NAMES) + ["text%d" % n for n in TEXTS] + ["no_gain_run%d" % r for r in RUNS]


def _batch(segs):
    return b"".join(segs), np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)


class Stages:
    """A BwtStage, a QlfcStage with its tables (the real ones where they can be read) and a BscStage."""

    def __init__(self, tables=None):
        from spring_amd import BscStage, BwtStage, QlfcStage
        self.bwt, self.qlfc, self.bsc = BwtStage(), QlfcStage(), BscStage()
        self.qlfc.set_state_tables(*(tables or TABLES or qm.random_tables(101)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for st in (self.bsc, self.qlfc, self.bwt):
            st.close()

    def frame(self, src, *a, **k):
        return self.bsc.frame(self.bwt, self.qlfc, src, *a, **k)

    def parts(self):
        """Per segment what the two inner contexts hold: (primary, indexes, coded bytes, the coder's return value)."""
        res, coded = self.bwt.download(), self.qlfc.segments()
        return [(int(res["primary"][j]), res["indexes"][j][:int(res["num_indexes"][j])], coded[j][0], coded[j][1])
                for j in range(len(coded))]


def _model_blocks(segs, parts):
    return [fm.block(seg, *p) for seg, p in zip(segs, parts)]


def _check_info(info, res, files, segs):
    assert info["num_files"] == len(files) and info["num_blocks"] == len(segs)
    assert info["bytes_in"] == sum(len(s) for s in segs) and info["bytes_out"] == len(res["bytes"])
    kinds = list(res["block_kind"])
    assert [info["coded"], info["stored_small"], info["stored_coder"], info["stored_no_gain"]] == [kinds.count(k) for k in range(4)]
    assert len(info["ms_pass"]) == 3 and info["ms_device"] >= 0


# ---------------------------------------------------------------------------------------------- sums
def test_sums_equal_zlib():
    from spring_amd import BscStage
    data, off = fm.sum_batch()
    with BscStage() as st:
        got = st.adler32(data, off)
        one = st.adler32(data[:5553])
        none = st.adler32(b"")
    want = [zlib.adler32(data[int(a):int(b)]) & 0xffffffff for a, b in zip(off[:-1], off[1:])]
    for j, (g, w) in enumerate(zip(got, want)):
        print(j, int(off[j]) % 16, int(off[j + 1] - off[j]), hex(int(g)), hex(w))
    assert [int(g) for g in got] == want
    assert int(one[0]) == zlib.adler32(data[:5553]) & 0xffffffff and int(none[0]) == 1
    assert want[0] == 1 and int(off[-1] - off[-2]) == (64 << 20) + 1


# ---------------------------------------------------------------------------------------------- blocks
@functools.lru_cache(maxsize=None)
def _blocks_run():
    segs = _segments()
    with Stages() as S:
        info = S.frame(*_batch(segs))
        res, files, parts = S.bsc.download(), S.bsc.files(), S.parts()
        inner = (S.bwt.download(), S.qlfc.download(), dict(S.bwt.info), dict(S.qlfc.info))
        again = S.frame(*_batch(segs)) and S.bsc.download()
        # the inner contexts still hold, and hand out, what they held
        after = (S.bwt.download(), S.qlfc.download())
        alone = [S.bsc.compress(S.bwt, S.qlfc, segs[j]) for j in (_labels().index(n) for n in ("len1", "a40", "random4096"))]
    return dict(info=info, res=res, files=files, parts=parts, inner=inner, again=again, after=after, alone=alone)


def test_blocks_equal_the_model_fed_with_the_contexts_own_results():
    segs, run = _segments(), _blocks_run()
    res, files = run["res"], run["files"]
    want = _model_blocks(segs, run["parts"])
    _check_info(run["info"], res, files, segs)
    assert [(s, b, f) for s, b, f, _ in files] == [(-1, j, j) for j in range(len(segs))]
    at = 0
    for j, (name, (blk, kind)) in enumerate(zip(_labels(), want)):
        print(name, len(segs[j]), "->", len(files[j][3]), "kind", int(res["block_kind"][j]), "expected", len(blk), kind)
        assert int(res["block_kind"][j]) == kind, name
        assert files[j][3] == blk, name
        assert int(res["block_off"][j]) == at == int(res["file_off"][j]), name
        at += len(blk)
    assert int(res["file_off"][-1]) == at == len(res["bytes"])
    kinds = {n: int(k) for n, k in zip(_labels(), res["block_kind"])}
    assert kinds["len1"] == kinds["text1"] == kinds["text28"] == fm.STORED_SMALL and kinds["text29"] != fm.STORED_SMALL
    assert kinds["random4096"] == fm.STORED_CODER and kinds["a300000"] == kinds["text65535"] == kinds["text65536"] == fm.CODED
    # below 64 KiB the indexes are dropped, from 64 KiB on they are kept
    small, big = files[_labels().index("text65535")][3], files[_labels().index("text65536")][3]
    assert small[-1] == 0 and big[-1] == 7
    assert big[-29:-1] == struct.pack("<7i", *[int(x) for x in run["parts"][_labels().index("text65536")][1]])
    if REAL:   # the stored-no-gain inputs were found with the real tables
        assert set(kinds.values()) == {0, 1, 2, 3}
        assert [kinds["no_gain_run%d" % r] for r in RUNS] == [fm.STORED_NO_GAIN, fm.STORED_NO_GAIN, fm.CODED]
    else:
        assert {0, 1, 2} <= set(kinds.values())


def test_a_repeated_call_and_the_inner_contexts():
    run = _blocks_run()
    assert run["again"]["bytes"] == run["res"]["bytes"]
    for k in ("file_off", "block_off", "block_kind"):
        assert np.array_equal(run["again"][k], run["res"][k]), k
    (bw, ql, bwi, qli), (bw2, ql2) = run["inner"], run["after"]
    assert bw["bwt"] == bw2["bwt"] and ql["coded"] == ql2["coded"]
    for k in ("seg_off", "primary", "num_indexes", "indexes"):
        assert np.array_equal(bw[k], bw2[k]), k
    assert np.array_equal(ql["coded_off"], ql2["coded_off"]) and np.array_equal(ql["status"], ql2["status"])
    assert bwi["num_segments"] == qli["num_segments"] == len(_segments())
    # the one-buffer entry point gives the same blocks
    for name, blk in zip(("len1", "a40", "random4096"), run["alone"]):
        assert blk == run["files"][_labels().index(name)][3], name


@needs_ref
def test_blocks_equal_the_real_bsc_compress_and_decompress_with_it():
    segs, run = _segments(), _blocks_run()
    for name, seg, f in zip(_labels(), segs, run["files"]):
        assert f[3] == fm.ref_block(seg), name
        back, rc = fm.ref_decompress(f[3], len(seg))
        assert rc == 0 and back == seg, name
    for run_len, blk in zip(RUNS, run["files"][-3:]):   # and the real functions take the branch the case is for
        rc = fm.ref_inplace_rc(fm.no_gain_case(run_len))
        assert (rc == fm.NOT_COMPRESSIBLE) == (run_len != fm.GAIN_RUN) and (rc == len(blk[3])) == (run_len == fm.GAIN_RUN)


@needs_ref
def test_compress_on_host_buffers_equals_the_real_call():
    with Stages() as S:
        for data in (fm.text(5000, seed=9), qm.case("random4096"), fm.text(20), b""):
            assert S.bsc.compress(S.bwt, S.qlfc, data) == fm.ref_block(data), len(data)
            assert S.bsc.info["num_blocks"] == 1 and S.bsc.info["bytes_in"] == len(data)


def test_sub_batches_in_the_sort_and_the_coder_give_the_same_bytes():
    from spring_amd import bwt as bwt_mod, qlfc as qlfc_mod
    pick = [j for j, n in enumerate(_labels()) if n in ("a40", "letters9", "text29", "text65535", "text65536", "random4096")]
    segs = [_segments()[j] for j in pick]
    want = b"".join(_blocks_run()["files"][j][3] for j in pick)
    with Stages() as S:
        info = S.frame(*_batch(segs))
        assert S.bsc.download()["bytes"] == want and S.bwt.info["sub_batches"] == 1 and S.qlfc.info["sub_batches"] == 1
        events = S.qlfc.info["events"]
        S.bwt.set_workspace_bytes(bwt_mod.workspace_need(65536, 1) + 4096)
        S.qlfc.set_workspace_bytes(qlfc_mod.workspace_need(sum(len(s) for s in segs), len(segs)) + events * 160 // 2)
        info2 = S.frame(*_batch(segs))
        assert S.bwt.info["sub_batches"] >= 2 and S.qlfc.info["sub_batches"] >= 2
        assert S.bsc.download()["bytes"] == want
        assert {k: v for k, v in info2.items() if not k.startswith("ms_")} == {k: v for k, v in info.items() if not k.startswith("ms_")}


def test_host_segments_grouped_into_files_of_both_framings():
    """file_first on a host batch: files without cuts at both ends and in the middle, the cut offsets the sums of the
    segments before them."""
    segs = [fm.text(n, seed=n) for n in (300, 29, 5000, 1, 700, 64)]
    first = [0, 0, 2, 2, 2, 3, 6, 6]
    with Stages() as S:
        for framing in ("blocks", "file", "str_array"):
            info = S.frame(*_batch(segs), framing=framing, file_first=first)
            blocks = [b for b, _ in _model_blocks(segs, S.parts())]
            res, files = S.bsc.download(), S.bsc.files()
            _check_info(info, res, files, segs)
            assert [(s, b, f) for s, b, f, _ in files] == [(-1, j, first[j]) for j in range(7)]
            for f in range(7):
                lo = [sum(len(s) for s in segs[first[f]:j]) for j in range(first[f], first[f + 1])]
                want = fm.frame(("blocks", "file", "str_array").index(framing), list(zip(lo, blocks[first[f]:first[f + 1]])))
                assert files[f][3] == want, (framing, f)
            for j, blk in enumerate(blocks):
                at = int(res["block_off"][j])
                assert res["bytes"][at:at + len(blk)] == blk, (framing, j)
            assert len(files[0][3]) == (0 if framing == "blocks" else 4)


# ---------------------------------------------------------------------------------------------- BSC files
def _streams_run(ss, name, pe, preserve_order, B):
    z = np.load(os.path.join(GOLDEN, "enc_%s.npz" % name))
    N = len(z["rlen"])
    return ss.from_host(z["pos"], z["rc"], z["noise"], z["noisepos"], z["order"], z["rlen"], z["unaligned"], N, pe,
                        preserve_order, B)


@pytest.mark.parametrize("block_bytes", [None, 500])
def test_bsc_files_from_the_streams_of_a_fixture(block_bytes):
    """var2k single-end, three blocks: one file per (stream, block) slice, the empty slices of the paired-end streams
    included.  With the default cut a slice is one block: the file is what the ref_bsc program writes.  With a cut of
    500 bytes some slices have three cuts and more: the file is BSC_compress's framing of the real bsc_compress of
    every cut, offsets included."""
    from spring_amd import StreamsStage, _lib
    with StreamsStage() as ss, Stages() as S:
        si = _streams_run(ss, "var2k", False, False, 800)
        nb = si["num_blocks"]
        assert nb == 3
        if block_bytes:
            S.bwt.set_block_bytes(block_bytes)
        info = S.frame(ss)
        res, files, parts = S.bsc.download(), S.bsc.files(), S.parts()
        stream, block, cut = S.bwt.segments()
        slices = {s: ss.blocks(s) for s in range(_lib.STREAMS_NUM)}
        assert ss.blocks(0) == slices[0]                       # the streams context is left as it was
    assert [(s, b) for s, b, _, _ in files] == [(s, b) for s in range(_lib.STREAMS_NUM) for b in range(nb)]
    first = [f for _, _, f, _ in files] + [len(parts)]
    most, segs = 0, []
    for f, (s, b, j0, got) in enumerate(files):
        data = slices[s][b]
        cuts = fm.cuts(len(data), block_bytes or 25 << 20)
        assert first[f + 1] - j0 == len(cuts), (s, b)
        assert [(int(stream[j]), int(block[j]), int(cut[j])) for j in range(j0, first[f + 1])] == [(s, b, c) for c in range(len(cuts))]
        model = fm.bsc_file([(lo, fm.block(data[lo:hi], *parts[j0 + c])[0]) for c, (lo, hi) in enumerate(cuts)])
        assert got == model, (s, b, "model")
        if not data:
            assert got == b"\0\0\0\0", (s, b)
        if REAL:
            assert got == fm.bsc_file([(lo, fm.ref_block(data[lo:hi])) for lo, hi in cuts]), (s, b, "real bsc_compress")
            if not block_bytes and fm.ref_bsc_bin():
                assert got == fm.ref_bsc_file(data), (s, b, "ref_bsc")
        most = max(most, len(cuts))
        segs += [data[lo:hi] for lo, hi in cuts]
    assert any(not slices[s][b] for s, b, _, _ in files)       # a single-end run: the pair streams are empty
    assert most >= 3 if block_bytes else most == 1
    _check_info(info, res, files, segs)
    assert b"".join(f[3] for f in files) == res["bytes"]


def test_a_stream_mask_takes_its_streams_only():
    from spring_amd import StreamsStage
    with StreamsStage() as ss, Stages() as S:
        _streams_run(ss, "var2k", False, False, 800)
        S.frame(ss)
        every = S.bsc.files()
        full = [s for s in range(9) if all(len(f[3]) > 4 for f in every if f[0] == s)][0]
        void = [s for s in range(9) if all(f[3] == b"\0\0\0\0" for f in every if f[0] == s)][-1]   # a paired-end stream
        assert full < void
        S.frame(ss, streams=[void, full])
        got = S.bsc.files()
    assert [(s, b) for s, b, _, _ in got] == [(full, 0), (full, 1), (full, 2), (void, 0), (void, 1), (void, 2)]
    assert [f[3] for f in got] == [f[3] for f in every if f[0] in (full, void)]
    assert [f[3] for f in got[3:]] == [b"\0\0\0\0"] * 3 and got[3][2] == got[4][2] == got[5][2]


# ---------------------------------------------------------------------------------------------- string-array files
def _fastq():
    return open(os.path.join(GOLDEN, "test_1.fastq"), "rb").read()


def _real_quality_files(image, order, n, B):
    """The quality_1.<b> files the real reorder_compress_quality_id leaves for the line image of quality_1."""
    from oracle import pyoracle as po
    Q = po.ref_qualid_lib()
    nb = (n + B - 1) // B
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "quality_1"), "wb") as f:
            f.write(image)
        with open(os.path.join(d, "read_order.bin"), "wb") as f:
            f.write(np.asarray(order, np.uint32).tobytes())
        assert Q.ref_q_write(d.encode(), n, 0, B, 1, 1, 0, 0) == 0
        return [open(os.path.join(d, "quality_1.%d" % b), "rb").read() for b in range(nb)]


@pytest.mark.parametrize("block_bytes", [0, 333])
def test_string_array_files_from_a_quality_context(block_bytes):
    """test_1.fastq under a fixed permutation, 40 reads a block: three blocks.  With the 64 MiB SPRING passes a block
    is one cut and the file is the one the real writer leaves; with 333 bytes the cuts fall inside the lines.  The real
    BSC_str_array_decompress reads every file of the device back into the block's lines."""
    from spring_amd import QualIdStage, _lib
    f = _fastq()
    n, B = f.count(b"\n") // 4, 40
    order = np.random.default_rng(5).permutation(n).astype(np.uint32)
    with QualIdStage() as qs, Stages() as S:
        qs.set_order(order, n)
        qi = qs.from_fastq(f, num_reads_per_block=B)
        assert qi["num_blocks"] == 3
        info = S.frame(qs, kind="quality", block_bytes=block_bytes)
        res, files, parts = S.bsc.download(), S.bsc.files(), S.parts()
        data, lens, off = qs.download("quality")
        id_info = S.frame(qs, kind="id", block_bytes=block_bytes)
        id_files, id_parts = S.bsc.files(), S.parts()
        ids, _, id_off = qs.download("id")
    cut = block_bytes or 64 << 20
    first = [x for _, _, x, _ in files] + [len(parts)]
    segs = []
    for b, (s, blk, j0, got) in enumerate(files):
        assert (s, blk) == (_lib.BWT_SRC_QUALITY, b)
        text = data[int(off[b]):int(off[b + 1])]
        cuts = fm.cuts(len(text), cut)
        assert first[b + 1] - j0 == len(cuts) and (len(cuts) >= 3 if block_bytes else len(cuts) == 1)
        segs += [text[lo:hi] for lo, hi in cuts]
        assert got == fm.str_array_file([fm.block(text[lo:hi], *parts[j0 + c])[0] for c, (lo, hi) in enumerate(cuts)]), b
        if REAL:
            from oracle import pyoracle as po
            assert got == fm.str_array_file([fm.ref_block(text[lo:hi]) for lo, hi in cuts]), (b, "real bsc_compress")
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "quality_1.%d" % b)
                with open(path, "wb") as out:
                    out.write(got)
                assert po.ref_read_quality(path, lens[b * B:(b + 1) * B]) == text, (b, "BSC_str_array_decompress")
    if block_bytes:
        line_ends = set(np.cumsum(lens[:B]).tolist())
        assert any(x not in line_ends for x in range(cut, int(off[1]), cut))      # a cut inside a line
    _check_info(info, res, files, segs)
    if REAL and not block_bytes:
        _, _, quals = qd.fastq_lines(f)
        real = _real_quality_files(b"".join(q + b"\n" for q in quals), order, n, B)
        assert [x[3] for x in files] == real
    # the id blocks are framed the same way
    assert id_info["num_files"] == 3 and [(s, b) for s, b, _, _ in id_files] == [(_lib.BWT_SRC_ID, b) for b in range(3)]
    first = [x for _, _, x, _ in id_files] + [len(id_parts)]
    for b, (_, _, j0, got) in enumerate(id_files):
        text = ids[int(id_off[b]):int(id_off[b + 1])]
        assert got == fm.str_array_file([fm.block(text[lo:hi], *id_parts[j0 + c])[0] for c, (lo, hi) in enumerate(fm.cuts(len(text), cut))]), b


def test_an_empty_quality_block_is_a_file_without_cuts():
    from spring_amd import QualIdStage
    f = b"@a\n\n+\n\n@b\n\n+\n\n@c\nACGT\n+\nIIII\n"
    with QualIdStage() as qs, Stages() as S:
        qs.set_order(None, 3)
        qs.from_fastq(f, num_reads_per_block=2)
        info = S.frame(qs, kind="quality")
        files = S.bsc.files()
    assert info["num_files"] == 2 and info["num_blocks"] == 1
    assert files[0][3] == b"\0\0\0\0" and files[1][3] == fm.str_array_file([fm.store(b"IIII")])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from spring_amd import BscStage, BwtStage, QlfcStage, QualIdStage, StreamsStage
    from spring_amd._stage import ReorderError
    data = qm.case("ab32") + qm.case("a40")
    with BscStage() as bs, BwtStage() as bw, QlfcStage() as ql:
        with pytest.raises(ReorderError, match="code -4"):      # nothing framed yet
            bs.download()
        with pytest.raises(ReorderError, match="code -4"):
            bs.get_info()
        with pytest.raises(ReorderError, match="code -4"):      # a QLFC context without state tables
            bs.frame(bw, ql, data)
        with pytest.raises(ReorderError, match="code -4"):
            bs.compress(bw, ql, data)
        ql.set_state_tables(*qm.random_tables(101))
        good = bs.frame(bw, ql, data, [0, 64, 104])
        assert good["num_blocks"] == 2
        for off in ([0, 60, 40, 104], [0, 50, 90], [0, 50, 105], [1, 50, 104]):
            with pytest.raises(ReorderError, match="code -1"):
                bs.frame(bw, ql, data, off)
            with pytest.raises(ReorderError, match="code -4"):  # a refused call leaves no result
                bs.download()
        for first in ([0, 1], [1, 2], [0, 2, 1, 2], [0, 3]):
            with pytest.raises(ReorderError, match="code -1"):
                bs.frame(bw, ql, data, [0, 64, 104], framing="file", file_first=first)
            with pytest.raises(ReorderError, match="code -4"):
                bs.files()
        with pytest.raises(ReorderError, match="code -1"):
            bs.frame(bw, ql, data, framing=3)
        big = np.zeros((1 << 30) + 1, np.uint8)                 # the block sort's refusal is passed on
        with pytest.raises(ReorderError, match="code -1"):
            bs.frame(bw, ql, big)
        del big
        with pytest.raises(ReorderError, match="code -4"):
            bs.download()
        with StreamsStage() as ss, QualIdStage() as qs:         # no run, no result: the inner stage says so
            with pytest.raises(ReorderError, match="code -4"):
                bs.frame(bw, ql, ss)
            with pytest.raises(ReorderError, match="code -4"):
                bs.frame(bw, ql, qs)
        with pytest.raises(ValueError):
            bs.frame(bw, None, data)
        try:
            other = BwtStage(device=1)
        except ReorderError:
            other = None                                        # one device: nothing to tell apart
        if other is not None:
            with other:
                with pytest.raises(ReorderError, match="code -1"):
                    bs.frame(other, ql, data)
        info = bs.frame(bw, ql, data, [0, 64, 64, 104])         # and the context works on: an empty segment is a stored block
        assert info["num_blocks"] == 3 and bs.files()[1][3] == fm.store(b"")
        assert int(bs.adler32(data)[0]) == zlib.adler32(data) & 0xffffffff
        assert bs.download()["bytes"] == b"".join(f[3] for f in bs.files())   # the sums leave the result alone
