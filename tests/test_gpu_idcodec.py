"""The id codec stage on the GPU (spring_amd.IdCodecStage; include/spring_idcodec.h): its bytes against the recorded
files of the reference's compress_id_block (tests/golden/ref_idcodec_*.npz) and against the plain-Python model, its
symbol words against the model's, so that a tokenizer fault and a coder fault show apart."""
import os

import numpy as np
import pytest

import idcodec_cases as ic
import idcodec_model as m

pytestmark = pytest.mark.gpu

GOLDEN = ic.GOLDEN


@pytest.fixture(scope="module")
def expected():
    """name -> (ids, B, recorded blocks, model symbols per block, largest token count), computed once."""
    out = {}
    for name in ic.ALL:
        ids, B, blocks = ic.load(name)
        sym, mt = [], 0
        for i in range(0, len(ids), B):
            w, t = m.block_symbols(ids[i:i + B])
            sym.append(np.asarray(w, np.uint32))
            mt = max(mt, t)
        out[name] = (ids, B, blocks, sym, mt)
    return out


def _check(st, ids, B, blocks, sym, mt, what):
    info = st.info
    assert info["num_lines"] == len(ids) and info["num_blocks"] == len(blocks), what
    words, off = st.symbols()
    assert [int(x) for x in off] == [0] + list(np.cumsum([len(s) for s in sym])), what
    for b, s in enumerate(sym):
        assert np.array_equal(words[int(off[b]):int(off[b + 1])], s), (what, "symbols of block", b)
    assert info["num_symbols"] == len(words) and info["max_tokens"] == mt, what
    got = st.blocks()
    for b, want in enumerate(blocks):
        assert got[b] == want, (what, "bytes of block", b)
    assert info["bytes"] == sum(len(x) for x in blocks), what
    assert st.get_info() == info, what


@pytest.mark.parametrize("name", ic.ALL)
def test_bytes_and_symbols_equal_reference_and_model(name, expected):
    from spring_amd import IdCodecStage
    ids, B, blocks, sym, mt = expected[name]
    assert [m.encode_symbols(s.tolist()) for s in sym] == blocks   # golden == model, here as well
    with IdCodecStage() as st:
        info = st.from_lines(ids, B)
        assert info["sub_batches"] == 1
        _check(st, ids, B, blocks, sym, mt, name)
        first = st.blocks()
        st.from_lines(ic.lines_image(ids), B)   # the image form, and a second run: the same bytes
        assert st.blocks() == first


def test_sub_batches_of_whole_blocks(expected):
    from spring_amd import IdCodecStage, ReorderError
    from spring_amd import idcodec
    ids, B, blocks, sym, mt = expected["illumina"]
    with IdCodecStage() as st:
        st.set_workspace_bytes(idcodec.workspace_need(2, mt))   # models for two of the three blocks
        info = st.from_lines(ids, B)
        assert info["sub_batches"] == 2
        _check(st, ids, B, blocks, sym, mt, "two sub-batches")
        st.set_workspace_bytes(idcodec.workspace_need(1, mt))
        assert st.from_lines(ids, B)["sub_batches"] == 3
        _check(st, ids, B, blocks, sym, mt, "three sub-batches")
        st.set_workspace_bytes(idcodec.workspace_need(1, mt) - 1)   # not even one block's models
        with pytest.raises(ReorderError, match=r"code -1\)"):
            st.from_lines(ids, B)
        with pytest.raises(ReorderError, match=r"code -4\)"):
            st.blocks()


def test_zero_lines_and_one_line():
    from spring_amd import IdCodecStage
    with IdCodecStage() as st:
        info = st.from_lines([], 5)
        assert info["num_blocks"] == 0 and info["bytes"] == 0 and info["num_symbols"] == 0
        assert st.blocks() == [] and len(st.symbols()[0]) == 0
        st.from_lines([b""], 5)
        assert st.blocks() == [m.compress_block([b""])]
        assert st.symbols()[0].tolist() == [m.word(m.K_TYPE, 0, m.END)]


def _fastq(j):
    with open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb") as f:
        return f.read()


@pytest.mark.parametrize("order", [False, True])
def test_from_a_qualid_context(order):
    """The ids of the FASTQ fixtures as the quality / id stage leaves them in HBM, with and without an order: the same
    as from_lines on the downloaded blocks, equal to the model, and the context is left as it was."""
    from spring_amd import IdCodecStage, QualIdStage
    B = 7
    with QualIdStage() as qs, IdCodecStage() as st, IdCodecStage() as host:
        for j in (1, 2):
            f = _fastq(j)
            n = f.count(b"\n") // 4
            qs.set_order(np.random.default_rng(5 + j).permutation(n).astype(np.uint32) if order else None, n)
            qs.from_fastq(f, want=("quality", "id"), num_reads_per_block=B)
            before = qs.download("id")
            info = st.from_qualid(qs)
            assert info["num_lines"] == n and info["num_blocks"] == (n + B - 1) // B
            ids = [x for blk in qs.blocks("id") for x in blk]
            host.from_lines(ids, B)
            assert st.blocks() == host.blocks() and np.array_equal(st.symbols()[0], host.symbols()[0])
            assert st.blocks() == m.compress_blocks(ids, B)
            after = qs.download("id")
            assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


REFUSED = {
    "an id of 1 024 bytes": b"@" + b"a1" * 511 + b"b",
    "a 256-letter run": b"@" + b"a" * 256,
    "a 256-zero run": b"@" + b"0" * 256,
    "a byte 0x80": b"@a\x80",
    "a byte 0": b"@ab\x00",
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals(what):
    from spring_amd import IdCodecStage, ReorderError
    bad = REFUSED[what]
    assert what != "an id of 1 024 bytes" or len(bad) == 1024
    with IdCodecStage() as st:
        for ids in ([bad], [b"@ok", b"@ok 2", bad, b"@ok 3"]):
            st.from_lines([b"@fine"], 4)   # a result the refused call must drop
            with pytest.raises(ReorderError, match=r"code -1\)"):
                st.from_lines(ids, 4)
            with pytest.raises(ReorderError, match=r"code -4\)"):
                st.download()
            with pytest.raises(ReorderError, match=r"code -4\)"):
                st.symbols()
            with pytest.raises(ReorderError, match=r"code -4\)"):
                st.get_info()
        st.from_lines([bad[:-1]], 4)   # one byte less is taken
        assert st.blocks() == [m.compress_block([bad[:-1]])]


def test_refused_calls():
    from spring_amd import IdCodecStage, QualIdStage, ReorderError
    with IdCodecStage() as st, QualIdStage() as qs:
        with pytest.raises(ReorderError, match=r"code -4\)"):
            st.download()   # nothing compressed yet
        with pytest.raises(ReorderError, match=r"code -1\)"):
            st.from_lines([b"@a"], 0)   # B = 0
        with pytest.raises(ReorderError, match=r"code -1\)"):
            st.from_lines(b"@a\n@b", 4)   # the last id has no newline
        with pytest.raises(ReorderError, match=r"code -4\)"):
            st.from_qualid(qs)   # a qualid context without any result
        f = _fastq(1)
        qs.set_order(None, f.count(b"\n") // 4)
        qs.from_fastq(f, want="quality", num_reads_per_block=7)
        with pytest.raises(ReorderError, match=r"code -4\)"):
            st.from_qualid(qs)   # ... and one with a quality result alone
        with pytest.raises(ReorderError, match=r"code -4\)"):
            st.download()
        # the device's own length check: lines in HBM that no host has seen
        fq = b"".join(i + b"\nACGT\n+\nIIII\n" for i in (b"@ok", REFUSED["an id of 1 024 bytes"], b"@ok 2"))
        qs.set_order(None, 3)
        qs.from_fastq(fq, want="id", num_reads_per_block=2)
        with pytest.raises(ReorderError, match=r"id 1 is longer.*code -1\)"):
            st.from_qualid(qs)
        with pytest.raises(ReorderError, match=r"code -4\)"):
            st.download()
