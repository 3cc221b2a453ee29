"""GPU tests of the stream decoder and the FASTQ assembler (include/spring_decode.h, include/spring_fastq_out.h) against
what the REFERENCE'S OWN decompressor wrote: tests/golden/ref_decomp_<case>.npz hold the blocks the real
reorder_compress_streams wrote, the quality and id lines, and the text the real decompress_short (oracle/_ref/ref_decompress)
made of them for a few ranges (tests/golden/make_ref_golden.py).  DecodeStage decodes the stored blocks, FastqOutStage
assembles its output with the stored lines, and the text and the record offset table must equal the stored text: no model
sits in between.  The live run -- the real decompressor reading what the GPU stages wrote -- is
tests/test_gpu_fastq_out.py::test_reference_decompressor_reads_what_the_gpu_wrote."""
import numpy as np
import pytest

import qualid_model as qm
import ref_cases as rc
from test_gpu_decode import pack_seq, window

pytestmark = pytest.mark.gpu


def record_offsets(text, quality):
    """Record offsets of a reference-written text: a record is four lines, two without quality."""
    per = 4 if quality else 2
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    assert len(nl) % per == 0 and (len(text) == 0 or nl[-1] == len(text) - 1)
    return np.concatenate([[0], nl[per - 1::per] + 1]).astype(np.uint64)


def same(fo, want, quality, what):
    text, off = fo.download()
    assert text == want, (what, "text")
    assert np.array_equal(off, record_offsets(want, quality)), (what, "rec_off")
    assert fo.info["bytes"] == len(want) and fo.info["num_units"] == len(off) - 1, what


@pytest.mark.parametrize("case", sorted(rc.DECOMP_FIXTURES))
def test_decode_and_assemble_equal_the_reference_text(case):
    """Every stored range two ways -- the whole file decoded and cut by unit_range = (start_num, end_num); the window of
    blocks the reference opened for it (first_block / num_blocks, decompress.cpp:122-138) decoded alone and cut by the
    range inside the window -- each from host arrays and from contexts in HBM."""
    from spring_amd import DecodeStage, FastqOutStage, QualIdStage
    g = rc.load_decomp_fixture(case)
    N, pe, preserve_order, B, code = g["N"], g["pe"], g["preserve_order"], g["B"], g["code"]
    U = N // 2 if pe else N
    nf = 2 if pe else 1
    quality, numbered = g["quality"] is not None, g["ids"] is None
    assert 8 <= U <= 40 and B in (3, 4) and len(g["ranges"]) >= 2
    with DecodeStage() as ds, FastqOutStage() as fo, QualIdStage() as q1, QualIdStage() as q2, QualIdStage() as i1, \
            QualIdStage() as i2:
        ds.seq_from_host(*pack_seq(g["seq"], 3))
        qctx, ictx = [q1, q2][:nf], [i1, i2][:nf]
        for m in range(nf):   # the file's quality and id blocks in HBM, in slot order
            for ctx, lines, kind in ((qctx[m], g["quality"], qm.QUALITY), (ictx[m], g["ids"], qm.ID)):
                if lines is not None:
                    ctx.set_order(None, N, pe)
                    ctx.from_lines(kind, rc.image(lines[m]), num_reads_per_block=B)

        def sources(m, lo, hi, hbm):
            """quality / ids / id keywords of file m + 1 for the units [lo, hi)."""
            src = 0 if (m == 1 and code is not None) else m   # paired_id_match: file 1's ids, modify_id makes file 2's
            kw = dict(paired_end=pe, num_reads_per_block=B, mate=m, preserve_id=not numbered,
                      paired_id_code=code if (m == 1 and code is not None) else None)
            if quality:
                kw["quality"] = qctx[m] if hbm else b"".join(g["quality"][m][lo:hi])
            if not numbered:
                kw["ids"] = ictx[src] if hbm else rc.image(g["ids"][src][lo:hi])
            return kw

        for (a, b, num_thr), want in g["text"].items():
            info = ds.from_host(g["streams"], N, pe, preserve_order, B)
            assert info["num_units"] == U
            whole = [ds.download(m) for m in range(nf)]
            for m in range(nf):
                for hbm in (False, True):
                    fo.assemble(ds if hbm else whole[m], N, unit_range=(a, b), **sources(m, 0, U, hbm))
                    same(fo, want[m], quality, (case, a, b, m, hbm, "file"))
                    assert fo.info["first_slot"] == a
            used = rc.consumed_blocks(U, B, num_thr, a, b)
            b0, nb = used[0], len(used)
            lo, hi = b0 * B, min((b0 + nb) * B, U)
            info = ds.from_host(window(g["streams"], b0, nb), N, pe, preserve_order, B, first_block=b0)
            assert info["num_units"] == hi - lo and info["first_block"] == b0
            for m in range(nf):
                part = ds.download(m)
                assert part[0] == whole[m][0][int(whole[m][1][lo]):int(whole[m][1][hi])]
                for hbm in (False, True):
                    fo.assemble(ds if hbm else part, N, first_block=b0, num_blocks=nb, unit_range=(a - lo, b - lo),
                                **sources(m, lo, hi, hbm))
                    same(fo, want[m], quality, (case, a, b, m, hbm, "window"))
                    assert fo.info["first_slot"] == a
