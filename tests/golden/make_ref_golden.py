"""Writes tests/golden/ref_streams_<case>.npz and ref_qualid_<case>.npz: what the REFERENCE'S OWN writers produce for
a handful of the hand-built cases of tests/ref_cases.py, so that the GPU tests can compare with reference-written
blocks where oracle/_ref is not built.  Reads only oracle/_ref (ref_streams, libref_qualid.so; `make -C oracle`), never
the reference tree.  Data only: the inputs and the raw blocks.  Run: python tests/golden/make_ref_golden.py [family]
(family = streams, qualid, decomp or stage writes that family's files alone).

ref_streams_<case>.npz   the encoder image (pos, rc, noise, noisepos, order, rlen, unaligned), the consensus `seq`, the
                         original `reads` in slot order ('\n'-joined), num_reads / paired_end / preserve_order /
                         num_reads_per_block, and per stream `<name>` = the raw blocks back to back as
                         reorder_compress_streams wrote them (inflated by the real BSC_decompress), `<name>.off` = the
                         block offsets.
ref_qualid_<case>.npz    the line images quality_1 / id_1 (/ quality_2 / id_2), `order` (read_order.bin), and per file
                         `<name>.bytes` / `.len` / `.off` = the lines of every block as reorder_compress_quality_id wrote
                         them (read back by the real BSC_str_array_decompress / decompress_id_block; ids with their
                         '\n'), the line lengths in slot order and the block offsets; `quality_<m>.illumina.*` = the
                         same after the real quantize_quality with the real Illumina table, as preprocess applies it.
ref_stage_<case>.npz     the cases of tests/ref_stage_cases.py through the reference's whole stages (ref_reorder,
                         ref_encoder): `in.dna` / `in.dnaN` / `in.order_N` (input_clean_1.dna, input_N.dna,
                         read_order_N.bin), n, L, T, K, `reorder/<file>` = every file reorder_main<N> left (its four gzip
                         files uncompressed; for thr3 the hand-made three-thread set instead, `reorder_by_reference` =
                         False), `unmatched` = the number it printed, `encoder/<file>` = every file encoder_main<N> left
                         on that set (read_seq.bin.<t>.raw = the .bsc inflated by the real BSC_decompress), `matched` =
                         the two numbers it printed.  fixed33 / fixed150 / fixed251 are recorded for a
                         reverse-complemented record in temp.dna.0 (asserted when they are written).
ref_decomp_<case>.npz    the cases of tests/ref_cases.py::DECOMP_FIXTURES through the reference's writers and then its real
                         decompressor (ref_decompress = decompress_short whole): the consensus `seq`, num_reads /
                         paired_end / preserve_order / num_reads_per_block / paired_id_code (0 = no paired_id_match), per
                         stream `<name>` / `<name>.off` as above, the line images `id_<m>` / `quality_<m>` in slot order
                         where the case preserves them, `ranges` = rows (start_num, end_num, decompressor num_thr), and
                         `text_<m>.<k>` = the file <m> that decompress_short wrote for row k.  No record of the kept
                         stale-quality divergence is in them (asserted when they are written)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_cases as rc  # noqa: E402
import streams_model as sm  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

import ref_stage_cases as sc  # noqa: E402

assert po.ref_streams_bin() and po.ref_qualid_lib() and po.ref_reorder_bin() and po.ref_encoder_bin(), "oracle/_ref is not built"
u8 = lambda b: np.frombuffer(bytes(b), np.uint8)  # noqa: E731
offsets = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)  # noqa: E731

only = sys.argv[1] if len(sys.argv) > 1 else None   # streams | qualid | decomp | stage: that family of files alone
assert only in (None, "streams", "qualid", "decomp", "stage")

for case in rc.STREAM_FIXTURES if only in (None, "streams") else ():
    enc, seq, N, reads, pe, preserve_order, B = rc.stream_fixture_inputs(case)
    blocks, left = po.ref_streams(enc, N, pe, preserve_order, B, num_thr=2)
    out = {k: (u8(enc[k]) if isinstance(enc[k], bytes) else np.asarray(enc[k])) for k in rc.ENC_KEYS}
    out.update(seq=u8(seq.encode()), reads=u8("\n".join(reads).encode()), num_reads=np.uint32(N), paired_end=np.bool_(pe),
               preserve_order=np.bool_(preserve_order), num_reads_per_block=np.uint32(B))
    for s in sm.stream_names(pe):
        out[s] = u8(b"".join(blocks[s]))
        out[s + ".off"] = offsets([len(x) for x in blocks[s]])
    path = os.path.join(HERE, "ref_streams_%s.npz" % case)
    np.savez_compressed(path, **out)
    print(case, N, len(blocks["read_flag.txt"]), os.path.getsize(path))

for case in rc.QUALID_FIXTURES if only in (None, "qualid") else ():
    files, order, n, pe, B = rc.qualid_fixture_inputs(case)
    U = n // 2 if pe else n
    out = dict(order=order, num_reads=np.uint32(n), paired_end=np.bool_(pe), num_reads_per_block=np.uint32(B))
    slot = po.ref_order("pe" if pe else "se", order)   # the real generate_order_pe / _se: line j -> slot
    for table in ("none", "illumina"):
        f = dict(files)
        if table == "illumina":
            f = {k: po.ref_quantize(v, po.ref_quality_table("illumina")) for k, v in files.items() if k.startswith("quality")}
        lens = {}
        for k, v in f.items():
            if k.startswith("quality"):
                ln = np.zeros(U, np.uint32)
                ln[slot] = [len(x) for x in v]
                lens[k] = ln
        got, left = po.ref_qualid({k: rc.image(v) for k, v in f.items()}, order, n, pe, B, lens, num_thr=2)
        for k in f:
            key = k + ("" if table == "none" else ".illumina")
            if k.startswith("id"):
                lines = [x for blk in got[k] for x in blk]
                out[key + ".bytes"] = u8(b"".join(x + b"\n" for x in lines))
                out[key + ".len"] = np.array([len(x) for x in lines], np.uint32)
                out[key + ".off"] = offsets([sum(len(x) + 1 for x in blk) for blk in got[k]])
            else:
                out[key + ".bytes"] = u8(b"".join(got[k]))
                out[key + ".len"] = lens[k]
                out[key + ".off"] = offsets([len(x) for x in got[k]])
    for k, v in files.items():
        out[k] = u8(rc.image(v))
    path = os.path.join(HERE, "ref_qualid_%s.npz" % case)
    np.savez_compressed(path, **out)
    print(case, n, os.path.getsize(path))

LARGEST = 28763   # enc_var2k.npz, the largest fixture before these: none of the ref_stage / ref_decomp files may be larger
if only in (None, "decomp"):
    assert po.ref_decompress_bin(), "oracle/_ref/ref_decompress is not built"
    for case in rc.DECOMP_FIXTURES:
        g = rc.decomp_fixture_inputs(case)
        N, pe, preserve_order, B = g["N"], g["pe"], g["preserve_order"], g["B"]
        U = N // 2 if pe else N
        blocks, _ = po.ref_streams(g["enc"], N, pe, preserve_order, B, num_thr=g["T"])
        out = dict(seq=u8(g["seq"].encode()), num_reads=np.uint32(N), paired_end=np.bool_(pe), preserve_order=np.bool_(preserve_order),
                   num_reads_per_block=np.uint32(B), paired_id_code=np.uint8(g["code"] or 0),
                   ranges=np.array(g["ranges"], np.uint32))
        for s in sm.stream_names(pe):
            out[s] = u8(b"".join(blocks[s]))
            out[s + ".off"] = offsets([len(x) for x in blocks[s]])
        for m in range(2 if pe else 1):
            if g["ids"] is not None:
                out["id_%d" % (m + 1)] = u8(rc.image(g["ids"][m]))
            if g["quality"] is not None:
                out["quality_%d" % (m + 1)] = u8(rc.image(g["quality"][m]))
        for k, (a, b, num_thr) in enumerate(g["ranges"]):
            texts, left = po.ref_decompress(blocks, rc.seq_pieces(g["seq"], g["T"]), N, pe, preserve_order, B, quality=g["quality"],
                                            ids=g["ids"], paired_id_code=g["code"] or 0, paired_id_match=g["code"] is not None,
                                            num_thr=num_thr, unit_range=(a, b))
            for m, t in enumerate(texts):
                lines = t.split(b"\n")[:-1]
                per = 4 if g["quality"] is not None else 2
                assert len(lines) == per * (b - a)
                # a fixture holds no record of the kept divergence (a stale quality line behind an empty read at the end
                # of a block, tests/test_models_vs_ref_decompress.py): pick another block size if this fails
                assert per == 2 or all(len(x) == len(y) for x, y in zip(lines[1::4], lines[3::4])), (case, a, b, m)
                out["text_%d.%d" % (m + 1, k)] = u8(t)
        path = os.path.join(HERE, "ref_decomp_%s.npz" % case)
        np.savez_compressed(path, **out)
        print(case, N, len(blocks["read_flag.txt"]), os.path.getsize(path))
        assert os.path.getsize(path) <= LARGEST, case

if only not in (None, "stage"):
    sys.exit(0)
for case in sc.FIXTURES:
    out = sc.record_fixture(case)
    if case in sc.R_RECORD_CASES:   # what the case is recorded for: a reverse-complemented record in temp.dna.0
        assert sc.holds_r_record({k[len("reorder/"):]: v.tobytes() for k, v in out.items() if k.startswith("reorder/")}, int(out["L"])), case
    path = os.path.join(HERE, "ref_stage_%s.npz" % case)
    np.savez_compressed(path, **out)
    print(case, int(out["n"]), os.path.getsize(path))
    assert os.path.getsize(path) <= LARGEST, case
