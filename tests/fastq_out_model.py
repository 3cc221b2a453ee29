"""Checker of the FASTQ assembler (include/spring_fastq_out.h): a direct Python restatement of the three reference
functions the stage replaces, on lists of ids, reads and qualities.  No attempt at speed.

  write_fastq_block   util.cpp:56-69 (the plain-text branch): id '\\n' read '\\n' and, with preserve_quality,
                      "+\\n" quality '\\n' per unit
  modify_id           util.cpp:255-267
  numbered ids, the start_num / end_num cut    decompress.cpp:373-378, :402-419

Pinned by the reference's own code: tests/test_models_vs_ref_decompress.py runs the real decompress_short
(oracle/_ref/ref_decompress: decompress.cpp whole, write_fastq_block without its gzip branch) on reference-written blocks
and compares the files it writes byte for byte with assemble() -- numbered ids across a digit change and block edges,
modify_id with codes 1, 2 and 3 (the first of two spaces, a one-character id), id_2 read without a match, ranges inside
a block, on block edges, across steps and to the last unit at one and three blocks per step, two-line records, block
windows.  One divergence is kept there: the reference writes a stale quality line behind an empty read that ends a
block (bsc_str_array.cpp:149-162); this model writes the empty line.  The round trips of tests/test_fastq_out_cpu.py and
tests/test_gpu_fastq_out.py end at the bytes of the FASTQ that went in."""
import numpy as np


class Refused(Exception):
    """Input the stage refuses (SPRING_REORDER_E_ARG)."""


def modify_id(rid, code):
    """modify_id; the cases where the reference has undefined behaviour are refused."""
    if code == 2:
        return rid
    if code == 1:
        if not rid:
            raise Refused("code 1 on an empty id")
        return rid[:-1] + b"2"
    if code == 3:
        i = rid.find(b" ")
        if i < 0 or i + 1 >= len(rid):
            raise Refused("code 3 without a space, or with a trailing one")
        return rid[:i + 1] + b"2" + rid[i + 2:]
    raise Refused("Invalid paired id code.")


def numbered_ids(first_slot, n, mate):
    """id_array[i] = "@" + to_string(num_reads_done + i + 1) + "/" + to_string(j + 1)"""
    return [b"@%d/%d" % (first_slot + i + 1, mate + 1) for i in range(n)]


def records(ids, reads, quals=None):
    """write_fastq_block over one window -> list of record texts."""
    if len(ids) != len(reads) or (quals is not None and len(quals) != len(reads)):
        raise Refused("array lengths differ")
    if quals is None:
        return [i + b"\n" + r + b"\n" for i, r in zip(ids, reads)]
    for r, q in zip(reads, quals):
        if len(r) != len(q):
            raise Refused("quality length differs from the read's")
    return [i + b"\n" + r + b"\n+\n" + q + b"\n" for i, r, q in zip(ids, reads, quals)]


def assemble(ids, reads, quals=None, unit_range=None, paired_id_code=None):
    """-> (text, rec_off: uint64 array of len + 1) of the units [start, end) of the window (all by default); ids are the
    window's (file 1's with paired_id_code, which modify_id turns into file 2's)."""
    if paired_id_code is not None:
        ids = [modify_id(i, paired_id_code) for i in ids]
    recs = records(ids, reads, quals)
    a, b = (0, len(recs)) if unit_range is None else unit_range
    if not 0 <= a <= b <= len(recs):
        raise Refused("range outside the window")
    recs = recs[a:b]
    off = np.zeros(len(recs) + 1, np.uint64)
    if recs:
        off[1:] = np.cumsum([len(r) for r in recs])
    return b"".join(recs), off


def reads_image(reads):
    """-> (bases back to back, len + 1 offsets): what DecodeStage.download gives."""
    off = np.zeros(len(reads) + 1, np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) for r in reads])
    return b"".join(reads), off


def id_image(ids):
    return b"".join(i + b"\n" for i in ids)


def block_table(lines, B, nl):
    """num_blocks + 1 offsets of lines cut into blocks of B (nl = 1: each line carries a '\\n')."""
    off = [0]
    for b in range(0, len(lines), B):
        off.append(off[-1] + sum(len(x) + nl for x in lines[b:b + B]))
    return np.array(off, np.uint64)
