"""Checker of the quality and id stage (include/spring_qualid.h), written from the reference's semantics in plain
Python: lines placed into a slot list, cut into blocks, joined.  No attempt at speed.

  order_array   reorder_compress_quality_id.cpp:101-125 (generate_order_pe / generate_order_se)
  lines         read_fastq_block + remove_CR_from_end (util.cpp:31-54)
  tables        generate_illumina_binning_table / generate_binary_binning_table (util.cpp:166-188)
  id patterns   find_id_pattern / check_id_pattern (util.cpp:196-253)"""
import numpy as np

QUALITY, ID = 0, 1


class Refused(Exception):
    """Input the stage refuses (SPRING_REORDER_E_ARG)."""


def order_array(order, num_reads, paired_end):
    """line j of a file -> slot (list of U entries); order None = identity."""
    if paired_end and num_reads % 2:
        raise Refused("odd num_reads")
    U = num_reads // 2 if paired_end else num_reads
    if order is None:
        return list(range(U))
    order = [int(x) for x in order]
    if len(order) != num_reads or sorted(order) != list(range(num_reads)):
        raise Refused("not a permutation")
    out = [None] * U
    if not paired_end:
        for i, o in enumerate(order):
            out[o] = i
    else:
        pos = 0
        for o in order:
            if o < num_reads // 2:
                out[o] = pos
                pos += 1
    return out


def _lines(text):
    """getline over a text: a missing final newline is accepted."""
    if not text:
        return []
    ls = text.split(b"\n")
    if text.endswith(b"\n"):
        ls.pop()
    return ls


def _no_cr(s):
    return s[:-1] if s.endswith(b"\r") else s


def fastq_lines(text):
    """-> (ids, reads, qualities) of a FASTQ text, CR trimmed."""
    ls = _lines(text)
    if len(ls) % 4:
        raise Refused("Invalid FASTQ(A) file. Number of lines not multiple of 4(2)")
    ids = [_no_cr(x) for x in ls[0::4]]
    reads = [_no_cr(x) for x in ls[1::4]]
    quals = [_no_cr(x) for x in ls[3::4]]
    for r, q in zip(reads, quals):
        if len(r) != len(q):
            raise Refused("Read length does not match quality length.")
    return ids, reads, quals


def illumina_table():
    t = []
    for c in range(128):
        q = c - 33
        for last, to in ((1, 0), (9, 6), (19, 15), (24, 22), (29, 27), (34, 33), (39, 37)):
            if q <= last:
                t.append(33 + to)
                break
        else:
            t.append(33 + 40)
    return bytes(t)


def binary_table(thr, high, low):
    return bytes(33 + low if c < 33 + thr else 33 + high for c in range(128))


def build(lines, kind, slots, B, table=None):
    """lines in file order -> dict(bytes, len, block_off, changed, max_len) of the stage's result."""
    U = len(slots)
    if B == 0:
        raise Refused("num_reads_per_block == 0")
    if len(lines) != U:
        raise Refused("line count differs from the units of the order")
    by_slot = [None] * U
    for j, s in enumerate(slots):
        by_slot[s] = lines[j]
    changed = 0
    if kind == QUALITY and table is not None:
        for s, q in enumerate(by_slot):
            if any(c >= 128 for c in q):
                raise Refused("quality byte >= 128 under a table")
            t = bytes(table[c] for c in q)
            changed += sum(a != b for a, b in zip(q, t))
            by_slot[s] = t
    term = b"\n" if kind == ID else b""
    data, off = [], [0]
    for b in range((U + B - 1) // B):
        blk = b"".join(x + term for x in by_slot[b * B:(b + 1) * B])
        data.append(blk)
        off.append(off[-1] + len(blk))
    return dict(bytes=b"".join(data), len=np.array([len(x) for x in by_slot], np.uint32),
                block_off=np.array(off, np.uint64), changed=changed, max_len=max([len(x) for x in by_slot] + [0]),
                lines=by_slot)


def from_fastq(text, kind, slots, B, table=None):
    ids, reads, quals = fastq_lines(text)
    return build(quals if kind == QUALITY else ids, kind, slots, B, table)


def from_lines(image, kind, slots, B, table=None):
    return build(_lines(image), kind, slots, B, table)


def _match(code, a, b):
    """check_id_pattern's three cases; codes 1 and 3 never match an empty id."""
    n = len(a)
    if code == 2:
        return a == b
    if n == 0:
        return False
    if code == 1:
        return a[-1:] == b"1" and b[-1:] == b"2" and a[:-1] == b[:-1]
    i = 0
    while i < n:
        if a[i] != b[i]:
            break
        if a[i] == 0x20:
            if i < n - 1 and a[i + 1] == 0x31 and b[i + 1] == 0x32:
                i += 1
            else:
                break
        i += 1
    return i == n


def find_id_pattern(a, b):
    if len(a) != len(b):
        return 0
    for code in (2, 1, 3):
        if _match(code, a, b):
            return code
    return 0


def check_id_pattern(a, b, code):
    return len(a) == len(b) and _match(code, a, b)


def id_pattern(text_1, text_2):
    """paired_id_code of two FASTQ texts (preprocess.cpp:116-121, :215-217, :287-292)."""
    ids1, ids2 = fastq_lines(text_1)[0], fastq_lines(text_2)[0]
    if len(ids1) != len(ids2):
        raise Refused("Number of reads in paired files do not match.")
    if not ids1:
        return 0
    code = find_id_pattern(ids1[0], ids2[0])
    if code and all(check_id_pattern(a, b, code) for a, b in zip(ids1, ids2)):
        return code
    return 0
