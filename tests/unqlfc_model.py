"""The checker of the QLFC decoder stage (include/spring_unqlfc.h): libbsc's bsc_coder_decompress for
LIBBSC_CODER_QLFC_STATIC in fast mode, restated in plain Python from what the format is (DESIGN.md sections 18 and 20).
Parameters, slot numbering, state tables, cases and the encoder come from tests/qlfc_model.py.  Where the real function
reads or writes outside its buffers the stage has rules of its own; decompress() returns (bytes, violation), violation
one of VIOLATIONS or None."""
import struct

import qlfc_model as qm

# the well-formedness rules of include/spring_unqlfc.h, in the order a segment is checked
VIOLATIONS = ("chunks", "table", "entry", "sum", "length", "size", "rank", "exponent", "run", "units")
COUNTERS = ("runs", "events", "escaped", "max_exp", "units")


class _Stop(Exception):
    pass


class _Decoder:
    """The range decoder (rangecoder.h:152-180): 16-bit units, three to start and one per normalisation.  A unit behind
    the payload's end stops the chunk."""

    def __init__(self, payload):
        self.units = struct.unpack("<%dH" % (len(payload) // 2), payload[:len(payload) // 2 * 2])
        self.at, self.code, self.range = 0, 0, 0xffffffff

    def start(self):
        for _ in range(3):
            self.code = (self.code << 16 | self.unit()) & 0xffffffff

    def unit(self):
        if self.at >= len(self.units):
            raise _Stop("units")
        self.at += 1
        return self.units[self.at - 1]

    def bit(self, p=2048):
        r = (self.range >> 12) * p
        if self.code >= r:
            self.code -= r
            self.range -= r
            b = 1
        else:
            self.range = r
            b = 0
        if self.range < 0x10000:
            self.range <<= 16
            self.code = (self.code << 16 | self.unit()) & 0xffffffff
        return b


def decode_chunk(payload, n, tables, stats=None):
    """bsc_qlfc_static_decode (qlfc.cpp:1038-1297) under the stage's rules -> (the chunk's bytes, violation).  n: the
    chunk's size as the segment's header states it.  stats, a dictionary, is added to by every chunk: runs, events,
    escaped (runs decoded on the escape path) and units (16-bit units read) as sums, max_exp (the largest run exponent)
    as a maximum, payload_units (the units the payload holds) as one entry per chunk."""
    rank_table, run_table = tables
    rows, mix = qm.params()
    count = dict.fromkeys(COUNTERS, 0)
    out = bytearray()
    slots = {}
    de = _Decoder(payload)
    try:
        de.start()
        size = 0
        for _ in range(32):
            size += size + de.bit()
        if size != n:
            raise _Stop("size")
        # the symbol table (qlfc.cpp:1061-1105): a bit is read only where both values are still possible
        mtf, used, prev = [], set(), -1
        max_rank = 7
        for _ in range(256):
            cur = 0
            for b in range(7, -1, -1):
                cand = [c for c in range(256) if (c == prev or c not in used) and c >> (b + 1) == cur]
                one, zero = any(c >> b & 1 for c in cand), not all(c >> b & 1 for c in cand)
                cur += cur + (de.bit() if one and zero else int(one))
            mtf.append(cur)
            if cur == prev:
                max_rank = qm.log2(len(mtf) - 2)
                break
            prev = cur
            used.add(cur)
        entries = len(mtf)             # the symbols, and the last one again unless all 256 are listed

        def code(fam, sym, state, hi, lo):
            count["events"] += 1
            lb = qm.LO_BITS[fam]
            p, mine = 0, []
            for kind, who in ((0, sym), (1, state), (2, 0)):
                cls = 3 * fam + kind
                slot = cls << qm.CLASS_SHIFT | hi << (8 + lb) | who << lb | lo
                v = slots.get(slot, 2048)
                p += v * mix[fam][kind]
                mine.append((slot, cls, v))
            bit = de.bit(p >> 5)
            for slot, cls, v in mine:
                th0, ar0, th1, ar1 = rows[cls]
                slots[slot] = v - (((v - th1) * ar1) >> 12) if bit else v + (((4096 - th0 - v) * ar0) >> 12)
            return bit

        rank_hist, run_hist = [0] * 256, [0] * 256
        ctx_rank0 = ctx_rank4 = ctx_run = avg_rank = 0
        while len(out) < n:
            count["runs"] += 1
            c = mtf[0]
            state = int(rank_table[ctx_run << 11 | ctx_rank4 << 3 | rank_hist[c]])
            rank = 1
            if avg_rank < 32:
                if code(qm.RANK_TOP, c, state, 0, 0):
                    if max_rank < 1:
                        raise _Stop("rank")          # one or two symbols: no rank but 1
                    e = 1
                    while e != max_rank and code(qm.RANK_EXP, c, state, 0, e - 1):
                        e += 1
                    rank_hist[c] = e
                    for _ in range(e):
                        rank += rank + code(qm.RANK_MAN, c, state, e, rank)
                else:
                    rank_hist[c] = 0
            else:
                count["escaped"] += 1
                rank, ctx = 0, 1
                for _ in range(max_rank + 1):
                    bit = code(qm.RANK_ESC, c, state, 0, ctx)
                    ctx += ctx + bit
                    rank += rank + bit
                if rank == 0:
                    raise _Stop("rank")
                rank_hist[c] = qm.log2(rank)
            if rank >= entries:
                raise _Stop("rank")
            mtf[:rank + 1] = mtf[1:rank + 1] + [c]
            avg_rank = (avg_rank * 124 + rank * 4) >> 7
            rank -= 1
            state = int(run_table[ctx_rank0 << 10 | ctx_run << 6 | min(rank, 7) << 3 | min(run_hist[c], 7)])
            run = 1
            if code(qm.RUN_TOP, c, state, 0, 0):
                e = 1
                while code(qm.RUN_EXP, c, state, 0, e - 1):
                    e += 1
                    if e == 32:
                        raise _Stop("exponent")
                count["max_exp"] = max(count["max_exp"], e)
                run_hist[c] = (run_hist[c] + 3 * e + 3) >> 2
                ctx = 1
                for _ in range(e):
                    bit = code(qm.RUN_MAN, c, state, e, ctx)
                    run += run + bit
                    ctx = ctx + ctx + bit if e <= 5 else ctx + 1
            else:
                run_hist[c] = (run_hist[c] + 2) >> 2
            ctx_rank0 = (ctx_rank0 << 1 | (rank == 0)) & 7
            ctx_rank4 = (ctx_rank4 << 2 | min(rank, 3)) & 0xff
            ctx_run = (ctx_run << 1 | (run < 3)) & 0xf
            if run > n - len(out):
                raise _Stop("run")
            out += bytes([c]) * run
        violation = None
    except _Stop as stop:
        violation = stop.args[0]
    if stats is not None:
        count["units"] = de.at
        for key in COUNTERS:
            stats[key] = max(stats.get(key, 0), count[key]) if key == "max_exp" else stats.get(key, 0) + count[key]
        stats.setdefault("payload_units", []).append(len(payload) // 2)
    return bytes(out), violation


def chunk_table(coded, out_size):
    """The header rules -> ([(input size, coded size, payload offset)], violation)."""
    n = len(coded)
    if n == 0 or coded[0] == 0:
        return [], "chunks"
    k = coded[0]
    if k == 1:
        return [(out_size, n - 1, 1)], None
    if 1 + 8 * k > n:
        return [], "table"
    v = struct.unpack_from("<%di" % (2 * k), coded, 1)
    sizes = list(zip(v[0::2], v[1::2]))
    if any(a < 0 or b < 0 or b > a for a, b in sizes):
        return [], "entry"
    if sum(a for a, _ in sizes) != out_size:
        return [], "sum"
    if 1 + 8 * k + sum(b for _, b in sizes) != n:
        return [], "length"
    chunks, at = [], 1 + 8 * k
    for a, b in sizes:
        chunks.append((a, b, at))
        at += b
    return chunks, None


def decompress(coded, out_size, tables, stats=None):
    """bsc_coder_decompress(coded, ., LIBBSC_CODER_QLFC_STATIC, .) under the stage's rules -> (bytes, violation); the
    bytes of a violation are what was decoded in front of it."""
    coded = bytes(coded)
    chunks, violation = chunk_table(coded, out_size)
    out = b""
    for j, (a, b, at) in enumerate(chunks):
        if coded[0] > 1 and a == b:
            part = coded[at:at + b]
            if stats is not None:
                stats["raw"] = stats.get("raw", 0) + 1
        else:
            part, violation = decode_chunk(coded[at:at + b], a, tables, stats)
        out += part
        if violation:
            break
    return out, violation


# ---------------------------------------------------------------------------------------------- malformed payloads
def encode_forced(data, tables, size=None, force=None):
    """qlfc_model.encode_chunk with CheckEOB off and one thing forced, for payloads the encoder never writes:
    size: the 32-bit size word; force = (run index, what, value) with what "rank" (the rank coded for that run, on the
    path the run takes) or "run" (the length coded for it).  Done by patching what encode_chunk reads."""
    real_ranks, real_bit = qm.chunk_ranks, qm._Coder.bit

    def ranks(d):
        runs, rk, order, max_rank = real_ranks(d)
        if force and force[1] == "rank":
            rk[force[0]] = force[2]
        if force and force[1] == "run":
            runs[force[0]][1] = force[2]
        return runs, rk, order, max_rank

    calls = [0]

    def bit(self, b, p):
        if size is not None and calls[0] < 32:
            b = size >> (31 - calls[0]) & 1
        calls[0] += 1
        real_bit(self, b, p)

    qm.chunk_ranks, qm._Coder.bit = ranks, bit
    try:
        return qm.encode_chunk(bytes(data), len(data), tables, check=False)
    finally:
        qm.chunk_ranks, qm._Coder.bit = real_ranks, real_bit


# ---------------------------------------------------------------------------------------------- the case contents
# (n, seed) of qm._letters(n, 9, seed) found by tools/qlfc_edge_search.py units, per pair of state tables: the payload
# holds 256 units (the last one on the last place of a 64-unit load) and 257 (on the first place of the next).
UNIT_CASES = {
    "real": dict(last=(1057, 1000), first=(1062, 1000)),
    101: dict(last=(1017, 1000), first=(1021, 1000)),
    202: dict(last=(1017, 1000), first=(1021, 1000)),
}
RUN_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 200)


def aligned_runs():
    """A text in which a run of every length of RUN_LENGTHS starts at every offset 0 .. 15 modulo 16, over three
    letters; starts: (length, position) of those runs."""
    out, starts, letter = bytearray(), [], 0
    for n in RUN_LENGTHS:
        for o in range(16):
            fill = (o - len(out)) % 16 or 16
            out += bytes([65 + letter % 3]) * fill
            starts.append((n, len(out)))
            out += bytes([65 + (letter + 1) % 3]) * n
            letter += 2
    return bytes(out), starts


def payload(data, tables):
    """One chunk coded to its end whatever its length: [1][payload], with CheckEOB off."""
    return b"\x01" + qm.encode_chunk(bytes(data), len(data), tables, check=False)


def escaped_run(data):
    """The first run of a text that is coded on the escape path (avgRank >= 32 in front of it)."""
    avg = 0
    for r, rank in enumerate(qm.chunk_ranks(data)[1]):
        if avg >= 32:
            return r
        avg = (avg * 124 + rank * 4) >> 7
    raise ValueError("no run on the escape path")


def malformed(tables):
    """-> {name: (coded bytes, out_size, the violation the rules name)}: one construction per rule."""
    one = qm.case("letters5")                     # one chunk, five symbols: maxRank 2, six table entries
    n = len(one)
    good = qm.compress(one, tables)[0]
    two = qm.case("eq262145")                     # two chunks
    good2 = qm.compress(two, tables)[0]
    (a0, b0), (a1, b1) = [struct.unpack_from("<ii", good2, 1 + 8 * j) for j in range(2)]
    table = lambda *v: bytes([2]) + struct.pack("<iiii", *v) + good2[17:]
    ring = qm.case("ring100")
    runs = qm.chunk_ranks(one)[0]
    return {
        "cut2": (good[:-2], n, "units"),
        "cut1": (good[:-1], n, "units"),
        "k0": (b"\0" + good[1:], n, "chunks"),
        "short_table": (good2[:9], len(two), "table"),
        "coded_above_input": (table(a0, a0 + 1, a1, b1), len(two), "entry"),
        "negative_entry": (table(a0, b0, a1, -1), len(two), "entry"),
        "sum_plus_one": (table(a0 + 1, b0, a1, b1), len(two), "sum"),
        "one_byte_more": (good2 + b"\0", len(two), "length"),
        "out_size_plus_one": (good, n + 1, "size"),
        "out_size_minus_one": (good, n - 1, "size"),
        "size_word": (b"\x01" + encode_forced(one, tables, size=n + 1), n, "size"),
        "rank_above": (b"\x01" + encode_forced(one, tables, force=(10, "rank", 6)), n, "rank"),
        "rank_zero": (b"\x01" + encode_forced(ring, tables, force=(escaped_run(ring), "rank", 0)), len(ring), "rank"),
        "exponent32": (b"\x01" + encode_forced(one, tables, force=(5, "run", 1 << 32)), n, "exponent"),
        "last_run_long": (b"\x01" + encode_forced(one, tables, force=(len(runs) - 1, "run", runs[-1][1] + 1)), n, "run"),
    }
