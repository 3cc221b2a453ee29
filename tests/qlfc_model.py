"""The checker of the QLFC stage (include/spring_qlfc.h): libbsc's bsc_coder_compress for LIBBSC_CODER_QLFC_STATIC in
fast mode, restated in plain Python from what the format is.  The predictors live in a dictionary
keyed by slot number and each is updated on its own; the parameters come from spring_amd/csrc/qlfc_params.h, the table
the kernels read too; the two state tables are arguments.  state_tables() reads libbsc's own tables out of the compiled
reference library (oracle/_ref/libref_units.so), which tests/test_qlfc_cpu.py also pins this model to."""
import ctypes as C
import functools
import os
import re
import struct

import numpy as np

import bwt_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("RANK_TOP", "RANK_EXP", "RANK_MAN", "RANK_ESC", "RUN_TOP", "RUN_EXP", "RUN_MAN")
KINDS = ("CHAR", "STATE", "STATIC")
RANK_TOP, RANK_EXP, RANK_MAN, RANK_ESC, RUN_TOP, RUN_EXP, RUN_MAN = range(7)
LO_BITS = (0, 3, 8, 8, 0, 5, 5)     # qlfc_plan.h: the bits of a slot's index below the byte / state
CLASS_SHIFT = 19
RANK_TABLE, RUN_TABLE = 32768, 8192
NOT_COMPRESSIBLE = -3               # LIBBSC_NOT_COMPRESSIBLE


@functools.lru_cache(maxsize=None)
def params():
    """-> (rows[class] = (th0, ar0, th1, ar1), mix[family] = (w_char, w_state, w_static)) from qlfc_params.h."""
    text = open(os.path.join(ROOT, "spring_amd", "csrc", "qlfc_params.h")).read()
    text = text[text.index("#define QLFC_PARAM_TABLE"):]
    rows, mix = {}, {}
    for fam, kind, *v in re.findall(r"ROW\((\w+), (\w+), (-?\d+), (-?\d+), (-?\d+), (-?\d+)\)", text):
        rows[3 * FAMILIES.index(fam) + KINDS.index(kind)] = tuple(int(x) for x in v)
    for fam, *v in re.findall(r"MIX\((\w+), (-?\d+), (-?\d+), (-?\d+)\)", text):
        mix[FAMILIES.index(fam)] = tuple(int(x) for x in v)
    assert sorted(rows) == list(range(21)) and sorted(mix) == list(range(7))
    return rows, mix


def state_tables(path=None):
    """libbsc's model_rank_state_table and model_run_state_table as two uint8 arrays, read from the symbol table of the
    compiled reference library; None when the library or a symbol is missing."""
    path = path or os.path.join(ROOT, "oracle", "_ref", "libref_units.so")
    try:
        blob = open(path, "rb").read()
    except OSError:
        return None
    if blob[:6] != b"\x7fELF\x02\x01":   # ELF64, little-endian
        return None
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    want = {b"_ZL22model_rank_state_table": RANK_TABLE, b"_ZL21model_run_state_table": RUN_TABLE}
    found = {}
    for s in sec:
        if s[1] != 2:                    # SHT_SYMTAB
            continue
        strtab = sec[s[6]]
        for k in range(s[5] // 24):
            name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", blob, s[4] + 24 * k)
            end = blob.index(b"\0", strtab[4] + name)
            sym = blob[strtab[4] + name:end]
            if sym in want and size == want[sym] and 0 < shndx < shnum:
                home = sec[shndx]
                at = home[4] + value - home[3]
                found[sym] = np.frombuffer(blob[at:at + size], np.uint8).copy()
    if len(found) != 2:
        return None
    return found[b"_ZL22model_rank_state_table"], found[b"_ZL21model_run_state_table"]


def random_tables(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, RANK_TABLE, dtype=np.uint8), rng.integers(0, 256, RUN_TABLE, dtype=np.uint8)


class _Coder:
    """The range coder (rangecoder.h:73-129): 16-bit units, carries counted in ffnum.  pend: the shifts that only
    counted a pending unit; flushed[carry]: the pending units written out later, without and with a carry."""

    def __init__(self):
        self.low, self.range, self.ffnum, self.cache, self.out = 0, 0xffffffff, 0, 0, []
        self.pend, self.flushed = 0, [0, 0]

    def shift_low(self):
        low32, carry = self.low & 0xffffffff, self.low >> 32
        if low32 < 0xffff0000 or carry:
            self.out.append((self.cache + carry) & 0xffff)
            self.out.extend([(carry - 1) & 0xffff] * self.ffnum)
            self.flushed[carry] += self.ffnum
            self.ffnum = 0
            self.cache = low32 >> 16
        else:
            self.ffnum += 1
            self.pend += 1
        self.low = (low32 << 16) & 0xffffffff

    def bit(self, b, p):
        r = (self.range >> 12) * p
        if b:
            self.low += r
            self.range -= r
        else:
            self.range = r
        if self.range < 0x10000:
            self.range <<= 16
            self.shift_low()

    def nbytes(self):
        return 2 * len(self.out)

    def finish(self):
        for _ in range(3):
            self.shift_low()
        return struct.pack("<%dH" % len(self.out), *self.out)


def log2(n):
    return n.bit_length() - 1           # bsc_log2 / bsc_log2_256: floor(log2 n), -1 for 0


def chunk_ranks(data):
    """-> (runs as (byte, length), rank per run, the symbols in the order of the table header, maxRank)."""
    a = np.frombuffer(bytes(data), np.uint8)
    heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1]))) if len(a) else np.zeros(0, np.int64)
    runs = [[b, n] for b, n in zip(a[heads].tolist(), np.diff(np.append(heads, len(a))).tolist())]
    mtf, seen, ranks = list(range(256)), [], [0] * len(runs)
    for r in range(len(runs) - 1, -1, -1):      # backwards, run by run (qlfc.cpp:52-109)
        c = runs[r][0]
        k = mtf.index(c)
        mtf.insert(0, mtf.pop(k))
        if c in seen:
            ranks[r] = k
        else:
            ranks[r] = len(seen)
            seen.append(c)
    ranks[-1] = 1
    order = mtf[:len(seen)]                     # by first occurrence in the chunk, front to back
    return runs, ranks, order, (log2(len(order) - 1) if len(order) < 256 else 7)


def encode_chunk(data, output_size, tables, stats=None, check=True):
    """bsc_qlfc_static_encode (qlfc.cpp:448-752) -> the chunk's payload, or None where CheckEOB fires.  stats, a
    dictionary, is added to by every chunk that is coded to its end: runs, events, the range coder's pend,
    flush_nocarry and flush_carry, escaped (runs coded on the escape path) and esc_switches (changes between the two
    rank paths) as sums; max_rank, symbols, lastev (the events in front of the last run) and margin (CheckEOB's
    (output_size - 16) - bytes written, at the last run) as one entry per chunk.  check=False switches CheckEOB off."""
    rank_table, run_table = tables
    rows, mix = params()
    n = len(data)
    runs, ranks, order, max_rank = chunk_ranks(data)
    co = _Coder()
    for b in range(31, -1, -1):
        co.bit(n >> b & 1, 2048)
    # the symbol table: every symbol in header order, then the last one again unless all 256 are used; a bit is coded
    # only where both values are still possible among the symbols not yet used (and the one before)
    used, prev = set(), -1
    for cur in order + (order[-1:] if len(order) < 256 else []):
        for b in range(7, -1, -1):
            cand = [c for c in range(256) if (c == prev or c not in used) and c >> (b + 1) == cur >> (b + 1)]
            if any(c >> b & 1 for c in cand) and not all(c >> b & 1 for c in cand):
                co.bit(cur >> b & 1, 2048)
        prev = cur
        used.add(cur)
    slots, events = {}, 0

    def code(fam, bit, sym, state, hi, lo):
        nonlocal events
        events += 1
        lb = LO_BITS[fam]
        p = 0
        for kind, who in ((0, sym), (1, state), (2, 0)):
            cls = 3 * fam + kind
            slot = cls << CLASS_SHIFT | hi << (8 + lb) | who << lb | lo
            v = slots.get(slot, 2048)
            p += v * mix[fam][kind]
            th0, ar0, th1, ar1 = rows[cls]
            slots[slot] = v - (((v - th1) * ar1) >> 12) if bit else v + (((4096 - th0 - v) * ar0) >> 12)
        co.bit(bit, p >> 5)

    rank_hist, run_hist = [0] * 256, [0] * 256
    ctx_rank0 = ctx_rank4 = ctx_run = avg_rank = 0
    escaped = switches = lastev = margin = 0
    was_escape = False
    for (c, run), rank in zip(runs, ranks):
        if check and co.nbytes() >= output_size - 16:
            return None
        lastev, margin = events, output_size - 16 - co.nbytes()
        escaped += avg_rank >= 32
        switches += (avg_rank >= 32) != was_escape
        was_escape = avg_rank >= 32
        state = int(rank_table[ctx_run << 11 | ctx_rank4 << 3 | rank_hist[c]])
        if avg_rank < 32:
            if rank == 1:
                rank_hist[c] = 0
                code(RANK_TOP, 0, c, state, 0, 0)
            else:
                code(RANK_TOP, 1, c, state, 0, 0)
                e = rank_hist[c] = log2(rank)
                for j in range(e - 1):
                    code(RANK_EXP, 1, c, state, 0, j)
                if e < max_rank:
                    code(RANK_EXP, 0, c, state, 0, e - 1)
                ctx = 1
                for b in range(e - 1, -1, -1):
                    bit = rank >> b & 1
                    code(RANK_MAN, bit, c, state, e, ctx)
                    ctx += ctx + bit
        else:
            rank_hist[c] = log2(rank)
            ctx = 1
            for b in range(max_rank, -1, -1):
                bit = rank >> b & 1
                code(RANK_ESC, bit, c, state, 0, ctx)
                ctx += ctx + bit
        avg_rank = (avg_rank * 124 + rank * 4) >> 7
        rank -= 1
        state = int(run_table[ctx_rank0 << 10 | ctx_run << 6 | min(rank, 7) << 3 | min(run_hist[c], 7)])
        if run == 1:
            run_hist[c] = (run_hist[c] + 2) >> 2
            code(RUN_TOP, 0, c, state, 0, 0)
        else:
            code(RUN_TOP, 1, c, state, 0, 0)
            e = log2(run)
            run_hist[c] = (run_hist[c] + 3 * e + 3) >> 2
            for j in range(e - 1):
                code(RUN_EXP, 1, c, state, 0, j)
            code(RUN_EXP, 0, c, state, 0, e - 1)
            ctx = 1
            for b in range(e - 1, -1, -1):
                bit = run >> b & 1
                code(RUN_MAN, bit, c, state, e, ctx)
                ctx = ctx + ctx + bit if e <= 5 else ctx + 1
        ctx_rank0 = (ctx_rank0 << 1 | (rank == 0)) & 7
        ctx_rank4 = (ctx_rank4 << 2 | min(rank, 3)) & 0xff
        ctx_run = (ctx_run << 1 | (run < 3)) & 0xf
    body = co.finish()                  # the three closing shifts count too
    if stats is not None:
        sums = dict(runs=len(runs), events=events, pend=co.pend, flush_nocarry=co.flushed[0], flush_carry=co.flushed[1],
                    escaped=escaped, esc_switches=switches)
        for key, v in sums.items():
            stats[key] = stats.get(key, 0) + v
        for key, v in dict(max_rank=max_rank, symbols=len(order), lastev=lastev, margin=margin).items():
            stats.setdefault(key, []).append(v)
    return body


def num_chunks(n):
    return 1 if n < 256 * 1024 else 2 if n < 4 << 20 else 4 if n < 16 << 20 else 8


def split(data, k):
    """bsc_coder_split_blocks (coder.cpp:69-108) -> the k + 1 cut positions."""
    a = np.frombuffer(data, np.uint8)
    n = len(a)
    pos = np.arange(1, n, 32)
    hits = pos[a[pos] != a[pos - 1]]
    if len(hits) > k:
        per = len(hits) // k
        return [0] + [int(hits[j * per - 1]) for j in range(1, k)] + [n]
    return [n // k * p for p in range(k)] + [n]


def compress(data, tables, stats=None):
    """bsc_coder_compress(data, ., n, LIBBSC_CODER_QLFC_STATIC, .) -> (bytes, return value)."""
    data = bytes(data)
    n = len(data)
    k = num_chunks(n)
    if k == 1:
        body = encode_chunk(data, n - 1, tables, stats)
        return (b"", NOT_COMPRESSIBLE) if body is None else (b"\x01" + body, 1 + len(body))
    cuts = split(data, k)
    table, payload, ptr = b"", b"", 1 + 8 * k
    for j in range(k):
        part = data[cuts[j]:cuts[j + 1]]
        body = encode_chunk(part, min(len(part), n - ptr), tables, stats)
        if body is None:
            if ptr + len(part) >= n:
                return b"", NOT_COMPRESSIBLE
            body = part
            if stats is not None:
                stats["raw"] = stats.get("raw", 0) + 1
        table += struct.pack("<ii", len(part), len(body))
        payload += body
        ptr += len(body)
    return bytes([k]) + table + payload, ptr


def last_run_margin(data, tables):
    """CheckEOB's margin (output_size - 16) - bytes written at the last run of a one-chunk segment, with the check
    switched off: below 1 the segment is not compressible."""
    stats = {}
    encode_chunk(bytes(data), len(data) - 1, tables, stats, check=False)
    return stats["margin"][0]


# ---------------------------------------------------------------------------------------------- the real functions
def ref_lib():
    U = bm.ref_lib()
    if U is not None and not getattr(U, "_qlfc_typed", False):
        U.bsc_coder_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        U._qlfc_typed = True
    return U


def ref_compress(data):
    """The real bsc_coder_compress(., ., n, 1, 3) -> (bytes, return value)."""
    U = ref_lib()
    src = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.zeros(len(src) + 4096, np.uint8)
    rc = U.bsc_coder_compress(src.ctypes.data, out.ctypes.data, len(src), 1, 3)
    return (out[:rc].tobytes() if rc > 0 else b""), rc


def ref_decompress(coded, n):
    U = ref_lib()
    src = np.frombuffer(bytes(coded), np.uint8).copy()
    out = np.zeros(n + 64, np.uint8)
    rc = U.bsc_coder_decompress(src.ctypes.data, out.ctypes.data, 1, 3)
    return out[:n].tobytes(), rc


# ---------------------------------------------------------------------------------------------- the case contents
def _letters(n, k, seed):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint8).tobytes()


def _mers(n, seed=11):
    """n bytes of 150-mers drawn from a genome a tenth as long: they overlap."""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, max(n // 10, 300))]
    reads = [g[s:s + 150] for s in rng.integers(0, len(g) - 150, n // 150 + 1)]
    return np.concatenate(reads)[:n].tobytes()


def _cycle(total, bump):
    """48 runs cycling over five letters, every run length a multiple of 32; bump: the first run one byte longer (and
    the last one shorter), which puts every run boundary on a sampled position."""
    lens = [total // 48 // 32 * 32] * 48
    lens[-1] = total - sum(lens[:-1])
    if bump:
        lens[0] += 1
        lens[-1] -= 1
    return b"".join(bytes([65 + r % 5]) * n for r, n in enumerate(lens))


def _strips(n):
    """n bytes in runs of 1000 over five letters: no run starts on a sampled position (1000 j = 1 mod 32 has no
    solution), so the chunk rule counts nothing and takes the equal split."""
    return (b"".join(bytes([65 + r % 5]) * 1000 for r in range(n // 1000 + 1)))[:n]


def _marked(n):
    """_strips(n) with a lone 'Z' on k + 1 sampled positions, the last of them the last sample there is,
    1 + 32 (ns - 1): one more than k, so the sampled cut is taken, and only because of the last sample."""
    k = num_chunks(n)
    last = 1 + 32 * ((n - 2) // 32)
    marks = [1 + 32 * (n * j // (k + 1) // 32) for j in range(1, k + 1)] + [last]
    a = bytearray(_strips(n))
    for p in marks:
        a[p] = 90
    return bytes(a)


def run_segment(count, seed, first):
    """A text of exactly `count` runs of 1 to 3 bytes over the four letters first .. first + 3, starting with `first`;
    a single run is 40 bytes long, so that it is coded."""
    rng = np.random.default_rng(seed)
    steps, lens = rng.integers(1, 4, count), rng.integers(1, 4, count) if count > 1 else [40]
    out, c = [], 0
    for r in range(count):
        out.append(bytes([first + c]) * int(lens[r]))
        c = (c + int(steps[r])) % 4
    return b"".join(out)


# Inputs found by tools/qlfc_edge_search.py, per pair of state tables ("real": libbsc's; else random_tables(seed)).
# pend: 3000 bytes over 9 letters, _letters(3000, 9, seed), whose coder flushes a pending unit without (n) and with (c)
# a carry.  eob: _letters(n, k, seed), one chunk, CheckEOB's margin at the last run 0 (n odd: not compressible by one
# comparison) and 1 (n even: coded by one unit).
SEARCHED = {
    "real": dict(pend_n=1004, pend_c=1994, eob_0=(1501, 114, 1000), eob_1=(1502, 68, 1003)),
    101: dict(pend_n=1209, pend_c=1269, eob_0=(1501, 67, 1000), eob_1=(1502, 67, 1000)),
    202: dict(pend_n=1032, pend_c=1220, eob_0=(1501, 67, 1001), eob_1=(1502, 67, 1001)),
}
ABSENT = {"no0": 0, "no127": 127, "no128": 128, "no255": 255}


def table_cases(which):
    """The names of the searched cases of one pair of tables."""
    return tuple("%s_%s" % (kind, which) for kind in ("pend_n", "pend_c", "eob_0", "eob_1"))


def _absent(c):
    """Eight shuffles of the 255 other bytes, in runs of one to three."""
    rng = np.random.default_rng(300 + c)
    rest = np.array([b for b in range(256) if b != c], np.uint8)
    return b"".join(bytes([int(b)]) * (1 + int(b) % 3) for _ in range(8) for b in rng.permutation(rest))


@functools.lru_cache(maxsize=None)
def case(name):
    rnd = lambda n, seed: np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if name.startswith(("pend_", "eob_")):
        kind, which = name.rsplit("_", 1)
        found = SEARCHED["real" if which == "real" else int(which)][kind]
        return _letters(3000, 9, found) if kind.startswith("pend") else _letters(*found)
    if name.startswith("esc"):
        return _letters(5000, int(name[3:]), 6)
    if name.startswith("eq"):
        return _strips(int(name[2:]))
    if name.startswith("smp"):
        return _marked(int(name[3:]))
    if name in ABSENT:
        return _absent(ABSENT[name])
    if name.startswith("len"):
        return rnd(int(name[3:]), 1)
    if name.startswith("letters"):
        return bytes(65 + b for b in _letters(5000, int(name[7:]), 2))
    if name.startswith("cycle"):   # cycle4 / cycle16, then e (equal split) or s (sampled cut)
        return _cycle(int(name[5:-1]) << 20, name[-1] == "s")
    return {
        "a40": lambda: b"A" * 40,
        "ab32": lambda: b"AB" * 32,
        "tail0": lambda: _letters(4999, 3, 3) + b"\0",
        "all256": lambda: bytes(range(256)) * 32,
        "all256runs": lambda: b"".join(bytes([c]) * (c % 7 + 1) for c in range(256)) * 8,
        "random4096": lambda: rnd(4096, 4),
        "exp16": lambda: b"A" * 3000 + b"C" + b"A" * 70000 + b"B" + b"G" * 40,
        "bwt5000": lambda: bm.bwt(_mers(5000))[0],
        "a300000": lambda: b"A" * 300000,
        "bwt300000": lambda: bm.bwt(_mers(300000))[0],
        "random_a": lambda: rnd(262144, 5) + b"A" * 262144,
        "a_random": lambda: b"A" * 262144 + rnd(262144, 5),
        "ring100": lambda: bytes(range(100)) * 50,
        "desc256": lambda: bytes(range(255, -1, -1)) + b"".join(bytes([c]) * (c % 7 + 1) for c in range(256)) * 4,
        "raw_coded": lambda: rnd(3000, 7) + b"A" * (262144 - 3000),
        "coded_raw": lambda: b"A" * (262144 - 2144) + rnd(2144, 8),
        "raw4": lambda: (rnd(2000, 9) + b"A" * (2 * MIB - 4000) + rnd(4000, 10) + b"C" * (2 * MIB - 4000) + rnd(2000, 12)),
        "random262144": lambda: rnd(262144, 13),
    }[name]()


SMALL = ("len1", "len2", "len16", "len17", "a40", "ab32", "letters1", "letters2", "letters3", "letters5", "letters9",
         "tail0", "all256", "all256runs", "random4096", "exp16", "bwt5000")
MODEL_CASES = SMALL + ("a300000", "bwt300000", "cycle4e", "cycle4s", "cycle16e", "cycle16s")
REF_ONLY_CASES = ("random_a", "a_random")     # about 3 * 10^6 events each: too slow for the Python model
# The branches the cases above do not reach, every one coded under the real tables and under
# random_tables(101) and (202); table_cases(which) adds what had to be searched for per pair of tables.
MIB = 1 << 20
CHUNK_SIZES = (262143, 262145, 262146, 4 * MIB - 1, 4 * MIB + 1)
ESCAPE_CASES = ("esc100", "esc128", "esc129", "ring100")
SYMBOL_CASES = ("letters4", "letters8", "no0", "no127", "no128", "no255", "desc256")
SPLIT_CASES = tuple("eq%d" % n for n in CHUNK_SIZES) + tuple("smp%d" % n for n in CHUNK_SIZES[1:])
RAW_CASES = ("raw_coded", "coded_raw", "raw4")
EDGE_CASES = ESCAPE_CASES + SYMBOL_CASES + SPLIT_CASES + RAW_CASES
ROLLBACK_CASE = "random262144"                # incompressible throughout: the real function only, as REF_ONLY_CASES

# Batches of one-chunk segments with exact run counts, so that chunk boundaries fall on the 256-run tiles of the rank
# pass (256, 512, 513, 768) and on the 64-run loads of the context walk.  Every segment has four letters of its own:
# the first byte of a segment is absent from the one before, which a rank pass that looked one run too far would list.
# The seeds of the 63- and 65-run segments (tools/qlfc_edge_search.py lanes) put the first event of the last run on
# the last and on the first lane of a 64-event load of the range coder.
RUN_ORDERS = ((256, 256, 1, 255, 512), (64, 64, 1, 63, 65, 128))
RUN_SEEDS = {63: 58, 65: 13}


def run_batch(counts):
    return [run_segment(c, RUN_SEEDS.get(c, 40 + j), 65 + 4 * j) for j, c in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def many_segments():
    """1500 segments of 40 to 200 random bytes over 2 to 4 letters, every hundredth one empty: more than 1024 chunks."""
    rng = np.random.default_rng(77)
    segs = []
    for j in range(1500):
        n, k = int(rng.integers(40, 201)), int(rng.integers(2, 5))
        segs.append(b"" if j % 100 == 99 else bytes((65 + rng.integers(0, k, n)).astype(np.uint8)))
    return tuple(segs)
