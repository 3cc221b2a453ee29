"""Hand-built inputs for the pins against the reference's own writers (test infrastructure, not product): encoder
images for reorder_compress_streams with the edges named in tests/test_models_vs_ref.py, and FASTQ line images for
reorder_compress_quality_id.  Everything is built here in Python; nothing is read from the reference."""
import functools

import numpy as np

import decode_cases as dc
import streams_model as sm

_RC = str.maketrans("ACGTN", "TGCAN")
SEQ_LEN = 400000
MOTIF = 4999   # the consensus repeats with this (prime) period, so that a fixture holding it stays small


def consensus(seed=0):
    rng = np.random.default_rng(seed)
    motif = "".join("ACGT"[x] for x in rng.integers(0, 4, MOTIF))
    return (motif * (SEQ_LEN // MOTIF + 1))[:SEQ_LEN]


def A(pos, rc="d", L=24, noise=()):
    """An aligned slot; noise = ((position in the read, code 0..3), ...) with ascending positions."""
    return ("A", int(pos), rc, int(L), tuple(noise))


def U(bases):
    return ("U", bases)


def full_noise(L, seed):
    rng = np.random.default_rng(seed)
    return tuple((p, int(rng.integers(0, 4))) for p in range(L))


def units(us):
    """Paired-end units (read 1, read 2) -> slots: read 2 of unit u sits in slot len(us) + u."""
    return [u[0] for u in us] + [u[1] for u in us]


def make_enc(slots, seq, shuffle, seed=0):
    """Encoder streams whose slot s holds slots[s]: the aligned records (in a shuffled order if `shuffle`, which needs
    a mode that reads read_order.bin), then the unaligned ones.  -> (enc, num_reads, reads in slot order)."""
    rng = np.random.default_rng(seed)
    al = [s for s in range(len(slots)) if slots[s][0] == "A"]
    un = [s for s in range(len(slots)) if slots[s][0] == "U"]
    if shuffle:
        al = [int(x) for x in rng.permutation(al)]
    lines, npos = [], []
    for s in al:
        _, _, _, L, noise = slots[s]
        assert all(0 <= p < L for p, _ in noise) and list(noise) == sorted(set(noise))
        lines.append("".join(str(c) for _, c in noise) + "\n")
        prev = 0
        for p, _ in noise:
            npos.append(p - prev)
            prev = p
    enc = dict(pos=np.array([slots[s][1] for s in al], np.uint64), rc="".join(slots[s][2] for s in al).encode(),
               noise="".join(lines).encode(), noisepos=np.array(npos, np.uint16), order=np.array(al + un, np.uint32),
               rlen=np.array([slots[s][3] for s in al] + [len(slots[s][1]) for s in un], np.uint16),
               unaligned=sm._pack_dnaN([slots[s][1] for s in un]))
    reads = [s[1] if s[0] == "U" else dc._apply(seq, s[1], s[3], s[2], s[4]) for s in slots]
    return enc, len(slots), reads


def _bases(n, seed):
    return "".join("ACGTN"[x] for x in np.random.default_rng(seed).integers(0, 5, n))


def escape_slots(name, seed=0):
    """decode_cases.escape_cases()[name] as slots, orientation and noise drawn from `seed`, two unaligned reads after."""
    rng = np.random.default_rng(seed)
    out = []
    for i, p in enumerate(dc.escape_cases()[name]):
        at = sorted(set(int(x) for x in rng.integers(0, 24, i % 3)))
        out.append(A(p, "dr"[int(rng.integers(0, 2))], 24, [(a, int(rng.integers(0, 4))) for a in at]))
    return out + [U("ACGTN" * 3), U("")]


# ---------------------------------------------------------------- single-end edges (aligned slots first: every mode)
def se_deltas():
    """read_pos.bin deltas of exactly 65534, 65535 and 65536 and a decreasing position; lengths 0 and 511, aligned and
    unaligned; a read without noise and reads whose noise fills them."""
    p = 1000
    s = [A(p, "d", 24, [(0, 1), (23, 3)])]
    for g, rc, L, noise in ((65534, "r", 24, ()), (65535, "d", 0, ()), (65536, "r", 511, full_noise(511, 1)),
                            (-150000, "d", 24, full_noise(24, 2)), (1, "r", 1, ((0, 2),)), (0, "d", 511, ())):
        p += g
        s.append(A(p, rc, L, noise))
    return s + [U(""), U(_bases(511, 3)), U("N"), U(_bases(20, 4))]


def se_all_aligned():
    return [A(100 + 37 * i, "dr"[i % 2], 10 + i, ((i % 10, i % 4),)) for i in range(7)]


def se_all_unaligned():
    return [U(_bases(n, n)) for n in (5, 0, 511, 1, 2, 30, 31)]


def se_mixed():
    """Aligned and unaligned slots interleaved: only for preserve_order, which reads read_order.bin."""
    s = se_deltas()
    return [s[i] for i in (7, 0, 8, 1, 2, 9, 3, 4, 10, 5, 6)]


# ---------------------------------------------------------------- paired-end edges
def pe_pairdist():
    """A pair distance of exactly +-32766, +-32767 and +-32768, mates of equal and of opposite orientation."""
    us = []
    for i, d in enumerate((32766, 32767, 32768, -32766, -32767, -32768, 32766, -32766, 0)):
        p1 = 60000 + 1013 * i
        rc1, rc2 = "dr"[i % 2], "dr"[(i // 2) % 2]
        us.append((A(p1, rc1, 24, ((3, i % 4),)), A(p1 + d, rc2, 24, ((0, 0), (5, (i + 1) % 4)))))
    return units(us)


def pe_flags():
    """The five flags in the sequence 4 0 3 1 2 0 2 4 1 3: each opens a block at B = 1, and 4, 3, 2, 1 / 4, 1, 2, 3 do at
    B = 2 / B = 3; lengths 0 and 511 on both mates, aligned and unaligned; both mates with noise, so that the order of
    the two noise lines shows; a mate without noise beside one whose noise fills it."""
    a = lambda p, rc="d", L=24, noise=((1, 1),): A(p, rc, L, noise)  # noqa: E731
    us = [
        (U(_bases(24, 5)), a(700, "r", 24, ((2, 3), (9, 0)))),                                   # 4
        (a(900, "d", 24, ((0, 2),)), a(905, "r", 24, ((4, 1), (5, 1), (23, 0)))),                # 0, opposite
        (a(100900, "r", 511, full_noise(511, 6)), U("")),                                        # 3
        (a(100000, "d", 0, ()), a(200000, "d", 511, ((510, 3),))),                               # 1
        (U(""), U(_bases(511, 7))),                                                              # 2
        (a(100001, "r", 24, ()), a(100001, "r", 24, full_noise(24, 8))),                         # 0, equal, distance 0
        (U("N"), U("ACGT")),                                                                     # 2
        (U(_bases(511, 9)), a(3, "d", 0, ())),                                                   # 4
        (a(250000, "d", 24, ((7, 0),)), a(250000 - 32767, "r", 24, ((7, 1),))),                  # 1
        (a(5, "r", 1, ((0, 3),)), U(_bases(3, 10))),                                             # 3
    ]
    return units(us)


def _pe_corner():
    """streams_model.PE_CORNER as units of this module's slots (no noise, length L_CORNER)."""
    conv = lambda x: U(x[1]) if x[0] == "U" else A(x[1], x[2], sm.L_CORNER)  # noqa: E731
    return [(conv(a), conv(b)) for a, b in sm.PE_CORNER]


def pe_all_aligned():
    return units([(A(200 + 11 * i, "dr"[i % 2], 20, ((i, 1),)), A(260 + 7 * i, "rd"[i % 2], 21, ((0, 2), (20, 0))))
                  for i in range(5)])


def pe_all_unaligned():
    return units([(U(_bases(3 * i, i)), U(_bases(40 - i, 20 + i))) for i in range(5)])


# name -> (slots, paired_end, may run without preserve_order)
STREAM_EDGES = {
    "se_deltas": (se_deltas, False, True), "se_all_aligned": (se_all_aligned, False, True),
    "se_all_unaligned": (se_all_unaligned, False, True), "se_mixed": (se_mixed, False, False),
    "pe_pairdist": (pe_pairdist, True, True), "pe_flags": (pe_flags, True, True),
    "pe_all_aligned": (pe_all_aligned, True, True), "pe_all_unaligned": (pe_all_unaligned, True, True),
}


# ---------------------------------------------------------------- quality and id lines
LENGTHS = (0, 1, 15, 16, 17, 31, 63, 64, 65, 255, 511)   # as tests/test_gpu_qualid.py
QUAL_ALPHABET = bytes(range(33, 127))
ID_FORMS = {
    # name -> (id of record i in file 1, in file 2, find_id_pattern of the pair)
    "illumina": (lambda i: b"@M01234:56:000000000-ABCDE:1:%d:%d:%d 1:N:0:ACGT" % (1101 + i // 100, 1000 + 7 * i, 2000 + i),
                 lambda i: b"@M01234:56:000000000-ABCDE:1:%d:%d:%d 2:N:0:ACGT" % (1101 + i // 100, 1000 + 7 * i, 2000 + i), 3),
    "srr": (lambda i: b"@SRR1234567.%d %d/1" % (i + 1, i + 1), lambda i: b"@SRR1234567.%d %d/2" % (i + 1, i + 1), 1),
    "r": (lambda i: b"@r.%d" % i, lambda i: b"@r.%d" % i, 2),
}


def qualid_lines(n, form, mate=0, compressible=False):
    """-> (ids, qualities) of n records, CR-free: quality lengths cycle through LENGTHS (file 2 starts elsewhere in the
    cycle) and use every byte 33..126; `compressible` draws the qualities as windows of the repeated alphabet (a fixture
    holding them stays small) instead of at random."""
    rng = np.random.default_rng(17 + mate)
    ids, quals = [], []
    rep = QUAL_ALPHABET * 7
    for i in range(n):
        L = LENGTHS[(i + 3 * mate) % len(LENGTHS)]
        ids.append(ID_FORMS[form][mate](i))
        if compressible:
            s = (i * 7) % 94
            quals.append(rep[s:s + L])
        else:
            quals.append(np.frombuffer(QUAL_ALPHABET, np.uint8)[rng.integers(0, 94, L)].tobytes())
    assert n < 110 or set(b"".join(quals)) == set(QUAL_ALPHABET)
    return ids, quals


def image(lines):
    return b"".join(x + b"\n" for x in lines)


def order_of(which, num_reads):
    if which == "identity":
        return np.arange(num_reads, dtype=np.uint32)
    if which == "reversed":
        return np.arange(num_reads, dtype=np.uint32)[::-1].copy()
    return np.random.default_rng(num_reads).permutation(num_reads).astype(np.uint32)


# ---------------------------------------------------------------- fixtures written by the reference (tests/golden)
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# case -> (slots, paired_end, preserve_order, B); recorded by tests/golden/make_ref_golden.py
STREAM_FIXTURES = {
    "pe_corner_B3": (lambda: units(_pe_corner()), True, False, 3),
    "pe_corner_B8": (lambda: units(_pe_corner()), True, False, 8),
    "se_gaps_B3": (lambda: escape_slots("gaps"), False, False, 3),
    "se_decreasing_B3": (lambda: escape_slots("decreasing"), False, False, 3),
    "pe_pairdist_B4": (pe_pairdist, True, False, 4),
    "pe_flags_B3": (pe_flags, True, False, 3),
    "pe_flags_po_B3": (pe_flags, True, True, 3),
    "se_deltas_B3": (se_deltas, False, False, 3),
    "se_mixed_po_B3": (se_mixed, False, True, 3),
}
QUALID_FIXTURES = {"se_B7": ("srr", False, 7), "pe_B7": ("illumina", True, 7)}   # case -> (id form, paired_end, B)
ENC_KEYS = ("pos", "rc", "noise", "noisepos", "order", "rlen", "unaligned")


def stream_fixture_inputs(case):
    make, pe, preserve_order, B = STREAM_FIXTURES[case]
    seq = consensus()
    enc, N, reads = make_enc(make(), seq, shuffle=pe or preserve_order)
    return enc, seq, N, reads, pe, preserve_order, B


def load_stream_fixture(case):
    """-> dict(enc, seq, reads, N, pe, preserve_order, B, streams = {name: (bytes, block offsets)}), all from the file."""
    z = np.load(os.path.join(GOLDEN, "ref_streams_%s.npz" % case))
    enc = {k: z[k] for k in ENC_KEYS}
    for k in ("rc", "noise", "unaligned"):
        enc[k] = enc[k].tobytes()
    pe = bool(z["paired_end"])
    return dict(enc=enc, seq=z["seq"].tobytes().decode(), reads=z["reads"].tobytes().decode().split("\n"),
                N=int(z["num_reads"]), pe=pe, preserve_order=bool(z["preserve_order"]), B=int(z["num_reads_per_block"]),
                streams={s: (z[s].tobytes(), z[s + ".off"]) for s in sm.stream_names(pe)})


def qualid_fixture_inputs(case):
    form, pe, B = QUALID_FIXTURES[case]
    files = {}
    for m in range(2 if pe else 1):
        ids, quals = qualid_lines(330, form, m, compressible=True)
        files["quality_%d" % (m + 1)] = quals
        files["id_%d" % (m + 1)] = ids
    n = 330 * (2 if pe else 1)
    return files, order_of("random", n), n, pe, B


def load_qualid_fixture(case):
    """-> dict(files = {name: line image}, order, N, pe, B, want = {(name, table): dict(bytes, len, block_off, max_len)})
    with table in ("none", "illumina") for the quality files and "none" for the id files."""
    z = np.load(os.path.join(GOLDEN, "ref_qualid_%s.npz" % case))
    pe = bool(z["paired_end"])
    names = [k + "_%d" % (m + 1) for m in range(2 if pe else 1) for k in ("quality", "id")]
    want = {}
    for name in names:
        for table in (("none", "illumina") if name.startswith("quality") else ("none",)):
            key = name + ("" if table == "none" else ".illumina")
            ln = z[key + ".len"]
            want[(name, table)] = dict(bytes=z[key + ".bytes"].tobytes(), len=ln, block_off=z[key + ".off"],
                                       max_len=int(ln.max()) if len(ln) else 0)
    return dict(files={name: z[name].tobytes() for name in names}, order=z["order"], N=int(z["num_reads"]), pe=pe,
                B=int(z["num_reads_per_block"]), want=want)


# ---------------------------------------------------------------- the real decompressor (oracle/_ref/ref_decompress)
def pe_singleton_open():
    """Blocks whose first read 1 is unaligned and whose later read 1s are too (decompress.cpp:240-250 never reads a u64
    for read 1 there): at B = 3 the flags 4 2 4 | 0 1 3 | 2 4 2 | 1; read 2 of the flag-4 units aligned, so read_pos.bin
    of such a block holds read 2 positions only."""
    a = lambda p, rc="d", L=24, noise=((1, 1),): A(p, rc, L, noise)  # noqa: E731
    us = [
        (U(_bases(24, 31)), a(3000, "r")), (U("N"), U(_bases(9, 32))), (U(_bases(511, 33)), a(90000, "d", 511, ((0, 3), (510, 0)))),
        (a(500, "d"), a(520, "r", 24, ())), (a(70000, "r", 24, full_noise(24, 34)), a(170000, "d")), (a(70010, "d", 0, ()), U(_bases(24, 35))),
        (U(""), U("")), (U(_bases(30, 36)), a(7, "d", 1, ((0, 2),))), (U("ACGTN"), U("NNNN")),
        (a(12, "r"), a(300000, "r", 24, ((23, 1),))),
    ]
    return units(us)


@functools.lru_cache(maxsize=8)
def seq_pieces(seq, T):
    """The consensus text cut into T encoder threads -> [(2-bit packed bytes, tail text)]: read_seq.bin.<t> / .tail as
    pack_compress_seq leaves them before BSC_compress (encoder.cpp:111-156; test_unpack_seq_format pins the format)."""
    from test_gpu_decode import pack_seq
    lens, pk, tl = pack_seq(seq, T)
    cut = np.concatenate([[0], np.cumsum(lens // 4)]).astype(int)
    return [(pk[cut[t]:cut[t + 1]], tl[t]) for t in range(T)]


def quality_for(reads, mate=0):
    """A quality line per read, of the read's length (BSC_str_array_decompress takes the lengths from read_lengths.bin):
    windows of the repeated alphabet 33..126, so that a fixture holding them stays small."""
    rep = QUAL_ALPHABET * 7
    return [rep[(7 * i + 13 * mate) % 94:][:len(r)] for i, r in enumerate(reads)]


TWO_SPACES = (lambda i: b"@M:%d 1:N:0 1" % i, lambda i: b"@M:%d 2:N:0 1" % i, 3)   # modify_id: the FIRST space counts


def ids_for(form, n, mate=0):
    f = TWO_SPACES if form == "two_spaces" else ID_FORMS[form]
    return [f[mate](i) for i in range(n)]


def consumed_blocks(units_, B, num_thr, a, b):
    """The blocks decompress_short opens for the range [a, b) (decompress.cpp:122-138, :402-423): it starts with the
    block that holds unit a, takes num_thr blocks per step, and stops after the step that reaches unit b."""
    first = a // B
    done, blk, out = first * B, first, []
    per_step = min(num_thr * B, units_)
    while True:
        cur = min(per_step, units_ - done)
        if cur == 0:
            break
        out += [blk + t for t in range(num_thr) if t * B < cur]
        if done + cur >= b:
            break
        done += cur
        blk += num_thr
    return out


# case -> (slots, paired_end, preserve_order, B, encoder threads, id source, quality, ((start, end, num_thr), ...))
# id source: a form of ID_FORMS read from both files; (form, code) = paired_id_match, file 2's ids by modify_id; None =
# preserve_id off, numbered ids.  Recorded by tests/golden/make_ref_golden.py as ref_decomp_<case>.npz.  Block sizes,
# quality and thread counts are chosen so that no record shows the reference's stale quality line behind an empty read
# at the end of a block (the kept divergence of tests/test_models_vs_ref_decompress.py); the maker asserts it.
DECOMP_FIXTURES = {
    "se_deltas_B3": (se_deltas, False, False, 3, 3, "srr", True, ((0, 11, 1), (4, 9, 1), (0, 11, 3))),
    "pe_flags_po_noqual_B3_code3": (pe_flags, True, True, 3, 1, ("two_spaces", 3), False, ((0, 10, 3), (2, 10, 3), (5, 6, 1))),
    "pe_singleton_numbered_B3": (pe_singleton_open, True, False, 3, 2, None, True, ((0, 10, 3), (5, 10, 3), (8, 10, 1))),
    "se_mixed_po_noqual_B4": (se_mixed, False, True, 4, 1, "r", False, ((0, 11, 3), (3, 4, 1), (4, 8, 1))),
    "pe_pairdist_B4_code1": (pe_pairdist, True, False, 4, 3, ("srr", 1), True, ((0, 9, 1), (3, 9, 3))),
    "pe_corner_po_B3_code2": (lambda: units(_pe_corner()), True, True, 3, 1, ("r", 2), True, ((0, 8, 1), (1, 7, 3))),
    "pe_pairdist_po_B4_id2": (pe_pairdist, True, True, 4, 1, "illumina", True, ((0, 9, 3), (4, 8, 1))),
}


def decomp_fixture_inputs(case):
    """-> dict(enc, seq, N, reads, pe, preserve_order, B, T, ids = [file 1, file 2] or None, quality = [...] or None,
    code = paired id code or None, ranges)."""
    make, pe, preserve_order, B, T, idsrc, quality, ranges = DECOMP_FIXTURES[case]
    seq = consensus()
    enc, N, reads = make_enc(make(), seq, shuffle=pe or preserve_order)
    n = N // 2 if pe else N
    nf = 2 if pe else 1
    form, code = idsrc if isinstance(idsrc, tuple) else (idsrc, None)
    ids = None if form is None else [ids_for(form, n, m) for m in range(nf)]
    quals = [quality_for(reads[m * n:(m + 1) * n], m) for m in range(nf)] if quality else None
    return dict(enc=enc, seq=seq, N=N, reads=reads, pe=pe, preserve_order=preserve_order, B=B, T=T, ids=ids, quality=quals,
                code=code, ranges=ranges)


def load_decomp_fixture(case):
    """-> dict(seq, N, pe, preserve_order, B, streams = {name: (bytes, block offsets)}, ids / quality = [lines of file 1,
    of file 2] or None, code, ranges, text = {(start, end, num_thr): [file 1's text, file 2's]}), all from the file."""
    z = np.load(os.path.join(GOLDEN, "ref_decomp_%s.npz" % case))
    pe = bool(z["paired_end"])
    nf = 2 if pe else 1
    lines = lambda k: z[k].tobytes().split(b"\n")[:-1]  # noqa: E731
    ranges = [tuple(int(x) for x in r) for r in z["ranges"]]
    return dict(seq=z["seq"].tobytes().decode(), N=int(z["num_reads"]), pe=pe, preserve_order=bool(z["preserve_order"]),
                B=int(z["num_reads_per_block"]), streams={s: (z[s].tobytes(), z[s + ".off"]) for s in sm.stream_names(pe)},
                ids=[lines("id_%d" % (m + 1)) for m in range(nf)] if "id_1" in z else None,
                quality=[lines("quality_%d" % (m + 1)) for m in range(nf)] if "quality_1" in z else None,
                code=int(z["paired_id_code"]) or None, ranges=ranges,
                text={r: [z["text_%d.%d" % (m + 1, k)].tobytes() for m in range(nf)] for k, r in enumerate(ranges)})
