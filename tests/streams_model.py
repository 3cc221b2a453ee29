"""Checker for the per-block read streams (test infrastructure, not product).

write_streams  vectorised numpy restatement of the writer, reference src/reorder_compress_streams.cpp:76-362
read_block     restatement of the decompressor's reader of one block, reference src/decompress.cpp:223-321; pinned by
               the real decompress_short on blocks the real writer wrote (tests/test_models_vs_ref_decompress.py)

Stream names are the reference's file names (reorder_compress_streams.cpp:34-74).
"""
import numpy as np

STREAMS = ("read_flag.txt", "read_pos.bin", "read_noise.txt", "read_noisepos.bin", "read_rev.txt",
           "read_unaligned.txt", "read_lengths.bin", "read_pos_pair.bin", "read_rev_pair.txt")
ENCODER_FILES = ("read_pos.bin", "read_noise.txt", "read_noisepos.bin", "read_rev.txt", "read_order.bin",
                 "read_lengths.bin", "read_unaligned.txt", "read_unaligned.txt.count")
INT2DNA = np.frombuffer(b"AGCTN", np.uint8)   # read_dnaN_from_bits (util.cpp:350-374)


def stream_names(paired_end):
    return STREAMS if paired_end else STREAMS[:7]


def _runs(lens):
    """-> (run id, index inside the run) of every element of runs of the given lengths."""
    lens = np.asarray(lens, np.int64)
    tot = int(lens.sum())
    rid = np.repeat(np.arange(len(lens)), lens)
    first = np.cumsum(lens) - lens
    return rid, np.arange(tot, dtype=np.int64) - first[rid]


def _copy_runs(out, dst, src, src_off, lens):
    rid, j = _runs(lens)
    out[np.asarray(dst, np.int64)[rid] + j] = src[np.asarray(src_off, np.int64)[rid] + j]


def _put(out, off, vals, width):
    """little-endian `width`-byte values at byte offsets off."""
    v = np.asarray(vals).astype("<u%d" % width).view(np.uint8).reshape(-1, width)
    out[np.asarray(off, np.int64)[:, None] + np.arange(width)] = v


def unaligned_records(un, lens):
    """write_dnaN_in_bits records (u16 length + nibbles, A G C T N = 0..4) -> (record byte offsets, flat bases)."""
    un = np.frombuffer(bytes(un), np.uint8)
    lens = np.asarray(lens, np.int64)
    sz = 2 + (lens + 1) // 2
    roff = np.cumsum(sz) - sz
    assert int(sz.sum()) == len(un), "read_unaligned.txt does not match read_lengths.bin"
    if len(lens):
        assert np.array_equal(un[roff].astype(np.int64) | (un[roff + 1].astype(np.int64) << 8), lens)
    rid, c = _runs(lens)
    codes = (un[roff[rid] + 2 + c // 2] >> (4 * (c & 1)).astype(np.uint8)) & 15
    return roff, INT2DNA[codes]


def write_streams(enc, num_reads, paired_end, preserve_order, num_reads_per_block):
    """enc: the encoder's streams (pos, rc, noise, noisepos, order, rlen, unaligned as in EncoderStage.streams()).
    -> {stream name: (bytes of all blocks back to back, block offsets [num_blocks + 1])}."""
    N, pe, po, B = int(num_reads), bool(paired_end), bool(preserve_order), int(num_reads_per_block)
    pos = np.asarray(enc["pos"], np.uint64)
    na = len(pos)
    rc = np.frombuffer(bytes(enc["rc"]), np.uint8) if isinstance(enc["rc"], bytes) else np.asarray(enc["rc"], np.uint8)
    noise = np.frombuffer(bytes(enc["noise"]), np.uint8)
    noisepos = np.asarray(enc["noisepos"], np.uint16)
    rlen = np.asarray(enc["rlen"], np.uint16)
    assert len(rlen) == N and (not pe or N % 2 == 0) and B > 0
    # :112-137 the aligned records: one noise line each
    nl = np.flatnonzero(noise == 10)
    assert len(nl) == na and (na == 0 or nl[-1] == len(noise) - 1)
    nstart = np.concatenate([[0], nl[:-1] + 1]).astype(np.int64) if na else np.zeros(0, np.int64)
    ncnt = nl - nstart
    assert int(ncnt.sum()) == len(noisepos)
    # :143-171 the unaligned records, bases concatenated in record order
    ulen = rlen[na:].astype(np.int64)
    _, ubases = unaligned_records(enc["unaligned"], ulen)
    uoff = np.cumsum(ulen) - ulen
    # record k -> slot (:113-136, :163-170)
    slot = np.asarray(enc["order"], np.int64) if (pe or po) else np.arange(N, dtype=np.int64)
    assert len(slot) == N and np.array_equal(np.sort(slot), np.arange(N))
    k_of = np.empty(N, np.int64)
    k_of[slot] = np.arange(N)
    al = k_of < na
    ka = np.where(al, k_of, 0)
    ku = np.where(al, 0, k_of - na)
    s_len = rlen[k_of].astype(np.int64)
    s_pos = np.where(al, pos[ka] if na else 0, 0).astype(np.uint64)
    s_rc = np.where(al, rc[ka] if na else 0, 0).astype(np.uint8)
    s_ncnt = np.where(al, ncnt[ka] if na else 0, 0)
    s_nstart = np.where(al, nstart[ka] if na else 0, 0)
    s_npoff = s_nstart - ka
    s_uoff = np.where(al, 0, uoff[ku] if len(uoff) else 0)

    U = N // 2 if pe else N
    half = N // 2 if pe else 0
    u = np.arange(U, dtype=np.int64)
    r2 = half + u
    a1 = al[:U]
    # flags (:248-249, :279, :286-298)
    if pe:
        a2 = al[r2]
        d = s_pos[r2].astype(np.int64) - s_pos[u].astype(np.int64)
        flag = np.select([a1 & a2 & (np.abs(d) < 32767), a1 & a2, ~a1 & ~a2, a1 & ~a2], [0, 1, 2, 3], 4)
    else:
        a2 = np.zeros(U, bool)
        flag = np.where(a1, 0, 2)
    # read 1 position (:251-271, :309-329): prevpos = last aligned read 1 earlier in the block, 0 if none
    bstart = u - u % B
    last = np.maximum.accumulate(np.where(a1, u, -1)) if U else np.zeros(0, np.int64)
    prev = np.concatenate([[-1], last[:-1]]) if U else last
    prevpos = np.where(prev >= bstart, s_pos[np.maximum(prev, 0)], 0).astype(np.uint64)
    diff = s_pos[:U] - prevpos   # uint64: a decreasing position wraps and takes the escape
    absolute = po | (u == bstart)
    p1 = np.where(~a1, 0, np.where(absolute, 8, np.where(diff < 65535, 2, 10)))
    r2_pos = pe & ((flag == 1) | (flag == 4))
    sizes = {
        "read_pos.bin": p1 + 8 * r2_pos,
        "read_noise.txt": np.where(a1, s_ncnt[:U] + 1, 0) + (np.where(a2, s_ncnt[r2] + 1, 0) if pe else 0),
        "read_noisepos.bin": 2 * (np.where(a1, s_ncnt[:U], 0) + (np.where(a2, s_ncnt[r2], 0) if pe else 0)),
        "read_rev.txt": a1.astype(np.int64) + r2_pos,
        "read_unaligned.txt": np.where(a1, 0, s_len[:U]) + (np.where(a2, 0, s_len[r2]) if pe else 0),
        "read_flag.txt": np.ones(U, np.int64),
        "read_lengths.bin": np.full(U, 4 if pe else 2, np.int64),
    }
    if pe:
        sizes["read_pos_pair.bin"] = 2 * (flag == 0)
        sizes["read_rev_pair.txt"] = (flag == 0).astype(np.int64)
    off = {s: np.concatenate([[0], np.cumsum(z)]).astype(np.int64) for s, z in sizes.items()}
    out = {s: np.zeros(int(o[-1]), np.uint8) for s, o in off.items()}

    out["read_flag.txt"][:] = ord("0") + flag
    if pe:
        _put(out["read_lengths.bin"], 4 * u, s_len[:U], 2)
        _put(out["read_lengths.bin"], 4 * u + 2, s_len[r2], 2)
        f0 = np.flatnonzero(flag == 0)
        _put(out["read_pos_pair.bin"], off["read_pos_pair.bin"][f0], d[f0].astype(np.int16).view(np.uint16), 2)
        out["read_rev_pair.txt"][off["read_rev_pair.txt"][f0]] = np.where(s_rc[f0] != s_rc[r2[f0]], ord("0"), ord("1"))
    else:
        _put(out["read_lengths.bin"], 2 * u, s_len[:U], 2)
    o = off["read_pos.bin"][:U]
    sel = np.flatnonzero(p1 == 8)
    _put(out["read_pos.bin"], o[sel], s_pos[sel], 8)
    sel = np.flatnonzero(p1 == 2)
    _put(out["read_pos.bin"], o[sel], diff[sel], 2)
    sel = np.flatnonzero(p1 == 10)
    _put(out["read_pos.bin"], o[sel], np.full(len(sel), 65535), 2)
    _put(out["read_pos.bin"], o[sel] + 2, s_pos[sel], 8)
    sel = np.flatnonzero(r2_pos)
    _put(out["read_pos.bin"], o[sel] + p1[sel], s_pos[r2[sel]], 8)
    orv = off["read_rev.txt"][:U]
    sel = np.flatnonzero(a1)
    out["read_rev.txt"][orv[sel]] = s_rc[sel]
    sel = np.flatnonzero(r2_pos)
    out["read_rev.txt"][orv[sel] + a1[sel]] = s_rc[r2[sel]]
    # noise lines (with their '\n') and noise positions: read 1, then read 2 (:272-277, :330-335, :344-349)
    np16 = out["read_noisepos.bin"].view(np.uint16)
    on, onp = off["read_noise.txt"][:U], off["read_noisepos.bin"][:U] // 2
    sel = np.flatnonzero(a1)
    _copy_runs(out["read_noise.txt"], on[sel], noise, s_nstart[sel], s_ncnt[sel] + 1)
    _copy_runs(np16, onp[sel], noisepos, s_npoff[sel], s_ncnt[sel])
    if pe:
        sel = np.flatnonzero(a2)
        add = np.where(a1[sel], s_ncnt[sel] + 1, 0)
        _copy_runs(out["read_noise.txt"], on[sel] + add, noise, s_nstart[r2[sel]], s_ncnt[r2[sel]] + 1)
        _copy_runs(np16, onp[sel] + add - (add > 0), noisepos, s_npoff[r2[sel]], s_ncnt[r2[sel]])
    # unaligned reads as characters (:280, :339, :357-358)
    ou = off["read_unaligned.txt"][:U]
    sel = np.flatnonzero(~a1)
    _copy_runs(out["read_unaligned.txt"], ou[sel], ubases, s_uoff[sel], s_len[sel])
    if pe:
        sel = np.flatnonzero(~a2)
        add = np.where(a1[sel], 0, s_len[sel])
        _copy_runs(out["read_unaligned.txt"], ou[sel] + add, ubases, s_uoff[r2[sel]], s_len[r2[sel]])
    nb = (U + B - 1) // B
    bu = np.minimum(np.arange(nb + 1, dtype=np.int64) * B, U)
    return {s: (out[s].tobytes(), off[s][bu].astype(np.uint64)) for s in stream_names(pe)}


def stream_sizes(enc, num_reads, paired_end, preserve_order, num_reads_per_block):
    """Closed-form per-stream totals and block tables (no byte images): {stream: block offsets}."""
    return {s: t for s, (_, t) in write_streams(enc, num_reads, paired_end, preserve_order, num_reads_per_block).items()}


def blocks_of(streams):
    """{stream: (bytes, offsets)} -> {stream: [block bytes]}."""
    return {s: [d[int(o[b]):int(o[b + 1])] for b in range(len(o) - 1)] for s, (d, o) in streams.items()}


DEC_NOISE = {"A": "CGTN", "C": "AGTN", "G": "TACN", "T": "GCAN", "N": "AGCT"}  # decompress.cpp:664-684
_RC = str.maketrans("ACGTN", "TGCAN")


def read_block(blk, seq, num_units, paired_end, preserve_order):
    """decompress.cpp:223-321 for one block: blk = {stream name: bytes}, seq = consensus text.
    -> list of reads of the block's units (single-end) or of (read 1, read 2) tuples (paired-end).
    Compared with the reads the real decompress_short restores from the same blocks in
    tests/test_models_vs_ref_decompress.py.  The final assertion (every stream consumed exactly) is this reader's refusal
    of a block the reference cannot read either: without preserve_order, one that opens with an unaligned read 1 and holds
    an aligned read 1 later (the writer stores a u16 delta there, this reader takes a u64)."""
    flag = blk["read_flag.txt"].decode()
    lens = np.frombuffer(blk["read_lengths.bin"], np.uint16)
    posb, rcs, un = blk["read_pos.bin"], blk["read_rev.txt"].decode(), blk["read_unaligned.txt"].decode()
    noise = blk["read_noise.txt"].decode().split("\n")
    npos = np.frombuffer(blk["read_noisepos.bin"], np.uint16)
    pp = np.frombuffer(blk.get("read_pos_pair.bin", b""), np.int16)
    rp = blk.get("read_rev_pair.txt", b"").decode()
    ip = irc = iun = inl = inp = ipp = 0
    first = True
    prevpos = 0
    out = []

    def u64(p):
        return int.from_bytes(posb[p:p + 8], "little")

    def aligned(p, rl, c):
        nonlocal inl, inp
        r = list(seq[p:p + rl])
        prev = 0
        for ch in noise[inl]:
            prev += int(npos[inp])
            inp += 1
            r[prev] = DEC_NOISE[r[prev]][int(ch)]
        inl += 1
        s = "".join(r)
        return s if c == "d" else s.translate(_RC)[::-1]

    li = 0
    for i in range(num_units):
        f = flag[i]
        rl1 = int(lens[li])
        li += 1
        if f not in "24":
            if preserve_order:
                pos1 = u64(ip)
                ip += 8
            elif first:
                first = False
                pos1 = u64(ip)
                ip += 8
                prevpos = pos1
            else:
                dp = int.from_bytes(posb[ip:ip + 2], "little")
                ip += 2
                if dp == 65535:
                    pos1 = u64(ip)
                    ip += 8
                else:
                    pos1 = prevpos + dp
                prevpos = pos1
            rc1 = rcs[irc]
            irc += 1
            read1 = aligned(pos1, rl1, rc1)
        else:
            read1 = un[iun:iun + rl1]
            iun += rl1
        if not paired_end:
            out.append(read1)
            continue
        rl2 = int(lens[li])
        li += 1
        if f not in "23":
            if f in "14":
                pos2 = u64(ip)
                ip += 8
                rc2 = rcs[irc]
                irc += 1
            else:
                pos2 = pos1 + int(pp[ipp])
                ipp += 1
                rel = rp[ipp - 1]
                rc2 = ("r" if rc1 == "d" else "d") if rel == "0" else rc1
            read2 = aligned(pos2, rl2, rc2)
        else:
            read2 = un[iun:iun + rl2]
            iun += rl2
        out.append((read1, read2))
    assert ip == len(posb) and irc == len(rcs) and iun == len(un) and inp == len(npos) and li == len(lens)
    return out


def read_all(streams, seq, num_reads, paired_end, preserve_order, num_reads_per_block):
    """Every block through read_block -> reads in slot order (single-end) or [read 1 ...] + [read 2 ...] (paired)."""
    bl = blocks_of(streams)
    U = num_reads // 2 if paired_end else num_reads
    got = []
    for b in range(len(bl["read_flag.txt"])):
        nu = min(num_reads_per_block, U - b * num_reads_per_block)
        got += read_block({s: v[b] for s, v in bl.items()}, seq, nu, paired_end, preserve_order)
    if paired_end:
        return [p[0] for p in got] + [p[1] for p in got]
    return got


# ---------------------------------------------------------------- hand-built corner cases
def _pack_dnaN(reads):
    """write_dnaN_in_bits (util.cpp:322-348) records."""
    code = {c: i for i, c in enumerate("AGCTN")}
    out = bytearray()
    for r in reads:
        out += len(r).to_bytes(2, "little")
        for b in range(0, len(r), 2):
            v = code[r[b]] | ((code[r[b + 1]] << 4) if b + 1 < len(r) else 0)
            out.append(v)
    return bytes(out)


L_CORNER = 20
# slot contents: ("A", pos, rc) aligned (no noise), ("U", bases) unaligned
SE_CORNER = [("A", 100, "d"), ("A", 100 + 65534, "r"), ("A", 100 + 65534 + 65535, "d"), ("A", 50, "d"),
             ("A", 7, "r"), ("A", 70000, "d"), ("U", "ACGTNACGTNACGTNACGT"), ("U", "NNACGTTGCAACGTTGCAAC")]
PE_CORNER = [  # units (read 1, read 2); read 2 of unit u sits in slot len(units) + u
    (("A", 1000, "d"), ("A", 1000 + 32766, "r")),                 # flag 0, pos_pair 32766, orientations differ
    (("A", 66534, "d"), ("A", 66534 + 32767, "d")),               # flag 1 (|pos_pair| = 32767); gap 65534
    (("A", 132069, "r"), ("A", 132069 - 32766, "r")),             # flag 0, pos_pair -32766, same orientation; gap 65535
    (("U", "ACGTNACGTNACGTNACGTA"), ("A", 500, "d")),             # flag 4: block 1 starts with an unaligned read 1
    (("A", 40, "r"), ("U", "TTTTTNNNNNAAAAACCCC")),               # flag 3: delta against prevpos 0
    (("U", "GGGGGCCCCCAAAAATTTTT"), ("U", "ACGTN")),              # flag 2
    (("A", 10, "d"), ("A", 12, "r")),                             # block 2: absolute
    (("A", 5, "d"), ("A", 40005, "d")),                           # decreasing position -> escape; flag 1
]


def corner_case(paired_end, shuffle=True, seed=0):
    """Encoder streams with the slot contents above (aligned records, in a shuffled order if `shuffle`, then the
    unaligned ones).  -> (enc, seq, num_reads, reads in slot order)."""
    rng = np.random.default_rng(seed)
    slots = list(SE_CORNER) if not paired_end else [u[0] for u in PE_CORNER] + [u[1] for u in PE_CORNER]
    seq = "".join("ACGT"[x] for x in rng.integers(0, 4, 200000))
    al = [s for s in range(len(slots)) if slots[s][0] == "A"]
    un = [s for s in range(len(slots)) if slots[s][0] == "U"]
    if shuffle:
        al = [int(x) for x in rng.permutation(al)]
    order = np.array(al + un, np.uint32)
    enc = dict(pos=np.array([slots[s][1] for s in al], np.uint64), rc="".join(slots[s][2] for s in al).encode(), noise=b"\n" * len(al),
               noisepos=np.zeros(0, np.uint16), order=order,
               rlen=np.array([L_CORNER] * len(al) + [len(slots[s][1]) for s in un], np.uint16),
               unaligned=_pack_dnaN([slots[s][1] for s in un]))
    reads = []
    for s in slots:
        if s[0] == "U":
            reads.append(s[1])
        else:
            r = seq[s[1]:s[1] + L_CORNER]
            reads.append(r if s[2] == "d" else r.translate(_RC)[::-1])
    return enc, seq, len(slots), reads
