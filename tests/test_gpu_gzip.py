"""GPU tests of the gzip stage (include/spring_gzip.h).  The checker is zlib itself: every member, sliced by the member
offsets, is inflated on its own with zlib.decompressobj(31), which verifies CRC-32 and ISIZE and fails with "invalid
distance too far back" on a match that reaches before its member; what comes out must be the member's slice of the
input.  Sizes are held against the bound of the header, ratios against zlib level 1."""
import functools
import gzip
import hashlib
import os
import types
import zlib

import numpy as np
import pytest

import fastq_out_model as fm
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 31, 63, 64, 65, 255, 511)
N_REC = 3003   # 273 cycles of LENGTHS
QUAL_BYTES = np.array([c for c in range(1, 256) if c not in (10, 13)], np.uint8)
ID_BYTES = np.array([c for c in range(32, 127)], np.uint8)
HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255])


@functools.lru_cache(maxsize=None)
def synth(seed, n=N_REC):
    """(ids, reads, quals) of n records (the generator of test_gpu_fastq_out.synth): read lengths cycle through
    LENGTHS, ids of 1 .. 1200 bytes with some of exactly 15, 16, 31 and 32."""
    rng = np.random.default_rng(seed)
    ids, reads, quals = [], [], []
    for i in range(n):
        L = LENGTHS[(i + 3 * seed) % len(LENGTHS)]
        il = {4: 15, 5: 16, 6: 32, 7: 31}.get(i % 97, 1 + (i * 7919 + seed) % 1200)
        ids.append(b"@" + ID_BYTES[rng.integers(0, len(ID_BYTES), il - 1)].tobytes())
        reads.append(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)].tobytes())
        quals.append(QUAL_BYTES[rng.integers(0, len(QUAL_BYTES), L)].tobytes())
    return ids, reads, quals


def stored_bound(info, cuts):
    """bytes_in + 18 * members + 5 * sum over chunks of ceil(chunk_len / 65535)."""
    cb = info["chunk_bytes"]
    blocks = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        n = int(b) - int(a)
        full, rest = divmod(n, cb)
        blocks += full * -(-cb // 65535) + (-(-rest // 65535) if rest else 0)
    return int(cuts[-1]) + 18 * (len(cuts) - 1) + 5 * blocks


def num_chunks(info, cuts):
    return sum(-(-(int(b) - int(a)) // info["chunk_bytes"]) for a, b in zip(cuts[:-1], cuts[1:]))


def check(gs, data, cuts=None, what=""):
    """The result in gs against the input: every member alone, the headers, the trailers, the counts, the bound."""
    data = bytes(data)
    if cuts is None:
        cuts = [0, len(data)] if data else [0]
    cuts = [int(x) for x in cuts]
    gz, off = gs.download()
    info = gs.info
    assert info["num_members"] == len(cuts) - 1 == len(off) - 1, what
    assert info["bytes_in"] == len(data) and info["bytes_out"] == len(gz) == int(off[-1]) and int(off[0]) == 0, what
    for m in range(len(cuts) - 1):
        member, part = gz[int(off[m]):int(off[m + 1])], data[cuts[m]:cuts[m + 1]]
        assert member[:10] == HEADER, (what, m)
        assert member[-8:] == zlib.crc32(part).to_bytes(4, "little") + (len(part) & 0xffffffff).to_bytes(4, "little"), (what, m)
        d = zlib.decompressobj(31)
        out = d.decompress(member)
        assert d.eof and d.unused_data == b"" and out == part, (what, m)
    if data:
        assert gzip.decompress(gz) == data, what
        assert info["num_chunks"] == num_chunks(info, cuts) and info["chunks_stored"] <= info["num_chunks"], what
        assert len(gz) <= stored_bound(info, cuts), what
    else:
        assert gz == b"" and info["num_chunks"] == 0
    return gz, off


def record_cuts(rec_off, R):
    n = len(rec_off) - 1
    if n == 0:
        return [0]
    idx = list(range(0, n, R if R else n)) + [n]
    return [int(rec_off[i]) for i in idx]


# ---------------------------------------------------------------- 1. the assembler's text
@pytest.mark.parametrize("quality", [False, True])
def test_assembler_text(quality):
    from spring_amd import FastqOutStage, GzipStage
    ids, reads, quals = synth(1)
    with FastqOutStage() as fo, GzipStage() as gs, GzipStage() as gh:
        fo.assemble(fm.reads_image(reads), N_REC, quality=b"".join(quals) if quality else None, ids=fm.id_image(ids),
                    num_reads_per_block=1000)
        text, rec_off = fo.download()
        assert (text, rec_off.tolist()) == (lambda w: (w[0], w[1].tolist()))(fm.assemble(ids, reads, quals if quality else None))
        for R in (0, 1, 7, 1000, 3003, 3004):
            cuts = record_cuts(rec_off, R)
            assert len(cuts) - 1 == (1 if R in (0, 3003, 3004) else -(-N_REC // R))
            info = gs.compress(fo, member_records=R)
            gz, off = check(gs, text, cuts, (quality, R))
            assert info["ms_device"] > 0
            # the same text and cuts from the host, and a second run
            gh.compress(text, member_off=cuts)
            assert gh.download()[0] == gz and gh.download()[1].tolist() == off.tolist(), (quality, R, "host")
            gs.compress(fo, member_records=R)
            assert gs.download()[0] == gz, (quality, R, "second run")
            # stored blocks only: the bound is met exactly
            info = gs.compress(fo, member_records=R, mode=0)
            check(gs, text, cuts, (quality, R, "stored"))
            assert info["bytes_out"] == stored_bound(info, cuts) and info["chunks_stored"] == info["num_chunks"]
        assert fo.download()[0] == text   # the assembler's context is as it was


# ---------------------------------------------------------------- 2. chunk and member edges
def test_chunk_and_member_edges():
    from spring_amd import GzipStage
    rng = np.random.default_rng(2)
    with GzipStage() as gs:
        gs.compress(b"x")
        cb = gs.info["chunk_bytes"]
        # half text-like, half repeats, so that coded chunks and matches across the chunk edge both occur
        pool = (b"".join(b"@r.%d ACGTTGCA%d\n" % (i, i * i) for i in range(9000)))[:2 * cb + 1]
        assert len(pool) == 2 * cb + 1
        for k in (0, 1, 2):
            for d in (-1, 0, 1):
                n = cb * k + d
                if n <= 0:
                    continue
                for mode in (0, 1):
                    gs.compress(pool[:n], mode=mode)
                    check(gs, pool[:n], None, (k, d, mode))
                    assert gs.info["num_chunks"] == -(-n // cb)
        for n in (1, 2, 3):
            for data in (pool[:n], b"\x00" * n, bytes(rng.integers(0, 256, n, dtype=np.uint8))):
                gs.compress(data)
                check(gs, data, None, ("tiny", n))
        # a stored chunk whose last bytes lie in the source's partial last word; outputs of 16 k + 12, + 1 and + 15 bytes
        for n, rest in ((4096 + 5, 12), (4096 + 10, 1), (4096 + 8, 15)):
            info = gs.compress(pool[:n], mode=0)
            check(gs, pool[:n], None, ("stored, partial words", n))
            assert info["chunks_stored"] == 1 and info["bytes_out"] == n + 23 and info["bytes_out"] % 16 == rest
        # members of exactly one byte
        data = pool[:40]
        gs.compress(data, member_off=list(range(41)))
        check(gs, data, list(range(41)), "one byte each")
        gs.compress(pool[:cb + 7], member_off=[0, 1, cb + 6, cb + 7])
        check(gs, pool[:cb + 7], [0, 1, cb + 6, cb + 7], "one byte at both ends")
        # a member cut one byte before and one byte after a chunk edge
        for cut in (cb - 1, cb + 1, cb):
            cuts = [0, cut, 2 * cb + 1]
            gs.compress(pool, member_off=cuts)
            check(gs, pool, cuts, ("cut", cut))
        # an empty input
        info = gs.compress(b"")
        assert info["num_members"] == 0 and info["bytes_out"] == 0 and gs.download()[0] == b""
        assert gs.download()[1].tolist() == [0]
        gs.compress(b"", member_off=[0])
        check(gs, b"", [0], "empty with cuts")


# ---------------------------------------------------------------- 3. every length and distance code
DIST_ENDS = [1, 2, 3, 4] + [x for e in range(1, 14) for b in (2 ** (e + 1) + 1, 2 ** (e + 1) + 2 ** e + 1)
                            for x in (b, b + 2 ** e - 1)]


def test_every_length_and_distance_code():
    from spring_amd import GzipStage
    assert DIST_ENDS[:8] == [1, 2, 3, 4, 5, 6, 7, 8] and DIST_ENDS[-1] == 32768 and len(set(DIST_ENDS)) == 4 + 2 * 26
    rng = np.random.default_rng(3)
    parts = []
    for L in range(3, 301):   # runs of every length between distinct separators
        parts.append(bytes([97 + L % 26]) * L + b"|%d|" % L)
    for i, d in enumerate(sorted(set(DIST_ENDS)) + [32769]):   # a repeat at exactly this distance
        if d < 9:
            parts.append(bytes(rng.integers(0, 256, d, dtype=np.uint8)) * 24 + b"<%d>" % d)
        else:
            mark = b"[%06d]" % (i * 7919)
            parts.append(mark + bytes([i]) * (d - 8) + mark + b"<%d>" % d)
    for P in (1, 2, 3, 257, 258, 259, 32767, 32768, 32769):   # three periods each
        parts.append(bytes(rng.integers(0, 256, P, dtype=np.uint8)) * 3 + b"{%d}" % P)
    data = b"".join(parts)
    with GzipStage() as gs:
        info = gs.compress(data)
        check(gs, data)
        # What cannot be matched is random: the first period of every unit, and all three periods of 32769 (a distance
        # deflate does not have).  Everything else repeats: runs and fillers go at 258 bytes per match of at most 6
        # bytes, the short runs at a literal, a match and a separator each; 5 % covers both with the block headers.
        # Without the repeats at 32767 and 32768 the output is 131 KB above this.
        periods = (1, 2, 3, 257, 258, 259, 32767, 32768, 32769)
        noise = sum(periods) + 2 * 32769
        assert info["bytes_out"] < 1.001 * noise + 0.05 * (len(data) - noise)
        half = len(data) // 2
        gs.compress(data, member_off=[0, half, len(data)])
        check(gs, data, [0, half, len(data)], "two members")


# ---------------------------------------------------------------- 4. code construction
def fib_buffer(nsym, total, seed):
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    scale = min(1.0, total / sum(f))
    counts = [max(1, int(x * scale)) for x in f]
    a = np.repeat(np.arange(1, nsym + 1, dtype=np.uint8), counts)
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes(), counts


def test_code_construction():
    from spring_amd import GzipStage
    rng = np.random.default_rng(4)
    with GzipStage() as gs:
        gs.compress(b"x")
        cb = gs.info["chunk_bytes"]
        cases = {"one byte": b"a", "one value": b"a" * 100000, "two values": bytes(rng.integers(0, 2, 5000, dtype=np.uint8) + 65),
                 "two values, no match": b"ab", "256 values": bytes(range(256)),
                 "256 values, shuffled": bytes(rng.permutation(np.arange(256, dtype=np.uint8).repeat(8)))}
        fib22, counts = fib_buffer(22, 1 << 30, 5)
        assert len(fib22) == 46367 and counts[-1] == 17711
        cases["fibonacci 22"] = fib22
        fib30, counts30 = fib_buffer(30, cb - 64, 6)
        assert len(fib30) <= cb and len(set(fib30)) == 30
        cases["fibonacci 30 in one chunk"] = fib30
        for what, data in cases.items():
            gs.compress(data)
            check(gs, data, None, what)
        gs.compress(fib30)
        assert gs.info["num_chunks"] == 1 and gs.info["chunks_stored"] == 0 and gs.info["bytes_out"] < len(fib30) // 2


# ---------------------------------------------------------------- 5. it compresses
def fastq_shaped(n=20000):
    rng = np.random.default_rng(5)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 50000)]
    qtab = [bytes(rng.choice(np.frombuffer(b"FFFFFFFF:,#IIJJ?A<", np.uint8), 100)) for _ in range(64)]
    starts = rng.integers(0, 50000 - 100, n)
    which = rng.integers(0, 64, n)
    return b"".join(b"@SRR1234567.%d %d length=100\n%s\n+\n%s\n" % (i + 1, i + 1, genome[s:s + 100].tobytes(), qtab[w])
                    for i, (s, w) in enumerate(zip(starts.tolist(), which.tolist())))


def test_it_compresses():
    from spring_amd import GzipStage
    rng = np.random.default_rng(55)
    block = bytes(rng.integers(0, 64, 1000, dtype=np.uint8) + 32)
    repeated = (block * 1049)[:1 << 20]
    sixteen = bytes(rng.integers(0, 16, 1 << 20, dtype=np.uint8) + 65)
    golden = open(os.path.join(GOLDEN, "test_1.fastq"), "rb").read()
    shaped = fastq_shaped()
    with GzipStage() as gs:
        for what, data, bound in (("repeated block", repeated, 0.5 * len(repeated)),
                                  ("16 symbols", sixteen, 0.65 * len(sixteen)),
                                  ("golden test_1.fastq", golden, 1.10 * len(zlib.compress(golden, 1))),
                                  ("fastq-shaped", shaped, 1.10 * len(zlib.compress(shaped, 1)))):
            info = gs.compress(data)
            print("%s: %d -> %d (%.4f), zlib level 1 %.4f, bound %.4f" % (
                what, len(data), info["bytes_out"], info["bytes_out"] / len(data), len(zlib.compress(data, 1)) / len(data),
                bound / len(data)))
            check(gs, data, None, what)
            assert info["bytes_out"] < bound if what in ("repeated block", "16 symbols") else info["bytes_out"] <= bound, what


# ---------------------------------------------------------------- 6. incompressible input
def test_incompressible_input():
    from spring_amd import GzipStage
    data = np.random.default_rng(6).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    with GzipStage() as gs:
        info = gs.compress(data)
        check(gs, data)
        assert info["chunks_stored"] == info["num_chunks"] > 0
        assert info["bytes_out"] == stored_bound(info, [0, len(data)])


# ---------------------------------------------------------------- 7. size and CRC combination
TR = bytes.maketrans(b"ACGTN", b"I5#?!")


def test_two_hundred_thousand_reads():
    from spring_amd import FastqOutStage, GzipStage
    n, L = 200_000, 150
    rng = np.random.default_rng(150)
    base = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1 << 20, dtype=np.uint8)]
    bb = np.lib.stride_tricks.sliding_window_view(base, L)[rng.integers(0, (1 << 20) - L, n)].tobytes()
    with FastqOutStage() as fo, GzipStage() as gs:
        fo.assemble((bb, np.arange(n + 1, dtype=np.uint64) * np.uint64(L)), n, quality=bb.translate(TR),
                    ids=fm.id_image([b"@r.%d" % i for i in range(n)]))
        text, rec_off = fo.download()
        want = hashlib.blake2b(text).digest()
        assert len(text) > 60_000_000
        for R in (0, 4096):
            info = gs.compress(fo, member_records=R)
            gz, off = gs.download()
            print("200k x 150, member_records %d: %d -> %d, ms_device %.2f, passes %s" % (
                R, len(text), len(gz), info["ms_device"], ["%.2f" % x for x in info["ms_pass"]]))
            cuts = record_cuts(rec_off, R)
            assert info["num_members"] == len(cuts) - 1 == len(off) - 1 and len(gz) <= stored_bound(info, cuts)
            assert hashlib.blake2b(gzip.decompress(gz)).digest() == want
            for m in sorted({0, (len(cuts) - 1) // 2, len(cuts) - 2}):   # members alone: their CRC-32 joins their chunks'
                d = zlib.decompressobj(31)
                assert d.decompress(gz[int(off[m]):int(off[m + 1])]) == text[cuts[m]:cuts[m + 1]] and d.eof


# ---------------------------------------------------------------- 8. the chain
B_CHAIN = 97


def _fastq(ids, reads):
    return b"".join(b"%s\n%s\n+\n%s\n" % (i, r, r.translate(TR)) for i, r in zip(ids, reads))


def _golden(j):
    """The golden file's reads under ids that match by paired id code 1 (as test_gpu_fastq_out has them)."""
    lines = open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb").read().split(b"\n")
    reads = [x.strip() for x in lines[1:-1:4]]
    return _fastq([b"@pair.%d/%d" % (i, j) for i in range(len(reads))], reads)


@pytest.fixture(scope="module")
def chain():
    """FASTQ -> reorder -> encoder -> streams -> decode, and the quality / id blocks of both files, under preserve_order
    (the chain of test_gpu_fastq_out)."""
    import spring_amd
    from spring_amd import DecodeStage, QualIdStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    f = [_golden(1), _golden(2)]
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=2, alternatives=1, phases=1)) as st:
        info = st.load_fastq(f[0], f[1])
        N = sum(info["num_reads"])
        st.run()
        dnaN, order_N = st.fastq_N(0)
        d2, o2 = st.fastq_N(1)
        dnaN, order_N = dnaN + d2, np.concatenate([order_N, o2 + info["num_reads"][0]]).astype(np.uint32)
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds, QualIdStage() as q0, QualIdStage() as q1:
            enc.encode(st, dnaN, order_N)
            ss.from_encoder(enc, N, True, True, B_CHAIN)
            ds.seq_from_encoder(enc)
            ds.from_streams(ss)
            for m, q in enumerate((q0, q1)):
                q.set_order(None, N, True)
                q.from_fastq(f[m], num_reads_per_block=B_CHAIN)
            yield types.SimpleNamespace(f=f, N=N, ds=ds, qs=[q0, q1])


def test_chain_ends_in_the_users_file(chain):
    from spring_amd import FastqOutStage, GzipStage
    c = chain
    with FastqOutStage() as fo, GzipStage() as gs:
        for m in range(2):
            fo.assemble(c.ds, c.N, quality=c.qs[m], ids=c.qs[m], paired_end=True, num_reads_per_block=B_CHAIN, mate=m)
            gs.compress(fo, member_records=1 + (B_CHAIN - 1) // 3)   # the reference's cut of a block for three threads
            gz, off = check(gs, c.f[m], record_cuts(fo.download()[1], 1 + (B_CHAIN - 1) // 3), m)
            assert gzip.decompress(gz) == c.f[m] and gs.info["bytes_out"] < len(c.f[m]) // 2


# ---------------------------------------------------------------- 9. write()
def test_write(tmp_path):
    from spring_amd import FastqOutStage, GzipStage
    from spring_amd.reorder import ReorderError
    ids, reads, quals = synth(1)
    text = fm.assemble(ids, reads, quals)[0]
    with FastqOutStage() as fo, GzipStage() as gs:
        fo.assemble(fm.reads_image(reads), N_REC, quality=b"".join(quals), ids=fm.id_image(ids), num_reads_per_block=1000)
        gs.compress(fo, member_records=500)
        p = tmp_path / "whole.fastq.gz"
        p.write_bytes(b"something longer than nothing" * 3)
        info = gs.write(p)
        assert p.read_bytes() == gs.download()[0] and info["ms_file"] > 0 and info["bytes_out"] == p.stat().st_size
        assert gzip.open(p).read() == text
        p2 = tmp_path / "twice.fastq.gz"
        gs.write(p2, append=True)
        gs.write(p2, append=True)
        assert gzip.open(p2).read() == text + text
        gs.write(p2)
        assert gzip.open(p2).read() == text
        with pytest.raises(ReorderError, match="code -2"):
            gs.write(tmp_path / "no_such_directory" / "x.gz")
        assert gs.download()[0] == p.read_bytes()   # an unwritable path leaves the result
        gs.compress(b"")
        gs.write(p2)
        assert p2.read_bytes() == b""


# ---------------------------------------------------------------- 10. refusals
def test_refusals():
    import ctypes as C
    from spring_amd import FastqOutStage, GzipStage, _lib
    from spring_amd.reorder import ReorderError
    data = b"@r\nACGT\n+\nIIII\n" * 100
    n = len(data)
    with GzipStage() as gs, FastqOutStage() as empty:
        def refused(call, code):
            gs.compress(data)   # a result to take away
            check(gs, data)
            with pytest.raises(ReorderError, match=code):
                call()
            for after in (gs.download, lambda: gs.write(os.devnull)):
                with pytest.raises(ReorderError, match="code -4"):
                    after()
            assert gs._L.spring_gzip_get_info(gs._h, C.byref(_lib.GzipInfo())) == -4

        for cuts in ([1, n], [0, n - 1], [0, n + 1], [0, 50, 50, n], [0, 60, 50, n], [0], [n]):
            refused(lambda: gs.compress(data, member_off=cuts), "code -1")
        refused(lambda: gs.compress(data, mode=2), "code -1")
        refused(lambda: gs.compress(data, mode=-1), "code -1")
        refused(lambda: gs.compress(empty), "code -4")          # an assembler context without a text
        refused(lambda: gs.compress(empty, mode=7), "code -1")
        try:
            other = FastqOutStage(device=1)
        except ReorderError:
            other = None                                         # one device only: no other one to refuse
        if other is not None:
            with other:
                other.assemble((b"ACGT", np.array([0, 4], np.uint64)), 1, ids=b"@r\n")
                refused(lambda: gs.compress(other), "code -1")
        # download / write before anything was compressed
        with GzipStage() as fresh:
            with pytest.raises(ReorderError, match="code -4"):
                fresh.download()
            with pytest.raises(ReorderError, match="code -4"):
                fresh.write(os.devnull)
        with pytest.raises(ReorderError, match="code -1"):
            gs.set_chunk_bytes(1000)
        gs.compress(data, member_off=[0, 16, n])   # and the context still works
        check(gs, data, [0, 16, n])


# ---------------------------------------------------------------- 11. batches of chunks
def text_like(n, seed=0):
    out = b"".join(b"@r.%d ACGTTGCA%d\n" % (i + 977 * seed, (i + seed) * i) for i in range(n // 16 + 8))
    assert len(out) >= n
    return out[:n]


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_batches_share_one_token_buffer():
    """Nine chunks of 4096 bytes in batches of three, of one and (a budget below one chunk) of one again: the chunks of
    the later batches index the per-chunk arrays by first + blockIdx.x and the tokens and codes by blockIdx.x.  The
    members and their offsets do not depend on the budget."""
    from spring_amd import GzipStage
    cb = 4096
    n = 8 * cb + 1
    cuts = [0, 2 * cb - 1000, 5 * cb - 3000, n]   # members of 2, 3 and 4 chunks: chunks 0-1, 2-4, 5-8
    assert [-(-(b - a) // cb) for a, b in zip(cuts[:-1], cuts[1:])] == [2, 3, 4]
    # batches of three are chunks 0-2, 3-5, 6-8: member 1 crosses the first edge, member 2 the second
    parts, c = [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        for x in range(a, b, cb):   # even chunks text-like, odd ones random: coded and stored chunks meet in a batch
            m = min(cb, b - x)
            parts.append(text_like(m, c) if c % 2 == 0 else random_bytes(m, 100 + c))
            c += 1
    data = b"".join(parts)
    assert c == 9 and len(data) == n
    with GzipStage() as gs:
        gs.set_chunk_bytes(cb)
        info = gs.compress(data, member_off=cuts)
        assert info["num_batches"] == 1 and info["num_chunks"] == 9 and info["chunks_stored"] == 4
        want = check(gs, data, cuts, "default budget")
        for budget, batches in ((3 * cb * 4, 3), (cb * 4, 9), (cb * 4 - 1, 9), (100, 9)):
            gs.set_token_bytes(budget)
            info = gs.compress(data, member_off=cuts)
            assert info["num_batches"] == batches, (budget, info["num_batches"])
            gz, off = check(gs, data, cuts, budget)
            assert info["chunks_stored"] == 4, budget
            assert gz == want[0] and off.tolist() == want[1].tolist(), budget
            info = gs.compress(data, member_off=cuts, mode=0)
            assert info["num_batches"] == 0
            check(gs, data, cuts, (budget, "stored"))
        gs.set_token_bytes(0)   # the default again
        info = gs.compress(data, member_off=cuts)
        assert info["num_batches"] == 1 and gs.download()[0] == want[0]


# ---------------------------------------------------------------- 12. every chunk size
CHUNK_SIZES = (4096, 16384, 32768, 36864, 61440, 65536)


@pytest.mark.parametrize("cb", CHUNK_SIZES)
def test_chunk_edges_at_every_chunk_size(cb):
    """The k * cb + d lengths of test_chunk_and_member_edges at a chunk size of its own.  At 65536 a stored chunk is two
    stored blocks (65535 + 1 bytes) and only the second one of a member's last chunk carries BFINAL."""
    from spring_amd import GzipStage
    pool = text_like(2 * cb + 1, 3)
    sources = [("text", pool)] + ([("random", random_bytes(2 * cb + 1, cb))] if cb == 65536 else [])
    with GzipStage() as gs:
        gs.set_chunk_bytes(cb)
        for what, src in sources:
            for k in (0, 1, 2):
                for d in (-1, 0, 1):
                    n = cb * k + d
                    if n <= 0:
                        continue
                    for mode in (0, 1):
                        info = gs.compress(src[:n], mode=mode)
                        assert info["chunk_bytes"] == cb and info["num_chunks"] == -(-n // cb), (what, k, d, mode)
                        assert info["num_batches"] == mode, (what, k, d, mode)
                        gz, _ = check(gs, src[:n], None, (cb, what, k, d, mode))
                        if mode == 0 or what == "random":
                            assert info["bytes_out"] == stored_bound(info, [0, n]), (what, k, d, mode)
                            assert info["chunks_stored"] == info["num_chunks"], (what, k, d, mode)
                        elif n >= 64:
                            assert info["chunks_stored"] < info["num_chunks"], (what, k, d, mode)   # text is coded
                        if cb == 65536 and n >= cb and (mode == 0 or what == "random"):
                            # the first chunk: 65535 bytes without BFINAL, then one byte, final only if the member ends here
                            assert gz[10:15] == bytes([0, 0xff, 0xff, 0, 0]), (what, k, d, mode)
                            assert gz[10 + 5 + 65535:10 + 5 + 65535 + 5] == bytes([1 if n == cb else 0, 1, 0, 0xfe, 0xff])
        if cb == 65536:   # a whole stored chunk that ends its member, and one that does not, side by side
            src = sources[1][1]
            for cuts in ([0, cb, 2 * cb + 1], [0, 1, cb + 1, 2 * cb + 1]):
                info = gs.compress(src, member_off=cuts)
                check(gs, src, cuts, cuts)
                assert info["chunks_stored"] == info["num_chunks"] and info["bytes_out"] == stored_bound(info, cuts)


# ---------------------------------------------------------------- 13. the window before a chunk is used
def window_of(cb):
    return min(32768, 65536 - cb)


@pytest.mark.parametrize("cb", (4096, 16384))
def test_matches_reach_into_the_window_small_chunks(cb):
    """Random bytes of period P = cb + 904: no match fits inside one chunk, every byte behind the first period has one
    P bytes back, inside the window.  A matcher that cannot reach across the chunk edge leaves >= n bytes; zlib level 1
    per chunk with the window as its preset dictionary gives 0.16 n (4096) and 0.14 n (16384)."""
    from spring_amd import GzipStage
    P = cb + 904
    n = max(8 * cb, 4 * P) + 1
    assert P <= window_of(cb)
    data = (random_bytes(P, 13 + cb) * (n // P + 1))[:n]
    with GzipStage() as gs:
        gs.set_chunk_bytes(cb)
        info = gs.compress(data)
        print("window, cb %d: period %d, %d -> %d (%.4f n)" % (cb, P, n, info["bytes_out"], info["bytes_out"] / n))
        check(gs, data, None, cb)
        assert info["bytes_out"] < n / 2, (cb, info["bytes_out"], n)


@pytest.mark.parametrize("cb", (32768, 36864, 61440))
def test_matches_reach_into_the_window_large_chunks(cb):
    """Four chunks and a byte; chunk i > 0 opens with a copy of the last D = window - 512 bytes of chunk i - 1 and is
    random behind that.  A matcher that cannot reach across the chunk edge leaves >= n bytes; with the window, three
    copies of D bytes go at well under half their size (zlib level 1 per chunk with the window as its preset dictionary
    saves 95 736, 83 422 and 10 425 bytes)."""
    from spring_amd import GzipStage
    w = window_of(cb)
    D = w - 512
    n = 4 * cb + 1
    chunks = [random_bytes(cb, 7 * cb)]
    for i in range(1, 5):
        m = cb if i < 4 else 1
        head = chunks[-1][-D:][:m]
        chunks.append(head + random_bytes(m - len(head), 7 * cb + i))
    data = b"".join(chunks)
    assert len(data) == n and data[cb:cb + D] == data[cb - D:cb]
    with GzipStage() as gs:
        gs.set_chunk_bytes(cb)
        info = gs.compress(data)
        print("window, cb %d: window %d, D %d, %d -> %d (saves %d, required %d)" % (
            cb, w, D, n, info["bytes_out"], n - info["bytes_out"], (D // 2) * 3))
        check(gs, data, None, cb)
        assert info["bytes_out"] <= n - (D // 2) * 3, (cb, info["bytes_out"], n)
