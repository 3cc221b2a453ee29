"""GPU tests of the dictionary build's one-pass kernels (run with `pytest -m gpu` on an MI355X): the unpack pass that
also writes the dictionary keys (k_unpack_fixed_keys) and the writer that produces the hash-addressed table front to
back (k_tab_partition / k_tab_write / k_tab_overflow_pairs), against the previous path (opts.dict_build_mode = 1).
Bar: through the C ABI and dict_lookup, both dictionaries equal the CPU oracle's -- every present key with its bin,
every absent key absent -- under either mode; reorder streams equal the oracle's, and one mode's equal the other's.

Keys are placed in chosen buckets by inverting the table's hash: mix64 is a bijection and, with reads of 100 bases, a
dictionary window is 32 bases = any 64-bit value, so a read can carry unmix64(h) for any hash h in either window."""
import ctypes as C
import functools

import numpy as np
import pytest

import readsets as rs
from helpers import KEYS, SMALL_SETS, named_set
from oracle import pyoracle as po
from test_gpu_frontend import BLOCK, _fixed, _hip

pytestmark = pytest.mark.gpu

MODES = (0, 1)
M64 = (1 << 64) - 1
WG_BUCKETS = 1024  # buckets per workgroup of k_tab_write (TAB_WRITE_LG, dict_build.h)


def _sa():
    import spring_amd
    return spring_amd


def mix64(x):
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & M64; x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & M64; x ^= x >> 33
    return x


def unmix64(x):
    x ^= x >> 33; x = x * 0x9cb4b2f8129337db & M64; x ^= x >> 33; x = x * 0x4f74430c22a54005 & M64; x ^= x >> 33
    return x


def table_buckets(nm, tab_scale=2):
    """Buckets of the table build_dict makes for nm unique (key, dictionary) pairs (reorder_pipeline.cpp)."""
    def p2(v):
        p = 1
        while p < v:
            p <<= 1
        return p
    return max(8, p2(max(2, (nm * 10 + 15) // 16)) * p2(tab_scale))


def hash_in_bucket(b, nb, low):
    """A hash whose home bucket is b of nb; `low` picks the bits below the bucket index."""
    lg = nb.bit_length() - 1
    return ((b << (64 - lg)) | (low & ((1 << (64 - lg)) - 1))) & M64


def reads_with_keys(k0, k1, seed, L=100):
    """uint8 [n, L] letters: read i carries key k0[i] in dictionary 0's window and k1[i] in dictionary 1's (L = 100:
    bases 18..49 and 50..81; base j of a window is bits 2j, 2j+1 of the key, SPRING code A0 G1 C2 T3)."""
    assert L == 100 and len(k0) == len(k1)
    n = len(k0)
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, (n, L), dtype=np.uint8)
    sh = (2 * np.arange(32)).astype(np.uint64)
    for keys, start in ((k0, 18), (k1, 50)):
        kk = np.array(keys, dtype=np.uint64)
        codes[:, start:start + 32] = ((kk[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8)
    return np.frombuffer(b"AGCT", dtype=np.uint8)[codes]


def check_dicts(load, read, ln, L, mode, path=None, tab_scale=0, extra_absent=(), oracle=None):
    """Build under `mode` and compare both dictionaries with the oracle's; -> stats."""
    sa = _sa()
    with sa.ReorderStage(sa.ReorderOpts(dict_build_mode=mode, tab_scale=tab_scale)) as s:
        load(s)
        s.build_dict()
        st = s.stats()
        for which in (0, 1):
            keys, sp, ids = oracle[which] if oracle else po.build_dict(read, ln, L, which)
            assert st["numkeys"][which] == len(keys) and st["dict_numreads"][which] == len(ids)
            absent = np.concatenate([keys ^ np.uint64(0x3333), np.array(extra_absent, dtype=np.uint64)])
            absent = absent[~np.isin(absent, keys)]
            sizes, gids = s.dict_lookup(which, np.concatenate([keys, absent]))
            assert np.array_equal(sizes[:len(keys)], np.diff(sp).astype(np.uint32)), (mode, which)
            assert np.all(sizes[len(keys):] == 0xFFFFFFFF), (mode, which)
            assert np.array_equal(gids[:len(ids)], ids), (mode, which)  # same ids, same in-bin order
    if path is not None:
        assert st["dict_build_path"] == path, (mode, st["dict_build_path"])
    return st


def check_both_modes(dna, n, L, load=None, path0=3, **kw):
    read, ln = po.load_dna(dna, n, L)
    oracle = [po.build_dict(read, ln, L, which) for which in (0, 1)]
    load = load or (lambda s: s.load_dna(dna, n, L))
    for mode in MODES:
        check_dicts(load, read, ln, L, mode, path=path0 if mode == 0 else 0, oracle=oracle, **kw)


# ------------------------------------------------------------------ the table writer
def placed_pool(tab_scale, seed, confine=None):
    """1 000 reads with distinct keys -> 2 000 pairs, a table of 2 048 * tab_scale buckets: two workgroups' ranges and
    more.  (c0, c1) pairs of dictionary 0 / 1 are placed in chosen buckets; the rest falls where `low`-random hashes
    fall (in buckets < confine, if given).  A few reads are repeated, so that multi-read and deep bins are among them."""
    n = 1000
    nb = table_buckets(2 * n, tab_scale)
    rng = np.random.default_rng(seed)
    low = lambda: int(rng.integers(1, 1 << 62))
    spec = {100: (3, 2), 200: (2, 4), 300: (5, 4),            # 5, 6 and 9 pairs in a bucket
            WG_BUCKETS - 1: (4, 5), WG_BUCKETS: (3, 2),       # ... where the run straddles two workgroups' ranges
            nb - 1: (5, 4), 0: (2, 3), 1: (4, 0),             # ... in the last bucket: the overflow wraps to bucket 0
            400: (0, 6), 401: (7, 0)}                         # one dictionary alone fills a bucket and overflows
    if nb > 2 * WG_BUCKETS:
        spec.update({2 * WG_BUCKETS - 1: (0, 6), 2 * WG_BUCKETS: (2, 2)})
    h = [[], []]
    absent = []
    for b, cnt in spec.items():
        for l in (0, 1):
            h[l] += [hash_in_bucket(b, nb, low()) for _ in range(cnt[l])]
        absent += [unmix64(hash_in_bucket(b, nb, low())) for _ in range(3)]  # probes that walk the full buckets
    # one hash in both dictionaries, in a bucket with other pairs either side of it; and one read whose two windows are equal
    mid = hash_in_bucket(500, nb, 1 << 40)
    for l in (0, 1):
        h[l] += [hash_in_bucket(500, nb, 1 << 39), mid, hash_in_bucket(500, nb, 1 << 41)][l:l + 2 + l]
    same = hash_in_bucket(600, nb, low())
    special = set(spec) | {500, 600}
    fill = [[], []]
    for l in (0, 1):
        while len(h[l]) + 1 + len(fill[l]) < n:
            b = int(rng.integers(0, confine or nb))
            if b not in special:
                fill[l].append(hash_in_bucket(b, nb, low()))
    h0 = [same] + h[0] + fill[0]
    h1 = [same] + h[1] + fill[1]
    assert len(set(h0)) == n and len(set(h1)) == n
    letters = reads_with_keys([unmix64(x) for x in h0], [unmix64(x) for x in h1], seed)
    letters = np.concatenate([letters, np.repeat(letters[5:15], 3, axis=0), np.repeat(letters[20:21], 20, axis=0)])
    rng.shuffle(letters, axis=0)
    return letters, nb, absent


@pytest.mark.parametrize("tab_scale", [1, 2, 4])
def test_table_writer_full_buckets_block_edges_and_wrap(tab_scale):
    letters, nb, absent = placed_pool(tab_scale, 40 + tab_scale)
    assert nb == 2048 * tab_scale
    n, L = letters.shape
    check_both_modes(rs.pack_fixed(letters), n, L, tab_scale=tab_scale, extra_absent=absent)


def test_table_writer_most_blocks_empty():
    """All keys but the placed ones in the first workgroup's 1 024 buckets of 8 192: two pairs per bucket there, many past
    the fourth, and four of the eight workgroups without a key, which must still write their buckets.  (A table has at
    most five buckets per pair, so workgroups of 1 024 buckets cannot outnumber the keys; this is what the sizes allow.)"""
    letters, nb, absent = placed_pool(4, 77, confine=WG_BUCKETS)
    n, L = letters.shape
    check_both_modes(rs.pack_fixed(letters), n, L, tab_scale=4, extra_absent=absent)


@pytest.mark.parametrize("lens", [(60,), (100,), (100, 60), (60, 60, 60, 60)])
def test_smallest_table_and_empty_second_dictionary(lens):
    """1, 2 and 3 keys in all in the table of 8 buckets (a read of 60 bases is in dictionary 0 only: dictionary 1's window
    ends at base 81), and a pool whose second dictionary is empty."""
    rng = np.random.default_rng(len(lens) * 7 + lens[0])
    reads = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, k)]) for k in lens]
    dna, n, L = rs.pack_var(reads), len(reads), 100
    read, ln = po.load_dna(dna, n, L)
    fixed = all(k == L for k in lens)
    for mode in MODES:
        st = check_dicts(lambda s: s.load_dna(dna, n, L), read, ln, L, mode,
                         path=0 if mode else (3 if fixed else 2))
        assert st["numkeys"][0] == len(lens) and st["numkeys"][1] == sum(k == 100 for k in lens)


@pytest.mark.parametrize("mode", MODES)
def test_second_build_on_memory_of_the_first(mode):
    """Two builds in one process: the 3 000-read pool's stage gets blocks the 200 000-read pool's stage gave back to the
    library's block pool, and nothing clears a table before it is written: keys of the first pool must be absent."""
    n1, n2, L = 200_000, 3_000, 100
    dna1 = rs.pack_fixed(rs.np_reads(501, n1 * L // 25, n1, L, 0.01))
    dna2 = rs.pack_fixed(rs.np_reads(502, n2 * L // 25, n2, L, 0.01))
    read1, ln1 = po.load_dna(dna1, n1, L)
    read2, ln2 = po.load_dna(dna2, n2, L)
    first = [po.build_dict(read1, ln1, L, which)[0] for which in (0, 1)]
    path = 0 if mode else 3
    check_dicts(lambda s: s.load_dna(dna1, n1, L), read1, ln1, L, mode, path=path)
    check_dicts(lambda s: s.load_dna(dna2, n2, L), read2, ln2, L, mode, path=path,
                extra_absent=np.concatenate(first)[::7])


# ------------------------------------------------------------------ keys in the unpack pass
@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1, 4321])
@pytest.mark.parametrize("L", [64, 65, 100, 150, 151, 192])
def test_keys_from_unpack_lengths_and_block_edges(n, L):
    check_both_modes(_fixed(7000 + L + n, n, L), n, L)


@pytest.mark.parametrize("shift", [0, 1, 3, 4, 8, 13])
def test_keys_from_unpack_device_pointer_any_alignment(shift):
    n, L = 2 * BLOCK + 5, 150
    dna = _fixed(7100, n, L)
    H = _hip()
    p = C.c_void_p()
    assert H.hipMalloc(C.byref(p), len(dna) + 64) == 0
    try:
        host = np.frombuffer(dna, dtype=np.uint8)
        assert H.hipMemcpy(p.value + shift, host.ctypes.data, len(dna), 1) == 0  # hipMemcpyHostToDevice
        assert H.hipDeviceSynchronize() == 0
        check_both_modes(dna, n, L, load=lambda s: s.load_dna_device(p.value + shift, len(dna), n, L, True))
    finally:
        assert H.hipFree(p) == 0


@pytest.mark.parametrize("where", [0, BLOCK, 699])
def test_wrong_length_field_discards_the_keys_of_the_unpack_pass(where):
    """The stream has the size of a fixed-length stream, one read is shorter: the records are walked, the pairs the unpack
    pass wrote are dropped with its limbs, and the key pass runs."""
    n, L = 5 * BLOCK + 60, 100
    a = bytearray(_fixed(78, n, L))
    a[where * (2 + (L + 3) // 4)] = L - 2  # 98 bases fill as many bytes as 100
    check_both_modes(bytes(a), n, L, path0=2)


def test_variable_length_pool_keeps_the_key_pass():
    dna, n, L = named_set("var2k")
    check_both_modes(dna, n, L, path0=2)


def test_fastq_load_keeps_the_key_pass():
    sa = _sa()
    a = rs.np_reads(503, 4000, 1500, 100, 0.01)
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(r), b"I" * 100) for i, r in enumerate(a))
    with sa.ReorderStage() as s:
        s.load_fastq(fq)
        s.build_dict()
        assert s.stats()["dict_build_path"] == 2


@pytest.mark.parametrize("mode", [-1, 2, 100])
def test_refused_dict_build_mode(mode):
    sa = _sa()
    with pytest.raises(sa.ReorderError):
        sa.ReorderStage(sa.ReorderOpts(dict_build_mode=mode))


# ------------------------------------------------------------------ the pipeline
@functools.lru_cache(maxsize=None)
def _want(name, K, T):
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    return po.reorder_rounds(read, ln, L, K, T)


@pytest.mark.parametrize("name", SMALL_SETS)
def test_reorder_equals_oracle_under_both_modes(name):
    sa = _sa()
    dna, n, L = named_set(name)
    for K, T in ((1, 1), (8, 2), (4096, 2)):
        want = _want(name, K, T)
        for mode in MODES:
            got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, dict_build_mode=mode))
            for k in KEYS:
                assert np.array_equal(got[k], want[k]), (name, K, mode, k)


def test_pool_2M_one_pass_equals_previous_path():
    """2 M synthetic reads at the library's defaults: mode 0 against mode 1, stream for stream."""
    sa = _sa()
    n, L = 2_000_000, 150
    out = []
    for mode in MODES:
        with sa.ReorderStage(sa.ReorderOpts(dict_build_mode=mode)) as st:
            st.load_synth(n, L, n * L // 25, 29, 10000)
            out.append(st.run().streams())
    a, b = out
    assert a["stats"]["dict_build_path"] == 3 and b["stats"]["dict_build_path"] == 0
    for k in KEYS + ("tid_off", "tid_off_s"):
        assert np.array_equal(a[k], b[k]), k
