"""GPU tests of the front end of the stage (run with `pytest -m gpu` on an MI355X): the wide unpack kernel for streams
of fixed-size records, and the dictionary build whose radix sort orders a prefix of the key hashes and repairs the
rest (opts.sort_prefix_bits).  Bar: bit-exact against the CPU oracle, whatever the prefix."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import readsets as rs
from helpers import KEYS, SMALL_SETS, named_set
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

BLOCK = 128  # reads per block of k_unpack_fixed (UNPACK_READS, reorder_device.h)
PREFIX_BITS = (64, 40, 32, 8, 4, 1)


def _sa():
    import spring_amd
    return spring_amd


@functools.lru_cache(maxsize=1)
def _hip():
    """The HIP runtime the library is bound to (already loaded: RTLD_NOLOAD never maps a second copy)."""
    from spring_amd import _lib
    _lib.lib()
    H = C.CDLL("libamdhip64.so.7", mode=os.RTLD_NOLOAD | os.RTLD_NOW)
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for f in (H.hipMalloc, H.hipFree, H.hipMemcpy, H.hipDeviceSynchronize):
        f.restype = C.c_int
    return H


def _fixed(seed, n, L):
    return rs.pack_fixed(rs.np_reads(seed, max(4 * L, n * L // 8), n, L, 0.02))


def _check_unpack(dna, n, L, load):
    read, ln = po.load_dna(dna, n, L)
    with _sa().ReorderStage() as s:
        load(s)
        limbs, lens = s.download_reads()
    assert np.array_equal(lens, ln), (n, L)
    assert np.array_equal(limbs, read), (n, L)


# record size 2 + ceil(L / 4): L = 1, 5, ..., 61 walks it through every residue modulo 16; the longer ones reach
# 2 .. 16 limbs (W = ceil(2 L / 64): 1 .. 8 limbs are L = 32 k), odd and even record sizes
@pytest.mark.parametrize("L", list(range(1, 65, 4)) + [32, 64, 96, 128, 150, 160, 192, 224, 251, 256, 300, 511])
def test_unpack_fixed_records_every_size(L):
    n = 3 * BLOCK + 17
    dna = _fixed(1000 + L, n, L)
    _check_unpack(dna, n, L, lambda s: s.load_dna(dna, n, L))


@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 4321])
@pytest.mark.parametrize("L", [8, 31, 100, 150])
def test_unpack_fixed_records_block_edges(n, L):
    dna = _fixed(2000 + L + n, n, L)
    _check_unpack(dna, n, L, lambda s: s.load_dna(dna, n, L))


@pytest.mark.parametrize("shift", [0, 2, 4, 8, 1, 3, 13])
@pytest.mark.parametrize("L", [36, 100, 150])
def test_unpack_device_pointer_any_alignment(shift, L):
    """load_dna_device borrows the caller's pointer: the stream may start anywhere inside an allocation."""
    n = 2 * BLOCK + 5
    dna = _fixed(3000 + L, n, L)
    H = _hip()
    p = C.c_void_p()
    assert H.hipMalloc(C.byref(p), len(dna) + 64) == 0
    try:
        host = np.frombuffer(dna, dtype=np.uint8)
        assert H.hipMemcpy(p.value + shift, host.ctypes.data, len(dna), 1) == 0  # hipMemcpyHostToDevice
        assert H.hipDeviceSynchronize() == 0
        _check_unpack(dna, n, L, lambda s: s.load_dna_device(p.value + shift, len(dna), n, L, True))
    finally:
        assert H.hipFree(p) == 0


@pytest.mark.parametrize("where", [0, BLOCK - 1, BLOCK, 699])
def test_unpack_wrong_length_field_walks_the_records(where):
    """A stream of the size of a fixed-length stream whose reads are not all L long: the device sees the length field,
    the result of the fixed-record kernel is discarded and the records are walked."""
    n, L = 5 * BLOCK + 60, 100
    a = bytearray(_fixed(77, n, L))
    rec = 2 + (L + 3) // 4
    a[where * rec] = L - 2  # 98 bases fill as many bytes as 100
    dna = bytes(a)
    read, ln = po.load_dna(dna, n, L)
    assert ln[where] == L - 2
    _check_unpack(dna, n, L, lambda s: s.load_dna(dna, n, L))


DICT_SETS = ["test_1+2", "syn2k_100", "syn5k_150", "syn3k_64", "syn2k_251", "var2k", "var_short", "heavy", "dups",
             "tandem", "repeat10k"]


def _check_dict(name, bits):
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage(sa.ReorderOpts(sort_prefix_bits=bits)) as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        st = s.stats()
        for which in (0, 1):
            keys, sp, ids = po.build_dict(read, ln, L, which)
            assert st["numkeys"][which] == len(keys) and st["dict_numreads"][which] == len(ids)
            absent = keys ^ np.uint64(0x3333)
            absent = absent[~np.isin(absent, keys)]
            sizes, gids = s.dict_lookup(which, np.concatenate([keys, absent]))
            assert np.array_equal(sizes[:len(keys)], np.diff(sp).astype(np.uint32)), (name, bits, which)
            assert np.all(sizes[len(keys):] == 0xFFFFFFFF)
            assert np.array_equal(gids[:len(ids)], ids), (name, bits, which)  # same ids, same in-bin order
    assert st["sort_prefix_bits"] == bits
    if bits == 64:
        assert st["sort_repaired_runs"] == 0 and st["sort_full_sorts"] == 0
    return st


@pytest.mark.parametrize("bits", PREFIX_BITS)
@pytest.mark.parametrize("name", DICT_SETS)
def test_dictionary_under_forced_prefix_collisions(name, bits):
    _check_dict(name, bits)


def _check_dict_reads(letters, bits):
    """A dictionary build of fixed-length reads (uint8 [n, L] letters) against the oracle, as _check_dict -> stats."""
    sa = _sa()
    n, L = letters.shape
    dna = rs.pack_fixed(letters)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage(sa.ReorderOpts(sort_prefix_bits=bits)) as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        st = s.stats()
        for which in (0, 1):
            keys, sp, ids = po.build_dict(read, ln, L, which)
            assert st["numkeys"][which] == len(keys)
            sizes, gids = s.dict_lookup(which, keys)
            assert np.array_equal(sizes, np.diff(sp).astype(np.uint32)), (bits, which)
            assert np.array_equal(gids[:len(ids)], ids), (bits, which)
    return st


def test_forced_collisions_reach_the_repair_and_each_fall_back():
    """The cases above prove nothing unless the in-place repair and both causes of the fall-back to the 64-bit sort ran,
    each on an input that cannot trigger the other."""
    # `dups` (40 reads, 30 copies each) at 4 bits: a few bins of 30 in each of 16 runs -- short runs, re-ordered in place
    st = _check_dict("dups", 4)
    assert st["sort_repaired_runs"] > 0 and st["sort_full_sorts"] == 0, st
    # list overflow only: 5 000 nearly distinct keys in 256 runs of ~20 -- nearly every entry differs from its
    # predecessor (more than m / 4 + 1 024 positions), no run comes near 1 024 entries
    st = _check_dict("syn5k_150", 8)
    assert st["sort_list_overflows"] == 2 and st["sort_long_runs"] == 0 and st["sort_full_sorts"] == 2, st
    # long run only: 2 000 error-free copies of one read (two keys per dictionary: 70 % forward, 30 % reverse
    # complement) + 50 others at 1 bit -- at most ~100 hash changes (the list holds 1 536), but the run of the
    # 1 400-entry bin holds other keys too and is longer than the repair takes
    st = _check_dict_reads(rs.heavy_bin_reads(31, 2000, 50, 100, 0.0), 1)
    assert st["sort_long_runs"] > 0 and st["sort_list_overflows"] == 0, st
    assert st["sort_full_sorts"] == st["sort_long_runs"]


def test_repair_of_runs_near_the_longest_it_takes():
    """1 000 reads at 1 bit: two runs, together 1 000 entries, and the one that holds the 490-entry bin of the forward
    copies also holds about half of the 300 other reads' keys: a run of 600 .. 1 000 entries with several keys, the
    upper end of what k_sort_runs walks (16 windows of 64 entries back and forth) and k_sort_fix ranks in place."""
    st = _check_dict_reads(rs.heavy_bin_reads(32, 700, 300, 100, 0.0), 1)
    assert st["sort_repaired_runs"] > 0 and st["sort_full_sorts"] == 0, st


@pytest.mark.parametrize("name", SMALL_SETS)
def test_reorder_equals_oracle_whatever_the_prefix(name):
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    for K, T in ((1, 1), (32, 2)):
        want = po.reorder_rounds(read, ln, L, K, T)
        for fused in (2, 3):  # one chain / four chains per wavefront
            for bits in PREFIX_BITS:
                got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, fused=fused, sort_prefix_bits=bits))
                for k in KEYS:
                    assert np.array_equal(got[k], want[k]), (name, K, fused, bits, k)


def test_pool_10M_forced_collisions_equal_default():
    """10 M reads at 8 prefix bits (runs of ~39 000 entries: every dictionary takes the fall-back) against the
    library's own choice, stream for stream."""
    sa = _sa()
    n, L = 10_000_000, 100
    out = []
    for bits in (0, 8):
        with sa.ReorderStage(sa.ReorderOpts(sort_prefix_bits=bits)) as st:
            st.load_synth(n, L, n * L // 25, 23, 10000)
            out.append(st.run().streams())
    a, b = out
    assert b["stats"]["sort_full_sorts"] == 2 and a["stats"]["sort_full_sorts"] == 0
    assert a["stats"]["sort_prefix_bits"] == 40
    for k in KEYS + ("tid_off", "tid_off_s"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("bits", [-1, -64, 65, 1000])
def test_refused_prefix_bits(bits):
    sa = _sa()
    with pytest.raises(sa.ReorderError):
        sa.ReorderStage(sa.ReorderOpts(sort_prefix_bits=bits))
