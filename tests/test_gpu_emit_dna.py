"""The temp.dna writers (run with `pytest -m gpu`): k_emit_dna_fixed / emit_dna_byte, which write temp.dna.<tid> and
temp.dna.singleton of every pool of one read length, at read lengths that are NOT a multiple of four, and k_emit_dna,
the variable-length kernel, at the same lengths.  Bar: byte for byte, against two references: po.write_dna_stream (pinned
to the reference's writetofile in tests/test_oracle_vs_ref_stages.py) and `plain_stream` below, a packer written here
from the read letters that knows neither limbs nor an oracle.

Why the lengths: a thread of k_emit_dna_fixed builds one 32-bit word of the output, and a reverse-complemented record
takes its bytes from the limb array through two special cases -- the cross-limb fetch (`sh > 56`, possible only when
len % 4 != 0) and the last, partial byte (`lo < 0`, the mask 0xff >> (-2 lo); only when len % 4 != 0).  SWEEP holds
every residue of L mod 4 on each side of the 1-, 2-, 4-, 8- and 16-limb edges, every value of the record size
2 + ceil(L / 4) mod 4, and the workload's 150 (40-byte records, no word straddles two of them) between 146 and 153
(whose records do).  The pools were run through the CPU oracle first: at every length of SWEEP the matched streams hold at
least 71 'r' and 153 'd' records, at most 362 of the 600 reads stay single, and the streams' byte counts reach all four
values mod 4.  A length added later is checked the same way on the CPU first.

That a pool was taken as one of a single read length is read from stats.dict_build_path: at default options bit 0 (the
keys came from the unpack pass) is set only for such pools, and clear for the cut pools of the variable-length test.  A
pool loaded from FASTQ text never takes the keys from the unpack pass, so for test_from_fastq_text no existing signal
says which kernel ran; what says so is the mutation run below, in which that test fails.

Shown to be able to fail -- two mutants of emit_dna_byte, neither of which changes an address that is read or written:
  M1  the line `if (sh > 56) v |= r[li + 1] << (64 - sh);` deleted
  M2  the line `if (lo < 0) v &= 0xffu >> (-2 * lo);` deleted
Run on an MI355X against the tests that compared temp.dna bytes before this file (test_emit_dna_matches_writetofile, the
test_call_reorder_* file-set tests, the older cases of test_gpu_vs_ref_stages.py, test_reorder_encode_run_file_contract,
the var2k encoder file contract) and against the tests added with it:
  the older tests   all pass on M1 and on M2
  M1 fails          test_fixed_length_sweep at the 24 lengths with L % 4 != 0 and L > 32 (up to 32 bases a read is one
                    limb), test_from_fastq_text (4 of 4), the fixed33 / fixed150 / fixed251 cases of
                    test_ref_stages_reorder_in_memory, _reorder_file_contract and _chained[two_calls],
                    test_call_reorder_file_set_at_lengths_not_a_multiple_of_four (4 of 4),
                    test_call_reorder_two_chain_groups_150bp, test_encoder_run_file_contract_after_reorder_run[syn5k_150]
  M2 fails          the same, plus the sweep at 21, 22 and 23 (27 lengths), less _chained[two_calls]: the encoder
                    never looks at the padding bits, which is why the encoder file contract compares temp.dna itself
  pass on both      the sweep at 20 and 152 (multiples of four: both lines are dead there), the variable-length and
                    tiny-pool tests (k_emit_dna; singleton streams hold no reverse-complemented record)
Two more mutants for those: the tail bytes of the last word stored in reverse order (k_emit_dna_fixed) fails
test_tiny_pools at 20 and 33 bases (not at 21: 8-byte records, no tail; not the 21-byte stream, whose tail is one byte)
and the sweep wherever a stream has a tail of two or three bytes; `3 - code` replaced by `code ^ 1` in k_emit_dna fails
test_variable_length_kernel_at_the_same_lengths (4 of 4)."""
import functools

import numpy as np
import pytest

import readsets as rs
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

SWEEP = (20, 21, 22, 23, 33, 34, 35, 63, 65, 66, 97, 101, 127, 129, 145, 146, 149, 150, 151, 152, 153, 191, 193, 254, 255,
         257, 509, 510, 511)
VAR_LENGTHS = (33, 150, 153, 511)
K, T = 16, 3

_CODE = bytes.maketrans(b"AGCT", bytes([0, 1, 2, 3]))      # write_dna_in_bits: A 0, G 1, C 2, T 3
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def plain_record(letters: bytes, rev: bool) -> bytes:
    """One temp.dna record from the read's letters: u16 length, four bases per byte (base j in bits 2 (j % 4)), the last
    byte zero padded; `rev`: the complement of the reversed read instead."""
    if rev:
        letters = letters[::-1].translate(_COMPLEMENT)
    c = letters.translate(_CODE)
    out = bytearray(len(c).to_bytes(2, "little"))
    for j in range(0, len(c), 4):
        b = 0
        for q, x in enumerate(c[j:j + 4]):
            b |= x << (2 * q)
        out.append(b)
    return bytes(out)


def plain_stream(reads, order, rc=None) -> bytes:
    """temp.dna.<tid> (rc: the tid's read_rev.txt bytes) or temp.dna.singleton (rc None) of the reads `order` names."""
    return b"".join(plain_record(reads[int(i)], rc is not None and rc[k] == ord("r")) for k, i in enumerate(order))


def pool_letters(L, n=600):
    return [bytes(r) for r in rs.np_reads(900 + L, 600 * L // 25, 600, L, 0.0 if L < 40 else 0.01)[:n]]


def _emit_all(dna, n, L, T_=T):
    """One run with 16 chains -> (streams, [emit_dna(0), .., emit_dna(T - 1)], emit_dna(-1))."""
    import spring_amd as sa
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T_)) as s:
        s.load_dna(dna, n, L)
        out = s.run().streams()
        return out, [s.emit_dna(t) for t in range(T_)], s.emit_dna(-1)


def _check_streams(what, reads, dna, n, L, out, tids, single):
    """Both references, every stream; -> the byte counts of the streams."""
    read, ln = po.load_dna(dna, n, L)
    assert len(out["order"]) + len(out["order_s"]) == n, what
    for t, got in enumerate(tids):
        a, b = int(out["tid_off"][t]), int(out["tid_off"][t + 1])
        order, rc = out["order"][a:b], out["rc"][a:b]
        assert got == po.write_dna_stream(read, ln, L, order, rc), (what, "tid", t, "oracle")
        assert got == plain_stream(reads, order, rc), (what, "tid", t, "plain packer")
    assert single == po.write_dna_stream(read, ln, L, out["order_s"], None), (what, "singleton", "oracle")
    assert single == plain_stream(reads, out["order_s"]), (what, "singleton", "plain packer")
    return [len(x) for x in tids] + [len(single)]


@functools.lru_cache(maxsize=None)
def _fixed_run(L):
    reads = pool_letters(L)
    dna = rs.pack_fixed(np.array([np.frombuffer(r, np.uint8) for r in reads]))
    return (reads, dna) + _emit_all(dna, len(reads), L)


@pytest.mark.parametrize("L", SWEEP)
def test_fixed_length_sweep(L):
    reads, dna, out, tids, single = _fixed_run(L)
    assert out["stats"]["dict_build_path"] & 1, "the pool was not taken as one of a single read length"
    # nothing is shown unless both orientations are among the matched records
    assert np.count_nonzero(out["rc"] == ord("r")) >= 1 and np.count_nonzero(out["rc"] == ord("d")) >= 1
    sizes = _check_streams(L, reads, dna, len(reads), L, out, tids, single)
    assert sum(sizes) == len(reads) * (2 + (L + 3) // 4)


def test_fixed_length_sweep_reaches_every_tail_of_the_last_word():
    """The last word of a stream is written whole or as 1, 2 or 3 single bytes (`nbytes < 4`): over the sweep the
    non-empty streams end at all four residues."""
    tails = set()
    for L in SWEEP:
        _, _, _, tids, single = _fixed_run(L)
        tails |= {len(x) % 4 for x in tids + [single] if x}
    assert tails == {0, 1, 2, 3}


@pytest.mark.parametrize("L", VAR_LENGTHS)
def test_variable_length_kernel_at_the_same_lengths(L):
    """The sweep's reads with one read cut by one base: the pool is no longer of one length, k_emit_dna runs, and is held
    to the same two answers."""
    reads = pool_letters(L)
    reads[7] = reads[7][:-1]
    dna = rs.pack_var(reads)
    out, tids, single = _emit_all(dna, len(reads), L)
    assert not out["stats"]["dict_build_path"] & 1
    assert np.count_nonzero(out["rc"] == ord("r")) >= 1 and np.count_nonzero(out["rc"] == ord("d")) >= 1
    sizes = _check_streams(("var", L), reads, dna, len(reads), L, out, tids, single)
    assert sum(sizes) == len(dna)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("L", [20, 21, 33])
def test_tiny_pools(L, n):
    """A stream shorter than a few words: the first word spans two records (7-, 8- and 11-byte records), a one-read stream is
    a word plus a tail of three bytes at L = 20 and ends on a word boundary at L = 21.  The reads are unrelated (uniform
    random), so all of them stay single and every tid stream is empty.  (Nothing shorter than 20 bases: nothing in the
    suite runs the chains there.)"""
    letters = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(4000 + L).integers(0, 4, (5, L))][:n]
    reads = [bytes(r) for r in letters]
    dna = rs.pack_fixed(letters)
    out, tids, single = _emit_all(dna, n, L)
    assert out["stats"]["dict_build_path"] & 1
    assert len(out["order"]) == 0 and sorted(out["order_s"].tolist()) == list(range(n))
    assert tids == [b""] * T
    assert len(single) == n * (2 + (L + 3) // 4)
    read, ln = po.load_dna(dna, n, L)
    assert single == po.write_dna_stream(read, ln, L, out["order_s"], None)
    assert single == plain_stream(reads, out["order_s"])


@pytest.mark.parametrize("L,shorter", [(150, 0), (151, 5), (153, 0), (153, 1)])
def test_from_fastq_text(L, shorter):
    """3000 reads of one length on a small genome as FASTQ text, 5 % of them with an N (`shorter` bases shorter than the
    clean ones, or as long): the front end's equal-length path, 16 chains, two tids; expected = the plain packer over the
    clean read lines of the text itself."""
    import spring_amd as sa
    n = 3000
    rng = np.random.default_rng(6000 + L + shorter)
    lines = [bytearray(r) for r in rs.np_reads(5000 + L, n * L // 25, n, L, 0.01)]
    for i in np.flatnonzero(rng.random(n) < 0.05):
        del lines[i][L - shorter:]
        lines[i][int(rng.integers(0, len(lines[i])))] = ord("N")
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(s), b"I" * len(s)) for i, s in enumerate(lines))
    clean = [s for s in text.split(b"\n")[1::4] if b"N" not in s]
    assert 0 < n - len(clean) < n // 10 and {len(s) for s in clean} == {L}
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=2)) as s:
        info = s.load_fastq(text)
        out = s.run().streams()
        tids, single = [s.emit_dna(t) for t in range(2)], s.emit_dna(-1)
    assert info["max_readlen"] == L and info["num_reads_clean"][0] == len(clean) and info["num_reads"][0] == n
    assert np.count_nonzero(out["rc"] == ord("r")) >= 1 and np.count_nonzero(out["rc"] == ord("d")) >= 1
    _check_streams(("fastq", L, shorter), clean, rs.pack_var(clean), len(clean), L, out, tids, single)
