"""CPU-only checks of the run-aware first keys of the block-sort stage: their numpy restatement
(tests/bwt_runs_model.py: key, hop and the doubling rounds) against bwt_model.suffix_ranks, the round counts DESIGN.md
section 15 quotes, the key layout and the planner at 76 bytes a position (spring_amd/csrc/bwt_plan.h) in a stand-alone
host build under the address and undefined-behaviour sanitizers, and the two facts about the options SPRING passes to
BSC (64 MiB cuts, LZP off) on the reference's own program (skipped when oracle/_ref/ref_bsc is not built)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bwt_model as bm
import bwt_runs_model as rm
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("acgt", "bytes", "const", "cac", "tail00", "tailff")
TEN_LENGTHS = (1, 2, 3, 7, 16, 17, 65, 257, 1025, 4097)
SETTINGS = ((3, 4), (2, 3), (4, 20))   # (text bytes, bits of the run field): caps of 15, 7 and 2^20 - 1
HARD = b"A" * 3000 + b"C" + b"A" * 2000 + b"B"


def _texts():
    return [bm.contents(kind, n, seed=9) for kind in KINDS for n in TEN_LENGTHS] + rm.quality_like_pool()


def test_quality_like_pool_is_what_it_says():
    pool = rm.quality_like_pool()
    assert len(pool) == 300 and min(map(len, pool)) >= 1 and max(map(len, pool)) <= 399
    seen = set(b"".join(pool))
    assert len(seen) == 6 and 0x00 in seen and 0xff in seen
    longest = max(int(rm.run_lengths(np.frombuffer(t, np.uint8)).max()) for t in pool)
    assert longest >= 90   # runs of 90 and, where two of one symbol meet, more: above the caps of 7 and 15


@pytest.mark.parametrize("k,R", SETTINGS)
def test_run_keys_and_hop_give_the_suffix_order(k, R):
    for t in _texts():
        got, rounds, entries = rm.ranks(t, k, R)
        assert np.array_equal(got, bm.suffix_ranks(t)), (k, R, len(t), t[:40])
        assert rounds == len(entries) <= len(t).bit_length() + 2


def test_first_key_is_a_coarsening_of_the_suffix_order_that_refines_the_first_bytes():
    for k, R in SETTINGS:
        for t in _texts()[::7]:
            T = np.frombuffer(t, np.uint8)
            key, hop, _ = rm.first_keys(T, k, R)
            sa = np.argsort(bm.suffix_ranks(T))
            assert (np.diff(key[sa]) >= 0).all(), (k, R, len(t))           # never against the true order
            plain = rm.first_keys(T, k, 1, 1)[0] >> 2                       # bytes | valid
            assert np.array_equal(key >> (R + 1), plain)                    # equal keys share their first k bytes
            L = rm.run_lengths(T)
            assert ((hop == 0) | ((hop == L) & (L >= k) & (L < (1 << R) - 1))).all()


def test_round_counts():
    r, rounds, entries = rm.ranks(HARD, 7, 0, runs=False)
    assert rounds == 10 and np.array_equal(r, bm.suffix_ranks(HARD))
    r, rounds, entries = rm.ranks(HARD, 4, 20)
    assert rounds == 2 and sum(entries) == 8996 and entries[1] == 2 * 1997 and np.array_equal(r, bm.suffix_ranks(HARD))
    # a cap below the runs' lengths: the long runs tie and take the doubling rounds, the result is the same
    r, rounds, _ = rm.ranks(HARD, 4, 20, cap_bits=3)
    assert rounds > 2 and np.array_equal(r, bm.suffix_ranks(HARD))


HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "bwt_plan.h"
int main(int argc, char **argv) {
  const uint64_t segs[] = {0, 1, 2, 255, 256, 257, 1000, 4096, 4097, 1ull << 20, (1ull << 20) + 1, 1ull << 21, bwt::MAX_SUB_SEGMENTS};
  for (uint64_t s : segs) {
    bwt::RunKeyLayout k = bwt::run_key_layout(s);
    printf("K %llu %d %d %d %d\n", (unsigned long long)s, k.seg_bits, k.key_bytes, k.run_bits, k.total_bits);
  }
  printf("W %llu %llu %llu\n", (unsigned long long)bwt::workspace_need(1000, 3), (unsigned long long)bwt::workspace_need(1000, 3, false),
         (unsigned long long)bwt::workspace_need(1000, 3, true));
  // plans: argv = budget, then the segment lengths
  std::vector<uint64_t> off(1, 0);
  const uint64_t budget = strtoull(argv[1], 0, 10);
  for (int i = 2; i < argc; i++) off.push_back(off.back() + strtoull(argv[i], 0, 10));
  const uint64_t S = off.size() - 1;
  std::vector<uint64_t> first(S + 1);   // exactly the room the planner asks for
  const long long nb = bwt::plan_sub_batches(off.data(), S, budget, first.data(), true);
  printf("P %lld", nb);
  for (long long b = 0; b <= nb; b++) printf(" %llu", (unsigned long long)first[b]);
  printf("\n");
  return 0;
}
"""


def _harness(tmp_path):
    src = tmp_path / "runs_plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "runs_plan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "spring_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return exe


def _run(exe, budget, lens):
    # leak detection needs ptrace, which not every box grants; the harness frees what it allocates anyway
    r = subprocess.run([str(exe), str(budget)] + [str(x) for x in lens], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_layout_and_planner_in_a_sanitized_host_build(tmp_path):
    exe = _harness(tmp_path)
    out = _run(exe, 76 * 4097 + 16, bm.LENGTHS)
    rows = [[int(x) for x in ln.split()[1:]] for ln in out if ln.startswith("K ")]
    assert len(rows) == 13
    for s, seg_bits, k, R, total in rows:
        assert (seg_bits, k, R, total) == rm.run_key_layout(s), s
        assert (1 << seg_bits) >= max(s, 1) and 2 <= k <= 4 and R in (16, 20) and total == seg_bits + 8 * k + 4 + R <= 64
        assert R == 20 or (64 - 4 - 20 - seg_bits) // 8 < 4   # 20 bits wherever four text bytes still fit beside them
    assert {s: (k, R) for s, _, k, R, _ in rows} == {0: (4, 20), 1: (4, 20), 2: (4, 20), 255: (4, 20), 256: (4, 20),
                                                     257: (4, 16), 1000: (4, 16), 4096: (4, 16), 4097: (3, 16),
                                                     1 << 20: (3, 16), (1 << 20) + 1: (2, 16), 1 << 21: (2, 16),
                                                     1 << 24: (2, 16)}
    assert [x for x in out if x.startswith("W ")][0].split()[1:] == [str(72 * 1000 + 48)] * 2 + [str(76 * 1000 + 48)]
    for budget, ls in ((76 * 4097 + 16, bm.LENGTHS), (10 ** 12, bm.LENGTHS), (76 * 4097 + 16, bm.LENGTHS[::-1]), (16, [0, 0, 0]),
                       (76 * 10 + 16, [10] * 7 + [0] * 5 + [3]), (10 ** 6, [])):
        row = [int(x) for x in [x for x in _run(exe, budget, ls) if x.startswith("P ")][0].split()[1:]]
        nb, first = row[0], row[1:]
        assert first == rm.plan(list(ls), budget) and nb == len(first) - 1, (budget, ls)
        for a, b in zip(first, first[1:]):
            assert 76 * sum(ls[a:b]) + 16 * (b - a) <= budget
    assert [x for x in _run(exe, 76 * 4097 + 16, bm.LENGTHS) if x.startswith("P ")][0].split()[1] == "3"
    # what fits at 72 bytes a position does not at 76
    assert [x for x in _run(exe, 72 * 4097 + 16, bm.LENGTHS) if x.startswith("P ")][0].split()[1] == str(-1 - bm.LENGTHS.index(4097))


# ------------------------------------------------------------------ what SPRING passes to BSC: "-b64", "-p", "-e1"
# The file BSC_compress writes (bsc.cpp:149-390): int32 nBlocks; per block the packed 10-byte header {int64 blockOffset,
# int8 recordSize, int8 sortingContexts} and then bsc_compress's block, whose 28-byte header is {blockSize, dataSize,
# mode, index, adler32 of the data, of the block, of the header}.  mode = sorter | coder << 5, plus lzpMinLen << 8 and
# lzpHashSize << 16 where LZP is on (libbsc.cpp:97-120).
needs_ref_bsc = pytest.mark.skipif(po.ref_bsc_bin() is None, reason="oracle/_ref/ref_bsc not built (needs the reference sources)")


def _ref_bsc(tmp_path, data):
    src, dst = tmp_path / "in.raw", tmp_path / "out.bsc"
    src.write_bytes(data)
    subprocess.run([po.ref_bsc_bin(), str(src), str(dst)], check=True, capture_output=True)
    return dst.read_bytes()


@needs_ref_bsc
def test_spring_writes_blocks_without_lzp(tmp_path):
    data = bm.contents("acgt", 4096, seed=1)
    out = _ref_bsc(tmp_path, data)
    n_blocks, block_off, record, contexts = struct.unpack_from("<iqbb", out, 0)
    assert (n_blocks, block_off, record, contexts) == (1, 0, 1, 1)   # LIBBSC_CONTEXTS_FOLLOWING
    block_size, data_size, mode = struct.unpack_from("<iii", out, 14)
    assert block_size == len(out) - 14 and data_size == len(data)
    assert mode == 1 | (1 << 5) and mode >> 8 == 0   # BWT, QLFC static; no LZP parameters above bit 7


@needs_ref_bsc
def test_spring_cuts_at_64_mib_not_25(tmp_path):
    n = 26 * 1024 * 1024 + 1
    out = _ref_bsc(tmp_path, b"G" * n)
    n_blocks, block_off, record, contexts = struct.unpack_from("<iqbb", out, 0)
    assert n_blocks == 1 and block_off == 0   # a 25 MiB cut would make two
    assert struct.unpack_from("<ii", out, 14)[1] == n
