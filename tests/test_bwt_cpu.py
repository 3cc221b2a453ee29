"""CPU-only checks of the block-sort stage: the numpy model of bsc_bwt_encode (tests/bwt_model.py) against the real
function of oracle/_ref/libref_units.so (skipped when that is not built), the ctypes mirror of spring_bwt_info against
the C header, the exported symbols, and the stage's host arithmetic (spring_amd/csrc/bwt_plan.h: index stride, key
layout, sub-batch planner) in a stand-alone host build under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bwt_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LENGTHS = [1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 100, 255, 256, 257, 1000, 4097, 70000]


def _cases(n):
    rng = np.random.default_rng(n)
    yield "4 symbols", np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    yield "256 symbols", rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    yield "constant", b"G" * n
    yield "CAC", (b"CAC" * (n // 3 + 1))[:n]


@pytest.mark.skipif(bm.ref_lib() is None, reason="oracle/_ref/libref_units.so not built (needs /root/reference)")
@pytest.mark.parametrize("n", REF_LENGTHS)
def test_model_equals_the_real_bsc_bwt_encode(n):
    for what, t in _cases(n):
        want = bm.bwt(t)
        for features in (0, bm.MULTITHREADING):
            got = bm.ref_bwt(t, features)
            assert got[0] == want[0], (n, what, features, "bytes")
            assert got[1] == want[1], (n, what, features, "primary index")
            assert np.array_equal(got[2], want[2]), (n, what, features, "indexes")


def test_model_on_a_worked_example():
    # suffixes of "banana": a(5) ana(3) anana(1) banana(0) na(4) nana(2)
    out, primary, idx = bm.bwt(b"banana")
    assert out == b"annbaa" and primary == 4
    assert list(idx) == [2, 5, 1, 4, 0]   # n / 8 = 0: step 1, rank[1 .. 5]
    assert bm.bwt(b"")[:2] == (b"", 0) and bm.bwt(b"x")[:2] == (b"x", 1)
    # the end of the string sorts below 0x00
    assert list(bm.suffix_ranks(b"a\x00\x00")) == [2, 1, 0]


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    from spring_amd import _lib
    fields = [k for k, _ in _lib.BwtInfo._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_bwt.h"\nint main(void) {\n'
                   '  printf("%zu %d", sizeof(spring_bwt_info), SPRING_BWT_MAX_INDEXES);\n'
                   + "".join('  printf(" %%zu", offsetof(spring_bwt_info, %s));\n' % k for k in fields)
                   + "  return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.BwtInfo), _lib.BWT_MAX_INDEXES] + [getattr(_lib.BwtInfo, k).offset for k in fields]
    assert got == want, (got, want)


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_bwt.h")).read()
    declared = set(re.findall(r"\b(spring_bwt_\w+)\s*\(", hdr))
    assert declared == set(_lib.BWT_EXPORTS)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert spring_amd.BwtStage is not None


HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "bwt_plan.h"
int main(int argc, char **argv) {
  for (uint32_t n = 0; n <= 70000; n++) printf("I %u %u %u\n", n, bwt::index_step(n), bwt::num_indexes(n));
  const uint32_t big[] = {1u << 20, (1u << 20) + 3, 25u << 20, (1u << 30) - 1, 1u << 30};
  for (uint32_t n : big) printf("I %u %u %u\n", n, bwt::index_step(n), bwt::num_indexes(n));
  const uint64_t segs[] = {0, 1, 2, 3, 1000, 1ull << 21, 1ull << 24};
  for (uint64_t s : segs) { bwt::KeyLayout k = bwt::key_layout(s); printf("K %llu %d %d %d\n", (unsigned long long)s, k.seg_bits, k.key_bytes, k.total_bits); }
  for (uint64_t x = 1; x <= 70000; x += 7) printf("B %llu %d %d\n", (unsigned long long)x, bwt::bits_for(x), bwt::max_rounds(x));
  // plans: argv = budget, then the segment lengths
  std::vector<uint64_t> off(1, 0);
  const uint64_t budget = strtoull(argv[1], 0, 10);
  for (int i = 2; i < argc; i++) off.push_back(off.back() + strtoull(argv[i], 0, 10));
  const uint64_t S = off.size() - 1;
  std::vector<uint64_t> first(S + 1);   // exactly the room the planner asks for
  const long long nb = bwt::plan_sub_batches(off.data(), S, budget, first.data());
  printf("P %lld", nb);
  for (long long b = 0; b <= nb; b++) printf(" %llu", (unsigned long long)first[b]);
  printf("\n");
  return 0;
}
"""


def _harness(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "plan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "spring_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return exe


def _run(exe, budget, lens):
    # leak detection needs ptrace, which not every box grants; the harness frees what it allocates anyway
    r = subprocess.run([str(exe), str(budget)] + [str(x) for x in lens], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_host_arithmetic_in_a_sanitized_host_build(tmp_path):
    exe = _harness(tmp_path)
    lens = bm.LENGTHS
    out = _run(exe, 72 * 4097 + 16, lens)
    for row in (x.split()[1:] for x in out if x.startswith("I ")):
        n, step, num = map(int, row)
        assert step == bm.index_step(n) and num == (((n - 1) // step) & 0xff if n else 0), n
        assert num == 0 or num * step <= n - 1                     # every sampled suffix exists
    for row in (x.split()[1:] for x in out if x.startswith("K ")):
        s, seg_bits, key_bytes, total = map(int, row)
        assert (1 << seg_bits) >= max(s, 1) and 1 <= key_bytes <= 7 and total == seg_bits + 8 * key_bytes + 3 <= 64
    for row in (x.split()[1:] for x in out if x.startswith("B ")):
        x, b, r = map(int, row)
        assert (1 << b) >= x and (b == 0 or (1 << (b - 1)) < x) and r == b + 2
    # the planner: whole consecutive segments, every sub-batch inside the budget, no segment left out
    for budget, ls in ((72 * 4097 + 16, lens), (10 ** 12, lens), (72 * 4097 + 16, lens[::-1]), (16, [0, 0, 0]),
                       (72 * 10 + 16, [10] * 7 + [0] * 5 + [3]), (10 ** 6, [])):
        row = [int(x) for x in [x for x in _run(exe, budget, ls) if x.startswith("P ")][0].split()[1:]]
        nb, first = row[0], row[1:]
        assert nb >= 0 and len(first) == nb + 1 and first[-1] == len(ls) and (nb == 0) == (len(ls) == 0)
        if nb:
            assert first[0] == 0 and all(a < b for a, b in zip(first, first[1:]))
        for a, b in zip(first, first[1:]):
            assert 72 * sum(ls[a:b]) + 16 * (b - a) <= budget
            if b < len(ls):                                        # greedy: the next segment did not fit
                assert 72 * sum(ls[a:b + 1]) + 16 * (b + 1 - a) > budget
    assert [x for x in _run(exe, 72 * 4097 + 16, lens) if x.startswith("P ")][0].split()[1] == "3"
    # a segment that does not fit on its own, or is above 1 GiB: refused, and which one
    assert [x for x in _run(exe, 72 * 4097 + 15, lens) if x.startswith("P ")][0].split()[1] == str(-1 - lens.index(4097))
    assert [x for x in _run(exe, 10 ** 15, [5, (1 << 30) + 1]) if x.startswith("P ")][0].split()[1] == "-2"
