"""CPU-only checks of the inverse block-sort stage: the numpy model of bsc_bwt_decode (tests/unbwt_model.py) against
the forward model and against the real function of oracle/_ref/libref_units.so (skipped when that is not built), the
ctypes mirror of spring_unbwt_info against the C header, the exported symbols, and the stage's host arithmetic
(spring_amd/csrc/unbwt_plan.h: head rule, round bound, budget, sub-batch planner) in a stand-alone host build under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bwt_model as bm
import unbwt_model as um
from test_bwt_cpu import REF_LENGTHS, _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("acgt", "bytes", "const", "cac", "tail00", "tailff")
POS, SEG = 34, 96   # unbwt::BYTES_PER_POS, BYTES_PER_SEG


@pytest.mark.parametrize("kind", KINDS)
def test_model_inverts_the_forward_model(kind):
    for n in bm.LENGTHS:
        t = bm.contents(kind, n, seed=5)
        out, primary, _ = bm.bwt(t)
        assert um.path_length(out, primary) == n, (kind, n)
        assert um.unbwt(out, primary) == t, (kind, n)


@pytest.mark.skipif(um.ref_lib() is None, reason="oracle/_ref/libref_units.so not built (needs /root/reference)")
@pytest.mark.parametrize("n", REF_LENGTHS + [65536])
def test_model_equals_the_real_bsc_bwt_decode(n):
    for what, t in _cases(n):
        out, primary, idx = bm.bwt(t)
        want = um.unbwt(out, primary)
        assert want == t, (n, what)
        for features in (0, bm.MULTITHREADING):
            for indexes in (None, idx):
                rc, got = um.ref_unbwt(out, primary, features, indexes)
                assert rc == 0 and got == want, (n, what, features, indexes is not None)


@pytest.mark.skipif(um.ref_lib() is None, reason="oracle/_ref/libref_units.so not built (needs /root/reference)")
def test_a_wrong_primary_with_a_complete_path_is_a_text_of_its_own():
    rc, got = um.ref_unbwt(b"annbaa", 6)
    assert rc == 0 and got == um.unbwt(b"annbaa", 6) != b"banana"
    assert um.ref_unbwt(b"annbaa", 0)[0] < 0 and um.ref_unbwt(b"annbaa", 7)[0] < 0   # out of range: refused there too


def test_model_on_a_worked_example():
    assert bm.bwt(b"banana")[:2] == (b"annbaa", 4)
    assert um.unbwt(b"annbaa", 4) == b"banana"
    assert [um.path_length(b"annbaa", p) for p in (1, 2, 3, 4, 5, 6)] == [1, 3, 5, 6, 2, 6]
    for p in (1, 2, 3, 5):
        with pytest.raises(ValueError, match="steps"):
            um.unbwt(b"annbaa", p)
    other = um.unbwt(b"annbaa", 6)   # a complete path: a different text, and its transform is the same bytes
    assert other != b"banana" and bm.bwt(other)[:2] == (b"annbaa", 6)
    for p in (0, 7, -1):
        with pytest.raises(ValueError, match="out of range"):
            um.unbwt(b"annbaa", p)
    assert um.unbwt(b"", 0) == b"" and um.unbwt(b"x", 1) == b"x"
    with pytest.raises(ValueError):
        um.unbwt(b"", 1)


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    from spring_amd import _lib
    fields = [k for k, _ in _lib.UnbwtInfo._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_unbwt.h"\nint main(void) {\n'
                   '  printf("%zu %d", sizeof(spring_unbwt_info), SPRING_UNBWT_PASSES);\n'
                   + "".join('  printf(" %%zu", offsetof(spring_unbwt_info, %s));\n' % k for k in fields)
                   + "  return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.UnbwtInfo), _lib.UNBWT_PASSES] + [getattr(_lib.UnbwtInfo, k).offset for k in fields]
    assert got == want, (got, want)
    from spring_amd import unbwt
    assert len(unbwt.PASSES) == _lib.UNBWT_PASSES


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib, build
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_unbwt.h")).read()
    declared = set(re.findall(r"\b(spring_unbwt_\w+)\s*\(", hdr))
    assert declared == set(_lib.UNBWT_EXPORTS) and len(_lib.UNBWT_EXPORTS) == len(declared)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "UNBWT_EXPORTS"]
    assert len(others) >= 7
    for lst in others:
        assert not declared & set(lst)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert spring_amd.UnbwtStage is not None
    assert "unbwt.hip" in build.SOURCES and "unbwt_plan.h" in build.HEADERS and "bwt_internal.h" in build.HEADERS
    assert "spring_unbwt.h" in build.PUBLIC_HEADERS


HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "unbwt_plan.h"
int main(int argc, char **argv) {
  for (uint64_t h = 0; h <= 70000; h++) printf("R %llu %d\n", (unsigned long long)h, unbwt::rank_rounds(h));
  const uint64_t big[] = {1ull << 20, (1ull << 20) + 1, (1ull << 24) + 4, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 4};
  for (uint64_t h : big) printf("R %llu %d\n", (unsigned long long)h, unbwt::rank_rounds(h));
  for (int lk = unbwt::LOG_K_MIN; lk <= unbwt::LOG_K_MAX; lk++) {
    // the head rule over rows 0 .. 2^20: how many heads, the widest gap between two, one regular head per block
    const uint32_t rows = (1u << 20) + 1;
    uint64_t heads = 0, gap = 0, last = 0, bad_blocks = 0;
    for (uint32_t r = 0; r < rows; r++) {
      if (!unbwt::is_head(r, r, lk)) continue;
      heads++;
      if (r - last > gap) gap = r - last;
      last = r;
    }
    for (uint32_t b = 0; b < (rows >> lk); b++) {
      const uint32_t r = unbwt::head_row(b, lk);
      if ((r >> lk) != b || !unbwt::is_regular_head(r, lk)) bad_blocks++;
    }
    printf("H %d %d %llu %llu %llu %llu\n", lk, (int)unbwt::is_head(12345u, 0, lk), (unsigned long long)heads,
           (unsigned long long)gap, (unsigned long long)bad_blocks, (unsigned long long)unbwt::regular_heads(rows, lk));
    const uint64_t ns[] = {0, 1, 63, 64, 4097, 70000, 1ull << 30};
    for (uint64_t n : ns) printf("M %d %llu %llu\n", lk, (unsigned long long)n, (unsigned long long)unbwt::max_heads_of_segment(n, lk));
  }
  const uint64_t ms[] = {0, 1, 4097, 1ull << 30, 0x7fff0000ull};
  for (uint64_t m : ms) printf("W %llu %llu %llu\n", (unsigned long long)m, (unsigned long long)unbwt::workspace_need(m, 1),
                               (unsigned long long)unbwt::workspace_need(m, 1ull << 24));
  // plans: argv = budget, then the segment lengths
  std::vector<uint64_t> off(1, 0);
  const uint64_t budget = strtoull(argv[1], 0, 10);
  for (int i = 2; i < argc; i++) off.push_back(off.back() + strtoull(argv[i], 0, 10));
  const uint64_t S = off.size() - 1;
  std::vector<uint64_t> first(S + 1);   // exactly the room the planner asks for
  const long long nb = unbwt::plan_sub_batches(off.data(), S, budget, first.data());
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


def _plan(exe, budget, lens):
    return [int(x) for x in [x for x in _run(exe, budget, lens) if x.startswith("P ")][0].split()[1:]]


def test_host_arithmetic_in_a_sanitized_host_build(tmp_path):
    exe = _harness(tmp_path)
    lens = bm.LENGTHS
    out = _run(exe, POS * 4097 + SEG, lens)
    rows = [[int(v) for v in x.split()[1:]] for x in out if x.startswith("R ")]
    assert len(rows) == 70001 + 6
    for h, r in rows:   # 2^(r - 1) pointer hops span a path of h heads, and r - 1 is the least such count
        assert (1 << (r - 1)) >= max(h, 1) and (r == 1 or (1 << (r - 2)) < h), (h, r)
    seen = 0
    for lk, row0, heads, gap, bad_blocks, regular in ([int(v) for v in x.split()[1:]] for x in out if x.startswith("H ")):
        K = 1 << lk
        n = (1 << 20) + 1
        assert row0 == 1                                           # row 0 of a segment is a head wherever it lies
        assert n / (2 * K) <= heads <= 2 * n / K, (K, heads)      # within a factor 2 of one in K
        assert gap <= 2 * K - 1 and bad_blocks == 0 and regular == (n + K - 1) // K
        seen += 1
    assert seen == 7
    for lk, n, mh in ([int(v) for v in x.split()[1:]] for x in out if x.startswith("M ")):
        assert mh >= -(-(n + 1) // (1 << lk)) + 1 + 2              # the blocks n + 1 rows can touch, row 0, primary row
    for m, w1, wmany in ([int(v) for v in x.split()[1:]] for x in out if x.startswith("W ")):
        assert w1 == POS * m + SEG and wmany == POS * m + SEG * (1 << 24)
    # the planner: whole consecutive segments, every sub-batch inside the budget, no segment left out
    for budget, ls in ((POS * 4097 + SEG, lens), (10 ** 12, lens), (POS * 4097 + SEG, lens[::-1]), (SEG, [0, 0, 0]),
                       (POS * 10 + SEG, [10] * 7 + [0] * 5 + [3]), (10 ** 6, [])):
        row = _plan(exe, budget, ls)
        nb, first = row[0], row[1:]
        assert nb >= 0 and len(first) == nb + 1 and first[-1] == len(ls) and (nb == 0) == (len(ls) == 0)
        if nb:
            assert first[0] == 0 and all(a < b for a, b in zip(first, first[1:]))
        for a, b in zip(first, first[1:]):
            assert POS * sum(ls[a:b]) + SEG * (b - a) <= budget
            if b < len(ls):                                        # greedy: the next segment did not fit
                assert POS * sum(ls[a:b + 1]) + SEG * (b + 1 - a) > budget
    assert _plan(exe, POS * 4097 + SEG, lens)[0] == 3
    # a segment that does not fit on its own, or is above 1 GiB: refused, and which one
    assert _plan(exe, POS * 4097 + SEG - 1, lens)[0] == -1 - lens.index(4097)
    assert _plan(exe, 10 ** 15, [5, (1 << 30) + 1])[0] == -2
