"""The reverse complement of a consensus, limb by limb (spring_amd/csrc/strand_filter.h: rc_limb, rc_limb_bitpos) on the host.
The four-chain round kernel no longer keeps a chain's reverse consensus: it rebuilds it from the forward one with this
arithmetic (reorder_round_mc.h: revref_limb), one 64-bit window of the zero-padded limbs per limb.  The header is compiled
into a small stand-alone program that does exactly that for every consensus length R in 1 .. 192 on random limbs, and this
test compares the limbs with a plain per-base reverse complement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WMAX, PAD = 6, 4  # limbs of a read of up to 192 bases; zero limbs either side (GLds)

PROG = r"""
#include <cinttypes>
#include <cstdio>
#include "strand_filter.h"
static const int WMAX = 6, PAD = 4;
// 64 bits from bit `bitpos` of the limbs (the kernel's lds_window)
static uint64_t window(const uint64_t *s, int bitpos) {
  const int li = bitpos >> 6, off = bitpos & 63;
  const uint64_t lo = s[li], hi = s[li + 1];
  return off ? (lo >> off) | (hi << (64 - off)) : lo;
}
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int R;
  while (fscanf(f, "%d", &R) == 1) {
    uint64_t buf[WMAX + 2 * PAD] = {0};
    for (int i = 0; i < WMAX; i++)
      if (fscanf(f, "%" SCNu64, &buf[PAD + i]) != 1) return 3;
    for (int j = 0; j < WMAX; j++) {
      const uint64_t rl = 32 * j < R ? sf::rc_limb(window(buf + PAD, sf::rc_limb_bitpos(R, j)), R - 32 * j) : 0ull;
      printf("%" PRIu64 "%c", rl, j == WMAX - 1 ? '\n' : ' ');
    }
  }
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("revref")
    src, exe = str(d / "revref_check.cpp"), str(d / "revref_check")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "spring_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def _limbs_of(codes):
    out = [0] * WMAX
    for p, c in enumerate(codes):
        out[p >> 5] |= int(c) << (2 * (p & 31))
    return out


def _cases(rng):
    """(R, limbs, the bases [0, R)).  No window reaches past base R (limb j reads the bases [R - 32 - 32 j, R - 32 j)), so
    the first case of every length has random bases above R as well: the answer must be that of the first R bases alone."""
    for R in range(1, 32 * WMAX + 1):
        for rep in range(3):
            full = rng.integers(0, 4, 32 * WMAX)
            if rep == 1:
                full[:R], full[R:] = 3, 0  # all T: the complement is all zero bits
            if rep == 2:
                full[:R], full[R:] = 0, 0  # all A: the complement is all ones, the mask must cut at R
            yield R, _limbs_of(full), full[:R].copy()


def test_every_length(prog, tmp_path):
    rng = np.random.default_rng(20261)
    cases = list(_cases(rng))
    p = tmp_path / "in.txt"
    p.write_text("".join("%d %s\n" % (R, " ".join(str(x) for x in limbs)) for R, limbs, _ in cases))
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    for (R, _, codes), got in zip(cases, rows):
        want = _limbs_of((3 - codes)[::-1])  # per base: position i of the reverse complement = 3 - base R - 1 - i
        assert got == want, (R, got, want)
