"""The arithmetic of the strand-symmetric presence table (spring_amd/csrc/strand_filter.h) on the host: the header is compiled
into a small stand-alone program (its own main, host sanitizers where the compiler has them) that evaluates the functions
on vectors written by this test, and the answers are compared with a numpy model written independently here: the window
reverse complement, canon, the flag a key sets, hash / bucket / fingerprint, and what a bucket's four slot words prove."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <cinttypes>
#include <cstdio>
#include "strand_filter.h"
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'w') {  // window: wl, W, lgb
      int wl, lgb;
      uint64_t w;
      if (fscanf(f, "%d %" SCNu64 " %d", &wl, &w, &lgb) != 3) return 3;
      bool sw;
      const uint64_t r = sf::rc_window(w, wl), c = sf::canon(w, wl, sw), h = sf::mix64(c);
      printf("w %" PRIu64 " %" PRIu64 " %d %u %u %" PRIu64 " %u %u\n", r, c, sw ? 1 : 0, sf::flags_of_key(w, wl, 0),
             sf::flags_of_key(w, wl, 1), h, sf::bucket_of(h, lgb), sf::fp_of(h));
    } else if (kind == 'b') {  // bucket: four slot words, fingerprint, swapped
      uint32_t s[4], fp;
      int sw;
      if (fscanf(f, "%u %u %u %u %u %d", &s[0], &s[1], &s[2], &s[3], &fp, &sw) != 6) return 3;
      const uint32_t a = sf::absent_of(s[0], s[1], s[2], s[3], fp);
      printf("b %u %u\n", a, sf::to_window_frame(a, sw != 0));
    } else return 3;
  }
  fclose(f);
  return 0;
}
"""

M64 = (1 << 64) - 1


def _rc(w, wl):  # 2 bits a base, base 0 in bits 0-1; complement of code c is 3 - c
    out = 0
    for i in range(wl):
        out |= (3 - ((w >> (2 * i)) & 3)) << (2 * (wl - 1 - i))
    return out


def _mix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def _absent(s, fp):
    """canonical frame: nothing unless the bucket is not full; then every flag that the fingerprint's slot (if any) has clear"""
    if s[3] != 0:
        return 0
    flags = 0
    for v in s:
        if v >> 4 == fp:
            flags |= v & 15
    return ~flags & 15


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sfcpu")
    src, exe = str(d / "sf_check.cpp"), str(d / "sf_check")
    with open(src, "w") as f:
        f.write(PROG)
    base = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "spring_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:  # (a compiler without the sanitizer runtimes: the plain program checks the same answers)
        subprocess.run(base, check=True)
    return exe


def _ask(prog, tmp_path, lines):
    p = tmp_path / "in.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.mark.parametrize("wl", [6, 20, 32])
def test_windows(prog, tmp_path, wl):
    rng = np.random.default_rng(wl)
    mask = (1 << (2 * wl)) - 1
    ws = [int(x) & mask for x in rng.integers(0, 1 << 63, 300, dtype=np.uint64) * 2 + rng.integers(0, 2, 300, dtype=np.uint64)]
    half = [int(x) & ((1 << wl) - 1) for x in rng.integers(0, 1 << 62, 60, dtype=np.uint64)]
    pals = [h | (_rc(h, wl // 2) << wl) for h in half]  # x + rc(x)
    ws += pals + [0, mask, 1, mask - 1]
    ws += [_rc(w, wl) for w in ws[:100]]
    lgbs = [0, 1, 4, 10, 28, 32]
    out = _ask(prog, tmp_path, ["w %d %d %d" % (wl, w, lgbs[i % len(lgbs)]) for i, w in enumerate(ws)])
    assert len(out) == len(ws)
    npal = 0
    for i, (w, o) in enumerate(zip(ws, out)):
        lgb = lgbs[i % len(lgbs)]
        r, c, sw, f0, f1, h, bk, fp = (int(x) for x in o[1:])
        rr = _rc(w, wl)
        assert r == rr and _rc(r, wl) == w, (wl, w)                 # the model's rc; rc o rc = id
        assert c == min(w, rr) and sw == (1 if rr < w else 0)
        pal = w == rr
        npal += pal
        assert f0 == (5 if pal else (1 if w < rr else 4)) and f1 == 2 * f0  # own strand's bit; both for a palindrome
        assert h == _mix64(c)
        assert bk == (h >> (64 - lgb) if lgb else 0) and bk < (1 << lgb)
        assert fp == ((h & 0x0fffffff) or 1) and 0 < fp < (1 << 28)
    assert npal >= len(pals)
    # canon(W) == canon(rc W), and the two strands' flags are each other's mirror
    by_w = {w: o for w, o in zip(ws, out)}
    for w in ws[:100]:
        a, b = by_w[w], by_w[_rc(w, wl)]
        assert a[2] == b[2] and a[6] == b[6]
        fa, fb = int(a[4]), int(b[4])
        assert fb == ((fa >> 2) | (fa << 2)) & 15


def test_slot_and_flag_arithmetic(prog, tmp_path):
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(600):
        fp = int(rng.integers(1, 1 << 28))
        k = int(rng.integers(0, 5))  # claimed slots (slots fill in order)
        s = [0, 0, 0, 0]
        for j in range(k):
            other = int(rng.integers(1, 1 << 28))
            s[j] = (other << 4) | int(rng.integers(0, 16))
        if k and rng.random() < 0.6:
            s[int(rng.integers(0, k))] = (fp << 4) | int(rng.integers(0, 16))
        cases.append((s, fp, int(rng.integers(0, 2))))
    cases.append(([0, 0, 0, 0], 1, 0))
    cases.append(([(5 << 4) | 15, 0, 0, 0], 5, 1))
    cases.append(([(5 << 4), (6 << 4) | 3, (7 << 4) | 1, (5 << 4) | 9], 5, 0))  # full: nothing, whatever the slots say
    out = _ask(prog, tmp_path, ["b %d %d %d %d %d %d" % (*s, fp, sw) for s, fp, sw in cases])
    assert len(out) == len(cases)
    for (s, fp, sw), o in zip(cases, out):
        a = _absent(s, fp)
        assert int(o[1]) == a, (s, fp)
        assert int(o[2]) == ((((a >> 2) | (a << 2)) & 15) if sw else a)
        if s[3] != 0:
            assert int(o[1]) == 0  # a full bucket proves nothing
    # the flag mapping end to end: a key W of dictionary l entered under canon(W) is "not absent" for exactly (W, l)
    for wl in (6, 20, 32):
        mask = (1 << (2 * wl)) - 1
        for w in [int(x) & mask for x in rng.integers(0, 1 << 63, 20, dtype=np.uint64)]:
            rr = _rc(w, wl)
            for l in (0, 1):
                flag = (1 << l if w <= rr else 0) | (4 << l if rr <= w else 0)
                a = _absent([(9 << 4) | flag, 0, 0, 0], 9)
                aw = (((a >> 2) | (a << 2)) & 15) if rr < w else a
                assert not (aw >> l) & 1                      # W itself: not proven absent from l
                assert (aw >> (1 - l)) & 1                    # ... but from the other dictionary
                assert ((aw >> (2 + l)) & 1) == (0 if w == rr else 1)  # rc(W): absent unless W is its own reverse complement
