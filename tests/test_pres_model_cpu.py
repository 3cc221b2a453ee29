"""tests/pres_model.py, the numpy model the presence-table build is checked against on the GPU, pinned to the arithmetic the
build itself uses: spring_amd/csrc/strand_filter.h is compiled for the host into a small stand-alone program, and both
answer the same windows -- reverse complement, canonical form, flags, hash, bucket, fingerprint.  Then the model's table
checker is tried on tables made here by the insert rule in plain Python: it accepts them in any insertion order and refuses
each kind of damage it is there to find."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pres_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <cinttypes>
#include <cstdio>
#include "strand_filter.h"
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int wl, lgb;
  uint64_t w;
  while (fscanf(f, "%d %" SCNu64 " %d", &wl, &w, &lgb) == 3) {
    uint32_t f0, f1;
    const uint64_t c = sf::canon_and_flags(w, wl, 0, f0), h = sf::mix64(c);
    (void)sf::canon_and_flags(w, wl, 1, f1);
    printf("%" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " %u %u\n", sf::rc_window(w, wl), c, f0, f1, h, sf::bucket_of(h, lgb), sf::fp_of(h));
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
    d = tmp_path_factory.mktemp("presmodel")
    src, exe = str(d / "pres_check.cpp"), str(d / "pres_check")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "spring_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def _windows(rng, wl, count):
    mask = (1 << (2 * wl)) - 1
    ws = [int(x) & mask for x in rng.integers(0, 1 << 63, count, dtype=np.uint64) * 2 + rng.integers(0, 2, count, dtype=np.uint64)]
    half = np.array([int(x) & ((1 << wl) - 1) for x in rng.integers(0, 1 << 62, count // 5, dtype=np.uint64)], dtype=np.uint64)
    if wl % 2 == 0:  # palindromes: x + rc(x)
        ws += [int(a) | (int(b) << wl) for a, b in zip(half, pm.rc_window(half, wl // 2))]
    ws += [0, mask, 1, mask - 1]
    ws += [int(x) for x in pm.rc_window(np.array(ws[:count // 3], dtype=np.uint64), wl)]
    return ws


@pytest.mark.parametrize("wl", [6, 20, 21, 32])
def test_model_equals_header(prog, tmp_path, wl):
    rng = np.random.default_rng(100 + wl)
    ws = _windows(rng, wl, 400)
    lgbs = [0, 1, 4, 10, 11, 17, 28, 32]
    p = tmp_path / "in.txt"
    p.write_text("".join("%d %d %d\n" % (wl, w, lgbs[i % len(lgbs)]) for i, w in enumerate(ws)))
    r = subprocess.run([prog, str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = np.array([[int(x) for x in ln.split()] for ln in r.stdout.splitlines()], dtype=object)
    assert rows.shape == (len(ws), 7)
    w = np.array(ws, dtype=np.uint64)
    c0, f0 = pm.canon_and_flags(w, wl, 0)
    c1, f1 = pm.canon_and_flags(w, wl, 1)
    h = pm.mix64(c0)
    assert np.array_equal(c0, c1)
    assert [int(x) for x in pm.rc_window(w, wl)] == list(rows[:, 0])
    assert [int(x) for x in c0] == list(rows[:, 1])
    assert [int(x) for x in f0] == list(rows[:, 2]) and [int(x) for x in f1] == list(rows[:, 3])
    assert [int(x) for x in h] == list(rows[:, 4])
    for lgb in lgbs:
        sel = np.arange(len(ws)) % len(lgbs) == lgbs.index(lgb)
        assert [int(x) for x in pm.bucket_of(h[sel], lgb)] == list(rows[sel, 5])
    assert [int(x) for x in pm.fp_of(h)] == list(rows[:, 6])
    assert int((f0 == 5).sum()) >= (80 if wl % 2 == 0 else 0)  # the palindromes set both strands' bits


def _insert_all(keys, wl, lgb, order_seed):
    """The insert rule of strand_filter.h, one key at a time, in a random order of the (key, dictionary) pairs."""
    items = []
    for l in (0, 1):
        c, f = pm.canon_and_flags(keys[l], wl, l)
        h = pm.mix64(c)
        items += list(zip(pm.bucket_of(h, lgb).tolist(), pm.fp_of(h).tolist(), f.tolist()))
    rng = np.random.default_rng(order_seed)
    slots = np.zeros((1 << lgb, 4), np.uint32)
    dropped = 0
    for i in rng.permutation(len(items)):
        b, fp, fl = items[i]
        for s in range(4):
            if slots[b, s] == 0:
                slots[b, s] = (fp << 4) | fl
                break
            if slots[b, s] >> 4 == fp:
                slots[b, s] |= fl
                break
        else:
            dropped += 1
    return slots, dropped


@pytest.mark.parametrize("wl,lgb", [(32, 12), (20, 6), (6, 4), (32, 0)])
def test_checker_accepts_any_order_and_finds_damage(wl, lgb):
    rng = np.random.default_rng(7 * wl + lgb)
    ws = np.array(_windows(rng, wl, 300), dtype=np.uint64)
    keys = [np.unique(ws[::2]), np.unique(np.concatenate([ws[1::2], pm.rc_window(ws[:60:2], wl)]))]
    for seed in (1, 2):
        slots, dropped = _insert_all(keys, wl, lgb, seed)
        info = pm.check_table(slots, lgb, keys, wl, dropped)
        assert info["keys"] == len(keys[0]) + len(keys[1])
    assert (dropped > 0) == (lgb <= 6)  # (about 470 keys: 4 096 buckets hold them all, 64 buckets of four slots cannot)
    with pytest.raises(AssertionError):
        pm.check_table(slots, lgb, keys, wl, dropped + 1)
    b = int(np.nonzero(slots[:, 0])[0][0])
    bad = slots.copy()
    bad[b, 0] ^= np.uint32(1 << 9)  # another fingerprint: a slot no key explains (and its key is gone)
    with pytest.raises(AssertionError):
        pm.check_table(bad, lgb, keys, wl, dropped)
    bad = slots.copy()
    bad[b, 0] = (bad[b, 0] & ~np.uint32(15)) | np.uint32(~int(bad[b, 0]) & 15)  # other flags
    with pytest.raises(AssertionError):
        pm.check_table(bad, lgb, keys, wl, dropped)
    if not slots[:, 3].all():  # stale memory in a bucket's free slot
        b = int(np.nonzero(slots[:, 3] == 0)[0][0])
        bad = slots.copy()
        bad[b, 3] = 0x12345670
        with pytest.raises(AssertionError):
            pm.check_table(bad, lgb, keys, wl, dropped)
        if slots[b, 0]:
            bad = slots.copy()
            bad[b, 0] = 0  # a key lost from a bucket that is not full; an empty slot in front of a taken one
            with pytest.raises(AssertionError):
                pm.check_table(bad, lgb, keys, wl, dropped)
