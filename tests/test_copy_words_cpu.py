"""CPU-only checks of spring_amd/csrc/copy_words.h, the helpers of the destination-driven copies (fetch, last_le, put16):
a stand-alone host build under the address and undefined-behaviour sanitizers runs the code the kernels run and compares
it with byte loops and linear scans.  Two device instructions have host stand-ins and are not what this program runs:
the 16-byte load of ld16 is a memcpy here, and put16 stores a whole word byte by byte as it does a partial one.  Every
source of fetch is a heap block of exactly `limit` bytes, so a read past the limit ends the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "copy_words.h"

using sr::u128;

static int bad = 0;   // of the running check; the first few are printed
#define BAD(...) do { if (bad++ < 5) { printf("BAD " __VA_ARGS__); printf("\n"); } } while (0)

// a 16-byte-aligned heap block of exactly n bytes (aligned_alloc takes whole multiples of the alignment only)
static uint8_t *exact(uint64_t n) {
  void *p = nullptr;
  if (posix_memalign(&p, 16, n)) abort();
  return (uint8_t *)p;
}

// ---- fetch: every offset in a word, every count, every limit from "ends with the bytes" to "a whole word behind them"
static void check_fetch() {
  long cases = 0, second_partial = 0, first_partial = 0;
  bad = 0;
  for (uint64_t base = 0; base <= 16; base += 16)
    for (uint32_t sh = 0; sh < 16; sh++)
      for (uint32_t c = 1; c <= 16; c++)
        for (uint64_t extra = 0; extra <= 17; extra++) {
          const uint64_t a = base + sh, limit = a + c + extra;
          uint8_t *t = exact(limit);
          for (uint64_t i = 0; i < limit; i++) t[i] = (uint8_t)((i * 37 + 11) | 1);   // no zero byte: the mask shows
          const u128 got = sr::fetch(t, a, c, limit);
          u128 want = 0;
          for (uint32_t i = 0; i < c; i++) want |= (u128)t[a + i] << (8 * i);
          if (got != want)
            BAD("fetch a=%llu c=%u limit=%llu: got %016llx%016llx want %016llx%016llx", (unsigned long long)a, c,
                (unsigned long long)limit, (unsigned long long)(got >> 64), (unsigned long long)got,
                (unsigned long long)(want >> 64), (unsigned long long)want);
          cases++;
          if (sh + c > 16 && limit < base + 32) second_partial++;   // first aligned word whole, second the partial last one
          if (limit < base + 16) first_partial++;
          free(t);
        }
  printf("fetch %ld %ld %ld %d\n", cases, second_partial, first_partial, bad);
}

// ---- last_le against a linear scan
template <class I>
static void check_last_le(const char *width) {
  long cases = 0;
  bad = 0;
  const I sizes[6] = {1, 2, 3, 64, 65, 1025};
  for (I n : sizes)
    for (int shape = 0; shape < 5; shape++) {
      // shape 0: strictly increasing; 1, 2, 3: a run of equal keys at the front, in the middle, at the end; 4: all three
      std::vector<I> key(n);
      const I run = n < 4 ? 1 : n / 4;
      I v = 7;
      for (I i = 0; i < n; i++) {
        // key[i] == key[i - 1] inside a run
        const bool front = i > 0 && i <= run, mid = i > n / 2 && i <= n / 2 + run, end = i > 0 && i + run >= n;
        const bool flat = (shape == 1 && front) || (shape == 2 && mid) || (shape == 3 && end) ||
                          (shape == 4 && (front || mid || end));
        if (i && !flat) v += 3;
        key[i] = v;
      }
      std::vector<I> xs;
      for (I i = 0; i < n; i++) { xs.push_back(key[i]); xs.push_back(key[i] + 1); }   // a key; between two keys
      xs.push_back(key[n - 1] + 5);                                                   // above the last
      for (I x : xs) {
        I want = 0;
        for (I i = 0; i < n; i++) if (key[i] <= x) want = i;
        const I by_ptr = sr::last_le(n, x, key.data());
        const I by_key = sr::last_le(n, x, [&](I i) { return key[i]; });
        if (by_ptr != want || by_key != want)
          BAD("last_le %s n=%llu shape=%d x=%llu: pointer %llu callable %llu want %llu", width, (unsigned long long)n, shape,
              (unsigned long long)x, (unsigned long long)by_ptr, (unsigned long long)by_key, (unsigned long long)want);
        cases++;
        // the shifted-key form: the same search inside [lo, hi], for the x that key(lo) does not exceed
        const I lo = n / 3, hi = n - 1 - n / 5;
        if (key[lo] <= x) {
          I w2 = lo;
          for (I i = lo; i <= hi; i++) if (key[i] <= x) w2 = i;
          const I got = lo + sr::last_le((I)(hi - lo + 1), x, [&](I i) { return key[lo + i]; });
          if (got != w2)
            BAD("last_le %s shifted n=%llu shape=%d x=%llu [%llu, %llu]: got %llu want %llu", width, (unsigned long long)n, shape,
                (unsigned long long)x, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)got,
                (unsigned long long)w2);
          cases++;
        }
      }
    }
  printf("last_le %s %ld %d\n", width, cases, bad);
}

// ---- put16: 16 guard bytes, then exactly nb bytes to the end of the heap block
static void check_put16() {
  long cases = 0;
  bad = 0;
  u128 acc = 0;
  for (int i = 0; i < 16; i++) acc |= (u128)(0x51 + 9 * i) << (8 * i);
  for (uint32_t nb = 1; nb <= 16; nb++) {
    uint8_t *out = exact(16 + nb);
    for (uint32_t i = 0; i < 16 + nb; i++) out[i] = 0xA5;
    sr::put16(out, 16, nb, acc);
    for (uint32_t i = 0; i < 16; i++)
      if (out[i] != 0xA5) BAD("put16 nb=%u: byte %d in front changed", nb, (int)i - 16);
    for (uint32_t i = 0; i < nb; i++)
      if (out[16 + i] != (uint8_t)(0x51 + 9 * i)) BAD("put16 nb=%u: byte %u is %02x", nb, i, out[16 + i]);
    free(out);
    // and in the middle of a buffer: nothing behind the nb bytes changes
    uint8_t mid[48];
    for (int i = 0; i < 48; i++) mid[i] = 0xA5;
    sr::put16(mid, 16, nb, acc);
    for (uint32_t i = 0; i < 48; i++) {
      const bool inside = i >= 16 && i < 16 + nb;
      if (mid[i] != (inside ? (uint8_t)(0x51 + 9 * (i - 16)) : 0xA5)) BAD("put16 nb=%u: byte %u of the guarded buffer is %02x", nb, i, mid[i]);
    }
    cases++;
  }
  printf("put16 %ld %d\n", cases, bad);
}

int main() {
  check_fetch();
  check_last_le<uint32_t>("u32");
  check_last_le<uint64_t>("u64");
  check_put16();
  return 0;
}
"""


@pytest.fixture(scope="module")
def words_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("copy_words")
    src, exe = d / "words.cpp", d / "words"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "spring_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")   # the harness frees what it allocates
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def _bad(out, what):
    return [x for x in out if x.startswith("BAD " + what)]


def _row(out, *tags):
    row, = [x.split()[len(tags):] for x in out if x.split()[:len(tags)] == list(tags)]
    return [int(v) for v in row]


def test_fetch_equals_a_byte_loop_and_stays_below_the_limit(words_out):
    assert _bad(words_out, "fetch") == []
    cases, second_partial, first_partial, bad = _row(words_out, "fetch")
    assert bad == 0
    assert cases == 2 * 16 * 16 * 18
    assert second_partial > 0 and first_partial > 0   # both words of a source met as its partial last one


@pytest.mark.parametrize("width", ["u32", "u64"])
def test_last_le_equals_a_linear_scan(words_out, width):
    assert _bad(words_out, "last_le " + width) == []
    cases, bad = _row(words_out, "last_le", width)
    assert bad == 0
    # 6 sizes x 5 shapes x (2 n + 1) values of x, and the sub-range searches on top
    assert cases > 5 * sum(2 * n + 1 for n in (1, 2, 3, 64, 65, 1025))


def test_put16_writes_its_bytes_and_no_other(words_out):
    assert _bad(words_out, "put16") == []
    assert _row(words_out, "put16") == [16, 0]
