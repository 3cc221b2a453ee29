"""The QLFC stage's checker (tests/qlfc_model.py) against the real bsc_coder_compress(., ., n, 1, 3) after bsc_init(3)
from oracle/_ref/libref_units.so: bytes and return value on every case, and the real bsc_coder_decompress gives the
input back.  Plus what needs no reference: the parameter table, the slot numbering, the ABI lists.  No GPU."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import qlfc_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = qm.ref_lib()
TABLES = qm.state_tables()
needs_ref = pytest.mark.skipif(REF is None or TABLES is None,
                               reason="oracle/_ref/libref_units.so not built (needs the reference sources)")


@needs_ref
def test_state_tables_are_read_from_the_library():
    rank, run = TABLES
    assert rank.shape == (qm.RANK_TABLE,) and run.shape == (qm.RUN_TABLE,)
    assert list(rank[:8]) == [224, 0, 0, 0, 0, 0, 0, 0] and list(run[:4]) == [80, 168, 115, 59]
    assert qm.state_tables(os.path.join(ROOT, "oracle", "_ref", "no_such_library.so")) is None
    assert qm.state_tables(os.path.join(ROOT, "README.md")) is None


@needs_ref
@pytest.mark.parametrize("name", qm.MODEL_CASES + qm.EDGE_CASES + qm.table_cases("real"))
def test_model_equals_bsc_coder_compress(name):
    data = qm.case(name)
    want, rc = qm.ref_compress(data)
    stats = {}
    got, grc = qm.compress(data, TABLES, stats)
    print(name, len(data), "->", rc, stats)
    assert grc == rc and got == want
    if rc > 0:
        back, drc = qm.ref_decompress(want, len(data))
        assert drc >= 0 and back == data
    else:
        assert rc == qm.NOT_COMPRESSIBLE


@needs_ref
def test_cases_reach_what_they_are_for():
    """The answers are the reference's, found here; what is pinned is which branch a case takes."""
    rc = {name: qm.ref_compress(qm.case(name))[1] for name in qm.MODEL_CASES + qm.REF_ONLY_CASES}
    for name in ("len1", "len2", "len16", "len17", "random4096"):
        assert rc[name] == qm.NOT_COMPRESSIBLE, name
    assert all(v > 0 for k, v in rc.items() if k not in ("len1", "len2", "len16", "len17", "random4096"))
    assert rc["a40"] == 13 and rc["ab32"] == 21 and rc["a300000"] == 49
    # the escape path: avgRank >= 32 on nearly every run of the 256-letter cycle
    runs, ranks, order, max_rank = qm.chunk_ranks(qm.case("all256"))
    avg, over = 0, 0
    for r in ranks:
        over += avg >= 32
        avg = (avg * 124 + r * 4) >> 7
    assert len(runs) == 8192 and over == 8156 and max_rank == 7 and len(order) == 256
    assert max(qm.log2(n) for _, n in qm.chunk_ranks(qm.case("exp16"))[0]) == 16
    assert qm.case("tail0")[-1] == 0
    # chunk rule: the equal split and the sampled cut, at two, four and eight chunks
    for name, k, equal in (("a300000", 2, True), ("bwt300000", 2, False), ("cycle4e", 4, True), ("cycle4s", 4, False),
                           ("cycle16e", 8, True), ("cycle16s", 8, False)):
        data = qm.case(name)
        cuts = qm.split(data, k)
        assert qm.num_chunks(len(data)) == k and len(cuts) == k + 1
        assert (cuts[:-1] == [len(data) // k * p for p in range(k)]) == equal, name
    # the half-random cases: one chunk stored raw, the other coded
    for name in qm.REF_ONLY_CASES:
        coded, _ = qm.ref_compress(qm.case(name))
        assert coded[0] == 2
        sizes = struct.unpack_from("<iiii", coded, 1)
        assert [sizes[0] == sizes[1], sizes[2] == sizes[3]] == ([True, False] if name == "random_a" else [False, True])
        back, drc = qm.ref_decompress(coded, len(qm.case(name)))
        assert drc >= 0 and back == qm.case(name)


def _sizes(coded):
    """-> per chunk of a coded multi-chunk segment (input size, stored size)."""
    v = struct.unpack_from("<%di" % (2 * coded[0]), coded, 1)
    return list(zip(v[0::2], v[1::2]))


@pytest.mark.parametrize("which", [pytest.param("real", marks=needs_ref), 101, 202])
def test_edge_cases_reach_what_they_are_for(which):
    """What each of EDGE_CASES and table_cases(which) is in the set for, read off the model's counters under the pair
    of tables it is compared with on the device."""
    tables = TABLES if which == "real" else qm.random_tables(which)
    out = {}
    for name in qm.EDGE_CASES + qm.table_cases(which):
        stats = {}
        coded, rc = qm.compress(qm.case(name), tables, stats)
        out[name] = (coded, rc, stats)
        print(name, len(qm.case(name)), "->", rc, stats)
    # only the margin-0 case is not compressible: everything else compares bytes
    for name, (coded, rc, _) in out.items():
        assert (rc == qm.NOT_COMPRESSIBLE and coded == b"") if name == "eob_0_%s" % which else (rc == len(coded) > 0), name
    # the range coder's pending units
    st = out["pend_n_%s" % which][2]
    assert st["pend"] >= 1 and st["flush_nocarry"] >= 1
    st = out["pend_c_%s" % which][2]
    assert st["pend"] >= 1 and st["flush_carry"] >= 1
    # the escape path below 256 symbols, maxRank 6 and 7, and going back and forth between the two rank paths
    for name, symbols, max_rank in (("esc100", 100, 6), ("esc128", 128, 6), ("esc129", 129, 7), ("ring100", 100, 6)):
        st = out[name][2]
        assert (st["symbols"], st["max_rank"]) == ([symbols], [max_rank]), name
        assert 2 * st["escaped"] > st["runs"], name
        assert st["esc_switches"] >= (100 if name == "esc100" else 1), name
    assert out["ring100"][2]["escaped"] >= 5000 - 100   # rank 99 on every run but the last hundred
    # symbol tables: 4 and 8 symbols, 255 (closed by listing the last symbol again) with either end and the middle
    # absent, 256 in descending order
    assert out["letters4"][2]["symbols"] == [4] and out["letters8"][2]["symbols"] == [8]
    for name, absent in qm.ABSENT.items():
        assert out[name][2]["symbols"] == [255] and absent not in qm.case(name), name
    assert qm.chunk_ranks(qm.case("desc256"))[2] == list(range(255, -1, -1))
    # the chunk rule around its thresholds
    for n in qm.CHUNK_SIZES:
        k = qm.num_chunks(n)
        assert k == (1 if n < 262144 else 2 if n < 4 << 20 else 4)
        data = qm.case("eq%d" % n)
        equal = [n // k * p for p in range(k)]
        assert len(data) == n and qm.split(data, k)[:-1] == equal
        assert out["eq%d" % n][2]["symbols"] == [5] * k
        if k == 1:
            assert out["eq%d" % n][0][0] == 1
            continue
        assert n % k or n == 262146                  # the equal split leaves a rest wherever the size allows one
        assert [a for a, _ in _sizes(out["eq%d" % n][0])] == [n // k] * (k - 1) + [n - n // k * (k - 1)]
        data = qm.case("smp%d" % n)
        a = np.frombuffer(data, np.uint8)
        pos = np.arange(1, n, 32)
        hits = pos[a[pos] != a[pos - 1]]
        assert len(data) == n and len(hits) == k + 1 and hits[-1] == pos[-1] >= n - 32   # one more than k, the last sample
        assert n % 32 not in (1, 2) or pos[-1] == n - 1 - (n % 32 == 1) * 31
        cuts = qm.split(data, k)
        assert cuts == [0] + [int(h) for h in hits[:k - 1]] + [n] and cuts[:-1] != equal
        assert qm.split(data[:int(pos[-1])] + bytes([data[int(pos[-1]) - 1]]) * (n - int(pos[-1])), k)[:-1] == equal
        assert [a for a, _ in _sizes(out["smp%d" % n][0])] == list(np.diff(cuts))
    # raw chunks beside coded ones
    for name, raw in (("raw_coded", [True, False]), ("coded_raw", [False, True]), ("raw4", [True, False, True, False])):
        sizes = _sizes(out[name][0])
        assert [a == b for a, b in sizes] == raw and out[name][2]["raw"] == sum(raw), name
        assert all(b < a // 8 for (a, b), r in zip(sizes, raw) if not r), name
    assert not any("raw" in out[name][2] for name in out if name not in qm.RAW_CASES)
    # CheckEOB at the last run, one unit either side
    for name, margin in (("eob_0_%s" % which, 0), ("eob_1_%s" % which, 1)):
        assert qm.num_chunks(len(qm.case(name))) == 1 and qm.last_run_margin(qm.case(name), tables) == margin
    assert out["eob_1_%s" % which][2]["margin"] == [1]


@needs_ref
def test_the_rollback_case_is_not_compressible():
    """262144 random bytes: two chunks, the first stored raw, the second fails where it can no longer be stored."""
    data = qm.case(qm.ROLLBACK_CASE)
    assert qm.num_chunks(len(data)) == 2 and qm.ref_compress(data) == (b"", qm.NOT_COMPRESSIBLE)
    cut = qm.split(data, 2)[1]
    assert qm.ref_compress(data[:cut])[1] == qm.NOT_COMPRESSIBLE and qm.ref_compress(data[cut:])[1] == qm.NOT_COMPRESSIBLE


def test_run_batches_and_many_segments_are_what_they_say():
    for counts in qm.RUN_ORDERS:
        segs = qm.run_batch(counts)
        assert [len(qm.chunk_ranks(s)[0]) for s in segs] == list(counts)
        assert all(b[0] not in a for a, b in zip(segs, segs[1:]))
        assert all(qm.compress(s, qm.random_tables(101))[1] > 0 for s in segs)
    lanes = {}
    for count, seg in zip(qm.RUN_ORDERS[1], qm.run_batch(qm.RUN_ORDERS[1])):
        stats = {}
        qm.encode_chunk(seg, len(seg) - 1, qm.random_tables(101), stats)
        lanes[count] = stats["lastev"][0] % 64
    assert lanes[63] == 63 and lanes[65] == 0
    segs = qm.many_segments()
    assert len(segs) == 1500 and [j for j, s in enumerate(segs) if not s] == list(range(99, 1500, 100))
    assert all(40 <= len(s) <= 200 and 2 <= len(set(s)) <= 4 for s in segs if s)


def test_parameter_table_and_slot_numbering():
    rows, mix = qm.params()
    assert len(rows) == 21 and len(mix) == 7
    assert rows[3 * qm.RUN_TOP + 2] == (0, 0, 0, 0) and mix[qm.RUN_TOP][2] == 0    # the run's static predictor is off
    plan = open(os.path.join(ROOT, "spring_amd", "csrc", "qlfc_plan.h")).read()
    order = re.search(r"enum Family \{([^}]*)\}", plan).group(1).replace(" ", "").split(",")
    assert tuple(order) == qm.FAMILIES
    assert int(re.search(r"CLASS_SHIFT = (\d+)", plan).group(1)) == qm.CLASS_SHIFT
    # the largest index of every family stays below the class field, so no two slots share a number
    top = {qm.RANK_TOP: (255, 0, 0), qm.RANK_EXP: (255, 0, 7), qm.RANK_MAN: (255, 7, 255), qm.RANK_ESC: (255, 0, 255),
           qm.RUN_TOP: (255, 0, 0), qm.RUN_EXP: (255, 0, 31), qm.RUN_MAN: (255, 31, 31)}
    for fam, (who, hi, lo) in top.items():
        lb = qm.LO_BITS[fam]
        assert lo < 1 << max(lb, 1) and hi << (8 + lb) | who << lb | lo < 1 << qm.CLASS_SHIFT, fam


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib, build
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_qlfc.h")).read()
    declared = set(re.findall(r"\b(spring_qlfc_\w+)\s*\(", hdr))
    assert declared == set(_lib.QLFC_EXPORTS) and len(_lib.QLFC_EXPORTS) == len(declared)
    for k in dir(_lib):
        if k.endswith("EXPORTS") and k != "QLFC_EXPORTS":
            assert not declared & set(getattr(_lib, k))
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert spring_amd.QlfcStage is not None
    assert "qlfc.hip" in build.SOURCES and "spring_qlfc.h" in build.PUBLIC_HEADERS
    assert "qlfc_plan.h" in build.HEADERS and "qlfc_params.h" in build.HEADERS


def test_info_struct_matches_the_header():
    from spring_amd import _lib
    from spring_amd.qlfc import QlfcInfo
    hdr = open(os.path.join(ROOT, "include", "spring_qlfc.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} spring_qlfc_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+)(?:\[\w+\])?;", body)
    assert [f for _, f in fields] == [k for k, _ in QlfcInfo._fields_]
    assert C.sizeof(QlfcInfo) == 8 * (len(fields) - 1 + _lib.QLFC_PASSES)
    defs = dict(re.findall(r"#define SPRING_QLFC_(\w+) \(?(-?\d+)\)?", hdr))
    assert int(defs["RANK_TABLE"]) == _lib.QLFC_RANK_TABLE == qm.RANK_TABLE
    assert int(defs["RUN_TABLE"]) == _lib.QLFC_RUN_TABLE == qm.RUN_TABLE
    assert int(defs["PASSES"]) == _lib.QLFC_PASSES and int(defs["NOT_COMPRESSIBLE"]) == _lib.QLFC_NOT_COMPRESSIBLE
    assert int(defs["EVENT_BYTES"]) == _lib.QLFC_EVENT_BYTES
    s = QlfcInfo()
    s.events, s.ms_pass[5] = 7, 1.5
    assert s.asdict()["events"] == 7 and s.asdict()["ms_pass"] == [0, 0, 0, 0, 0, 1.5]


def test_stage_lifecycle_against_a_stub(monkeypatch):
    """As tests/test_stage_frame_cpu.py does for the other stages: create, get_info, destroy, once each."""
    from spring_amd import _lib
    from spring_amd.qlfc import QlfcStage
    calls = []

    class Stub:
        def __getattr__(self, name):
            def fn(*args):
                calls.append(name)
                if name.endswith("_create"):
                    args[1]._obj.value = 0x1000
                return 0
            return fn
    monkeypatch.setattr(_lib, "lib", lambda: Stub())
    with QlfcStage() as st:
        assert st._h.value == 0x1000 and st.info is None
        assert isinstance(st.get_info(), dict) and st.info is None
    assert calls == ["spring_qlfc_create", "spring_qlfc_get_info", "spring_qlfc_destroy"] and not st._h


def test_no_state_table_in_the_tree():
    """The tables come from the caller: no source file of the package or the tests carries 8 KiB of them."""
    if TABLES is None:
        pytest.skip("the tables cannot be read without oracle/_ref")
    def window(t):   # the first 32 bytes of the table with a dozen different values among them
        return next(bytes(t[i:i + 32]) for i in range(len(t) - 32) if len(set(t[i:i + 32].tolist())) >= 12)
    probe = [window(TABLES[0]), window(TABLES[1])]
    texts = [", ".join(str(b) for b in p[:12]) for p in probe]
    for top in ("spring_amd", "tests", "include", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            if "__pycache__" in dirpath or dirpath.endswith(os.path.join("spring_amd", "lib")):
                continue
            for f in files:
                blob = open(os.path.join(dirpath, f), "rb").read()
                assert not any(p in blob for p in probe), f
                if f.endswith((".py", ".h", ".hip", ".cpp", ".md")):
                    text = re.sub(r"\s+", " ", blob.decode("utf-8", "replace"))
                    assert not any(t in text for t in texts), f
