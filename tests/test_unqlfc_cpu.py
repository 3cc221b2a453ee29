"""The QLFC decoder's checker (tests/unqlfc_model.py): it gives back what tests/qlfc_model.py coded, under libbsc's state
tables and under two seeded random pairs; it equals the real bsc_coder_decompress(., ., 1, 3) from
oracle/_ref/libref_units.so on what the real bsc_coder_compress wrote; it reads every payload exactly to its end; and
every malformed construction gives the violation the rules name.  Plus what needs no reference: the layout of the
predictors and the ABI lists.  No GPU."""
import ctypes as C
import functools
import os
import re

import pytest

import qlfc_model as qm
import unqlfc_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = qm.ref_lib()
TABLES = qm.state_tables()
needs_ref = pytest.mark.skipif(REF is None or TABLES is None,
                               reason="oracle/_ref/libref_units.so not built (needs the reference sources)")
WHICH = [pytest.param("real", marks=needs_ref), 101, 202]
CASES = qm.MODEL_CASES + qm.EDGE_CASES
NOT_CODED = ("len1", "len2", "len16", "len17", "random4096")   # the real coder leaves no bytes of these to decode


@functools.lru_cache(maxsize=None)
def _tables(which):
    return TABLES if which == "real" else qm.random_tables(which)


def _exact(stats):
    """Every coded chunk was read exactly to its end."""
    return stats.get("units", 0) == sum(stats.get("payload_units", []))


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", CASES)
def test_model_gives_back_what_the_model_coded(name, which):
    data = qm.case(name)
    coded, rc = qm.compress(data, _tables(which))
    if rc == qm.NOT_COMPRESSIBLE:                      # one chunk that CheckEOB stopped: coded to its end all the same
        assert qm.num_chunks(len(data)) == 1
        coded = um.payload(data, _tables(which))
    stats = {}
    back, violation = um.decompress(coded, len(data), _tables(which), stats)
    print(name, which, len(data), len(coded), stats.get("runs"), stats.get("events"), stats.get("units"))
    assert violation is None and back == data
    assert _exact(stats)
    assert stats.get("raw", 0) == (dict(raw_coded=1, coded_raw=1, raw4=2).get(name, 0) if rc > 0 else 0)


@needs_ref
@pytest.mark.parametrize("name", tuple(n for n in CASES if n not in NOT_CODED) + qm.REF_ONLY_CASES)
def test_model_equals_bsc_coder_decompress(name):
    data = qm.case(name)
    coded, rc = qm.ref_compress(data)
    assert rc == len(coded) > 0
    want, drc = qm.ref_decompress(coded, len(data))
    stats = {}
    got, violation = um.decompress(coded, len(data), TABLES, stats)
    assert drc == len(data) and violation is None and got == want == data
    assert _exact(stats)
    if name in qm.REF_ONLY_CASES:                      # a raw chunk in front of a coded one, and behind one
        assert stats["raw"] == 1 and len(stats["payload_units"]) == 1


def test_cases_reach_what_they_are_for():
    t = _tables(101)
    stats = {}
    um.decompress(qm.compress(qm.case("a40"), t)[0], 40, t, stats)
    assert (stats["runs"], stats["events"], stats["max_exp"]) == (1, 12, 5)      # one symbol: the table ends at rank 1
    for name, exp in (("a300000", 17), ("exp16", 16)):
        stats = {}
        um.decompress(qm.compress(qm.case(name), t)[0], len(qm.case(name)), t, stats)
        assert stats["max_exp"] == exp, name
    stats = {}
    um.decompress(qm.compress(qm.case("ring100"), t)[0], 5000, t, stats)
    assert stats["escaped"] >= 4900
    for which in (101, 202) + (("real",) if TABLES is not None else ()):
        for kind, rest in (("last", 0), ("first", 1)):
            n, seed = um.UNIT_CASES[which][kind]
            data = qm._letters(n, 9, seed)
            stats = {}
            back, violation = um.decompress(um.payload(data, _tables(which)), n, _tables(which), stats)
            assert violation is None and back == data and _exact(stats)
            assert stats["payload_units"][0] % 64 == rest and stats["payload_units"][0] > 64, (which, kind)
    data, starts = um.aligned_runs()
    assert sorted({(n, p % 16) for n, p in starts}) == [(n, o) for n in um.RUN_LENGTHS for o in range(16)]
    assert all(data[p - 1] != data[p] and data[p:p + n] == data[p:p + 1] * n and data[p + n:p + n + 1] != data[p:p + 1]
               for n, p in starts)
    for n in (1, 2, 16, 17):                           # lengths bsc_coder_compress refuses and the format allows
        assert qm.compress(qm.case("len%d" % n), t)[1] == qm.NOT_COMPRESSIBLE
        assert um.decompress(um.payload(qm.case("len%d" % n), t), n, t) == (qm.case("len%d" % n), None)


@pytest.mark.parametrize("which", WHICH)
def test_every_malformed_construction_gives_its_violation(which):
    t = _tables(which)
    cases = um.malformed(t)
    assert {v for _, _, v in cases.values()} == set(um.VIOLATIONS)
    for name, (coded, n, want) in cases.items():
        out, violation = um.decompress(coded, n, t)
        print(name, len(coded), n, "->", violation, len(out))
        assert violation == want, name
        assert len(out) <= n, name
    assert um.decompress(b"", 0, t) == (b"", "chunks")


@pytest.mark.parametrize("which", WHICH)
def test_a_flipped_bit_is_a_violation_or_other_bytes_of_the_right_length(which):
    t = _tables(which)
    data = qm.case("letters5")
    good = qm.compress(data, t)[0]
    seen = set()
    for bit in range(8):
        coded = bytearray(good)
        coded[len(good) // 2] ^= 1 << bit
        out, violation = um.decompress(bytes(coded), len(data), t)
        assert (violation in um.VIOLATIONS and len(out) <= len(data)) or (violation is None and len(out) == len(data))
        assert out != data
        seen.add(violation)
    print(which, seen)


def test_predictor_layout_holds_every_place():
    plan = open(os.path.join(ROOT, "spring_amd", "csrc", "unqlfc_plan.h")).read()
    hdr = open(os.path.join(ROOT, "include", "spring_unqlfc.h")).read()
    places = {qm.RANK_TOP: 1, qm.RANK_EXP: 8, qm.RANK_MAN: 256, qm.RANK_ESC: 256, qm.RUN_TOP: 1, qm.RUN_EXP: 32, qm.RUN_MAN: 1024}
    entries = 513 * sum(places.values())
    assert int(re.search(r"#define SPRING_UNQLFC_MODEL_BYTES (\d+)", hdr).group(1)) == (2 * entries + 255) // 256 * 256
    # the places of a family do not collide and stay below its count
    man = [(1 << e) - e - 2 + ctx for e in range(1, 8) for ctx in range(1, 1 << e)]
    assert len(set(man)) == len(man) and max(man) < places[qm.RANK_MAN] and min(man) == 0
    run = [e << 5 | ctx for e in range(1, 32) for ctx in range(1, 32 if e <= 5 else e + 1)]
    assert len(set(run)) == len(run) and max(run) < places[qm.RUN_MAN]
    assert [v for v in um.VIOLATIONS] == re.search(r'"none", (.*?)\}', plan).group(1).replace('"', "").split(", ")


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib, build
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_unqlfc.h")).read()
    declared = set(re.findall(r"\b(spring_unqlfc_\w+)\s*\(", hdr))
    assert declared == set(_lib.UNQLFC_EXPORTS) and len(_lib.UNQLFC_EXPORTS) == len(declared)
    for k in dir(_lib):
        if k.endswith("EXPORTS") and k != "UNQLFC_EXPORTS":
            assert not declared & set(getattr(_lib, k))
    L = _lib.lib()
    for name in sorted(declared) + ["spring_unbwt_from_unqlfc"]:
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert "spring_unbwt_from_unqlfc" in _lib.UNBWT_EXPORTS
    assert spring_amd.UnqlfcStage is not None
    assert "unqlfc.hip" in build.SOURCES and "spring_unqlfc.h" in build.PUBLIC_HEADERS and "unqlfc_plan.h" in build.HEADERS


def test_info_struct_matches_the_header():
    from spring_amd import _lib
    from spring_amd.unqlfc import PASSES, UnqlfcInfo
    hdr = open(os.path.join(ROOT, "include", "spring_unqlfc.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} spring_unqlfc_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+)(?:\[\w+\])?;", body)
    assert [f for _, f in fields] == [k for k, _ in UnqlfcInfo._fields_]
    assert C.sizeof(UnqlfcInfo) == 8 * (len(fields) - 1 + _lib.UNQLFC_PASSES)
    defs = dict(re.findall(r"#define SPRING_UNQLFC_(\w+) \(?(-?\d+)\)?", hdr))
    assert int(defs["PASSES"]) == _lib.UNQLFC_PASSES == len(PASSES)
    assert int(defs["MODEL_BYTES"]) == _lib.UNQLFC_MODEL_BYTES


def test_stage_lifecycle_against_a_stub(monkeypatch):
    from spring_amd import _lib
    from spring_amd.unqlfc import UnqlfcStage
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
    with UnqlfcStage() as st:
        assert st._h.value == 0x1000 and st.info is None
        assert isinstance(st.get_info(), dict) and st.info is None
    assert calls == ["spring_unqlfc_create", "spring_unqlfc_get_info", "spring_unqlfc_destroy"] and not st._h
