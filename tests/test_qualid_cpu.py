"""CPU tests of the quality and id stage: the checker (tests/qualid_model.py) against the reference's inverse orders
through the oracle, and the C ABI surface that needs no device (tables, header, struct layout, refusals)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import qualid_model as qm
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 10, 1000])
def test_model_orders_equal_the_reference(n):
    rng = np.random.default_rng(n)
    for _ in range(3):
        order = rng.permutation(n).astype(np.uint32)
        assert qm.order_array(order, n, False) == po.generate_order_se(order).tolist()
        assert qm.order_array(order, n, True) == po.generate_order_pe(order).tolist()
    assert qm.order_array(None, n, False) == list(range(n))
    assert qm.order_array(None, n, True) == list(range(n // 2))


def test_model_refuses_bad_orders():
    for order, n, pe in (([0, 0, 1], 3, False), ([0, 1, 3], 3, False), ([0, 1, 2], 3, True), ([0, 1], 3, False)):
        with pytest.raises(qm.Refused):
            qm.order_array(order, n, pe)


def _illumina_spelled_out():
    t = []
    for c in range(128):
        q = c - 33
        if q <= 1:
            v = 0
        elif q <= 9:
            v = 6
        elif q <= 19:
            v = 15
        elif q <= 24:
            v = 22
        elif q <= 29:
            v = 27
        elif q <= 34:
            v = 33
        elif q <= 39:
            v = 37
        else:
            v = 40
        t.append(v + 33)
    return t


def _table(mode, thr=0, high=0, low=0):
    from spring_amd import _lib
    t = np.zeros(128, np.uint8)
    rc = _lib.lib().spring_quality_table(mode, thr, high, low, t.ctypes.data)
    return rc, t.tolist()


def test_illumina_table_at_all_128_indices():
    rc, t = _table(1)
    assert rc == 0
    assert t == _illumina_spelled_out() == list(qm.illumina_table())
    assert all(t[c] == 33 for c in range(35)) and t[35] == 39 and t[127] == 73


@pytest.mark.parametrize("thr,high,low", [(20, 40, 6), (17, 17, 17), (0, 0, 0), (94, 94, 0)])
def test_binary_table_at_all_128_indices(thr, high, low):
    rc, t = _table(2, thr, high, low)
    assert rc == 0
    assert t == [33 + low if c < 33 + thr else 33 + high for c in range(128)] == list(qm.binary_table(thr, high, low))


def test_table_refusals():
    from spring_amd import _lib
    L = _lib.lib()
    assert _table(2, 5, 40, 6)[0] == -1     # low > thr
    assert b"low <= thr <= high" in L.spring_reorder_last_error()
    assert _table(2, 41, 40, 6)[0] == -1    # thr > high
    assert _table(2, 20, 95, 6)[0] == -1    # 33 + high past the 128-entry table's range
    assert _table(0)[0] == -1 and _table(3)[0] == -1
    assert L.spring_quality_table(1, 0, 0, 0, None) == -1


PATTERNS = [
    # (id_1, id_2, find_id_pattern)
    (b"@r1/1", b"@r1/2", 1),
    (b"@SRR1.5 5", b"@SRR1.5 5", 2),
    (b"@A:1:2 1:N:0:ACGT", b"@A:1:2 2:N:0:ACGT", 3),
    (b"@A:1:2 1:N:0 1:x", b"@A:1:2 2:N:0 2:x", 3),       # every space is followed by 1 / 2
    (b"@r1/1", b"@r1/3", 0),
    (b"@r1/1", b"@r10/2", 0),                            # different length
    (b"@r1/1", b"@r2/2", 0),
    (b"@A 1:", b"@A 2:", 3),                             # ' 1:' at the very end
    (b"@A 1", b"@A 2", 1),                               # ... and without the ':' the older pattern wins
    (b"@A x 1:N", b"@A x 2:N", 0),                       # a space not followed by 1 / 2
    (b"@A 3:N", b"@A 3:N", 2),
    (b"@A 1:N ", b"@A 2:N ", 0),                         # a space as the last character
    (b"@A 1:N", b"@B 2:N", 0),
    (b"", b"", 2),                                       # equal empty ids
    (b"", b"1", 0),
]


@pytest.mark.parametrize("a,b,code", PATTERNS)
def test_model_id_patterns(a, b, code):
    assert qm.find_id_pattern(a, b) == code
    # check_id_pattern accepts the code find_id_pattern gave; "@A 1" / "@A 2" alone also fits the newer pattern
    ok = {c for c in (1, 2, 3) if qm.check_id_pattern(a, b, c)}
    assert ok == (({code} if code else set()) | ({3} if a == b"@A 1" else set()))


def test_model_empty_ids_match_code_2_only():
    assert qm.check_id_pattern(b"", b"", 2)
    assert not qm.check_id_pattern(b"", b"", 1) and not qm.check_id_pattern(b"", b"", 3)


def test_model_id_pattern_over_files():
    def fq(ids):
        return b"".join(i + b"\nAC\n+\nII\n" for i in ids)
    a = [b"@r%d/1" % i for i in range(20)]
    b = [b"@r%d/2" % i for i in range(20)]
    assert qm.id_pattern(fq(a), fq(b)) == 1
    b[18] = b"@r18/3"
    assert qm.id_pattern(fq(a), fq(b)) == 0
    assert qm.id_pattern(fq(a), fq(a)) == 2
    assert qm.id_pattern(b"", b"") == 0


def test_model_blocks_by_hand():
    text = b"@a\nACG\n+\nIJK\r\n@bb\n\n+\n\n@c\nA\n+x\n#"   # CR, an empty read, no final newline
    slots = qm.order_array([2, 0, 1], 3, False)             # line 0 -> slot 1, line 1 -> slot 2, line 2 -> slot 0
    q = qm.from_fastq(text, qm.QUALITY, slots, 2)
    assert q["bytes"] == b"#IJK" and q["len"].tolist() == [1, 3, 0] and q["block_off"].tolist() == [0, 4, 4]
    i = qm.from_fastq(text, qm.ID, slots, 2)
    assert i["bytes"] == b"@c\n@a\n@bb\n" and i["len"].tolist() == [2, 2, 3] and i["block_off"].tolist() == [0, 6, 10]
    t = qm.from_fastq(text, qm.QUALITY, slots, 2, qm.illumina_table())
    assert t["bytes"] == b"'III" and t["changed"] == 3    # '#' is q = 2 -> 6; J, K -> q = 40
    assert qm.from_lines(b"IJK\n\n#\n", qm.QUALITY, slots, 2)["bytes"] == q["bytes"]
    for bad in (b"@a\nACG\n+\nIJ\n", b"@a\nACG\n+\nIJK\n@b\n"):
        with pytest.raises(qm.Refused):
            qm.from_fastq(bad, qm.QUALITY, [0], 1)


def test_header_declarations_equal_qualid_exports():
    from spring_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spring_qualid.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(spring_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.QUALID_EXPORTS)
    assert not set(_lib.QUALID_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.STREAMS_EXPORTS) | set(_lib.DECODE_EXPORTS))
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name


def test_info_mirror_matches_the_c_layout(tmp_path):
    from spring_amd import _lib
    fields = [f for f, _ in _lib.QualIdInfo._fields_]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_qualid.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(spring_qualid_info));\n'
                   + "".join('printf("%%zu\\n", offsetof(spring_qualid_info, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.QualIdInfo)
    assert got[1:] == [getattr(_lib.QualIdInfo, f).offset for f in fields]


def test_refusals_without_a_device():
    from spring_amd import _lib
    import spring_amd
    assert spring_amd.QualIdStage is not None
    L = _lib.lib()
    info = _lib.QualIdInfo()
    code = C.c_uint8(9)
    assert L.spring_qualid_create(0, None) == -1
    assert L.spring_qualid_order_from_host(None, None, 0, 0) == -1
    assert L.spring_qualid_order_from_encoder(None, None, 0, 0) == -1
    assert L.spring_qualid_from_fastq(None, None, 0, 3, None, 1, C.byref(info)) == -1
    assert L.spring_qualid_from_lines(None, 0, None, 0, None, 1, C.byref(info)) == -1
    assert L.spring_qualid_download(None, 0, None, None, None) == -1
    assert L.spring_qualid_get_info(None, C.byref(info)) == -1
    assert L.spring_id_pattern(None, 0, None, 0, -1, None, None) == -1
    assert L.spring_id_pattern(None, 5, None, 0, -1, C.byref(code), None) == -1
    L.spring_qualid_destroy(None)
