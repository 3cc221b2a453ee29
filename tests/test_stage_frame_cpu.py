"""What the stage wrappers share, without the library: asdict() of the info structures, and the life of a context
handle against a stub that records the calls."""
import ctypes as C

import pytest

from spring_amd import _lib
from spring_amd.bwt import BwtStage
from spring_amd.decode import DecodeStage
from spring_amd.encoder import EncoderStage
from spring_amd.fastq_out import FastqOutStage
from spring_amd.gzip import GzipStage
from spring_amd.idcodec import IdCodecStage
from spring_amd.qualid import QualIdStage
from spring_amd.streams import StreamsStage
from spring_amd.unbwt import UnbwtStage

STAGES = [(EncoderStage, "spring_encoder"), (StreamsStage, "spring_streams"), (DecodeStage, "spring_decode"),
          (QualIdStage, "spring_qualid"), (FastqOutStage, "spring_fastq_out"), (GzipStage, "spring_gzip"),
          (BwtStage, "spring_bwt"), (UnbwtStage, "spring_unbwt"), (IdCodecStage, "spring_idcodec")]
INFO_STRUCTS = [c for c in vars(_lib).values()
                if isinstance(c, type) and issubclass(c, C.Structure) and hasattr(c, "asdict") and hasattr(c, "_fields_")]


def test_every_info_structure_is_found():
    names = {c.__name__ for c in INFO_STRUCTS}
    assert names == {"EncoderInfo", "StreamsInfo", "QualIdInfo", "FastqOutInfo", "GzipInfo", "BwtInfo", "UnbwtInfo",
                     "IdCodecInfo", "DecodeInfo", "Stats"}


@pytest.mark.parametrize("cls", INFO_STRUCTS, ids=lambda c: c.__name__)
def test_asdict(cls):
    s, want, v = cls(), {}, 0
    for name, typ in cls._fields_:
        if issubclass(typ, C.Array):
            vals = []
            for i in range(typ._length_):
                v += 1
                vals.append(typ._type_(v).value)
                getattr(s, name)[i] = vals[-1]
            want[name] = vals
        else:
            v += 1
            want[name] = typ(v).value
            setattr(s, name, want[name])
    got = s.asdict()
    assert list(got) == [name for name, _ in cls._fields_]
    assert got == want
    for name, typ in cls._fields_:
        assert type(got[name]) is (list if issubclass(typ, C.Array) else type(want[name])), name


class StubLib:
    """Every export succeeds and is recorded; <prefix>_create hands out a handle."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            if name.endswith("_create"):
                args[1]._obj.value = 0x1000
            return 0
        return fn


@pytest.mark.parametrize("cls,prefix", STAGES, ids=[c.__name__ for c, _ in STAGES])
def test_stage_lifecycle(cls, prefix, monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    for name in ("close", "__enter__", "__exit__", "get_info"):
        assert callable(getattr(cls, name)), name
    st = cls()
    assert stub.calls == [prefix + "_create"]
    assert st._h.value == 0x1000 and st._L is stub and st.info is None
    info = st.get_info()
    assert stub.calls == [prefix + "_create", prefix + "_get_info"]
    assert isinstance(info, dict) and info and st.info is None
    st.close()
    assert stub.calls[2:] == [prefix + "_destroy"] and not st._h
    st.close()
    assert stub.calls[2:] == [prefix + "_destroy"]
    with cls(0) as st2:
        assert st2._h
    assert not st2._h
    assert stub.calls[3:] == [prefix + "_create", prefix + "_destroy"]
