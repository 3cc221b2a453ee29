"""The life of every stage context against the real library: what a fresh, a closed and a re-made context answer.
Nothing here launches a kernel; get_info checks its arguments and the context's state and returns."""
import pytest

from spring_amd.bwt import BwtStage
from spring_amd.decode import DecodeStage
from spring_amd.encoder import EncoderStage
from spring_amd.fastq_out import FastqOutStage
from spring_amd.gzip import GzipStage
from spring_amd.idcodec import IdCodecStage
from spring_amd.qualid import QualIdStage
from spring_amd.reorder import ReorderError
from spring_amd.streams import StreamsStage
from spring_amd.unbwt import UnbwtStage

pytestmark = pytest.mark.gpu

E_STATE = -4   # SPRING_REORDER_E_STATE
STAGES = [(EncoderStage, "nothing encoded yet"), (StreamsStage, "no streams computed yet"),
          (DecodeStage, "nothing decoded yet"), (QualIdStage, "no quality / id blocks computed yet"),
          (FastqOutStage, "no text assembled yet"), (GzipStage, "nothing compressed yet"),
          (BwtStage, "nothing transformed yet"), (UnbwtStage, "nothing inverted yet"),
          (IdCodecStage, "no id blocks compressed yet")]


@pytest.mark.parametrize("cls,yet", STAGES, ids=[c.__name__ for c, _ in STAGES])
def test_stage_context(cls, yet):
    st = cls(0)
    assert st._h and st.info is None
    with pytest.raises(ReorderError) as e:
        st.get_info()
    assert str(e.value) == "%s (code %d)" % (yet, E_STATE)
    st.close()
    assert not st._h
    with pytest.raises(ReorderError) as e:
        st.get_info()
    assert str(e.value) == "NULL argument (code -1)"
    st.close()
    with cls(0) as st2:
        assert st2._h
        with pytest.raises(ReorderError, match=yet):
            st2.get_info()
    assert not st2._h
