"""spring_amd -- MI355X-native replacement for SPRING's read-reordering stage
(reference src/reorder.h + bitset_util.{h,cpp}).  Python is only the host-side
mirror of the stage interface; all compute is in lib/libspring_reorder_hip.so
(hand-written HIP for gfx950).  There is no CPU fallback: importing works
anywhere, running requires the built library and a GPU."""
from .reorder import (CompressionParams, ReorderError, ReorderOpts, ReorderStage, call_reorder, reorder_dna,  # noqa: F401
                      synth_dna_host, synth_genome_host, SYNTH_GENOMIC, SYNTH_PAIRED, SYNTH_REPEATS)
from .streams import StreamsStage, call_reorder_compress_streams  # noqa: F401,E402
from .decode import DecodeStage  # noqa: F401,E402
from .qualid import QualIdStage  # noqa: F401,E402
from .fastq_out import FastqOutStage  # noqa: F401,E402
from .gzip import GzipStage  # noqa: F401,E402
from .bwt import BwtStage  # noqa: F401,E402
from .unbwt import UnbwtStage  # noqa: F401,E402
from .idcodec import IdCodecStage  # noqa: F401,E402
from .qlfc import QlfcStage  # noqa: F401,E402
from .bsc import BscStage  # noqa: F401,E402
from .unqlfc import UnqlfcStage  # noqa: F401,E402
