"""The loop control of the chain phase's host drivers (reorder_pipeline.cpp: run_round_loop under spring_reorder_run_chains,
run_chains_phased, spring_reorder_mg_run and mg_run_phased).  The parity suites pin every driver's output; they cannot see
a batch too many or too few, because a round over finished chains changes nothing.  stats["rounds"] can, and the loops obey
a law by construction.  Let r1 be the rounds of a run that looks at the running chains after every round
(rounds_per_sync = 1, a batch at a time).  With R rounds per look, on the same path and pool:

    a batch at a time               R * ceil(r1 / R)        (the first look that sees no running chain ends the run)
    the host looks one batch late   R * ceil(r1 / R) + R    (the batch queued in front of that look is run as well)

Which form a driver takes: run_chains with one group runs late where the round is fused and untimed, the two-kernel round
(whose count is Globals::alive, so it has an r1 of its own) and every timed run go a batch at a time; both two-group drivers
run late unless timed; a pool over a host communicator always goes a batch at a time (the caller's all-gather is
synchronous), and so does the one-group pool.  The pool paths count what run_chains counts, so their r1 is its r1.

Timed runs also pin the search figures: with two groups the union of the round kernels' spans is positive and at most
their sum (1e-6 relative: float rounding of the summed spans) and each round is two launches; with one group the union
is the sum and each round one launch.  Every run's streams equal those of the first run of its schedule."""
import ctypes as C
import functools
import types

import pytest

from test_gpu_phases import _same

pytestmark = pytest.mark.gpu

N, L, SEED, ERR = 60_000, 100, 23, 10000  # the smallest pool at which two chain groups are allowed (K = 4096)
GEN = N * L // 25
K, T = 4096, 2
BATCH, LATE = "a batch at a time", "one batch late"

# path: (driver, phases, fused, form of the untimed run); every timed run goes a batch at a time
PATHS = {
    "chains_fused": ("chains", 1, 3, LATE),
    "chains_two_kernel": ("chains", 1, -1, BATCH),
    "chains_phased": ("chains", 2, 3, LATE),
    "pool_host_one_group": ("host", 1, 3, BATCH),
    "pool_host_two_groups": ("host", 2, 3, BATCH),
    "pool_rccl_one_group": ("rccl", 1, 3, BATCH),
    "pool_rccl_two_groups": ("rccl", 2, 3, LATE),
}


def _sa():
    import spring_amd
    return spring_amd


def _load(st):
    st.load_synth(N, L, GEN, SEED, ERR)


class _HostComm:
    """A one-rank communicator over the host transport: the library's staging buffer already holds the only slice."""
    transport, world, rank = "host", 1, 0

    def __init__(self):
        from spring_amd import _lib
        self._L = _lib.lib()
        self._cb = _lib.MG_ALLGATHER_FN(lambda buf, off, nbytes, total, user: 0)  # (lives as long as the communicator)
        self._h = C.c_void_p()
        rc = self._L.spring_mg_comm_create_host(C.byref(self._h), self._cb, None, 0, 1)
        assert rc == 0, rc
        self.device = types.SimpleNamespace(index=0, type="cuda")

    def close(self):
        if self._h:
            self._L.spring_mg_comm_destroy(self._h)
            self._h = C.c_void_p()


@pytest.fixture(scope="module")
def rccl_comm():
    from spring_amd.pool import OneRankComm
    comm = OneRankComm(0)
    yield comm
    comm.close()


@pytest.fixture(scope="module")
def host_comm():
    comm = _HostComm()
    yield comm
    comm.close()


def _run(driver, phases, fused, R, timed, comm=None):
    sa = _sa()
    kw = dict(num_chains=K, num_thr=T, deep_bins=-1, fused=fused, phases=phases, rounds_per_sync=R, time_search=timed)
    if driver == "chains":
        with sa.ReorderStage(sa.ReorderOpts(**kw)) as st:
            _load(st)
            return st.run().streams()
    from spring_amd.pool import DistPool
    kw.pop("num_chains")
    dp = DistPool(comm, K, **kw)
    try:
        dp.run(_load)
        return dp.streams()
    finally:
        dp.close()


@functools.lru_cache(maxsize=None)
def _first(phases):
    """The first run of a schedule: run_chains, fused, a look after every round.  Its rounds are the fused r1."""
    got = _run("chains", phases, 3, 1, True)
    assert got["stats"]["phases"] == phases and got["stats"]["chains"] == K
    return got


@functools.lru_cache(maxsize=None)
def _r1_two_kernel():
    return int(_run("chains", 1, -1, 1, True)["stats"]["rounds"])


@pytest.mark.parametrize("R", [1, 3, 16])
@pytest.mark.parametrize("timed", [True, False], ids=["timed", "untimed"])
@pytest.mark.parametrize("path", list(PATHS))
def test_rounds_follow_the_law_of_the_loop(path, timed, R, request):
    driver, phases, fused, untimed_form = PATHS[path]
    comm = request.getfixturevalue(driver + "_comm") if driver != "chains" else None
    ref = _first(phases)
    r1 = _r1_two_kernel() if fused < 0 else int(ref["stats"]["rounds"])
    got = _run(driver, phases, fused, R, timed, comm)
    s = got["stats"]
    form = BATCH if timed else untimed_form
    want = R * -(-r1 // R) + (R if form == LATE else 0)
    print("%s %s R=%d (%s): r1 %d, rounds %d, expected %d; ms_search_kernel %r ms_search_busy %r search_launches %d"
          % (path, "timed" if timed else "untimed", R, form, r1, s["rounds"], want, s["ms_search_kernel"], s["ms_search_busy"],
             s["search_launches"]))
    assert s["phases"] == phases and s["chains"] == K
    assert r1 >= 1
    assert s["rounds"] == want, (path, timed, R, form, r1, s["rounds"], want)
    if timed and phases == 2:
        assert 0 < s["ms_search_busy"] <= s["ms_search_kernel"] * (1 + 1e-6), (s["ms_search_busy"], s["ms_search_kernel"])
        assert s["search_launches"] == 2 * s["rounds"]
    elif timed:
        assert s["ms_search_busy"] == s["ms_search_kernel"]
        assert s["search_launches"] == s["rounds"]
    _same(got, ref, (path, timed, R))
