"""GPU: the pinned runs of the n-tuple call-mix fuzz (tests/ntuple_fuzz.py: random mixes of the n-tuple calls -- evaluate, the
searches, play, every learner, the move log, carousel, restart, tile-downgrading, state save / restore -- every output and every
piece of live state compared with the model after every call).  tests/test_ntuple_fuzz_cpu.py shows from the model alone that
these seeds together draw every operation kind and reach every event, and that the comparison catches a sabotaged model.  The long
runs are in profiles/r31_ntuple_fuzz.txt.

The work is pinned by case counts, not by the clock, so a run reproduces: ntuple_fuzz.PINNED is (seed, cases, own streams), eight
cases and 141 to 173 calls per seed.  The pure-Python model dominates the time: alone, on a CPU without a GPU, the four seeds
take 4.9, 6.0, 9.6 and 9.7 s, inside the 12 s the runs of tests/test_gpu_fuzz.py give themselves.  No test here raises a fault on purpose: the fuzz issues valid calls and documented
refusals only."""
import pytest

import ntuple_fuzz

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,cases,own_streams", ntuple_fuzz.PINNED)
def test_ntuple_call_mixes_vs_model(torch_cuda, seed, cases, own_streams):
    """own_streams: every case on a fresh non-default (non-blocking) stream."""
    line = ntuple_fuzz.run(seed=seed, cases=cases, own_streams=own_streams)
    assert line.startswith("ntuple fuzz ok")
    print(line)
