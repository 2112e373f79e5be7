"""The n-tuple call-mix fuzz (tests/ntuple_fuzz.py) without a GPU: what the pinned seeds of tests/test_gpu_ntuple_fuzz.py reach,
that a seed is a call trace, and that the comparison has teeth.

1. Coverage, from the model's counters alone (the oracle drives the model, nothing else runs): across the pinned seeds every
   operation kind of ntuple_fuzz.OPS is drawn and every event of ntuple_fuzz.EVENTS is reached at least once.
2. Determinism: the same (seed, case) gives the same text of operation names and parameters twice.
3. Teeth: the model against a sabotaged copy of itself -- eight sabotages, each in another state owner (the hooks are the
   subclasses below, not the reference modules) -- is reported as a Mismatch within the pinned seeds, the message names the seed,
   the case, the call, the operation and the field, and the same (seed, case) alone gives the same message again.
An unsabotaged copy agrees with the model on every call (the comparison reports nothing on its own)."""
import hashlib

import numpy as np
import pytest

import ntuple_fuzz as nf


def pinned_cases():
    return [(seed, case) for seed, cases, _ in nf.PINNED for case in range(cases)]


@pytest.fixture(scope="module")
def pinned_run():
    """The pinned seeds with the model alone, once: (the counters, {(seed, case): the call trace})."""
    nf.counts.clear()
    traces = {}
    for seed, case in pinned_cases():
        traces[seed, case] = []
        nf.one_case(seed, case, trace=traces[seed, case])
    return dict(nf.counts), traces


def test_pinned_seeds_draw_every_operation_and_reach_every_event(pinned_run):
    counts, traces = pinned_run
    assert [op for op in nf.OPS if counts.get(op, 0) < 1] == [], "operation kinds the pinned seeds never draw"
    assert [ev for ev in nf.EVENTS if counts.get("event." + ev, 0) < 1] == [], "events the pinned seeds never reach"
    assert "out_of_domain" not in counts, "a pinned case left the score range the record keeps exactly"
    assert set(counts) - {"cases", "calls"} - {"event." + ev for ev in nf.EVENTS} <= set(nf.OPS), "an operation kind OPS does not list"
    assert counts["calls"] == sum(len(t) for t in traces.values()) and all(12 <= len(t) <= 30 for t in traces.values())


def test_a_seed_is_a_call_trace(pinned_run):
    _, traces = pinned_run
    seed, case = min(traces, key=lambda k: len(traces[k]))
    again = []
    nf.one_case(seed, case, trace=again)
    sha = lambda t: hashlib.sha256("\n".join(t).encode()).hexdigest()      # noqa: E731
    assert sha(again) == sha(traces[seed, case])
    assert len({sha(t) for t in traces.values()}) == len(traces), "two cases with the same trace"


def test_an_unsabotaged_copy_agrees(pinned_run):
    _, traces = pinned_run
    seed, case = min(traces, key=lambda k: len(traces[k]))
    nf.one_case(seed, case, nf.against(nf.Model))


# ------------------------------------------------------------------------------------------------ the sabotaged models
class MeanLeavesACount(nf.Model):
    """NTupleMean: one ``count`` stays non-zero after an update."""
    needs = staticmethod(lambda cfg: cfg.mean)

    def _mean_update(self, fn, *args):
        super()._mean_update(fn, *args)
        self.mean.count.reshape(-1)[0] = 1


class LogSkipsTheCarry(nf.Model):
    """NTupleLog: slot M is not carried into slot 0."""
    needs = staticmethod(lambda cfg: cfg.log_depth)

    def _log_carry(self):
        pass


class TraceKeepsItsLength(nf.Model):
    """NTupleTrace: a board's length survives the end of its episode (the "ended" bit is not set)."""
    needs = staticmethod(lambda cfg: cfg.ring == "trace")

    def _push(self, ring, *args):
        delta = super()._push(ring, *args)
        ring.len &= 0x7f
        return delta


class PlayClockOneShort(nf.Model):
    """The engine: a K-move launch advances the clock by K - 1."""
    needs = staticmethod(lambda cfg: True)

    def _play_clock(self, k_steps):
        if k_steps > 1:
            self.o.t -= 1


class TCAccumulatesSigned(nf.Model):
    """NTupleTC: ``mag`` accumulates delta, not |delta|."""
    needs = staticmethod(lambda cfg: cfg.tc)

    def _tc_update(self, fn, *args):
        err, mag = self.tc.err.copy(), self.tc.mag.copy()
        super()._tc_update(fn, *args)
        self.tc.mag[:] = mag + (self.tc.err.view(np.uint64) - err.view(np.uint64))       # (uint64 arithmetic wraps)


class FlushLeavesOneItem(nf.Model):
    """NTupleDelay: the flush leaves one weight of a due item unapplied."""
    needs = staticmethod(lambda cfg: cfg.ring == "delay")

    def _delay_flush(self, algo, lr_shift):
        before = self.net.weights.copy()
        super()._delay_flush(algo, lr_shift)
        moved = np.argwhere(self.net.weights != before)
        if len(moved):
            i = tuple(moved[0])
            self.net.weights[i] = before[i]


class RestartKeepsStart(nf.Model):
    """Restart: ``start`` survives a refusal."""
    needs = staticmethod(lambda cfg: cfg.restart is not None)

    def _restart_step(self, rec, term):
        start = self.rst.start.copy()
        super()._restart_step(rec, term)
        refused = np.asarray(term, bool) & (self.rst.pos == 0)
        self.rst.start[refused] = start[refused]


class CarouselForgetsTheEpisode(nf.Model):
    """Carousel: an episode that ends is not counted in ``episodes``."""
    needs = staticmethod(lambda cfg: cfg.carousel is not None)

    def _ride(self, ride, term):
        episodes = None if self.car is None else self.car.episodes.copy()
        super()._ride(ride, term)
        if ride == "carousel":
            self.car.episodes[:] = episodes


# what the driver must name first: a field of the sabotaged owner's state -- or, for the log, the sweep's own output (the error of
# slot 0, which the call returns, is compared before the state)
SABOTAGES = {"mean.count": (MeanLeavesACount, ("state mean.count",)), "log": (LogSkipsTheCarry, ("state log.", "output delta")),
             "trace.len": (TraceKeepsItsLength, ("state trace.len",)), "clock": (PlayClockOneShort, ("state clock",)),
             "tc.mag": (TCAccumulatesSigned, ("state tc.mag",)), "weights": (FlushLeavesOneItem, ("state weights",)),
             "restart.start": (RestartKeepsStart, ("state restart.start",)),
             "carousel.episodes": (CarouselForgetsTheEpisode, ("state carousel.episodes",))}


@pytest.mark.parametrize("field", list(SABOTAGES))
def test_a_sabotaged_copy_is_caught(field):
    """The first difference the driver reports is in what the sabotage touches; the replay of that (seed, case) reports the same
    message."""
    sabotaged, named = SABOTAGES[field]
    for seed, case in pinned_cases():
        if not sabotaged.needs(nf.Config(np.random.default_rng([seed, case]))):
            continue
        try:
            nf.one_case(seed, case, nf.against(sabotaged))
        except nf.Mismatch as caught:
            message = str(caught)
            break
    else:
        pytest.fail(f"{sabotaged.__name__}: no mismatch within the pinned seeds")
    assert f"seed {seed} case {case}:" in message and " call " in message and any(text in message for text in named), message
    with pytest.raises(nf.Mismatch) as again:
        nf.one_case(seed, case, nf.against(sabotaged))
    assert str(again.value) == message
