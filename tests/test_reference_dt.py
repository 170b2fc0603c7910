"""Frame intervals outside the 0.05 .. 0.2 s every other differential test draws from (tests/_fuzz.py: DT_SCHEDULES -- equal
timestamps, 1e-9 s, milliseconds, sums that are inexact in binary, 1 s .. an hour, a clock that stepped back, all of them mixed,
another schedule per scene): the live reference against oracle/c, through tests/test_reference_fuzz.py::run_case with the
intervals replaced.  Integers equal, fp64 state within tests/_golden.py's 1e-7, as in that file.

dt enters TrackBuffer.track as `lifetime + dt` in the predict (F, Q and the gate matrix inverted from them; Tracking.py:372-385)
and as `lifetime += dt`, `lifetime > lim` (Tracking.py:513-528).  Any finite double is an interval here; NaN and +-inf are not
pinned.  The seeds and what makes them worth running: tests/_dt_cases.py; those conditions are asserted here on the oracle
alone (no reference, no GPU), for the size of this file and for the size tests/test_gpu_dt.py runs."""
import numpy as np
import pytest

from tests import _dt_cases as dc
from tests._fuzz import DT_BAND, DT_SCHEDULES, draw_case, dt_out_of_band, dt_schedule, scene_inputs


@pytest.mark.reference
@pytest.mark.parametrize("name", DT_SCHEDULES)
@pytest.mark.parametrize("seed", dc.SEEDS)
def test_live_reference_vs_c_oracle_under_interval_schedule(seed, name):
    """draw_case(seed, "wide", max_pts=300, max_scenes=2, frames=12) is the draw of run_case's "small" size with draw_arm "wide"."""
    from tests import test_reference_fuzz as rf
    assert rf._SIZES["small"] == dc.CPU_SIZE
    case = draw_case(seed, arm="wide", **dc.CPU_SIZE)
    seen = rf.run_case("small", seed, draw_arm="wide", dts=dt_schedule(case, name))
    assert seen["ints"] > 0 and seen["raised"] == 0


@pytest.mark.parametrize("max_scenes", [dc.CPU_SIZE["max_scenes"], dc.GPU_SIZE["max_scenes"]])
@pytest.mark.parametrize("name", DT_SCHEDULES)
def test_every_seed_meets_the_schedules_conditions_on_the_oracle(name, max_scenes):
    for seed in dc.SEEDS:
        dc.check(seed, name, max_scenes)
    print(name, max_scenes, dc.schedule_tally(name, max_scenes))


def test_per_scene_gives_four_scenes_four_schedules():
    """`per_scene` at the size tests/test_gpu_dt.py runs: in the seeds that draw four scenes, one k_predict launch reads four
    different dt (zero, tiny, short, inexact)."""
    four = [sd for sd in dc.SEEDS if draw_case(sd, **dc.GPU_SIZE)["S"] == 4]
    assert len(four) >= 4, four
    for sd in four:
        dts = dt_schedule(draw_case(sd, **dc.GPU_SIZE), "per_scene")
        assert len({dts[:, s].tobytes() for s in range(4)}) == 4 and np.any(np.ptp(dts, axis=1) > 0)


def test_schedules_are_pure_functions_that_leave_the_generators_alone():
    """dt_schedule depends on (seed, name, scene) alone -- not on the number of scenes or on what was drawn before -- and takes
    nothing from the generators of draw_case / scene_inputs: recorded seeds keep their draws."""
    for seed in dc.SEEDS[:3]:
        small, big = draw_case(seed, **dc.CPU_SIZE), draw_case(seed, **dc.GPU_SIZE)
        before = scene_inputs(small)
        for name in DT_SCHEDULES:
            a, b = dt_schedule(small, name), dt_schedule(big, name)
            assert a.shape == (small["F"], small["S"]) and a.dtype == np.float64 and np.all(np.isfinite(a))
            k = min(small["S"], big["S"])
            assert np.array_equal(a[:, :k], b[:, :k]) and np.array_equal(a, dt_schedule(small, name)), (seed, name)
        after = scene_inputs(small)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert not dt_out_of_band(before[2]).any()            # what scene_inputs draws IS the band


def test_schedule_contents():
    case = dict(seed=7, F=24, S=12)
    f = np.arange(24)

    def every(period, odd):
        return np.where(f % period == period - 1, odd, 0.1)
    want = {"zero": every(3, 0.0), "tiny": every(3, 1e-9), "long1": every(4, 1.0), "long5": every(4, 5.0),
            "long60": every(5, 60.0), "hour": every(5, 3600.0), "negative": every(4, -0.05)}
    sets = {"short": {0.001, 0.01, 0.03}, "inexact": {0.1, 0.2, 0.3, 0.7, 1.1}, "mixed": {0.0, 0.001, 0.05, 0.1, 0.2, 0.5, 2.0}}
    assert set(want) | set(sets) | {"per_scene"} == set(DT_SCHEDULES) and DT_SCHEDULES[-1] == "per_scene"
    for name, col in want.items():
        d = dt_schedule(case, name)
        assert all(np.array_equal(d[:, s], col) for s in range(12)), name
    for name, vals in sets.items():
        d = dt_schedule(case, name)
        assert set(d.reshape(-1).tolist()) == vals, name                                   # every value is drawn ...
        assert len({d[:, s].tobytes() for s in range(12)}) == 12, name                     # ... and every scene has its own sequence
    d = dt_schedule(case, "per_scene")
    for s in range(12):
        assert np.array_equal(d[:, s], dt_schedule(case, DT_SCHEDULES[s % 10])[:, s]), s
    assert DT_BAND == (0.05, 0.2)
    assert dt_out_of_band(np.array([0.0, 1e-9, 0.03, 0.3, -0.05, 60.0])).all() and not dt_out_of_band(np.array([0.05, 0.1, 0.2])).any()
