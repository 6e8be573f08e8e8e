"""The switch between the host and the device solver of the exposure gain systems (config.set_exposure_solver,
STITCHING_AMD_EXPOSURE_SOLVER, ExposureEstimator(solver=)) — everything that needs no GPU."""
import os
import subprocess
import sys

import pytest

import stitching_amd as S
from stitching_amd import _lib, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_trip_returns_the_previous_mode():
    start = S.exposure_solver()
    assert start in ("host", "device")
    try:
        assert S.set_exposure_solver("device") == start
        assert S.exposure_solver() == "device"
        assert S.set_exposure_solver("host") == "device"
        assert S.exposure_solver() == "host"
    finally:
        S.set_exposure_solver(start)


def test_unknown_modes_raise_and_change_nothing():
    before = S.exposure_solver()
    for bad in ("gpu", "", None, 1):
        with pytest.raises(S.StitchingError):
            S.set_exposure_solver(bad)
    assert S.exposure_solver() == before
    assert _lib.lib().stx_set_exposure_solver(7) != 0
    assert S.exposure_solver() == before
    with pytest.raises(S.StitchingError):
        S.ExposureEstimator("gain_blocks", solver="opencv")


@pytest.mark.parametrize("value,want", [(None, "host"), ("", "host"), ("host", "host"), ("device", "device")])
def test_environment_variable_sets_the_start_up_value(value, want):
    env = dict(os.environ)
    env.pop("STITCHING_AMD_EXPOSURE_SOLVER", None)
    if value is not None:
        env["STITCHING_AMD_EXPOSURE_SOLVER"] = value
    code = "import stitching_amd as S; print(S.exposure_solver())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == want


def test_estimator_takes_the_solver_without_a_gpu():
    e = S.ExposureEstimator("gain_blocks", 1, 32, solver="device")
    assert (e.kind, e.nr_feeds, e.block_size, e.solver) == ("gain_blocks", 1, 32, "device")
    assert S.ExposureEstimator("channel", solver="host").solver == "host"
    assert S.ExposureEstimator("gain").solver is None  # the process-wide mode, read at every feed
    e.feed([], [], [])  # empty lists: a no-op


def test_compensator_passes_the_process_wide_solver_through(monkeypatch):
    monkeypatch.setattr(config, "_exposure_estimator", "device")
    start = S.exposure_solver()
    try:
        S.set_exposure_solver("device")
        assert S.ExposureErrorCompensator("gain_blocks").compensator.solver == "device"
        assert S.ExposureErrorCompensator("channel", nr_feeds=2).compensator.solver == "device"
        S.set_exposure_solver("host")
        assert S.ExposureErrorCompensator("gain_blocks").compensator.solver == "host"
    finally:
        S.set_exposure_solver(start)


def test_new_symbols_are_exported():
    L = _lib.lib()
    for name in ("stx_lu_solve_device", "stx_exposure_solve_device", "stx_exposure_feed_ex", "stx_set_exposure_solver",
                 "stx_get_exposure_solver"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.EXPOSURE_SOLVERS == {"host": 0, "device": 1}
    assert _lib.LU_NB == 32 and _lib.LU_MAX_N == 16384


def test_device_entries_need_a_context():
    import ctypes as C

    L = _lib.lib()
    x = (C.c_double * 4)()
    assert L.stx_lu_solve_device(None, 4, x, x, x, None) != 0
    assert b"ctx" in L.stx_last_error()
