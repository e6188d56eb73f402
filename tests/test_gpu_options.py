"""
The engine's options (``isccsearch_set_option`` / ``isccsearch_get_option``, ``HipEngine.options``): every live name reads back
what was set, dropped and unknown names and values outside the range are refused and change nothing, and a block of
``options()`` leaves the engine with the values it found -- the session's, which an ``ISCC_HIP_OPTS`` rerun sets, not the defaults.
"""

import ctypes
import errno

import pytest

from helpers import session_options

pytestmark = pytest.mark.gpu

LIVE = ("queries_per_pass", "profile", "count_candidates", "mfma", "mfma_pack", "mfma_pack3", "mfma_min_queries", "mfma_min_rows",
        "self_tighten", "self_hint", "speculate", "spec_max_queries", "stretch_mb", "mfma_stretch_factor", "candidate_cap",
        "self_boot_rows", "self_boot_per_k", "tiny_rows", "select_wide_from", "device_search_hint")
DROPPED = ("nontemporal", "sample_cost", "fold", "fold_tau", "blocks_per_cu", "boot_rows", "level_growth", "mfma_level_growth",
           "repick", "boot_multi", "self_refresh_steps", "self_max_k", "mfma_few_rows", "mfma_pack_min_queries")


def _raw_set(engine, name, value):
    rc = engine._lib.isccsearch_set_option(engine.handle, name.encode(), value)
    return rc, engine._lib.isccsearch_last_error().decode()


def _raw_get(engine, name):
    value = ctypes.c_int64(-12345)
    rc = engine._lib.isccsearch_get_option(engine.handle, name.encode(), ctypes.byref(value))
    return rc, engine._lib.isccsearch_last_error().decode(), value.value


def test_every_live_option_reads_back_what_was_set(hip_engine):
    for name in LIVE:
        value = hip_engine.get_option(name)
        hip_engine.set_option(name, value)
        assert hip_engine.get_option(name) == value, name


@pytest.mark.parametrize("name", DROPPED + ("no_such_option",))
def test_dropped_and_unknown_names_are_refused(hip_engine, name):
    rc, error = _raw_set(hip_engine, name, 1)
    assert rc == -errno.EINVAL and name in error, (rc, error)
    rc, error, value = _raw_get(hip_engine, name)
    assert rc == -errno.EINVAL and name in error and value == -12345, (rc, error, value)
    with pytest.raises(ValueError, match=name):
        hip_engine.set_option(name, 1)
    with pytest.raises(ValueError, match=name):
        hip_engine.get_option(name)


def test_null_arguments_are_refused(hip_engine):
    lib = hip_engine._lib
    value = ctypes.c_int64()
    assert lib.isccsearch_get_option(hip_engine.handle, None, ctypes.byref(value)) == -errno.EINVAL
    assert lib.isccsearch_get_option(hip_engine.handle, b"mfma", None) == -errno.EINVAL
    assert lib.isccsearch_get_option(None, b"mfma", ctypes.byref(value)) == -errno.EINVAL


@pytest.mark.parametrize("name,bad", [("queries_per_pass", 12), ("tiny_rows", -1)])
def test_a_value_outside_the_range_changes_nothing(hip_engine, name, bad):
    before = hip_engine.get_option(name)
    rc, error = _raw_set(hip_engine, name, bad)
    assert rc == -errno.EINVAL and name in error, (rc, error)
    assert hip_engine.get_option(name) == before
    if name == "queries_per_pass":
        assert hip_engine.stats()["queries_per_pass"] == before


def test_queries_per_pass_shows_in_the_statistics(hip_engine):
    for tq in (16, 8):
        with hip_engine.options(queries_per_pass=tq):
            assert hip_engine.stats()["queries_per_pass"] == tq
    assert hip_engine.stats()["queries_per_pass"] == hip_engine.get_option("queries_per_pass")


def test_options_restores_the_values_it_found(hip_engine):
    # values that are neither the defaults nor what a documented rerun sets: the session's values for this test
    session = dict(tiny_rows=777, queries_per_pass=16, mfma_min_rows=4321)
    found = {name: hip_engine.get_option(name) for name in session}
    with hip_engine.options(**session):
        with hip_engine.options(tiny_rows=0, queries_per_pass=8):
            assert hip_engine.get_option("tiny_rows") == 0 and hip_engine.get_option("queries_per_pass") == 8
            assert hip_engine.get_option("mfma_min_rows") == 4321
        assert {name: hip_engine.get_option(name) for name in session} == session
        with pytest.raises(KeyError, match="from the block"):
            with hip_engine.options(tiny_rows=5, mfma_min_rows=1):
                assert hip_engine.get_option("tiny_rows") == 5
                raise KeyError("from the block")
        assert {name: hip_engine.get_option(name) for name in session} == session
        # a refused value leaves the block's other options as they were found, too
        with pytest.raises(ValueError, match="queries_per_pass"):
            with hip_engine.options(tiny_rows=5, queries_per_pass=12):
                pytest.fail("the block ran under a refused option")
        assert {name: hip_engine.get_option(name) for name in session} == session
    assert {name: hip_engine.get_option(name) for name in session} == found


def test_the_session_still_runs_under_its_options(hip_engine):
    """What ISCC_HIP_OPTS set for the session (tests/conftest.py) is still in force: no test before this one left a default behind."""
    for name, value in session_options().items():
        assert hip_engine.get_option(name) == value, name
