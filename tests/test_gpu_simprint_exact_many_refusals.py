"""
What ``isccsearch_simprint_exact_many`` refuses, called through ``ctypes`` as a binding would: the return code and the exact
``isccsearch_last_error()`` text of every refusal, the ORDER of the checks (a call that breaks two rules gets the message of the
earlier one), whether ``out_info`` has been zeroed by then, and the empty calls that are answered with zero counts instead.
Every refusal is raised on the host, before anything is launched.
"""

import errno

import numpy as np
import pytest

from iscc_search_amd import _lib
from iscc_search_amd._lib import MAX_K, MAX_SCORED_SIMPRINTS, METRIC_HAMMING, METRIC_NPHD, SIMPRINT_CHUNK_DTYPE, SIMPRINT_RESULT_DTYPE

pytestmark = pytest.mark.gpu

EINVAL, E2BIG = -errno.EINVAL, -errno.E2BIG
UNTOUCHED = 0xFFFFFFFF
NAN = float("nan")
WRONG_TABLE = "simprint scoring is defined for fixed-length (Hamming) tables with 128-bit chunk-pointer keys"
MANY = MAX_SCORED_SIMPRINTS + 1
ORDER = ["h", "table", "n_req", "distinct_offsets", "q_words", "given_offsets", "given", "queried", "dup_limit", "threshold", "limit",
         "out_results", "out_chunks", "out_info"]
u32 = lambda *v: np.array(v, dtype=np.uint32)


@pytest.fixture(scope="module")
def tables(hip_engine):
    """4 assets x 2 chunks of 64-bit simprints under 128-bit chunk-pointer keys; tables no scoring call takes; an empty one."""
    keys = np.array([[a + 1, c] for a in range(4) for c in range(2)], dtype=np.uint64)
    words = np.array([[0x1111111111111111 * (i + 1)] for i in range(8)], dtype=np.uint64)
    made = {
        "simprints": hip_engine.open_table(METRIC_HAMMING, 2, 8),
        "keys64": hip_engine.open_table(METRIC_HAMMING, 1, 8),
        "nphd": hip_engine.open_table(METRIC_NPHD, 2, 8),
        "empty": hip_engine.open_table(METRIC_HAMMING, 2, 8),
    }
    made["simprints"].add(keys, words)
    made["keys64"].add(keys[:, 0] * 10 + keys[:, 1], words)
    made["nphd"].add(keys, words, np.full(8, 8, dtype=np.uint8))
    yield {name: t.id for name, t in made.items()}
    for t in made.values():
        t.drop()


# two requests: {Q0, Q1} given as (0, 1, 0), and {Q0} given once; values that pass
Q = np.array([0x1111111111111111, 0x2222222222222223, 0x1111111111111111], dtype=np.uint64)
ARGS = dict(n_req=2, distinct_offsets=u32(0, 2, 3), q_words=Q, given_offsets=u32(0, 3, 4), given=u32(0, 1, 0, 0), queried=u32(3, 1),
            dup_limit=8, threshold=0.0, limit=2,
            out_results=np.zeros(2 * 2, dtype=SIMPRINT_RESULT_DTYPE), out_chunks=np.zeros(8 * 4, dtype=SIMPRINT_CHUNK_DTYPE),
            out_info=np.zeros(4 * 2, dtype=np.uint32))


def _call(hip_engine, tables, **overrides):
    a = dict(ARGS, h=hip_engine.handle, table=tables["simprints"])
    a.update(overrides)
    if isinstance(a["table"], str):
        a["table"] = tables[a["table"]]
    info = a["out_info"]
    if info is not None:
        info[:] = UNTOUCHED
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]             # (the arrays live until the call returns)
    rc = _lib.load_library().isccsearch_simprint_exact_many(*[_lib.ptr(a[n]) if isinstance(a[n], np.ndarray) else a[n] for n in ORDER])
    del keep
    return rc, (_lib.last_error() if rc else ""), info


# (what breaks the rule, return code, message, out_info zeroed by then) in the order of the checks
RULES = [
    (dict(h=None), EINVAL, "handle is NULL", False),
    (dict(dup_limit=0), EINVAL, "dup_limit must be >= 1", False),
    (dict(limit=0), EINVAL, "limit must be >= 1", False),
    (dict(out_info=None), EINVAL, "NULL argument", False),
    (dict(given_offsets=u32(0, 4, 3)), EINVAL, "given_offsets must not decrease (request 1)", True),
    (dict(queried=u32(3, 0)), EINVAL, "request 1: queried (0) counts every query simprint as given: it cannot be below its given simprints (1)", True),
    (dict(out_results=None), EINVAL, "NULL argument", True),
    (dict(given=u32(0, 1, 0, 1)), EINVAL, "request 1: given[3] = 1 is no index into its 1 distinct simprints", True),
    (dict(limit=0x80000000), E2BIG, f"limit {0x80000000} x 2 requests exceeds the 32-bit result addressing", True),
    (dict(threshold=NAN), EINVAL, "threshold is not a number", True),
    (dict(table="keys64"), EINVAL, WRONG_TABLE, True),
]
# further ways to break a rule of the list above: the same refusal, checked on its own
_WIDE = 129                   # requests of 8 192 given simprints each: 4 096 x 1 056 768 chunk records are past 32 bits
ALSO = [
    (dict(distinct_offsets=None), EINVAL, "NULL argument", False),
    (dict(given_offsets=None), EINVAL, "NULL argument", False),
    (dict(queried=None), EINVAL, "NULL argument", False),
    (dict(distinct_offsets=u32(0, 3, 2)), EINVAL, "distinct_offsets must not decrease (request 1)", True),
    (dict(distinct_offsets=u32(0, 0, MANY), q_words=np.zeros(MANY, dtype=np.uint64), given_offsets=u32(0, 0, 1), given=u32(0), queried=u32(0, 1)), E2BIG,
     f"request 1: {MANY} / 1 query simprints exceed the {MAX_SCORED_SIMPRINTS} one scoring call takes", True),
    (dict(given_offsets=u32(0, MANY, MANY + 1), given=np.zeros(MANY + 1, dtype=np.uint32), queried=u32(MANY, 1)), E2BIG,
     f"request 0: 2 / {MANY} query simprints exceed the {MAX_SCORED_SIMPRINTS} one scoring call takes", True),
    (dict(queried=u32(2, 1)), EINVAL, "request 0: queried (2) counts every query simprint as given: it cannot be below its given simprints (3)", True),
    (dict(q_words=None), EINVAL, "NULL argument", True),
    (dict(given=None), EINVAL, "NULL argument", True),
    (dict(given=u32(0, 2, 0, 0)), EINVAL, "request 0: given[1] = 2 is no index into its 2 distinct simprints", True),
    (dict(n_req=_WIDE, distinct_offsets=np.arange(_WIDE + 1, dtype=np.uint32), q_words=np.zeros(_WIDE, dtype=np.uint64),
          given_offsets=np.arange(_WIDE + 1, dtype=np.uint32) * np.uint32(MAX_SCORED_SIMPRINTS), given=np.zeros(_WIDE * MAX_SCORED_SIMPRINTS, dtype=np.uint32),
          queried=np.full(_WIDE, MAX_SCORED_SIMPRINTS, dtype=np.uint32), dup_limit=MAX_K + 5, out_chunks=None,
          out_results=np.zeros(_WIDE * 2, dtype=SIMPRINT_RESULT_DTYPE), out_info=np.zeros(4 * _WIDE, dtype=np.uint32)), E2BIG,
     f"{MAX_K} collisions x {_WIDE * MAX_SCORED_SIMPRINTS} given simprints exceed the 32-bit chunk addressing", True),
    (dict(table="nphd"), EINVAL, WRONG_TABLE, True),
]


def _refused(hip_engine, tables, overrides, rc, message, zeroed):
    got_rc, got_message, info = _call(hip_engine, tables, **overrides)
    assert (got_rc, got_message) == (rc, message), list(overrides)
    if info is not None:
        assert info.tolist() == [0 if zeroed else UNTOUCHED] * len(info), list(overrides)


def test_the_arguments_that_pass_are_answered(hip_engine, tables):
    rc, _, info = _call(hip_engine, tables)
    assert rc == 0 and info[0] >= 1 and info[4] >= 1
    rc, _, info = _call(hip_engine, tables, out_chunks=None)                # chunks are optional
    assert rc == 0 and info[0] >= 1 and info[3] == 0 and info[7] == 0


def test_every_refusal_with_its_code_and_text(hip_engine, tables):
    for overrides, rc, message, zeroed in RULES + ALSO:
        _refused(hip_engine, tables, overrides, rc, message, zeroed)


def test_of_two_broken_rules_the_earlier_one_answers(hip_engine, tables):
    for i, (first, rc, message, zeroed) in enumerate(RULES):
        for second, _, _, _ in RULES[i + 1:]:
            both = dict(second, **first)
            if "out_info" in both and both["out_info"] is None:
                zeroed = False
            _refused(hip_engine, tables, both, rc, message, zeroed)


def test_empty_calls_are_answered_with_zero_counts(hip_engine, tables):
    for overrides in [
        dict(given_offsets=u32(0, 0, 0), given=None, queried=u32(0, 0), q_words=None, out_results=None),
        dict(distinct_offsets=u32(0, 0, 0), given_offsets=u32(0, 0, 0), given=None, queried=u32(5, 0), q_words=None),
        dict(table="empty"),
    ]:
        rc, _, info = _call(hip_engine, tables, **overrides)
        assert rc == 0 and info.tolist() == [0] * len(info), list(overrides)
    # no request at all: nothing is read, nothing is written
    rc, _, info = _call(hip_engine, tables, n_req=0, distinct_offsets=None, given_offsets=None, queried=None)
    assert rc == 0 and info.tolist() == [UNTOUCHED] * len(info)
    rc, _, _ = _call(hip_engine, tables, n_req=0, out_info=None)
    assert rc == 0
