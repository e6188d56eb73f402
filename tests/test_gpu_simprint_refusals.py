"""
What ``isccsearch_simprint_score``, ``isccsearch_simprint_score_many`` and ``isccsearch_simprint_exact`` refuse, called through
``ctypes`` as a binding would: the return code and the exact ``isccsearch_last_error()`` text of every refusal, the ORDER of the
checks (a call that breaks two rules gets the message of the earlier one), whether ``out_info`` has been zeroed by then, and the
empty requests that are answered with zero counts instead of a refusal.

Every entry point's rules are listed once, in the order the library checks them; the tests walk that list.
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


class Call:
    """One entry point, its arguments in the header's order with values that pass, and the buffers they point to."""

    def __init__(self, name, order, **args):
        self.name, self.order, self.args = name, order, args

    def __call__(self, hip_engine, tables, **overrides):
        a = dict(self.args, h=hip_engine.handle, table=tables["simprints"])
        a.update(overrides)
        if isinstance(a["table"], str):
            a["table"] = tables[a["table"]]
        keep = []                                      # (the arrays live until the call returns)
        info = a["out_info"]
        if info is not None:
            info[:] = UNTOUCHED

        def arg(v):
            if isinstance(v, np.ndarray):
                keep.append(v)
                return _lib.ptr(v)
            return v

        rc = getattr(_lib.load_library(), self.name)(*[arg(a[n]) for n in self.order])
        return rc, (_lib.last_error() if rc else ""), info


def _buffers(n_req=1, limit=2, nq=2):
    return dict(out_results=np.zeros(n_req * limit, dtype=SIMPRINT_RESULT_DTYPE), out_chunks=np.zeros(limit * nq, dtype=SIMPRINT_CHUNK_DTYPE),
                out_chunk_words=np.zeros(limit * nq, dtype=np.uint64), out_info=np.zeros(4 * n_req, dtype=np.uint32))


Q = np.array([0x1111111111111111, 0x2222222222222223], dtype=np.uint64)
Q_MANY = np.zeros(MANY, dtype=np.uint64)

SCORE = Call("isccsearch_simprint_score",
             ["h", "table", "nq", "q_words", "count", "max_hamming", "threshold", "limit", "total_assets", "dup_limit",
              "out_results", "out_chunks", "out_chunk_words", "out_info"],
             nq=2, q_words=Q, count=4, max_hamming=-1, threshold=0.0, limit=2, total_assets=4, dup_limit=8, **_buffers())
SCORE_MANY = Call("isccsearch_simprint_score_many",
                  ["h", "table", "n_req", "req_offsets", "q_words", "count", "max_hamming", "threshold", "limit", "total_assets", "dup_limit",
                   "out_results", "out_chunks", "out_chunk_words", "out_info"],
                  n_req=2, req_offsets=np.array([0, 1, 2], dtype=np.uint32), q_words=Q, count=4, max_hamming=-1, threshold=0.0, limit=2,
                  total_assets=4, dup_limit=8, **_buffers(n_req=2))
_exact_buffers = _buffers()
del _exact_buffers["out_chunk_words"]
EXACT = Call("isccsearch_simprint_exact",
             ["h", "table", "n_distinct", "q_words", "n_given", "given", "queried", "dup_limit", "threshold", "limit",
              "out_results", "out_chunks", "out_info"],
             n_distinct=2, q_words=Q, n_given=3, given=np.array([0, 1, 0], dtype=np.uint32), queried=3, dup_limit=8, threshold=0.0, limit=2,
             **_exact_buffers)

# (what breaks the rule, return code, message, out_info zeroed by then) in the order of the checks
_SHARED = [
    (dict(h=None), EINVAL, "handle is NULL", False),
    (dict(count=0), EINVAL, "`count` must be >= 1", False),
    (dict(max_hamming=257), EINVAL, "max_hamming 257 exceeds 256", False),
    (dict(dup_limit=MAX_K + 1), EINVAL, f"dup_limit {MAX_K + 1} exceeds ISCCSEARCH_MAX_K ({MAX_K})", False),
    (dict(limit=0), EINVAL, "limit must be >= 1", False),
]
RULES = {
    SCORE: _SHARED + [
        (dict(out_info=None), EINVAL, "NULL argument", False),
        (dict(out_results=None), EINVAL, "NULL argument", True),
        (dict(nq=MANY, q_words=Q_MANY), E2BIG, f"{MANY} query simprints exceed the {MAX_SCORED_SIMPRINTS} one scoring call takes", True),
        (dict(threshold=NAN), EINVAL, "threshold is not a number", True),
        (dict(table="keys64"), EINVAL, WRONG_TABLE, True),
    ],
    SCORE_MANY: _SHARED + [
        (dict(out_info=None), EINVAL, "NULL argument", False),
        (dict(req_offsets=np.array([0, 2, 1], dtype=np.uint32)), EINVAL, "req_offsets must not decrease (request 1)", True),
        (dict(out_results=None), EINVAL, "NULL argument", True),
        (dict(limit=0x80000000), E2BIG, f"limit {0x80000000} x 2 requests exceeds the 32-bit result addressing", True),
        (dict(threshold=NAN), EINVAL, "threshold is not a number", True),
        (dict(table="keys64"), EINVAL, WRONG_TABLE, True),
    ],
    EXACT: [
        (dict(h=None), EINVAL, "handle is NULL", False),
        (dict(dup_limit=0), EINVAL, "dup_limit must be >= 1", False),
        (dict(limit=0), EINVAL, "limit must be >= 1", False),
        (dict(out_info=None), EINVAL, "NULL argument", False),
        (dict(out_results=None), EINVAL, "NULL argument", True),
        (dict(n_distinct=MANY, q_words=Q_MANY), E2BIG, f"{MANY} / 3 query simprints exceed the {MAX_SCORED_SIMPRINTS} one scoring call takes", True),
        (dict(queried=2), EINVAL, "queried (2) counts every query simprint as given: it cannot be below n_given (3)", True),
        (dict(threshold=NAN), EINVAL, "threshold is not a number", True),
        (dict(given=np.array([0, 2, 0], dtype=np.uint32)), EINVAL, "given[1] = 2 is no index into the 2 distinct simprints", True),
        (dict(table="keys64"), EINVAL, WRONG_TABLE, True),
    ],
}
# further ways to break a rule of the lists above: the same refusal, checked on its own
ALSO = {
    SCORE: [
        (dict(count=MAX_K + 1), EINVAL, f"count {MAX_K + 1} exceeds ISCCSEARCH_MAX_K ({MAX_K})", False),
        (dict(q_words=None), EINVAL, "NULL argument", True),
        (dict(out_chunks=None), EINVAL, "NULL argument", True),
        (dict(out_chunk_words=None), EINVAL, "NULL argument", True),
        (dict(table="nphd"), EINVAL, WRONG_TABLE, True),
    ],
    SCORE_MANY: [
        (dict(count=MAX_K + 1), EINVAL, f"count {MAX_K + 1} exceeds ISCCSEARCH_MAX_K ({MAX_K})", False),
        (dict(req_offsets=None), EINVAL, "NULL argument", False),
        (dict(req_offsets=np.array([0, 0, MANY], dtype=np.uint32), q_words=Q_MANY), E2BIG,
         f"request 1: {MANY} query simprints exceed the {MAX_SCORED_SIMPRINTS} one scoring call takes", True),
        (dict(q_words=None), EINVAL, "NULL argument", True),
        (dict(out_chunks=None), EINVAL, "NULL argument", True),
        (dict(out_chunk_words=None), EINVAL, "NULL argument", True),
        (dict(table="nphd"), EINVAL, WRONG_TABLE, True),
    ],
    EXACT: [
        (dict(q_words=None), EINVAL, "NULL argument", True),
        (dict(given=None), EINVAL, "NULL argument", True),
        (dict(n_given=MANY, given=np.zeros(MANY, dtype=np.uint32), queried=MANY), E2BIG,
         f"2 / {MANY} query simprints exceed the {MAX_SCORED_SIMPRINTS} one scoring call takes", True),
        (dict(table="nphd"), EINVAL, WRONG_TABLE, True),
    ],
}
CALLS = [SCORE, SCORE_MANY, EXACT]
_ids = lambda c: c.name


def _refused(call, hip_engine, tables, overrides, rc, message, zeroed):
    got_rc, got_message, info = call(hip_engine, tables, **overrides)
    assert (got_rc, got_message) == (rc, message), overrides
    if info is not None:
        assert info.tolist() == [0 if zeroed else UNTOUCHED] * len(info), overrides


@pytest.mark.parametrize("call", CALLS, ids=_ids)
def test_the_arguments_that_pass_are_answered(call, hip_engine, tables):
    rc, _, info = call(hip_engine, tables)
    assert rc == 0 and info[0] >= 1


@pytest.mark.parametrize("call", CALLS, ids=_ids)
def test_every_refusal_with_its_code_and_text(call, hip_engine, tables):
    for overrides, rc, message, zeroed in RULES[call] + ALSO[call]:
        _refused(call, hip_engine, tables, overrides, rc, message, zeroed)


@pytest.mark.parametrize("call", CALLS, ids=_ids)
def test_of_two_broken_rules_the_earlier_one_answers(call, hip_engine, tables):
    rules = RULES[call]
    for i, (first, rc, message, zeroed) in enumerate(rules):
        for second, _, _, _ in rules[i + 1:]:
            both = dict(second, **first)
            if "out_info" in both and both["out_info"] is None:
                zeroed = False
            _refused(call, hip_engine, tables, both, rc, message, zeroed)


def test_empty_requests_are_answered_with_zero_counts(hip_engine, tables):
    for call, overrides in [
        (SCORE, dict(nq=0, q_words=None, out_results=None)),
        (SCORE, dict(table="empty")),
        (SCORE_MANY, dict(req_offsets=np.array([0, 0, 0], dtype=np.uint32), q_words=None, out_results=None)),
        (SCORE_MANY, dict(table="empty")),
        (EXACT, dict(n_distinct=0, q_words=None)),
        (EXACT, dict(n_given=0, given=None, queried=0)),
        (EXACT, dict(table="empty")),
    ]:
        rc, _, info = call(hip_engine, tables, **overrides)
        assert rc == 0 and info.tolist() == [0] * len(info), (call.name, overrides)
    # no request at all: nothing is read, nothing is written
    rc, _, info = SCORE_MANY(hip_engine, tables, n_req=0, req_offsets=None)
    assert rc == 0 and info.tolist() == [UNTOUCHED] * len(info)
    rc, _, _ = SCORE_MANY(hip_engine, tables, n_req=0, req_offsets=None, out_info=None)
    assert rc == 0
