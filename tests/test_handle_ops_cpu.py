"""CPU: the table of handle operations (handle_ops.py) classifies every public method of api.Problem and api.Batch.

A method added later has to become an operation of the table -- and with that part of the history tests
(test_gpu_handle_history.py, test_gpu_batch_history.py) -- or be excluded with a reason; it cannot be left out silently."""
import pytest

import handle_ops as ops
from spherical_bundle_adjuster_amd import api

TABLES = {"Problem": (api.Problem, ops.PROBLEM_OPS, ops.PROBLEM_EXCLUDED, ops.PROBLEM_DISTURBERS),
          "Batch": (api.Batch, ops.BATCH_OPS, ops.BATCH_EXCLUDED, ops.BATCH_DISTURBERS)}


@pytest.mark.parametrize("which", TABLES)
def test_every_public_method_is_classified_exactly_once(which):
    cls, table, excluded, _ = TABLES[which]
    public = set(ops.public_names(cls))
    behind = {m for op in table for m in op.methods}
    assert behind <= public, f"the table names methods {which} does not have: {sorted(behind - public)}"
    assert set(excluded) <= public, f"excluded names {which} does not have: {sorted(set(excluded) - public)}"
    assert not behind & set(excluded), f"both behind an operation and excluded: {sorted(behind & set(excluded))}"
    missing = public - behind - set(excluded)
    assert not missing, f"{which} methods that are neither behind an operation of handle_ops nor excluded: {sorted(missing)}"
    assert all(isinstance(r, str) and r.strip() for r in excluded.values())


@pytest.mark.parametrize("which", TABLES)
def test_operations_call_the_methods_they_stand_for(which):
    _, table, _, _ = TABLES[which]
    for op in table:
        assert op.methods, op.name
        unused = set(op.methods) - ops.names_used(op)
        assert not unused, f"{op.name} does not refer to {sorted(unused)}"


@pytest.mark.parametrize("which", TABLES)
def test_names_are_unique_and_kinds_known(which):
    _, table, _, disturbers = TABLES[which]
    names = [op.name for op in table]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert all(op.kind in ops.KINDS for op in table), [op.name for op in table if op.kind not in ops.KINDS]
    assert all(ops.by_kind(table, k) for k in ops.KINDS)
    assert set(disturbers) <= {op.name for op in table if op.kind != ops.MUTATOR}
    assert set(ops.PROBLEM_FINITE) <= {op.name for op in ops.by_kind(ops.PROBLEM_OPS, ops.PROBE)}


def test_outputs_as_bytes():
    """The byte form keeps what the comparisons rest on: NaN payloads and signed zeros differ, timings do not count."""
    import numpy as np
    s = api.SolveSummary("CONVERGENCE_FUNCTION", 3, 2, 4, 1.0, 0.5, 1e-9, 10.0, 0.25, 0.125)
    t = api.SolveSummary("CONVERGENCE_FUNCTION", 3, 2, 4, 1.0, 0.5, 1e-9, 10.0, 9.0, 8.0)
    assert ops.to_bytes((np.zeros(3), s)) == ops.to_bytes((np.zeros(3), t))
    assert ops.to_bytes(s) != ops.to_bytes(api.SolveSummary("CONVERGENCE_FUNCTION", 3, 2, 4, 1.0, 0.5000000000000001, 1e-9, 10.0, 0, 0))
    assert ops.to_bytes(np.array([0.0])) != ops.to_bytes(np.array([-0.0]))
    assert ops.to_bytes(np.zeros(2)) != ops.to_bytes(np.zeros(2, dtype=np.float32)) != ops.to_bytes(np.zeros((2, 1)))
    assert ops.to_bytes({"a": 1.0, "seconds_x": 2.0}) == ops.to_bytes({"a": 1.0, "seconds_x": 3.0})
    assert ops.to_bytes(None) != ops.to_bytes(0)
    c = api.JointCovariance(np.eye(6), None, 1.0, 2.0, 3, 0, 5, -2)
    assert ops.to_bytes(c) != ops.to_bytes(api.JointCovariance(np.eye(6), None, 1.0, 2.0, 3, 1, 5, -2))
    assert np.array_equal(ops.float_values((c, s, [np.arange(3), 2.5])), np.concatenate([np.eye(6).reshape(-1), [1.0, 2.0, 2.5]]))
