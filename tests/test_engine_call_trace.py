"""CPU: the engine issues exactly the C-ABI calls pinned in tests/golden/engine_call_trace_v1.json.gz -- same entry points, same order,
same buffers, same scalars -- for the five training networks (fix_bn off and on: set-up, parameter refresh, forward, backward, one
optimizer update), R101 with per-layer weight gradients and with the split backward pass, and the R101 test-time graph at three batch
shapes (folded, dual-output, split-K and plain forward launches; parameters shared between the shapes).  Recorder, cases and the rule
for regenerating the file: tests/golden/make_call_trace.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_call_trace import case_names, load, trace  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return load()


def test_golden_holds_every_case(golden):
    assert sorted(golden) == sorted(case_names())


@pytest.mark.parametrize('case', case_names())
def test_call_trace(case, golden, monkeypatch):
    got = [(phase, line) for phase, lines in trace(case, monkeypatch) for line in lines]
    want = [(phase, line) for phase, lines in golden[case] for line in lines]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, '%s: call %d differs\n  phase %s: %s\nexpected\n  phase %s: %s' % (case, k, g[0], g[1], w[0], w[1])
    extra = (got if len(got) > len(want) else want)[min(len(got), len(want)):]
    assert not extra, '%s: %d calls, expected %d; the first one beyond the common part (phase %s): %s' % (
        (case, len(got), len(want)) + extra[0])
