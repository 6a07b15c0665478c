"""What the convolutive engine decides and launches, pinned without a GPU.

tests/golden/g22_conv_plan.npz was recorded by tools/make_golden_conv_plan.py from the tree before ConvMU's constructor
became ``plan_conv`` + allocation (tests/golden/PROVENANCE_conv_plan.txt): over a grid of shapes, precisions and switches,
every decision the engine carries and every buffer size; and for every case of ``conv_emulation.conv_cases`` every library
call of construction and three iterations with its arguments.  The test walks the same points on the working tree --
ConvMU on meta / CPU tensors, nothing launched -- and requires equal outcomes, then requires ``plan_conv`` alone (no
tensor, no device) to say what the engine built from it carries.  A path chosen differently but eligible passes every parity
test; here it is a differing outcome.  A change of a rule made on purpose re-records the fixture with the tool and reviews
the difference it prints.
"""
import dataclasses
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_golden_conv_plan as trace  # noqa: E402


@pytest.fixture(scope='module')
def fixture():
    return trace.load_fixture()


def test_plans_and_launches_equal_the_recorded_trace(fixture):
    table, ids = fixture
    report = trace.difference(table, ids, trace.walk())
    if report:
        print(report)
    assert not report, report.splitlines()[0]


def test_plan_conv_alone_says_what_the_engine_carries(fixture):
    """plan_conv from sizes, CU count and an ``env`` mapping against the decisions recorded from the engine (the fixture's
    outcome of the same grid point), field by field."""
    from torchnmf_amd import _capi, nmfd_engine as N
    table, ids = fixture
    lib, seen = _capi.load(), 0
    for i, pt in enumerate(trace.points()):
        want = table[ids[i]]
        if not want.startswith('('):
            continue                                        # (an exception of the constructor: covered by the test above)
        B, C, ls, R, ts, beta, _, own_loop, ncu, env = pt
        p = dataclasses.asdict(N.plan_conv(lib, B, C, ls, R, ts, beta, own_loop, ncu,
                                           env={trace.PREFIX + k: v for k, v in env}))
        rec = dict(eval(want, {})[0])                       # noqa: S307 -- a repr the tool wrote
        for k in trace.FIELDS[1:]:
            assert p[k] == rec[k], (pt, k, p[k], rec[k])
        seen += 1
    assert seen > 5000


def test_fixture_is_no_larger_than_the_largest_one():
    golden = os.path.dirname(trace.FIXTURE)
    assert os.path.getsize(trace.FIXTURE) <= os.path.getsize(os.path.join(golden, 'g2_cfg1.npz'))
