"""What the C ABI launches for a dense MU half-step, pinned without a GPU.

csrc/nmfmu_capi.hip is compiled from the working tree, linked against tests/dispatch_trace_stubs.hip (launchers that log
their arguments) and walked over the grid of tools/make_golden_dispatch.py: every entry's return code and launches must equal
tests/golden/g21_dispatch.npz, which was recorded from the tree before the selection moved into one function.  The pipelined
kernels are bit-identical to the ones they replace at equal splits, so a half-step on the wrong but eligible kernel passes
every parity test; here it is a differing outcome string.  A change of dispatch made on purpose re-records the fixture with
the tool and reviews the difference it prints.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_golden_dispatch as trace  # noqa: E402

CSRC = os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc')
needs_hipcc = pytest.mark.skipif(not trace.HIPCC, reason='hipcc is absent')


@pytest.fixture(scope='module')
def fixture():
    return trace.load_fixture()


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):      # (shared: the stub unit is compiled once)
    return str(tmp_path_factory.mktemp('dispatch_trace'))


@needs_hipcc
@pytest.mark.parametrize('build', list(trace.BUILDS))
def test_dispatch_equals_the_recorded_trace(build, fixture, workdir):
    table, ids = fixture
    got = trace.walk(trace.load(trace.compile_lib(CSRC, trace.BUILDS[build], workdir, build)))
    report = trace.difference(table, ids[build], got)
    if report:
        print(report)
    assert not report, report.splitlines()[0]


def test_fixture_is_no_larger_than_the_largest_one():
    golden = os.path.dirname(trace.FIXTURE)
    assert os.path.getsize(trace.FIXTURE) <= os.path.getsize(os.path.join(golden, 'g2_cfg1.npz'))
