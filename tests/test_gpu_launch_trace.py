"""MI355X: the C-ABI calls of fixed tiny U-Net evaluations -- symbol, order and every non-address descriptor field -- against
tests/golden/engine_trace_gpu.json (tests/launch_trace.py: the recorder, the cases and how the fixture was written).

The cases reach every route of the engine's launch path: forward, input VJP and the training route of a two-level 2-D net (circular
and zero padded, shared and per-image time), the same under the f16 x 2 multiply, each rung of the stride-2 head's and the
up-sampling tail's VJP ladders with one switch off at a time, a width without Winograd / f16 x 2 packing, and the block1d route."""
import json

import pytest
import torch

from tests import launch_trace as LT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fixture():
    with open(LT.GPU_FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(fixture):
    assert sorted(fixture['cases']) == sorted(c[0] for c in LT.gpu_cases())
    assert sorted(fixture['profile']) == sorted(LT.PROFILE_CASES)


@pytest.mark.parametrize('case', LT.gpu_cases(), ids=lambda c: c[0])
def test_launch_sequence(case, fixture, monkeypatch):
    got = LT.run_case(case, torch.device('cuda'), monkeypatch, LT.trace)
    want = LT.decode(fixture, case[0])
    assert got == want, LT.first_difference(got, want)


@pytest.mark.parametrize('name', LT.PROFILE_CASES)
def test_profile_records(name, fixture, monkeypatch):
    """ops.ConvProfile over the same evaluation: per-family launches and flops, family_bytes, the memory-bound kernels' launches and
    bytes (times are not compared)."""
    case = {c[0]: c for c in LT.gpu_cases()}[name]
    got = LT.run_profile(case, torch.device('cuda'), monkeypatch)
    assert got == fixture['profile'][name]
