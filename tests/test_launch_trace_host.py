"""CPU: the launch sequence of the U-Net engine on the host replay (tests/cpu_shim.py) -- every call that reaches ops.conv_igemm,
ops.ln_stats, ops.ln_bwd, ops.conv_wgrad and ops.plane_sum, with its whole descriptor -- against
tests/golden/engine_trace_host.json (tests/launch_trace.py).  The fp32 route of the two-level 2-D and 1-D nets, forward, input VJP
and training, with the stride-2 heads' VJP split by parity and as one zero-insertion launch."""
import json

import pytest
import torch

from tests import cpu_shim
from tests import launch_trace as LT


@pytest.fixture(scope='module')
def fixture():
    with open(LT.HOST_FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(fixture):
    assert sorted(fixture['cases']) == sorted(c[0] for c in LT.host_cases())


@pytest.mark.parametrize('case', LT.host_cases(), ids=lambda c: c[0])
def test_launch_sequence(case, fixture, monkeypatch):
    cpu_shim.install(monkeypatch)
    got = LT.run_case(case, torch.device('cpu'), monkeypatch, lambda: LT.host_trace(monkeypatch), warm_up=False)
    want = LT.decode(fixture, case[0])
    assert got == want, LT.first_difference(got, want)
