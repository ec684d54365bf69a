"""Host side of FlowTrainer's small-batch switch (flow.py): the route over its boundaries and the parsing of VPC_FLOW_SMALL.
No GPU."""
import pytest

from vpc_amd import VpcError, flow


def test_route_boundaries():
    r = flow.small_step_route
    assert r(128, 12, 500, 128) and r(1, 12, 500, 128) and r(64, 12, 500, 64)
    assert not r(0, 12, 500, 128) and not r(-1, 12, 500, 128)
    assert not r(129, 12, 500, 128) and not r(129, 12, 500, 1 << 30)  # never past the kernels' 128 rows
    assert r(128, 12, 500, 1 << 30)
    assert not r(65, 12, 500, 64) and not r(1, 12, 500, 0)  # the limit from the environment; 0 = never
    assert r(128, 512, 1024, 128)  # 2 d = 1024 and hid = 1024: the widest layers
    assert not r(128, 513, 500, 128) and not r(128, 12, 1025, 128)
    assert not r(128, 0, 500, 128) and not r(128, 12, 0, 128)
    assert (flow.SMALL_MAX_ROWS, flow.SMALL_MAX_WIDTH) == (128, 1024)


def test_environment_parsing(monkeypatch):
    monkeypatch.delenv("VPC_FLOW_SMALL", raising=False)
    assert flow.small_max_rows() == flow.SMALL_ROWS_DEFAULT == 0  # unset: the chain stays the default
    monkeypatch.setenv("VPC_FLOW_SMALL", "")
    assert flow.small_max_rows() == 0
    monkeypatch.setenv("VPC_FLOW_SMALL", "0")
    assert flow.small_max_rows() == 0
    monkeypatch.setenv("VPC_FLOW_SMALL", "128")
    assert flow.small_max_rows() == 128
    monkeypatch.setenv("VPC_FLOW_SMALL", " 64 ")
    assert flow.small_max_rows() == 64
    for bad in ("abc", "12.5", "1e3"):
        monkeypatch.setenv("VPC_FLOW_SMALL", bad)
        with pytest.raises(VpcError, match="VPC_FLOW_SMALL"):
            flow.small_max_rows()
    assert 0 < flow.SMALL_ROWS_MEASURED <= flow.SMALL_MAX_ROWS
