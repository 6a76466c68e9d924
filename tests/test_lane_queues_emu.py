"""vello_hip_lane_stream_priority and the VELLO_HIP_DEBUG_LANE_QUEUES seam on the SIMT-emulated build, which has no hardware queues: one
priority, a degenerate range, the seam's values read by vello_hip_create all the same.  The GPU's side: test_lane_queues_gpu.py."""
import pytest

import vello_amd


def test_emu_lanes_report_one_priority(emu_engine):
    e = emu_engine
    assert e.lane_stream_priority(0) == (0, 0, 0)
    with pytest.raises(vello_amd.VelloHipError, match=r"\(-1\)"):
        e.lane_stream_priority(1)  # not created yet
    e.set_frames_in_flight(8)
    assert [e.lane_stream_priority(k) for k in range(8)] == [(0, 0, 0)] * 8
    e.set_frames_in_flight(1)
    assert e.lane_stream_priority(7) == (0, 0, 0)  # out of the rotation, still there
    with pytest.raises(vello_amd.VelloHipError, match=r"\(-1\)"):
        e.lane_stream_priority(8)
    lib = e._lib
    assert lib.vello_hip_lane_stream_priority(None, 0, None, None, None) == -1
    assert lib.vello_hip_lane_stream_priority(e._h, 0, None, None, None) == 0  # every output is optional


@pytest.mark.parametrize("value", ["default", "least", "greatest", ""])
def test_emu_seam_values_accepted(emu_engine, monkeypatch, value):
    monkeypatch.setenv("VELLO_HIP_DEBUG_LANE_QUEUES", value)
    e = vello_amd.Engine()
    assert e.lane_stream_priority(0) == (0, 0, 0)


def test_emu_unknown_seam_value_is_refused(emu_engine, monkeypatch):
    monkeypatch.setenv("VELLO_HIP_DEBUG_LANE_QUEUES", "fastest")
    with pytest.raises(vello_amd.VelloHipError, match=r"\(-1\).*VELLO_HIP_DEBUG_LANE_QUEUES"):
        vello_amd.Engine()
