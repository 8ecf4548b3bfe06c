"""The choice between a stream per table and one stream per proof (vx_table_streams_mode, host only): a pure function of the
values of VX_TABLE_STREAMS and GPU_MAX_HW_QUEUES."""
import pytest


@pytest.mark.parametrize("setting,queues,want", [
    ("auto", "4", "shared"), ("auto", "16", "own"), ("auto", "2", "shared"),
    (None, "4", "shared"), ("", "16", "own"), ("auto", "1", "shared"), ("auto", "5", "own"), ("auto", "8", "own"),
    ("own", "4", "own"), ("own", "2", "own"), ("shared", "16", "shared"), ("shared", None, "shared"), ("own", None, "own"),
    ("auto", None, "shared"),  # unset: the runtime's own default of 4 queues
    ("auto", "many", "own"), ("auto", "0", "own"), ("auto", "4x", "own"),  # no positive number: the streams of before
])
def test_mode(vx, setting, queues, want):
    assert vx.lib.table_streams_mode(setting, queues) == want
