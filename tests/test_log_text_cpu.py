"""Host side of the device-formatted arrival log (gs_run_log and friends): the
buffer bound gs_log_line_max against the longest line the host writer's format
(gs_host.cpp log_line_ms; main.rs:93 in the grep form of shadow/run.sh:61) can
produce, and the new symbols' presence in the library and the ctypes table."""
import os

import pytest

import gossipsim

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gossipsim.h")

NEW = ("gs_run_log", "gs_format_lat_log", "gs_log_text_reset", "gs_log_line_max")


@pytest.mark.parametrize("node", ["rust", "go", "nim"])
def test_log_line_max_bounds_the_longest_line(node):
    peers = 2 ** 24 - 1
    cfg = gossipsim.PeerConfig(node=node, peers=peers)
    msg_id = 9223372036854775807 if node == "nim" else 1234567890123456789  # 19 digits
    line = "shadow.data/hosts/peer%d/main.1000.stdout:%d:%d milliseconds: %d\n" % (peers - 1, 4294967295, msg_id, 65534)
    assert len(str(msg_id)) == 19 and len(line) == 99
    bound = gossipsim.log_line_max(cfg)
    assert len(line) <= bound <= 112
    # fewer peers: a shorter peer id, a smaller bound, still a bound
    small = gossipsim.PeerConfig(node=node, peers=130)
    line = "shadow.data/hosts/peer%d/main.1000.stdout:%d:%d milliseconds: %d\n" % (129, 4294967295, msg_id, 65534)
    assert len(line) <= gossipsim.log_line_max(small) < bound


def test_new_symbols_exported_and_declared():
    L = gossipsim.lib()
    header = open(HEADER).read()
    for name in NEW:
        assert name in gossipsim.SIGNATURES, name
        assert hasattr(L, name), name
        assert name + "(" in header, name
    assert "gs_text_fn" in header
    for name in ("run_log", "format_lat_log", "log_text_reset"):
        assert callable(getattr(gossipsim.Simulator, name))
    assert gossipsim.lib().gs_log_line_max(None) == 0
