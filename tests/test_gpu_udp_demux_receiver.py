"""GPU: GpuUdpReceiver::gatherBySub / gatherBySubIndexed (include/pollnet_amd/udp_receiver.hpp) against the handler
calls poll / pollIndexed make on the same ring, bucketed per subscription in call order
(tests/cpp/test_gpu_udp_demux.cpp), from pinned and from device slots; and a relay -- gatherBySub,
GpuUdpSender::buildDevice with the grouped arrays, a second receiver -- through which every payload arrives intact,
one channel after the other."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_gpu_udp_demux")


@pytest.mark.gpu
def test_gather_by_sub_matches_the_bucketed_handler_calls_and_relays():
    assert os.path.exists(BIN), "tests/cpp/test_gpu_udp_demux not built (make)"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout and "(FAILED)" not in p.stdout, p.stdout
    for stage in ("gatherBySub (pinned slots)", "gatherBySub (device slots)", "gatherBySub (70 slots from slot 7)",
                  "gatherBySubIndexed (pinned ring)", "gatherBySubIndexed (device ring)"):
        assert re.search(re.escape(stage) + r": [1-9]\d* messages", p.stdout), p.stdout
    m = re.search(r"relay: (\d+) of (\d+) payloads arrived intact, grouped by channel", p.stdout)
    assert m and m.group(1) == m.group(2) and int(m.group(1)) > 60, p.stdout
