"""GPU: GpuUdpReceiver (include/pollnet_amd/udp_receiver.hpp) against a sequential host filter followed by the
reference's read / recvfrom arithmetic (tests/cpp/test_gpu_udp_rx.cpp): the same handler calls in the same
order with the same pointers, lengths and source addresses, equal drop counters, ZeroCopy and Copy."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_gpu_udp_rx")


@pytest.mark.gpu
def test_gpu_udp_receiver_matches_sequential_loop():
    assert os.path.exists(BIN), "tests/cpp/test_gpu_udp_rx not built (make)"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout and "ZeroCopy round 2" in p.stdout and "Copy round 2" in p.stdout, p.stdout
