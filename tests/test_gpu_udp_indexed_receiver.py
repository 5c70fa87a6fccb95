"""GPU: GpuUdpReceiver::pollIndexed / pollFromIndexed (include/pollnet_amd/udp_receiver.hpp) over an
EfviUdpRingLayout RX-event run against a sequential host filter followed by the reference's read / recvfrom
arithmetic (tests/cpp/test_gpu_udp_rx_indexed.cpp): the same handler calls in the same order with the same
pointers, lengths and source addresses, equal drop counters, two rounds, chunks smaller than the run; Copy mode
returns the error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_gpu_udp_rx_indexed")


@pytest.mark.gpu
def test_gpu_udp_receiver_indexed_matches_sequential_loop():
    assert os.path.exists(BIN), "tests/cpp/test_gpu_udp_rx_indexed not built (make)"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout, p.stdout
    for prefix in (0, 2, 14):
        assert "prefix %d round 1" % prefix in p.stdout, p.stdout
    assert "Copy mode: pollIndexed needs Mode::ZeroCopy" in p.stdout, p.stdout
