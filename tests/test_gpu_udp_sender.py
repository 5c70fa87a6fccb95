"""GPU: GpuUdpSender (include/pollnet_amd/udp_sender.hpp) against a sequential twin of EfviUdpSender::init + write
per channel (tests/cpp/test_gpu_udp_tx.cpp): the same ring bytes and the same sink calls in the same order with
the same buf_index over three flushes that cross the ring's wrap, buildDevice, and the PLAIN-mode ring through a
GpuUdpReceiver subscribed to the same destinations.  Host only: addChannel's 42 bytes against hand-written
headers (tests/cpp/test_udp_sender_template.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_gpu_udp_tx")
TEMPLATE_BIN = os.path.join(ROOT, "tests", "cpp", "test_udp_sender_template")


def test_add_channel_template_equals_hand_written_headers():
    assert os.path.exists(TEMPLATE_BIN), "tests/cpp/test_udp_sender_template not built (make)"
    p = subprocess.run([TEMPLATE_BIN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "PASS" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_gpu_udp_sender_matches_sequential_twin():
    assert os.path.exists(BIN), "tests/cpp/test_gpu_udp_tx not built (make)"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PASS" in p.stdout, p.stdout
    for stage in ("flush 1: 100 sink calls, buf_index 100", "flush 2: 60 sink calls, buf_index 32",
                  "flush 3: 100 sink calls, buf_index 4", "buildDevice: 49 sink calls, buf_index 54",
                  "plain flush 1: 100 sink calls", "plain flush 2: 28 sink calls, buf_index 54",
                  "receiver: 128 of 128 frames delivered intact"):
        assert stage in p.stdout, p.stdout
    assert "(FAILED)" not in p.stdout, p.stdout
