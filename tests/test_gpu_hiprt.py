"""prt_amd.DeviceArrays on the MI355X (the CPU half is tests/test_hiprt_cpu.py): bytes go up and come down unchanged, on the null
stream and on a created one, and the block leaves nothing behind.  No scene, no context, no kernel."""
import numpy as np
import pytest

import prt_amd
from prt_gpukit import dev  # noqa: F401  (fixture: a DeviceArrays whose allocations are asserted to be 16-byte aligned)

pytestmark = pytest.mark.gpu


def pattern(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


@pytest.mark.parametrize("nbytes", [1, 64, 1092])  # 1092 = 13 x 7 x 12, the lens tests' image: no multiple of 16
def test_round_trip(dev, nbytes):
    a, back = pattern(nbytes, nbytes), np.zeros(nbytes, np.uint8)
    p = dev.upload(a)
    assert type(p) is int and p % 16 == 0
    dev.download(back, p)
    assert back.tobytes() == a.tobytes()


def test_fill_then_download(dev):
    p = dev.alloc(1092)
    dev.fill(p, 0xA5, 1092)
    dev.fill(p + 100, 0x3C, 92)
    back = np.zeros(1092, np.uint8)
    dev.download(back, p)
    assert (back[:100] == 0xA5).all() and (back[100:192] == 0x3C).all() and (back[192:] == 0xA5).all()


def test_a_chain_on_a_created_stream(dev):
    """A copy up, a fill of a second buffer and both copies down, queued on one stream before anything is waited for."""
    s = dev.stream()
    a = pattern(1092, 7)
    p = dev.upload_async(a, s)
    q = dev.alloc(1092)
    dev.fill_async(q, 0x5A, 1092, s)
    back_p, back_q = np.zeros(1092, np.uint8), np.zeros(1092, np.uint8)
    dev.download_async(back_p, p, s)
    dev.download_async(back_q, q, s)
    dev.synchronize(s)
    assert back_p.tobytes() == a.tobytes() and (back_q == 0x5A).all()


def test_the_block_leaves_nothing_behind():
    with prt_amd.DeviceArrays() as d:
        p, s = d.upload(pattern(64, 1)), d.stream()
        assert d._held == [p] and d._streams == [s]
    assert d._held == [] and d._streams == []
