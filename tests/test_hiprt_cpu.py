"""prt_amd.DeviceArrays without a GPU, against a fake runtime that records every call: what a `with` block allocates and creates is
freed and destroyed exactly once however the block ends, a non-zero return raises PrtError naming the call, and the real binding
(prt_amd.hip_runtime) is one typed handle per process.  Nothing here calls into the HIP runtime."""
import ctypes as C

import numpy as np
import pytest

import prt_amd
from prt_amd import _hiprt


class FakeRuntime:
    """The functions of _hiprt.SIGNATURES over plain Python state.  calls: (name, arguments) in order; fail: {name: (n, code)}
    makes the n-th call (from 1) of that function return `code`."""

    def __init__(self, fail=None):
        self.calls, self.fail, self.count, self.next = [], fail or {}, {}, 0x1000

    def __getattr__(self, name):
        if name not in _hiprt.SIGNATURES:
            raise AttributeError(name)

        def call(*args):
            self.count[name] = self.count.get(name, 0) + 1
            n, code = self.fail.get(name, (0, 0))
            rc = code if n == self.count[name] else 0
            values = tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)
            if rc == 0 and name in ("hipMalloc", "hipStreamCreate"):
                self.next += 0x100
                args[0]._obj.value = self.next
                values = (self.next,) + values[1:]
            if name == "hipGetErrorString":
                return b"fake error %d" % args[0]
            self.calls.append((name, values))
            return rc
        return call

    def of(self, name):
        return [v for n, v in self.calls if n == name]


def test_every_allocation_is_freed_once_and_streams_go_first():
    h = FakeRuntime()
    with prt_amd.DeviceArrays(device=3, runtime=h) as dev:
        a, s, b = dev.alloc(100), dev.stream(), dev.alloc(0)
        assert h.calls[0] == ("hipSetDevice", (3,))
        assert [size for _, size in h.of("hipMalloc")] == [100, 64], "alloc(0) asks for 64 bytes"
        assert len({a, s, b}) == 3 and all(type(v) is int for v in (a, s, b))
    names = [n for n, _ in h.calls]
    assert sorted(p for p, in h.of("hipFree")) == sorted([a, b])
    assert h.of("hipStreamSynchronize") == [(s,)] and h.of("hipStreamDestroy") == [(s,)]
    assert names.index("hipStreamSynchronize") < names.index("hipStreamDestroy") < names.index("hipFree")
    dev.__exit__(None, None, None)  # a second exit finds nothing left
    assert len(h.of("hipFree")) == 2 and len(h.of("hipStreamDestroy")) == 1


def test_the_same_when_the_body_raises():
    h = FakeRuntime()
    with pytest.raises(KeyError):
        with prt_amd.DeviceArrays(runtime=h) as dev:
            a, s, b = dev.alloc(1), dev.stream(), dev.upload(np.zeros(5, np.float32))
            raise KeyError("the body's own")
    assert sorted(p for p, in h.of("hipFree")) == sorted([a, b]) and h.of("hipStreamDestroy") == [(s,)]


def test_a_failed_third_allocation_frees_the_first_two():
    h = FakeRuntime(fail={"hipMalloc": (3, 2)})
    got = []
    with pytest.raises(prt_amd.PrtError, match="hipMalloc.*fake error 2"):
        with prt_amd.DeviceArrays(runtime=h) as dev:
            for n in (10, 20, 30):
                got.append(dev.alloc(n))
    assert len(got) == 2 and sorted(p for p, in h.of("hipFree")) == sorted(got)


def test_copies_and_fills_pass_their_arguments_on_and_raise_on_an_error():
    h = FakeRuntime(fail={"hipMemcpy": (2, 1)})
    a = np.arange(7, dtype=np.float32)
    with prt_amd.DeviceArrays(runtime=h) as dev:
        p, s = dev.upload(a), dev.stream()
        assert h.of("hipMemcpy") == [(p, a.ctypes.data, 28, 1)]
        dev.fill(p, 0xA5, 28)
        dev.upload_async(a, s, p)
        dev.fill_async(p, 0, 28, s)
        dev.download_async(a, p, s)
        dev.synchronize(s)
        dev.synchronize()
        assert h.of("hipMemset") == [(p, 0xA5, 28)] and h.of("hipMemsetAsync") == [(p, 0, 28, s)]
        assert h.of("hipMemcpyAsync") == [(p, a.ctypes.data, 28, 1, s), (a.ctypes.data, p, 28, 2, s)]
        assert h.of("hipStreamSynchronize") == [(s,)] and h.of("hipDeviceSynchronize") == [()]
        with pytest.raises(prt_amd.PrtError, match="hipMemcpy.*fake error 1"):
            dev.download(a, p)
    assert h.of("hipFree") == [(p,)]


def test_the_real_binding_is_one_typed_handle():
    h = prt_amd.hip_runtime()
    assert prt_amd.hip_runtime() is h
    for name, argtypes in _hiprt.SIGNATURES.items():
        f = getattr(h, name)
        assert f.argtypes is not None and list(f.argtypes) == argtypes, name
    assert h.hipGetErrorString.restype is C.c_char_p and h.hipMalloc.restype is C.c_int
