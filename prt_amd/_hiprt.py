"""The one place Python talks to the HIP runtime: a typed ctypes binding (runtime()) and an owner of device memory and streams
(DeviceArrays) for callers that hand device pointers to the *_async methods of PathTracer."""
import ctypes as C

from . import PrtError

H2D, D2H, D2D = 1, 2, 3  # hipMemcpyKind

_P, _N, _I = C.c_void_p, C.c_size_t, C.c_int
SIGNATURES = {
    "hipSetDevice": [_I],
    "hipMalloc": [C.POINTER(_P), _N],
    "hipFree": [_P],
    "hipMemcpy": [_P, _P, _N, _I],
    "hipMemcpyAsync": [_P, _P, _N, _I, _P],
    "hipMemset": [_P, _I, _N],
    "hipMemsetAsync": [_P, _I, _N, _P],
    "hipStreamCreate": [C.POINTER(_P)],
    "hipStreamDestroy": [_P],
    "hipStreamSynchronize": [_P],
    "hipDeviceSynchronize": [],
    "hipGetErrorString": [_I],
}
_runtime = None


def runtime():
    """libamdhip64.so, loaded once per process, with argtypes and restype of every function of SIGNATURES set."""
    global _runtime
    if _runtime is None:
        h = C.CDLL("libamdhip64.so")  # the runtime the library itself is linked to
        for name, argtypes in SIGNATURES.items():
            f = getattr(h, name)
            f.argtypes, f.restype = argtypes, C.c_char_p if name == "hipGetErrorString" else _I
        _runtime = h
    return _runtime


class DeviceArrays:
    """Device memory and streams from the HIP runtime the library is linked to, freed and destroyed on exit.  Addresses and
    streams are ints.  The synchronous copies run on the null stream, which a context's (blocking) stream is ordered with.
    runtime: an object with the functions of SIGNATURES (a test's fake); None: runtime()."""

    def __init__(self, device=0, runtime=None):
        self._h, self._device, self._held, self._streams = runtime, device, [], []

    def _chk(self, rc, call):
        if rc != 0:
            text = self._h.hipGetErrorString(rc)
            raise PrtError(f"{call} failed: {text.decode() if isinstance(text, bytes) else text} ({rc})")

    def __enter__(self):
        if self._h is None:
            self._h = runtime()
        self._chk(self._h.hipSetDevice(self._device), f"hipSetDevice({self._device})")
        return self

    def __exit__(self, *exc):
        streams, held, self._streams, self._held = self._streams, self._held, [], []
        for s in streams:
            self._h.hipStreamSynchronize(s)
            self._h.hipStreamDestroy(s)
        for p in held:
            self._h.hipFree(p)

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self._h.hipMalloc(C.byref(p), max(int(nbytes), 64)), f"hipMalloc of {nbytes} bytes")
        self._held.append(p.value)
        return p.value

    def stream(self):
        s = C.c_void_p()
        self._chk(self._h.hipStreamCreate(C.byref(s)), "hipStreamCreate")
        self._streams.append(s.value)
        return s.value

    def upload(self, a, ptr=None):
        """Copy `a` to ptr (None: a new allocation); returns the device address."""
        p = self.alloc(a.nbytes) if ptr is None else ptr
        self._chk(self._h.hipMemcpy(p, a.ctypes.data, a.nbytes, H2D), "hipMemcpy to the device")
        return p

    def download(self, a, ptr):
        self._chk(self._h.hipMemcpy(a.ctypes.data, ptr, a.nbytes, D2H), "hipMemcpy from the device")

    def fill(self, ptr, byte, nbytes):
        self._chk(self._h.hipMemset(ptr, byte, nbytes), "hipMemset")

    def upload_async(self, a, stream, ptr=None):
        """Queue the copy of `a` to ptr (None: a new allocation) on `stream`; `a` must stay alive until the stream has run it."""
        p = self.alloc(a.nbytes) if ptr is None else ptr
        self._chk(self._h.hipMemcpyAsync(p, a.ctypes.data, a.nbytes, H2D, stream), "hipMemcpyAsync to the device")
        return p

    def download_async(self, a, ptr, stream):
        self._chk(self._h.hipMemcpyAsync(a.ctypes.data, ptr, a.nbytes, D2H, stream), "hipMemcpyAsync from the device")

    def copy_async(self, dst, src, nbytes, stream):
        self._chk(self._h.hipMemcpyAsync(dst, src, nbytes, D2D, stream), "hipMemcpyAsync on the device")

    def fill_async(self, ptr, byte, nbytes, stream):
        self._chk(self._h.hipMemsetAsync(ptr, byte, nbytes, stream), "hipMemsetAsync")

    def synchronize(self, stream=None):
        """Wait for `stream`, or for the whole device when None."""
        if stream is None:
            self._chk(self._h.hipDeviceSynchronize(), "hipDeviceSynchronize")
        else:
            self._chk(self._h.hipStreamSynchronize(stream), "hipStreamSynchronize")
