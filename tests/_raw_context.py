"""What every GPU test file needs of ctypes (TEST infrastructure): an array as a void pointer, and a context of another build of the
library — the race-stress build the jitter tests run on."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _RawContext:
    """A context of another build of the library (ctypes only: the package binds the product library).
    entries: {entry name: argtypes} of what the test calls through it."""

    def __init__(self, path, entries, flags=0):
        self.lib = C.CDLL(path)
        vp = C.c_void_p
        self.lib.tl_create.argtypes = [C.c_int, C.c_uint32, C.POINTER(vp)]
        self.lib.tl_destroy.argtypes = [vp]
        self.lib.tl_destroy.restype = None
        self.lib.tl_last_error.argtypes = [vp]
        self.lib.tl_last_error.restype = C.c_char_p
        self.lib.tl_device_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        for name, argtypes in entries.items():
            getattr(self.lib, name).argtypes = argtypes
        self.handle = vp()
        rc = self.lib.tl_create(0, flags, C.byref(self.handle))
        assert rc == 0, self.lib.tl_last_error(None)

    @property
    def cus(self):
        cus = C.c_int()
        assert self.lib.tl_device_info(self.handle, C.byref(cus), None, None, 0) == 0
        return cus.value

    def close(self):
        self.lib.tl_destroy(self.handle)


def jitter_context(entries, flags=0):
    """the race-stress build (-DTL_JITTER: waves leave every barrier far apart); close() it in a `finally`"""
    lib = os.path.join(ROOT, "teeline_amd", "libteeline_gpu_jitter.so")
    assert os.path.exists(lib), "built by __graft_entry__.build()"
    return _RawContext(lib, entries, flags)
