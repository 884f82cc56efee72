"""ctypes access to libbramble_selftest.so (bramble_amd/csrc/selftest_kernels.hip): the probes of the scan unit, the wave
primitives and the rows' CIGARs (cigar_inl.h), and guarded device buffers for them.  Test-only: the product never loads this library."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "bramble_amd", "libbramble_selftest.so")

GUARD = 16                      # items before and after every payload: a multiple of 16 bytes for every type used
OUT_FILL = 0xa5a5a5a5a5a5a5a5   # what outputs hold before a launch
TMP_FILL = 0xc3c3c3c3c3c3c3c3   # what the scratch holds before a launch: nonzero, so no result can depend on zeros there
WAVE_OPS = {"scan": 0, "sum": 1, "max": 2, "min": 3, "or": 4, "and": 5}
WAVE_TYPES = {np.dtype(np.uint32): 0, np.dtype(np.uint64): 1, np.dtype(np.float64): 2}


@functools.lru_cache(maxsize=None)
def lib():
    if not os.path.exists(SO):   # a checkout built before this library existed: make that one target, once
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bramble_amd", "csrc"), "../libbramble_selftest.so"])
    import torch  # noqa: F401  (first, so that the library binds to torch's HIP runtime as libbramble_amd.so does: lib.py)
    L = C.CDLL(SO)
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.brst_scan_tiles_for.restype = i64
    L.brst_scan_tiles_for.argtypes = [i64]
    L.brst_scan_small_tiles.restype = i64
    L.brst_scan_small_tiles.argtypes = []
    for name, args in (("brst_scan_u32", [p, p, i64, p, p, i32, p]), ("brst_scan_u64_inplace", [p, p, i64, p]),
                       ("brst_scan3", [p, i64, p, p, p, p, p, p, p, p, p]), ("brst_top_rounds", [p, i32, i32, p, i64, p]),
                       ("brst_copy8", [p, i32, p, i64, p, p]), ("brst_wave", [p, i32, i32, i32, p, p, i32]), ("brst_block_scan", [p, i32, p, p, p, i32]),
                       ("brst_block_bits", [p, p, p, p, p, i32]), ("brst_wave_turns", [p, p, p, p, p]),
                       ("brst_cigar", [p, p, p, p, i32, p, p, p, p, p, p]), ("brst_pool_holds", [p, C.c_uint64, p, p, i32, p])):
        f = getattr(L, name)
        f.restype, f.argtypes = i32, args
    return L


def tiles_for(n):
    return int(lib().brst_scan_tiles_for(n))


def _fill_of(dtype, fill):
    dtype = np.dtype(dtype)
    return np.frombuffer(int(fill).to_bytes(8, "little"), dtype=np.uint8)[:dtype.itemsize].view(dtype)[0]


class Buf:
    """`n` items of `dtype` on the device, `off` items behind a 16-byte boundary, with GUARD items before and after that hold
    `fill`, as do the items themselves unless `values` is given.  read() brings the items back and asserts that nothing
    around them changed."""

    def __init__(self, dtype, n, off=0, fill=OUT_FILL, values=None):
        import torch
        self.dtype, self.n, self.lo = np.dtype(dtype), int(n), GUARD + off
        self.host = np.full(self.lo + self.n + GUARD, _fill_of(dtype, fill), dtype=self.dtype)
        if values is not None:
            assert np.asarray(values).dtype == self.dtype and np.asarray(values).size == self.n
            self.host[self.lo:self.lo + self.n] = values
        self.t = torch.from_numpy(self.host.view(np.uint8).copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo * self.dtype.itemsize

    def read(self, what="buffer"):
        got = self.t.cpu().numpy().view(self.dtype)
        assert np.array_equal(got[:self.lo], self.host[:self.lo]), "%s: written before its first item" % what
        assert np.array_equal(got[self.lo + self.n:], self.host[self.lo + self.n:]), "%s: written past its last item" % what
        return got[self.lo:self.lo + self.n].copy()

    def assert_untouched(self, what="buffer"):
        assert np.array_equal(self.t.cpu().numpy().view(self.dtype), self.host), "%s: changed" % what


def scratch_for(n, channels=1):
    """the scan's scratch, exactly channels x scan_tiles_for(n) words, prefilled and guarded"""
    return Buf(np.uint64, channels * tiles_for(n), fill=TMP_FILL)


def check_scratch(buf, n, what):
    """nothing written outside the scratch; up to SCAN_SMALL_TILES tiles nothing written in it either (scan_kernels.h)"""
    if tiles_for(n) <= int(lib().brst_scan_small_tiles()):
        buf.assert_untouched(what + ": scratch of a one-launch scan")
    else:
        buf.read(what + ": scratch")


def call(fn, *args):
    import torch
    torch.cuda.synchronize()
    rc = fn(*args)   # (pointers: integers, None for a null pointer; the first one is the stream)
    assert rc == 0, "HIP error %d" % rc
