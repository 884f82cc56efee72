"""SAM text out without a GPU: the new C ABI symbols and the command line's usage errors for -O / --output-fmt (they are
found before any device is touched, and leave no output file)."""
import ctypes as C
import os
import subprocess

from bramble_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")


def test_sam_out_symbols_and_argument_checks():
    L = lib.lib()
    for name in ("br_ctx_set_sam_refs", "br_sam_format_device"):
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_ctx_set_sam_refs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.br_sam_format_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.br_ctx_set_sam_refs(None, None, 0) == -1
    assert L.br_sam_format_device(None, None, None, None, None) == -1
    assert lib.OUT_SAM_TEXT == 2 and lib.KERNEL_NAMES[lib.K_SAM_FORMAT] == "k_samfmt_*" and len(lib.KERNEL_NAMES) == lib.K_NUM


def run(tmp_path, *args):
    out = str(tmp_path / "out.sam")
    r = subprocess.run([BIN, str(tmp_path / "in.bam"), "-G", str(tmp_path / "g.gtf"), "-o", out] + list(args),
                       capture_output=True, text=True, timeout=60)
    return r, out


def test_output_format_usage_errors_leave_no_file(tmp_path):
    for args in (["--output-fmt", "cram"], ["-O", "sam", "--compression-level", "3"], ["--output-fmt=SAM", "--host-deflate"],
                 ["-O", "sam", "--device-deflate"], ["-O"]):
        r, out = run(tmp_path, *args)
        assert r.returncode == 2, (args, r.stderr)
        assert "usage" in r.stderr and not os.listdir(tmp_path), args


def test_output_format_in_usage():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--output-fmt bam|sam" in r.stdout
