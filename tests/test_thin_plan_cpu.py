"""The thin Linear's host side without a GPU: its argument and refusal logic in a stand-alone program under the host
sanitizers (tools/thin_plan_check.cpp), and the same statuses through the C ABI."""

import ctypes
import os
import shutil
import subprocess

from conftest import ROOT


def test_plan_logic_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/gemm_thin_plan.hpp compiled into a program of its own with -fsanitize=address,undefined on the host side and run:
    every shape of the table at row counts around a block, batched and refused combinations, alignment and handshake."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "thin_plan_check")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "thin_plan_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "thin_plan_check: ok" in ran.stdout, ran.stdout + ran.stderr


def test_refusals_come_back_through_the_abi_without_a_device():
    from anemoi_models_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    keep = ctypes.create_string_buffer(4096 + 64)  # never dereferenced: looked at for NULL and alignment only
    base = (ctypes.addressof(keep) + 63) // 64 * 64

    def args(n, k, m=100, **more):
        a = _lib.LinearThinArgs()
        a.struct_bytes = ctypes.sizeof(_lib.LinearThinArgs)
        a.out_dtype, a.x, a.w, a.y, a.ldx, a.ldy, a.M, a.N, a.K = _lib.BF16, base, base + 64, base + 128, k, n, m, n, k
        for name, value in more.items():
            setattr(a, name, value)
        return a

    assert lib.anemoi_linear_thin(None, None) == _lib.ANEMOI_ERR_INVALID and b"null argument" in lib.anemoi_last_error()
    a = args(80, 1024, struct_bytes=8)
    assert lib.anemoi_linear_thin(ctypes.byref(a), None) == _lib.ANEMOI_ERR_INVALID and b"out of sync" in lib.anemoi_last_error()
    for n, k in ((128, 128), (80, 512), (256, 1024), (64, 64), (8, 256)):
        assert (n, k) not in _lib.THIN_SHAPES
        assert lib.anemoi_linear_thin(ctypes.byref(args(n, k)), None) == _lib.ANEMOI_ERR_UNSUPPORTED
        assert b"no register-resident kernel" in lib.anemoi_last_error()
    assert lib.anemoi_linear_thin(ctypes.byref(args(80, 1024, batch=4)), None) == _lib.ANEMOI_ERR_UNSUPPORTED
    assert lib.anemoi_linear_thin(ctypes.byref(args(256, 256, stats_out=base + 512, residual=base + 1024, ldr=256)), None) \
        == _lib.ANEMOI_ERR_UNSUPPORTED
    assert lib.anemoi_linear_thin(ctypes.byref(args(64, 256, ldx=252)), None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_linear_thin(ctypes.byref(args(64, 256, x=base + 2)), None) == _lib.ANEMOI_ERR_INVALID
    assert b"16-byte aligned" in lib.anemoi_last_error()
    # the table of the Python side is the library's
    for n, k in _lib.THIN_SHAPES:
        st = lib.anemoi_linear_thin(ctypes.byref(args(n, k, x=None)), None)
        assert st == _lib.ANEMOI_ERR_INVALID and b"null pointer" in lib.anemoi_last_error(), (n, k)
