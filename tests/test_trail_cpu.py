"""Launch trail without a GPU: the two host references of the record agree, known answers of the digest, the argument checks
of the C ABI that come before any device call, and a static check that every exported entry point carries the hook."""

import ctypes
import glob
import os
import re

import pytest
import torch

from _trail_ref import GOLDEN
from _trail_ref import MASK
from _trail_ref import m
from _trail_ref import numpy_record
from _trail_ref import torch_record
from conftest import ROOT


def _seeded(dtype, rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype in (torch.float32, torch.bfloat16):
        return (torch.randn(rows, cols, generator=g) * 3).to(dtype)
    if dtype == torch.int32:
        return torch.randint(-2**31, 2**31 - 1, (rows, cols), generator=g, dtype=torch.int64).to(torch.int32)
    return torch.randint(0, 256, (rows, cols), generator=g, dtype=torch.int64).to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32, torch.uint8])
@pytest.mark.parametrize("rows,cols", [(0, 5), (1, 1), (7, 3), (33, 129)])
def test_the_two_references_agree(dtype, rows, cols):
    x = _seeded(dtype, rows, cols, 11 * rows + cols)
    want = numpy_record(x)
    assert torch_record(x) == want
    assert torch_record(x, chunk_rows=2) == want  # chunking changes nothing: the sum is order independent
    # a strided view enters by its logical elements only
    wide = _seeded(dtype, rows, cols + 3, 5)
    wide[:, :cols] = x
    assert numpy_record(wide[:, :cols]) == want and torch_record(wide[:, :cols]) == want


def test_known_answers():
    assert numpy_record(torch.zeros(0, 4))[0] == 0 and torch_record(torch.zeros(0, 4))[0] == 0
    assert m(0) == (GOLDEN | 1) == 0x9E3779B97F4A7C15 | 1
    for dtype in (torch.float32, torch.bfloat16, torch.int32, torch.uint8):
        assert numpy_record(torch.zeros(1, 1, dtype=dtype))[0] == m(0)  # (0 + 1) * m(0)
    # two elements by hand
    x = torch.tensor([[1.0, -2.0]])
    b0, b1 = 0x3F800000, 0xC0000000
    assert numpy_record(x)[0] == ((b0 + 1) * m(0) + (b1 + 1) * m(1)) & MASK
    # swapping two unequal elements changes the digest; so does the sign of a zero
    assert numpy_record(torch.tensor([[1.0, 2.0, 3.0]]))[0] != numpy_record(torch.tensor([[2.0, 1.0, 3.0]]))[0]
    assert numpy_record(torch.tensor([[0.0]]))[0] != numpy_record(torch.tensor([[-0.0]]))[0]
    # the other two fields
    y = torch.tensor([[float("nan"), float("inf"), -float("inf"), -7.5, 2.0]])
    assert numpy_record(y)[1:] == (3, 7.5) and torch_record(y)[1:] == (3, 7.5)
    assert numpy_record(torch.tensor([[float("nan")]]))[1:] == (1, 0.0)


def test_trail_abi_argument_checks_without_a_device():
    from anemoi_models_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    keep = ctypes.create_string_buffer(64)  # never dereferenced by the host side: only its address is taken
    ptr = ctypes.addressof(keep)
    n, d = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.anemoi_trail_end(ctypes.byref(n), ctypes.byref(d)) == _lib.ANEMOI_ERR_INVALID  # end without begin
    assert b"no trail is armed" in lib.anemoi_last_error()
    assert lib.anemoi_trail_begin(None, 8) == _lib.ANEMOI_ERR_INVALID
    assert b"null record buffer" in lib.anemoi_last_error()
    assert lib.anemoi_trail_begin(ptr, 0) == _lib.ANEMOI_ERR_INVALID
    assert b"not positive" in lib.anemoi_last_error()
    assert lib.anemoi_trail_note(b"nothing armed", _lib.F32, ptr, 4, 1, 4, None) == _lib.ANEMOI_OK
    assert lib.anemoi_trail_begin(ptr, 2) == _lib.ANEMOI_OK
    try:
        assert lib.anemoi_trail_begin(ptr, 2) == _lib.ANEMOI_ERR_INVALID
        assert b"already armed" in lib.anemoi_last_error()
    finally:
        assert lib.anemoi_trail_end(ctypes.byref(n), ctypes.byref(d)) == _lib.ANEMOI_OK
    assert (n.value, d.value) == (0, 0)
    assert lib.anemoi_trail_entry(0, None, None, None, None) == _lib.ANEMOI_ERR_INVALID
    assert lib.anemoi_trail_end(None, None) == _lib.ANEMOI_ERR_INVALID  # disarmed again


# entry points that launch nothing themselves: every kernel behind them runs through another exported entry point, which
# carries the hook (at most 10 names)
HOOK_EXEMPT = {
    "anemoi_gt_block_tail": "calls the edge-attention and Linear entry points only",
    "anemoi_gt_processor_block_forward": "calls anemoi_linear_ln and the block tail only",
    "anemoi_transformer_block_forward": "calls anemoi_layer_norm / anemoi_linear / anemoi_mhsa only",
}


def _functions(text):
    """{name: (signature, body)} of the function definitions `int name(...) {` that start a line of one .hip file."""
    out = {}
    for mt in re.finditer(r'^(extern "C" |static |static inline )?int (\w+)\(', text, flags=re.M):
        depth, i = 0, mt.end() - 1
        while True:  # matching parenthesis of the parameter list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
            if depth == 0:
                break
        rest = text[i:].lstrip()
        if not rest.startswith("{"):
            continue  # a declaration
        start = text.index("{", i)
        depth, j = 0, start
        while True:
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
            if depth == 0:
                break
        out[mt.group(2)] = (text[mt.start():i], text[start:j])
    return out


def test_every_exported_entry_point_that_launches_carries_the_hook():
    assert len(HOOK_EXEMPT) <= 10
    seen, launching = set(), 0
    for path in sorted(glob.glob(os.path.join(ROOT, "anemoi_models_amd", "csrc", "*.hip"))):
        funcs = _functions(open(path).read())
        for name, (sig, body) in funcs.items():
            if not name.startswith("anemoi_"):
                continue
            seen.add(name)
            # the rule as stated: a body that checks a launch notes its outputs -- the entry point's own body together with
            # the helpers of its file that it calls (the folded edge phase's five entry points launch in one)
            called = [hb for h, (_, hb) in funcs.items() if not h.startswith("anemoi_") and re.search(r"\b" + h + r"\s*[<(]", body)]
            if any("check_launch(" in b for b in [body] + called):
                launching += 1
                assert any("trail::note(" in b for b in [body] + called) or name in HOOK_EXEMPT, \
                    f"{name} ({os.path.basename(path)}) launches without trail::note"
            # and the stronger one: every entry point that takes a stream is hooked itself, or through a helper of its file
            if "anemoi_stream_t stream" not in sig:
                continue
            helpers = [h for h, (_, hb) in funcs.items() if not h.startswith("anemoi_") and "trail::note(" in hb
                       and re.search(r"\b" + h + r"\s*[<(]", body)]
            assert "trail::note(" in body or helpers or name in HOOK_EXEMPT, f"{name} ({os.path.basename(path)}) carries no hook"
    assert launching >= 30 and {"anemoi_linear", "anemoi_mhsa", "anemoi_weight_grad_tn", "anemoi_linear_mx"} <= seen
    assert set(HOOK_EXEMPT) <= seen
