"""``GraphTransformerMapperBlock.route``: the one route decision of the mapper block as a table.  The expectation is the
precedence list of DESIGN.md section 4.2 restated here on the switches and the row descriptions -- it never calls the function
under test."""

import inspect
import itertools

import pytest
import torch

import _dec_fold_ref as R
from anemoi_models_amd import runtime
from anemoi_models_amd.layers import block as block_module
from anemoi_models_amd.layers.block import Rows

BF16, F32 = torch.bfloat16, torch.float32
SWITCHES = {"ANEMOI_AMD_DEC_FOLD": "1", "ANEMOI_AMD_EDGE_RAW": "1", "ANEMOI_AMD_EDGE_FOLD": "1", "ANEMOI_AMD_LN_FOLD": "1",
            "ANEMOI_AMD_EMBED_FOLD": "1", "ANEMOI_AMD_THIN_STATS": "0", "ANEMOI_AMD_MXFP8": "0"}  # name -> default
NON_DEFAULT = {name: "0" if default == "1" else "1" for name, default in SWITCHES.items()}
MX_HALO = (NotImplementedError, "ANEMOI_AMD_MXFP8=1: the node-partitioned forward has no MXFP8 route")
HALO_UNFOLDED = (NotImplementedError, "node-partitioned blocks need the folded edge kernel")


def _expected(case, env, dtype, src, dst, chunks, halo, update_src, gpu, grad=False):
    """``(route name, up, mx, chunked, block tail, src_h, dst_h)`` or ``(exception type, message)``: the precedence list."""
    d, heads, ks, k_in, one_col = case["d"], 16, case["ks"], case["k_in"], case["one_col"]
    on = lambda name: env[name] != "0"  # noqa: E731
    bf16 = dtype == BF16
    ln_fold = bf16 and on("ANEMOI_AMD_LN_FOLD")
    embed_fold = ln_fold and on("ANEMOI_AMD_EMBED_FOLD")
    mxfp8 = bf16 and env["ANEMOI_AMD_MXFP8"] == "1"
    mx = mxfp8  # (these blocks keep ``mx_node_mlp``; their widths, 512 and 1024, are multiples of 128)
    if mx and halo:
        return MX_HALO
    up = case["up"] if on("ANEMOI_AMD_EDGE_FOLD") else None  # (both cases have shapes the folded kernel takes, bf16 and f32)
    plain = bf16 and chunks == 1 and not halo and not update_src and up is not None
    sum_col = ks - 1 if one_col != ks - 1 else ks - 2
    if (plain and dst == "raw" and src == "tensor" and gpu and on("ANEMOI_AMD_DEC_FOLD") and not grad and not mxfp8
            and embed_fold and ks in (64, 128, 256) and env["ANEMOI_AMD_THIN_STATS"] != "1" and (heads * (d + up)) % 64 == 0):
        name = "dec_fold"
    elif (plain and src == "raw" and not mx and gpu and on("ANEMOI_AMD_EDGE_RAW") and heads == 16 and ks in (64, 128, 256)
          and sum_col >= k_in):
        name = "raw_sources"
    elif up is not None:
        name = "folded"
    elif halo:
        return HALO_UNFOLDED
    else:
        name = "unfolded"
    block_tail = name == "folded" and chunks == 1 and not update_src and not mx
    return name, up, mx, chunks > 1, block_tail, update_src, name != "dec_fold"


def _rows(case, kind, gpu):
    return Rows(on_gpu=gpu) if kind == "tensor" else Rows(kind, case["ks"], case["one_col"], case["k_in"], gpu)


def _check(blk, case, env, dtype, src, dst, chunks, halo, update_src, gpu, grad=False):
    blk.update_src_nodes = update_src
    want = _expected(case, env, dtype, src, dst, chunks, halo, update_src, gpu, grad)
    what = f"{dtype} src={src} dst={dst} chunks={chunks} halo={halo} update_src={update_src} gpu={gpu}"
    args = (dtype, _rows(case, src, gpu), _rows(case, dst, gpu), chunks, halo)
    if isinstance(want[0], type):
        with pytest.raises(want[0]) as err:
            blk.route(*args)
        assert str(err.value) == want[1], what
    else:
        assert tuple(blk.route(*args)) == want, what
    return want[0]


@pytest.fixture(scope="module", params=[(64, 32, 8), (256, 64, 4)], ids=lambda s: "Ks%d_D%d_up%d" % s)
def case(request):
    return R.block_case(*request.param)


@pytest.mark.parametrize("switch", [None] + list(SWITCHES))
def test_route_table(monkeypatch, case, switch):
    """Every combination of dtype, source kind, destination kind, chunks, halo, ``update_src_nodes`` and device, at the default
    switches and with each switch alone at its non-default value."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    env = dict(SWITCHES)
    if switch is not None:
        env[switch] = NON_DEFAULT[switch]
        monkeypatch.setenv(switch, NON_DEFAULT[switch])
    blk = case["blk"]
    monkeypatch.setattr(blk, "update_src_nodes", False)  # (restored after the test; _check sets it per combination)
    seen = set()
    kinds = ("tensor", "embedded", "raw")
    with torch.no_grad():
        for combo in itertools.product((BF16, F32), kinds, kinds, (1, 2), (False, True), (False, True), (False, True)):
            seen.add(_check(blk, case, env, *combo))
    if switch is None:
        assert seen == {"dec_fold", "raw_sources", "folded"}
    print(f"{switch}={NON_DEFAULT.get(switch)}: {sorted(str(s) for s in seen)}")
    # the table above is not vacuous: each switch removes, or brings, what it is there for
    absent = {"ANEMOI_AMD_DEC_FOLD": "dec_fold", "ANEMOI_AMD_EDGE_RAW": "raw_sources", "ANEMOI_AMD_EMBED_FOLD": "dec_fold",
              "ANEMOI_AMD_THIN_STATS": "dec_fold", "ANEMOI_AMD_MXFP8": "dec_fold"}
    if switch in absent:
        assert absent[switch] not in seen
    if switch == "ANEMOI_AMD_LN_FOLD":
        assert "dec_fold" not in seen and "raw_sources" in seen  # (rows that are EmbeddedRows stay a caller's choice)
    if switch == "ANEMOI_AMD_EDGE_FOLD":
        assert "unfolded" in seen and NotImplementedError in seen and not seen & {"dec_fold", "raw_sources", "folded"}
    if switch == "ANEMOI_AMD_MXFP8":
        assert NotImplementedError in seen


def test_grad_mode_takes_neither_the_decoder_fold_nor_the_hoist(monkeypatch, case):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.delenv("ANEMOI_AMD_ENC_HOIST", raising=False)
    blk = case["blk"]
    monkeypatch.setattr(blk, "update_src_nodes", False)
    with torch.no_grad():
        assert _check(blk, case, SWITCHES, BF16, "tensor", "raw", 1, False, False, True) == "dec_fold"
        assert runtime.enc_hoist_enabled()
    with torch.enable_grad():
        assert _check(blk, case, SWITCHES, BF16, "tensor", "raw", 1, False, False, True, grad=True) == "folded"
        assert _check(blk, case, SWITCHES, BF16, "raw", "embedded", 1, False, False, True, grad=True) == "raw_sources"
        assert not runtime.enc_hoist_enabled()  # ... whose destination side is then recomputed on every call


def test_dec_fold_route_is_a_view_of_the_decision(monkeypatch):
    """``dec_fold_route(dtype, k_pad, num_chunks)`` == "the decision for plain sources and raw destination rows on the GPU is
    ``dec_fold``", on the cases of ``test_dec_fold_cpu.test_route_conditions``."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    blk = R.block_case(64, 32, 8)["blk"]

    def both(dtype, k_pad, num_chunks=1):
        view = blk.dec_fold_route(dtype, k_pad, num_chunks)
        decided = blk.route(dtype, Rows(), Rows("raw", k_pad, on_gpu=True), num_chunks).name == "dec_fold"
        assert view == decided
        return view

    with torch.no_grad():
        assert both(BF16, 64) and both(BF16, 128) and both(BF16, 256)
        assert not both(BF16, 192) and not both(F32, 64) and not both(BF16, 64, 2)
        for name, value in (("ANEMOI_AMD_DEC_FOLD", "0"), ("ANEMOI_AMD_THIN_STATS", "1"), ("ANEMOI_AMD_MXFP8", "1"),
                            ("ANEMOI_AMD_EDGE_FOLD", "0"), ("ANEMOI_AMD_EMBED_FOLD", "0")):
            monkeypatch.setenv(name, value)
            assert not both(BF16, 64), name
            monkeypatch.delenv(name)
        assert both(BF16, 64)
    with torch.enable_grad():
        assert not both(BF16, 64)


def test_block_module_reads_no_switch_itself():
    """Every switch has its predicate in ``runtime``: ``layers/block.py`` reads the environment in ``inference_num_chunks``
    (the reference's own variable) and nowhere else."""
    source = inspect.getsource(block_module)
    own = inspect.getsource(block_module.inference_num_chunks)
    assert "os.environ" in own and source.count(own) == 1
    assert "os.environ" not in source.replace(own, "") and "getenv" not in source
