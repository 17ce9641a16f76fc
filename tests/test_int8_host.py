"""Host-side checks of the w8a8 int8 operator (no GPU): the CPU restatement reproduces the fixture the reference's own operator class made, the
C ABI carries the new entries and refuses what the fp8 twins refuse, and the operator class loads, stores and sizes its tensors as the reference's
does."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
from safetensors import safe_open
from safetensors.torch import load_file, save_file

from tests import int8_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "W-int8-channel-sym-A-int8-channel-sym-dynamic-Hip"
NEW_ENTRIES = ("x2v_quant_int8_rowwise", "x2v_quant_int8_rowwise_blocked", "x2v_layernorm_quant_int8", "x2v_gemm_int8", "x2v_gemm_int8_variant", "x2v_gemm_int8_resid_period",
               "x2v_gemm_int8_blocked", "x2v_gemm_int8_kernel_choice")
E_SHAPE, E_ALIGN, E_ARG = -1, -2, -5  # include/x2v.h
ZERO_ROW, OUTLIER_ROW, TIE_ROW, ZERO_CH, TINY_CH = 3, 5, 7, 7, 9  # tools/gen_golden_int8.py


@pytest.fixture(scope="module")
def fx():
    return load_file(os.path.join(ROOT, "tests", "golden", "int8_mm.safetensors"))


# ------------------------------------------------------------------------------------------------ restatement == fixture
def test_fixture_holds_the_edge_rows(fx):
    x, xq, sx = fx["x"].float(), fx["xq"], fx["sx"]
    assert xq.dtype == torch.int8 and fx["auto_wq"].dtype == torch.int8
    assert not x[ZERO_ROW].any() and not xq[ZERO_ROW].any() and sx[ZERO_ROW].item() == 0.0
    assert x[OUTLIER_ROW].abs().amax() == 300.0 and (xq[OUTLIER_ROW].abs() <= 1).sum() >= x.shape[1] - 8  # the outlier flattens the rest of the row
    assert sx[TIE_ROW].item() == 1.0  # amax exactly 127: every x.5 entry is a tie
    assert xq[TIE_ROW, :6].tolist() == [0, 2, 2, 4, 4, 6] and xq[TIE_ROW, 64:70].tolist() == [0, -2, -2, -4, -4, -6]  # half to even
    w = fx["w"].float()
    assert w[ZERO_CH].abs().amax() == 0 and 0 < w[TINY_CH].abs().amax() < 1e-5
    assert torch.equal(fx["auto_wscale"][[ZERO_CH, TINY_CH]], torch.full((2, 1), 1e-5) / 127)  # the clamp
    assert fx["xq"].min() == -127 or fx["xq"].min() == -128  # symmetric codes reach the range's end
    assert torch.isfinite(fx["auto_y"].float()).all()


def test_restatement_reproduces_the_fixture(fx):
    xq, sx = R.quant_act(fx["x"])
    assert torch.equal(xq, fx["xq"]) and torch.equal(sx, fx["sx"])
    wq, sw = R.quant_weight(fx["w"])
    assert torch.equal(wq, fx["auto_wq"]) and torch.equal(sw, fx["auto_wscale"])
    y = R.gemm(xq, sx, wq, sw, fx["b"])
    assert torch.equal(y.view(torch.int16), fx["auto_y"].view(torch.int16)), "scaled GEMM: not bit-equal with the reference class (auto-quantised)"
    assert torch.equal(y.view(torch.int16), fx["ckpt_y"].view(torch.int16)), "scaled GEMM: not bit-equal with the reference class (checkpoint-loaded)"


# ------------------------------------------------------------------------------------------------ ABI
def test_header_prototypes_and_exports_name_the_new_entries():
    from lightx2v_amd import lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "x2v.h")).read(), flags=re.S)
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/x2v.h"
        assert name in lib.PROTOTYPES and hasattr(so, name), name
    for fp8, int8 in (("x2v_quant_fp8_rowwise", "x2v_quant_int8_rowwise"), ("x2v_quant_fp8_rowwise_blocked", "x2v_quant_int8_rowwise_blocked"),
                      ("x2v_layernorm_quant_fp8", "x2v_layernorm_quant_int8"), ("x2v_gemm_fp8", "x2v_gemm_int8"), ("x2v_gemm_fp8_variant", "x2v_gemm_int8_variant"),
                      ("x2v_gemm_fp8_resid_period", "x2v_gemm_int8_resid_period"), ("x2v_gemm_fp8_blocked", "x2v_gemm_int8_blocked")):
        assert lib.PROTOTYPES[int8] == lib.PROTOTYPES[fp8], f"{int8} must have the signature of {fp8}"
    for fn in ("quant_int8_rowwise", "layernorm_quant_int8", "gemm_int8", "gemm_int8_blocked"):
        assert callable(getattr(lib, fn))


P = 0x10000  # a non-null, 16-byte aligned address: every call below is refused by the argument checks, before anything is read or launched


def _variant(fn, M=256, N=256, K=512, ldx=None, ldw=None, sx=P, variant=0, epilogue=0, resid=None):
    return fn(P, K if ldx is None else ldx, sx, P, K if ldw is None else ldw, P, None, P, N, M, N, K, epilogue, resid, N if resid else 0, None, variant, None)


def test_gemm_argument_checks_return_the_fp8_twins_codes():
    from lightx2v_amd import lib

    i8, f8 = lib._lib.x2v_gemm_int8_variant, lib._lib.x2v_gemm_fp8_variant
    for kw in (dict(K=192), dict(K=64), dict(sx=None), dict(N=12), dict(ldx=500), dict(ldx=520), dict(epilogue=2), dict(M=-1)):
        assert _variant(i8, **kw) == _variant(f8, **kw) != 0, kw
    assert _variant(i8, K=192) == E_SHAPE and _variant(i8, sx=None) == E_ARG and _variant(i8, ldx=520) == E_ALIGN
    assert b"gemm_int8" in lib._lib.x2v_last_error()
    assert _variant(i8, K=65536 + 128) == E_SHAPE and b"65536" in lib._lib.x2v_last_error()  # the int32 accumulator's limit
    for v in (2, 3, 4):  # no int8 ping-pong / one-tile-per-workgroup kernel
        assert _variant(i8, variant=v) == E_ARG, v
    for kw in (dict(N=136), dict(K=384), dict(K=256)):  # shapes the continuous form refuses: N % 256, an odd number of K tiles, fewer than 4
        assert _variant(i8, variant=5, **kw) == _variant(f8, variant=5, **kw) == E_SHAPE, kw
    assert _variant(i8, M=0) == 0  # nothing to do

    # the plain, the residual-period and the blocked entries
    assert lib._lib.x2v_gemm_int8(P, 192, P, P, 192, P, None, P, 256, 256, 256, 192, 0, None, 0, None, None) == E_SHAPE
    rp8, rpf = lib._lib.x2v_gemm_int8_resid_period, lib._lib.x2v_gemm_fp8_resid_period
    for K, resid, period in ((192, P + (1 << 24), 64), (512, None, 64), (512, P, 64)):  # K % 128; no resid; y overlapping a periodic resid
        args = (P, K, P, P, K, P, None, P, 256, 256, 256, K, resid, 256, period, None, 1, None)
        assert rp8(*args) == rpf(*args) != 0, (K, resid, period)
    b8, bf = lib._lib.x2v_gemm_int8_blocked, lib._lib.x2v_gemm_fp8_blocked

    def blocked(fn, K=512, kblock=0, nblock=0, epilogue=0, sx=P):
        return fn(P, kblock or K, kblock, 1 << 16, sx, P, K, P, None, P, nblock or 256, nblock, 1 << 16, 256, 256, K, epilogue, P if epilogue == 2 else None, 256, None, None)

    for kw in (dict(K=192), dict(sx=None), dict(nblock=128, epilogue=2), dict(kblock=192), dict(nblock=100)):
        assert blocked(b8, **kw) == blocked(bf, **kw) != 0, kw
    assert blocked(b8, nblock=128, epilogue=2) == E_ARG  # an N-blocked y with the residual epilogue


def test_quantiser_argument_checks_return_the_fp8_twins_codes():
    from lightx2v_amd import lib

    for tag in ("fp8", "int8"):
        q, qb, ln = (getattr(lib._lib, f"x2v_{n}") for n in (f"quant_{tag}_rowwise", f"quant_{tag}_rowwise_blocked", f"layernorm_quant_{tag}"))
        assert q(None, 128, P, 128, P, 4, 128, None) == E_ARG
        assert q(P, 132, P, 132, P, 4, 132, None) == E_SHAPE  # K % 8
        assert q(P, 16392, P, 16392, P, 4, 16392, None) == E_SHAPE  # K > 16384
        assert q(P, 132, P, 128, P, 4, 128, None) == E_ALIGN
        assert qb(P, 64, 48, 1 << 12, P, 128, P, 4, 128, None) == E_SHAPE  # K block does not divide K
        assert q(P, 128, P, 128, P, 0, 128, None) == 0
        assert ln(P, 512, None, None, None, None, P, 512, P, 4, 512, 1e-6, None) == E_SHAPE  # D <= 512: the two kernels
        assert ln(P, 1024, None, None, P, None, P, 1024, P, 4, 1024, 1e-6, None) == E_ARG  # scale without shift
        assert ln(P, 1024, None, None, None, None, None, 1024, P, 4, 1024, 1e-6, None) == E_ARG
        assert ln(P, 1024, None, None, None, None, P, 1024, P, 0, 1024, 1e-6, None) == 0


def test_kernel_choice_is_host_only_and_reports_the_128_kernel():
    from lightx2v_amd import lib

    assert lib.gemm_int8_kernel_choice(75600, 5120, 5120, with_form=True) == (2, True)  # choose_kernel's rule: the continuous 256x256 kernel
    assert lib.gemm_int8_kernel_choice(75600, 5120, 5120) == lib.gemm_kernel_choice(75600, 5120, 5120, fp8=True)
    assert lib.gemm_int8_kernel_choice(75600, 5000, 5120, with_form=True) == (1, False)  # N % 256: no 256x256 int8 kernel takes it
    assert lib.gemm_int8_kernel_choice(130, 136, 256, with_form=True) == (1, False)
    assert lib._lib.x2v_gemm_int8_kernel_choice(0, 128, 128, 128, 128) == E_SHAPE
    assert lib._lib.x2v_gemm_int8_kernel_choice(128, 128, 192, 192, 192) == E_SHAPE


def test_wrappers_refuse_wrong_dtype_and_host_tensors():
    from lightx2v_amd import lib

    xq, wq = torch.zeros(4, 128, dtype=torch.int8), torch.zeros(8, 128, dtype=torch.int8)
    s = torch.ones(4, 1)
    with pytest.raises(lib.X2VError, match="gemm_int8: operands must be int8"):
        lib.gemm_int8(xq.view(torch.float8_e4m3fn), s, wq, torch.ones(8, 1))
    with pytest.raises(lib.X2VError, match="gemm_int8"):
        lib.gemm_int8(xq, s, wq, torch.ones(8, 1))  # host tensors: no CPU fall-back
    with pytest.raises(lib.X2VError, match="gemm_int8_blocked"):
        lib.gemm_int8_blocked(xq, s, wq, torch.ones(8, 1))
    with pytest.raises(lib.X2VError):
        lib.quant_int8_rowwise(torch.zeros(4, 128, dtype=torch.bfloat16))
    with pytest.raises(lib.X2VError, match="bfloat16"):
        lib.quant_int8_rowwise(torch.zeros(4, 128))


# ------------------------------------------------------------------------------------------------ operator class
def test_registry_key_present_and_duplicate_registration_raises():
    from lightx2v_amd import ops
    from lightx2v_amd.registry import MM_WEIGHT_REGISTER

    assert MM_WEIGHT_REGISTER[KEY] is ops.MMWeightInt8Hip
    assert ops.MMWeightInt8Hip.accepts_blocked and ops.MMWeightInt8Hip.accepts_resid_period
    with pytest.raises(Exception):
        MM_WEIGHT_REGISTER(KEY)(type("Other", (), {}))


def _op(config=None):
    from lightx2v_amd import ops

    op = ops.MMWeightInt8Hip("w.weight", "w.bias")
    op.set_config(config or {})
    return op


def test_class_load_auto_quant_gives_the_fixture_bytes(fx):
    op = _op({"weight_auto_quant": True})
    op.load({"w.weight": fx["w"].clone(), "w.bias": fx["b"].clone()})
    assert op.weight.dtype == torch.int8 and op.weight.is_contiguous() and op.weight_scale.dtype == torch.float32
    assert torch.equal(op.weight, fx["auto_wq"]) and torch.equal(op.weight_scale, fx["auto_wscale"]) and torch.equal(op.bias, fx["b"])
    op2 = _op()  # no auto-quant flag, but a bf16 weight: quantised all the same
    op2.load({"w.weight": fx["w"].clone(), "w.bias": fx["b"].clone()})
    assert torch.equal(op2.weight, fx["auto_wq"])
    op3 = _op()  # checkpoint path: int8 weight + <name>.weight_scale (any float dtype on disk)
    op3.load({"w.weight": fx["auto_wq"].clone(), "w.weight_scale": fx["auto_wscale"].to(torch.float64), "w.bias": fx["b"].clone()})
    assert torch.equal(op3.weight, fx["auto_wq"]) and op3.weight_scale.dtype == torch.float32 and torch.equal(op3.weight_scale, fx["auto_wscale"])


def test_class_state_dict_round_trip_size_and_clear(fx, tmp_path):
    op = _op({"weight_auto_quant": True})
    op.load({"w.weight": fx["w"].clone(), "w.bias": fx["b"].clone()})
    sd = op.state_dict()
    assert sorted(sd) == ["w.bias", "w.weight", "w.weight_scale"] and sd["w.weight"].dtype == torch.int8
    N, K = fx["w"].shape
    assert op._calculate_size() == N * K + N * 4 + N * 2  # int8 weight + fp32 scales + bf16 bias (mm_weight.py:154-158)
    op2 = _op()
    op2.load(sd)
    assert all(torch.equal(getattr(op, a), getattr(op2, a)) for a in ("weight", "weight_scale", "bias"))
    path = str(tmp_path / "w.safetensors")  # load_from_disk: the lazy-load path of the quantised template (mm_weight.py:125-138)
    save_file(sd, path)
    with safe_open(path, framework="pt") as fh:
        from lightx2v_amd import ops

        op3 = ops.MMWeightInt8Hip("w.weight", "w.bias", lazy_load=True, lazy_load_file=fh)
        op3.load_from_disk()
    assert torch.equal(op3.weight, op.weight) and torch.equal(op3.weight_scale, op.weight_scale) and torch.equal(op3.bias, op.bias)
    op.to_cpu()
    assert op.weight.device.type == "cpu"
    nobias = _op()
    nobias.bias_name = None
    nobias.load({"w.weight": fx["auto_wq"], "w.weight_scale": fx["auto_wscale"]})
    assert nobias._calculate_size() == N * K + N * 4 and sorted(nobias.state_dict()) == ["w.weight", "w.weight_scale"]
    op.clear()
    assert op.weight is None and op.weight_scale is None and op.bias is None


def test_class_apply_has_no_cpu_fallback(fx):
    from lightx2v_amd import lib

    op = _op()
    op.load({"w.weight": fx["auto_wq"], "w.weight_scale": fx["auto_wscale"], "w.bias": fx["b"]})
    with pytest.raises(lib.X2VError):
        op.apply(fx["x"])


def test_converter_written_int8_file_loads_into_the_class(tmp_path):
    """tools/convert_ckpt.py --quantized --linear_dtype torch.int8 writes `<name>.weight` int8 + `<name>.weight_scale`; the class takes them as they are."""
    from lightx2v_amd import checkpoint as ck
    from lightx2v_amd import synth

    dims = dict(dim=64, ffn_dim=128, num_heads=1, num_layers=1, text_len=8, text_dim=64)
    src = synth.synth_wan_weights(dims, seed=5, dtype=torch.float32)
    os.makedirs(tmp_path / "src")
    save_file({k: v.contiguous() for k, v in src.items()}, str(tmp_path / "src" / "model.safetensors"))
    out = str(tmp_path / "int8")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_ckpt.py"), "-s", str(tmp_path / "src"), "-o", out, "--quantized", "--linear_dtype", "torch.int8"],
                   check=True, capture_output=True)
    wd = {}
    for f in sorted(os.listdir(out)):
        if f.endswith(".safetensors"):
            wd.update(load_file(os.path.join(out, f)))
    name = "blocks.0.ffn.0"
    assert wd[f"{name}.weight"].dtype == torch.int8
    op = _op()
    op.weight_name, op.weight_scale_name, op.bias_name = f"{name}.weight", f"{name}.weight_scale", f"{name}.bias"
    op.load(wd)
    want_q, want_s = ck.quantize_tensor(src[f"{name}.weight"], torch.int8)
    assert torch.equal(op.weight, want_q) and torch.equal(op.weight, wd[f"{name}.weight"]) and torch.equal(op.weight_scale, want_s.float())
    rq, rs = R.quant_weight(src[f"{name}.weight"])  # the class's own auto-quant rule gives the converter's bytes
    assert torch.equal(rq, want_q) and torch.equal(rs, want_s.float())
