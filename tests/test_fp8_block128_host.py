"""fp8 block-128 linear layers without a GPU: the registry key, the weight quantiser at load against the reference's per_block_cast_to_fp8
(mm_weight.py:218-230) bit for bit, the state_dict round trip, and the argument refusals of the two C entries (before any HIP call)."""
import ctypes

import pytest
import torch

KEY = "W-fp8-block128-sym-A-fp8-channel-group128-sym-dynamic-Hip"


def _op(config):
    from lightx2v_amd import ops, registry

    assert registry.MM_WEIGHT_REGISTER[KEY] is ops.MMWeightFp8Block128Hip
    op = registry.MM_WEIGHT_REGISTER[KEY]("w.weight", "w.bias")
    op.set_config(config)
    return op


def per_block_cast_to_fp8(x):  # the reference's lines, with ceil_div written out
    m, n = x.shape
    x_padded = torch.zeros((-(-m // 128) * 128, -(-n // 128) * 128), dtype=x.dtype, device=x.device)
    x_padded[:m, :n] = x
    x_view = x_padded.view(-1, 128, x_padded.size(1) // 128, 128)
    x_amax = x_view.abs().float().amax(dim=(1, 3), keepdim=True).clamp(1e-4)
    x_scaled = (x_view * (448.0 / x_amax)).to(torch.float8_e4m3fn)
    return x_scaled.view_as(x_padded)[:m, :n].contiguous(), (x_amax / 448.0).view(x_view.size(0), x_view.size(2))


@pytest.mark.parametrize("shape", [(256, 384), (200, 256)])
def test_load_quantises_per_block_as_the_reference_and_round_trips(shape):
    g = torch.Generator().manual_seed(shape[0])
    w = (torch.randn(*shape, generator=g) / 16).to(torch.bfloat16)
    w[:128, :128] = 0  # a block under the 1e-4 clamp
    op = _op({"weight_auto_quant": True})
    op.load({"w.weight": w, "w.bias": torch.randn(shape[0], generator=g).to(torch.bfloat16)})
    codes, scales = per_block_cast_to_fp8(w)
    assert op.weight.dtype == torch.float8_e4m3fn and torch.equal(op.weight.view(torch.uint8), codes.view(torch.uint8))
    assert op.weight_scale.shape == (-(-shape[0] // 128), shape[1] // 128) and torch.equal(op.weight_scale, scales)
    sd = op.state_dict()
    assert set(sd) == {"w.weight", "w.weight_scale", "w.bias"}
    again = _op({})
    again.load(sd)  # an e4m3 weight with its scale: taken as it is
    assert all(torch.equal(getattr(again, a).view(torch.uint8), getattr(op, a).view(torch.uint8)) for a in ("weight", "weight_scale", "bias"))
    assert op._calculate_size() == w.numel() + 4 * scales.numel() + 2 * shape[0]


def test_entries_refuse_bad_arguments_before_any_hip_call():
    from lightx2v_amd import lib

    L, a, SHAPE, ARG = lib._lib, ctypes.c_void_p(4096), -1, -5
    # x2v_quant_fp8_group128(x, ldx, xq, ldq, sx, lds, M, K, stream)
    assert L.x2v_quant_fp8_group128(a, 256, a, 256, a, 4, 4, 192, None) == SHAPE and b"K=192" in L.x2v_last_error()
    assert L.x2v_quant_fp8_group128(a, 256, a, 256, None, 4, 4, 256, None) == ARG
    assert L.x2v_quant_fp8_group128(a, 256, a, 256, a, 3, 4, 256, None) == SHAPE and b"lds=3" in L.x2v_last_error()
    # x2v_gemm_fp8_block128(xq, ldx, sx, lds, wq, ldw, sw, ldsw, bias, y, ldy, M, N, K, epilogue, resid, ldr, gate, stream)
    gemm = lambda sx=a, lds=4, K=256, epi=0: L.x2v_gemm_fp8_block128(a, 256, sx, lds, a, 256, a, 2, None, a, 64, 4, 64, K, epi, None, 0, None, None)
    assert gemm(K=192) == SHAPE and b"K=192" in L.x2v_last_error()
    assert gemm(sx=None) == ARG
    assert gemm(lds=3) == SHAPE and b"lds=3" in L.x2v_last_error()
    assert gemm(epi=lib.EPI_RESIDUAL) == ARG and b"resid" in L.x2v_last_error()
