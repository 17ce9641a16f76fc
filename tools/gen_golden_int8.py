#!/usr/bin/env python
"""Writes tests/golden/int8_mm.safetensors: the reference's own operator class MMWeightWint8channelAint8channeldynamicVllm
(common/ops/mm/mm_weight.py:322-354) — `weight_auto_quant` load from a bf16 weight (:185-201, IntegerQuantizer) and load of a converter-format
pair, then apply() — executed unmodified on CPU through oracle.ref_import, as oracle/gen_golden.py::gen_fp8 does for the fp8 class.

The two vLLM kernels it calls are absent offline.  `torch.ops._C.cutlass_scaled_mm` is the stub of oracle/ref_shims/vllm (it multiplies in fp32:
exact for int8 codes while K * 128 * 128 <= 2^24, hence K <= 1024 here); `scaled_int8_quant` is installed onto that shimmed module below, at run
time, RESTATED from vLLM's dynamic per-token kernel (csrc/quantization/compressed_tensors/int8_quant_kernels.cu, symmetric branch).  As with fp8
the fixture pins the reference's glue — quantiser class, scale handling, transposes, bias — and marks the two kernels' arithmetic as restated.

    python tools/gen_golden_int8.py          (needs the reference checkout; see oracle/ref_import.py)"""
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

M, K, N = 48, 512, 64
ZERO_ROW, OUTLIER_ROW, TIE_ROW = 3, 5, 7  # tokens
ZERO_CH, TINY_CH = 7, 9  # weight rows under the 1e-5 clamp


def scaled_int8_quant(input, scale=None, azp=None, symmetric=True):
    """vLLM's call form at mm_weight.py:248: dynamic, symmetric, per token.  fp32 throughout: scale = absmax / 127, q = rint(x * (127 / absmax))
    saturated to int8; returns (codes, scales [M, 1], None)."""
    if scale is not None or azp is not None or not symmetric:
        raise NotImplementedError("stub covers the reference's only call form: dynamic symmetric per-token scales")
    xf = input.float()
    amax = xf.abs().amax(dim=1, keepdim=True)
    c = torch.tensor(127.0, dtype=torch.float32)
    inv = torch.where(amax > 0, c / amax, torch.zeros_like(amax))
    return torch.round(xf * inv).clamp(-128, 127).to(torch.int8), amax / c, None


def inputs():
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    x[ZERO_ROW] = 0  # an all-zero token: codes 0, scale 0
    x[OUTLIER_ROW, 17] = 300.0  # one dominating outlier: most of the row quantises to 0 / +-1
    tie = torch.zeros(K)
    tie[:64] = torch.arange(64) + 0.5  # 0.5, 1.5, ... 63.5: exact ties at inv = 1, half to even
    tie[64:128] = -(torch.arange(64) + 0.5)
    tie[128] = 127.0  # amax exactly 127
    x[TIE_ROW] = tie.to(torch.bfloat16)
    w = (torch.randn(N, K, generator=gen) / K**0.5).to(torch.bfloat16)
    w[ZERO_CH] = 0
    w[TINY_CH] = (torch.randn(K, generator=gen) * 1e-6).to(torch.bfloat16)
    b = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    return x, w, b


def main():
    ref_import.patch_and_import()
    import vllm._custom_ops as ops
    from lightx2v.utils.registry_factory import MM_WEIGHT_REGISTER

    ops.scaled_int8_quant = scaled_int8_quant
    x, w, b = inputs()
    out = {"x": x, "w": w, "b": b}
    cls = MM_WEIGHT_REGISTER["W-int8-channel-sym-A-int8-channel-sym-dynamic-Vllm"]
    op = cls("w.weight", "w.bias")
    op.set_config({"weight_auto_quant": True})
    op.load({"w.weight": w.clone(), "w.bias": b.clone()})
    out["auto_wq"] = op.weight.t().contiguous()  # stored [N, K]
    out["auto_wscale"] = op.weight_scale.clone()
    out["auto_y"] = op.apply(x.clone())
    out["xq"], out["sx"] = op.act_quant_func(x.clone())
    op2 = cls("w.weight", "w.bias")
    op2.set_config({})
    op2.load({"w.weight": op.weight.t().contiguous().clone(), "w.weight_scale": op.weight_scale.clone(), "w.bias": b.clone()})  # as a loader hands it over
    out["ckpt_y"] = op2.apply(x.clone())
    path = os.path.join(ROOT, "tests", "golden", "int8_mm.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print("int8 fixture:", {k: (tuple(v.shape), str(v.dtype)) for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
