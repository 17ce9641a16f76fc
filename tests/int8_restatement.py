"""CPU restatement of the w8a8 int8 operator's numeric contract (include/x2v.h), in plain PyTorch and in the kernels' statement order.  Nothing
here imports the package: it is the reference tests/test_int8_host.py pins to the fixture tests/golden/int8_mm.safetensors (made by the
reference's own operator class, tools/gen_golden_int8.py) and tests/test_gpu_int8.py compares the kernels with.

  quant_act     vLLM's dynamic scaled_int8_quant(x, scale=None, azp=None, symmetric=True), restated; every operation one fp32 operation
  quant_weight  the reference's IntegerQuantizer(8, True, "per_channel") (utils/quant_utils.py:93-113) as mm_weight.py:185-201 calls it
  gemm          the integer product exactly (int64), rounded to fp32 once, then the fp32 epilogue: * sx * sw, + bias, activation, residual
"""
import torch

EPI_NONE, EPI_GELU_TANH, EPI_RESIDUAL, EPI_SILU = 0, 1, 2, 3


def quant_act(x):
    """x [M, K] bf16 (or fp32) -> (int8 codes [M, K], fp32 scales [M, 1])."""
    xf = x.to(torch.float32)
    amax = xf.abs().amax(dim=1, keepdim=True)
    one27 = torch.tensor(127.0, dtype=torch.float32)
    scale = amax / one27
    inv = torch.where(amax > 0, one27 / amax, torch.zeros_like(amax))  # an all-zero row: codes 0, scale 0, no NaN
    q = torch.round(xf * inv).clamp(-128, 127)  # torch.round: half to even
    return q.to(torch.int8), scale


def quant_weight(w):
    """w [N, K] -> (int8 codes [N, K], fp32 scales [N, 1])."""
    wf = w.to(torch.float32)
    scale = wf.abs().amax(dim=1, keepdim=True).clamp(min=1e-5) / torch.tensor(127.0, dtype=torch.float32)
    return torch.round(wf / scale).clamp(-128, 127).to(torch.int8), scale


def _rbf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def gemm(xq, sx, wq, sw, bias=None, epilogue=EPI_NONE, resid=None, gate=None, resid_period=0):
    """epi(float(xq . wq^T) * sx[m] * sw[n] + bias[n]) -> bf16.  The residual epilogue rounds y to bf16, then resid + bf16(y * gate) (or
    resid + y), as the bf16 and fp8 kernels do; resid_period: output row r reads resid row r mod resid_period."""
    acc = xq.to(torch.int64) @ wq.to(torch.int64).t()  # exact
    v = acc.to(torch.float32)  # one rounding, to nearest even (|acc| may exceed 2^24)
    v = v * sx.reshape(-1, 1).to(torch.float32) * sw.reshape(1, -1).to(torch.float32)
    if bias is not None:
        v = v + bias.reshape(1, -1).to(torch.float32)
    if epilogue == EPI_GELU_TANH:
        v = torch.nn.functional.gelu(_rbf(v), approximate="tanh")
    elif epilogue == EPI_SILU:
        v = torch.nn.functional.silu(_rbf(v))
    elif epilogue == EPI_RESIDUAL:
        y = _rbf(v)
        r = resid.to(torch.float32)
        if resid_period:
            r = r[torch.arange(y.shape[0]) % resid_period]
        v = r + (_rbf(y * gate.reshape(1, -1).to(torch.float32)) if gate is not None else y)
    return v.to(torch.bfloat16)
