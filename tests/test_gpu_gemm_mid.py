"""x2v_gemm_mid_f16 (csrc/gemm_mid.h: LDS tiles, split K, last-arriving workgroup reduces) against fp64 math with the entry's rounding points, the
ticket's workspace discipline, and the Llama driver's mid_gemm switch against the tiny tower's reference fixture."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ULP16 = 2.0**-10
FLIP_SHARE = 2e-3  # tests/test_gpu_clip.py::FLIP_SHARE
F16 = torch.float16
NONE, RESIDUAL, SWIGLU = 0, 2, 4
ROWS = 351


@functools.lru_cache(maxsize=None)
def _case(N, K, epi):
    """Operands of ROWS rows (x ~ N(0, 1), W ~ N(0, 1) / sqrt(K), resid ~ N(0, 1), bias ~ 0.1 N(0, 1), rounded to fp16) and the fp64 result with the
    entry's rounding points; smaller M take the first rows.  Shared by every test of the shape and never written."""
    g = torch.Generator().manual_seed(N * 7 + K + epi)
    x = torch.randn(ROWS, K, generator=g).half().cuda()
    w = (torch.randn(2 * N if epi == SWIGLU else N, K, generator=g) / K**0.5).half().cuda()
    bias = None if epi == SWIGLU else (torch.randn(N, generator=g) * 0.1).half().cuda()
    resid = torch.randn(ROWS, N, generator=g).half().cuda() if epi == RESIDUAL else None
    acc = x.double() @ w.double().t()
    if epi == SWIGLU:
        gate, up = acc[:, 0::2].to(F16).double(), acc[:, 1::2].to(F16).double()
        ref = gate * torch.sigmoid(gate) * up
    else:
        ref = (acc + bias.double()).to(F16).double()
        if epi == RESIDUAL:
            ref = resid.double() + ref
    return x, w, bias, resid, ref


def _share_outside(got, ref64, what):
    """tests/test_gpu_clip.py::_ulp_check: |got - fp16(ref64)| <= 1 ulp |ref| + 2^-23 except for FLIP_SHARE of the elements."""
    ref, got = ref64.to(F16).double(), got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = ((got - ref).abs() > ULP16 * ref.abs() + 2.0**-23).double().mean().item()
    print(f"{what}: share outside 1 ulp {bad:.2e}, max |d| {(got - ref).abs().max().item():.3e}")
    assert bad <= FLIP_SHARE, f"{what}: {bad:.2e} of elements outside 1 ulp + 2^-23; max |d| {(got - ref).abs().max().item():.3e}"
    return bad


@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("epi", [NONE, RESIDUAL, SWIGLU], ids=["bias", "residual_in_place", "swiglu"])
@pytest.mark.parametrize("N, K", [(136, 2080), (256, 512)])
@pytest.mark.parametrize("M", [127, 128, 129, 351])
def test_gemm_mid_f16_vs_fp64(M, N, K, epi, splits):
    """Below, at and above a row tile and the workload's 351; a partial column tile with a K tail (33 K tiles, the last of 32 elements) and the plain
    case; one range, three, and the library's choice (16 uneven ranges at K = 2080, 4 at K = 512).  y is written into a NaN-poisoned oversized buffer;
    the residual epilogue runs in place.  CPU stand-in (fp32 accumulation of four K ranges summed in order) on these inputs: at most 4.4e-4 outside."""
    from lightx2v_amd import lib
    from tests.util import record

    x, w, bias, resid, ref = _case(N, K, epi)
    store = torch.full((M * N + 4096,), float("nan"), dtype=F16, device="cuda")
    out = store[: M * N].view(M, N)
    if epi == RESIDUAL:
        out.copy_(resid[:M])
    lib.gemm_mid_f16(x[:M], w, bias, epilogue=epi, resid=out if epi == RESIDUAL else None, out=out, splits=splits)
    torch.cuda.synchronize()
    assert torch.isnan(store[M * N :]).all(), "gemm_mid_f16 wrote past its output"
    what = f"gemm_mid_f16 M={M} N={N} K={K} epi={epi} splits={splits}"
    record(what, share_outside_1ulp=_share_outside(out, ref[:M], what))


def test_gemm_mid_f16_ticket_leaves_the_workspace_reusable():
    """Two launches in a row on one workspace that is not cleared in between, three K ranges, residual epilogue, then a launch of another shape (other tile
    and slot counts) and the first once more: equal bits every time, and every counter word of the workspace (its first 4096 bytes, whatever the shape)
    is zero afterwards."""
    from lightx2v_amd import lib

    M, N, K = 351, 136, 2080
    x, w, bias, resid, ref = _case(N, K, RESIDUAL)
    outs = [lib.gemm_mid_f16(x, w, bias, epilogue=RESIDUAL, resid=resid, splits=3) for _ in range(2)]
    x2, w2, bias2, _, _ = _case(256, 512, NONE)
    lib.gemm_mid_f16(x2, w2, bias2, splits=0)
    outs.append(lib.gemm_mid_f16(x, w, bias, epilogue=RESIDUAL, resid=resid, splits=3))
    torch.cuda.synchronize()
    ws = lib.gemm_mid_workspace(x.device)
    assert ws.numel() * 4 >= lib._lib.x2v_gemm_mid_workspace_bytes(M, N, K, 3) and not ws[:1024].any(), "a tile counter was left non-zero"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _share_outside(outs[1], ref, "gemm_mid_f16 second launch on the same workspace")


def test_llama_tower_mid_gemm_vs_reference_fixture():
    """The tiny tower with mid_gemm=True on the fixture's prompts of 130 and 136 valid tokens (>= 128 packed rows): tests/test_gpu_hunyuan_text.py's
    triangle against the reference's fp16 output, and the plan's four Linears per layer are x2v_gemm_mid_f16 launches; a 96-token prompt keeps x2v_gemm_f16."""
    from lightx2v_amd import lib, llama, synth
    from tests import llama_restatement as R
    from tests.test_gpu_hunyuan_text import _triangle
    from tests.util import load_golden

    gold = load_golden("llama_encoder_tiny")
    dims = synth.LLAMA_DIMS["llama-tiny"]
    sd = synth.synth_llama_weights(dims, seed=int(gold["seed"][0]))
    with torch.no_grad():
        truth = R.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=torch.float64)[0]
    m = llama.TextEncoderHFLlamaModel((sd, dims), "cuda", mid_gemm=True)
    lens = gold["mask"].sum(1).tolist()
    for b in (3, 2, 0):
        n = lens[b]
        states, _ = m.infer_ids(gold["ids"][b : b + 1], gold["mask"][b : b + 1])
        assert not states[0, n - 95 :].any()
        _triangle(states[0, : n - 95], gold["out_f16"][b, : n - 95], truth[b, : n - 95], f"llama tiny tower, mid_gemm, prompt {b} ({n} tokens)")
        names = [fn.__name__ for fn, _ in m._plan((n,), lib._stream())]
        want = "x2v_gemm_mid_f16" if n >= llama.MID_GEMM_ROWS else "x2v_gemm_f16"
        assert names.count(want) == 4 * m.num_layers and sum("gemm" in s for s in names) == 4 * m.num_layers, names
