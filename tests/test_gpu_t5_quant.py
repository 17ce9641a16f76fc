"""The quantised umT5 text encoder on the HIP kernels (csrc/gemm_rows8.h, csrc/t5_quant.hip, lightx2v_amd/t5.py with t5_quantized): the 8-bit
weight-streaming GEMM against exact arithmetic, the fused norm + quantiser against its two kernels, and the encoder against the fp64 restatement
(tests/t5_quant_restatement.py) with the reference-order bf16 restatement as the yardstick.  Bars and helpers are tests/test_gpu_t5.py's."""
import pytest
import torch

from tests.test_gpu_t5 import BF, _gelu64, _rel, _triangle, _ulp_check, gold  # noqa: F401  (gold: the fixture)

pytestmark = pytest.mark.gpu

KINDS = {"int8": (torch.int8, 64, 4), "fp8": (torch.float8_e4m3fn, 128, 2)}  # codes dtype, k-step, ring depth (csrc/gemm_rows8.h)
MS = (1, 37, 203, 300)


def _shapes(kstep, ring):
    """(N, K, GEGLU): the encoder's Linears at the tiny widths, an N tail that is no multiple of 16, K of one k-step and of ring - 1, ring, ring + 1
    k-steps, and one released-width pair per epilogue."""
    edge = [(64, s * kstep, False) for s in sorted({1, ring - 1, ring, ring + 1})]
    return [(768, 256, False), (640, 256, True), (256, 640, False), (484, 256, False), *edge, (4096, 4096, False), (10240, 4096, True), (4096, 10240, False)]


GEMM_CASES = [(kind, *s) for kind, (_, kstep, ring) in KINDS.items() for s in _shapes(kstep, ring)]


def _scales(kind, n, K, g, device):
    """Positive, over three binades, around the value at which sx * sw undoes the accumulator's spread (codes of standard deviation ~74 for int8, ~128 for
    e4m3: |acc| ~ std^2 sqrt(K)), so that the outputs are O(1) as the 16-bit test's are."""
    return (torch.exp2(3 * torch.rand(n, generator=g) - 1.5) / ((74.0 if kind == "int8" else 128.0) * K**0.25)).to(device)


def _codes(kind, rows, K, g, device):
    """int8: uniform over the full range with -128 present; e4m3: N(0, 1) rows quantised per row as the quantisers do (amax -> 448)."""
    if kind == "int8":
        q = torch.randint(-128, 128, (rows, K), generator=g, dtype=torch.int8)
        q[0, 0] = -128
        return q.to(device)
    x = torch.randn(rows, K, generator=g)
    return (x / (x.abs().amax(dim=1, keepdim=True) / 448)).to(torch.float8_e4m3fn).to(device)


def _expected(kind, acc64, sx, sw, resid, geglu):
    """[(epilogue, resid, reference, exact)]: exact references are bf16 tensors to equal bit for bit — int8 without a transcendental: the exact integer
    sum (float64 holds it) converted to fp32, times sx, times sw in fp32, with the epilogue's bf16 roundings — the others float64 for the 1-ulp check."""
    from lightx2v_amd import lib

    v64 = acc64 * sx.double()[:, None] * sw.double()[None, :]
    if geglu:
        return [(lib.EPIR_GEGLU, None, v64[:, 0::2].to(BF).double() * _gelu64(v64[:, 1::2].to(BF).double()), False)]
    if kind == "int8":
        v = ((acc64.float() * sx[:, None]) * sw[None, :]).to(BF)
        return [(lib.EPIR_NONE, None, v, True), (lib.EPIR_RESIDUAL, resid, (resid.float() + v.float()).to(BF), True)]
    return [(lib.EPIR_NONE, None, v64, False), (lib.EPIR_RESIDUAL, resid, resid.double() + v64.to(BF).double(), False)]


@pytest.mark.parametrize("kind, N, K, geglu", GEMM_CASES)
def test_gemm_rows_w8a8_every_epilogue(kind, N, K, geglu):
    """x2v_gemm_rows_w8a8 for M = 1, 37, 203, 300 into a NaN-poisoned oversized buffer.  int8 NONE / RESIDUAL: bit equality with the fp32 restatement of
    the contract (the integer sum has no order and the contract no transcendental: nothing may differ).  int8 GEGLU and every e4m3 case: the 1-ulp check
    of tests/test_gpu_t5.py against the float64 product of the decoded codes (2^-7 relative + 2^-24, at most 2e-3 of the elements outside).  The same inputs
    through an fp32-accumulating matmul on the CPU (the exact sum for int8; the GELU as x / (1 + exp(-2u)) in fp32) leave at worst 5.2e-6 (int8 GEGLU), 8.1e-7
    (e4m3 NONE), 1.3e-5 (e4m3 RESIDUAL) and 1.1e-5 (e4m3 GEGLU) of the elements outside over these cases (measured before the kernel was run), far inside
    the 2e-3 share.
    On MI355X (profiles/t5_quant_parity.txt) the worst e4m3 share is 1.4e-5.  The e4m3 product is taken on codes decoded to fp16 in registers (exact)
    with the fp16 matrix instruction; the e4m3 matrix instructions themselves truncate addends when they align them and left 1.2e-3 .. 4.7e-3 outside."""
    from lightx2v_amd import lib
    from tests.util import record

    g = torch.Generator().manual_seed(N * 7 + K + geglu)
    rows = 2 * N if geglu else N
    w, sw = _codes(kind, rows, K, g, "cuda"), _scales(kind, rows, K, g, "cuda")
    worst = 0.0
    for M in MS:
        x, sx = _codes(kind, M, K, g, "cuda"), _scales(kind, M, K, g, "cuda")
        resid = (torch.randn(M, N, generator=g) * 2).to(BF).cuda()
        for epi, r, ref, exact in _expected(kind, x.double() @ w.double().t(), sx, sw, resid, geglu):
            store = torch.full((M * N + 4096,), float("nan"), dtype=BF, device="cuda")
            out = store[: M * N].view(M, N)
            lib.gemm_rows_w8a8(x, sx, w, sw, epilogue=epi, resid=r, out=out)
            torch.cuda.synchronize()
            assert torch.isnan(store[M * N :]).all(), "gemm_rows_w8a8 wrote past its output"
            what = f"gemm_rows_w8a8 {kind} M={M} N={N} K={K} epilogue {epi}"
            if exact:
                assert torch.equal(out, ref), f"{what}: {(out != ref).sum().item()} elements differ from the contract's bits"
            else:
                worst = max(worst, _ulp_check(out, ref, what))
    record(f"gemm_rows_w8a8 {kind} N={N} K={K} geglu={geglu}", worst_share_outside_1ulp=worst)


def test_gemm_cases_launch_every_tile():
    from lightx2v_amd import lib

    tiles = {lib.gemm_rows_w8a8_tile_choice(M, N, lib.EPIR_GEGLU if geglu else lib.EPIR_NONE) for _, N, _, geglu in GEMM_CASES for M in MS}
    assert tiles == {(128, 64), (64, 64), (64, 32), (64, 16)}


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_rows_w8a8_residual_in_place_and_packed_rows_bit_equal(kind):
    """y may alias resid; the rows of an M = 203 call equal the M = 77 and M = 126 calls on the same rows, bit for bit, for every epilogue, across
    different tile choices."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(5)
    x, sx, w, sw = _codes(kind, 203, 4096, g, "cuda"), _scales(kind, 203, 4096, g, "cuda"), _codes(kind, 4096, 4096, g, "cuda"), _scales(kind, 4096, 4096, g, "cuda")
    r = torch.randn(203, 4096, generator=g).to(BF).cuda()
    assert lib.gemm_rows_w8a8_tile_choice(203, 4096) != lib.gemm_rows_w8a8_tile_choice(77, 4096)
    assert lib.gemm_rows_w8a8_tile_choice(203, 2048, lib.EPIR_GEGLU) != lib.gemm_rows_w8a8_tile_choice(77, 2048, lib.EPIR_GEGLU)
    full = {epi: lib.gemm_rows_w8a8(x, sx, w, sw, epilogue=epi, resid=r if epi == lib.EPIR_RESIDUAL else None) for epi in (lib.EPIR_NONE, lib.EPIR_RESIDUAL, lib.EPIR_GEGLU)}
    for lo, hi in ((0, 77), (77, 203)):
        part = r[lo:hi].clone()
        lib.gemm_rows_w8a8(x[lo:hi], sx[lo:hi], w, sw, epilogue=lib.EPIR_RESIDUAL, resid=part, out=part)  # in place
        assert torch.equal(part, full[lib.EPIR_RESIDUAL][lo:hi])
        for epi in (lib.EPIR_NONE, lib.EPIR_GEGLU):
            assert torch.equal(lib.gemm_rows_w8a8(x[lo:hi], sx[lo:hi], w, sw, epilogue=epi), full[epi][lo:hi])


@pytest.mark.parametrize("D", [256, 4096, 10240])
@pytest.mark.parametrize("kind", KINDS)
def test_rmsnorm_quant_equals_the_two_kernels(kind, D):
    """Codes and scales of x2v_rmsnorm_quant_* equal x2v_rmsnorm_bf16 (X2V_ROUND_FP32) followed by x2v_quant_*_rowwise, for M = 1, 37, 300, with an all-zero
    row and a row with a single huge element."""
    from lightx2v_amd import lib

    fused, quant = (lib.rmsnorm_quant_int8, lib.quant_int8_rowwise) if kind == "int8" else (lib.rmsnorm_quant_fp8, lib.quant_fp8_rowwise)
    g = torch.Generator().manual_seed(D)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF).cuda()
    for M in (1, 37, 300):
        x = torch.randn(M, D, generator=g)
        x[M // 2] = 0
        x[-1, D // 3] = 3e4
        x = x.to(BF).cuda()
        (q, s), (q2, s2) = fused(x, w), quant(lib.rmsnorm(x, w))
        assert q.dtype == KINDS[kind][0] and torch.equal(s, s2) and torch.equal(q.view(torch.uint8), q2.view(torch.uint8)), f"{kind} D={D} M={M}"


@pytest.mark.parametrize("scheme", KINDS)
def test_quantised_encoder_vs_restatement(gold, scheme):
    """t5-tiny (256 / 4 heads / 640 / 2 blocks) from quantize_state_dict on the fixture's four prompts in one packed pass: the project's triangle with the
    fp64 quantised restatement as the truth and its reference-order bf16 evaluation as the yardstick.  Two valid evaluations differ where an activation
    code flips by one; with the restatement in fp32 as the stand-in for a correct kernel path the CPU gives, per prompt, err(fp32) / err(bf16) <= 0.47
    (int8) and <= 0.69 (fp8) against the 1.5, and fp32-vs-bf16 / err(bf16) <= 1.01 against the 2: the project's factors stand for both schemes."""
    from lightx2v_amd import synth, t5
    from tests import t5_quant_restatement as Q

    sd = synth.synth_t5_weights(synth.T5_DIMS["t5-tiny"], seed=int(gold["seed"][0]))
    qsd = t5.quantize_state_dict(sd, scheme)
    m = t5.T5EncoderModel(512, torch.bfloat16, "cuda", None, t5_quantized=True, t5_quantized_ckpt=qsd, quant_scheme=scheme)
    assert 2 * m.weight_bytes() == t5.T5EncoderModel(512, torch.bfloat16, "cpu", sd).weight_bytes()
    outs = m.infer_ids(gold["ids"], gold["mask"])
    truth = Q.infer_ids(qsd, gold["ids"], gold["mask"], scheme, dtype=torch.float64)
    ref16 = Q.infer_ids(qsd, gold["ids"], gold["mask"], scheme, dtype=torch.bfloat16)
    for b, (o, n) in enumerate(zip(outs, (37, 64, 1, 130))):
        assert tuple(o.shape) == (n, 256) and o.dtype == torch.bfloat16 and o.is_cuda
        _triangle(o, ref16[b], truth[b], f"t5 tiny {scheme} encoder prompt {b} ({n} tokens)")
    assert torch.equal(m.infer_ids(gold["ids"][1:2], gold["mask"][1:2])[0], outs[1])  # alone: the same bits as inside the packed pass
