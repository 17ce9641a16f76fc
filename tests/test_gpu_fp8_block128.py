"""gemm_b128.hip on the GPU: the quantiser bit for bit against the reference's torch expression (mm_weight.py:251-256, on the CPU); the GEMM against the float64 contract of
include/x2v.h, family I (integer codes, power-of-two scales) bit for bit and family R on every element inside gemm_ref's bound at K + K/128 + 3 units; the operator class.  The GEMM's edges: ten and nine row tiles (a partial
last group of the kernel's 8-row-tile remap), xq / wq / resid / sx as windows of wider NaN-filled buffers, and no bias under every epilogue."""
import os

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
KEY = "W-fp8-block128-sym-A-fp8-channel-group128-sym-dynamic-Hip"
POISON = -1984.0  # exact in bf16
BF16, F32, F64, E4M3 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
CASES = {n: G.Case(n, prefix="fp8_block128") for n in ("family I", "family R")}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    if path := os.environ.get("X2V_B128_PARITY_TABLE"):  # where to write the table of measured ratios (profiles/gemm_block128_parity.txt is one run's)
        with open(path, "w") as f:
            f.write("\n".join([c.header() for c in CASES.values()] + [r for c in CASES.values() for r in c.table()]) + "\n")


@pytest.mark.parametrize("M,K,ldx", [(1, 384, 384), (63, 128, 128), (130, 384, 392), (130, 128, 128)])
def test_quantiser_equals_the_reference_expression_bit_for_bit(lib, M, K, ldx):
    g, ng = torch.Generator().manual_seed(M * 1000 + K), K // 128
    x = (torch.randn(M, ng, 128, generator=g) * torch.ldexp(torch.ones(M, ng, 1), torch.randint(-12, 9, (M, ng, 1), generator=g))).to(BF16)
    flat = x.view(-1, 128)  # the three pinned groups: first, middle and last (row, group) slot
    flat[0] = 0  # under the 1e-4 clamp
    flat[flat.shape[0] // 2, :4] = torch.tensor([3.3895e38, -3.3895e38, 1.0, -2.0]).to(BF16)  # +-bf16 max: 1 / amax is an fp32 denormal
    flat[-1] = (torch.randn(128, generator=g) * 0.1).to(BF16).clamp(-1, 1)
    flat[-1, :4] = torch.tensor([7.0, 17 / 64, 19 / 64, -17 / 64]).to(BF16)  # amax 7 = 448 / 64: 17, 19 and -17 are exact e4m3 ties after scaling
    xv = x.view(M, -1, 128)  # mm_weight.py:251-256
    amax = xv.abs().float().amax(dim=2).view(M, -1).clamp(1e-4)
    want_q, want_s = (xv * (448.0 / amax.unsqueeze(2))).to(E4M3).view(M, K), (amax / 448.0).view(M, -1)
    assert want_q.view(-1, 128)[-1, :4].float().tolist() == [448.0, 16.0, 20.0, -16.0]
    xb = torch.full((M, ldx), 3.0, dtype=BF16)
    xb[:, :K] = x.view(M, K)
    xq, sx = lib.quant_fp8_group128(xb.cuda()[:, :K])
    assert sx.shape == (M, ng) and (M == 1 or sx.stride(0) == 1)
    nq, ns = int((xq.cpu().view(torch.uint8) != want_q.view(torch.uint8)).sum()), int((sx.cpu().view(torch.int32) != want_s.view(torch.int32)).sum())
    assert nq == 0 and ns == 0, f"{nq} of {M * K} codes and {ns} of {M * ng} scales differ"


class Inputs:
    """What G.Expect reads of a case.  K counts the bound's rounding units, K + K / 128 (Expect adds 3): 128 adds, the scale roundings and the group sum per group, the bias."""

    def __init__(self, family, M, N, K, xq, sx, wq, sw, seed):
        g = torch.Generator().manual_seed(seed)
        self.family, self.M, self.N, self.dtype, self.K, self.name = family, M, N, "e4m3", K + K // 128, f"{family} b128 {M}x{N}x{K}"
        self.xq, self.sx, self.wq, self.sw = xq, sx, wq, sw  # sx [M, K/128], sw [ceil(N/128), K/128]
        if family == "I":
            self.bias = torch.randint(-64, 65, (N,), generator=g).to(BF16)
            self.gate = (0.5 * torch.randint(-3, 4, (N,), generator=g)).to(BF16)
            self.resid = torch.randint(-200, 201, (M, N), generator=g).to(BF16)
        else:
            self.bias, self.gate, self.resid = torch.randn(N, generator=g).to(BF16), torch.randn(N, generator=g).to(BF16), torch.randn(M, N, generator=g).to(BF16)
        x64, w64 = xq.to(F32).to(F64).view(M, -1, 128), wq.to(F32).to(F64).view(N, -1, 128)
        s = (sx.to(F64).t()[:, :, None] * sw.to(F64).t()[:, None, :]).repeat_interleave(128, dim=2)[:, :, :N]  # [G, M, N]
        acc, absacc, b64 = (torch.einsum("mgk,ngk->gmn", x64, w64) * s).sum(0), (torch.einsum("mgk,ngk->gmn", x64.abs(), w64.abs()) * s).sum(0), self.bias.to(F64)[None, :]
        self.t = lambda use_bias=True: acc + b64 if use_bias else acc
        self.S = lambda use_bias=True: absacc + b64.abs() if use_bias else absacc
        self.resid_rows = lambda period=0: self.resid.to(F64)


def _window(t, before, after):
    """t on the device as the column window [before : before + cols] of a buffer `before + after` columns wider, every byte of the padding a NaN of t's type
    (0x7f is e4m3's, 0x7f7f one of bf16's, 0x7f7f7f7f one of fp32's)."""
    es = t.element_size()
    raw = torch.full((t.shape[0], (before + t.shape[1] + after) * es), 0x7F, dtype=torch.uint8, device="cuda")
    raw[:, before * es : (before + t.shape[1]) * es] = t.contiguous().view(torch.uint8).cuda()
    return raw.view(t.dtype)[:, before : before + t.shape[1]]


def run(lib, inp, epi, use_gate, use_bias=True, padded=False):
    """The kernel's y as a window of a poisoned buffer, whose surroundings must come back untouched.  padded: xq, wq and resid are column windows of wider
    buffers (ldx = K + 32, ldw = K + 48 bytes, ldr = N + 16 elements, each window 16 bytes in) and sx a window of a [K/128, M + 8] table (lds = M + 8)."""
    M, N = inp.M, inp.N
    buf = torch.full((M + 2, N + 16), POISON, dtype=BF16, device="cuda")
    out = buf[1 : M + 1, 8 : 8 + N]
    if padded:
        xq, wq, resid, sx = _window(inp.xq, 16, 16), _window(inp.wq, 16, 32), _window(inp.resid, 8, 8), _window(inp.sx.t().contiguous(), 0, 8).t()
        assert xq.stride(0) == xq.shape[1] + 32 and wq.stride(0) == wq.shape[1] + 48 and resid.stride(0) == N + 16 and sx.stride() == (1, M + 8)
    else:
        xq, wq, resid = inp.xq.cuda(), inp.wq.cuda(), inp.resid.cuda()
        sx = inp.sx.t().contiguous().cuda().t()  # k-group-major, as the quantiser returns it
    lib.gemm_fp8_block128(xq, sx, wq, inp.sw.cuda(), inp.bias.cuda() if use_bias else None, epilogue=epi, resid=resid if epi == G.EPI_RESIDUAL else None,
                          gate=inp.gate.cuda() if use_gate else None, out=out)
    got = out.clone()
    out.fill_(POISON)
    assert bool((buf == POISON).all()), f"{inp.name}: a store outside y[{M}, {N}]"
    return got.cpu()


@pytest.mark.parametrize("M,N,K", [(1, 8, 128), (127, 136, 256), (129, 256, 384), (257, 392, 1152), (1, 392, 384), (127, 256, 1152), (129, 8, 256), (257, 136, 128),
                                   (129, 392, 128), (257, 256, 256), (127, 392, 384), (1, 136, 1152), (1153, 264, 128), (1025, 8, 256)])
def test_gemm_equals_the_float64_chain_bit_for_bit(lib, M, N, K):
    """The last two shapes have ten and nine row tiles: the second group of the kernel's 8-row-tile remap holds 2 and 1.  (1025, 8, 256) and (257, 392, 1152)
    run once more through padded strides (run's padded form), (127, 136, 256) once more without a bias."""
    g, ng, nb = torch.Generator().manual_seed(M + N + K), K // 128, -(-N // 128)
    xq, wq = torch.randint(-4, 5, (M, K), generator=g).to(F32).to(E4M3), torch.randint(-2, 3, (N, K), generator=g).to(F32).to(E4M3)
    m, gi, b = torch.arange(M)[:, None], torch.arange(ng)[None, :], torch.arange(nb)[:, None]
    sx, sw = torch.ldexp(torch.ones(M, ng), (m + gi) % 4 - 2), torch.ldexp(torch.ones(nb, ng), (3 * b + gi) % 4 - 2)  # 2^-2 .. 2^1
    inp = Inputs("I", M, N, K, xq, sx, wq, sw, seed=K)
    assert float(inp.S().max()) * 2.0 ** 4 < 2.0 ** 24  # multiples of 2^-4 below 2^20: every partial sum is an fp32 number
    for epi, use_gate in ((G.EPI_NONE, False), (G.EPI_RESIDUAL, True)):
        CASES["family I"].check_exact(run(lib, inp, epi, use_gate), G.Expect(inp, epi, use_gate=use_gate), "gemm_b128")
        if (M, N, K) in ((1025, 8, 256), (257, 392, 1152)):
            CASES["family I"].check_exact(run(lib, inp, epi, use_gate, padded=True), G.Expect(inp, epi, use_gate=use_gate), "gemm_b128 padded strides")
        if (M, N, K) == (127, 136, 256):
            CASES["family I"].check_exact(run(lib, inp, epi, use_gate, use_bias=False), G.Expect(inp, epi, use_bias=False, use_gate=use_gate), "gemm_b128")


@pytest.mark.parametrize("M,N,K", [(129, 392, 384), (257, 256, 1152)])
def test_gemm_stays_inside_the_derived_bound_on_every_element(lib, M, N, K):
    """(129, 392, 384) runs every epilogue once more without a bias."""
    from lightx2v_amd import ops

    g = torch.Generator().manual_seed(K)
    xq, sx = lib.quant_fp8_group128(torch.randn(M, K, generator=g).to(BF16).cuda())
    wq, sw = ops.MMWeightFp8Block128Hip.per_block_cast_to_fp8((torch.randn(N, K, generator=g) / K ** 0.5).to(BF16))
    inp = Inputs("R", M, N, K, xq.cpu(), sx.cpu(), wq, sw, seed=M)
    for epi, use_gate in ((G.EPI_NONE, False), (G.EPI_GELU, False), (G.EPI_SILU, False), (G.EPI_RESIDUAL, True)):
        exp = G.Expect(inp, epi, use_gate=use_gate)
        print(f"{inp.name} {exp.what}: d/tol {CASES['family R'].check_bound(run(lib, inp, epi, use_gate), exp, 'gemm_b128'):.3f}")
        if (M, N, K) == (129, 392, 384):
            exp = G.Expect(inp, epi, use_bias=False, use_gate=use_gate)
            print(f"{inp.name} {exp.what}: d/tol {CASES['family R'].check_bound(run(lib, inp, epi, use_gate, use_bias=False), exp, 'gemm_b128'):.3f}")


def test_operator_class_is_the_two_calls_and_slices_whole_scale_blocks(lib):
    from lightx2v_amd import registry

    g, M, N, K, sl = torch.Generator().manual_seed(5), 70, 512, 256, slice(128, 384)
    op = registry.MM_WEIGHT_REGISTER[KEY]("w.weight", "w.bias")
    op.set_config({"weight_auto_quant": True})
    op.load({"w.weight": (torch.randn(N, K, generator=g) / 16).to(BF16).cuda(), "w.bias": torch.randn(N, generator=g).to(BF16).cuda()})
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    xq, sx = lib.quant_fp8_group128(x)
    y = op.apply(x)
    assert torch.equal(y, lib.gemm_fp8_block128(xq, sx, op.weight, op.weight_scale, op.bias)) and torch.equal(y, op.apply(x, quantized=(xq, sx)))
    ys = op.apply(x, row_slice=sl)
    assert torch.equal(ys, lib.gemm_fp8_block128(xq, sx, op.weight[sl].contiguous(), op.weight_scale[1:3].contiguous(), op.bias[sl].contiguous())) and torch.equal(ys, y[:, sl])
    with pytest.raises(lib.X2VError):
        op.apply(x, row_slice=slice(64, 384))


def test_wan_tiny_forward_keeps_the_per_channel_fp8_accuracy(lib):
    from lightx2v_amd import ops, scheduler, synth, wan
    from tests.util import rel_l2

    dims, wl = synth.WAN_DIMS["wan-tiny"], synth.WORKLOADS["wan-tiny"]
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=0).items()}
    lat, ctx, ctx_null = synth.synth_inputs(dims, wl["target_shape"])
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    outs = []
    for mm in ({"mm_type": "Hip-bf16"}, {"mm_type": "W-fp8-channel-sym-A-fp8-channel-sym-dynamic-Hip", "weight_auto_quant": True}, {"mm_type": KEY, "weight_auto_quant": True}):
        cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=4, mm_config=mm)
        model = wan.WanModel(cfg, wd)
        sch = scheduler.WanScheduler(cfg, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        sch.step_pre(0)
        model.infer(inputs)
        outs.append(sch.noise_pred.float().cpu())
    assert type(model.transformer_weights.blocks[0].compute_phases[3].ffn_0) is ops.MMWeightFp8Block128Hip
    per_channel, block128 = rel_l2(outs[1], outs[0]), rel_l2(outs[2], outs[0])
    print(f"wan-tiny forward vs bf16: per-channel fp8 rel_l2 {per_channel:.3e}, block-128 fp8 {block128:.3e}")
    assert torch.isfinite(outs[2]).all() and 0 < block128 <= 1.5 * per_channel
