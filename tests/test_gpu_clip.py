"""The CLIP image tower on the HIP kernels (csrc/clip.hip, lightx2v_amd/clip.py) against
  * fp64 torch math for the fp16 GEMM (every epilogue), the head-dim-80 attention, the LayerNorm and the token assembly,
  * torch's own bicubic + normalise for the image front end,
  * the fixture generated from the unmodified reference (tests/golden/clip_visual_tiny.*.safetensors) and, at the released dims, the plain-PyTorch
    restatement (tests/clip_restatement.py, pinned to that fixture bit for bit) run in fp32 and fp16 on the same GPU.
Whole-tower bar: the project's fp32 triangle, err(HIP vs fp32 truth) <= 1.5 x err(reference fp16 vs fp32 truth) in relative L2 per image, plus
rel L2(HIP vs reference fp16) <= 1e-2.  Measured numbers are appended to the parity summary (tests/util.py::record)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ULP16 = 2.0**-10  # the widest relative spacing of fp16 (an ulp at the bottom of a binade)
FLIP_SHARE = 2e-3  # the project's share of rounding-boundary flips (tests/util.py::assert_bf16_close callers)

# max |torch CPU bicubic + normalise - torch GPU bicubic + normalise| over the four sizes of test_front_end_vs_torch_bicubic, fp32, measured on an
# MI355X with this file's inputs (see the test's docstring); the kernel's bar is twice this.
TORCH_CPU_GPU_BICUBIC_DIFF = 9.537e-7


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _ulp_check(got, ref64, what, atol, ulps=1.0):
    """|got - fp16(ref64)| <= ulps * 2^-10 |ref| + atol except for FLIP_SHARE of the elements; returns the share outside."""
    ref = ref64.to(torch.float16).double()
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = ((got - ref).abs() > ulps * ULP16 * ref.abs() + atol).double().mean().item()
    assert bad <= FLIP_SHARE, f"{what}: {bad:.2e} of elements outside {ulps} ulp + {atol}; max |d| {(got - ref).abs().max().item():.3e}"
    return bad


GEMM_SHAPES = [(3840, 1280), (1280, 1280), (5120, 1280), (1280, 5120), (1280, 608)]  # (N, K); 608 = 3 * 14 * 14 = 588 zero-padded to a multiple of 32


@pytest.mark.parametrize("N, K", GEMM_SHAPES + [(160, 160), (484, 96)])
def test_gemm_f16_every_epilogue(N, K):
    """x2v_gemm_f16 vs fp64 math rounded once to fp16: <= 1 fp16 ulp + 2^-23 (two fp16 subnormal steps) outside of at most 2e-3 of the elements, for
    M = 257, 514, 1028 and the tail 300, every epilogue (no bias, bias, bias + exact GELU, bias + residual), into a NaN-poisoned oversized buffer.  The
    residual epilogue rounds twice, as the reference's fp16 add of two fp16 tensors does, and its fp64 reference does the same: fp16(resid +
    fp16(acc64 + bias)), held to the same 1 ulp + 2^-23, which a single rounding of the sum does not meet.  An fp32 accumulation that lands on the other
    side of the inner rounding than fp64 moves y by one ulp of the Linear output, which can be several ulps of a cancelling sum: with x ~ N(0, 1),
    W ~ N(0, 1 / K), resid ~ N(0, 4) an fp32 matmul on the CPU leaves at most 1.1e-4 of the elements outside (measured at every shape of this test before the
    kernel was run), inside the 2e-3 share.  y ~ N(0, 1): the GELU's 1 + erf cancellation (torch's own fp32 formula) stays below an ulp down to
    x ~ -4, a 3e-5 tail.  (484, 96): an N tail that is not a multiple of 16."""
    from lightx2v_amd import lib
    from tests.util import record

    g = torch.Generator().manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) / K**0.5).half().cuda()
    bias = (torch.randn(N, generator=g) * 0.1).half().cuda()
    if K == 608:
        w[:, 588:] = 0
    worst = 0.0
    for M in (257, 514, 1028, 300):
        x = torch.randn(M, K, generator=g).half().cuda()
        resid = (torch.randn(M, N, generator=g) * 2).half().cuda()
        acc = x.double() @ w.double().t()
        for epi, b, what in ((lib.EPI16_NONE, None, "no bias"), (lib.EPI16_NONE, bias, "bias"), (lib.EPI16_GELU_ERF, bias, "gelu"), (lib.EPI16_RESIDUAL, bias, "residual")):
            y64 = acc if b is None else acc + b.double()
            if epi == lib.EPI16_GELU_ERF:
                y64 = F.gelu(y64)
            elif epi == lib.EPI16_RESIDUAL:
                y64 = resid.double() + y64.to(torch.float16).double()
            store = torch.full((M * N + 4096,), float("nan"), dtype=torch.float16, device="cuda")
            out = store[: M * N].view(M, N)
            lib.gemm_f16(x, w, b, epilogue=epi, resid=resid if epi == lib.EPI16_RESIDUAL else None, out=out)
            torch.cuda.synchronize()
            assert torch.isnan(store[M * N :]).all(), "gemm_f16 wrote past its output"
            worst = max(worst, _ulp_check(out, y64, f"gemm_f16 M={M} N={N} K={K} {what}", 2.0**-23))
    record(f"gemm_f16 N={N} K={K}", worst_share_outside_1ulp=worst)


def test_gemm_f16_residual_in_place_and_batch_rows_bit_equal():
    """y may alias resid (the tower's x = x + proj(...)); rows of a batched call equal the same rows computed alone, bit for bit, across tile choices."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(5)
    x = torch.randn(771, 1280, generator=g).half().cuda()
    w = (torch.randn(1280, 1280, generator=g) / 1280**0.5).half().cuda()
    b = (torch.randn(1280, generator=g) * 0.1).half().cuda()
    r = torch.randn(771, 1280, generator=g).half().cuda()
    full = lib.gemm_f16(x, w, b, epilogue=lib.EPI16_RESIDUAL, resid=r)
    assert lib.gemm_f16_tile_choice(771, 1280) != lib.gemm_f16_tile_choice(257, 1280)
    for i in range(3):
        part = r[257 * i : 257 * (i + 1)].clone()
        lib.gemm_f16(x[257 * i : 257 * (i + 1)], w, b, epilogue=lib.EPI16_RESIDUAL, resid=part, out=part)
        assert torch.equal(part, full[257 * i : 257 * (i + 1)])


@pytest.mark.parametrize("batch, heads", [(1, 2), (1, 16), (4, 16)])
def test_attention_f16_d80(batch, heads):
    """x2v_attn_f16_d80 vs fp64 softmax attention on a strided QKV buffer (row stride 3 * H * 80 + 16), 257 keys; output into a NaN-poisoned oversized
    buffer.  Bar from the formats: the probabilities enter the PV product rounded to fp16 (relative 2^-11 each, so at most 2^-11 max|v| on a convex
    combination) and the output is rounded once (2^-11 |o|); fp32 softmax statistics add ~1e-6.  |d| <= 2^-10 |ref| + 1.05 * 2^-11 max|v| holds
    everywhere (no share)."""
    from lightx2v_amd import lib
    from tests.util import record

    S, D = 257, heads * 80
    g = torch.Generator().manual_seed(batch * 100 + heads)
    buf = torch.randn(batch * S, 3 * D + 16, generator=g).half().cuda()
    qkv = buf[:, : 3 * D]
    store = torch.full((batch * S * D + 4096,), float("nan"), dtype=torch.float16, device="cuda")
    out = store[: batch * S * D].view(batch * S, D)
    lib.attention_f16_d80(qkv, batch, heads, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(store[batch * S * D :]).all(), "the attention kernel wrote past its output"
    q, k, v = qkv.double().view(batch, S, 3, heads, 80).unbind(2)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * 80**-0.5, dim=-1)
    ref = torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(batch * S, D)
    assert torch.isfinite(out).all()
    d = (out.double() - ref).abs()
    tol = ULP16 * ref.abs() + 1.05 * 2.0**-11 * v.abs().max()
    assert (d <= tol).all(), f"max |d| {d.max().item():.3e}, worst excess {(d - tol).max().item():.3e}"
    record(f"attn_f16_d80 batch={batch} heads={heads}", max_abs=d.max().item(), rel_l2=_rel(out, ref))


def test_attention_f16_d80_short_sequences():
    """Fewer keys than the LDS image holds (S = 1, 17, 64, 272): the masked tail and the query-block tail."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(8)
    for S in (1, 17, 64, 272):
        qkv = torch.randn(2 * S, 3 * 160, generator=g).half().cuda()
        out = lib.attention_f16_d80(qkv, 2, 2)
        q, k, v = qkv.double().view(2, S, 3, 2, 80).unbind(2)
        ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * 80**-0.5, dim=-1), v).reshape(2 * S, 160)
        d = (out.double() - ref).abs()
        assert (d <= ULP16 * ref.abs() + 1.05 * 2.0**-11 * v.abs().max()).all(), (S, d.max().item())


def test_layernorm_f16_and_token_assembly():
    """x2v_layernorm_f16 vs fp64 LayerNorm rounded once (1 ulp + 1e-5: the fp32 statistics' ~1e-6 relative error on |x - mean| / sigma <= 6 weighs more
    than an ulp only next to zero), D = 1280 and 160; x2v_clip_embed_f16 vs fp64 LayerNorm of fp16(cls | patch + pos)."""
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(6)
    for M, D in ((257, 1280), (300, 160), (5, 2048)):
        x = (torch.randn(M, D, generator=g) * 2 + 3).half().cuda()
        w, b = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
        store = torch.full((M * D + 1024,), float("nan"), dtype=torch.float16, device="cuda")
        out = store[: M * D].view(M, D)
        lib.layernorm_f16(x, w, b, eps=1e-5, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(store[M * D :]).all()
        _ulp_check(out, F.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5), f"layernorm_f16 {M}x{D}", 1e-5)
    for B, D in ((1, 1280), (3, 160)):
        patches = torch.randn(B * 256, D, generator=g).half().cuda()
        cls, pos = torch.randn(D, generator=g).half().cuda(), (0.5 * torch.randn(257, D, generator=g)).half().cuda()
        w, b = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
        out = lib.clip_embed(patches, cls, pos, w, b, B)
        tok = (torch.cat([cls.expand(B, 1, D), patches.view(B, 256, D)], dim=1) + pos).view(B * 257, D)  # the fp16 add
        _ulp_check(out, F.layer_norm(tok.double(), (D,), w.double(), b.double(), 1e-5), f"clip_embed B={B} D={D}", 1e-5)


def test_wrapper_refuses_outputs_of_the_wrong_shape():
    """lib.layernorm_f16 / clip_embed / clip_preprocess check a caller's `out` before the kernel is launched: a smaller buffer, a patch count that
    the batch does not divide, and a column-sliced operand (the front end zero-fills every row up to its stride) are errors, not writes."""
    from lightx2v_amd import lib, synth

    x = torch.zeros(8, 160, dtype=torch.float16, device="cuda")
    w = torch.ones(160, device="cuda")
    with pytest.raises(lib.X2VError, match="out must be"):
        lib.layernorm_f16(x, w, w, out=torch.empty(4, 160, dtype=torch.float16, device="cuda"))
    cls, pos = torch.zeros(160, dtype=torch.float16, device="cuda"), torch.zeros(5, 160, dtype=torch.float16, device="cuda")
    with pytest.raises(lib.X2VError, match="out must be"):
        lib.clip_embed(x, cls, pos, w, w, 2, out=torch.empty(8, 160, dtype=torch.float16, device="cuda"))
    with pytest.raises(lib.X2VError, match="is not"):
        lib.clip_embed(x, cls, pos, w, w, 3)
    img = torch.zeros(3, 32, 32, device="cuda")
    with pytest.raises(lib.X2VError, match="column slice"):
        lib.clip_preprocess(img, torch.empty(256, 608, dtype=torch.float16, device="cuda")[:, :592], 224, 14, synth.CLIP_MEAN, synth.CLIP_STD)


def _patch_major(pre):
    """[3, 224, 224] → [256, 588], column c * 196 + py * 14 + px (the flattened Conv2d weight's order)."""
    return pre.view(3, 16, 14, 16, 14).permute(1, 3, 0, 2, 4).reshape(256, 588)


def test_front_end_vs_torch_bicubic():
    """x2v_clip_preprocess_f16 vs F.interpolate(mode="bicubic", align_corners=False) + (x * 0.5 + 0.5 - mean) / std in fp32 on the CPU, for 720 x 1280,
    480 x 832, an odd 333 x 517 and 224 x 224.  The 224 x 224 case (weights exactly 0 / 1) must equal the fp16 rounding of the reference exactly.  For
    the others two fp32 evaluations of the same taps differ in summation order: the bar is 2 x the difference between torch's own CPU and GPU results on
    these inputs, TORCH_CPU_GPU_BICUBIC_DIFF (measured on an MI355X: 9.537e-7 = 2^-20 at each of the three sizes, 0 at 224 x 224; printed again by this test), plus the
    fp16 rounding of the output (2^-11 |ref|).  Pad columns 588..607 are zero; the operand is written into a NaN-poisoned buffer."""
    from lightx2v_amd import lib, synth
    from tests import clip_restatement as R
    from tests.util import record

    g = torch.Generator().manual_seed(12)
    for H, W in ((720, 1280), (480, 832), (333, 517), (224, 224)):
        img = torch.rand(3, H, W, generator=g) * 2 - 1
        ref = R.preprocess([img[:, None]])[0]
        ref_gpu = R.preprocess([img[:, None].cuda()])[0].cpu()
        d_torch = (ref - ref_gpu).abs().max().item()
        store = torch.full((256 * 608 + 1024,), float("nan"), dtype=torch.float16, device="cuda")
        out = store[: 256 * 608].view(256, 608)
        padded = torch.zeros(3, H, W + 3, device="cuda")[..., :W]  # a strided view: read in place
        padded.copy_(img)
        lib.clip_preprocess(padded, out, 224, 14, synth.CLIP_MEAN, synth.CLIP_STD)
        torch.cuda.synchronize()
        assert torch.isnan(store[256 * 608 :]).all() and not out[:, 588:].any()
        got, want = out[:, :588].cpu(), _patch_major(ref)
        d = (got.float() - want).abs()
        print(f"front end {H}x{W}: torch CPU vs GPU max |d| {d_torch:.3e}; HIP vs CPU max |d| {d.max().item():.3e}")
        record(f"clip_preprocess {H}x{W}", torch_cpu_vs_gpu_max_abs=d_torch, hip_vs_cpu_max_abs=d.max().item())
        if (H, W) == (224, 224):
            assert torch.equal(got, want.half()), f"identity resize: max |d| {d.max().item():.3e}"
        else:
            assert (d <= 2 * TORCH_CPU_GPU_BICUBIC_DIFF + 2.0**-11 * want.abs() + 2.0**-24).all(), f"{H}x{W}: max |d| {d.max().item():.3e}"


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("clip_visual_tiny")


def _tiny(gold):
    from lightx2v_amd import clip, synth

    sd = synth.synth_clip_weights(synth.CLIP_DIMS["clip-tiny"], seed=int(gold["seed"][0]))
    return clip.CLIPModel(torch.float16, "cuda", sd, False, None, None)


def _triangle(hip, ref16, truth, what):
    from tests.util import record

    e_hip, e_ref, e_pair = _rel(hip, truth), _rel(ref16, truth), _rel(hip, ref16)
    print(f"{what}: HIP vs fp32 truth {e_hip:.3e}; reference fp16 vs truth {e_ref:.3e}; HIP vs reference fp16 {e_pair:.3e}")
    record(what, hip_vs_truth=e_hip, ref_fp16_vs_truth=e_ref, hip_vs_ref_fp16=e_pair)
    assert torch.isfinite(hip.float()).all()
    assert e_hip <= 1.5 * e_ref, f"{what}: err(HIP) {e_hip:.3e} > 1.5 x err(reference fp16) {e_ref:.3e}"
    assert e_pair <= 1e-2, f"{what}: HIP vs reference fp16 {e_pair:.3e}"


@pytest.mark.parametrize("graph", [False, True])
def test_tower_vs_reference_fixture(gold, graph):
    """The tiny tower (160 / 2 heads / 2 of 3 blocks) on both fixture images against the reference's fp16 and fp32 outputs; eager launches and the
    captured-graph replay give the same bits."""
    m = _tiny(gold)
    m.graph = graph
    for name in "ab":
        out = m.visual([gold[f"image_{name}"].cuda()], None)
        assert out.shape == (1, 257, 160) and out.dtype == torch.float16
        _triangle(out, gold[f"out_f16_{name}"], gold[f"out_f32_{name}"], f"clip tiny tower image {name} (graph={graph})")
    if graph:
        e = _tiny(gold)
        assert torch.equal(e.visual([gold["image_a"].cuda()], None), m.visual([gold["image_a"].cuda()], None))


def test_tower_released_dims():
    """1280 / 16 heads / 31 of 32 blocks with seeded weights on seeded 720p images, B = 1 and B = 3, against the restatement run in fp32 (truth) and in
    fp16 (what the reference computes) through plain PyTorch on the same GPU; the B = 3 rows equal the three B = 1 runs bit for bit."""
    from lightx2v_amd import clip, synth
    from tests import clip_restatement as R

    sd = synth.synth_clip_weights(synth.CLIP_DIMS["clip-vit-h-14"], seed=1)
    m = clip.CLIPModel(torch.float16, "cuda", sd, False, None, None)
    assert (m.dim, m.num_heads, len(m.blocks), m.k_pad) == (1280, 16, 31, 608)
    g = torch.Generator().manual_seed(31)
    imgs = [(torch.rand(3, 1, 720, 1280, generator=g) * 2 - 1).cuda() for _ in range(3)]
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    singles = []
    for i, im in enumerate(imgs):
        out = m.visual([im], None)
        assert out.shape == (1, 257, 1280)
        truth = R.visual(sd_dev, [im], dtype=torch.float32, device="cuda")
        ref16 = R.visual(sd_dev, [im], dtype=torch.float16, device="cuda")
        _triangle(out, ref16, truth, f"clip ViT-H/14 tower, 720p image {i}, B=1")
        singles.append(out)
    out3 = m.visual(imgs, None)
    assert out3.shape == (3, 257, 1280)
    for i in range(3):
        assert torch.equal(out3[i], singles[i][0]), f"row block {i} of the B = 3 run differs from its B = 1 run"


def test_run_image_encoder_and_i2v_forward(gold):
    """run_image_encoder's shape and dtype ([257, dim] bf16), and one wan-tiny-i2v conditional forward whose clip_encoder_out comes from the HIP tower.
    wan-tiny-i2v's clip_dim is 64, not a multiple of the tower's head dim 80, so the fixture tower's 160-wide tokens are projected to 64 by a fixed seeded
    matrix (test glue); the HIP forward must be finite and agree with the oracle fed the same tokens at the existing i2v forward tolerance (2e-2)."""
    from lightx2v_amd import clip, scheduler, synth, wan
    from oracle import wan_oracle as O

    m = _tiny(gold)
    img = gold["image_a"][:, 0].cuda()
    tokens = clip.run_image_encoder(m, img)
    assert tokens.shape == (257, 160) and tokens.dtype == torch.bfloat16 and tokens.is_cuda
    assert torch.equal(tokens, m.visual([img[:, None]], None)[0].to(torch.bfloat16))
    dims = synth.WAN_DIMS["wan-tiny-i2v"]
    ts, frames = (16, 3, 8, 8), 9
    proj = torch.randn(160, dims["clip_dim"], generator=torch.Generator().manual_seed(2)) / 160**0.5
    clip_out = (tokens.float().cpu() @ proj).to(torch.bfloat16)
    wd = synth.synth_wan_i2v_weights(dims, seed=0)
    lat, ctx, _ = synth.synth_inputs(dims, ts)
    image = {"clip_encoder_out": clip_out, "vae_encode_out": synth.synth_i2v_inputs(dims, ts)["vae_encode_out"]}
    cfg = wan.default_config(dims, task="i2v", in_dim=36, cross_attn_2_type="hip_flash", target_shape=ts, target_video_length=frames, infer_steps=2)
    model = wan.WanModel(cfg, {k: v.cuda() for k, v in wd.items()})
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": []}, "image_encoder_output": {k: v.cuda() for k, v in image.items()}}
    sch.step_pre(0)
    got = model._forward(inputs, True)
    assert torch.isfinite(got.float()).all()
    with torch.no_grad():
        ref = O.wan_forward(wd, dims, lat.to(torch.bfloat16), sch.timesteps[0].cpu(), ctx, image=image)
    e = _rel(got, ref)
    assert e <= 2e-2, f"i2v forward with HIP CLIP tokens vs oracle: relative L2 {e:.3e}"
